"""`MMGCLIP(config)` — drop-in for mmgclip/networks/mmgclip_model.py:12-166 on the MI355X kernels.

Same constructor, attributes (`config, device, text_encoder, image_projection_layer, text_projection_layer,
logit_scale`, `image_encoder` when configured), methods (`count_parameters`, `encode_images`, `encode_text`,
`forward(batch, **kwargs)`) and output-dict keys.  Differences are additive and config-gated:
  * image encoders that take pixels (`ConvNextTinyEncoder`, `ConvNextBaseEncoder`); `ConvNextTiny` keeps the reference
    behaviour (pre-extracted features pass through, no module built);
  * `networks.learnable_logit_scale` (default false = the reference's behaviour on a GPU, where `.to(device)` turns
    the Parameter into a constant tensor: SURVEY.md §0);
  * `forward(..., materialize_logits=False)` skips the two [n,n] matrices for the fused loss path.
"""
import os

import numpy as np

import torch
import torch.nn as nn

from .. import head
from ..kernels import stack_images
from ..utils.logger import logger
from .bert import EosPool
from .network_controller import getNetworkClass
from .projection_controller import get_projection_head
from .view_pool import normalize_method, offsets_to_device, pool_views, study_offsets

PIXEL_ENCODERS = ("ConvNextTinyEncoder", "ConvNextBaseEncoder", "ViTB16Encoder")


def _get(cfg, path, default=None):
    cur = cfg
    for k in path.split("."):
        try:
            cur = cur[k] if isinstance(cur, dict) else getattr(cur, k)
        except (KeyError, AttributeError):
            return default
    return cur


class MMGCLIP(nn.Module):
    def __init__(self, config=None):
        super().__init__()
        assert config is not None, 'Error in initializing the model. Missing training config object.'
        self.config = config
        if not torch.cuda.is_available():
            logger.warning("WARNING: No CUDA device is found. The MI355X kernels have no CPU fallback.")
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

        enc_name = self.config.networks.image_encoder.name
        if enc_name == "ResNet50Encoder":
            self.image_encoder = getNetworkClass(enc_name)(
                pretrained=True, image_features_dimension=self.config.networks.image_encoder.image_features_dimension).to(self.device)
        elif enc_name in PIXEL_ENCODERS:
            ie = self.config.networks.image_encoder
            # (stack / concat of a study's k views: image_features_dimension is k x the tower's width, checked at the first batch of studies)
            joined = self._view_method() in ("stack", "concat")
            self.image_encoder = getNetworkClass(enc_name)(
                pretrained=_get(ie, "pretrained_path"), image_features_dimension=None if joined else ie.image_features_dimension,
                in_chans=_get(ie, "in_chans", 1), scale16=_get(ie, "scale16", True), micro_batch=_get(ie, "micro_batch", 64),
                freeze=_get(ie, "freeze", False),
                checkpoint=_get(ie, "checkpoint", False), augment=_get(ie, "augment"),
                **({"image_size": _get(ie, "image_size", 224), "patch_dropout": _get(ie, "patch_dropout", 0.0),
                    "patch_prior": _get(ie, "patch_prior", "uniform"), "patch_threshold": _get(ie, "patch_threshold", 0.0),
                    "patch_min_pixels": _get(ie, "patch_min_pixels", 1), "patch_dropout_eval": _get(ie, "patch_dropout_eval", False)}
                   if enc_name == "ViTB16Encoder" else
                   {"fp8": _get(ie, "fp8", False), "stochastic_depth_prob": _get(ie, "stochastic_depth_prob", 0.0)})).to(self.device)
            logger.info(f"Using {self.image_encoder.__class__.__name__}")

        te = self.config.networks.text_encoder
        self.text_encoder = getNetworkClass(te.name)(
            pretrained=self.config.tokenizer.config.tokenizer_name, freeze=_get(te, "freeze", True),
            random_init=_get(te, "random_init", False), dropout=bool(_get(te, "dropout", True))).to(self.device)

        if self.config.projection.config.projection_name != "ZeroProjection":
            head_cls = get_projection_head(self.config.projection.config.projection_name)
            self.image_projection_layer = head_cls(
                embedding_dim=self.config.networks.image_encoder.image_features_dimension,
                projection_dim=self.config.projection.config.output_projection_dimension,
                dropout=self.config.networks.dropout.config.dropout).to(self.device)
            self.text_projection_layer = head_cls(
                embedding_dim=self.text_encoder.model_output_dimension,
                projection_dim=self.config.projection.config.output_projection_dimension,
                dropout=self.config.networks.dropout.config.dropout).to(self.device)
            logger.info(f"Embeddings are projected to {self.config.projection.config.output_projection_dimension} "
                        f"features using {self.config.projection.config.projection_name}.")
        else:
            self.image_projection_layer = None
            self.text_projection_layer = None

        init = torch.ones([]) * np.log(1 / self.config.networks.logit_temperature)
        if _get(self.config, "networks.learnable_logit_scale", False) or self.device.type == "cpu":
            self.logit_scale = nn.Parameter(init.float().to(self.device))
        else:
            self.register_buffer("logit_scale", init.float().to(self.device), persistent=False)
        # the sigmoid pairwise loss alone has a bias: with any other loss there is no parameter and no output key
        if self.config.loss.config.loss_name == "SigmoidCLIPLoss":
            bias = _get(self.config, "loss.config.logit_bias", -10.0)
            self.logit_bias = nn.Parameter(torch.tensor(-10.0 if bias is None else float(bias), dtype=torch.float32).to(self.device))

    def count_parameters(self, model):
        """Logs a table of trainable parameters and returns their total count (mmgclip_model.py:54-74)."""
        rows, total = [], 0
        for name, parameter in model.named_parameters():
            if not parameter.requires_grad:
                continue
            rows.append((name, parameter.numel()))
            total += parameter.numel()
        width = max([len(r[0]) for r in rows] + [7])
        table = "\n".join([f"| {'Modules'.ljust(width)} | Parameters |"] + [f"| {n.ljust(width)} | {c:>10} |" for n, c in rows])
        logger.info(f"\n{table}")
        logger.info(f"Total Trainable Params: {total}")
        return total

    def _view_method(self):
        """dataset.config.concatenate_features_method (avgpool when the dataset has no such key), in view_pool's spelling."""
        return normalize_method(_get(self.config, "dataset.config.concatenate_features_method", "avgpool"))

    def _encode_studies(self, pix):
        """A batch of exams: a list of studies, each a non-empty list / tuple of [Cin, H, W] views (sizes may differ inside and across
        studies), or one [S, k, Cin, H, W] tensor.  The views go through the image tower once, flattened in study order, and
        `pool_views` joins each study's rows: [V, F] -> [S, F] (stack / concat: [S, k F]).  What the reference does offline under a
        frozen encoder (StudyFeatureExtractor, mmgclip/networks/image_features.py:187-263), with gradients."""
        name = self.config.networks.image_encoder.name
        if torch.is_tensor(pix):
            counts = [pix.shape[1]] * pix.shape[0]
            views = pix.reshape(pix.shape[0] * pix.shape[1], *pix.shape[2:])
        else:
            if any(not isinstance(s, (list, tuple)) or not s or any(not torch.is_tensor(v) or v.dim() != 3 for v in s) for s in pix):
                raise ValueError("a batch of studies must be a list of non-empty lists of [Cin, H, W] tensors")
            counts = [len(s) for s in pix]
            views = [v for s in pix for v in s]
            if len({tuple(v.shape) for v in views}) == 1:
                views = stack_images(list(views))                   # every view of one size: the towers' 4-D path (any pixel dtype)
            elif name == "ViTB16Encoder":
                raise ValueError(f"ViTB16Encoder needs every view at {self.image_encoder.image_size}x{self.image_encoder.image_size} "
                                 f"(learned positions fix the size), got views of the sizes {sorted({tuple(v.shape[-2:]) for v in views})}")
        n_max = _get(self.config, "dataset.config.n_images_per_study")
        if n_max is not None and max(counts) > int(n_max):
            raise ValueError(f"a study with {max(counts)} views, but dataset.config.n_images_per_study is {n_max}: "
                             "the dataset cuts a study to its first n views, the model does not")
        method = self._view_method()
        offsets = None
        if method in ("stack", "concat"):
            if len(set(counts)) == 1:               # (ragged counts: pool_views says so)
                want, have = counts[0] * self.image_encoder.model_output_dimension, self.config.networks.image_encoder.image_features_dimension
                if want != have:
                    raise ValueError(f"concatenate_features_method={method} joins {counts[0]} views of "
                                     f"{self.image_encoder.model_output_dimension} features each: set "
                                     f"networks.image_encoder.image_features_dimension={want} (it is {have})")
        else:                                       # copied before the tower's kernels are enqueued: the pooling launch never waits for it
            offsets = offsets_to_device(study_offsets(counts), self.device)
        if torch.is_tensor(views):
            feat = self.image_encoder(views.to(self.device))
        else:
            feat = self.image_encoder([v.to(self.device) for v in views])
        return pool_views(feat, counts, method, offsets=offsets)

    def encode_images(self, batch):
        """[n,1,F,1,1] pre-extracted features -> [n,F] (mmgclip_model.py:76-93); pixel encoders take `batch['image']`
        (or a 4-D `image_features`) and run the ConvNeXt tower; `batch['image']` may be a list of [Cin,H_i,W_i] tensors of different sizes,
        or a batch of exams (a list of lists of views, or a 5-D [S,k,Cin,H,W] tensor): one feature row per study (`_encode_studies`)."""
        name = self.config.networks.image_encoder.name
        if name in PIXEL_ENCODERS:
            pix = batch["image"] if "image" in batch else batch["image_features"]
            if (torch.is_tensor(pix) and pix.dim() == 5 and "image" in batch) or \
                    (isinstance(pix, (list, tuple)) and any(isinstance(s, (list, tuple)) for s in pix)):
                return self._encode_studies(pix)
            if isinstance(pix, (list, tuple)):      # images of different sizes (ConvNeXt towers): [Cin, H_i, W_i] each
                return self.image_encoder([p.to(self.device) for p in pix])
            return self.image_encoder(pix.to(self.device))
        flattened_embeddings = torch.flatten(batch['image_features'].to(self.device), 1)
        if name == "ResNet50Encoder":
            return self.image_encoder(flattened_embeddings)
        return flattened_embeddings

    def encode_text(self, batch, text_pooling='eos'):
        """BERT last hidden state pooled at the [SEP] position = attention_mask.sum(-1) - 1 (mmgclip_model.py:95-115)."""
        src = batch['text_tokens']
        host_mask = src['attention_mask'] if ('attention_mask' in src and not src['attention_mask'].is_cuda) else None
        tokens = src.to(self.device) if hasattr(src, "to") else {k: v.to(self.device) for k, v in src.items()}
        if host_mask is not None and tokens['attention_mask'] is not host_mask:
            # prompt lengths read from the batch while it is still on the host: the unpadded text tower needs them there
            m = tokens['attention_mask']
            m._mmg_seq_lens = (m._version, type(self.text_encoder).sequence_lengths(host_mask))
        if isinstance(batch, dict):
            batch['text_tokens'] = tokens                      # the reference's BatchEncoding.to() is in-place
        hidden = self.text_encoder.hidden_states(tokens)       # bf16 [n*S, H]
        if text_pooling == 'eos':
            B, S = tokens['input_ids'].shape
            return EosPool.apply(hidden, tokens['attention_mask'], B, S)
        raise NotImplementedError(f"{text_pooling} method is not implemented...")

    # ---- the two towers on two HIP streams (default with a pixel image encoder; MMG_TEXT_STREAM=0 / networks.text_stream: false = off) ----
    # The text tower's kernels are small (~11 k tokens: its GEMMs fill half the GPU) next to the image tower's.  The text tower - every
    # pass of it, so that its backwards stay serialised on one stream - is enqueued on a side stream before the image tower goes onto the
    # current one, and autograd replays each backward on the stream of its forward, so both directions overlap (same-run A/B at C2:
    # 332.4 -> 327.5 ms/step).  Cross-stream tensors are registered with the allocator (record_stream); join_streams() makes the
    # current stream wait for the side stream (call it after backward, before optimizer.step()).
    text_stream_enabled = True      # set False on an instance to run both towers on the caller's stream (bench.py's profiled steps)

    def _text_stream(self):
        if not self.text_stream_enabled:
            return None
        on = os.environ.get("MMG_TEXT_STREAM")
        on = (on == "1") if on is not None else bool(_get(self.config.networks, "text_stream", True))
        if not on or not torch.cuda.is_available() or self.config.networks.image_encoder.name not in PIXEL_ENCODERS:
            return None
        if getattr(self, "_side_stream", None) is None:
            self._side_stream = torch.cuda.Stream()
        return self._side_stream

    def join_streams(self):
        side = getattr(self, "_side_stream", None)
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)

    def forward(self, batch, **kwargs):
        side = self._text_stream()
        if side is not None:
            main = torch.cuda.current_stream()
            side.wait_stream(main)                                   # parameters updated by the optimizer, tokens copied by the caller
            # the image tower is enqueued first: its large kernels keep the GPU busy while the host is still launching the text
            # tower's several hundred small ones (MMG_TEXT_FIRST=1: the other order, for A/B runs)
            text_first = os.environ.get("MMG_TEXT_FIRST", "0") == "1"
            if not text_first:
                image_features = self.encode_images(batch)
            with torch.cuda.stream(side):
                text_features = self.encode_text(batch, text_pooling='eos')
            if text_first:
                image_features = self.encode_images(batch)
            main.wait_stream(side)
            text_features.record_stream(main)
        else:
            image_features = self.encode_images(batch)
            text_features = self.encode_text(batch, text_pooling='eos')

        image_embeddings = self.image_projection_layer(image_features) if self.image_projection_layer is not None else image_features
        text_embeddings = self.text_projection_layer(text_features) if self.text_projection_layer is not None else text_features

        image_embeddings = head.L2Normalize.apply(image_embeddings)        # :128
        text_embeddings = head.L2Normalize.apply(text_embeddings)          # :129
        logit_scale = self.logit_scale.exp()                               # :132

        output = {"image_embeddings": image_embeddings, "text_embeddings": text_embeddings, "logit_scale": logit_scale}
        if self.config.loss.config.loss_name == "SigmoidCLIPLoss":
            output["logit_bias"] = self.logit_bias
        if kwargs.get("materialize_logits", True):
            li, lt = head.ScaledLogits.apply(image_embeddings, text_embeddings, logit_scale)   # :135-136
            output["logits_per_image"], output["logits_per_text"] = li, lt

        if self.config.loss.config.loss_name == "MMGCLIPLoss" and not kwargs.get('validation', False) == True:  # noqa: E712
            batch['text_tokens'] = batch['image_impression_tokens']        # :160 (mutates the batch, like the reference)
            if side is not None:                                           # the same tower: same stream as its first pass
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    text_features2 = self.encode_text(batch, text_pooling='eos')
                torch.cuda.current_stream().wait_stream(side)
                text_features2.record_stream(torch.cuda.current_stream())
            else:
                text_features2 = self.encode_text(batch, text_pooling='eos')
            text_embeddings2 = self.text_projection_layer(text_features2)
            output['text_embeddings2'] = head.L2Normalize.apply(text_embeddings2)
        return output


class PromptClassifier(nn.Module):
    """Zero-shot classifier wrapper around an MMGCLIP model — drop-in for mmgclip/networks/mmgclip_model.py:168-257.

    `forward(image_features, class_list, visualize, image_id, ground_truth)` tokenises the class prompts
    (`padding="max_length"`, `max_length = config.tokenizer.config.sequence_length`), runs the model in eval mode without
    gradients and returns `classes_similarities = softmax(logits_per_image)` [n, k], `similarities_argmax` (of the first
    image, like the reference) and `class_list`.  `tokenizer` (additive argument): a callable with the HF tokenizer call
    signature; by default `AutoTokenizer.from_pretrained(config.tokenizer.config.tokenizer_name)` as in the reference
    (`:185`), and - only where that vocabulary cannot be loaded (offline box) - the hashed stand-in ids of
    `dataset/synthetic.py`, with a warning.  The bar plot (`:212-255`) is drawn when matplotlib is importable.
    """

    def __init__(self, model=None, tokenizer=None):
        super().__init__()
        self.model = model
        self.device = model.device
        self.tokenizer = tokenizer
        if self.tokenizer is None:
            name = self.model.config.tokenizer.config.tokenizer_name
            try:
                from transformers import AutoTokenizer
                self.tokenizer = AutoTokenizer.from_pretrained(pretrained_model_name_or_path=name)
            except Exception as e:      # no vocabulary on an offline machine
                logger.warning(f"tokenizer `{name}` unavailable ({type(e).__name__}); using hashed stand-in token ids")

    def _tokens(self, class_list):
        S = self.model.config.tokenizer.config.sequence_length
        if self.tokenizer is not None:
            return self.tokenizer(class_list, padding="max_length", truncation=True, return_tensors="pt", max_length=S)
        from ..dataset.synthetic import synthetic_prompt_tokens
        vocab = self.model.text_encoder.model.embeddings.word_embeddings.weight.shape[0]
        return synthetic_prompt_tokens(list(class_list), S, vocab_size=vocab)

    def forward(self, image_features, class_list, visualize=True, image_id=None, ground_truth=None):
        inputs = {"image_features": image_features, "text_tokens": self._tokens(class_list)}
        self.model.eval()
        with torch.no_grad():
            classes_similarities = self.model(inputs)['logits_per_image']        # images are rows, prompts are columns
            classes_similarities = classes_similarities.softmax(dim=-1)
        outputs = {"classes_similarities": classes_similarities,
                   "similarities_argmax": torch.argmax(classes_similarities, dim=-1)[0].item(),
                   "class_list": class_list}
        if visualize:
            assert image_id is not None, "For visualizing results, image_id value is required."
            try:
                import matplotlib.pyplot as plt
            except ImportError:
                logger.warning("matplotlib is not installed: skipping the probability plot")
                return outputs
            probs = classes_similarities.detach().cpu().numpy().reshape(-1)[:len(class_list)]
            y = np.arange(len(class_list))
            plt.figure(figsize=(7, 6))
            plt.barh(y, probs)
            plt.gca().invert_yaxis()
            plt.yticks(y, class_list)
            plt.xlabel("probability")
            plt.title(f"{image_id}" + (f"  TP: {ground_truth}" if ground_truth else ""))
            plt.show()
        return outputs


class ReportRetriever(PromptClassifier):
    """Nearest-report search around an MMGCLIP model, beside `PromptClassifier` (additive: the reference has no search, only the
    dense scoring of a handful of prompts above).  The tokenizer is resolved exactly as `PromptClassifier` resolves it, the hashed
    stand-in included.

    `build(texts)` encodes the strings once, in batches, into the normalised text embeddings the model's forward returns (the ones
    `validate()` feeds to `RetrievalMetrics.update`) and keeps them in a `search.EmbeddingIndex`; `forward(image_features, k)` embeds
    the images the same way and returns, per image, the k nearest strings under (score descending, index ascending):
    `{"indices": int64 [n,k], "scores": fp32 [n,k], "texts": n lists of k strings}` (None where k exceeds the number of strings).
    No [n,N] matrix is formed (csrc/topk_head.hip)."""

    def __init__(self, model=None, tokenizer=None):
        super().__init__(model=model, tokenizer=tokenizer)
        self.texts = []
        self.index = None

    def _embed(self, features, projection):
        if projection is not None:
            features = projection(features)
        return head.L2Normalize.apply(features).float().contiguous()

    def build(self, texts, batch_size=256):
        from ..search import EmbeddingIndex
        texts = list(texts)
        if not texts or any(not isinstance(t, str) for t in texts):
            raise ValueError("build() needs a non-empty list of strings")
        self.model.eval()
        rows = []
        with torch.no_grad():
            for a in range(0, len(texts), batch_size):
                feats = self.model.encode_text({"text_tokens": self._tokens(texts[a:a + batch_size])}, text_pooling='eos')
                rows.append(self._embed(feats, self.model.text_projection_layer))
        self.texts = texts
        self.index = EmbeddingIndex(torch.cat(rows).contiguous())
        return self

    def forward(self, image_features, k=5):
        if self.index is None:
            raise RuntimeError("ReportRetriever.forward() before build(texts)")
        self.model.eval()
        with torch.no_grad():
            queries = self._embed(self.model.encode_images({"image_features": image_features}), self.model.image_projection_layer)
            scores, indices = self.index.search(queries, k)
        return {"indices": indices, "scores": scores,
                "texts": [[self.texts[j] if j >= 0 else None for j in row] for row in indices.tolist()]}
