"""Host side of native-size training: rectangular synthetic images, the [H, W] config form, floored feature-map sizes, grouping a batch of
differently sized images into micro-batches.  No GPU needed."""
import os

import pytest
import torch
import torch.nn.functional as F

CFG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmg-clip_amd", "configs")


def test_synthetic_batch_square_draw_is_unchanged_and_pairs_give_rectangles():
    from mmgclip.dataset.synthetic import synthetic_batch, synthetic_tokens
    b = synthetic_batch(5, S=33, image_size=64, in_chans=1, vocab_size=3000, seed=11)
    # the draw as it has always been: same generator calls in the same order
    g = torch.Generator().manual_seed(11)
    img = torch.rand(5, 1, 64, 64, generator=g)
    tok = synthetic_tokens(5, 33, 3000, g)
    lab = torch.randint(0, 2, (5, 1), generator=g)
    assert torch.equal(b["image"], img) and torch.equal(b["image_label"], lab)
    assert all(torch.equal(b["text_tokens"][k], tok[k]) for k in tok)
    for size in ((100, 70), [100, 70]):
        r = synthetic_batch(3, S=33, image_size=size, in_chans=2, vocab_size=3000, seed=11)
        assert r["image"].shape == (3, 2, 100, 70) and r["image"].dtype == torch.float32
    # a square pair is the int's draw
    assert torch.equal(synthetic_batch(5, S=33, image_size=(64, 64), vocab_size=3000, seed=11)["image"], img)
    with pytest.raises(ValueError, match="pair"):
        synthetic_batch(2, image_size=(1, 2, 3))


def test_config_override_takes_an_h_w_pair_and_train_passes_it_to_the_dataset(tmp_path, monkeypatch):
    """`networks.image_encoder.image_size=[100,70]` composes, train.py's dataset keywords carry the pair, the loaders draw [n, Cin, 100, 70] and
    the experiment is constructed (the epochs need the GPU: tests/test_native_size_gpu.py)."""
    import train
    from mmgclip.config import compose
    from mmgclip.experiments import ClassifierExperiment as CE
    from mmgclip.networks import bert
    cfg = compose(CFG_DIR, "train_binary_class_clf", ["networks=clip_convnexttiny_bert_pixels", "networks.image_encoder.image_size=[100,70]"])
    assert cfg.networks.image_encoder.image_size == [100, 70]
    assert compose(CFG_DIR, "train_binary_class_clf", ["networks=clip_convnexttiny_bert_pixels"]).networks.image_encoder.image_size == 1024
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):
        kw.setdefault("num_hidden_layers", 1)
        kw.setdefault("vocab_size", 2000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)
    ran = []
    monkeypatch.setattr(CE.ClassifierExperiment, "run", lambda self: ran.append(self))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    exp = train.main(["--config-name", "train_prompt_clf", "networks=clip_convnexttiny_bert_pixels", "tokenizer=bert_clinical_seqlen=77",
                      "networks.image_encoder.image_size=[100,70]", "dataset.config.synthetic_samples=1000",
                      f"checkpoints.checkpoints_export_dir={tmp_path}/ckpt", f"base.tensorboard_export_dir={tmp_path}/tb",
                      f"base.results_export_dir={tmp_path}/results"])
    assert ran == [exp]
    for loader in (exp.train_dataloader, exp.valid_dataloader, exp.test_dataloader):
        assert loader.kw["image_size"] == (100, 70)
    b = next(iter(exp.test_dataloader))
    assert b["image"].shape == (64, 1, 100, 70) and b["text_tokens"]["input_ids"].shape == (64, 77)
    assert type(exp.model.image_encoder).__name__ == "ConvNextTinyEncoder"


@pytest.mark.parametrize("H,W,want", [(1906, 818, (59, 25)), (1024, 1024, (32, 32)), (77, 50, (2, 1)), (100, 70, (3, 2)), (238, 258, (7, 8)),
                                      (32, 32, (1, 1)), (63, 95, (1, 2))])
def test_feature_map_shape_follows_the_strided_convolutions(H, W, want):
    """The floor chain (H // 4, then // 2 three times) against torch's own 4x4 / 4 and 2x2 / 2 convolutions on zeros."""
    from mmgclip.networks.convnext import ConvNextTower
    tower = ConvNextTower("tiny")
    assert tower.feature_map_shape(H, W) == want
    x = F.conv2d(torch.zeros(1, 1, H, W), torch.zeros(1, 1, 4, 4), stride=4)
    for _ in range(3):
        x = F.conv2d(x, torch.zeros(1, 1, 2, 2), stride=2)
    assert tuple(x.shape[-2:]) == want


def test_feature_map_shape_equals_the_oracles_last_map():
    from mmgclip.networks.convnext import ConvNextTower
    from oracle import encoders_oracle as E
    torch.manual_seed(0)
    tower = ConvNextTower("tiny")
    sd = {k[len("model."):]: v for k, v in tower.state_dict().items()}
    with torch.no_grad():
        _, fmap = E.convnext_forward(sd, torch.rand(1, 1, 77, 50))
    assert tuple(fmap.shape[-2:]) == tower.feature_map_shape(77, 50) == (2, 1)


def test_group_by_size_order_boundaries_and_inverse():
    from mmgclip.networks.convnext import group_by_size
    sizes = [(100, 70), (77, 50), (100, 70), (64, 64), (77, 50), (100, 70), [77, 50]]
    mbs, inv = group_by_size(sizes, 2)
    # groups in order of first appearance, images in input order, at most 2 per micro-batch, never two sizes in one
    assert mbs == [[0, 2], [5], [1, 4], [6], [3]]
    order = [i for mb in mbs for i in mb]
    assert sorted(order) == list(range(len(sizes))) and [order[p] for p in inv] == list(range(len(sizes)))
    assert all(len({tuple(sizes[i]) for i in mb}) == 1 for mb in mbs)
    # one size: the micro-batch boundaries of a 4-D tensor, identity permutation
    mbs, inv = group_by_size([(64, 64)] * 5, 2)
    assert mbs == [[0, 1], [2, 3], [4]] and inv == [0, 1, 2, 3, 4]
    assert group_by_size([(40, 40), (32, 32)], 64) == ([[0], [1]], [0, 1])
    assert group_by_size([], 4) == ([], [])
    with pytest.raises(ValueError):
        group_by_size([(64, 64)], 0)


def test_fixed_size_encoders_reject_a_list_of_images():
    """ViT has learned positions (one size), the ResNet path is not part of this: both say so instead of failing somewhere inside."""
    from mmgclip.networks.encoder import ResNet50Encoder, ViTB16Encoder
    imgs = [torch.rand(1, 32, 32), torch.rand(1, 64, 32)]
    with pytest.raises(ValueError, match="not a list"):
        ViTB16Encoder(image_size=32, layers=1)(imgs)
    with pytest.raises(ValueError, match="not a list"):
        ResNet50Encoder(pretrained=False)(imgs)


def test_convnext_tower_checks_a_list_before_touching_the_device():
    from mmgclip.networks.convnext import ConvNextTower
    tower = ConvNextTower("tiny")
    with pytest.raises(ValueError, match=r"\[Cin, H, W\]"):
        tower([torch.rand(1, 1, 64, 64)])
    with pytest.raises(ValueError, match=r"\[Cin, H, W\]"):
        tower([])
