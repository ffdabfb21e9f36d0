"""Retrieval metrics at validation: image-to-text and text-to-image recall@K, median rank and MRR of the validation set's own
(image, report) pairs, from the fused rank kernel of csrc/retrieval_head.hip (`head._HipRetrievalBackend`).  The reference has no such
metric; nothing here runs unless `experiments.config.retrieval` is set (ClassifierExperiment.validate).

What is a hit.  For query i the kernel gives the best score among its positives and the number of NEGATIVES scoring above (`n_gt`) and
exactly at (`n_eq`) that score; rank_i = 1 + n_gt + n_eq.  Ties count against the model: a collapsed model whose scores are all equal
ranks every query last, R@K = 0, not first.  Other positives never push a positive down - which is the point on this data, where
validation batches repeat prompts:
    positives "diagonal"  pair (i, i) only, the textbook metric;
              "text"      every report with the same token ids as report i (exact duplicates share a key);
              "clusters"  every report in the greedy-threshold cluster of report i: the clustering of `FusedAveragedLoss` /
                          `SigmoidCLIPLoss(positives="clusters")` on the gathered text (same kernels, same threshold; it forms a
                          transient [N,N] fp32 similarity, 1 GiB at N = 16384 - the one dense allocation of this module, and only
                          in this mode).
The same keys serve both directions: text j is a positive of image i, and image j of text i, when report j carries report i's key.

No [n,N] matrix and no sort: per direction the device holds four [n_loc] vectors, then one histogram of the ranks.

Ranks of a data-parallel run: every rank ranks its LOCAL queries against the GLOBAL gallery.  Shards may be uneven (a validation set
rarely divides by the world size): the row counts are gathered first, every rank pads its stack to the longest shard for the
all-gather, and the padding is dropped by index afterwards, so no padded row ever reaches the kernel.  The per-query indicators are
summed over the ranks as ONE int64 all-reduce per `compute()`: for each direction the histogram of the ranks plus the tie and
no-positive counts.  Every metric is a function of those integers alone, so the dict is the same on every rank, bit for bit, and
does not depend on how the queries were split."""
import math

import torch

from . import head

POSITIVES = ("diagonal", "text", "clusters")
PAD_ID = 0          # what a shorter batch's token ids are filled with up to the common length (BERT's [PAD], as the tokenizer pads)


def parse_config(node):
    """`experiments.config.retrieval` -> the keyword arguments of RetrievalMetrics, or None when the key is null / absent."""
    if node is None:
        return None
    if not isinstance(node, dict):
        raise ValueError(f"experiments.config.retrieval must be null or a mapping with ks / positives / similarity_threshold, got {node!r}")
    unknown = set(node) - {"ks", "positives", "similarity_threshold"}
    if unknown:
        raise ValueError(f"experiments.config.retrieval: unknown keys {sorted(unknown)}")
    kw = {k: node[k] for k in ("ks", "positives", "similarity_threshold") if node.get(k) is not None}
    RetrievalMetrics(**kw)          # validates
    return kw


class RetrievalMetrics:
    def __init__(self, ks=(1, 5, 10), positives="diagonal", similarity_threshold=0.65, comm=None):
        if positives not in POSITIVES:
            raise ValueError(f"positives must be one of {POSITIVES}, got {positives!r}")
        if isinstance(ks, (str, bytes)) or not hasattr(ks, "__iter__"):
            raise ValueError(f"ks must be a list of positive integers, got {ks!r}")
        ks = list(ks)
        if not ks or any(isinstance(k, bool) or not isinstance(k, int) or k < 1 for k in ks) or len(set(ks)) != len(ks):
            raise ValueError(f"ks must be a non-empty list of distinct positive integers, got {ks!r}")
        self.ks = tuple(sorted(ks))
        self.positives = positives
        self.similarity_threshold = float(similarity_threshold)
        self.comm = comm
        self.reset()

    def reset(self):
        self._img, self._txt, self._ids = [], [], []

    def update(self, image_embeddings, text_embeddings, text_ids=None):
        """One validation batch: the L2-normalised rows as the model returns them ([n,D] each) and, for positives="text", the
        batch's `input_ids` [n,S].  Kept on the device in fp32; nothing is computed here."""
        img, txt = image_embeddings.detach().float(), text_embeddings.detach().float()
        if img.ndim != 2 or img.shape != txt.shape:
            raise ValueError(f"image / text embeddings must be [n,D] with one report per image, got {tuple(img.shape)} / {tuple(txt.shape)}")
        self._img.append(img.clone())
        self._txt.append(txt.clone())
        if self.positives == "text":
            if text_ids is None or text_ids.ndim != 2 or text_ids.shape[0] != img.shape[0]:
                raise ValueError('positives="text" needs the token ids [n,S] of every batch')
            self._ids.append(text_ids.detach().to(device=img.device, dtype=torch.int64))

    # ---- the exchanges ----------------------------------------------------------------------------------------------------------
    @property
    def _sharded(self):
        return self.comm is not None and self.comm.active

    def _shard_counts(self, n_loc, device):
        """Rows held by every rank, in rank order."""
        if not self._sharded:
            return [n_loc]
        return self.comm.all_gather_rows(torch.tensor([n_loc], dtype=torch.int64, device=device)).tolist()

    def _gather(self, t, counts):
        """The ranks' stacks `t` [counts[r], ...] one under the other.  Each rank pads to the longest shard for the all-gather; the
        padding is dropped by index."""
        if not self._sharded:
            return t
        longest = max(counts)
        if t.shape[0] < longest:
            t = torch.cat([t, t.new_zeros((longest - t.shape[0],) + tuple(t.shape[1:]))])
        keep = torch.cat([torch.arange(r * longest, r * longest + c, device=t.device) for r, c in enumerate(counts)])
        return self.comm.all_gather_rows(t).index_select(0, keep).contiguous()

    def _stack_ids(self, device):
        """The local token ids as one [n_loc,S] matrix, S the longest sequence on any rank."""
        width = max(t.shape[1] for t in self._ids)
        if self._sharded:
            width = max(self.comm.all_gather_rows(torch.tensor([width], dtype=torch.int64, device=device)).tolist())
        return torch.cat([torch.nn.functional.pad(t, (0, width - t.shape[1]), value=PAD_ID) for t in self._ids])

    # ---- the metrics --------------------------------------------------------------------------------------------------------------
    def compute(self):
        """{"i2t_R@1": ..., "i2t_median_rank": ..., "i2t_mrr": ..., "i2t_ties": ..., "i2t_n_queries": ..., "i2t_no_positive": ...,
        "t2i_...": ...}: plain Python numbers, identical on every rank."""
        if not self._img:
            raise ValueError("RetrievalMetrics.compute() before any update() on this rank")
        be = head._HipRetrievalBackend
        img, txt = torch.cat(self._img).contiguous(), torch.cat(self._txt).contiguous()
        n_loc, dev = img.shape[0], img.device
        counts = self._shard_counts(n_loc, dev)
        rank_id = self.comm.rank if self._sharded else 0
        off, N = sum(counts[:rank_id]), sum(counts)
        img_all, txt_all = self._gather(img, counts), self._gather(txt, counts)
        if self.positives == "diagonal":
            labels = key = None
        else:
            if self.positives == "text":
                labels = torch.unique(self._gather(self._stack_ids(dev), counts), dim=0, return_inverse=True)[1]
            else:
                labels = head._HipAveragedBackend.cluster(txt_all, self.similarity_threshold)[0]
            labels = labels.to(torch.int64).contiguous()
            key = labels[off:off + n_loc].contiguous()
        # per direction: the histogram of the ranks 1..N in [1..N], then the tie and no-positive counts
        stats = torch.stack([self._indicators(be.rank(x, y, key, labels, off), N)
                             for x, y in ((img, txt_all), (txt, img_all))])
        if self._sharded:
            stats = self.comm.all_reduce_sum(stats)
        out = {}
        for name, row in zip(("i2t", "t2i"), stats.tolist()):
            out.update(self._from_histogram(name, row[:N + 1], row[N + 1], row[N + 2]))
        return out

    @staticmethod
    def _indicators(ranked, N):
        _, n_pos, n_gt, n_eq = ranked
        has = n_pos > 0
        rank = (1 + n_gt.to(torch.int64) + n_eq.to(torch.int64))[has]
        hist = torch.bincount(rank, minlength=N + 1)[:N + 1]          # (a query with a positive has at most N - 1 negatives)
        tail = torch.stack([((n_eq > 0) & has).sum(), (~has).sum()]).to(torch.int64)
        return torch.cat([hist, tail])

    def _from_histogram(self, name, hist, ties, no_positive):
        """hist[r] = queries of rank r.  Integers in, so every figure below is the same whoever computes it: the recalls and `ties`
        are one correctly rounded division each, the MRR an exactly rounded sum (math.fsum) of its per-rank terms hist[r] / r."""
        n = sum(hist)
        nan = float("nan")
        out = {f"{name}_R@{k}": sum(hist[1:k + 1]) / n if n else nan for k in self.ks}
        lo = hi = None
        if n:
            seen = 0
            for r, h in enumerate(hist):          # the two middle order statistics (one and the same for an odd n)
                seen += h
                if lo is None and seen > (n - 1) // 2:
                    lo = r
                if seen > n // 2:
                    hi = r
                    break
        out[f"{name}_median_rank"] = (lo + hi) / 2 if n else nan
        out[f"{name}_mrr"] = math.fsum(h / r for r, h in enumerate(hist) if h) / n if n else nan
        out[f"{name}_ties"] = ties / n if n else nan
        out[f"{name}_n_queries"] = n
        out[f"{name}_no_positive"] = no_positive
        return out
