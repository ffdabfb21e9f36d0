"""Nearest-report search: which of the N rows of a gallery (reports, prompts, earlier exams) stand closest to a query, from the fused
top-K kernel of csrc/topk_head.hip (`head._HipTopKBackend`).  The reference has no search: its `PromptClassifier` scores a handful of
hand-written prompts densely (mmgclip/networks/mmgclip_model.py:168-257).

The order.  Row i receives its k best admissible columns under ONE total order: score descending, then global column index ascending.
A total order has a unique top-k, so the answer does not depend on how it was reached: the gallery may be streamed in chunks
(`chunk_rows`), sharded over the ranks of a data-parallel run, or searched in one launch, and scores AND indices come out bit for bit
the same.  Slots beyond the number of admissible columns hold -inf / -1.  `torch.topk` on `X @ Y.T` promises no tie order and needs the
[n,N] matrix; nothing here allocates one: per launch the device holds the [n,k] lists.

Exclusions (the hardest negatives of a batch are its top-k with the positives left out):
    None                               every column is admissible
    ("diagonal", off)                  query i does not see column off + i (i counts the queries of all ranks, in rank order)
    ("labels", row_key, col_label)     query i does not see the columns whose label equals row_key[i] (`retrieval_positive`'s rule);
                                       int64, `col_label` one per LOCAL gallery row

Sharded (an active `comm`): the constructor's rows are this rank's shard of the gallery, in rank order; shards may be uneven, the row
counts are gathered once.  A search all-gathers the queries (padded to the longest shard, the padding dropped by index, as
`RetrievalMetrics._gather`), searches the own shard with `j_base` at its offset, all-gathers the [n_all,k] lists, merges them with
`merge_topk` under the same order and hands back the local queries' rows."""
import torch

from . import head

MAX_K = 32
_PAD_LAST = torch.iinfo(torch.int64).max


def merge_topk(scores, indices, k):
    """[n,m] candidate lists (any order inside a row, padding = -inf / -1, every real index at most once) -> the [n,k] best under
    (score descending, index ascending), padded.  Two stable sorts: by index ascending with the padding last, then by score descending."""
    if scores.ndim != 2 or scores.shape != indices.shape:
        raise ValueError(f"scores / indices must be [n,m] candidate lists of one shape, got {tuple(scores.shape)} / {tuple(indices.shape)}")
    n, m = scores.shape
    by_index = torch.sort(torch.where(indices < 0, _PAD_LAST, indices.to(torch.int64)), dim=1, stable=True).indices
    s, j = scores.gather(1, by_index), indices.gather(1, by_index)
    by_score = torch.sort(s, dim=1, descending=True, stable=True).indices
    s, j = s.gather(1, by_score)[:, :k], j.gather(1, by_score)[:, :k]
    if m < k:
        s = torch.cat([s, s.new_full((n, k - m), float("-inf"))], dim=1)
        j = torch.cat([j, j.new_full((n, k - m), -1)], dim=1)
    return s.contiguous(), j.contiguous()


def _check_rows(name, t, D=None):
    if not torch.is_tensor(t) or t.ndim != 2:
        raise ValueError(f"{name} must be a [rows,D] tensor, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be fp32 (L2-normalised rows as the model returns them), got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if D is not None and t.shape[1] != D:
        raise ValueError(f"{name} has D={t.shape[1]}, the index holds D={D}")


class EmbeddingIndex:
    """A gallery of fp32, contiguous, L2-normalised rows (it does not normalise) and `search()` over it."""

    def __init__(self, embeddings, comm=None, chunk_rows=None):
        _check_rows("embeddings", embeddings)
        if chunk_rows is not None and (isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1):
            raise ValueError(f"chunk_rows must be None or a positive integer, got {chunk_rows!r}")
        self.embeddings = embeddings.detach()
        self.comm = comm
        self.chunk_rows = chunk_rows
        n = self.embeddings.shape[0]
        self.counts = self._counts(n)                       # gallery rows of every rank, in rank order (gathered once)
        self.offset = sum(self.counts[:comm.rank]) if self._sharded else 0
        self.total = sum(self.counts)

    @property
    def _sharded(self):
        return self.comm is not None and self.comm.active

    def __len__(self):
        return self.total

    def _counts(self, n):
        if not self._sharded:
            return [n]
        return self.comm.all_gather_rows(torch.tensor([n], dtype=torch.int64, device=self.embeddings.device)).tolist()

    def _gather(self, t, counts):
        """The ranks' stacks `t` [counts[r], ...] one under the other: padded to the longest for the all-gather, the padding dropped
        by index."""
        longest = max(counts)
        if t.shape[0] < longest:
            t = torch.cat([t, t.new_zeros((longest - t.shape[0],) + tuple(t.shape[1:]))])
        keep = torch.cat([torch.arange(r * longest, r * longest + c, device=t.device) for r, c in enumerate(counts)])
        return self.comm.all_gather_rows(t).index_select(0, keep).contiguous()

    def _parse_exclude(self, exclude, n):
        """-> (mode, row_key, col_label, diag_off) in the kernel's spelling."""
        if exclude is None:
            return 0, None, None, 0
        if not isinstance(exclude, (tuple, list)) or not exclude or exclude[0] not in ("diagonal", "labels"):
            raise ValueError(f'exclude must be None, ("diagonal", off) or ("labels", row_key, col_label), got {exclude!r}')
        if exclude[0] == "diagonal":
            if len(exclude) != 2 or isinstance(exclude[1], bool) or not isinstance(exclude[1], int) or exclude[1] < 0:
                raise ValueError(f'exclude=("diagonal", off) needs one integer off >= 0, got {exclude!r}')
            return 1, None, None, exclude[1]
        if len(exclude) != 3:
            raise ValueError('exclude=("labels", row_key, col_label) needs the queries\' keys and the local gallery\'s labels')
        row_key, col_label = exclude[1], exclude[2]
        for name, t, rows in (("row_key", row_key, n), ("col_label", col_label, self.embeddings.shape[0])):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or t.ndim != 1 or t.shape[0] != rows:
                raise ValueError(f"{name} must be an int64 vector with one entry per {'query' if name == 'row_key' else 'local gallery row'} ({rows})")
        return 2, row_key.contiguous(), col_label.contiguous(), 0

    def _search_local(self, queries, k, mode, row_key, col_label, diag_off):
        """The local shard, streamed in chunks of `chunk_rows` through j_base / accumulate -> (fp32 [n,k], int32 [n,k])."""
        be = head._HipTopKBackend
        n, rows = queries.shape[0], self.embeddings.shape[0]
        if rows == 0:                                        # an empty shard has nothing to offer: all padding
            return (torch.full((n, k), float("-inf"), device=queries.device, dtype=torch.float32),
                    torch.full((n, k), -1, device=queries.device, dtype=torch.int32))
        step = rows if self.chunk_rows is None else self.chunk_rows
        out = None
        for a in range(0, rows, step):
            lab = None if col_label is None else col_label[a:a + step]
            out = be.topk(queries, self.embeddings[a:a + step], k, mode, row_key, lab, diag_off, self.offset + a, out)
        return out

    def search(self, queries, k, exclude=None):
        """(scores fp32 [n,k], indices int64 [n,k]) of the local `queries` [n,D] against the WHOLE gallery."""
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"k must be a positive integer, got {k!r}")
        if k > MAX_K:
            raise ValueError(f"k={k} is above the limit of {MAX_K} neighbours per query")
        D = self.embeddings.shape[1]
        _check_rows("queries", queries, D)
        if not head._HipTopKBackend.supported(D, k):
            raise ValueError(f"D={D} with k={k} is unsupported: the staged rows and the candidate lists do not fit the LDS of one launch")
        if self.total > 2 ** 31 - 1:
            raise ValueError(f"a gallery of {self.total} rows does not fit the int32 indices of the kernel")
        queries = queries.detach()
        n = queries.shape[0]
        mode, row_key, col_label, diag_off = self._parse_exclude(exclude, n)
        if not self._sharded:
            scores, indices = self._search_local(queries, k, mode, row_key, col_label, diag_off)
            return scores, indices.to(torch.int64)
        qcounts = self.comm.all_gather_rows(torch.tensor([n], dtype=torch.int64, device=queries.device)).tolist()
        q_all = self._gather(queries, qcounts)
        key_all = None if row_key is None else self._gather(row_key, qcounts)
        scores, indices = self._search_local(q_all, k, mode, key_all, col_label, diag_off)
        world, n_all = self.comm.world_size, q_all.shape[0]
        scores = self.comm.all_gather_rows(scores).reshape(world, n_all, k).transpose(0, 1).reshape(n_all, world * k)
        indices = self.comm.all_gather_rows(indices).reshape(world, n_all, k).transpose(0, 1).reshape(n_all, world * k)
        scores, indices = merge_topk(scores, indices.to(torch.int64), k)
        q_off = sum(qcounts[:self.comm.rank])
        return scores[q_off:q_off + n].contiguous(), indices[q_off:q_off + n].contiguous()
