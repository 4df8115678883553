"""Weighted k-NN classification on frozen embeddings - the evaluation MoCo / DINO / DeepCluster-v2 run beside the linear probe
(`knn_classifier` of DINO's eval_knn.py: cosine similarity, top-k, votes weighted by exp(sim / T)).  One pass over the data, no
optimiser.

The hot path is `audiossl_knn_topk` (csrc/knn.hip): bf16 MFMA dot products reduced to each query's k best bank rows inside the
kernel, so the [Nq, Nb] similarity matrix is never stored; `audiossl_knn_vote` turns the k neighbours into a label.
Everything here allocates through torch (outputs, the kernel's workspace, the normalised bf16 copies), so torch's memory
statistics see every byte.  Single GPU: the bank lives on one device (sharding it over ranks is out of scope).
"""

import torch

from src import _native as N

MAX_K = 128
SLAB = 4096          # queries per launch: bounds the workspace and the outputs of one call, not Nq
NORM_ROWS = 16384    # rows normalised per launch: bounds the fp32 scratch of a large bank


def normalize_bf16(x):
    """[n, d] fp32 / bf16 (device) -> L2-normalised rows rounded to bf16, zero-padded to a multiple of 32 columns (a zero column
    changes no dot product): `l2norm_fwd`, the kernel the MoCo head normalises its queries with."""
    if not x.is_cuda:
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    n, d = x.shape
    dp = (d + 31) // 32 * 32
    out = torch.empty(n, dp, dtype=torch.bfloat16, device=x.device)
    rows = min(n, NORM_ROWS)
    n32 = torch.empty(rows, dp, dtype=torch.float32, device=x.device)       # l2norm_fwd's fp32 twin: scratch here
    inv = torch.empty(rows, dtype=torch.float32, device=x.device)
    for i in range(0, n, rows):
        xs = x[i:i + rows].float()
        if dp != d:
            xs = torch.nn.functional.pad(xs, (0, dp - d))
        xs = xs.contiguous()
        N.call("l2norm_fwd", N.BF16, xs, xs.shape[0], dp, out[i:i + rows], n32, inv)
    return out


def workspace_bytes(nq, nb, k):
    return N.workspace_bytes("knn_workspace", nq, nb, k)


def knn_topk_bf16(q, bank, k):
    """The kernel as it is: q [Nq, D], bank [Nb, D] bf16 rows (D % 32 == 0, 32 <= D <= 4096) -> (top_sim fp32 [Nq, k] descending,
    top_idx int32 [Nq, k]); equal similarities in ascending bank row.  No normalisation."""
    if q.dtype != torch.bfloat16 or bank.dtype != torch.bfloat16:
        raise TypeError("knn_topk_bf16 takes bf16 rows; knn_topk normalises and rounds fp32 input")
    nq, d = q.shape
    nb = bank.shape[0]
    if bank.shape[1] != d:
        raise ValueError(f"query width {d} != bank width {bank.shape[1]}")
    top_sim = torch.empty(nq, k, dtype=torch.float32, device=q.device)
    top_idx = torch.empty(nq, k, dtype=torch.int32, device=q.device)
    nbytes = workspace_bytes(nq, nb, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    N.call("knn_topk", q, bank, nq, nb, d, k, top_sim, top_idx, ws, nbytes)
    return top_sim, top_idx


def _slabs(qn, bank_n, k, slab):
    if qn.shape[0] <= slab:
        return knn_topk_bf16(qn, bank_n, k)
    parts = [knn_topk_bf16(qn[i:i + slab], bank_n, k) for i in range(0, qn.shape[0], slab)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def knn_topk(q, bank, k, slab=SLAB):
    """Cosine top-k: q [Nq, d], bank [Nb, d] fp32 or bf16 of any width -> (top_sim [Nq, k], top_idx [Nq, k]).  Rows are
    normalised and rounded to bf16 first; queries go through the kernel `slab` rows at a time, so Nq is unbounded."""
    return _slabs(normalize_bf16(q), normalize_bf16(bank), int(k), int(slab))


def knn_predict(top_sim, top_idx, bank_labels, temperature=0.07):
    """-> (pred int64 [Nq], conf fp32 [Nq]): the label with the largest sum of exp((sim - row max) / T) over a query's
    neighbours, ties to the smaller label; temperature None / inf = plain majority.  A row with an index outside the bank gets
    pred -1, conf NaN."""
    nq, k = top_sim.shape
    labels = bank_labels.to(device=top_sim.device, dtype=torch.int64).contiguous()
    inv_t = 0.0 if temperature is None or temperature == float("inf") else 1.0 / float(temperature)
    pred = torch.empty(nq, dtype=torch.int64, device=top_sim.device)
    conf = torch.empty(nq, dtype=torch.float32, device=top_sim.device)
    N.call("knn_vote", top_sim.float().contiguous(), top_idx.to(torch.int32).contiguous(), labels, nq, k, labels.shape[0], inv_t,
           pred, conf)
    return pred, conf


class KnnClassifier:
    """`KnnClassifier(k=20, temperature=0.07).fit(bank, labels).predict(q)`: the bank is normalised once."""

    def __init__(self, k=20, temperature=0.07, slab=SLAB):
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}]")
        self.k, self.temperature, self.slab = int(k), temperature, int(slab)
        self.bank = self.labels = None

    def fit(self, bank, labels):
        if bank.shape[0] != len(labels):
            raise ValueError("one label per bank row")
        if bank.shape[0] < self.k:
            raise ValueError(f"k = {self.k} neighbours need at least as many bank rows, got {bank.shape[0]}")
        self.bank = normalize_bf16(bank)
        self.labels = torch.as_tensor(labels).to(device=bank.device, dtype=torch.int64).contiguous()
        return self

    def neighbours(self, q):
        if self.bank is None:
            raise RuntimeError("fit() first")
        return _slabs(normalize_bf16(q), self.bank, self.k, self.slab)

    def predict(self, q, return_conf=False):
        pred, conf = knn_predict(*self.neighbours(q), self.labels, self.temperature)
        return (pred, conf) if return_conf else pred

    def score(self, q, y):
        y = torch.as_tensor(y).to(device=q.device, dtype=torch.int64)
        return float((self.predict(q) == y).float().mean())
