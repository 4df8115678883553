"""Exact nearest-neighbour graphs and the graph stages of power-iteration clustering (csrc/graph.hip), the partition score the
reference's DeepCluster trainers use to compare successive labelings, and the silhouette coefficient of one labeling on the
features it was computed on (csrc/silhouette.hip).

`knn_graph` is NOT `knn_topk`: that one forms cosine similarities on the bf16 MFMA pipe, which suits a vote over 20 neighbours
at temperature 0.07.  A graph is a discrete input to everything after it, and on whitened, L2-normalised features the gap
between the 5th and 6th neighbour is around 1e-4 of the squared norm - below bf16 resolution.  `audiossl_knn_graph_l2` works in
fp32 end to end (fp32-input MFMA, the n x n matrix never stored) and orders candidates by (d2 ascending, row ascending).
Everything allocates through torch; single GPU.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from src import _native as N

MAX_K, MAX_WIDTH = 64, 4096

# W = A + A^T in CSR on the device: rowptr int32 [n + 1], col int32 / w fp64 [capacity] (the first `nnz` entries are the matrix)
Csr = namedtuple("Csr", "rowptr col w nnz n")


def graph_workspace_bytes(n, k):
    return N.workspace_bytes("knn_graph_workspace", n, k)


def pic_workspace_bytes(n, k):
    return N.workspace_bytes("pic_workspace", n, k)


def silhouette_workspace_bytes(n):
    return N.workspace_bytes("silhouette_workspace", n)


def knn_graph(x, k):
    """x [n, d] (device) -> (idx int64 [n, k], d2 fp32 [n, k]): for every row its k nearest OTHER rows in squared L2, nearest
    first, equal distances by ascending row.  Self is excluded by index, so a duplicate of row i is its neighbour at distance 0.
    d is zero-padded to a multiple of 4 (a zero column changes no distance)."""
    if not x.is_cuda:
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    if x.dim() != 2:
        raise ValueError(f"points are [n, d], got {tuple(x.shape)}")
    n, d = x.shape
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    if k > n - 1:
        raise ValueError(f"k = {k} neighbours need at least {k + 1} points, got {n}")
    if not 1 <= d <= MAX_WIDTH:
        raise ValueError(f"width must be in [1, {MAX_WIDTH}], got {d}")
    x = x.float()
    if d % 4:
        x = F.pad(x, (0, 4 - d % 4))
    x = x.contiguous()
    idx = torch.empty(n, k, dtype=torch.int32, device=x.device)
    d2 = torch.empty(n, k, dtype=torch.float32, device=x.device)
    nbytes = graph_workspace_bytes(n, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    N.call("knn_graph_l2", x, n, x.shape[1], k, idx, d2, ws, nbytes)
    return idx.long(), d2


def pic_build(idx, d2, sigma, workspace=None):
    """Neighbour lists idx [n, k] (no self, no repeats in a row), d2 [n, k] -> `Csr` of W = A + A^T, A_ij = exp(-d2_ij / sigma^2)
    in fp64; columns ascending in every row, a mutual pair is one entry."""
    if not (idx.is_cuda and d2.is_cuda):
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    n, k = idx.shape
    idx = idx.to(torch.int32).contiguous()
    d2 = d2.float().contiguous()
    cap = 2 * n * k
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=idx.device)
    col = torch.empty(cap, dtype=torch.int32, device=idx.device)
    w = torch.empty(cap, dtype=torch.float64, device=idx.device)
    nnz = torch.empty(1, dtype=torch.int32, device=idx.device)
    nbytes = pic_workspace_bytes(n, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=idx.device) if workspace is None else workspace
    N.call("pic_build", idx, d2, n, k, float(sigma), rowptr, col, w, nnz, ws, nbytes)
    return Csr(rowptr, col, w, nnz, n)


def pic_power(W, alpha, iters=200):
    """-> v fp64 [n] after `iters` rounds of v <- normalise_1(alpha W v + (1 - alpha) / n) from v = 1 / n."""
    n = W.n
    v = torch.empty(n, dtype=torch.float64, device=W.col.device)
    nbytes = pic_workspace_bytes(n, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
    N.call("pic_power", W.rowptr, W.col, W.w, n, W.col.numel(), float(alpha), int(iters), v, ws, nbytes)
    return v


def pic_assign(W, v):
    """-> (label int32 [n], count int32 [1]) on the device: every node follows its steepest positive W_ij (v_j - v_i) to a local
    maximum of v; maxima are numbered in ascending node order."""
    n = W.n
    label = torch.empty(n, dtype=torch.int32, device=v.device)
    count = torch.empty(1, dtype=torch.int32, device=v.device)
    nbytes = pic_workspace_bytes(n, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
    N.call("pic_assign", W.rowptr, W.col, W.w, v.contiguous(), n, W.col.numel(), label, count, ws, nbytes)
    return label, count


def _entropy(counts, n):
    p = counts[counts > 0].double() / n
    return -(p * p.log()).sum()


def partition_nmi(a, b):
    """Normalised mutual information of two labelings of the same items - sklearn's `normalized_mutual_info_score(a, b)`
    (arithmetic mean of the entropies in the denominator), which the reference's DeepCluster trainers print between epochs.
    a, b: integer sequences / arrays / tensors (any device); label values are arbitrary.  -> python float; 1.0 when both
    labelings have a single cluster (sklearn's convention)."""
    a = torch.as_tensor(a).reshape(-1)
    b = torch.as_tensor(b).reshape(-1).to(a.device)
    if a.numel() != b.numel():
        raise ValueError(f"labelings of {a.numel()} and {b.numel()} items")
    n = a.numel()
    if n == 0:
        return 1.0
    ua, ia = torch.unique(a, return_inverse=True)
    ub, ib = torch.unique(b, return_inverse=True)
    ka, kb = ua.numel(), ub.numel()
    if ka == kb == 1:
        return 1.0
    ca, cb = torch.bincount(ia, minlength=ka), torch.bincount(ib, minlength=kb)
    pair = torch.bincount(ia * kb + ib, minlength=ka * kb)                   # the contingency table, flattened
    nz = pair.nonzero().reshape(-1)
    nij = pair[nz].double()
    outer = ca[nz // kb].double() * cb[nz % kb].double()
    log_n = math.log(n)
    mi = (nij / n * ((nij.log() - log_n) + (2.0 * log_n - outer.log()))).sum().clamp_min(0.0)
    ha, hb = _entropy(ca, n), _entropy(cb, n)
    denom = 0.5 * (ha + hb)
    eps = torch.finfo(torch.float64).eps
    return float(mi / denom.clamp_min(eps))


@torch.no_grad()
def silhouette_samples(x, labels):
    """sklearn's `silhouette_samples(x, labels)` (Euclidean) -> fp64 [n] on x's device, in the caller's order: s_i = (b_i - a_i) /
    max(a_i, b_i) with a_i the mean distance to the other members of i's cluster and b_i the smallest mean distance to another
    cluster's members; 0 for a one-member cluster.  x [n, d] (device); labels: any integer sequence / array / tensor, values are
    arbitrary (negative, sparse).  No distance matrix is stored: the rows are sorted by cluster (stable) and `audiossl_silhouette`
    walks all pairs once.  d is zero-padded to a multiple of 4.  Reads the cluster sizes back (one small copy to the host)."""
    if not x.is_cuda:
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    if x.dim() != 2:
        raise ValueError(f"points are [n, d], got {tuple(x.shape)}")
    n, d = x.shape
    labels = torch.as_tensor(labels).reshape(-1)
    if labels.numel() != n:
        raise ValueError(f"{n} points and {labels.numel()} labels")
    if labels.is_floating_point() or labels.is_complex():
        raise ValueError(f"labels are integers, got {labels.dtype}")
    if not 1 <= d <= MAX_WIDTH:
        raise ValueError(f"width must be in [1, {MAX_WIDTH}], got {d}")
    _, inverse, counts = torch.unique(labels.to(x.device), return_inverse=True, return_counts=True)
    K = counts.numel()
    if not 2 <= K <= n - 1:
        raise ValueError(f"Number of labels is {K}. Valid values are 2 to n_samples - 1 (inclusive)")      # sklearn's rule and wording
    order = torch.sort(inverse, stable=True).indices
    xs = x.float()[order]
    if d % 4:
        xs = F.pad(xs, (0, 4 - d % 4))
    xs = xs.contiguous()
    seg = torch.zeros(K + 1, dtype=torch.int32, device=x.device)
    seg[1:] = torch.cumsum(counts, 0)
    seg_host = seg.cpu()                                                     # the entry point checks it before any launch
    s = torch.empty(n, dtype=torch.float64, device=x.device)
    nbytes = silhouette_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    N.call("silhouette", xs, n, xs.shape[1], seg, seg_host.data_ptr(), K, s, ws, nbytes)
    out = torch.empty_like(s)
    out[order] = s
    return out


def silhouette_score(x, labels):
    """sklearn's `silhouette_score(x, labels)`: the fp64 mean of `silhouette_samples` -> python float."""
    return float(silhouette_samples(x, labels).mean())
