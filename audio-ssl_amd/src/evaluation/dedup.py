"""Near-duplicate and leakage search on embeddings (csrc/range.hip): the exact radius graph of a feature matrix - every pair of rows
closer than a radius, however many there are - and the connected components of that graph.

A top-k list cannot answer "which files are copies of each other": a group larger than k is cut off, and a clip without a copy
still gets k neighbours.  `range_graph` counts first (`audiossl_range_count`), reads the total back - the one host read of the
feature - allocates, and fills (`audiossl_range_fill`); distances are `knn_graph`'s (fp32 end to end, a repeated row at exactly 0,
d2_ij == d2_ji bit for bit).  Groups are SINGLE-LINKAGE: A-B and B-C within the threshold put A and C into one group even when A-C
is not; a loose threshold can chain.  Everything allocates through torch; single GPU.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from src import _native as N

MAX_WIDTH = 4096
DEFAULT_EDGES_PER_ROW = 64

# rowptr int32 [rows + 1], col int32 / d2 fp32 [total] on the device: row r's matches in ascending column
RangeCsr = namedtuple("RangeCsr", "rowptr col d2")

# group / size / degree / nearest int64 [n], nearest_sim fp64 [n], keep bool [n]: numpy, on the host; csr: the device graph
Duplicates = namedtuple("Duplicates", "group n_groups size degree keep nearest nearest_sim csr")


def cosine_to_radius2(tau):
    """Cosine similarity threshold -> squared L2 radius between UNIT rows: |a - b|^2 = 2 - 2 <a, b>, rounded to fp32 as the
    kernels compare it."""
    tau = float(tau)
    if not 0.0 < tau <= 1.0:
        raise ValueError(f"a cosine threshold lies in (0, 1], got {tau}")
    return float(np.float32(2.0 - 2.0 * tau))


def range_workspace_bytes(n, rows, splits=0):
    return N.workspace_bytes("range_workspace", n, rows, splits)


def components_workspace_bytes(n):
    return N.workspace_bytes("graph_components_workspace", n)


def _span(span, n, what):
    lo, hi = (0, n) if span is None else (int(span[0]), int(span[1]))
    if not 0 <= lo < hi <= n:
        raise ValueError(f"{what} rows [{lo}, {hi}) are not a non-empty range inside [0, {n})")
    return lo, hi


def range_graph(x, radius2, own=None, walk=None, max_edges=None, splits=0):
    """x [n, d] (device) -> `RangeCsr`: for every owned row i in own = (lo, hi) (default: all) the walked rows j != i in walk =
    (lo, hi) (default: all) with |x_i - x_j|^2 <= radius2, columns ABSOLUTE and ascending.  i == j leaves by index, so a repeated
    row is a match at distance 0.  d is zero-padded to a multiple of 4.  Raises ValueError when the graph has more than
    `max_edges` entries (default 64 per owned row) or 2^31: the threshold is too loose for a duplicate search."""
    if not x.is_cuda:
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    if x.dim() != 2:
        raise ValueError(f"points are [n, d], got {tuple(x.shape)}")
    n, d = x.shape
    if not 1 <= d <= MAX_WIDTH:
        raise ValueError(f"width must be in [1, {MAX_WIDTH}], got {d}")
    radius2 = float(np.float32(radius2))
    if not (radius2 >= 0.0 and np.isfinite(radius2)):
        raise ValueError(f"radius2 must be finite and >= 0, got {radius2}")
    splits = int(splits)
    if not 0 <= splits <= 64:
        raise ValueError(f"splits must be in [0, 64], got {splits}")
    own_lo, own_hi = _span(own, n, "owned")
    walk_lo, walk_hi = _span(walk, n, "walked")
    rows = own_hi - own_lo
    max_edges = DEFAULT_EDGES_PER_ROW * rows if max_edges is None else int(max_edges)
    x = x.float()
    if d % 4:
        x = F.pad(x, (0, 4 - d % 4))
    x = x.contiguous()
    nbytes = range_workspace_bytes(n, rows, splits)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    rowptr = torch.empty(rows + 1, dtype=torch.int32, device=x.device)
    total_d = torch.empty(1, dtype=torch.int64, device=x.device)
    geometry = (x, n, x.shape[1], own_lo, own_hi, walk_lo, walk_hi, radius2, splits)
    N.call("range_count", *geometry, rowptr, total_d, ws, nbytes)
    total = int(total_d.item())                                              # the one host read
    if total > max_edges or total >= 2 ** 31:
        raise ValueError(f"the radius graph has total = {total} entries for {rows} rows, more than max_edges = {max_edges}"
                         f"{' and than 2^31' if total >= 2 ** 31 else ''}: the threshold is too loose")
    col = torch.empty(total, dtype=torch.int32, device=x.device)
    d2 = torch.empty(total, dtype=torch.float32, device=x.device)
    if total:
        N.call("range_fill", *geometry, rowptr, total, col, d2, total, ws, nbytes)
    return RangeCsr(rowptr, col, d2)


def range_search(q, bank, radius2, max_edges=None, splits=0):
    """faiss `range_search`: q [nq, d], bank [nb, d] (device) -> `RangeCsr` over the queries, columns bank-relative: every bank
    row within radius2 of the query, ascending.  The two are stacked [bank; q]: the queries are owned, the bank is walked."""
    if q.dim() != 2 or bank.dim() != 2 or q.shape[1] != bank.shape[1]:
        raise ValueError(f"queries {tuple(q.shape)} and bank {tuple(bank.shape)} are not [nq, d] and [nb, d]")
    nb, nq = bank.shape[0], q.shape[0]
    if nb < 1 or nq < 1:
        raise ValueError("range_search needs at least one query and one bank row")
    x = torch.cat([bank.float(), q.float()], 0)
    return range_graph(x, radius2, own=(nb, nb + nq), walk=(0, nb), max_edges=max_edges, splits=splits)


def graph_components(rowptr, col, n):
    """Weakly connected components of a CSR graph on n nodes (an entry (i, j) links i and j whether or not (j, i) is stored) ->
    (label int32 [n] on the device, count): components are numbered by their smallest member."""
    if not rowptr.is_cuda:
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    n = int(n)
    if rowptr.numel() != n + 1:
        raise ValueError(f"rowptr of {rowptr.numel()} entries for {n} nodes")
    rowptr = rowptr.to(torch.int32).contiguous()
    col = col.to(torch.int32).contiguous()
    label = torch.empty(n, dtype=torch.int32, device=rowptr.device)
    count = torch.empty(1, dtype=torch.int32, device=rowptr.device)
    nbytes = components_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=rowptr.device)
    N.call("graph_components", rowptr, col if col.numel() else None, n, col.numel(), label, count, ws, nbytes)
    return label, int(count.item())


def select_keep(group, degree, mode="first"):
    """Which member of every group stays (host code) -> bool [n].  group [n]: group ids; degree [n]: matches per row.
    `first`: the smallest index of the group.  `central`: the member with the most matches, ties to the smaller index."""
    group = np.asarray(group).reshape(-1).astype(np.int64)
    degree = np.asarray(degree).reshape(-1).astype(np.int64)
    if group.shape != degree.shape:
        raise ValueError(f"{group.size} group ids and {degree.size} degrees")
    if mode not in ("first", "central"):
        raise ValueError(f"keep is 'first' or 'central', got {mode!r}")
    n = group.size
    idx = np.arange(n)
    key = np.zeros(n, dtype=np.int64) if mode == "first" else -degree
    order = np.lexsort((idx, key, group))                                    # by group, then best key, then smallest index
    head = np.ones(n, dtype=bool)
    head[1:] = group[order][1:] != group[order][:-1]
    keep = np.zeros(n, dtype=bool)
    keep[order[head]] = True
    return keep


def row_nearest(csr, rows):
    """-> (nearest int64 [rows], d2 fp32 [rows]) on the device: the column of every row's smallest d2 (ties to the smaller
    column), -1 / inf for a row without a match."""
    dev = csr.rowptr.device
    degree = (csr.rowptr[1:] - csr.rowptr[:-1]).long()
    nearest = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    best = torch.full((rows,), float("inf"), dtype=torch.float32, device=dev)
    total = csr.col.numel()
    if total:
        row = torch.repeat_interleave(torch.arange(rows, device=dev), degree)
        best = best.scatter_reduce(0, row, csr.d2, "amin")
        is_min = csr.d2 == best[row]
        pos = torch.arange(total, device=dev)
        first = torch.full((rows,), total, dtype=torch.int64, device=dev).scatter_reduce(0, row[is_min], pos[is_min], "amin")
        has = first < total
        nearest[has] = csr.col[first[has]].long()
    return nearest, best


def near_duplicates(x, threshold=0.98, metric="cosine", keep="first", normalize=True, max_edges=None, splits=0):
    """Groups of near-duplicate rows of x [n, d] (device) -> `Duplicates`.

    metric "cosine": rows are L2-normalised (unless normalize=False says they already are) and two rows match when their cosine
    similarity is at least `threshold`; nearest_sim is that similarity.  metric "l2": `threshold` is the squared L2 radius and
    nearest_sim the nearest squared distance.  group: connected components of the match graph numbered by smallest member -
    single linkage, so A-B and B-C put A and C together.  size: the size of the row's group; degree: its matches; nearest: its
    closest match (-1 for none).  keep: `first` keeps the smallest index of each group, `central` the member with the most
    matches (ties to the smaller index); a row without a match is its own group and is kept."""
    if metric not in ("cosine", "l2"):
        raise ValueError(f"metric is 'cosine' or 'l2', got {metric!r}")
    if keep not in ("first", "central"):
        raise ValueError(f"keep is 'first' or 'central', got {keep!r}")
    x = x.float()
    if metric == "cosine":
        radius2 = cosine_to_radius2(threshold)
        if normalize:
            x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)
    else:
        radius2 = float(threshold)
    n = x.shape[0]
    csr = range_graph(x, radius2, max_edges=max_edges, splits=splits)
    label, n_groups = graph_components(csr.rowptr, csr.col, n)
    group = label.long()
    size = torch.bincount(group, minlength=n_groups)[group]
    degree = (csr.rowptr[1:] - csr.rowptr[:-1]).long()
    nearest, best = row_nearest(csr, n)
    sim = best.double()
    if metric == "cosine":
        sim = 1.0 - 0.5 * sim
    sim = torch.where(nearest >= 0, sim, torch.full_like(sim, float("nan")))
    group_h, degree_h = group.cpu().numpy(), degree.cpu().numpy()
    return Duplicates(group_h, n_groups, size.cpu().numpy(), degree_h, select_keep(group_h, degree_h, keep), nearest.cpu().numpy(),
                      sim.cpu().numpy(), csr)
