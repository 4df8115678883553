"""HDBSCAN (Campello et al. 2013; `sklearn.cluster.HDBSCAN`) on embeddings: single linkage over every threshold at once, on
mutual-reachability distances.  It finds the number of clusters, copes with clusters of different density and says "this row
belongs nowhere" (label -1) - which k-means, PIC and label spreading cannot.

The heavy stage is on the GPU: core distances from `knn_graph` and the exact minimum spanning tree of the COMPLETE
mutual-reachability graph (csrc/mst.hip: `audiossl_mreach_mst`, Boruvka over Gram tiles, the n x n matrix never stored; a unique
tree under the strict order (w2 bits, min(i, j), max(i, j))).  The rest is host code in numpy on the n - 1 tree edges, in fp64:
tree -> dendrogram (`single_linkage`) -> condensed tree (`condense_tree`) -> excess-of-mass selection (`select_eom`) -> labels and
membership strengths, in sklearn's conventions (`allow_single_cluster=False`, `cluster_selection_epsilon=0`).  `cut_mst` cuts the
same tree at one threshold: the single-linkage groups of `src.evaluation.dedup` at every radius from one tree.
Everything on the device allocates through torch; single GPU.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from src import _native as N

MAX_WIDTH = 4096
MAX_MIN_SAMPLES = 65                                                     # knn_graph lists at most 64 other rows

# u, v int64 [n - 1] (u < v), w2 fp32 [n - 1]: the tree's edges sorted by (w2, u, v); device tensors from the GPU stage
MstEdges = namedtuple("MstEdges", "u v w2")
# merge t joins nodes left[t] and right[t] (a point < n, or n + an earlier merge) at distance dist[t] into a node of size[t] points
Linkage = namedtuple("Linkage", "left right dist size n")
# one row per point or child cluster that leaves / splits off `parent` at `lam`; clusters are numbered from n (the root) upwards,
# a child after its parent
CondensedTree = namedtuple("CondensedTree", "parent child lam child_size n")
# labels int64 [n] (-1: noise), probabilities fp64 [n], n_clusters, mst: the `MstEdges` the labels came from
HdbscanResult = namedtuple("HdbscanResult", "labels probabilities n_clusters mst")


def mst_workspace_bytes(n, splits=0):
    return N.workspace_bytes("mreach_mst_workspace", n, splits)


def _shape(x):
    if x.dim() != 2:
        raise ValueError(f"points are [n, d], got {tuple(x.shape)}")
    n, d = x.shape
    if n < 2:
        raise ValueError(f"a spanning tree needs at least 2 points, got {n}")
    if not 1 <= d <= MAX_WIDTH:
        raise ValueError(f"width must be in [1, {MAX_WIDTH}], got {d}")
    return n, d


def _points(x):
    """Shape checks done: the fp32 [n, d4] device matrix the kernels read."""
    if not x.is_cuda:
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    x = x.float()
    if x.shape[1] % 4:
        x = F.pad(x, (0, 4 - x.shape[1] % 4))
    return x.contiguous()


def _min_samples(min_samples, n):
    min_samples = int(min_samples)
    if not 1 <= min_samples <= MAX_MIN_SAMPLES:
        raise ValueError(f"min_samples must be in [1, {MAX_MIN_SAMPLES}], got {min_samples}")
    if min_samples > n:
        raise ValueError(f"min_samples = {min_samples} needs at least that many points, got {n}")
    return min_samples


def core_distances2(x, min_samples):
    """x [n, d] (device) -> fp32 [n]: the squared distance to the `min_samples`-th nearest point COUNTING THE POINT ITSELF
    (sklearn's convention): column min_samples - 2 of `knn_graph`'s d2, zeros for min_samples == 1."""
    from src.evaluation.graph import knn_graph
    n, _ = _shape(x)
    min_samples = _min_samples(min_samples, n)
    x = _points(x)
    if min_samples == 1:
        return torch.zeros(n, dtype=torch.float32, device=x.device)
    return knn_graph(x, min_samples - 1)[1][:, min_samples - 2].contiguous()


def mutual_reachability_mst(x, min_samples=1, splits=0, return_rounds=False):
    """x [n, d] (device) -> `MstEdges`: the n - 1 edges of the minimum spanning tree of the complete graph with weights
    w2_ij = max(|x_i - x_j|^2, core2_i, core2_j), sorted by (w2, u, v).  The tree is unique (strict order on (w2 bits, u, v)) and
    does not depend on `splits`.  d is zero-padded to a multiple of 4.  return_rounds: also the Boruvka rounds that did work."""
    n, _ = _shape(x)
    splits = int(splits)
    if not 0 <= splits <= 64:
        raise ValueError(f"splits must be in [0, 64], got {splits}")
    min_samples = _min_samples(min_samples, n)
    x = _points(x)
    d = x.shape[1]
    core2 = None if min_samples == 1 else core_distances2(x, min_samples)
    eu = torch.empty(n - 1, dtype=torch.int32, device=x.device)
    ev = torch.empty(n - 1, dtype=torch.int32, device=x.device)
    ew2 = torch.empty(n - 1, dtype=torch.float32, device=x.device)
    rounds = torch.zeros(1, dtype=torch.int32, device=x.device)
    nbytes = mst_workspace_bytes(n, splits)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    N.call("mreach_mst", x, n, d, core2, splits, eu, ev, ew2, rounds, ws, nbytes)
    order = torch.arange(n - 1, device=x.device)
    for key in (ev, eu, ew2):                                                # stable sorts, least significant key first
        order = order[torch.sort(key[order], stable=True)[1]]
    mst = MstEdges(eu[order].long(), ev[order].long(), ew2[order])
    return (mst, int(rounds.item())) if return_rounds else mst


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=dtype)


def _edges(u, v, w, n):
    n = int(n)
    u, v, w = _host(u, np.int64), _host(v, np.int64), _host(w, np.float64)
    if n < 1 or not (len(u) == len(v) == len(w) == n - 1):
        raise ValueError(f"a spanning tree on {n} points has {n - 1} edges, got {len(u)}, {len(v)} and {len(w)}")
    if n > 1 and (min(u.min(), v.min()) < 0 or max(u.max(), v.max()) >= n):
        raise ValueError(f"edge ends must lie in [0, {n})")
    if not (w >= 0).all():                                                   # NaN fails the comparison
        raise ValueError("edge weights must be >= 0")
    return u, v, w, n


def _find(parent, a):
    root = a
    while parent[root] != root:
        root = parent[root]
    while parent[a] != root:
        parent[a], a = root, parent[a]
    return root


def _renumber(label):
    """Ids >= 0 -> 0 .. C - 1 in the order of each group's smallest member (pic_assign's convention); -1 stays."""
    label = np.asarray(label, dtype=np.int64)
    out = np.full(len(label), -1, dtype=np.int64)
    keep = np.flatnonzero(label >= 0)
    if len(keep):
        _, first, inverse = np.unique(label[keep], return_index=True, return_inverse=True)
        rank = np.empty(len(first), dtype=np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(len(first))
        out[keep] = rank[inverse.reshape(-1)]
    return out


def single_linkage(u, v, w, n):
    """The n - 1 edges of a spanning tree with distances w (NOT squared) -> `Linkage`: the edges taken in the order (w, u, v),
    each merging the two nodes its ends are in."""
    u, v, w, n = _edges(u, v, w, n)
    order = np.lexsort((v, u, w))
    parent = list(range(2 * n - 1))
    left, right = np.empty(n - 1, dtype=np.int64), np.empty(n - 1, dtype=np.int64)
    dist, size = np.empty(n - 1, dtype=np.float64), np.empty(n - 1, dtype=np.int64)
    sizes = [1] * n + [0] * (n - 1)
    for t, e in enumerate(order.tolist()):
        a, b = _find(parent, int(u[e])), _find(parent, int(v[e]))
        if a == b:
            raise ValueError("the edges contain a cycle: not a spanning tree")
        node = n + t
        parent[a] = parent[b] = node
        sizes[node] = sizes[a] + sizes[b]
        left[t], right[t], dist[t], size[t] = a, b, w[e], sizes[node]
    return Linkage(left, right, dist, size, n)


def condense_tree(linkage, min_cluster_size):
    """`Linkage` -> `CondensedTree`.  Walking down from the root (cluster n), lambda = 1 / distance (inf at distance 0): a merge
    whose two sides both have >= min_cluster_size points is a true split into two new clusters; otherwise the points of every
    side smaller than that fall out of the parent at that lambda and the larger side, if any, IS the parent further down."""
    n = linkage.n
    m = int(min_cluster_size)
    if m < 2:
        raise ValueError(f"min_cluster_size must be at least 2, got {m}")
    left, right = linkage.left.tolist(), linkage.right.tolist()
    dist = linkage.dist.tolist()
    size = [1] * n + linkage.size.tolist()
    # the leaves under a node are a contiguous run of the depth-first leaf order
    first, leaves = [0] * (2 * n - 1), []
    stack = [2 * n - 2]
    while stack:
        node = stack.pop()
        first[node] = len(leaves)
        if node < n:
            leaves.append(node)
        else:
            stack.append(right[node - n])                                    # the left side is popped first, then the right one
            stack.append(left[node - n])
    parents, children, lams, csizes = [], [], [], []
    next_label = n + 1
    stack = [(2 * n - 2, n)] if n > 1 else []
    while stack:
        node, cluster = stack.pop()
        a, b, dd = left[node - n], right[node - n], dist[node - n]
        lam = 1.0 / dd if dd > 0.0 else np.inf
        if size[a] >= m and size[b] >= m:
            for side in (a, b):
                parents.append(cluster); children.append(next_label); lams.append(lam); csizes.append(size[side])
                stack.append((side, next_label))
                next_label += 1
            continue
        for side in (a, b):
            if size[side] >= m:
                stack.append((side, cluster))
            else:
                for p in leaves[first[side]:first[side] + size[side]]:
                    parents.append(cluster); children.append(p); lams.append(lam); csizes.append(1)
    return CondensedTree(np.asarray(parents, dtype=np.int64), np.asarray(children, dtype=np.int64),
                         np.asarray(lams, dtype=np.float64), np.asarray(csizes, dtype=np.int64), n)


def cluster_stabilities(tree):
    """-> fp64 [clusters]: for cluster n + c the sum over the points that were ever in it of (lambda at which the point left it,
    on its own or inside a child cluster) - (lambda at which the cluster was born); the root is born at 0.  A term inf - inf (a
    cluster of identical points) counts as 0."""
    n = tree.n
    count = int(max(tree.parent.max(initial=n), tree.child.max(initial=n))) - n + 1
    birth = np.zeros(count)
    is_cluster = tree.child >= n
    birth[tree.child[is_cluster] - n] = tree.lam[is_cluster]
    with np.errstate(invalid="ignore"):
        term = (tree.lam - birth[tree.parent - n]) * tree.child_size
    term[np.isnan(term)] = 0.0
    stability = np.zeros(count)
    np.add.at(stability, tree.parent - n, term)
    return stability


def select_eom(tree):
    """Excess of mass with the root excluded -> sorted ids of the selected clusters.  Children first: a cluster stays selected
    unless its child clusters' (propagated) stabilities sum to strictly more than its own."""
    n = tree.n
    stability = cluster_stabilities(tree)
    count = len(stability)
    kids = [[] for _ in range(count)]
    is_cluster = tree.child >= n
    for p, c in zip((tree.parent[is_cluster] - n).tolist(), (tree.child[is_cluster] - n).tolist()):
        kids[p].append(c)
    selected = np.ones(count, dtype=bool)
    selected[0] = False                                                      # the root: allow_single_cluster=False
    for c in range(count - 1, 0, -1):                                        # a child's id is larger than its parent's
        below = sum(stability[k] for k in kids[c])
        if below > stability[c]:
            selected[c] = False
            stability[c] = below
        else:
            stack = list(kids[c])
            while stack:
                k = stack.pop()
                selected[k] = False
                stack.extend(kids[k])
    return np.flatnonzero(selected) + n


def label_points(tree, selected):
    """-> (labels int64 [n] numbered by smallest member, -1 = in no selected cluster; probabilities fp64 [n]).  A point belongs to
    the selected cluster at or above the cluster it fell out of.  Probability (sklearn's `_get_probabilities`): min(lambda_p,
    death_c) / death_c, death_c = the largest lambda among the condensed-tree rows whose parent is c ITSELF; 1 where death_c is 0
    or lambda_p is infinite."""
    n = tree.n
    count = int(max(tree.parent.max(initial=n), tree.child.max(initial=n))) - n + 1
    chosen = np.zeros(count, dtype=bool)
    chosen[np.asarray(selected, dtype=np.int64) - n] = True
    up = np.zeros(count, dtype=np.int64)
    is_cluster = tree.child >= n
    up[tree.child[is_cluster] - n] = tree.parent[is_cluster] - n
    owner = np.full(count, -1, dtype=np.int64)                               # the selected cluster at or above, -1 for none
    for c in range(count):                                                   # a parent's id is smaller than its child's
        owner[c] = c if chosen[c] else (owner[up[c]] if c else -1)
    death = np.zeros(count)
    np.maximum.at(death, tree.parent - n, tree.lam)
    raw = np.full(n, -1, dtype=np.int64)
    prob = np.zeros(n)
    pt = ~is_cluster
    points, lam, own = tree.child[pt], tree.lam[pt], owner[tree.parent[pt] - n]
    raw[points] = own
    has = own >= 0
    dmax = death[np.where(has, own, 0)]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.minimum(lam, dmax) / dmax
    full = (dmax == 0.0) | np.isinf(lam)
    prob[points] = np.where(has, np.where(full, 1.0, ratio), 0.0)
    return _renumber(raw), prob


def cut_mst(mst, n, radius2):
    """`MstEdges` (or any (u, v, w2) of a spanning tree) -> int64 [n]: the components of the edges with w2 <= radius2, numbered by
    smallest member.  With min_samples = 1 these are the single-linkage groups of `dedup.near_duplicates` at that radius."""
    u, v, w2, n = _edges(mst[0], mst[1], mst[2], n)
    radius2 = float(np.float32(radius2))
    if not radius2 >= 0.0:
        raise ValueError(f"radius2 must be >= 0, got {radius2}")
    parent = list(range(n))
    for e in np.flatnonzero(w2 <= radius2).tolist():
        a, b = _find(parent, int(u[e])), _find(parent, int(v[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return _renumber(np.asarray([_find(parent, i) for i in range(n)], dtype=np.int64))


def hdbscan_from_mst(u, v, w, n, min_cluster_size):
    """The host stage alone: tree edges with distances w (not squared) -> (labels, probabilities, n_clusters)."""
    tree = condense_tree(single_linkage(u, v, w, n), min_cluster_size)
    labels, prob = label_points(tree, select_eom(tree))
    return labels, prob, int(labels.max(initial=-1)) + 1


def hdbscan(x, min_cluster_size=5, min_samples=None):
    """x [n, d] (device) -> `HdbscanResult`: sklearn's `HDBSCAN(min_cluster_size, min_samples)` with its defaults otherwise.
    min_samples defaults to min_cluster_size.  Labels are numbered by smallest member, noise is -1."""
    min_cluster_size = int(min_cluster_size)
    if min_cluster_size < 2:
        raise ValueError(f"min_cluster_size must be at least 2, got {min_cluster_size}")
    min_samples = min_cluster_size if min_samples is None else min_samples
    mst = mutual_reachability_mst(x, min_samples)
    n = x.shape[0]
    w = np.sqrt(mst.w2.double().cpu().numpy())
    labels, prob, count = hdbscan_from_mst(mst.u, mst.v, w, n, min_cluster_size)
    return HdbscanResult(labels, prob, count, mst)
