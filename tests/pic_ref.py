"""float64 numpy restatement of every stage of PIC (`extras/decar-v2/clustering.py:118-295`): brute-force neighbour graph, the
affinity matrix W = A + A^T in canonical CSR, the power iteration, the walk to the local maxima, singleton redistribution and
the final numbering.  Shared by tests/test_host_pic.py, tests/test_gpu_graph.py and tests/golden/make_pic_goldens.py."""
import numpy as np

CASES = ((64, 16, 4), (300, 32, 8), (1000, 128, 20))      # (n, dim, centres) of tests/golden/pic_reference.npz
SIGMA, NNN, ALPHA, ITERS = 0.2, 5, 0.001, 200


def blobs(n, dim, centres, seed):
    """RandomState(seed): unit-norm Gaussian centres, centre + 0.15 N(0, I) / sqrt(dim), rows L2-normalised, fp32."""
    g = np.random.RandomState(seed)
    c = g.randn(centres, dim)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[g.randint(centres, size=n)] + 0.15 * g.randn(n, dim) / np.sqrt(dim)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def sq_dists(x):
    """[n, d] -> [n, n] squared distances, float64 (int64 for integer input: exact), by differences (no cancellation)."""
    x = np.asarray(x)
    x = x.astype(np.int64) if np.issubdtype(x.dtype, np.integer) else x.astype(np.float64)
    n = x.shape[0]
    out = np.empty((n, n), dtype=x.dtype)
    for i in range(n):
        diff = x - x[i]
        out[i] = (diff * diff).sum(1)
    return out


def knn_graph(x, k):
    """-> (idx int64 [n, k], d2 [n, k]): the k rows j != i with the smallest distance, order (d2 ascending, j ascending)."""
    dist = sq_dists(x)
    n = dist.shape[0]
    idx = np.empty((n, k), dtype=np.int64)
    d2 = np.empty((n, k), dtype=dist.dtype)
    for i in range(n):
        others = np.delete(np.arange(n), i)
        order = others[np.argsort(dist[i, others], kind="stable")][:k]          # stable: equal distances keep ascending j
        idx[i], d2[i] = order, dist[i, order]
    return idx, d2


def make_graph(x, nnn):
    """faiss's `search(xb, nnn + 1)` layout: column 0 the row itself at distance 0; D in float32 as an index returns it."""
    idx, d2 = knn_graph(x, nnn)
    n = idx.shape[0]
    I = np.concatenate([np.arange(n)[:, None], idx], 1)
    D = np.concatenate([np.zeros((n, 1)), d2], 1).astype(np.float32)
    return I, D


def adjacency(I, D, sigma):
    """-> (rowptr int64 [n + 1], col int64 [nnz], w float64 [nnz]) of W = A + A^T, A_ij = exp(-D_ij / sigma^2) in float64
    from the float32 distance; columns ascending, a mutual pair one entry a_ij + a_ji."""
    I, D = np.asarray(I), np.asarray(D)
    n = I.shape[0]
    rows = [dict() for _ in range(n)]
    a = np.exp(-D[:, 1:].astype(np.float64) / sigma ** 2)
    for i in range(n):
        for t, j in enumerate(I[i, 1:]):
            j = int(j)
            rows[i][j] = rows[i].get(j, 0.0) + a[i, t]
            rows[j][i] = rows[j].get(i, 0.0) + a[i, t]
    rowptr, col, w = [0], [], []
    for r in rows:
        for j in sorted(r):
            col.append(j)
            w.append(r[j])
        rowptr.append(len(col))
    return np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(w, dtype=np.float64)


def power(rowptr, col, w, alpha, iters=ITERS):
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    v = np.full(n, 1.0 / n)
    for _ in range(iters):
        u = alpha * np.bincount(row, weights=w * v[col], minlength=n) + (1.0 - alpha) / n
        v = u / u.sum()
    return v


def maxima(rowptr, col, w, v):
    """`find_maxima_cluster` -> (label int64 [n], margin): margin = the smallest relative gap of any decision - between the
    winning neighbour and the runner-up (0 counts as a contender: "no positive value"), relative to the largest |value| of the row."""
    n = len(rowptr) - 1
    parent = np.arange(n)
    margin = np.inf
    for i in range(n):
        l0, l1 = rowptr[i], rowptr[i + 1]
        val = w[l0:l1] * (v[col[l0:l1]] - v[i])
        cand = np.concatenate([[0.0], val])                      # staying put is worth 0
        order = np.argsort(-cand, kind="stable")
        scale = np.abs(cand).max()
        if len(cand) > 1 and scale > 0:
            margin = min(margin, (cand[order[0]] - cand[order[1]]) / scale)
        best = 0.0
        for l in range(l0, l1):
            if val[l - l0] > best:
                best, parent[i] = val[l - l0], col[l]
    root = parent.copy()
    for _ in range(max(1, int(np.ceil(np.log2(max(n, 2)))))):
        root = root[root]
    ids = np.cumsum(parent == np.arange(n)) - 1
    return ids[root], float(margin)


def singletons(clust, I):
    """One-member clusters join the cluster of their first listed neighbour whose ORIGINAL cluster is not a singleton."""
    clust = np.asarray(clust, dtype=np.int64)
    size = np.bincount(clust)
    out = clust.copy()
    for s in range(len(clust)):
        if size[clust[s]] != 1:
            continue
        for j in np.asarray(I)[s, 1:]:
            if size[clust[j]] != 1:
                out[s] = clust[j]
                break
    return out


def renumber(labels):
    """Clusters numbered by first appearance = by smallest member."""
    seen = {}
    return np.asarray([seen.setdefault(int(c), len(seen)) for c in labels], dtype=np.int64)


def pic(I, D, sigma=SIGMA, alpha=ALPHA, distribute=True):
    """-> (raw labels, final labels renumbered, margin)."""
    rowptr, col, w = adjacency(I, D, sigma)
    v = power(rowptr, col, w, alpha)
    raw, margin = maxima(rowptr, col, w, v)
    final = singletons(raw, I) if distribute else raw
    return raw, renumber(final), margin


def ulp_diff(a, b):
    """|a - b| in units of the spacing of float64 at b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


def bad_argument_codes(lib, graph_ws, pic_ws):
    """Every malformed call of the graph entry points with the code it must return BEFORE any launch (-1 EINVAL, -3 EALIGN);
    pointers are made-up addresses that no kernel may ever see.  graph_ws / pic_ws: workspace sizes for (n, k) = (100, 5).
    -> [(what, got, want)]"""
    P, n, d, k = 4096, 100, 32, 5
    g = lib.audiossl_knn_graph_l2
    b, pw, pa = lib.audiossl_pic_build, lib.audiossl_pic_power, lib.audiossl_pic_assign
    return [
        ("graph ok-shaped but k > n - 1", g(P, 5, d, 5, P, P, P, 1 << 30, None), -1),
        ("graph k > 64", g(P, 1000, d, 65, P, P, P, 1 << 30, None), -1),
        ("graph k = 0", g(P, n, d, 0, P, P, P, 1 << 30, None), -1),
        ("graph d % 4", g(P, n, 30, k, P, P, P, 1 << 30, None), -1),
        ("graph d > 4096", g(P, n, 4100, k, P, P, P, 1 << 30, None), -1),
        ("graph n = 1", g(P, 1, d, 1, P, P, P, 1 << 30, None), -1),
        ("graph n k >= 2^31", g(P, 1 << 26, d, 64, P, P, P, 1 << 40, None), -1),
        ("graph null x", g(None, n, d, k, P, P, P, 1 << 30, None), -1),
        ("graph null idx", g(P, n, d, k, None, P, P, 1 << 30, None), -1),
        ("graph null d2", g(P, n, d, k, P, None, P, 1 << 30, None), -1),
        ("graph null workspace", g(P, n, d, k, P, P, None, 1 << 30, None), -1),
        ("graph short workspace", g(P, n, d, k, P, P, P, graph_ws - 1, None), -1),
        ("graph misaligned x", g(P + 4, n, d, k, P, P, P, 1 << 30, None), -3),
        ("graph misaligned workspace", g(P, n, d, k, P, P, P + 8, 1 << 30, None), -3),
        ("build k > n - 1", b(P, P, 5, 5, 0.2, P, P, P, P, P, 1 << 30, None), -1),
        ("build sigma = 0", b(P, P, n, k, 0.0, P, P, P, P, P, 1 << 30, None), -1),
        ("build sigma nan", b(P, P, n, k, float("nan"), P, P, P, P, P, 1 << 30, None), -1),
        ("build null idx", b(None, P, n, k, 0.2, P, P, P, P, P, 1 << 30, None), -1),
        ("build null nnz", b(P, P, n, k, 0.2, P, P, P, None, P, 1 << 30, None), -1),
        ("build short workspace", b(P, P, n, k, 0.2, P, P, P, P, P, pic_ws - 1, None), -1),
        ("build misaligned workspace", b(P, P, n, k, 0.2, P, P, P, P, P + 4, 1 << 30, None), -3),
        ("power n = 1", pw(P, P, P, 1, 10, 0.001, 200, P, P, 1 << 30, None), -1),
        ("power negative iters", pw(P, P, P, n, 10, 0.001, -1, P, P, 1 << 30, None), -1),
        ("power null v", pw(P, P, P, n, 10, 0.001, 200, None, P, 1 << 30, None), -1),
        ("power short workspace", pw(P, P, P, n, 10, 0.001, 200, P, P, 8, None), -1),
        ("assign null label", pa(P, P, P, P, n, 10, None, P, P, 1 << 30, None), -1),
        ("assign null count", pa(P, P, P, P, n, 10, P, None, P, 1 << 30, None), -1),
        ("assign short workspace", pa(P, P, P, P, n, 10, P, P, P, 8, None), -1),
        ("assign negative cap", pa(P, P, P, P, n, -1, P, P, P, 1 << 30, None), -1),
    ]
