"""float64 restatement of the radius graph and its components (csrc/range.hip), the inputs of tests/test_gpu_dedup.py and the
malformed calls every entry must refuse.  Nothing here needs a GPU.

Radius graph: d2 in float64 from the float32 rows, `d2 <= r2` minus the diagonal (i == j leaves by INDEX: a repeated row is a
match).  Components: scipy's `connected_components`, renumbered by smallest member.  tests/test_host_dedup.py pins the graph to
sklearn's `radius_neighbors_graph` on one case."""
import functools

import numpy as np

EPS24 = 2.0 ** -24

GRID_N, GRID_D = 333, 20
GRID_RADII = (0.5, 3.5, 6.5, 1e9)
# r2 -> (edges, max degree, components, largest component)
GRID_FACTS = {0.5: (17, 3, 322, 4), 3.5: (1170, 34, 88, 37), 6.5: (3813, 40, 14, 41), 1e9: (55278, 332, 1, 333)}

# (n, d, G, noise, seed) -> (edges, max degree, components) at tau = 0.9
REAL_CASES = ((389, 36, 40, 0.25, 0), (389, 36, 40, 0.25, 2), (517, 132, 60, 0.3, 3))
REAL_FACTS = ((1784, 19, 42), (1820, 15, 40), (1887, 14, 61))
REAL_TAU = 0.9


@functools.lru_cache(maxsize=None)
def grid():
    """333 x 20 small integers around 9 centres: every product, sum and difference is exact in fp32 (|x|^2 <= 179)."""
    g = np.random.default_rng(7)
    n, d = GRID_N, GRID_D
    base = g.integers(-4, 5, (9, d))
    a = g.integers(0, 9, n)
    x = base[a] + (g.random((n, d)) < 0.15) * g.choice([-1, 1], (n, d))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def real(case):
    """Unit rows around G centres, the last five rows repeat the first five."""
    n, d, G, noise, seed = REAL_CASES[case]
    g = np.random.default_rng(seed)
    c = g.standard_normal((G, d))
    a = g.integers(0, G, n)
    x = c[a] + noise * g.standard_normal((n, d))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    x[n - 5:] = x[:5]
    x.setflags(write=False)
    return x


def real_r2():
    return float(np.float32(2.0 - 2.0 * REAL_TAU))


@functools.lru_cache(maxsize=None)
def path():
    """1,000 points on a line under shuffled ids: one component of diameter 999 at r2 = 1.5."""
    p = np.random.default_rng(11).permutation(1000)
    x = np.zeros((1000, 4), dtype=np.float32)
    x[:, 0] = p
    x.setflags(write=False)
    return x


def sq_dists(x, rows=None, cols=None):
    """float64 |x_i - x_j|^2 by differences (no cancellation), i in rows = (lo, hi), j in cols = (lo, hi)."""
    x = np.asarray(x, dtype=np.float64)
    r0, r1 = rows or (0, len(x))
    c0, c1 = cols or (0, len(x))
    out = np.empty((r1 - r0, c1 - c0))
    for i in range(r0, r1):
        out[i - r0] = ((x[c0:c1] - x[i]) ** 2).sum(1)
    return out


def radius_graph(x, r2, own=None, walk=None):
    """-> (rowptr int64 [rows + 1], col int64 absolute, d2 float64): owned rows own = (lo, hi) against walked rows walk = (lo, hi),
    `d2 <= r2` minus i == j, columns ascending."""
    n = len(x)
    own, walk = own or (0, n), walk or (0, n)
    dist = sq_dists(x, own, walk)
    hit = dist <= float(r2)
    ii = np.arange(own[0], own[1])[:, None]
    jj = np.arange(walk[0], walk[1])[None, :]
    hit &= ii != jj
    rowptr = np.zeros(own[1] - own[0] + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(hit.sum(1))
    r, c = np.nonzero(hit)                                                    # row-major: columns ascend inside a row
    return rowptr, c.astype(np.int64) + walk[0], dist[r, c]


def bands(x, rowptr, col, own_lo=0):
    """The worst-case rounding bound of the fp32 chain for every stored pair: 2 (d + 3) 2^-24 (n_i + n_j)."""
    x = np.asarray(x, dtype=np.float64)
    nrm = (x ** 2).sum(1)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)) + own_lo
    return 2.0 * (x.shape[1] + 3) * EPS24 * (nrm[rows] + nrm[col])


def smallest_band_gap(x, r2):
    """min over all pairs i != j of |d2_ij - r2| / band_ij: above 1, no pair's membership depends on fp32 rounding."""
    x64 = np.asarray(x, dtype=np.float64)
    nrm = (x64 ** 2).sum(1)
    dist = sq_dists(x)
    band = 2.0 * (x.shape[1] + 3) * EPS24 * (nrm[:, None] + nrm[None, :])
    gap = np.abs(dist - float(r2)) / band
    np.fill_diagonal(gap, np.inf)
    return float(gap.min())


def renumber(label):
    """Component ids -> ids in the order of each component's smallest member."""
    label = np.asarray(label)
    _, first, inverse = np.unique(label, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inverse.reshape(-1)]


def components(rowptr, col, n):
    """-> (label int64 [n] numbered by smallest member, count): weakly connected components by scipy."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    m = csr_matrix((np.ones(len(col), dtype=np.int8), col, rowptr), shape=(n, n))
    count, label = connected_components(m, directed=True, connection="weak")
    return renumber(label), int(count)


def nearest(rowptr, col, d2):
    """-> (column of every row's smallest d2, ties to the smaller column, -1 for none; that d2, inf for none)."""
    rows = len(rowptr) - 1
    near, best = np.full(rows, -1, dtype=np.int64), np.full(rows, np.inf)
    for i in range(rows):
        lo, hi = rowptr[i], rowptr[i + 1]
        if hi > lo:
            t = lo + int(np.argmin(d2[lo:hi]))                                # the first of equal minima: the smaller column
            near[i], best[i] = col[t], d2[t]
    return near, best


def keep_first(group):
    group = np.asarray(group)
    keep = np.zeros(len(group), dtype=bool)
    seen = set()
    for i, g in enumerate(group.tolist()):
        if g not in seen:
            seen.add(g)
            keep[i] = True
    return keep


def keep_central(group, degree):
    group, degree = np.asarray(group), np.asarray(degree)
    keep = np.zeros(len(group), dtype=bool)
    best = {}
    for i, (g, dg) in enumerate(zip(group.tolist(), degree.tolist())):
        if g not in best or dg > best[g][0]:                                  # strictly more matches: ties stay with the smaller index
            best[g] = (dg, i)
    for _, i in best.values():
        keep[i] = True
    return keep


def star(n=600, both=True):
    """Hub 0 with n - 1 leaves -> (rowptr, col); both: the leaves list the hub too, else only the hub row is stored."""
    deg = np.zeros(n, dtype=np.int64)
    deg[0] = n - 1
    cols = [np.arange(1, n)]
    if both:
        deg[1:] = 1
        cols.append(np.zeros(n - 1, dtype=np.int64))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    return rowptr, np.concatenate(cols)


def bad_argument_codes(lib, ws_bytes, cc_bytes):
    """Every malformed call with the code it must return BEFORE any launch (-1 EINVAL, -3 EALIGN); pointers are made-up addresses
    that no kernel may ever see.  ws_bytes: range_workspace(100, 100, 0); cc_bytes: graph_components_workspace(100).
    -> [(what, got, want)]"""
    import ctypes
    P, n, d, r2, BIG = 4096, 100, 32, 0.5, 1 << 30
    c, f, g = lib.audiossl_range_count, lib.audiossl_range_fill, lib.audiossl_graph_components
    b = ctypes.c_long(0)
    w, gw = lib.audiossl_range_workspace, lib.audiossl_graph_components_workspace
    return [
        ("count null x", c(None, n, d, 0, n, 0, n, r2, 0, P, P, P, BIG, None), -1),
        ("count null rowptr", c(P, n, d, 0, n, 0, n, r2, 0, None, P, P, BIG, None), -1),
        ("count null total", c(P, n, d, 0, n, 0, n, r2, 0, P, None, P, BIG, None), -1),
        ("count null workspace", c(P, n, d, 0, n, 0, n, r2, 0, P, P, None, BIG, None), -1),
        ("count d % 4", c(P, n, 30, 0, n, 0, n, r2, 0, P, P, P, BIG, None), -1),
        ("count d = 0", c(P, n, 0, 0, n, 0, n, r2, 0, P, P, P, BIG, None), -1),
        ("count d > 4096", c(P, n, 4100, 0, n, 0, n, r2, 0, P, P, P, BIG, None), -1),
        ("count empty owned range", c(P, n, d, 40, 40, 0, n, r2, 0, P, P, P, BIG, None), -1),
        ("count empty walked range", c(P, n, d, 0, n, 7, 7, r2, 0, P, P, P, BIG, None), -1),
        ("count reversed range", c(P, n, d, 50, 40, 0, n, r2, 0, P, P, P, BIG, None), -1),
        ("count owned past n", c(P, n, d, 0, n + 1, 0, n, r2, 0, P, P, P, BIG, None), -1),
        ("count negative walk_lo", c(P, n, d, 0, n, -1, n, r2, 0, P, P, P, BIG, None), -1),
        ("count n = 0", c(P, 0, d, 0, 0, 0, 0, r2, 0, P, P, P, BIG, None), -1),
        ("count negative r2", c(P, n, d, 0, n, 0, n, -0.5, 0, P, P, P, BIG, None), -1),
        ("count r2 inf", c(P, n, d, 0, n, 0, n, float("inf"), 0, P, P, P, BIG, None), -1),
        ("count r2 nan", c(P, n, d, 0, n, 0, n, float("nan"), 0, P, P, P, BIG, None), -1),
        ("count splits 65", c(P, n, d, 0, n, 0, n, r2, 65, P, P, P, BIG, None), -1),
        ("count splits -1", c(P, n, d, 0, n, 0, n, r2, -1, P, P, P, BIG, None), -1),
        ("count short workspace", c(P, n, d, 0, n, 0, n, r2, 0, P, P, P, ws_bytes - 1, None), -1),
        ("count misaligned x", c(P + 4, n, d, 0, n, 0, n, r2, 0, P, P, P, BIG, None), -3),
        ("count misaligned workspace", c(P, n, d, 0, n, 0, n, r2, 0, P, P, P + 8, BIG, None), -3),
        ("fill null x", f(None, n, d, 0, n, 0, n, r2, 0, P, 10, P, P, 10, P, BIG, None), -1),
        ("fill null rowptr", f(P, n, d, 0, n, 0, n, r2, 0, None, 10, P, P, 10, P, BIG, None), -1),
        ("fill null col", f(P, n, d, 0, n, 0, n, r2, 0, P, 10, None, P, 10, P, BIG, None), -1),
        ("fill null d2", f(P, n, d, 0, n, 0, n, r2, 0, P, 10, P, None, 10, P, BIG, None), -1),
        ("fill null workspace", f(P, n, d, 0, n, 0, n, r2, 0, P, 10, P, P, 10, None, BIG, None), -1),
        ("fill cap < total", f(P, n, d, 0, n, 0, n, r2, 0, P, 10, P, P, 9, P, BIG, None), -1),
        ("fill negative total", f(P, n, d, 0, n, 0, n, r2, 0, P, -1, P, P, 9, P, BIG, None), -1),
        ("fill total = 2^31", f(P, n, d, 0, n, 0, n, r2, 0, P, 1 << 31, P, P, 1 << 32, P, BIG, None), -1),
        ("fill d % 4", f(P, n, 30, 0, n, 0, n, r2, 0, P, 10, P, P, 10, P, BIG, None), -1),
        ("fill empty range", f(P, n, d, 3, 3, 0, n, r2, 0, P, 10, P, P, 10, P, BIG, None), -1),
        ("fill r2 nan", f(P, n, d, 0, n, 0, n, float("nan"), 0, P, 10, P, P, 10, P, BIG, None), -1),
        ("fill short workspace", f(P, n, d, 0, n, 0, n, r2, 0, P, 10, P, P, 10, P, ws_bytes - 1, None), -1),
        ("fill misaligned workspace", f(P, n, d, 0, n, 0, n, r2, 0, P, 10, P, P, 10, P + 4, BIG, None), -3),
        ("components null rowptr", g(None, P, n, 10, P, P, P, BIG, None), -1),
        ("components null col", g(P, None, n, 10, P, P, P, BIG, None), -1),
        ("components null label", g(P, P, n, 10, None, P, P, BIG, None), -1),
        ("components null count", g(P, P, n, 10, P, None, P, BIG, None), -1),
        ("components null workspace", g(P, P, n, 10, P, P, None, BIG, None), -1),
        ("components n = 0", g(P, P, 0, 10, P, P, P, BIG, None), -1),
        ("components negative cap", g(P, P, n, -1, P, P, P, BIG, None), -1),
        ("components short workspace", g(P, P, n, 10, P, P, P, cc_bytes - 1, None), -1),
        ("components misaligned workspace", g(P, P, n, 10, P, P, P + 4, BIG, None), -3),
        ("workspace null bytes", w(n, n, 0, None), -1),
        ("workspace rows > n", w(n, n + 1, 0, ctypes.addressof(b)), -1),
        ("workspace rows = 0", w(n, 0, 0, ctypes.addressof(b)), -1),
        ("workspace splits 65", w(n, n, 65, ctypes.addressof(b)), -1),
        ("components workspace null bytes", gw(n, None), -1),
        ("components workspace n = 0", gw(0, ctypes.addressof(b)), -1),
    ]
