"""float64 restatement of sklearn's `silhouette_samples` (Euclidean), the cases and the bad-argument table shared by
tests/test_host_silhouette.py (CPU: the restatement against sklearn itself) and tests/test_gpu_silhouette.py (the kernel against the
restatement).

The restatement also returns what the GPU test's tolerance is made of: a, b per row and the smallest non-zero / the largest distance."""
import ctypes
import functools
from collections import namedtuple

import numpy as np

Ref = namedtuple("Ref", "s a b d_min d_max")


def silhouette(x, labels):
    """x [n, d], labels [n] (any integers) -> Ref: s, a (0 for a one-member cluster), b float64 [n], d_min (smallest non-zero
    distance), d_max.  Distances from the float64 Gram matrix, as sklearn's `euclidean_distances` forms them; (i, i) is 0."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    _, inv, counts = np.unique(np.asarray(labels), return_inverse=True, return_counts=True)
    K = len(counts)
    assert 2 <= K <= n - 1
    onehot = np.zeros((n, K))
    onehot[np.arange(n), inv] = 1.0
    sq = (x * x).sum(1)
    sums = np.empty((n, K))
    d_min, d_max = np.inf, 0.0
    for lo in range(0, n, 1024):
        hi = min(lo + 1024, n)
        dist = np.sqrt(np.maximum(sq[lo:hi, None] + sq[None, :] - 2.0 * (x[lo:hi] @ x.T), 0.0))
        dist[np.arange(hi - lo), np.arange(lo, hi)] = 0.0
        sums[lo:hi] = dist @ onehot
        d_max = max(d_max, float(dist.max()))
        if (dist > 0).any():
            d_min = min(d_min, float(dist[dist > 0].min()))
    rows = np.arange(n)
    size = counts[inv]
    a = np.where(size > 1, sums[rows, inv] / np.maximum(size - 1, 1), 0.0)
    other = sums / counts[None, :]
    other[rows, inv] = np.inf
    b = other.min(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.nan_to_num((b - a) / np.maximum(a, b))
    s[size == 1] = 0.0
    return Ref(s, a, b, d_min, d_max)


def _randn(n, d, seed):
    return np.random.RandomState(seed).randn(n, d).astype(np.float32)


def _case_a():
    g = np.random.RandomState(101)
    return _randn(333, 19, 1), 13 * g.randint(7, size=333) - 100           # width padded to 20; label values sparse and negative


def _case_b():
    """After the sort the boundaries sit on the tile edges 128 and 384, inside the last tile (448) and before a trailing singleton."""
    labels = np.repeat(np.arange(5), [128, 256, 64, 63, 1])
    return _randn(512, 32, 2), labels[np.random.RandomState(102).permutation(512)]


def _case_c():
    """K = n - 1: 128 one-member clusters and one pair - every run of every tile is one column long but one."""
    labels = np.concatenate([np.arange(129), [40]])
    return _randn(130, 8, 3), labels[np.random.RandomState(103).permutation(130)]


def _case_d():
    labels = np.zeros(200, dtype=np.int64)
    labels[77] = 1                                                         # K = 2: one singleton and the rest
    return _randn(200, 36, 4), labels


def _case_f():
    """Unit rows around 37 centres, labelled by the nearest centre: the labeler's kind of input, 32 walked tiles, 64 row blocks."""
    g = np.random.RandomState(105)
    centres = g.randn(37, 128)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[g.randint(37, size=4096)] + 0.1 * g.randn(4096, 128)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return x, (x.astype(np.float64) @ centres.T).argmax(1)


def _case_g():
    return _randn(257, 516, 6), np.random.RandomState(106).randint(3, size=257)      # 17 feature chunks, the last one short


def _case_h():
    return _randn(3, 4, 7), np.array([0, 0, 1])


def _case_e():
    """Integer entries in -2..2 (every product, norm and squared distance exact in fp32): rows 0..39 = u in cluster 0, rows 40..69 = v
    in cluster 1, rows 70..94 = u again in cluster 2, 50 random rows in cluster 3; then permuted.  A u row has a = 0 and b = 0 (its
    copies in the other cluster): s = 0 / 0 -> exactly 0.  A v row has a = 0 and b > 0: s exactly 1."""
    g = np.random.RandomState(108)
    u = np.array([1, -2, 0, 2, 1, 1, -1, 0, 2, -2, 0, 1])
    v = np.array([0, -2, 1, 2, -1, 1, -1, 0, 2, 2, 0, 1])
    x = np.concatenate([np.tile(u, (40, 1)), np.tile(v, (30, 1)), np.tile(u, (25, 1)), g.randint(-2, 3, size=(50, 12))])
    labels = np.repeat(np.arange(4), [40, 30, 25, 50])
    p = g.permutation(145)
    return x[p].astype(np.float32), labels[p]


CASES = {"A": _case_a, "B": _case_b, "C": _case_c, "D": _case_d, "F": _case_f, "G": _case_g, "H": _case_h, "E": _case_e}


@functools.lru_cache(maxsize=None)
def _case(name):
    x, labels = CASES[name]()
    labels = np.asarray(labels, dtype=np.int64)
    ref = silhouette(x, labels)
    for arr in ref[:3]:
        arr.setflags(write=False)
    return x, labels, ref


def case(name):
    """-> (x float32 [n, d], labels int64 [n], Ref): the reference is computed once, shared and read-only; x and labels are the
    caller's own copies."""
    x, labels, ref = _case(name)
    return x.copy(), labels.copy(), ref


def bad_argument_codes(lib, ws_bytes):
    """Every malformed call of `audiossl_silhouette` with the code it must return BEFORE any launch (-1 EINVAL, -3 EALIGN).  Device
    pointers are made-up addresses that no kernel may ever see; seg_host is a real host array wherever the entry point gets as far
    as reading it.  ws_bytes: the workspace size for n = 100.  -> [(what, got, want)]"""
    P, n, d, K = 4096, 100, 32, 3
    f = lib.audiossl_silhouette

    def host(*offsets):
        arr = (ctypes.c_int * len(offsets))(*offsets)
        return arr, ctypes.addressof(arr)

    keep, good = host(0, 40, 70, 100)
    tables = [("seg_host[0] != 0", host(1, 40, 70, 100)), ("seg_host[K] != n", host(0, 40, 70, 99)),
              ("an empty segment", host(0, 40, 40, 100)), ("a decreasing segment", host(0, 70, 40, 100)),
              ("seg_host[K] beyond n", host(0, 40, 70, 101))]
    big = 1 << 30
    out = [
        ("null xs", f(None, n, d, P, good, K, P, P, big, None), -1),
        ("null seg", f(P, n, d, None, good, K, P, P, big, None), -1),
        ("null seg_host", f(P, n, d, P, None, K, P, P, big, None), -1),
        ("null s", f(P, n, d, P, good, K, None, P, big, None), -1),
        ("null workspace", f(P, n, d, P, good, K, P, None, big, None), -1),
        ("n = 2", f(P, 2, d, P, P, 2, P, P, big, None), -1),
        ("n = 0", f(P, 0, d, P, P, 2, P, P, big, None), -1),
        ("d % 4", f(P, n, 30, P, P, K, P, P, big, None), -1),
        ("d = 0", f(P, n, 0, P, P, K, P, P, big, None), -1),
        ("d > 4096", f(P, n, 4100, P, P, K, P, P, big, None), -1),
        ("K = 1", f(P, n, d, P, P, 1, P, P, big, None), -1),
        ("K = n", f(P, n, d, P, P, n, P, P, big, None), -1),
        ("K < 0", f(P, n, d, P, P, -3, P, P, big, None), -1),
        ("short workspace", f(P, n, d, P, P, K, P, P, ws_bytes - 1, None), -1),
        ("misaligned xs", f(P + 4, n, d, P, good, K, P, P, big, None), -3),
        ("misaligned workspace", f(P, n, d, P, good, K, P, P + 8, big, None), -3),
    ]
    out += [(what, f(P, n, d, P, addr, K, P, P, big, None), -1) for what, (_, addr) in tables]
    del keep
    return out
