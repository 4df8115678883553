"""float64 numpy / scipy restatement of label spreading (Zhou et al. 2004; sklearn's `LabelSpreading`) on a canonical CSR of
W = A + A^T: normalise, spread from F_0 = Y, the dense closed form, assign and confidence; plus the inputs the tests share and
the table of malformed calls.  Shared by tests/test_host_spread.py and tests/test_gpu_spread.py."""
import numpy as np
import scipy.sparse as sp

import pic_ref as P

EPS32 = 2.0 ** -24


def blobs(n, dim, centres, seed, spread=0.15):
    """`pic_ref.blobs` with the membership: -> (x fp32 [n, dim] on the unit sphere, centre of every row)."""
    g = np.random.RandomState(seed)
    c = g.randn(centres, dim)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    member = g.randint(centres, size=n)
    x = c[member] + spread * g.randn(n, dim) / np.sqrt(dim)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), member


def star(n):
    """k = 1 neighbour lists in which node 0 is everybody's neighbour (and node 1 is node 0's): row 0 of W has n - 1 entries.
    -> (idx int64 [n, 1], d2 fp32 [n, 1])"""
    idx = np.zeros((n, 1), dtype=np.int64)
    idx[0, 0] = 1
    d2 = (0.02 + 0.3 * np.random.RandomState(n).rand(n, 1)).astype(np.float32)
    return idx, d2


def csr_from_lists(idx, d2, sigma):
    """Neighbour lists without the self column -> (rowptr, col, w) as `pic_ref.adjacency` builds them."""
    n = idx.shape[0]
    I = np.concatenate([np.arange(n)[:, None], idx], 1)
    D = np.concatenate([np.zeros((n, 1), dtype=np.float32), np.asarray(d2, dtype=np.float32)], 1)
    return P.adjacency(I, D, sigma)


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def normalize(rowptr, col, w):
    """-> (s float64 [nnz] = w_l / sqrt(deg_i deg_j), 0 where the product is 0; deg float64 [n] = row sums in column order)."""
    n = len(rowptr) - 1
    deg = np.zeros(n)
    for i in range(n):
        d = 0.0
        for l in range(rowptr[i], rowptr[i + 1]):
            d += w[l]
        deg[i] = d
    prod = deg[rows_of(rowptr)] * deg[col]
    s = np.zeros(len(col))
    ok = prod > 0
    s[ok] = w[ok] / np.sqrt(prod[ok])
    return s, deg


def matrix(rowptr, col, s):
    n = len(rowptr) - 1
    return sp.csr_matrix((s, col, rowptr), shape=(n, n))


def seeds_dense(rows, cols, n, m, dtype=np.float64):
    Y = np.zeros((n, m), dtype=dtype)
    Y[np.asarray(rows), np.asarray(cols)] = 1
    return Y


def spread(S, Y, alpha, iters, dtype=np.float64):
    """F_0 = Y, `iters` rounds of F <- alpha S F + (1 - alpha) Y in `dtype`."""
    S = S.astype(dtype)
    Y = Y.astype(dtype)
    a, b = dtype(alpha), dtype(1.0 - alpha)
    F = Y.copy()
    for _ in range(iters):
        F = a * (S @ F) + b * Y
    return F


def closed_form(S, Y, alpha):
    """F* = (1 - alpha) (I - alpha S)^-1 Y, dense."""
    n = S.shape[0]
    return (1.0 - alpha) * np.linalg.solve(np.eye(n) - alpha * S.toarray(), Y)


def assign(F, classes):
    """F [n, classes * trials] -> (label int64 [n, trials]: arg-max, ties to the lowest class, -1 when the largest value is <= 0;
    confidence float64 [n, trials] = 1 - H(p) / log(classes), 0 for an unreached row, else 1 when classes == 1;
    margin [n, trials] = largest minus second largest value of the trial's columns, inf when classes == 1)."""
    n, m = F.shape
    trials = m // classes
    G = np.asarray(F, dtype=np.float64)[:, :trials * classes].reshape(n, trials, classes)
    top = G.max(2)
    label = np.where(top > 0, G.argmax(2), -1).astype(np.int64)
    pos = np.where(G > 0, G, 0.0)
    tot = pos.sum(2, keepdims=True)
    p = np.divide(pos, tot, out=np.zeros_like(pos), where=tot > 0)
    h = -(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)).sum(2)
    conf = np.ones((n, trials)) if classes == 1 else 1.0 - h / np.log(classes)
    conf = np.where(top > 0, conf, 0.0)
    if classes == 1:
        margin = np.full((n, trials), np.inf)
    else:
        part = np.sort(G, axis=2)
        margin = part[:, :, -1] - part[:, :, -2]
    return label, conf, margin


def rounding_bound(longest_row, alpha, column_max):
    """First-order rounding bound of the fp32 recurrence per column: one rounding each for s, the product, the scale and the add,
    L - 1 for the sum, amplified by at most 1 / (1 - alpha)."""
    return (longest_row + 3) * EPS32 / (1.0 - alpha) * column_max


def bad_argument_codes(lib, ws):
    """Every malformed call of the four spreading entry points with the code it must return BEFORE any launch; pointers are made-up
    addresses that no kernel may ever see.  ws: `spread_workspace` bytes for (n, m) = (100, 8).  -> [(what, got, want)]"""
    import ctypes
    P_, n, m, cap = 4096, 100, 8, 1000
    b = ctypes.c_long(0)
    bp = ctypes.addressof(b)
    wsz, nz, run, asg = lib.audiossl_spread_workspace, lib.audiossl_spread_normalize, lib.audiossl_spread_run, lib.audiossl_spread_assign
    big = 1 << 40

    def r(rowptr=P_, col=P_, s=P_, n=n, cap=cap, sp_=P_, sc=P_, seeds=3, m=m, alpha=0.99, iters=10, f=P_, w=P_, wb=big):
        return run(rowptr, col, s, n, cap, sp_, sc, seeds, m, alpha, iters, f, w, wb, None)

    return [
        ("workspace null bytes", wsz(n, m, None), -1),
        ("workspace n = 1", wsz(1, m, bp), -1),
        ("workspace m = 0", wsz(n, 0, bp), -1),
        ("workspace m % 4", wsz(n, 6, bp), -1),
        ("workspace m too wide", wsz(n, 16388, bp), -1),
        ("workspace n m >= 2^31", wsz(1 << 20, 2048, bp), -1),
        ("normalize null rowptr", nz(None, P_, P_, n, cap, P_, P_, None), -1),
        ("normalize null col", nz(P_, None, P_, n, cap, P_, P_, None), -1),
        ("normalize null w", nz(P_, P_, None, n, cap, P_, P_, None), -1),
        ("normalize null deg", nz(P_, P_, P_, n, cap, None, P_, None), -1),
        ("normalize null s", nz(P_, P_, P_, n, cap, P_, None, None), -1),
        ("normalize n = 1", nz(P_, P_, P_, 1, cap, P_, P_, None), -1),
        ("normalize negative cap", nz(P_, P_, P_, n, -1, P_, P_, None), -1),
        ("run null rowptr", r(rowptr=None), -1),
        ("run null col", r(col=None), -1),
        ("run null s", r(s=None), -1),
        ("run null seed_ptr", r(sp_=None), -1),
        ("run null seed_col", r(sc=None), -1),
        ("run null f", r(f=None), -1),
        ("run null workspace", r(w=None), -1),
        ("run n = 1", r(n=1), -1),
        ("run m = 0", r(m=0), -1),
        ("run m % 4", r(m=10), -1),
        ("run m too wide", r(m=16388), -1),
        ("run n m >= 2^31", r(n=1 << 20, m=2048), -1),
        ("run alpha = 0", r(alpha=0.0), -1),
        ("run alpha = 1", r(alpha=1.0), -1),
        ("run alpha nan", r(alpha=float("nan")), -1),
        ("run iters = 0", r(iters=0), -1),
        ("run negative seeds", r(seeds=-1), -1),
        ("run negative cap", r(cap=-1), -1),
        ("run short workspace", r(wb=ws - 1), -1),
        ("run misaligned f", r(f=P_ + 4), -3),
        ("run misaligned workspace", r(w=P_ + 8), -3),
        ("assign null f", asg(None, n, m, 4, 2, P_, P_, None), -1),
        ("assign null label", asg(P_, n, m, 4, 2, None, P_, None), -1),
        ("assign null confidence", asg(P_, n, m, 4, 2, P_, None, None), -1),
        ("assign n = 0", asg(P_, 0, m, 4, 2, P_, P_, None), -1),
        ("assign classes = 0", asg(P_, n, m, 0, 2, P_, P_, None), -1),
        ("assign trials = 0", asg(P_, n, m, 4, 0, P_, P_, None), -1),
        ("assign classes trials > ldf", asg(P_, n, m, 4, 3, P_, P_, None), -1),
        ("assign n ldf >= 2^31", asg(P_, 1 << 20, 2048, 4, 2, P_, P_, None), -1),
    ]
