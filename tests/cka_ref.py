"""Restatements of centred kernel alignment for the tests, written from the formulas (no code of the reference):

    CKA = HSIC(K, L) / sqrt(HSIC(K, K) HSIC(L, L)),  HSIC(K, L) = sum(HKH * HLH),  H = I - 11^T / n
    linear: K = X X^T;   RBF: d_ij = g_ii + g_jj - 2 g_ij, K = exp(-d / (2 sigma^2)), sigma^2 = median of the non-zero d

* fp64, two independent forms: the explicit HKH products (`hsic_explicit`) and the row-sum identity
  sum(HKH * HLH) = S_KL - (2 / n) sum_i k_i l_i + k l / n^2 (`hsic_identity`);
* an int64 exact version for integer inputs (`exact_linear_terms`, `exact_sigma2`);
* an fp32 emulation of the kernel's arithmetic (fp32 Gram entries and distances, fp64 sums) that tells what error to expect.
"""
import numpy as np


# ---- fp64 ------------------------------------------------------------------------------------------------------------------
def gram(x):
    x = np.asarray(x, dtype=np.float64)
    return x @ x.T


def sqdist(g):
    d = np.diag(g)
    return (d[:, None] + d[None, :]) - 2.0 * g


def median_sigma2(x):
    """median of the non-zero squared distances over the full matrix (every off-diagonal value counts twice)."""
    d = sqdist(gram(x))
    return float(np.median(d[d != 0]))


def rbf(x, sigma2=None):
    d = sqdist(gram(x))
    if sigma2 is None:
        sigma2 = float(np.median(d[d != 0]))
    return np.exp(d * (-0.5 / sigma2))


def hsic_explicit(k, l):
    n = k.shape[0]
    h = np.eye(n) - np.ones((n, n)) / n
    return float(np.sum((h @ k @ h) * (h @ l @ h)))


def hsic_identity(k, l):
    n = k.shape[0]
    ki, li = k.sum(1), l.sum(1)
    return float(np.sum(k * l) - 2.0 / n * np.dot(ki, li) + ki.sum() * li.sum() / (n * n))


def kernels(x, y, kernel="linear", sigma=None):
    if kernel == "linear":
        return gram(x), gram(y)
    s2 = None if sigma is None else float(sigma) ** 2
    return rbf(x, s2), rbf(y, s2)


def terms(x, y, kernel="linear", sigma=None, form=hsic_identity):
    """-> dict(cka, hsic_xy, hsic_xx, hsic_yy) in fp64 on the inputs as given (centre them first for the default Python path:
    the result does not change)."""
    k, l = kernels(x, y, kernel, sigma)
    xy, xx, yy = form(k, l), form(k, k), form(l, l)
    return dict(cka=xy / np.sqrt(xx * yy), hsic_xy=xy, hsic_xx=xx, hsic_yy=yy)


def center(x):
    x = np.asarray(x, dtype=np.float64)
    return x - x.mean(0, keepdims=True)


# ---- int64, exact ----------------------------------------------------------------------------------------------------------
def exact_linear_terms(x, y):
    """integer x [n, p], y [n, q] -> (S_kl, S_kk, S_ll, rowsum_k, rowsum_l) as python ints / int64 arrays."""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    k, l = x @ x.T, y @ y.T
    return int((k * l).sum()), int((k * k).sum()), int((l * l).sum()), k.sum(1), l.sum(1)


def exact_sigma2(x):
    """integer x -> (median of the non-zero integer distances as np.median gives it, M = their count above the diagonal)."""
    x = np.asarray(x, dtype=np.int64)
    g = x @ x.T
    d = np.diag(g)[:, None] + np.diag(g)[None, :] - 2 * g
    upper = d[np.triu_indices(d.shape[0], 1)]
    m = int((upper != 0).sum())
    return (float(np.median(d[d != 0])) if m else float("nan")), m


# ---- fp32 emulation of the kernel's scheme ---------------------------------------------------------------------------------
def emulate_fp32(x, y, kernel="linear", sigma=None):
    """fp32 column-centred inputs, fp32 Gram entries (numpy's fp32 matmul: another summation order than the MFMA chain, the same
    error level), fp32 distances and exponentials, fp64 sums through the identity -> dict like `terms`, plus sigma2_x."""
    def c32(a):
        a = np.asarray(a, dtype=np.float32)
        return (a.astype(np.float64) - a.astype(np.float64).mean(0, keepdims=True)).astype(np.float32)
    x, y = c32(x), c32(y)
    gx, gy = x @ x.T, y @ y.T
    out = {}
    if kernel == "linear":
        k, l = gx.astype(np.float64), gy.astype(np.float64)
    else:
        def rbf32(g, s2):
            dg = np.diag(g)
            d = np.maximum((dg[:, None] + dg[None, :]) - np.float32(2) * g, np.float32(0))
            np.fill_diagonal(d, 0)
            if s2 is None:
                s2 = float(np.median(d[d != 0].astype(np.float64)))
            return np.exp(d * np.float32(-0.5 / s2)).astype(np.float64), s2
        s2 = None if sigma is None else float(sigma) ** 2
        k, out["sigma2_x"] = rbf32(gx, s2)
        l, _ = rbf32(gy, s2)
    xy, xx, yy = hsic_identity(k, l), hsic_identity(k, k), hsic_identity(l, l)
    out.update(cka=xy / np.sqrt(xx * yy), hsic_xy=xy, hsic_xx=xx, hsic_yy=yy)
    return out


# ---- test data -------------------------------------------------------------------------------------------------------------
def correlated(n, p, q, seed, offset=3.0):
    """fp32 X [n, p], Y [n, q]: Y shares a low-rank part with X; both carry a non-zero offset."""
    r = np.random.RandomState(seed)
    z = r.standard_normal((n, 6))
    x = z @ r.standard_normal((6, p)) + 0.7 * r.standard_normal((n, p)) + offset
    y = z @ r.standard_normal((6, q)) + 0.7 * r.standard_normal((n, q)) - 0.5 * offset
    return x.astype(np.float32), y.astype(np.float32)
