"""Centred kernel alignment (CKA) between two sets of features of the same clips - `linear_CKA` / `kernel_CKA` of the
reference's `extras/CKA.py`, the tool behind the "which layer learned what" figures of the DeLoRes and UnFuSeD papers.

    CKA(X, Y) = HSIC(K, L) / sqrt(HSIC(K, K) HSIC(L, L)),   HSIC(K, L) = sum(HKH * HLH),   H = I - 11^T / n

with K, L the Gram matrices of X [n, p] and Y [n, q] (linear: X X^T; RBF: exp(-d_ij / (2 sigma^2)), d_ij the squared distances,
sigma^2 = the median non-zero distance per matrix when no sigma is given).  The reference forms the n x n matrices in numpy and
centres them with n x n x n products.  Here `audiossl_cka_hsic` (csrc/cka.hip) sweeps the tiles of K and L together on the fp32
MFMA pipe and reduces them where they are formed:

    sum(HKH * HLH) = S_KL - (2 / n) sum_i k_i l_i + k l / n^2     (S_KL = sum_ij K_ij L_ij; k_i, l_i row sums; k, l totals)

so no n x n matrix is ever stored.  The median is an exact order statistic of the kernel's own fp32 distances (radix select,
`audiossl_cka_sigma2`).  Column means are subtracted first by default (`audiossl_cka_center`): that changes neither the centred
linear Gram nor any distance, and it removes the cancellation an offset would bring into both.
Everything allocates through torch; the only host synchronisation is reading the 8 result values.  Single GPU.
"""

import torch
import torch.nn.functional as F

from src import _native as N

LINEAR, RBF = 0, 1
KERNELS = {"linear": LINEAR, "rbf": RBF}
MAX_N, MAX_WIDTH = 65536, 4096
TERMS = ("cka", "hsic_xy", "hsic_xx", "hsic_yy", "s_kl", "s_kk", "s_ll")


def workspace_bytes(n, p, q):
    return N.workspace_bytes("cka_workspace", n, p, q)


def _prepare(x, center):
    """[n, d] device tensor -> contiguous fp32 [n, d4], d4 = d rounded up to a multiple of 4 with zero columns (a zero column
    changes no Gram entry), column means subtracted when `center`."""
    if not x.is_cuda:
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    if x.dim() != 2:
        raise ValueError(f"features are [n, d], got {tuple(x.shape)}")
    x = x.float()
    d = x.shape[1]
    if d % 4:
        x = F.pad(x, (0, 4 - d % 4))
    x = x.contiguous()
    if not center:
        return x
    out = torch.empty_like(x)
    N.call("cka_center", x, x.shape[0], x.shape[1], out)
    return out


def median_sigma2(x, center=True, workspace=None):
    """-> (sigma2 fp64 [1], count int64 [1]) on the device: the median of the non-zero squared distances between rows of x
    (the reference's `np.median(KX[KX != 0])`), an exact order statistic of the fp32 distances the kernel forms."""
    x = _prepare(x, center)
    return _sigma2(x, workspace)


def _sigma2(x, ws=None):
    n, p = x.shape
    nbytes = workspace_bytes(n, p, p)
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    s2 = torch.empty(1, dtype=torch.float64, device=x.device)
    cnt = torch.empty(1, dtype=torch.int64, device=x.device)
    N.call("cka_sigma2", x, n, p, s2, cnt, ws, nbytes)
    return s2, cnt


def _check(x, y, kernel, sigma):
    if kernel not in KERNELS:
        raise ValueError(f"kernel must be one of {tuple(KERNELS)}")
    if not (x.is_cuda and y.is_cuda):
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    if x.dim() != 2 or y.dim() != 2:
        raise ValueError(f"features are [n, d], got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"x has {x.shape[0]} rows, y has {y.shape[0]}: row i of both must come from the same clip")
    if not 2 <= x.shape[0] <= MAX_N:
        raise ValueError(f"n must be in [2, {MAX_N}], got {x.shape[0]}")
    if max(x.shape[1], y.shape[1]) > MAX_WIDTH or min(x.shape[1], y.shape[1]) < 1:
        raise ValueError(f"feature widths must be in [1, {MAX_WIDTH}]")
    if sigma is not None and not float(sigma) > 0.0:
        raise ValueError("sigma must be positive")


def _hsic(x, y, kernel, sigma, s2x=None, s2y=None):
    """x, y as `_prepare` leaves them; s2x / s2y: device medians already taken (RBF with sigma None), else taken here."""
    n, p, q = x.shape[0], x.shape[1], y.shape[1]
    nbytes = workspace_bytes(n, p, q)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(8, dtype=torch.float64, device=x.device)
    given = 0.0
    if KERNELS[kernel] == RBF:
        if sigma is not None:
            given, s2x, s2y = float(sigma), None, None
        else:
            s2x = _sigma2(x, ws)[0] if s2x is None else s2x
            s2y = _sigma2(y, ws)[0] if s2y is None else s2y
    else:
        s2x = s2y = None
    N.call("cka_hsic", x, y, n, p, q, KERNELS[kernel], given, s2x, s2y, out, None, None, ws, nbytes)
    return out


def hsic_terms(x, y, kernel="linear", sigma=None, center=True):
    """-> fp64 [8] on the device: {cka, hsic_xy, hsic_xx, hsic_yy, S_kl, S_kk, S_ll, 0} (`TERMS`).  x [n, p], y [n, q]: row i of
    both from the same clip.  kernel "rbf": sigma None = per-matrix median rule, else the same sigma for both matrices."""
    _check(x, y, kernel, sigma)
    return _hsic(_prepare(x, center), _prepare(y, center), kernel, sigma)


def linear_cka(x, y, center=True):
    """`linear_CKA(X, Y)` of extras/CKA.py -> python float."""
    return float(hsic_terms(x, y, "linear", None, center)[0])


def kernel_cka(x, y, sigma=None, center=True):
    """`kernel_CKA(X, Y, sigma)` of extras/CKA.py (RBF) -> python float."""
    return float(hsic_terms(x, y, "rbf", sigma, center)[0])


def cka_matrix(feats_a, feats_b=None, kernel="linear", sigma=None):
    """feats_a, feats_b: sequences (or dicts, in their own order) of [n, d_l] device tensors over the same n clips ->
    fp64 [La, Lb] CPU tensor of CKA values; feats_b None = feats_a against itself.  Every feature matrix is centred once and
    its median taken once; the entries are what `hsic_terms` gives pair by pair."""
    a = list(feats_a.values()) if isinstance(feats_a, dict) else list(feats_a)
    b = a if feats_b is None else (list(feats_b.values()) if isinstance(feats_b, dict) else list(feats_b))
    for x in a:
        for y in b:
            _check(x, y, kernel, sigma)
    median = KERNELS[kernel] == RBF and sigma is None

    def prepared(feats):
        out = []
        for f in feats:
            f = _prepare(f, True)
            out.append((f, _sigma2(f)[0] if median else None))
        return out
    pa = prepared(a)
    pb = pa if feats_b is None else prepared(b)
    res = [torch.stack([_hsic(x, y, kernel, sigma, sx, sy)[0] for y, sy in pb]) for x, sx in pa]
    return torch.stack(res).cpu()
