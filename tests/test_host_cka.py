"""CPU: the fp64 restatement of CKA (tests/cka_ref.py) against the values recorded from the reference's module
(tests/golden/cka_reference.npz), its two forms against each other, and the argument checks of the `audiossl_cka_*` entries,
which all return their code before anything is launched (no device here)."""
import ctypes
import os

import numpy as np
import pytest

import cka_ref as R
from src import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cka_reference.npz")
EINVAL, EALIGN = -1, -3


def _golden():
    z = np.load(GOLDEN)
    fields = [str(f) for f in z["fields"]]
    cases = []
    for i in range(3):
        cases.append((z[f"x_{i}"], z[f"y_{i}"], dict(zip(fields, z[f"ref_{i}"]))))
    return cases, float(z["sigma"])


def _close(a, b, rel=1e-12):
    return abs(a - b) <= rel * abs(b)


def test_restatement_matches_the_recorded_reference_values_and_its_two_forms_agree():
    cases, sigma = _golden()
    assert [c[0].shape + c[1].shape[1:] for c in cases] == [(5, 4, 8), (97, 64, 32), (130, 100, 36)]
    for x, y, ref in cases:
        assert x.dtype == np.float32 and y.dtype == np.float32
        for kernel, sg, tag in (("linear", None, "linear_{}"), ("rbf", None, "kernel_{}_median"), ("rbf", sigma, "kernel_{}_sigma")):
            for form in (R.hsic_identity, R.hsic_explicit):
                t = R.terms(x, y, kernel, sg, form=form)
                for name in ("cka", "hsic_xy", "hsic_xx", "hsic_yy"):
                    want = ref[tag.format(name)]
                    # the explicit form (the reference's own) to 1e-12; the identity on these UNCENTRED offset inputs subtracts
                    # sums about 1e3 times the result, so its raw HSIC values get 1e-10 (its CKA, a ratio, still 1e-12)
                    assert _close(t[name], want, 1e-12 if name == "cka" or form is R.hsic_explicit else 1e-10), (kernel, sg, name, t[name], want)
            a, b = R.terms(x, y, kernel, sg, form=R.hsic_identity), R.terms(x, y, kernel, sg, form=R.hsic_explicit)
            assert _close(a["cka"], b["cka"], 1e-12)
            # column centring changes nothing
            c = R.terms(R.center(x), R.center(y), kernel, sg)
            assert _close(c["cka"], a["cka"], 1e-10)
        assert _close(R.median_sigma2(x), ref["median_x"]) and _close(R.median_sigma2(y), ref["median_y"])


def test_median_over_the_upper_triangle_is_the_median_over_the_full_matrix():
    for seed, shape in ((1, (7, 4)), (2, (8, 4)), (3, (40, 8))):
        x = np.random.RandomState(seed).randint(-2, 3, shape)
        x[3] = x[1]                                                    # a duplicated row: a zero off the diagonal
        full, m = R.exact_sigma2(x)
        g = x @ x.T
        d = np.diag(g)[:, None] + np.diag(g)[None, :] - 2 * g
        up = np.sort(d[np.triu_indices(len(x), 1)])
        up = up[up != 0]
        assert m == len(up) and full == (up[(m - 1) // 2] + up[m // 2]) / 2


def test_exact_terms_agree_with_the_fp64_forms():
    x = np.random.RandomState(5).randint(-2, 3, (33, 8))
    y = np.random.RandomState(6).randint(-2, 3, (33, 12))
    s_kl, s_kk, s_ll, rk, rl = R.exact_linear_terms(x, y)
    k, l = R.gram(x), R.gram(y)
    n = 33
    want = s_kl - 2.0 / n * float(np.dot(rk, rl)) + float(rk.sum()) * float(rl.sum()) / n ** 2
    assert _close(R.hsic_explicit(k, l), want, 1e-11)
    assert (s_kk, s_ll) == (int((k * k).sum()), int((l * l).sum()))


# ---- argument checks: every code comes back before a launch -----------------------------------------------------------------
def _ws(n, p=8, q=8):
    b = ctypes.c_long(-7)
    rc = N.lib().audiossl_cka_workspace(n, p, q, ctypes.addressof(b))
    return rc, b.value


def test_workspace_checks_and_is_monotone_in_n():
    lib = N.lib()
    assert lib.audiossl_cka_workspace(100, 8, 8, None) == EINVAL
    for n, p, q in ((1, 8, 8), (0, 8, 8), (-3, 8, 8), (65537, 8, 8), (100, 6, 8), (100, 8, 10), (100, 0, 8), (100, 8, 4100), (100, 5000, 8)):
        assert _ws(n, p, q)[0] == EINVAL, (n, p, q)
    prev = 0
    for n in list(range(2, 700)) + [1000, 1100, 4096, 8192, 8193, 32768, 65536]:
        rc, b = _ws(n, 64, 2048)
        assert rc == 0 and b >= prev and b % 16 == 0, n
        prev = b
    assert _ws(32768, 4096, 4096)[0] == 0
    assert _ws(2, 4, 4)[1] >= 2 * 2048 * 8                             # the two histograms at least


def test_center_and_sigma2_argument_checks():
    lib = N.lib()
    big = _ws(100)[1]
    A = 4096                                                           # an aligned non-null address; never dereferenced
    assert lib.audiossl_cka_center(None, 100, 8, A, None) == EINVAL
    assert lib.audiossl_cka_center(A, 100, 8, None, None) == EINVAL
    assert lib.audiossl_cka_center(A, 1, 8, A, None) == EINVAL
    assert lib.audiossl_cka_center(A, 65537, 8, A, None) == EINVAL
    assert lib.audiossl_cka_center(A, 100, 6, A, None) == EINVAL
    assert lib.audiossl_cka_center(A, 100, 4100, A, None) == EINVAL
    assert lib.audiossl_cka_center(A + 4, 100, 8, A, None) == EALIGN
    assert lib.audiossl_cka_center(A, 100, 8, A + 8, None) == EALIGN
    sig = lib.audiossl_cka_sigma2
    assert sig(None, 100, 8, A, A, A, big, None) == EINVAL
    assert sig(A, 100, 8, None, A, A, big, None) == EINVAL
    assert sig(A, 100, 8, A, A, None, big, None) == EINVAL
    assert sig(A, 1, 8, A, A, A, big, None) == EINVAL
    assert sig(A, 65537, 8, A, A, A, 1 << 40, None) == EINVAL
    assert sig(A, 100, 7, A, A, A, big, None) == EINVAL
    assert sig(A, 100, 0, A, A, A, big, None) == EINVAL
    assert sig(A, 100, 8, A, A, A, big - 1, None) == EINVAL           # short workspace
    assert sig(A + 4, 100, 8, A, A, A, big, None) == EALIGN
    assert sig(A, 100, 8, A, A, A + 8, big, None) == EALIGN


def test_hsic_argument_checks():
    lib = N.lib()
    big = _ws(100)[1]
    A = 4096
    h = lib.audiossl_cka_hsic

    def call(x=A, y=A, n=100, p=8, q=8, kernel=0, sigma=0.0, s2x=None, s2y=None, out=A, ws=A, nbytes=big):
        return h(x, y, n, p, q, kernel, sigma, s2x, s2y, out, None, None, ws, nbytes, None)
    assert call(x=None) == EINVAL and call(y=None) == EINVAL and call(out=None) == EINVAL and call(ws=None) == EINVAL
    assert call(n=1) == EINVAL and call(n=65537, nbytes=1 << 40) == EINVAL
    assert call(p=6) == EINVAL and call(q=6) == EINVAL and call(p=0) == EINVAL and call(q=4100) == EINVAL
    assert call(nbytes=big - 1) == EINVAL
    assert call(kernel=2) == EINVAL and call(kernel=-1) == EINVAL
    assert call(kernel=1, sigma=0.0) == EINVAL and call(kernel=1, sigma=-1.0) == EINVAL          # sigma <= 0
    assert call(kernel=1, sigma=float("nan")) == EINVAL and call(kernel=1, sigma=float("inf")) == EINVAL
    assert call(kernel=1, sigma=0.0, s2x=A) == EINVAL                                             # one median pointer only
    assert call(kernel=1, sigma=2.0, s2x=A, s2y=A) == EINVAL                                      # both rules at once
    assert call(x=A + 4) == EALIGN and call(y=A + 8) == EALIGN and call(ws=A + 4) == EALIGN and call(out=A + 8) == EALIGN


def test_python_layer_refuses_cpu_tensors_and_row_mismatch():
    import torch
    from src.evaluation import cka_matrix, hsic_terms, kernel_cka, linear_cka
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        linear_cka(torch.zeros(8, 4), torch.zeros(8, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernel_cka(torch.zeros(8, 4), torch.zeros(8, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cka_matrix([torch.zeros(8, 4)])
    with pytest.raises(ValueError):
        hsic_terms(torch.zeros(8, 4), torch.zeros(8, 4), kernel="cosine")
