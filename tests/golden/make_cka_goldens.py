#!/usr/bin/env python3
"""Writes tests/golden/cka_reference.npz: what the reference's CKA module computes on small recorded inputs.

    python tests/golden/make_cka_goldens.py /path/to/reference/extras/CKA.py

The module is loaded from the path given (nothing of it is copied here); it runs on float64 copies of the recorded fp32 inputs.
Recorded per case c in CASES: x_c, y_c (fp32) and ref_c (fp64 [13]) in the order of FIELDS.  The two medians are what the module
itself hands to `np.median` (captured by a recording stand-in for its `np`) during `kernel_CKA(X, Y, sigma=None)`.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cka_ref  # noqa: E402

CASES = ((5, 4, 8), (97, 64, 32), (130, 100, 36))
SIGMA = 7.5
FIELDS = ("linear_cka", "linear_hsic_xy", "linear_hsic_xx", "linear_hsic_yy", "kernel_cka_median", "kernel_hsic_xy_median",
          "kernel_hsic_xx_median", "kernel_hsic_yy_median", "kernel_cka_sigma", "kernel_hsic_xy_sigma", "kernel_hsic_xx_sigma",
          "kernel_hsic_yy_sigma", "median_x", "median_y")


class RecordingNumpy:
    """numpy, except that `median` remembers what it returned."""

    def __init__(self):
        self.medians = []

    def __getattr__(self, name):
        return getattr(np, name)

    def median(self, *a, **k):
        m = np.median(*a, **k)
        self.medians.append(float(m))
        return m


def main(path):
    spec = importlib.util.spec_from_file_location("reference_cka", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rec = RecordingNumpy()
    ref.np = rec
    out = {}
    for i, (n, p, q) in enumerate(CASES):
        x32, y32 = cka_ref.correlated(n, p, q, seed=100 + i)
        x, y = x32.astype(np.float64), y32.astype(np.float64)
        vals = [ref.linear_CKA(x, y), ref.linear_HSIC(x, y), ref.linear_HSIC(x, x), ref.linear_HSIC(y, y)]
        rec.medians.clear()
        vals.append(ref.kernel_CKA(x, y, sigma=None))
        med = list(rec.medians)                       # kernel_HSIC(X, Y): rbf(X) then rbf(Y) come first
        vals += [ref.kernel_HSIC(x, y, None), ref.kernel_HSIC(x, x, None), ref.kernel_HSIC(y, y, None)]
        vals += [ref.kernel_CKA(x, y, sigma=SIGMA), ref.kernel_HSIC(x, y, SIGMA), ref.kernel_HSIC(x, x, SIGMA), ref.kernel_HSIC(y, y, SIGMA)]
        vals += [med[0], med[1]]
        out[f"x_{i}"], out[f"y_{i}"], out[f"ref_{i}"] = x32, y32, np.asarray(vals, dtype=np.float64)
    out["sigma"] = np.float64(SIGMA)
    out["fields"] = np.array(FIELDS)
    target = os.path.join(HERE, "cka_reference.npz")
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
