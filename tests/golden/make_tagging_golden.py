#!/usr/bin/env python3
"""Writes tests/golden/tagging_stats.npz: what the reference's tagging metrics give on five small recorded matrices.

    python tests/golden/make_tagging_golden.py /path/to/reference/extras/mast_new/mast/utilities/stats.py

The module is loaded from the path given (nothing of it is copied here; it needs sklearn and scipy, at generation time only).
Recorded per case i of `tagging_ref.GOLDEN_CASES`: scores_i (fp32 [N, C]), targets_i (uint8 [N, C]) and the per-class AP_i, auc_i,
dprime_i (fp64 [C]) of `calculate_stats` / `d_prime`.  Arrays only: the file loads with allow_pickle=False.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tagging_ref  # noqa: E402


def main(path):
    spec = importlib.util.spec_from_file_location("reference_tagging_stats", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for i in range(len(tagging_ref.GOLDEN_CASES)):
        s, t = tagging_ref.golden_matrix(i)
        st = ref.calculate_stats(s, t.astype(np.int64))
        out[f"scores_{i}"], out[f"targets_{i}"] = s, t
        out[f"AP_{i}"] = np.array([c["AP"] for c in st], dtype=np.float64)
        out[f"auc_{i}"] = np.array([c["auc"] for c in st], dtype=np.float64)
        out[f"dprime_{i}"] = np.array([ref.d_prime(c["auc"]) for c in st], dtype=np.float64)
    target = os.path.join(HERE, "tagging_stats.npz")
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
