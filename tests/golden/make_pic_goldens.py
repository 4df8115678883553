#!/usr/bin/env python3
"""Writes tests/golden/pic_reference.npz: what the reference's PIC computes on small recorded inputs.

    python tests/golden/make_pic_goldens.py /path/to/reference/extras/decar-v2/clustering.py

The module is loaded from the path given (nothing of it is copied here).  `faiss` is an empty stand-in module (the graph is the
only thing the module asks of it), `preprocess_features` is replaced by the identity and `make_graph` by the float64 brute force
of tests/pic_ref.py under this project's order (d2 ascending, row ascending).  Everything after the graph - `make_adjacencyW`,
`run_pic`, `find_maxima_cluster` and the singleton redistribution of `PIC.cluster` - is the module's own code.

Under numpy 2.x the module's arithmetic stays in float32 end to end, under the numpy it pins it would be float64.  A case is
therefore recorded only if (a) the float64 restatement of tests/pic_ref.py gives the same partition as the module's run, raw and
after redistribution, and (b) every decision of the restatement's walk, "no positive value" at the roots included, has a relative
margin of at least MIN_MARGIN; otherwise the next seed is tried.
Recorded per case c: x_c (fp32), I_c (int64), D_c (fp32), raw_c (the module's `run_pic` output), final_c (the label of every row
in the module's final `images_lists`), margin_c, seed_c.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pic_ref as R  # noqa: E402

MIN_MARGIN = 1e-4


def load_reference(path):
    sys.modules.setdefault("faiss", types.ModuleType("faiss"))
    spec = importlib.util.spec_from_file_location("reference_clustering", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    ref.preprocess_features = lambda data, *a, **k: data
    ref.make_graph = R.make_graph
    return ref


def run_case(ref, n, dim, centres, seed):
    x = R.blobs(n, dim, centres, seed)
    I, D = R.make_graph(x, R.NNN)
    raw = np.asarray(ref.run_pic(I, D, R.SIGMA, R.ALPHA), dtype=np.int64)
    model = ref.PIC(sigma=R.SIGMA, nnn=R.NNN, alpha=R.ALPHA, distribute_singletons=True)
    model.cluster(x)
    final = np.full(n, -1, dtype=np.int64)
    for c, members in enumerate(model.images_lists):
        final[np.asarray(members, dtype=np.int64)] = c
    assert (final >= 0).all()
    raw64, final64, margin = R.pic(I, D)
    same = np.array_equal(R.renumber(raw), R.renumber(raw64)) and np.array_equal(R.renumber(final), final64)
    return same and margin >= MIN_MARGIN, dict(x=x, I=I, D=D, raw=raw, final=final, margin=np.float64(margin), seed=np.int64(seed))


def main(path):
    ref = load_reference(path)
    out = {}
    for i, (n, dim, centres) in enumerate(R.CASES):
        for seed in range(100):
            ok, rec = run_case(ref, n, dim, centres, seed)
            if ok:
                break
            print(f"case {i}: seed {seed} rejected (margin {float(rec['margin']):.3g})")
        else:
            raise RuntimeError(f"no seed below 100 serves case {i}")
        print(f"case {i}: n {n} dim {dim} seed {seed}: {len(set(rec['raw'].tolist()))} raw clusters, "
              f"{len(set(rec['final'].tolist()))} after redistribution, margin {float(rec['margin']):.3g}")
        for key, val in rec.items():
            out[f"{key}_{i}"] = val
    out["params"] = np.asarray([R.SIGMA, R.NNN, R.ALPHA, R.ITERS], dtype=np.float64)
    target = os.path.join(HERE, "pic_reference.npz")
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
