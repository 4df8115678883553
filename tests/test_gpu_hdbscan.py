"""The exact mutual-reachability spanning tree on the GPU (`audiossl_mreach_mst`, csrc/mst.hip), the Python layer above it
(src/evaluation/hdbscan.py) and `store_clusters --clustering hdbscan`.

Bars.  The tree is unique under the strict order (w2 bits, lo, hi), so wherever the kernel's own distance bits are known - from
`range_graph` at a radius that takes every pair, core distances from `knn_graph`, or integer data whose fp64 distances ARE the
fp32 ones - the edge set {(u, v, w2 bits)} must EQUAL host Kruskal's under that order.  On real data the sorted weights lie
within 8 sqrt(32) 2^-24 max|x|^2 of the sorted fp64 weights (the bar tests/test_gpu_graph.py uses for d2; the k-th smallest tree
weight moves by at most the largest change of any weight), and the labels are sklearn's (ARI exactly 1.0, equal noise sets)."""
import functools

import numpy as np
import pytest
import torch

import hdbscan_ref as R

pytestmark = pytest.mark.gpu

GUARD = 2
EPS24 = 2.0 ** -24
ALL_PAIRS = 1e30                                                             # a large finite radius: every pair is inside


def _launch_mst(x, core2=None, splits=0):
    """x [n, d] fp32 numpy (d % 4 == 0), core2 [n] fp32 numpy or None -> (eu, ev int64 [n - 1], ew2 fp32 [n - 1], rounds) in the
    entry point's own order; guards behind every output, the workspace checked past its size, the inputs compared unchanged."""
    from src import _native as N
    n, d = x.shape
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    cd = None if core2 is None else torch.from_numpy(np.array(core2, dtype=np.float32)).cuda()
    eu = torch.full((n - 1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    ev = torch.full((n - 1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    ew2 = torch.full((n - 1 + GUARD,), -7.5, dtype=torch.float32, device="cuda")
    rounds = torch.full((1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    nbytes = N.workspace_bytes("mreach_mst_workspace", n, splits)
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")   # the kernels clear what they need
    N.call("mreach_mst", xd, n, d, cd, splits, eu, ev, ew2, rounds, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((eu[n - 1:] == -7).all()) and bool((ev[n - 1:] == -7).all()) and bool((ew2[n - 1:] == -7.5).all()), "guards overwritten"
    assert bool((rounds[1:] == -7).all()) and bool((ws[nbytes:] == 0xA5).all()), "workspace overrun"
    assert torch.equal(xd.cpu(), torch.from_numpy(np.array(x, dtype=np.float32))), "input changed"
    if cd is not None:
        assert torch.equal(cd.cpu(), torch.from_numpy(np.array(core2, dtype=np.float32))), "core2 changed"
    return (eu[:n - 1].cpu().numpy().astype(np.int64), ev[:n - 1].cpu().numpy().astype(np.int64), ew2[:n - 1].cpu().numpy(),
            int(rounds[0]))


def _pad4(x):
    d = x.shape[1]
    return x if d % 4 == 0 else np.concatenate([x, np.zeros((len(x), 4 - d % 4), dtype=x.dtype)], 1)


def _kernel_d2_bits(x):
    """The kernel's own d2 of every pair as a dense uint32 [n, n] (the diagonal is 0): the complete radius graph."""
    from src.evaluation.dedup import range_graph
    n = len(x)
    csr = range_graph(torch.from_numpy(np.array(x, dtype=np.float32)).cuda(), ALL_PAIRS, max_edges=n * (n - 1))
    rowptr, col, d2 = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy(), csr.d2.cpu().numpy()
    assert np.array_equal(np.diff(rowptr), np.full(n, n - 1))
    dense = np.zeros((n, n), dtype=np.float32)
    dense[np.repeat(np.arange(n), n - 1), col] = d2
    assert np.array_equal(dense.view(np.uint32), dense.T.view(np.uint32)), "d2_ij != d2_ji"
    return dense


def _kernel_core2(x, min_samples):
    from src.evaluation.graph import knn_graph
    if min_samples == 1:
        return None
    d2 = knn_graph(torch.from_numpy(np.array(x, dtype=np.float32)).cuda(), min_samples - 1)[1]
    return d2[:, min_samples - 2].cpu().numpy()


def _assert_tree_equals_kruskal(got, w2, what):
    """got = (eu, ev, ew2, rounds); w2 fp32 [n, n], symmetric: the weights in the kernel's own bits."""
    eu, ev, ew2, rounds = got
    n = len(w2)
    assert len(eu) == n - 1 and (eu < ev).all() and (eu >= 0).all() and (ev < n).all(), what
    assert R.is_spanning_tree(eu, ev, n), f"{what}: not a spanning tree"
    ku, kv, kw = R.kruskal(np.ascontiguousarray(w2, dtype=np.float32).view(np.uint32))
    want = set(zip(ku.tolist(), kv.tolist(), kw.tolist()))
    have = set(zip(eu.tolist(), ev.tolist(), ew2.view(np.uint32).tolist()))
    assert have == want, f"{what}: {len(have ^ want)} edges differ from Kruskal under (w2 bits, lo, hi)"
    bound = 0
    while (1 << bound) < n:
        bound += 1
    assert 1 <= rounds <= bound, f"{what}: {rounds} rounds for n = {n}"


def _mreach(d2, core2):
    if core2 is None:
        return d2
    return np.maximum(d2, np.maximum(core2[:, None], core2[None, :])).astype(np.float32)


# ---- 1. the unique tree, bit for bit, at the tile edges ---------------------------------------------------------------------
# QT = 64 owned rows, BT = 128 walked rows, KC = 32 features per chunk (36: one chunk and a remainder of 4; 132: four and 4).
# min_samples = 4 needs four points: on 2 and 3 points every point counts (min_samples = n), the largest value there is.
@pytest.mark.parametrize("min_samples", [1, 4])
@pytest.mark.parametrize("d", [4, 36, 132])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 128, 129, 193])
def test_tree_is_kruskals_bit_for_bit(n, d, min_samples):
    x = np.random.default_rng(1000 * n + d).normal(size=(n, d)).astype(np.float32)
    ms = min(min_samples, n)
    core2 = _kernel_core2(x, ms)
    w2 = _mreach(_kernel_d2_bits(x), core2)
    _assert_tree_equals_kruskal(_launch_mst(x, core2), w2, f"n {n} d {d} min_samples {ms}")


# ---- 2. heavy ties ------------------------------------------------------------------------------------------------------------
def _ties(kind):
    g = np.random.default_rng(5)
    if kind == "integers":                                                    # exact in fp32: the fp64 reference applies directly
        return g.integers(0, 4, size=(200, 4)).astype(np.float32)
    if kind == "identical":                                                   # every weight is 0
        return np.repeat(g.normal(size=(1, 8)), 70, 0).astype(np.float32)
    x = g.normal(size=(200, 36)).astype(np.float32)                           # two planted blocks of 40 repeated rows
    p = g.permutation(200)
    x[p[:40]] = x[p[0]]
    x[p[40:80]] = x[p[40]]
    return x


@pytest.mark.parametrize("min_samples", [1, 5])
@pytest.mark.parametrize("kind", ["integers", "identical", "planted"])
def test_heavy_ties_cannot_close_a_cycle(kind, min_samples):
    x = _ties(kind)
    core2 = _kernel_core2(x, min_samples)
    if kind == "integers":
        ref, ref_core = R.mutual_reachability2(x, min_samples)
        w2 = ref.astype(np.float32)
        assert np.array_equal(w2.astype(np.float64), ref)
        if core2 is not None:
            np.testing.assert_array_equal(core2.astype(np.float64), ref_core)
    else:
        w2 = _mreach(_kernel_d2_bits(x), core2)
    if kind == "identical":
        assert not w2.any()
    got = _launch_mst(x, core2)
    _assert_tree_equals_kruskal(got, w2, f"{kind} min_samples {min_samples}")
    if kind == "planted" and min_samples == 1:
        assert int((got[2] == 0).sum()) == 78                                 # 39 + 39 edges inside the blocks, at exactly 0


# ---- 3. splits and reproducibility ------------------------------------------------------------------------------------------
def test_output_bits_do_not_depend_on_splits_or_on_the_launch():
    for case, ms in ((1, 5), (3, 1)):                                         # 545 rows: five walked tiles; 280 rows: three
        x = R.case_points(case)
        core2 = _kernel_core2(x, ms)
        base = _launch_mst(x, core2, 0)
        for splits in (0, 1, 3):
            got = _launch_mst(x, core2, splits)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), f"splits {splits}"
            assert np.array_equal(got[2].view(np.uint32), base[2].view(np.uint32)) and got[3] == base[3]


# ---- 4. against fp64, and sklearn end to end ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_weights(case):
    w2, _ = R.mutual_reachability2(R.case_points(case), R.CASES[case][5])
    return np.sort(R.kruskal(w2)[2])


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_cases_against_fp64_and_sklearn(case):
    from src.evaluation import hdbscan as H
    x = R.case_points(case)
    n, (ms, mcs) = len(x), R.CASES[case][5:]
    xd = torch.from_numpy(np.array(x)).cuda()
    mst, rounds = H.mutual_reachability_mst(xd, ms, return_rounds=True)
    u, v, w2 = mst.u.cpu().numpy(), mst.v.cpu().numpy(), mst.w2.cpu().numpy()
    assert mst.u.dtype == torch.int64 and mst.w2.dtype == torch.float32 and len(u) == n - 1
    assert R.is_spanning_tree(u, v, n) and (u < v).all()
    key = list(zip(w2.tolist(), u.tolist(), v.tolist()))
    assert key == sorted(key), "not sorted by (w2, u, v)"
    bar = 8.0 * np.sqrt(32) * EPS24 * float((x.astype(np.float64) ** 2).sum(1).max())
    err = float(np.abs(w2.astype(np.float64) - _ref_weights(case)).max())
    print(f"case {case}: n {n}, {rounds} rounds, max |sorted w2 - fp64| = {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    res = H.hdbscan(xd, min_cluster_size=mcs, min_samples=ms)
    want, want_prob = R.sklearn_answer(case)
    print(f"case {case}: {res.n_clusters} clusters, {int((res.labels < 0).sum())} noise; sklearn {int(want.max()) + 1}, {int((want < 0).sum())}")
    assert res.n_clusters == R.CASE_FACTS[case][0]
    R.assert_same_clustering(res.labels, want)
    assert res.probabilities.shape == (n,) and ((res.probabilities >= 0) & (res.probabilities <= 1)).all()
    assert (res.probabilities[res.labels < 0] == 0).all()
    first = [int(np.flatnonzero(res.labels == c)[0]) for c in range(res.n_clusters)]
    assert first == sorted(first)                                             # numbered by smallest member


# ---- 5. the bridge to the duplicate search --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,radii", [(0, (0.6, 2.5)), (2, (0.05, 0.4))])
def test_cut_mst_is_the_duplicate_search_at_every_radius(case, radii):
    from src.evaluation import hdbscan as H
    from src.evaluation.dedup import graph_components, range_graph
    x = torch.from_numpy(np.array(R.case_points(case))).cuda()
    n = x.shape[0]
    mst = H.mutual_reachability_mst(x, 1)
    for r2 in radii:
        csr = range_graph(x, r2, max_edges=n * (n - 1))
        label, count = graph_components(csr.rowptr, csr.col, n)
        assert 1 < count < n
        np.testing.assert_array_equal(H.cut_mst(mst, n, r2), label.cpu().numpy().astype(np.int64))


# ---- 6. arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_the_wrapper_pads():
    from src import _native as N
    from src.evaluation import hdbscan as H
    lib = N.lib()
    x = torch.from_numpy(np.array(R.case_points(2))).cuda()                   # [191, 4]
    n = x.shape[0]
    eu = torch.full((n - 1,), -7, dtype=torch.int32, device="cuda")
    ev, ew2 = eu.clone(), torch.full((n - 1,), -7.5, dtype=torch.float32, device="cuda")
    nbytes = N.workspace_bytes("mreach_mst_workspace", n, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    x5 = torch.zeros(n, 5, device="cuda")

    def call(xx, nn, dd, splits, bytes_):
        return lib.audiossl_mreach_mst(xx.data_ptr(), nn, dd, None, splits, eu.data_ptr(), ev.data_ptr(), ew2.data_ptr(), None,
                                       ws.data_ptr(), bytes_, None)
    assert call(x, 1, 4, 0, nbytes) == -1                                     # n = 1
    assert call(x5, n, 5, 0, nbytes) == -1                                    # d % 4 at the ABI
    assert call(x, n, 4, 65, nbytes) == -1                                    # splits
    assert call(x, n, 4, 0, nbytes - 1) == -1                                 # a short workspace
    torch.cuda.synchronize()
    assert bool((eu == -7).all()) and bool((ev == -7).all()) and bool((ew2 == -7.5).all()), "a refused call wrote something"
    assert call(x, n, 4, 0, nbytes) == 0                                      # rounds = NULL is allowed
    torch.cuda.synchronize()
    assert R.is_spanning_tree(eu.cpu().numpy().astype(np.int64), ev.cpu().numpy().astype(np.int64), n)
    # the Python layer pads d = 5 with zero columns: the tree of the padded points
    g = np.random.default_rng(8).normal(size=(100, 5)).astype(np.float32)
    mst = H.mutual_reachability_mst(torch.from_numpy(g).cuda(), 3)
    core2 = _kernel_core2(_pad4(g), 3)
    got = (mst.u.cpu().numpy(), mst.v.cpu().numpy(), mst.w2.cpu().numpy(), 1)
    _assert_tree_equals_kruskal(got, _mreach(_kernel_d2_bits(_pad4(g)), core2), "d = 5 through the wrapper")
    np.testing.assert_array_equal(H.core_distances2(torch.from_numpy(g).cuda(), 3).cpu().numpy(), core2)
    assert not H.core_distances2(torch.from_numpy(g).cuda(), 1).any()


# ---- 7. the command -------------------------------------------------------------------------------------------------------------
def test_store_clusters_hdbscan_command(tmp_path, cfg_s, capsys):
    import pandas as pd
    from scipy.io import wavfile
    from src.evaluation import hdbscan as H
    from src.evaluation.embed import extract_embeddings, load_embedder
    from src.upstream.decar_v2 import store_clusters as sc
    from src.upstream.decar_v2.clustering import preprocess_features
    from test_gpu_graph import _checkpoint, _write_wavs
    ckpt = _checkpoint(tmp_path, cfg_s)
    # three groups of five clips that differ by a whisper of noise, and four clips of their own
    files = _write_wavs(tmp_path, [16000] * 7, salt=700)
    g = np.random.default_rng(3)
    for k in range(3):
        rate, base = wavfile.read(files[k])
        for c in range(4):
            p = str(tmp_path / f"copy_{k}_{c}.wav")
            wavfile.write(p, rate, (base.astype(np.int32) + g.integers(-40, 41, size=base.shape)).clip(-32768, 32767).astype(np.int16))
            files.append(p)
    files = [files[i] for i in g.permutation(len(files))]
    n = len(files)
    assert n == 19
    files_csv = str(tmp_path / "files.csv")
    pd.DataFrame({"files": files}).to_csv(files_csv, index=False)
    base = ["--checkpoint", ckpt, "--upstream", "delores_s", "--input", files_csv, "--pca", "8", "--window", "center",
            "--clustering", "hdbscan", "--min_cluster_size", "4", "--min_samples", "3"]
    # what the command has to compute, from the same library calls
    embedder = load_embedder(ckpt, "delores_s", config=None, layer="backbone")
    feats = extract_embeddings(embedder, files, batch_size=64, window="center", duration=1.0)
    want = H.hdbscan(preprocess_features(feats, pca=8), min_cluster_size=4, min_samples=3)
    noise, count = int((want.labels < 0).sum()), want.n_clusters
    print(f"command fixture: {count} clusters, {noise} noise of {n}")
    assert count >= 2 and noise >= 1, "the fixture must have clusters and noise for the command to show both"

    out = str(tmp_path / "all.csv")
    labels = sc.main(sc.get_args(base + ["--out", out, "--score"]))
    text = capsys.readouterr().out
    assert np.array_equal(np.asarray(labels), want.labels)
    assert f"{n} files, {count} clusters, {noise} noise, hdbscan min_cluster_size 4 min_samples 3 -> " in text
    assert "silhouette " in text and f"({count} clusters, " in text
    got = pd.read_csv(out)
    assert list(got.columns) == ["files", "label"] and list(got["files"]) == files
    assert got["label"].tolist() == want.labels.tolist() and int((got["label"] == -1).sum()) == noise

    out = str(tmp_path / "kept.csv")
    sc.main(sc.get_args(base + ["--out", out, "--drop_unreached", "--confidence"]))
    assert f"{noise} noise (dropped)" in capsys.readouterr().out
    got = pd.read_csv(out)
    keep = want.labels >= 0
    assert list(got.columns) == ["files", "label", "confidence"]
    assert list(got["files"]) == [f for f, k in zip(files, keep) if k]
    assert got["label"].tolist() == want.labels[keep].tolist() and sorted(set(got["label"])) == list(range(count))
    assert float(np.abs(got["confidence"].to_numpy() - want.probabilities[keep]).max()) <= 5e-7       # six decimals in the file
