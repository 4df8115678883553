"""The exact radius graph and its connected components on the GPU: `audiossl_range_count`, `audiossl_range_fill` and
`audiossl_graph_components` against the float64 restatement of tests/range_ref.py, the Python layer above them
(src/evaluation/dedup.py) and the `find_duplicates.py` command.

Bars.  Grid (small integers, |x|^2 <= 179): every product, sum and difference is exact in fp32, so rowptr, col and d2 must EQUAL
the reference.  Real data: the worst-case bound of the fp32 chain per pair, band_ij = 2 (d + 3) 2^-24 (n_i + n_j); the three cases
have no pair whose float64 d2 lies within band_ij of r2 (asserted here on the CPU), so col must be EQUAL and |d2 - d2_64| <= band_ij;
a repeated row is at exactly 0.  Components: labels EQUAL to scipy's under the "smallest member first" numbering."""
import functools
import json

import numpy as np
import pandas as pd
import pytest
import torch

import range_ref as R

pytestmark = pytest.mark.gpu

GUARD = 2


def _ws(nbytes):
    return torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")          # the kernels clear what they need


def _launch_range(x, r2, own=None, walk=None, splits=0):
    """x [n, d] fp32 numpy (d % 4 == 0) -> (rowptr int64 [rows + 1], col int64, d2 fp32) numpy; guards behind every output, the
    workspace checked past its size, the input compared unchanged."""
    from src import _native as N
    n, d = x.shape
    own, walk = own or (0, n), walk or (0, n)
    rows = own[1] - own[0]
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    rowptr = torch.full((rows + 1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    total = torch.full((1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    nbytes = N.workspace_bytes("range_workspace", n, rows, splits)
    ws = _ws(nbytes)
    geometry = (xd, n, d, own[0], own[1], walk[0], walk[1], float(r2), splits)
    N.call("range_count", *geometry, rowptr, total, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((rowptr[rows + 1:] == -7).all()) and bool((total[1:] == -7).all()), "guard entries overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "workspace overrun"
    t = int(total[0])
    assert t == int(rowptr[rows]) and int(rowptr[0]) == 0
    col = torch.full((t + GUARD,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((t + GUARD,), -7.5, dtype=torch.float32, device="cuda")
    N.call("range_fill", *geometry, rowptr, t, col, d2, t, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((col[t:] == -7).all()) and bool((d2[t:] == -7.5).all()), "entries past total written"
    assert bool((rowptr[rows + 1:] == -7).all()) and bool((ws[nbytes:] == 0xA5).all())
    assert torch.equal(xd.cpu(), torch.from_numpy(np.array(x, dtype=np.float32))), "input changed"
    return rowptr[:rows + 1].cpu().numpy().astype(np.int64), col[:t].cpu().numpy().astype(np.int64), d2[:t].cpu().numpy()


def _launch_components(rowptr, col, n):
    """rowptr [n + 1], col numpy -> (label int64 [n], count)."""
    from src import _native as N
    cap = len(col)
    rp = torch.from_numpy(np.asarray(rowptr, dtype=np.int32)).cuda()
    cl = torch.from_numpy(np.asarray(col, dtype=np.int32)).cuda() if cap else torch.zeros(4, dtype=torch.int32, device="cuda")
    rp0, cl0 = rp.clone(), cl.clone()
    label = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    nbytes = N.workspace_bytes("graph_components_workspace", n)
    ws = _ws(nbytes)
    N.call("graph_components", rp, cl, n, cap, label, count, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((label[n:] == -7).all()) and bool((count[1:] == -7).all()) and bool((ws[nbytes:] == 0xA5).all())
    assert torch.equal(rp, rp0) and torch.equal(cl, cl0), "input changed"
    return label[:n].cpu().numpy().astype(np.int64), int(count[0])


@functools.lru_cache(maxsize=None)
def _ref_grid(r2):
    return R.radius_graph(R.grid(), r2)


@functools.lru_cache(maxsize=None)
def _ref_real(case):
    return R.radius_graph(R.real(case), R.real_r2())


@functools.lru_cache(maxsize=None)
def _gpu_grid(r2):
    return _launch_range(R.grid(), r2)


@functools.lru_cache(maxsize=None)
def _gpu_real(case):
    return _launch_range(_pad4(R.real(case)), R.real_r2())


def _pad4(x):
    d = x.shape[1]
    return x if d % 4 == 0 else np.concatenate([x, np.zeros((len(x), 4 - d % 4), dtype=x.dtype)], 1)


def _assert_exact(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2].astype(np.float64), want[2])


def _assert_real(got, want, x, own_lo=0):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    band = R.bands(x, want[0], want[1], own_lo)
    err = np.abs(got[2].astype(np.float64) - want[2])
    print(f"real n {len(x)} d {x.shape[1]}: max |d2 - fp64| / band = {float((err / band).max()):.4f}")
    assert (err <= band).all()


# ---- 1. grid: exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r2", R.GRID_RADII)
def test_grid_csr_equals_the_reference(r2):
    want = _ref_grid(r2)
    assert len(want[1]) == 2 * R.GRID_FACTS[r2][0] and int(np.diff(want[0]).max()) == R.GRID_FACTS[r2][1]
    _assert_exact(_gpu_grid(r2), want)


# ---- 2. real data ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(R.REAL_CASES)))
def test_real_cases_columns_equal_distances_within_the_chain_bound(case):
    x = R.real(case)
    n = len(x)
    gap = R.smallest_band_gap(x, R.real_r2())
    print(f"real case {case}: smallest |d2 - r2| / band = {gap:.1f}")
    assert gap > 1.0, "a pair lies within its band of the radius: pick another seed, do not widen the bar"
    want = _ref_real(case)
    assert len(want[1]) == 2 * R.REAL_FACTS[case][0] and int(np.diff(want[0]).max()) == R.REAL_FACTS[case][1]
    got = _gpu_real(case)
    _assert_real(got, want, x)
    rowptr, col, d2 = got
    for i in range(5):                                                        # the five repeated pairs, at exactly 0
        for a, b in ((i, n - 5 + i), (n - 5 + i, i)):
            row = col[rowptr[a]:rowptr[a + 1]].tolist()
            assert b in row and d2[rowptr[a] + row.index(b)] == 0.0


# ---- 3. symmetry and reproducibility ---------------------------------------------------------------------------------------
def test_symmetric_bit_for_bit_and_reproducible():
    for got, x, r2 in ((_gpu_real(0), _pad4(R.real(0)), R.real_r2()), (_gpu_grid(6.5), R.grid(), 6.5)):
        rowptr, col, d2 = got
        rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
        bits = d2.view(np.int32)
        fwd = {(int(i), int(j)): int(b) for i, j, b in zip(rows, col, bits)}
        assert len(fwd) == len(col)
        assert all(fwd.get((j, i)) == b for (i, j), b in fwd.items()), "(j, i) missing or with other bits"
        again = _launch_range(x, r2)
        assert np.array_equal(again[0], rowptr) and np.array_equal(again[1], col) and np.array_equal(again[2].view(np.int32), bits)


# ---- 4. splits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3, 7])
def test_result_does_not_depend_on_splits(splits):
    # base: splits = 0.  Real case 2 has five walked tiles: three splits walk two, two and one of them
    for base, x, r2 in ((_gpu_grid(6.5), R.grid(), 6.5), (_gpu_real(0), _pad4(R.real(0)), R.real_r2()),
                        (_gpu_real(2), _pad4(R.real(2)), R.real_r2())):
        got = _launch_range(x, r2, splits=splits)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
        assert np.array_equal(got[2].view(np.int32), base[2].view(np.int32))


# ---- 5. ranges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own,walk", [((300, 389), (0, 300)), ((37, 211), (0, 389)), ((0, 389), (101, 150))])
def test_owned_and_walked_ranges(own, walk):
    x = R.real(0)
    want = R.radius_graph(x, R.real_r2(), own, walk)
    full = _ref_real(0)                                                       # the matching slice of the full reference
    for r in range(own[0], own[1]):
        whole = full[1][full[0][r]:full[0][r + 1]]
        part = want[1][want[0][r - own[0]]:want[0][r - own[0] + 1]]
        np.testing.assert_array_equal(part, whole[(whole >= walk[0]) & (whole < walk[1])])
    assert len(want[1]) > 0
    got = _launch_range(_pad4(x), R.real_r2(), own, walk)
    _assert_real(got, want, x, own[0])


# ---- 6. tile edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 65, 127, 128, 129, 193])
def test_tile_edges_complete_graph(n):
    rowptr, col, d2 = _launch_range(R.grid()[:n], 1e9)
    np.testing.assert_array_equal(np.diff(rowptr), np.full(n, n - 1))
    want = np.concatenate([np.delete(np.arange(n), i) for i in range(n)])
    np.testing.assert_array_equal(col, want)
    np.testing.assert_array_equal(d2.astype(np.float64), R.radius_graph(R.grid()[:n], 1e9)[2])


# ---- 7. capacity and arguments ---------------------------------------------------------------------------------------------
def test_capacity_and_bad_arguments():
    from src import _native as N
    lib = N.lib()
    x = R.grid()
    n, d = x.shape
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    rowptr = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    total = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    nbytes = N.workspace_bytes("range_workspace", n, n, 0)
    ws = _ws(nbytes)
    N.call("range_count", xd, n, d, 0, n, 0, n, 6.5, 0, rowptr, total, ws, nbytes)
    torch.cuda.synchronize()
    t = int(total[0])
    assert total.dtype == torch.int64 and t == 2 * R.GRID_FACTS[6.5][0]
    col = torch.full((t,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((t,), -7.5, dtype=torch.float32, device="cuda")
    rc = lib.audiossl_range_fill(xd.data_ptr(), n, d, 0, n, 0, n, 6.5, 0, rowptr.data_ptr(), t, col.data_ptr(), d2.data_ptr(), t - 1,
                                 ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    assert rc == -1
    assert bool((col == -7).all()) and bool((d2 == -7.5).all()), "a refused fill wrote something"
    for what, got, want in R.bad_argument_codes(lib, N.workspace_bytes("range_workspace", 100, 100, 0),
                                                N.workspace_bytes("graph_components_workspace", 100)):
        assert got == want, what
    torch.cuda.synchronize()                                                  # nothing was launched: nothing can have faulted
    # a spare capacity is left alone: entries at or past total are not written
    col = torch.full((t + 50,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((t + 50,), -7.5, dtype=torch.float32, device="cuda")
    N.call("range_fill", xd, n, d, 0, n, 0, n, 6.5, 0, rowptr, t, col, d2, t + 50, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((col[t:] == -7).all()) and bool((d2[t:] == -7.5).all())
    np.testing.assert_array_equal(col[:t].cpu().numpy().astype(np.int64), _ref_grid(6.5)[1])


# ---- 8. components -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [("grid", r2) for r2 in R.GRID_RADII] + [("real", c) for c in range(len(R.REAL_CASES))])
def test_components_equal_scipy(which):
    kind, key = which
    rowptr, col, _ = _gpu_grid(key) if kind == "grid" else _gpu_real(key)
    n = len(rowptr) - 1
    want_label, want_count = R.components(rowptr, col, n)
    assert want_count == (R.GRID_FACTS[key][2] if kind == "grid" else R.REAL_FACTS[key][2])
    label, count = _launch_components(rowptr, col, n)
    assert count == want_count
    np.testing.assert_array_equal(label, want_label)


def test_components_path_star_empty_and_repeat():
    x = R.path()
    rowptr, col, d2 = _launch_range(x, 1.5)
    _assert_exact((rowptr, col, d2), R.radius_graph(x, 1.5))
    label, count = _launch_components(rowptr, col, 1000)                      # one component of diameter 999 under shuffled ids
    assert count == 1 and (label == 0).all()
    again = _launch_components(rowptr, col, 1000)
    assert again[1] == 1 and np.array_equal(again[0], label)
    # half the path: two components, numbered by smallest member
    cut = int(x[:, 0].tolist().index(500.0))
    keep = (col != cut) & (np.repeat(np.arange(1000), np.diff(rowptr)) != cut)
    rp2 = np.zeros(1001, dtype=np.int64)
    np.add.at(rp2, np.repeat(np.arange(1000), np.diff(rowptr))[keep] + 1, 1)
    rp2 = np.cumsum(rp2)
    want = R.components(rp2, col[keep], 1000)
    got = _launch_components(rp2, col[keep], 1000)
    assert want[1] == 3 and got[1] == 3
    np.testing.assert_array_equal(got[0], want[0])
    # the empty graph
    label, count = _launch_components(np.zeros(601, dtype=np.int64), np.zeros(0, dtype=np.int64), 600)
    assert count == 600 and np.array_equal(label, np.arange(600))
    # a star: both directions stored, and only the hub's row
    for both in (True, False):
        rp, cl = R.star(600, both)
        assert rp[1] == 599
        label, count = _launch_components(rp, cl, 600)
        assert count == 1 and (label == 0).all()
    # a hub that is not the smallest member, columns out of range skipped, rowptr clamped to cap
    rp = np.array([0, 0, 0, 4, 4, 4, 9], dtype=np.int64)                      # row 5 claims entries 4..8, cap is 6
    cl = np.array([4, 1, -3, 77, 0, 3], dtype=np.int64)
    label, count = _launch_components(rp, cl, 6)
    assert label.tolist() == [0, 1, 1, 0, 1, 0] and count == 2


# ---- 9. the Python layer ---------------------------------------------------------------------------------------------------
def test_near_duplicates_range_search_and_the_edge_limit():
    from src.evaluation import dedup as D
    x = R.real(0)
    n = len(x)
    rowptr, col, d2 = _ref_real(0)
    want_group, want_count = R.components(rowptr, col, n)
    degree = np.diff(rowptr)
    near, best = R.nearest(rowptr, col, d2)
    # the reference's nearest is beyond fp32's reach of change: best and second best differ by more than two bands or are equal
    band = R.bands(x, rowptr, col)
    for i in range(n):
        s = np.sort(d2[rowptr[i]:rowptr[i + 1]])
        if len(s) >= 2 and s[1] != s[0]:
            assert s[1] - s[0] > 2 * band[rowptr[i]:rowptr[i + 1]].max()
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    for mode, want_keep in (("first", R.keep_first(want_group)), ("central", R.keep_central(want_group, degree))):
        dup = D.near_duplicates(xd, threshold=R.REAL_TAU, metric="cosine", keep=mode, normalize=False)
        assert dup.n_groups == want_count
        np.testing.assert_array_equal(dup.group, want_group)
        np.testing.assert_array_equal(dup.size, np.bincount(want_group)[want_group])
        np.testing.assert_array_equal(dup.degree, degree)
        np.testing.assert_array_equal(dup.nearest, near)
        np.testing.assert_array_equal(dup.keep, want_keep)
        has = near >= 0
        assert np.isnan(dup.nearest_sim[~has]).all()
        assert float(np.abs(dup.nearest_sim[has] - (1.0 - 0.5 * best[has])).max()) <= 1e-5
        np.testing.assert_array_equal(dup.csr.col.cpu().numpy().astype(np.int64), col)
    assert (R.keep_central(want_group, degree) != R.keep_first(want_group)).any()       # the two modes do differ on this case
    # width 36 needs no padding, 30 does: range_graph pads with zero columns
    got = D.range_graph(xd[:, :30].contiguous(), 0.15)
    want = R.radius_graph(x[:, :30], 0.15)
    assert R.smallest_band_gap(x[:, :30], 0.15) > 1.0
    np.testing.assert_array_equal(got.col.cpu().numpy().astype(np.int64), want[1])
    # range_search = owned [300, 389) against walked [0, 300), columns bank-relative
    want = R.radius_graph(x, R.real_r2(), (300, 389), (0, 300))
    got = D.range_search(xd[300:], xd[:300], R.real_r2())
    np.testing.assert_array_equal(got.rowptr.cpu().numpy().astype(np.int64), want[0])
    np.testing.assert_array_equal(got.col.cpu().numpy().astype(np.int64), want[1])
    assert (np.abs(got.d2.cpu().numpy().astype(np.float64) - want[2]) <= R.bands(x, want[0], want[1], 300)).all()
    # too loose a threshold
    g = torch.from_numpy(np.array(R.grid(), dtype=np.float32)).cuda()
    with pytest.raises(ValueError, match=r"total = 110556 .* max_edges = 1000.*too loose"):
        D.range_graph(g, 1e9, max_edges=1000)
    with pytest.raises(ValueError, match="total = 110556"):
        D.range_graph(g, 1e9)                                                 # the default: 64 per row
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.range_graph(g.cpu(), 1.0)
    label, count = D.graph_components(got.rowptr.new_zeros(11), got.col[:0], 10)
    assert count == 10 and label.tolist() == list(range(10))


# ---- 10. the command -------------------------------------------------------------------------------------------------------
def test_find_duplicates_command(tmp_path, capsys):
    import find_duplicates as FD
    x = R.real(0)
    n = len(x)
    paths = [f"/data/clip_{i:04d}.wav" for i in range(n)]
    labels = [f"class{i % 7}" for i in range(n)]
    frame = pd.DataFrame({"wav": paths, "label": labels, "fold": np.arange(n) % 5})
    csv, emb = str(tmp_path / "all.csv"), str(tmp_path / "all.npy")
    frame.to_csv(csv, index=False)
    np.save(emb, 3.0 * x)                                                     # the command normalises
    rowptr, col, d2 = _ref_real(0)
    group, count = R.components(rowptr, col, n)
    degree = np.diff(rowptr)
    size = np.bincount(group)[group]
    near, best = R.nearest(rowptr, col, d2)
    out, groups = str(tmp_path / "kept.csv"), str(tmp_path / "groups.csv")
    for mode, keep in (("first", R.keep_first(group)), ("central", R.keep_central(group, degree))):
        res = FD.main(FD.get_args(["--input", csv, "--embeddings", emb, "--threshold", str(R.REAL_TAU), "--keep", mode, "--out", out,
                                   "--groups", groups]))
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line == res
        assert res == dict(N=n, N_against=0, threshold=R.REAL_TAU, edges=len(col), groups=int((np.bincount(group) >= 2).sum()),
                           removed=int((~keep).sum()), largest_group=int(size.max()), max_degree=int(degree.max()), d=36)
        kept = pd.read_csv(out)
        assert list(kept.columns) == ["wav", "label", "fold"]
        assert list(kept["wav"]) == [p for p, k in zip(paths, keep) if k]
        assert list(kept["label"]) == [l for l, k in zip(labels, keep) if k]
        got = pd.read_csv(groups)
        rows = np.flatnonzero(size >= 2)
        assert list(got.columns) == FD.GROUP_COLUMNS
        assert list(got["files"]) == [paths[i] for i in rows] and list(got["group"]) == group[rows].tolist()
        assert list(got["size"]) == size[rows].tolist() and list(got["kept"]) == keep[rows].astype(int).tolist()
        assert list(got["nearest"]) == [paths[near[i]] for i in rows]
        assert float(np.abs(got["similarity"].to_numpy() - (1.0 - 0.5 * best[rows])).max()) <= 1e-5
    # leakage: rows 300.. against rows ..299, a `files` list this time
    a_csv, b_csv = str(tmp_path / "new.csv"), str(tmp_path / "old.csv")
    pd.DataFrame({"files": paths[300:], "source": ["web"] * (n - 300)}).to_csv(a_csv, index=False)
    pd.DataFrame({"files": paths[:300]}).to_csv(b_csv, index=False)
    a_emb, b_emb = str(tmp_path / "new.npy"), str(tmp_path / "old.npy")
    np.save(a_emb, x[300:])
    np.save(b_emb, 0.5 * x[:300])
    want = R.radius_graph(x, R.real_r2(), (300, n), (0, 300))
    wdeg = np.diff(want[0])
    wnear, wbest = R.nearest(want[0], want[1], want[2])
    res = FD.main(FD.get_args(["--input", a_csv, "--against", b_csv, "--embeddings", a_emb, "--against_embeddings", b_emb,
                               "--threshold", str(R.REAL_TAU), "--out", out, "--groups", groups]))
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    leaking = int((wdeg > 0).sum())
    assert leaking >= 5                                                       # the five repeated clips at least
    assert res == dict(N=n - 300, N_against=300, threshold=R.REAL_TAU, edges=len(want[1]), groups=leaking, removed=leaking,
                       largest_group=int(wdeg.max()), max_degree=int(wdeg.max()), d=36)
    kept = pd.read_csv(out)
    assert list(kept.columns) == ["files", "source"] and list(kept["files"]) == [paths[300 + i] for i in np.flatnonzero(wdeg == 0)]
    got = pd.read_csv(groups)
    rows = np.flatnonzero(wdeg > 0)
    assert list(got.columns) == FD.LEAK_COLUMNS and list(got["files"]) == [paths[300 + i] for i in rows]
    assert list(got["matches"]) == wdeg[rows].tolist() and list(got["nearest"]) == [paths[wnear[i]] for i in rows]
    assert float(np.abs(got["similarity"].to_numpy() - (1.0 - 0.5 * wbest[rows])).max()) <= 1e-5
    for i in range(5):                                                        # clip n - 5 + i repeats clip i
        r = got[got["files"] == paths[n - 5 + i]]
        assert len(r) == 1 and r["nearest"].iloc[0] == paths[i] and abs(r["similarity"].iloc[0] - 1.0) <= 1e-6
