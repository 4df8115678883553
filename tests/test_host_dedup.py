"""CPU: the float64 restatement of the radius graph (tests/range_ref.py) against sklearn, the host half of the duplicate search
(`cosine_to_radius2`, `select_keep`), the CSV writers and argument checks of `find_duplicates.py`, and the argument validation of
the range / components entry points (no launch)."""
import os

import numpy as np
import pandas as pd
import pytest

import range_ref as R


def test_reference_matches_sklearn_radius_neighbors_graph():
    from sklearn.neighbors import radius_neighbors_graph
    x = R.real(0)
    r2 = R.real_r2()
    rowptr, col, d2 = R.radius_graph(x, r2)
    g = radius_neighbors_graph(x.astype(np.float64), radius=np.sqrt(r2), mode="distance", include_self=False)
    g.sort_indices()
    # sklearn leaves a repeated row's zero distance in the structure (explicit zeros): the same pairs
    np.testing.assert_array_equal(g.indptr.astype(np.int64), rowptr)
    np.testing.assert_array_equal(g.indices.astype(np.int64), col)
    np.testing.assert_allclose(g.data ** 2, d2, rtol=0, atol=1e-12)
    assert R.smallest_band_gap(x, r2) > 1.0                                   # no pair sits on the radius: the comparison is fair


def test_reference_facts():
    """The inputs are the ones the expected counts were recorded for (edges are undirected: two stored entries each)."""
    x = R.grid()
    assert float((x.astype(np.float64) ** 2).sum(1).max()) <= 179 and (x == np.round(x)).all()
    for r2 in R.GRID_RADII:
        rowptr, col, _ = R.radius_graph(x, r2)
        label, count = R.components(rowptr, col, len(x))
        assert (len(col) // 2, int(np.diff(rowptr).max()), count, int(np.bincount(label).max())) == R.GRID_FACTS[r2]
    for case in range(len(R.REAL_CASES)):
        x = R.real(case)
        rowptr, col, d2 = R.radius_graph(x, R.real_r2())
        _, count = R.components(rowptr, col, len(x))
        assert (len(col) // 2, int(np.diff(rowptr).max()), count) == R.REAL_FACTS[case]
    rowptr, col, _ = R.radius_graph(R.path(), 1.5)
    assert len(col) == 2 * 999 and R.components(rowptr, col, 1000)[1] == 1


def test_renumber_orders_components_by_smallest_member():
    assert R.renumber([7, 7, 2, 9, 2, 7]).tolist() == [0, 0, 1, 2, 1, 0]
    rowptr, col = R.star(6, both=False)
    label, count = R.components(rowptr, col, 6)
    assert count == 1 and label.tolist() == [0] * 6


def test_cosine_to_radius2():
    from src.evaluation.dedup import cosine_to_radius2
    assert cosine_to_radius2(1.0) == 0.0
    assert cosine_to_radius2(0.5) == 1.0
    assert cosine_to_radius2(0.9) == float(np.float32(2 - 2 * 0.9)) == R.real_r2()
    assert cosine_to_radius2(0.98) == float(np.float32(0.04000000000000003))
    for bad in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            cosine_to_radius2(bad)


def test_select_keep_first_and_central_with_ties():
    from src.evaluation.dedup import select_keep
    group = np.array([0, 1, 0, 2, 1, 0, 3, 1])
    degree = np.array([1, 2, 2, 0, 2, 2, 0, 1])
    assert select_keep(group, degree, "first").tolist() == [True, True, False, True, False, False, True, False]
    # group 0: rows 2 and 5 tie at degree 2 -> 2; group 1: rows 1 and 4 tie -> 1; singletons stay
    assert select_keep(group, degree, "central").tolist() == [False, True, True, True, False, False, True, False]
    np.testing.assert_array_equal(select_keep(group, degree, "first"), R.keep_first(group))
    np.testing.assert_array_equal(select_keep(group, degree, "central"), R.keep_central(group, degree))
    g = np.random.default_rng(3)
    group, degree = g.integers(0, 40, 500), g.integers(0, 4, 500)
    np.testing.assert_array_equal(select_keep(group, degree, "first"), R.keep_first(group))
    np.testing.assert_array_equal(select_keep(group, degree, "central"), R.keep_central(group, degree))
    assert select_keep([], [], "first").tolist() == []
    with pytest.raises(ValueError):
        select_keep(group, degree, "last")
    with pytest.raises(ValueError):
        select_keep(group, degree[:-1], "first")


def test_path_column_and_writers(tmp_path):
    import find_duplicates as FD
    from src.evaluation.dedup import Duplicates
    assert FD.path_column(pd.DataFrame({"wav": ["a"], "label": [1]}), "x.csv") == "wav"
    assert FD.path_column(pd.DataFrame({"label": [1], "files": ["a"], "wav": ["b"]}), "x.csv") == "files"
    with pytest.raises(ValueError, match="neither"):
        FD.path_column(pd.DataFrame({"path": ["a"]}), "x.csv")
    frame = pd.DataFrame({"wav": ["a.wav", "b.wav", "c.wav", "d.wav"], "label": ["dog", "cat", "dog", "owl"], "fold": [1, 2, 3, 4]})
    keep = np.array([True, False, True, True])
    FD.write_kept(frame, keep, tmp_path / "kept.csv")
    back = pd.read_csv(tmp_path / "kept.csv")
    assert list(back.columns) == ["wav", "label", "fold"] and list(back["wav"]) == ["a.wav", "c.wav", "d.wav"]
    assert list(back["label"]) == ["dog", "dog", "owl"] and list(back["fold"]) == [1, 3, 4]
    dup = Duplicates(group=np.array([0, 0, 1, 2]), n_groups=3, size=np.array([2, 2, 1, 1]), degree=np.array([1, 1, 0, 0]), keep=keep,
                     nearest=np.array([1, 0, -1, -1]), nearest_sim=np.array([0.99, 0.99, np.nan, np.nan]), csr=None)
    FD.write_groups(list(frame["wav"]), dup, tmp_path / "groups.csv")
    got = pd.read_csv(tmp_path / "groups.csv")
    assert list(got.columns) == FD.GROUP_COLUMNS
    assert got.values.tolist() == [["a.wav", 0, 2, 1, "b.wav", 0.99], ["b.wav", 0, 2, 0, "a.wav", 0.99]]
    FD.write_leaks(list(frame["wav"]), ["t0.wav", "t1.wav"], np.array([0, 2, 0, 1]), np.array([-1, 1, -1, 0]),
                   np.array([np.nan, 1.0, np.nan, 0.95]), tmp_path / "leaks.csv")
    got = pd.read_csv(tmp_path / "leaks.csv")
    assert list(got.columns) == FD.LEAK_COLUMNS
    assert got.values.tolist() == [["b.wav", 2, "t1.wav", 1.0], ["d.wav", 1, "t0.wav", 0.95]]


def test_command_refuses_bad_arguments_before_the_gpu(tmp_path):
    import find_duplicates as FD
    csv = str(tmp_path / "in.csv")
    pd.DataFrame({"files": ["a", "b", "c"]}).to_csv(csv, index=False)
    np.save(tmp_path / "x.npy", np.zeros((3, 8), dtype=np.float32))
    np.save(tmp_path / "short.npy", np.zeros((2, 8), dtype=np.float32))
    np.save(tmp_path / "wide.npy", np.zeros((3, 12), dtype=np.float32))
    x, out = str(tmp_path / "x.npy"), str(tmp_path / "out.csv")
    base = ["--input", csv, "--out", out]
    with pytest.raises(SystemExit):
        FD.get_args(["--input", csv])                                         # --out is required
    with pytest.raises(SystemExit):
        FD.get_args(base + ["--window", "random"])                            # only deterministic windows
    bad = [([], "--checkpoint"),
           (["--embeddings", x, "--threshold", "0"], "threshold"),
           (["--embeddings", x, "--threshold", "1.5"], "threshold"),
           (["--embeddings", x, "--against_embeddings", x], "--against"),
           (["--checkpoint", "c.ckpt", "--against", csv, "--against_embeddings", x], "--embeddings"),
           (["--embeddings", x, "--against", csv], "--against_embeddings"),
           (["--embeddings", x, "--dump_embeddings", str(tmp_path)], "exclude"),
           (["--embeddings", x, "--max_edges", "-3"], "max_edges"),
           (["--embeddings", str(tmp_path / "short.npy")], "3 rows"),
           (["--embeddings", x, "--against", csv, "--against_embeddings", str(tmp_path / "wide.npy")], "width")]
    for extra, word in bad:
        with pytest.raises(ValueError, match=word):
            FD.main(FD.get_args(base + extra))
    assert not os.path.exists(out)
    nopath = str(tmp_path / "nopath.csv")
    pd.DataFrame({"path": ["a"]}).to_csv(nopath, index=False)
    with pytest.raises(ValueError, match="neither"):
        FD.main(FD.get_args(["--input", nopath, "--out", out, "--embeddings", x]))


def test_entries_refuse_bad_arguments_before_any_launch():
    from src import _native as N
    lib = N.lib()
    ws = N.workspace_bytes("range_workspace", 100, 100, 0)
    cc = N.workspace_bytes("graph_components_workspace", 100)
    for what, got, want in R.bad_argument_codes(lib, ws, cc):
        assert got == want, what
    # the workspace figure is non-decreasing in each argument, and a forced split count also serves the library's own choice
    prev = 0
    for splits in range(0, 65):
        cur = N.workspace_bytes("range_workspace", 70000, 65536, splits)
        assert cur >= prev
        prev = cur
    sizes = [N.workspace_bytes("range_workspace", 5000, rows, 0) for rows in (1, 64, 65, 1000, 5000)]
    assert sizes == sorted(sizes)
    sizes = [N.workspace_bytes("range_workspace", n, 100, 3) for n in (100, 101, 5000, 1 << 20)]
    assert sizes == sorted(sizes)
    sizes = [N.workspace_bytes("graph_components_workspace", n) for n in (1, 2, 1000, 1 << 20)]
    assert sizes == sorted(sizes)
