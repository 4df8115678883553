"""CPU: the host stage of HDBSCAN (src/evaluation/hdbscan.py: tree -> dendrogram -> condensed tree -> excess of mass -> labels and
probabilities) against sklearn's `HDBSCAN(algorithm="brute")` and the plain restatement of tests/hdbscan_ref.py, fed with the
scipy minimum spanning tree of the fp64 mutual-reachability matrix.  Both sides are fp64 on the same tree: labels must agree as
partitions (ARI exactly 1.0, equal noise sets and cluster counts), probabilities within 1e-9."""
import numpy as np
import pytest
import torch

import hdbscan_ref as R
from src.evaluation import hdbscan as H


def _tree(case):
    ms = R.CASES[case][5]
    w2, _ = R.mutual_reachability2(R.case_points(case), ms)
    return R.scipy_mst(np.sqrt(w2))


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_host_stage_equals_sklearn(case):
    x = R.case_points(case)
    n, mcs = len(x), R.CASES[case][6]
    want, want_prob = R.sklearn_answer(case)
    assert (int(want.max()) + 1, int((want < 0).sum())) == R.CASE_FACTS[case]
    u, v, w = _tree(case)
    labels, prob, count = H.hdbscan_from_mst(u, v, w, n, mcs)
    print(f"case {case}: n {n}, {count} clusters, {int((labels < 0).sum())} noise, "
          f"max |p - sklearn| = {float(np.abs(prob - want_prob).max()):.3e}")
    assert count == R.CASE_FACTS[case][0]
    R.assert_same_clustering(labels, want)
    assert float(np.abs(prob - want_prob).max()) <= 1e-9
    # numbered by smallest member
    first = [int(np.flatnonzero(labels == c)[0]) for c in range(count)]
    assert first == sorted(first)
    # the plain restatement says the same, and so does the unique tree of Kruskal under (w, lo, hi)
    pl, pp, pc = R.hdbscan_plain(u, v, w, n, mcs)
    assert pc == count and np.array_equal(pl, labels) and float(np.abs(pp - prob).max()) <= 1e-12
    ku, kv, kw = R.kruskal(np.sqrt(R.mutual_reachability2(x, R.CASES[case][5])[0]))
    np.testing.assert_allclose(np.sort(kw), np.sort(w), rtol=0, atol=0)
    kl, kp, _ = H.hdbscan_from_mst(ku, kv, kw, n, mcs)
    assert np.array_equal(kl, labels) and np.array_equal(kp, prob)


def test_death_is_taken_over_the_cluster_itself_not_its_descendants():
    # case 2 is the one where a maximum over descendants gives other probabilities: pin sklearn's rule on it
    x = R.case_points(2)
    u, v, w = _tree(2)
    tree = H.condense_tree(H.single_linkage(u, v, w, len(x)), R.CASES[2][6])
    selected = H.select_eom(tree)
    labels, prob = H.label_points(tree, selected)
    n = len(x)
    over = 0
    for c in selected:
        rows = np.flatnonzero(tree.parent == c)
        death = tree.lam[rows].max()
        inside = [c]
        for k in inside:
            inside += tree.child[(tree.parent == k) & (tree.child >= n)].tolist()
        deepest = max(tree.lam[tree.parent == k].max() for k in inside)
        over += int(deepest > death)
        pts = np.flatnonzero(labels == labels[tree.child[rows][tree.child[rows] < n][0]])
        lam_p = np.empty(n)
        lam_p[tree.child[tree.child < n]] = tree.lam[tree.child < n]
        np.testing.assert_allclose(prob[pts], np.minimum(lam_p[pts], death) / death, rtol=0, atol=1e-15)
    assert over >= 1, "no selected cluster of this case has a deeper descendant: the case pins nothing"


def test_min_cluster_size_above_every_blob_gives_all_noise():
    x = R.case_points(0)
    u, v, w = _tree(0)
    labels, prob, count = H.hdbscan_from_mst(u, v, w, len(x), 150)
    assert count == 0 and (labels == -1).all() and (prob == 0).all()


def test_single_linkage_merges_in_weight_order():
    u, v, w = _tree(2)
    n = len(R.case_points(2))
    z = H.single_linkage(u, v, w, n)
    assert (np.diff(z.dist) >= 0).all() and z.size[-1] == n
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    w2, _ = R.mutual_reachability2(R.case_points(2), R.CASES[2][5])
    m = np.sqrt(w2)
    np.fill_diagonal(m, 0.0)
    want = linkage(squareform(m, checks=False), "single")
    np.testing.assert_allclose(z.dist, want[:, 2], rtol=1e-12, atol=0)
    # core distances make equal weights common, and inside a run of equal weights the merge order is free: sizes must agree
    # wherever a run ends (the partition at a threshold does not depend on the order inside the run)
    ends = np.r_[z.dist[1:] != z.dist[:-1], True]
    assert ends.sum() > 50
    def partition_sizes(left, right, t_end):
        parent = list(range(2 * n - 1))
        for t in range(t_end + 1):
            parent[int(left[t])] = parent[int(right[t])] = n + t
        roots = []
        for p in range(n):
            while parent[p] != p:
                p = parent[p]
            roots.append(p)
        return sorted(np.unique(roots, return_counts=True)[1].tolist())
    for t in np.flatnonzero(ends)[::10]:
        assert partition_sizes(z.left, z.right, t) == partition_sizes(want[:, 0], want[:, 1], t)


@pytest.mark.parametrize("case,radius2", [(0, 0.6), (0, 2.5), (2, 0.05), (2, 0.4)])
def test_cut_mst_equals_components_of_the_thresholded_matrix(case, radius2):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    x = R.case_points(case)
    d2 = R.sq_dists(np.asarray(x, dtype=np.float32))
    d2 = d2.astype(np.float32).astype(np.float64)                            # cut_mst compares in fp32
    u, v, w2 = R.kruskal(d2)
    count, want = connected_components(csr_matrix((d2 <= float(np.float32(radius2))) & ~np.eye(len(x), dtype=bool)), directed=False)
    assert 1 < count < len(x)
    got = H.cut_mst(H.MstEdges(u, v, w2), len(x), radius2)
    np.testing.assert_array_equal(got, R.renumber(want))
    got_t = H.cut_mst(H.MstEdges(torch.from_numpy(u), torch.from_numpy(v), torch.from_numpy(w2.astype(np.float32))), len(x), radius2)
    np.testing.assert_array_equal(got_t, got)


def test_argument_checks():
    u, v, w = _tree(2)
    n = len(R.case_points(2))
    with pytest.raises(ValueError, match="min_cluster_size must be at least 2"):
        H.hdbscan_from_mst(u, v, w, n, 1)
    with pytest.raises(ValueError, match="min_cluster_size must be at least 2"):
        H.hdbscan(torch.zeros(10, 4), min_cluster_size=1)
    with pytest.raises(ValueError, match=f"has {n - 1} edges"):
        H.single_linkage(u[:-1], v[:-1], w[:-1], n)
    with pytest.raises(ValueError, match="cycle"):
        H.single_linkage(np.r_[u[:-1], u[0]], np.r_[v[:-1], v[0]], w, n)
    with pytest.raises(ValueError, match=r"must lie in \[0"):
        H.single_linkage(u, np.r_[v[:-1], n], w, n)
    with pytest.raises(ValueError, match="weights must be >= 0"):
        H.single_linkage(u, v, np.r_[w[:-1], np.nan], n)
    with pytest.raises(ValueError, match="radius2 must be >= 0"):
        H.cut_mst((u, v, w), n, -1.0)
    x = torch.zeros(10, 8)
    for bad in (0, 66, 11):
        with pytest.raises(ValueError, match="min_samples"):
            H.core_distances2(x, bad)
        with pytest.raises(ValueError, match="min_samples"):
            H.mutual_reachability_mst(x, bad)
    with pytest.raises(ValueError, match="splits must be in"):
        H.mutual_reachability_mst(x, 1, splits=65)
    with pytest.raises(ValueError, match="at least 2 points"):
        H.mutual_reachability_mst(x[:1])
    with pytest.raises(ValueError, match="points are"):
        H.core_distances2(x[0], 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.core_distances2(x, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.mutual_reachability_mst(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.hdbscan(x)


def test_labeler_command_line_admits_hdbscan(capsys):
    from src.upstream.decar_v2 import store_clusters as sc
    base = ["--checkpoint", "c", "--input", "f.csv", "--out", "o.csv"]
    a = sc.get_args(base + ["--clustering", "hdbscan"])
    assert (a.clustering, a.min_cluster_size, a.min_samples, a.drop_unreached, a.confidence, a.k) == ("hdbscan", 25, 5, False, False, None)
    a = sc.get_args(base + ["--clustering", "hdbscan", "--min_cluster_size", "10", "--min_samples", "3", "--drop_unreached", "--confidence",
                            "--score", "--map", "m.csv"])
    assert (a.min_cluster_size, a.min_samples, a.drop_unreached, a.confidence, a.score, a.map) == (10, 3, True, True, True, "m.csv")
    capsys.readouterr()
    h = base + ["--clustering", "hdbscan"]
    for argv in (h + ["--k", "9"], h + ["--k_sweep", "4,8"], h + ["--seed_labels", "few.csv"], h + ["--min_cluster_size", "1"],
                 h + ["--min_samples", "0"], h + ["--min_samples", "66"],
                 base + ["--k", "9", "--drop_unreached"], base + ["--clustering", "pic", "--confidence"]):      # still tied to spread / hdbscan
        with pytest.raises(SystemExit) as e:
            sc.get_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    import src.evaluation as E
    import types
    assert isinstance(E.hdbscan, types.ModuleType) and E.mutual_reachability_mst is H.mutual_reachability_mst


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes
    from src import _native as N
    lib = N.lib()
    P, BIG, n, d = 4096, 1 << 30, 100, 32
    m, w = lib.audiossl_mreach_mst, lib.audiossl_mreach_mst_workspace
    b = ctypes.c_long(0)
    assert w(n, 0, ctypes.addressof(b)) == 0 and b.value > 0
    need = b.value
    assert w(n, 64, ctypes.addressof(b)) == 0 and b.value >= need
    assert w(1, 0, ctypes.addressof(b)) == -1 and w(n, 65, ctypes.addressof(b)) == -1 and w(n, -1, ctypes.addressof(b)) == -1
    assert w(n, 0, None) == -1
    assert m(P, 1, d, P, 0, P, P, P, P, P, BIG, None) == -1                    # n = 1
    assert m(P, n, 30, P, 0, P, P, P, P, P, BIG, None) == -1                   # d % 4
    assert m(P, n, 0, P, 0, P, P, P, P, P, BIG, None) == -1
    assert m(P, n, 4100, P, 0, P, P, P, P, P, BIG, None) == -1
    assert m(P, n, d, P, 65, P, P, P, P, P, BIG, None) == -1                   # splits
    assert m(P, n, d, P, -1, P, P, P, P, P, BIG, None) == -1
    assert m(P, n, d, P, 0, P, P, P, P, P, need - 1, None) == -1               # short workspace
    assert m(None, n, d, P, 0, P, P, P, P, P, BIG, None) == -1
    assert m(P, n, d, P, 0, None, P, P, P, P, BIG, None) == -1
    assert m(P, n, d, P, 0, P, None, P, P, P, BIG, None) == -1
    assert m(P, n, d, P, 0, P, P, None, P, P, BIG, None) == -1
    assert m(P, n, d, P, 0, P, P, P, P, None, BIG, None) == -1
    assert m(P + 4, n, d, P, 0, P, P, P, P, P, BIG, None) == -3                # misaligned x
    assert m(P, n, d, P, 0, P, P, P, P, P + 8, BIG, None) == -3                # misaligned workspace
