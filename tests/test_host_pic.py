"""CPU: the float64 restatement of PIC (tests/pic_ref.py) against what the reference's own code recorded
(tests/golden/pic_reference.npz), the host-side pieces of `src.upstream.decar_v2.clustering.PIC` (singleton rule, numbering),
`partition_nmi` against sklearn, and the labeler's command line."""
import os

import numpy as np
import pytest
import torch

import pic_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pic_reference.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN, allow_pickle=False)


def test_pic_is_part_of_the_labeler():
    from src.upstream.decar_v2 import clustering as CL
    from src.upstream.decar_v2.clustering import PIC
    p = PIC()
    assert (p.sigma, p.nnn, p.alpha, p.distribute_singletons) == (0.2, 5, 0.001, True)
    for name in ("make_graph", "make_adjacencyW", "run_pic", "find_maxima_cluster", "Kmeans", "rearrange_clusters"):
        assert callable(getattr(CL, name)), name


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_restatement_reproduces_the_reference(gold, case):
    n, dim, centres = R.CASES[case]
    x, I, D = gold[f"x_{case}"], gold[f"I_{case}"], gold[f"D_{case}"]
    assert x.shape == (n, dim) and x.dtype == np.float32 and I.shape == (n, R.NNN + 1)
    np.testing.assert_array_equal(x, R.blobs(n, dim, centres, int(gold[f"seed_{case}"])))
    I2, D2 = R.make_graph(x, R.NNN)
    np.testing.assert_array_equal(I, I2)
    np.testing.assert_array_equal(D, D2)
    raw, final, margin = R.pic(I, D)
    # the reference numbers its final clusters through a Python set: partitions are compared after renumbering by first appearance
    np.testing.assert_array_equal(R.renumber(raw), R.renumber(gold[f"raw_{case}"]))
    np.testing.assert_array_equal(final, R.renumber(gold[f"final_{case}"]))
    assert margin >= 1e-4 and abs(margin - float(gold[f"margin_{case}"])) <= 1e-9
    # raw ids number the roots in ascending node order: 0..C-1 are all used
    assert raw.max() + 1 == len(set(gold[f"raw_{case}"].tolist()))


def test_fixture_counts(gold):
    raw = [len(set(gold[f"raw_{c}"].tolist())) for c in range(3)]
    final = [len(set(gold[f"final_{c}"].tolist())) for c in range(3)]
    assert raw == [4, 15, 37] and final == [4, 14, 37]


def test_csr_is_canonical(gold):
    rowptr, col, w = R.adjacency(gold["I_1"], gold["D_1"], R.SIGMA)
    n = len(rowptr) - 1
    dense = np.zeros((n, n))
    a = np.exp(-gold["D_1"][:, 1:].astype(np.float64) / R.SIGMA ** 2)
    for i in range(n):
        dense[i, gold["I_1"][i, 1:]] = a[i]
    dense = dense + dense.T
    got = np.zeros((n, n))
    for i in range(n):
        cols = col[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(cols) > 0).all()
        got[i, cols] = w[rowptr[i]:rowptr[i + 1]]
    np.testing.assert_array_equal(got, dense)


def test_ring_graph_gives_one_cluster_per_node():
    """I = (i, i + 1, i - 1) with equal distances: W is a circulant, v stays uniform, no value is positive, every node is a root."""
    n = 12
    i = np.arange(n)
    I = np.stack([i, (i + 1) % n, (i - 1) % n], 1)
    D = np.concatenate([np.zeros((n, 1)), np.full((n, 2), 0.3)], 1).astype(np.float32)
    raw, final, _ = R.pic(I, D, distribute=False)
    assert len(set(raw.tolist())) == n and np.array_equal(final, np.arange(n))


def _singleton_cases():
    # 6 nodes: clusters {0, 1}, {2} (singleton), {3, 4}, {5} (singleton)
    clust = np.array([7, 7, 3, 9, 9, 1])
    I = np.array([[0, 1, 2], [1, 0, 2], [2, 5, 3], [3, 4, 2], [4, 3, 5], [5, 2, 0]])
    # node 2: first neighbour 5 is a singleton -> skipped, second neighbour 3 -> cluster 9
    # node 5: first neighbour 2 WAS a singleton in the original clustering -> skipped although 2 has moved; then 0 -> cluster 7
    want = np.array([7, 7, 9, 9, 9, 7])
    yield clust, I, want
    # a singleton whose neighbours are all singletons stays
    clust = np.array([0, 1, 2, 2])
    I = np.array([[0, 1], [1, 0], [2, 3], [3, 2]])
    yield clust, I, clust.copy()


def test_singleton_rule_and_numbering():
    from src.upstream.decar_v2.clustering import distribute_singletons, lists_from_labels
    for clust, I, want in _singleton_cases():
        np.testing.assert_array_equal(R.singletons(clust, I), want)
        np.testing.assert_array_equal(distribute_singletons(clust, I), want)
        np.testing.assert_array_equal(distribute_singletons(clust, torch.from_numpy(I)), want)
    # numbering: ascending smallest member, members ascending - whatever the label values are
    lists = lists_from_labels([5, 2, 5, 9, 2, 0])
    assert lists == [[0, 2], [1, 4], [3], [5]]
    np.testing.assert_array_equal(R.renumber([5, 2, 5, 9, 2, 0]), [0, 1, 0, 2, 1, 3])
    from src.upstream.decar_v2.clustering import rearrange_clusters
    np.testing.assert_array_equal(rearrange_clusters(lists), [0, 1, 0, 2, 1, 3])


def test_singleton_rule_on_the_fixture(gold):
    from src.upstream.decar_v2.clustering import distribute_singletons, lists_from_labels, rearrange_clusters
    for case in range(3):
        moved = distribute_singletons(gold[f"raw_{case}"], gold[f"I_{case}"])
        labels = rearrange_clusters(lists_from_labels(moved))
        np.testing.assert_array_equal(labels, R.renumber(gold[f"final_{case}"]))


def test_partition_nmi_matches_sklearn():
    from sklearn.metrics import normalized_mutual_info_score
    from src.evaluation.graph import partition_nmi
    g = np.random.RandomState(0)
    cases = [(g.randint(7, size=500), g.randint(5, size=500)),
             (g.randint(3, size=64), g.randint(40, size=64)),
             (np.zeros(100, dtype=np.int64), g.randint(9, size=100)),            # one cluster against many
             (g.randint(9, size=100), np.zeros(100, dtype=np.int64)),
             (np.zeros(10, dtype=np.int64), np.ones(10, dtype=np.int64)),         # one against one
             (np.arange(50), np.arange(50)[::-1].copy()),                         # all singletons: identical partitions
             (g.randint(4, size=300) * 10 - 7, g.randint(4, size=300))]           # label values are arbitrary
    a = g.randint(6, size=400)
    cases.append((a, (a + (g.rand(400) < 0.1)) % 6))                              # nearly equal
    for a, b in cases:
        want = normalized_mutual_info_score(a, b)
        assert abs(partition_nmi(a, b) - want) <= 1e-12, (want, partition_nmi(a, b))
        assert abs(partition_nmi(torch.from_numpy(a), list(b)) - want) <= 1e-12
    with pytest.raises(ValueError):
        partition_nmi([0, 1], [0, 1, 2])


def test_labeler_command_line(capsys):
    from src.upstream.decar_v2 import store_clusters as sc
    base = ["--checkpoint", "c", "--input", "f.csv", "--out", "o.csv"]
    a = sc.get_args(base + ["--clustering", "pic"])
    assert (a.clustering, a.k, a.sigma, a.nnn, a.alpha, a.no_distribute_singletons, a.compare) == ("pic", None, 0.2, 5, 0.001, False, None)
    a = sc.get_args(base + ["--clustering", "pic", "--sigma", "0.3", "--nnn", "7", "--alpha", "0.01", "--no_distribute_singletons",
                            "--k", "9", "--compare", "other.csv"])
    assert (a.sigma, a.nnn, a.alpha, a.no_distribute_singletons, a.k, a.compare) == (0.3, 7, 0.01, True, 9, "other.csv")
    a = sc.get_args(base + ["--k", "585"])
    assert (a.clustering, a.k) == ("kmeans", 585)
    capsys.readouterr()
    for argv in (base, base + ["--clustering", "kmeans"]):
        with pytest.raises(SystemExit) as e:
            sc.get_args(argv)
        assert e.value.code == 2
        assert "the following arguments are required: --k" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        sc.get_args(base + ["--clustering", "spectral"])


def test_cpu_tensors_are_refused():
    from src.evaluation.graph import knn_graph
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn_graph(torch.zeros(8, 4), 2)


def test_bad_arguments_are_refused_without_a_gpu():
    """The same table tests/test_gpu_graph.py checks on the GPU box: here no device exists, so a launch would fail loudly."""
    from src import _native as N
    from src.evaluation.graph import graph_workspace_bytes, pic_workspace_bytes
    for what, got, want in R.bad_argument_codes(N.lib(), graph_workspace_bytes(100, 5), pic_workspace_bytes(100, 5)):
        assert got == want, what
    # workspace sizes grow with n and with k, and refuse what the kernels refuse
    assert graph_workspace_bytes(65536, 5) >= graph_workspace_bytes(1100, 5) >= graph_workspace_bytes(100, 5)
    assert graph_workspace_bytes(1100, 64) >= graph_workspace_bytes(1100, 5)
    assert pic_workspace_bytes(1100, 64) >= pic_workspace_bytes(1100, 5) >= pic_workspace_bytes(100, 5)
    for n, k in ((1, 1), (5, 5), (100, 65), (100, 0)):
        with pytest.raises(RuntimeError, match="EINVAL"):
            graph_workspace_bytes(n, k)
