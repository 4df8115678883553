"""CPU: the float64 restatement of the silhouette coefficient (tests/silhouette_ref.py) against sklearn itself on every case the GPU
test uses, the host side of `audiossl_silhouette` (arguments refused before any launch, workspace size), and the labeler's
`--score` / `--k_sweep` command line."""
import numpy as np
import pytest
import torch

import silhouette_ref as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_sklearn(name):
    from sklearn.metrics import silhouette_samples, silhouette_score
    x, labels, ref = R.case(name)
    want = silhouette_samples(x.astype(np.float64), labels, metric="euclidean")
    assert float(np.abs(ref.s - want).max()) <= 1e-12
    assert abs(float(ref.s.mean()) - silhouette_score(x.astype(np.float64), labels)) <= 1e-12
    assert 0 < ref.d_min <= ref.d_max and (ref.b > 0).any()


def test_the_cases_are_what_they_say():
    sizes = {name: np.unique(R.case(name)[1], return_counts=True)[1].tolist() for name in R.CASES}
    assert len(sizes["A"]) == 7 and R.case("A")[1].min() < 0 and R.case("A")[0].shape == (333, 19)
    assert sizes["B"] == [128, 256, 64, 63, 1]
    assert sorted(sizes["C"]) == [1] * 128 + [2] and len(sizes["C"]) == 130 - 1
    assert sorted(sizes["D"]) == [1, 199]
    assert len(sizes["F"]) == 37 and min(sizes["F"]) >= 2
    assert len(sizes["G"]) == 3 and R.case("G")[0].shape == (257, 516)
    assert sizes["H"] == [2, 1]
    x, labels, ref = R.case("E")
    assert sizes["E"] == [40, 30, 25, 50]
    u = x[labels == 0][0]
    assert (x[(labels == 0) | (labels == 2)] == u).all() and not (x[labels == 1] == u).all(1).any()
    assert (ref.s[(labels == 0) | (labels == 2)] == 0).all() and (ref.s[labels == 1] == 1).all()


def test_bad_arguments_are_refused_without_a_gpu():
    """The same table tests/test_gpu_silhouette.py checks on the GPU box: here no device exists, so a launch would fail loudly."""
    from src import _native as N
    from src.evaluation.graph import silhouette_workspace_bytes
    protos = N.parse_header()
    assert protos["audiossl_silhouette"][-1][0] == "stream"
    assert protos["audiossl_silhouette_workspace"][-1][0] == "bytes"     # a host entry point: no stream
    for what, got, want in R.bad_argument_codes(N.lib(), silhouette_workspace_bytes(100)):
        assert got == want, what


def test_workspace_is_monotone_in_n():
    from src.evaluation.graph import silhouette_workspace_bytes
    sizes = [silhouette_workspace_bytes(n) for n in (3, 63, 64, 65, 100, 4096, 65536, 1 << 24)]
    assert sizes == sorted(sizes) and sizes[0] >= 3 * 4 and sizes[-2] >= 65536 * 4
    for n in (2, 0, -5):
        with pytest.raises(RuntimeError, match="EINVAL"):
            silhouette_workspace_bytes(n)


def test_cpu_tensors_are_refused():
    from src.evaluation import silhouette_samples, silhouette_score
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        silhouette_samples(torch.zeros(8, 4), [0, 0, 1, 1, 2, 2, 0, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        silhouette_score(torch.zeros(8, 4), [0, 0, 1, 1, 2, 2, 0, 1])


def test_labeler_command_line(capsys):
    from src.upstream.decar_v2 import store_clusters as sc
    base = ["--checkpoint", "c", "--input", "f.csv", "--out", "o.csv"]
    a = sc.get_args(base + ["--k", "585"])
    assert (a.k, a.k_sweep, a.score) == (585, None, False)
    a = sc.get_args(base + ["--k", "9", "--score"])
    assert (a.clustering, a.k, a.k_sweep, a.score) == ("kmeans", 9, None, True)
    a = sc.get_args(base + ["--clustering", "pic", "--score"])
    assert (a.clustering, a.k, a.score) == ("pic", None, True)
    a = sc.get_args(base + ["--k_sweep", "64,128,256"])
    assert (a.clustering, a.k, a.k_sweep, a.score) == ("kmeans", None, [64, 128, 256], False)
    assert sc.get_args(base + ["--k_sweep", "7", "--score", "--clustering", "kmeans"]).k_sweep == [7]
    capsys.readouterr()
    for argv, message in ((base + ["--k_sweep", "2,3", "--k", "3"], "--k_sweep takes the place of --k"),
                          (base + ["--k_sweep", "2,3", "--clustering", "pic"], "--k_sweep is for k-means"),
                          (base, "the following arguments are required: --k"),
                          (base + ["--k_sweep", "2,x"], "comma-separated list of integers"),
                          (base + ["--k_sweep", "0,3"], "at least 1")):
        with pytest.raises(SystemExit) as e:
            sc.get_args(argv)
        assert e.value.code == 2
        assert message in capsys.readouterr().err
