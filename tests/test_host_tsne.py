"""CPU: the float64 restatement of t-SNE (tests/tsne_ref.py) against finite differences of its own loss and against sklearn's joint
probabilities, the host side of the `audiossl_tsne_*` entries (arguments refused before any launch, workspace size), the argument
checks of `src.evaluation.tsne` and the labeler's `--map` command line."""
import ctypes

import numpy as np
import pytest
import torch

import tsne_ref as R


def test_reference_gradient_is_the_derivative_of_its_kl():
    x, _ = R.blobs(10, 4, 6, 3.0, seed=1)
    idx, d2 = R.neighbours(x, 16)
    P = R.joint(idx, R.calibrate(d2, 5.0)[0])
    assert abs(P.sum() - 1.0) <= 1e-7 and np.array_equal(P, P.T) and (np.diag(P) == 0).all()
    y = np.random.RandomState(2).randn(40, 2)
    grad, kl, Z, _ = R.kl_and_gradient(P, y)
    assert kl > 0 and Z > 0
    h = 1e-6
    for i, c in ((0, 0), (7, 1), (39, 0), (20, 1)):
        yp, ym = y.copy(), y.copy()
        yp[i, c] += h
        ym[i, c] -= h
        fd = (R.kl_and_gradient(P, yp)[1] - R.kl_and_gradient(P, ym)[1]) / (2 * h)
        assert abs(fd - grad[i, c]) <= 1e-8 + 1e-6 * abs(grad[i, c]), (i, c, fd, grad[i, c])


def test_reference_calibration_reaches_the_perplexity():
    x, _ = R.blobs(30, 3, 5, 3.0, seed=3)
    idx, d2 = R.neighbours(x, 31)
    for f32 in (False, True):
        p, beta, h = R.calibrate(d2, 10.0, f32=f32)
        assert float(np.abs(h - np.log(10.0)).max()) <= 1e-5 and np.abs(p.sum(1) - 1).max() <= 1e-6 and (beta > 0).all()
    # a row of equal distances cannot reach the entropy: 100 doublings, the uniform row, finite
    p, beta, _ = R.calibrate(np.zeros((1, 7)), 3.0)
    assert np.array_equal(p, np.full((1, 7), float(np.float32(1.0 / 7)))) and beta[0] == 2.0 ** 100


def test_reference_p_matches_sklearn():
    try:
        from sklearn.manifold._t_sne import _joint_probabilities_nn
    except ImportError:
        pytest.skip("sklearn.manifold._t_sne._joint_probabilities_nn is not importable")
    from scipy.sparse import csr_matrix
    x, _ = R.blobs(40, 3, 7, 3.0, seed=4)
    n, k = len(x), 31
    idx, d2 = R.neighbours(x, k)
    D = csr_matrix((d2.astype(np.float32).reshape(-1), idx.reshape(-1), np.arange(0, n * k + 1, k)), shape=(n, n))
    want = _joint_probabilities_nn(D, 10.0, 0).toarray()
    got = R.joint(idx, R.calibrate(d2.astype(np.float32), 10.0)[0])
    assert R.rel_l2(got, want) <= 1e-6                                   # sklearn's conditional P is float32


def test_update_rule():
    y, upd, gains, grad = (np.array(v, dtype=np.float64) for v in ([[1.0, 2.0]], [[0.5, -0.5]], [[1.0, 0.01]], [[-2.0, -2.0]]))
    y2, u2, g2 = R.update(y, upd, gains, grad, 0.5, 10.0)
    assert g2.tolist() == [[1.2, 0.01]]                                   # opposite signs: + 0.2; same sign: * 0.8, clipped at 0.01
    np.testing.assert_allclose(u2, [[0.25 + 24.0, -0.25 + 0.2]], rtol=1e-15)
    np.testing.assert_allclose(y2, y + u2, rtol=0)


def test_header_declares_the_entries():
    from src import _native as N
    protos = N.parse_header()
    for name in ("calibrate", "symmetrize", "repulsion", "gradient", "update"):
        assert protos["audiossl_tsne_" + name][-1][0] == "stream"
    assert protos["audiossl_tsne_workspace"][-1][0] == "bytes"


def test_bad_arguments_are_refused_without_a_gpu():
    """No device exists here, so a launch would fail loudly: every one of these returns before it."""
    from src import _native as N
    from src.evaluation.tsne import tsne_workspace_bytes
    lib = N.lib()
    P, big = 4096, tsne_workspace_bytes(100, 31)                          # a non-null, aligned address that is never dereferenced
    assert lib.audiossl_tsne_calibrate(None, 100, 31, 10.0, P, P, None) == -1
    assert lib.audiossl_tsne_calibrate(P, 1, 1, 1.0, P, P, None) == -1
    assert lib.audiossl_tsne_calibrate(P, 100, 0, 10.0, P, P, None) == -1
    assert lib.audiossl_tsne_calibrate(P, 100, 65, 10.0, P, P, None) == -1
    assert lib.audiossl_tsne_calibrate(P, 20, 31, 10.0, P, P, None) == -1            # k > n - 1
    assert lib.audiossl_tsne_calibrate(P, 100, 31, 32.0, P, P, None) == -1           # perplexity > k
    assert lib.audiossl_tsne_calibrate(P, 100, 31, float("nan"), P, P, None) == -1
    assert lib.audiossl_tsne_symmetrize(P, P, 100, 31, P, P, None, P, P, big, None) == -1
    assert lib.audiossl_tsne_symmetrize(P, P, 100, 65, P, P, P, P, P, big, None) == -1
    assert lib.audiossl_tsne_symmetrize(P, P, 1, 1, P, P, P, P, P, big, None) == -1
    assert lib.audiossl_tsne_symmetrize(P, P, 100, 31, P, P, P, P, P, big - 1, None) == -1
    assert lib.audiossl_tsne_symmetrize(P, P, 100, 31, P, P, P, P, P + 4, big, None) == -3
    assert lib.audiossl_tsne_repulsion(P, 100, None, P, P, big, None) == -1
    assert lib.audiossl_tsne_repulsion(P, 1, P, P, P, big, None) == -1
    assert lib.audiossl_tsne_repulsion(P, 100, P, P, P, 8, None) == -1
    assert lib.audiossl_tsne_repulsion(P + 4, 100, P, P, P, big, None) == -3
    assert lib.audiossl_tsne_gradient(P, P, None, 10, P, P, P, 100, 1.0, P, None, None, 0, None) == -1
    assert lib.audiossl_tsne_gradient(P, P, P, 10, P, P, P, 1, 1.0, P, None, None, 0, None) == -1
    assert lib.audiossl_tsne_gradient(P, P, P, 10, P, P, P, 100, 1.0, P, P, None, 0, None) == -1      # KL wanted, no workspace
    assert lib.audiossl_tsne_gradient(P, P, P, 10, P, P, P, 100, float("nan"), P, None, None, 0, None) == -1
    assert lib.audiossl_tsne_update(P, 100, 0.5, 50.0, P, None, P, None) == -1
    assert lib.audiossl_tsne_update(P, 1, 0.5, 50.0, P, P, P, None) == -1
    b = ctypes.c_long(0)
    assert lib.audiossl_tsne_workspace(100, 31, None) == -1
    for n, k in ((1, 1), (100, 0), (100, 65), (20, 31)):
        assert lib.audiossl_tsne_workspace(n, k, ctypes.addressof(b)) == -1


def test_workspace_is_monotone():
    from src.evaluation.tsne import tsne_workspace_bytes
    by_n = [tsne_workspace_bytes(n, 61) for n in (62, 257, 600, 1030, 4096, 65536)]
    assert by_n == sorted(by_n)
    by_k = [tsne_workspace_bytes(65536, k) for k in (1, 16, 61, 64)]
    assert by_k == sorted(by_k) and by_k[0] >= 65536 * 2 * 8
    # n = 65,536 at k = 61: the CSR builder's raw and sorted rows, far below an n x n matrix
    assert tsne_workspace_bytes(65536, 61) < 65536 * 65536 // 16


def test_python_layer_refuses_bad_arguments():
    from src.evaluation import tsne, tsne_affinities, tsne_gradient
    from src.evaluation.graph import Csr
    from src.evaluation.tsne import neighbour_count
    assert neighbour_count(62, 20) == 61 and neighbour_count(600, 21) == 64 and neighbour_count(257, 5) == 16
    assert neighbour_count(12, 3) == 10
    x = torch.zeros(100, 8)
    for perplexity in (0, 0.5, 22, 21.5, float("nan")):
        with pytest.raises(ValueError, match="perplexity"):
            tsne(x, perplexity=perplexity)
        with pytest.raises(ValueError, match="perplexity"):
            tsne_affinities(x, perplexity=perplexity)
    with pytest.raises(ValueError, match="64"):                          # the message names the neighbour limit
        tsne(x, perplexity=22)
    with pytest.raises(ValueError, match="below the 11 neighbours"):     # perplexity >= k
        tsne(torch.zeros(12, 8), perplexity=11)
    with pytest.raises(ValueError):
        tsne(torch.zeros(100), perplexity=5)
    for init in (torch.zeros(100, 3), torch.zeros(99, 2), torch.zeros(200), "spectral"):
        with pytest.raises(ValueError, match="init"):
            tsne(x, init=init)
    with pytest.raises(ValueError, match="learning_rate"):
        tsne(x, learning_rate=0.0)
    P = Csr(None, None, None, None, 100)
    with pytest.raises(ValueError, match="layout"):
        tsne_gradient(P, torch.zeros(100, 3))
    for call in (lambda: tsne(x), lambda: tsne(x, init=torch.zeros(100, 2)), lambda: tsne_affinities(x),
                 lambda: tsne_gradient(P, torch.zeros(100, 2))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_pca_init_matches_the_reference():
    from src.evaluation.tsne import pca_init
    x, _ = R.blobs(50, 3, 9, 3.0, seed=6)
    y = pca_init(torch.from_numpy(x)).numpy()
    want = R.pca_init(x)
    assert y.dtype == np.float32 and np.abs(y - want).max() <= 1e-10
    assert abs(float(want[:, 0].std()) - 1e-4) <= 1e-15


def test_labeler_command_line():
    from src.upstream.decar_v2 import store_clusters as sc
    base = ["--checkpoint", "c", "--input", "f.csv", "--out", "o.csv", "--k", "9"]
    a = sc.get_args(base)
    assert (a.map, a.perplexity, a.map_iters) == (None, 20.0, 1000)
    a = sc.get_args(base + ["--map", "m.csv", "--perplexity", "3", "--map_iters", "50"])
    assert (a.map, a.perplexity, a.map_iters) == ("m.csv", 3.0, 50)
    a = sc.get_args(["--checkpoint", "c", "--input", "f.csv", "--out", "o.csv", "--clustering", "pic", "--map", "m.csv"])
    assert (a.clustering, a.map) == ("pic", "m.csv")
    a = sc.get_args(["--checkpoint", "c", "--input", "f.csv", "--out", "o.csv", "--k_sweep", "2,3", "--map", "m.csv"])
    assert (a.k_sweep, a.map) == ([2, 3], "m.csv")
