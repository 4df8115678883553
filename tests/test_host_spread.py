"""CPU: the float64 restatement of label spreading (tests/spread_ref.py) against sklearn's `LabelSpreading`, the seed draws of the
low-shot protocol, the C ABI's refusals before any launch and the two commands' parsers."""
import warnings

import numpy as np
import pytest
import torch

import pic_ref as P
import spread_ref as R


@pytest.mark.parametrize("alpha,T", [(0.9, 30), (0.99, 200)])
def test_the_reference_is_sklearns(alpha, T):
    """`LabelSpreading` with a precomputed W and tol = 0 runs exactly T rounds of the same recurrence from the same start."""
    from sklearn.semi_supervised import LabelSpreading
    n, C, k = 200, 4, 5
    x, member = R.blobs(n, 16, C, 11)
    idx, d2 = P.knn_graph(x, k)
    rowptr, col, w = R.csr_from_lists(idx, d2, 0.3)
    s, deg = R.normalize(rowptr, col, w)
    assert deg.min() > 0
    S = R.matrix(rowptr, col, s)
    g = np.random.RandomState(5)
    y = np.full(n, -1)
    for c in range(C):
        y[g.choice(np.flatnonzero(member == c), 3, replace=False)] = c
    rows = np.flatnonzero(y >= 0)
    F = R.spread(S, R.seeds_dense(rows, y[rows], n, C), alpha, T)
    W_dense = R.matrix(rowptr, col, w).toarray()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # "max_iter reached without convergence" is the point
        model = LabelSpreading(kernel=lambda a, b=None: W_dense, alpha=alpha, max_iter=T, tol=0.0).fit(x, y)
    assert model.n_iter_ == T
    tot = F.sum(1, keepdims=True)
    assert tot.min() > 0                                           # every node is reached: sklearn's normaliser is the row sum
    diff = np.abs(model.label_distributions_ - F / tot).max()
    print(f"alpha {alpha} T {T}: max |sklearn - ref| = {diff:.2e}")
    assert diff <= 1e-12
    label, conf, _ = R.assign(F, C)
    np.testing.assert_array_equal(model.transduction_, label[:, 0])
    assert ((conf >= 0) & (conf <= 1)).all()


def test_closed_form_is_the_fixed_point():
    n, C = 120, 3
    x, member = R.blobs(n, 8, C, 3)
    rowptr, col, w = R.csr_from_lists(*P.knn_graph(x, 4), 0.3)
    S = R.matrix(rowptr, col, R.normalize(rowptr, col, w)[0])
    Y = R.seeds_dense(np.arange(6), np.arange(6) % C, n, C)
    Fs = R.closed_form(S, Y, 0.9)
    np.testing.assert_allclose(0.9 * (S @ Fs) + 0.1 * Y, Fs, atol=1e-14)
    FT = R.spread(S, Y, 0.9, 100)
    for c in range(C):
        assert np.linalg.norm(FT[:, c] - Fs[:, c]) <= 2 * 0.9 ** 100 * np.linalg.norm(Y[:, c])


def test_reference_assign_rules():
    F = np.array([[0.2, 0.2, 0.1, 0.0, 0.0, 0.0],        # a tie -> lowest class; second trial unreached
                  [0.0, 0.0, 0.5, 0.1, 0.1, 0.1],        # one non-zero entry -> confidence 1; uniform -> confidence 0
                  [0.0, 0.0, 0.0, 0.0, 0.3, 0.0]])
    label, conf, margin = R.assign(F, 3)
    np.testing.assert_array_equal(label, [[0, -1], [2, 0], [-1, 1]])
    np.testing.assert_allclose(conf[[0, 1, 1, 2, 2], [1, 0, 1, 0, 1]], [0, 1, 0, 0, 1], atol=1e-15)
    assert margin[0, 0] == 0 and abs(margin[1, 0] - 0.5) < 1e-15
    label, conf, _ = R.assign(F, 1)
    np.testing.assert_array_equal(label[0], [0, 0, 0, -1, -1, -1])
    np.testing.assert_array_equal(conf[0], [1, 1, 1, 0, 0, 0])


def test_lowshot_seeds():
    from src.evaluation import lowshot_seeds
    g = np.random.RandomState(0)
    classes, trials, shots = 5, 4, 3
    y = g.randint(classes - 1, size=200)
    y[:2] = classes - 1                                   # class 4 has two members: short at 3 shots
    rows, cols, short = lowshot_seeds(torch.from_numpy(y), classes, shots, trials, 7)
    assert short == 1 and rows.dtype == np.int64 and cols.dtype == np.int64
    assert len(rows) == trials * ((classes - 1) * shots + 2)
    for t in range(trials):
        for c in range(classes):
            mine = rows[cols == t * classes + c]
            assert len(mine) == (2 if c == classes - 1 else shots) and len(set(mine.tolist())) == len(mine)
            assert (y[mine] == c).all()                   # draws come only from the class's members
    assert sorted(rows[cols == 4].tolist()) == [0, 1]
    assert ((cols // classes) < trials).all()
    again = lowshot_seeds(y, classes, shots, trials, 7)
    np.testing.assert_array_equal(rows, again[0])
    np.testing.assert_array_equal(cols, again[1])
    other = lowshot_seeds(y, classes, shots, trials, 8)
    assert not np.array_equal(rows, other[0])
    per_trial = [sorted(rows[(cols // classes) == t].tolist()) for t in range(trials)]
    assert per_trial[0] != per_trial[1]
    # the draw is the documented one: default_rng([seed, shots, t]), classes in ascending id, members in ascending index
    rng = np.random.default_rng([7, shots, 2])
    want = rng.choice(np.flatnonzero(y == 0), size=shots, replace=False)
    assert sorted(rows[cols == 2 * classes].tolist()) == sorted(want.tolist())
    assert lowshot_seeds(y, classes, 1, 2, 0)[2] == 0


def test_bad_arguments_are_refused_without_a_gpu():
    """No device exists here, so a launch would fail loudly: every refusal comes before one."""
    from src import _native as N
    from src.evaluation.spread import spread_workspace_bytes
    for what, got, want in R.bad_argument_codes(N.lib(), spread_workspace_bytes(100, 8)):
        assert got == want, what
    assert spread_workspace_bytes(100, 8) >= 100 * 8 * 4
    assert spread_workspace_bytes(65536, 528) >= spread_workspace_bytes(1100, 528) >= spread_workspace_bytes(1100, 8) >= spread_workspace_bytes(100, 8)
    assert spread_workspace_bytes(100, 8192) >= spread_workspace_bytes(100, 528)          # at least 8,192 columns are accepted
    for n, m in ((1, 8), (100, 0), (100, 6), (100, 16388), (1 << 20, 2048)):
        with pytest.raises(RuntimeError, match="EINVAL"):
            spread_workspace_bytes(n, m)


def test_cpu_tensors_are_refused():
    from src.evaluation import label_spread, lowshot_evaluate, spread_assign, spread_normalize
    from src.evaluation.graph import Csr
    W = Csr(torch.zeros(5, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.float64),
            torch.zeros(1, dtype=torch.int32), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spread_normalize(W)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        label_spread(W, torch.tensor([0]), torch.tensor([0]), 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spread_assign(torch.zeros(4, 4), 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lowshot_evaluate(torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64), torch.zeros(4, 4), torch.zeros(4, dtype=torch.int64))


def test_default_iters():
    from src.evaluation.spread import default_iters
    assert default_iters(0.99) == 688 and default_iters(0.9) == 66


def test_lowshot_command_line(capsys):
    import evaluate_lowshot as EL
    base = ["--checkpoint", "c", "--train_csv", "a.csv", "--test_csv", "b.csv"]
    a = EL.get_args(base)
    assert (a.shots, a.trials, a.seed, a.k, a.sigma, a.alpha, a.iters, a.upstream, a.layer, a.window, a.batch_size) == \
        ([1, 5, 10], 5, 0, 10, None, 0.99, None, "delores_m", "backbone", "center", 64)
    a = EL.get_args(base + ["--shots", "2,7", "--trials", "3", "--seed", "4", "-k", "6", "--sigma", "0.4", "--alpha", "0.9", "--iters", "50",
                            "--dump_embeddings", "d"])
    assert (a.shots, a.trials, a.seed, a.k, a.sigma, a.alpha, a.iters, a.dump_embeddings) == ([2, 7], 3, 4, 6, 0.4, 0.9, 50, "d")
    assert EL.get_args(["--embeddings", "d"]).embeddings == "d"
    capsys.readouterr()
    for argv in ([], base[:4], base + ["--shots", "0"], base + ["--shots", "a"], base + ["--trials", "0"], base + ["--alpha", "1"],
                 base + ["--alpha", "0"], base + ["--iters", "0"], base + ["--sigma", "0"], base + ["-k", "0"],
                 ["--embeddings", "d", "--dump_embeddings", "e"]):
        with pytest.raises(SystemExit) as e:
            EL.get_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_labeler_command_line(capsys):
    from src.upstream.decar_v2 import store_clusters as sc
    base = ["--checkpoint", "c", "--input", "f.csv", "--out", "o.csv"]
    a = sc.get_args(base + ["--clustering", "spread", "--seed_labels", "few.csv"])
    assert (a.clustering, a.seed_labels, a.spread_alpha, a.spread_iters, a.drop_unreached, a.confidence) == \
        ("spread", "few.csv", 0.99, None, False, False)
    assert (a.alpha, a.sigma, a.nnn, a.k, a.k_sweep) == (0.001, 0.2, 5, None, None)         # PIC's --alpha keeps its meaning and default
    a = sc.get_args(base + ["--clustering", "spread", "--seed_labels", "few.csv", "--spread_alpha", "0.9", "--spread_iters", "40",
                            "--drop_unreached", "--confidence", "--nnn", "8", "--sigma", "0.5", "--score", "--map", "m.csv", "--compare", "x.csv"])
    assert (a.spread_alpha, a.spread_iters, a.drop_unreached, a.confidence, a.nnn, a.sigma, a.score, a.map, a.compare) == \
        (0.9, 40, True, True, 8, 0.5, True, "m.csv", "x.csv")
    a = sc.get_args(base + ["--k", "585"])                         # the defaults of the other algorithms are what they were
    assert (a.clustering, a.k, a.seed_labels) == ("kmeans", 585, None)
    capsys.readouterr()
    spread = base + ["--clustering", "spread", "--seed_labels", "few.csv"]
    for argv in (spread + ["--k", "9"], spread + ["--k_sweep", "4,8"], base + ["--clustering", "spread"],
                 base + ["--k", "9", "--seed_labels", "few.csv"], base + ["--clustering", "pic", "--seed_labels", "few.csv"],
                 spread + ["--spread_alpha", "1.0"], spread + ["--spread_iters", "0"], base + ["--clustering", "spectral"]):
        with pytest.raises(SystemExit) as e:
            sc.get_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_seed_label_files(tmp_path):
    from src.upstream.decar_v2.store_clusters import read_seed_labels
    files = [f"f{i}.wav" for i in range(6)]
    few = tmp_path / "few.csv"
    few.write_text("files,label\nf4.wav,dog\nf1.wav,cat\nf0.wav,dog\n")
    rows, ids, names = read_seed_labels(str(few), files)
    assert names == ["cat", "dog"] and rows.tolist() == [4, 1, 0] and ids.tolist() == [1, 0, 1]
    few.write_text("files,label\nf4.wav,10\nf1.wav,9\n")          # sorted as strings: "10" < "9"
    assert read_seed_labels(str(few), files)[2] == ["10", "9"]
    few.write_text("files,label\nf4.wav,a\nf9.wav,b\nf8.wav,b\n")
    with pytest.raises(ValueError, match="f9.wav is not a file"):
        read_seed_labels(str(few), files)
    few.write_text("files,label\nf4.wav,a\nf4.wav,b\n")
    with pytest.raises(ValueError, match="f4.wav is listed more than once"):
        read_seed_labels(str(few), files)
    few.write_text("files,tag\nf4.wav,a\n")
    with pytest.raises(ValueError, match="no `label` column"):
        read_seed_labels(str(few), files)
    few.write_text("files,label\n")
    with pytest.raises(ValueError, match="lists no file"):
        read_seed_labels(str(few), files)
