"""GPU: label spreading (csrc/spread.hip, src/evaluation/spread.py) against its float64 restatement (tests/spread_ref.py): the
normalisation, the iteration at the edges of its tiling, its bit-for-bit properties, convergence to the closed form, the
assignment, unreached nodes, the low-shot evaluation and both commands end to end."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import spread_ref as R
from oracle import fill

pytestmark = pytest.mark.gpu

SIGMA = 0.3


def _host(W):
    nnz = int(W.nnz)
    return (W.rowptr.cpu().numpy().astype(np.int64), W.col[:nnz].cpu().numpy().astype(np.int64), W.w[:nnz].cpu().numpy())


@functools.lru_cache(maxsize=None)
def _blob_graph(n, dim, centres, k, seed):
    """-> (W on the device, (rowptr, col, w) on the host, centre of every node)"""
    from src.evaluation.graph import knn_graph, pic_build
    x, member = R.blobs(n, dim, centres, seed)
    idx, d2 = knn_graph(torch.from_numpy(x).cuda(), k)
    W = pic_build(idx, d2, SIGMA)
    return W, _host(W), member


@functools.lru_cache(maxsize=None)
def _star_graph(n):
    from src.evaluation.graph import pic_build
    idx, d2 = R.star(n)
    W = pic_build(torch.from_numpy(idx).cuda(), torch.from_numpy(d2).cuda(), SIGMA)
    return W, _host(W), np.zeros(n, dtype=np.int64)


def _graph(kind, n, k):
    return _star_graph(n) if kind == "star" else _blob_graph(n, 16, 4, k, n + k)


def _seeds(n, m, per_column, seed):
    g = np.random.RandomState(seed)
    rows = np.concatenate([g.choice(n, per_column, replace=False) for _ in range(m)])
    cols = np.repeat(np.arange(m), per_column)
    return rows, cols


def _run(W, s, rows, cols, m, alpha, iters, fill_byte=None):
    """`audiossl_spread_run` on m columns (padded to a multiple of 4 as `label_spread` pads) -> F [n, m] on the host."""
    from src import _native as N
    from src.evaluation import spread as SP
    n = W.n
    mp = (m + 3) // 4 * 4
    seed_ptr, seed_col = SP._seed_lists(torch.from_numpy(rows), torch.from_numpy(cols), n, m, W.col.device)
    f = torch.empty(n, mp, dtype=torch.float32, device="cuda")
    nbytes = SP.spread_workspace_bytes(n, mp)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if fill_byte is not None:
        ws.fill_(fill_byte)
        f.view(torch.uint8).fill_(fill_byte)
    N.call("spread_run", W.rowptr, W.col, s, n, W.col.numel(), seed_ptr, seed_col, seed_col.numel(), mp, float(alpha), int(iters), f, ws, nbytes)
    out = f.cpu().numpy()
    assert not out[:, m:].any()                              # the padding columns have no seed
    return out[:, :m]


# (kind, n, k, m, alpha, iters): m = 3 pads to 4; 12 and 64: 16 lanes per row; 68: one wave per row; 260: two slices of 132
# columns, the last one partial; 524: three slices; the star's row 0 has n - 1 entries, across the 64- and 256-entry lengths
CASES = [("blobs", 257, 3, 3, 0.9, 100), ("blobs", 300, 5, 12, 0.99, 700), ("blobs", 300, 5, 64, 0.9, 100),
         ("blobs", 300, 5, 68, 0.9, 100), ("blobs", 300, 5, 260, 0.9, 100), ("blobs", 1000, 8, 524, 0.9, 100),
         ("star", 600, 1, 12, 0.9, 100), ("star", 70, 1, 8, 0.9, 100)]


@functools.lru_cache(maxsize=None)
def _case(i):
    """-> (F of the GPU, float64 reference F, per-column rounding bound, longest row)"""
    from src.evaluation import spread_normalize
    kind, n, k, m, alpha, iters = CASES[i]
    W, (rowptr, col, w), _ = _graph(kind, n, k)
    s, _ = spread_normalize(W)
    rows, cols = _seeds(n, m, 2, 100 + i)
    got = _run(W, s, rows, cols, m, alpha, iters)
    S = R.matrix(rowptr, col, R.normalize(rowptr, col, w)[0])
    ref = R.spread(S, R.seeds_dense(rows, cols, n, m), alpha, iters)
    L = int(np.diff(rowptr).max())
    return got, ref, R.rounding_bound(L, alpha, np.abs(ref).max(0)), L


def test_normalize_against_fp64():
    """The library is built without fast-math: the fp64 product, root and quotient are IEEE-correct on the device, so `s` is
    expected to equal (float) of numpy's fp64 value bit for bit.  The assertion allows what the issue allows and no more: an entry
    may differ by one fp32 ulp only where moving the fp64 value by one of ITS ulps changes the fp32 rounding."""
    from src.evaluation import spread_normalize
    W, (rowptr, col, w), _ = _blob_graph(257, 16, 4, 3, 260)
    s, deg = spread_normalize(W)
    nnz = len(col)
    s, deg = s[:nnz].cpu().numpy(), deg.cpu().numpy()
    s_ref, deg_ref = R.normalize(rowptr, col, w)
    rel = np.abs(deg - deg_ref) / deg_ref
    print(f"deg: max relative difference {rel.max():.2e}")
    assert rel.max() <= 1e-14
    want = s_ref.astype(np.float32)
    differ = np.flatnonzero(s != want)
    print(f"s: {len(differ)} of {nnz} entries differ from (float) of the fp64 value")
    for l in differ:
        near = {np.float32(np.nextafter(s_ref[l], 0.0)), np.float32(np.nextafter(s_ref[l], 2.0))}
        assert s[l] in near and abs(float(s[l]) - float(want[l])) <= np.spacing(want[l]), l
    M = sp.csr_matrix((s, col, rowptr), shape=(W.n, W.n))
    assert np.isfinite(s).all() and (M != M.T).nnz == 0          # s_ij == s_ji for every mutual entry (every entry of W = A + A^T)


def test_normalize_isolated_outlier():
    from src.evaluation import spread_normalize
    from src.evaluation.graph import knn_graph, pic_build
    x, _ = R.blobs(64, 8, 2, 5)
    x = np.concatenate([x, np.array([[40.0] + [0.0] * 7], dtype=np.float32)])         # distance^2 / sigma^2 > 1500^2 / 0.09
    idx, d2 = knn_graph(torch.from_numpy(x).cuda(), 3)
    assert float(d2[64].min()) / SIGMA ** 2 > 800
    W = pic_build(idx, d2, SIGMA)
    rowptr, col, w = _host(W)
    s, deg = spread_normalize(W)
    s, deg = s[:len(col)].cpu().numpy(), deg.cpu().numpy()
    assert deg[64] == 0 and (deg[:64] > 0).all()
    assert np.isfinite(s).all() and np.isfinite(deg).all()
    assert rowptr[65] - rowptr[64] == 3 and not s[rowptr[64]:rowptr[65]].any() and not s[col == 64].any()
    assert s[(col != 64) & (R.rows_of(rowptr) != 64)].min() > 0
    # the outlier stays unreached and poisons nobody
    from src.evaluation import label_spread
    res = label_spread(W, torch.tensor([0, 1]), torch.tensor([0, 1]), 2, 2, alpha=0.9, iters=50)
    assert torch.isfinite(res.F).all() and int(res.labels[64, 0]) == -1 and float(res.confidence[64, 0]) == 0.0


@pytest.mark.parametrize("i", range(len(CASES)))
def test_spread_against_fp64(i):
    got, ref, bound, L = _case(i)
    err = np.abs(got - ref).max(0)
    worst = int(np.argmax(err / bound))
    print(f"{CASES[i]}: longest row {L}, worst column {worst}: error {err[worst]:.3e} / bound {bound[worst]:.3e} = {err[worst] / bound[worst]:.4f}")
    assert np.isfinite(got).all() and (bound > 0).all()
    assert (err <= bound).all()


def test_bit_for_bit_properties():
    from src.evaluation import spread_normalize
    W, _, _ = _blob_graph(300, 16, 4, 5, 305)
    s, _ = spread_normalize(W)
    classes, trials = 4, 5
    rows, cols = _seeds(300, classes * trials, 2, 9)
    a = _run(W, s, rows, cols, classes * trials, 0.9, 31)
    b = _run(W, s, rows, cols, classes * trials, 0.9, 31)
    assert a.tobytes() == b.tobytes()
    c = _run(W, s, rows, cols, classes * trials, 0.9, 31, fill_byte=0xFF)          # the workspace needs no clearing
    assert a.tobytes() == c.tobytes()
    for t in range(trials):
        mine = (cols // classes) == t
        alone = _run(W, s, rows[mine], cols[mine] - t * classes, classes, 0.9, 31)
        assert alone.tobytes() == np.ascontiguousarray(a[:, t * classes:(t + 1) * classes]).tobytes(), t
    # the same columns inside a launch of another shape (one wave per row, two slices) are the same bits too
    wide_rows, wide_cols = _seeds(300, 260, 2, 10)
    keep = wide_cols >= 20
    wide = _run(W, s, np.concatenate([rows, wide_rows[keep]]), np.concatenate([cols, wide_cols[keep]]), 260, 0.9, 31)
    assert np.ascontiguousarray(wide[:, :20]).tobytes() == a.tobytes()
    # an even number of rounds ends in the caller's buffer as well
    d = _run(W, s, rows, cols, classes * trials, 0.9, 30, fill_byte=0xFF)
    e = _run(W, s, rows, cols, classes * trials, 0.9, 30)
    assert d.tobytes() == e.tobytes() and d.tobytes() != a.tobytes()


@pytest.mark.parametrize("alpha,T", [(0.9, 100), (0.99, 700)])
def test_convergence_to_the_closed_form(alpha, T):
    """|F_T - F*|_2 <= 2 alpha^T |Y_c|_2 per column (F* - F_T = (alpha S)^T (F* - Y), |S|_2 <= 1, |F*|_2 <= |Y|_2) plus the
    rounding bound of the iteration, which bounds every element: sqrt(n) times it bounds the 2-norm."""
    from src.evaluation import spread_normalize
    n, m = 300, 12
    W, (rowptr, col, w), _ = _blob_graph(n, 16, 4, 5, 305)
    s, _ = spread_normalize(W)
    rows, cols = _seeds(n, m, 2, 21)
    got = _run(W, s, rows, cols, m, alpha, T).astype(np.float64)
    S = R.matrix(rowptr, col, R.normalize(rowptr, col, w)[0])
    Y = R.seeds_dense(rows, cols, n, m)
    star = R.closed_form(S, Y, alpha)
    L = int(np.diff(rowptr).max())
    for c in range(m):
        dist = np.linalg.norm(got[:, c] - star[:, c])
        tail = 2 * alpha ** T * np.linalg.norm(Y[:, c])
        bound = tail + np.sqrt(n) * R.rounding_bound(L, alpha, np.abs(star[:, c]).max())
        print(f"alpha {alpha} T {T} column {c}: {dist:.3e} <= {tail:.3e} + rounding = {bound:.3e}")
        assert dist <= bound


@pytest.mark.parametrize("i,classes", [(1, 4), (5, 4)])
def test_assign_on_spread_results(i, classes):
    from src.evaluation import spread_assign
    got, ref, bound, _ = _case(i)
    trials = got.shape[1] // classes
    label, conf = spread_assign(torch.from_numpy(got).cuda(), classes, trials)
    label, conf = label.cpu().numpy(), conf.cpu().numpy()
    assert label.shape == (got.shape[0], trials) and label.dtype == np.int64
    want, conf_ref, margin = R.assign(ref, classes)
    clear = margin > 2 * bound.reshape(trials, classes).max(1)[None, :]
    # a row the reference leaves at exactly 0 has no seed of the trial within reach: sums of zeros, -1 in any precision
    clear |= ref.reshape(-1, trials, classes).max(2) == 0
    skipped = 1.0 - clear.mean()
    loose = (margin <= 1e-4 * np.abs(ref).reshape(-1, trials, classes).max((0, 2))[None, :]).mean()
    print(f"{CASES[i]}: {skipped * 100:.2f} % of (row, trial) pairs skipped; {loose * 100:.2f} % within 1e-4 of the column maximum")
    assert skipped <= 0.05
    np.testing.assert_array_equal(label[clear], want[clear])
    # the assignment itself is exact on the matrix it is given
    own, own_conf, _ = R.assign(got, classes)
    np.testing.assert_array_equal(label, own)
    assert np.abs(conf - own_conf).max() <= 1e-6
    diff = np.abs(conf - conf_ref).max()
    print(f"confidence: max difference {diff:.2e}")
    assert diff <= 1e-5


def test_assign_hand_written_rows():
    from src.evaluation import spread_assign
    F = np.zeros((5, 8), dtype=np.float32)                   # classes = 3, trials = 2, ldf = 8: the padding is not read
    F[0, :3] = [0.25, 0.25, 0.1]                             # an exact tie -> the lowest class
    F[1, 3:6] = [0.0, 0.0, 0.7]                              # one non-zero entry -> confidence 1
    F[2, :3] = [0.2, 0.2, 0.2]                               # uniform -> confidence 0
    F[3, 6:] = 9.0                                           # only the padding is non-zero
    F[4, :6] = [0.0, 1e-30, 0.0, 3e-37, 2e-37, 1e-37]
    label, conf = spread_assign(torch.from_numpy(F).cuda(), 3, 2)
    np.testing.assert_array_equal(label.cpu().numpy(), [[0, -1], [-1, 2], [0, -1], [-1, -1], [1, 0]])
    conf = conf.cpu().numpy()
    want = R.assign(F[:, :6], 3)[1]
    assert np.abs(conf - want).max() <= 1e-6
    assert conf[0, 1] == 0 and conf[1, 0] == 0 and conf[1, 1] == 1 and abs(conf[2, 0]) <= 1e-7 and (conf[3] == 0).all() and conf[4, 0] == 1
    one, c1 = spread_assign(torch.from_numpy(F).cuda(), 1, 8)            # classes == 1: reached -> (0, 1), else (-1, 0)
    np.testing.assert_array_equal(one.cpu().numpy(), np.where(F > 0, 0, -1))
    np.testing.assert_array_equal(c1.cpu().numpy(), (F > 0).astype(np.float32))


def _two_blobs(per):
    g = np.random.RandomState(3)
    c = np.zeros((2, 8))
    c[0, 0], c[1, 0] = 1.0, -1.0
    x = np.repeat(c, per, axis=0) + 0.15 * g.randn(2 * per, 8) / np.sqrt(8)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def test_unreached_nodes():
    from src.evaluation import label_spread, lowshot_evaluate
    from src.evaluation.graph import knn_graph, pic_build
    per = 40
    x = torch.from_numpy(_two_blobs(per)).cuda()
    idx, d2 = knn_graph(x, 3)
    assert bool((idx[:per] < per).all()) and bool((idx[per:] >= per).all())          # two components
    W = pic_build(idx, d2, SIGMA)
    res = label_spread(W, torch.tensor([0, 5, 9]), torch.tensor([0, 1, 0]), 2, 2, alpha=0.9, iters=200)
    labels = res.labels.cpu().numpy()[:, 0]
    assert (labels[per:] == -1).all() and (labels[:per] >= 0).all()
    assert not res.F[per:].any() and not res.confidence[per:].any()
    assert res.F.shape == (2 * per, 2) and res.labels.shape == (2 * per, 1) and res.labels.dtype == torch.int64
    # train: 30 nodes of the first blob; test: its other 10 and 10 of the second blob, which no seed reaches
    train, test = x[:30], torch.cat([x[30:40], x[40:50]])
    y_train = torch.arange(30) % 2
    y_test = torch.arange(20) % 2
    out = lowshot_evaluate(train, y_train, test, y_test, shots=(2,), trials=3, k=3, sigma=SIGMA, alpha=0.9, iters=200)
    assert out["unreached"] == [0.5] and out["top1"][0] <= 0.5 and out["short_classes"] == [0]


def test_label_spread_refuses_bad_seeds():
    from src.evaluation import label_spread
    W, _, _ = _blob_graph(300, 16, 4, 5, 305)
    for rows, cols, what in (([0, 0], [1, 1], "more than once"), ([300], [0], "outside"), ([0], [4], "outside"), ([-1], [0], "outside")):
        with pytest.raises(ValueError, match=what):
            label_spread(W, torch.tensor(rows), torch.tensor(cols), 4, 4)
    with pytest.raises(ValueError, match="multiple of classes"):
        label_spread(W, torch.tensor([0]), torch.tensor([0]), 6, 4)
    with pytest.raises(ValueError, match="alpha"):
        label_spread(W, torch.tensor([0]), torch.tensor([0]), 4, 4, alpha=1.0)


KEYS = ["shots", "trials", "top1", "top1_std", "unreached", "short_classes", "k", "sigma", "alpha", "iters", "N_train", "N_test", "d", "columns"]


def test_lowshot_evaluate_on_synthetic_embeddings():
    from src import _native as N
    from src.evaluation import lowshot_evaluate, lowshot_seeds
    from src.evaluation.graph import knn_graph, pic_build
    classes, n_train, n_test, shots, trials = 4, 400, 200, (1, 5), 3
    x, member = R.blobs(n_train + n_test, 16, classes, 77, spread=1.2)
    scale = 1.0 + np.random.RandomState(1).rand(len(x), 1).astype(np.float32)        # the evaluation normalises the rows itself
    emb = torch.from_numpy(x * scale).cuda()
    y = torch.from_numpy(member)
    args = (emb[:n_train].contiguous(), y[:n_train], emb[n_train:].contiguous(), y[n_train:])
    N.PROFILE, N.PROFILE_ALL = {}, True
    try:
        out = lowshot_evaluate(*args, shots=shots, trials=trials, seed=3)
        torch.cuda.synchronize()
        calls = {k: len(v) for k, v in N.PROFILE.items()}
    finally:
        N.PROFILE, N.PROFILE_ALL = None, False
    assert calls["audiossl_spread_run"] == 1 and calls["audiossl_spread_normalize"] == 1 and calls["audiossl_knn_graph_l2"] == 1
    assert list(out) == KEYS
    assert out["columns"] == classes * 2 * 3 and out["shots"] == [1, 5] and out["trials"] == 3 and out["iters"] == 688
    assert (out["N_train"], out["N_test"], out["d"], out["k"], out["alpha"], out["short_classes"]) == (400, 200, 16, 10, 0.99, [0, 0])
    assert out == lowshot_evaluate(*args, shots=shots, trials=trials, seed=3)
    assert json.loads(json.dumps(out)) == out
    # the same graph and the same seeds through the float64 restatement
    idx, d2 = knn_graph(torch.nn.functional.normalize(emb, dim=1), 10)
    assert abs(float(d2.median().sqrt()) - out["sigma"]) <= 1e-7
    rowptr, col, w = _host(pic_build(idx, d2, out["sigma"]))
    S = R.matrix(rowptr, col, R.normalize(rowptr, col, w)[0])
    rows, cols = [], []
    for si, sh in enumerate(shots):
        r, c, _ = lowshot_seeds(y[:n_train], classes, sh, trials, 3)
        assert r.max() < n_train                              # seeds come from train rows only
        rows.append(r)
        cols.append(c + si * trials * classes)
    ref = R.spread(S, R.seeds_dense(np.concatenate(rows), np.concatenate(cols), n_train + n_test, out["columns"]), 0.99, 688)
    want = R.assign(ref, classes)[0][n_train:].reshape(n_test, 2, trials)
    acc = (want == member[n_train:, None, None]).mean(0)                               # [shots, trials]
    print(f"top1 {out['top1']} +- {out['top1_std']}, unreached {out['unreached']}; float64 {acc.mean(1).tolist()}")
    for si in range(2):
        assert abs(out["top1"][si] - acc[si].mean()) <= 1.0 / n_test + 1e-12           # one flipped test row per trial
    assert out["top1"][1] > 0.5                               # five shots on four noisy blobs: far above chance


def _checkpoint(tmp_path, cfg_s):
    from src.encoder import AudioNTT2020Task6
    from src.upstream.delores_s.upstream_expert import Upstream_Expert
    expert = Upstream_Expert(copy.deepcopy(cfg_s), base_encoder=AudioNTT2020Task6)
    fill.fill_state_dict_(expert, seed=9)
    ck = expert.checkpoint()
    ck["hyper_parameters"]["config"] = expert.config                  # as HipTrainer.save_checkpoint writes it
    ck["hyper_parameters"]["base_encoder"] = expert.config["pretrain"]["base_encoder"]["type"]
    path = str(tmp_path / "delores_s.ckpt")
    torch.save(ck, path)
    return path


def _write_wavs(tmp_path, count):
    from scipy.io import wavfile
    files = []
    for i in range(count):
        L = 16000 + 500 * (i % 3)
        w = fill.uniform((L,), 500 + i, -0.3, 0.3) + 0.2 * np.sin(2 * np.pi * (200 + 300 * (i % 2)) * np.arange(L) / 16000).astype(np.float32)
        p = str(tmp_path / f"clip_{i}.wav")
        wavfile.write(p, 16000, (w * 32767).astype(np.int16))
        files.append(p)
    return files


def test_both_commands_end_to_end(tmp_path, cfg_s, capsys):
    import pandas as pd

    import evaluate_lowshot as EL
    from src.upstream.decar_v2 import store_clusters as sc
    ckpt = _checkpoint(tmp_path, cfg_s)
    files = _write_wavs(tmp_path, 12)
    names = ["low" if i % 2 == 0 else "high" for i in range(12)]
    train_csv, test_csv, dump = str(tmp_path / "train.csv"), str(tmp_path / "test.csv"), str(tmp_path / "emb")
    pd.DataFrame({"wav": files[:8], "label": names[:8]}).to_csv(train_csv, index=False)
    pd.DataFrame({"wav": files[8:], "label": names[8:]}).to_csv(test_csv, index=False)
    common = ["--shots", "1,2", "--trials", "2", "-k", "3", "--alpha", "0.9"]
    capsys.readouterr()
    first = EL.main(EL.get_args(["--checkpoint", ckpt, "--upstream", "delores_s", "--train_csv", train_csv, "--test_csv", test_csv,
                                 "--dump_embeddings", dump] + common))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == first and list(first) == KEYS
    assert (first["N_train"], first["N_test"], first["columns"], first["iters"], first["k"]) == (8, 4, 2 * 2 * 2, 66, 3)
    assert all(0.0 <= v <= 1.0 for v in first["top1"] + first["unreached"])
    assert sorted(os.listdir(dump)) == ["test_embeddings.npy", "test_labels.npy", "train_embeddings.npy", "train_labels.npy"]
    again = EL.main(EL.get_args(["--embeddings", dump] + common))
    assert again == first and json.loads(capsys.readouterr().out) == first

    files_csv, few_csv, out_csv = str(tmp_path / "files.csv"), str(tmp_path / "few.csv"), str(tmp_path / "spread.csv")
    pd.DataFrame({"files": files}).to_csv(files_csv, index=False)
    seeds = {files[0]: "low", files[5]: "high", files[6]: "high"}          # files[6] is a "low" clip labelled "high": it keeps that label
    pd.DataFrame({"files": list(seeds), "label": list(seeds.values())}).to_csv(few_csv, index=False)
    head = ["--checkpoint", ckpt, "--upstream", "delores_s", "--input", files_csv, "--pca", "8", "--window", "center", "--clustering", "spread",
            "--sigma", "0.5", "--spread_alpha", "0.9"]
    base = head + ["--seed_labels", few_csv, "--nnn", "3"]
    labels = sc.main(sc.get_args(base + ["--out", out_csv, "--score"]))
    text = capsys.readouterr().out
    assert "classes: 0=high, 1=low" in text and "12 files, 2 classes from 3 seeds, " in text and "silhouette" in text
    rows = open(out_csv).read().split()
    assert rows[0] == "files,label" and [r.rsplit(",", 1)[0] for r in rows[1:]] == files
    got = [int(r.rsplit(",", 1)[1]) for r in rows[1:]]
    assert got == [int(v) for v in labels] and set(got) <= {-1, 0, 1}
    assert (got[0], got[5], got[6]) == (1, 0, 0)                          # seed files keep their labels
    unreached = sum(1 for v in got if v < 0)
    assert f"{unreached} unreached" in text

    # two seeds, one neighbour per file, one round: most files are out of reach.  --drop_unreached leaves them out,
    # --confidence adds the third column
    seeds = {files[0]: "low", files[5]: "high"}
    pd.DataFrame({"files": list(seeds), "label": list(seeds.values())}).to_csv(few_csv, index=False)
    base = head + ["--seed_labels", few_csv, "--nnn", "1"]
    conf_csv = str(tmp_path / "conf.csv")
    sc.main(sc.get_args(base + ["--out", conf_csv, "--confidence", "--drop_unreached", "--spread_iters", "1"]))
    text = capsys.readouterr().out
    table = pd.read_csv(conf_csv)
    assert list(table.columns) == ["files", "label", "confidence"] and (table["label"] >= 0).all()
    assert ((table["confidence"] >= 0) & (table["confidence"] <= 1)).all()
    kept = set(table["files"])
    assert set(seeds) <= kept and "(dropped)" in text
    dropped = 12 - len(table)
    assert f"{dropped} unreached (dropped)" in text
    full_csv = str(tmp_path / "full.csv")
    sc.main(sc.get_args(base + ["--out", full_csv, "--spread_iters", "1"]))
    capsys.readouterr()
    full = pd.read_csv(full_csv)
    assert len(full) == 12 and int((full["label"] < 0).sum()) == dropped and dropped >= 1
    assert list(full["files"][full["label"] >= 0]) == list(table["files"])

    few_bad = str(tmp_path / "bad.csv")
    pd.DataFrame({"files": [files[0], "nowhere.wav"], "label": ["low", "high"]}).to_csv(few_bad, index=False)
    with pytest.raises(ValueError, match="nowhere.wav is not a file"):
        sc.main(sc.get_args(head + ["--seed_labels", few_bad, "--out", out_csv]))
