"""`audiossl_tsne_*` on the GPU against the float64 restatement of tests/tsne_ref.py (itself checked against finite differences and
sklearn on the CPU), the Python layer above them and the labeler's `--map`.

Bars.  P and grad: 4 x the rel-L2 distance between the float64 restatement and the same restatement with its exponentials /
reciprocals and sums in float32, computed here on the CPU for every case - the margin is for a different summation order, the
hardware reciprocal (plus one Newton step) and a search that may stop a step apart inside its 1e-5 window.  KL: w carries at most
three fp32 roundings (1.8e-7 relative), Z is an fp64 fold of such terms, the log and its sum are fp64 and sum P = 1, so
|KL - KL_ref| < 4e-7: the bar is 1e-6, and 1e-6 relative for Z by the same argument.  Every case prints its figures before it
asserts (the tables of DESIGN.md section 19).
Measured on MI355X: P rel-L2 2.5e-8 .. 2.6e-8 (0.005 - 0.106 of its bar), max |H - log perplexity| 9.993e-6; grad rel-L2 3.8e-8 .. 3.2e-7
(0.050 - 0.242 of its bar), Z relative <= 3.4e-8, |KL - ref| <= 3.3e-8; update 7.0e-8 and y 4.1e-8 of their largest magnitude; the map of six
blobs: purity 1.0000, KL 3.2217 -> 0.8901."""
import copy
import functools

import numpy as np
import pytest
import torch

import tsne_ref as R
from oracle import fill

pytestmark = pytest.mark.gpu

GUARD = 2


def _guarded(numel, dtype, value):
    return torch.full((numel + GUARD,), value, dtype=dtype, device="cuda")


def _intact(t, numel, value):
    return bool((t[numel:] == value).all())


def _workspace(n, k=1):
    from src.evaluation.tsne import tsne_workspace_bytes
    nbytes = tsne_workspace_bytes(n, k)
    return torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda"), nbytes          # the kernels need nothing cleared


def _affinities(idx, d2, perplexity):
    """idx int64 / d2 fp32 [n, k] on the device -> (p_cond [n, k], beta [n], rowptr, col, p, nnz) on the CPU; guard entries, the
    workspace's end and the inputs checked."""
    from src import _native as N
    n, k = d2.shape
    cap = 2 * n * k
    idx32 = idx.to(torch.int32).contiguous()
    keep_i, keep_d = idx32.clone(), d2.clone()
    pc, beta = _guarded(n * k, torch.float32, -7.5), _guarded(n, torch.float32, -7.5)
    N.call("tsne_calibrate", d2, n, k, float(perplexity), pc, beta)
    rowptr, col = _guarded(n + 1, torch.int32, -77), _guarded(cap, torch.int32, -77)
    p, nnz = _guarded(cap, torch.float32, -7.5), _guarded(1, torch.int32, -77)
    ws, nbytes = _workspace(n, k)
    pcc = pc[:n * k].clone()
    N.call("tsne_symmetrize", idx32, pcc, n, k, rowptr, col, p, nnz, ws, nbytes)
    torch.cuda.synchronize()
    assert _intact(pc, n * k, -7.5) and _intact(beta, n, -7.5) and _intact(rowptr, n + 1, -77) and _intact(col, cap, -77)
    assert _intact(p, cap, -7.5) and _intact(nnz, 1, -77), "guard entries overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "workspace overrun"
    assert torch.equal(idx32, keep_i) and torch.equal(d2, keep_d) and torch.equal(pcc, pc[:n * k])
    m = int(nnz[0])
    assert bool((col[m:cap] == -77).all()) and bool((p[m:cap] == -7.5).all())               # nothing behind nnz is touched
    return (pc[:n * k].reshape(n, k).cpu().numpy(), beta[:n].cpu().numpy(), rowptr[:n + 1].cpu().numpy(), col[:m].cpu().numpy(),
            p[:m].cpu().numpy(), m)


def _points(n, d, seed):
    rng = np.random.RandomState(seed)
    c = rng.randn(5, d) * 3.0
    return (c[np.arange(n) % 5] + rng.randn(n, d)).astype(np.float32)


def _check_csr(rowptr, col, p, nnz, n, idx):
    assert rowptr[0] == 0 and rowptr[n] == nnz and (np.diff(rowptr) > 0).all()
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    assert (col >= 0).all() and (col < n).all() and (col != rows).all()                       # no diagonal entry
    same = rows[1:] == rows[:-1]
    assert (np.diff(col)[same] > 0).all()                                                     # columns ascend in every row
    D = R.csr_to_dense(rowptr, col, p, n)
    assert np.array_equal(D, D.T) and (p > 0).all()
    pattern = np.zeros((n, n), dtype=bool)
    pattern[np.repeat(np.arange(n), idx.shape[1]), idx.reshape(-1)] = True
    assert nnz == int((pattern | pattern.T).sum())
    return D


@pytest.mark.parametrize("n,d,perplexity", [(62, 8, 20.0), (257, 30, 5.0), (600, 16, 21.0)])
def test_affinities_against_the_restatement(n, d, perplexity):
    """k = 61 = n - 1; d % 4 != 0 and n % 256 = 1; k = 64.  The stages are judged from the idx and d2 that knn_graph itself returned."""
    from src.evaluation.graph import knn_graph
    from src.evaluation.tsne import neighbour_count, tsne_affinities
    x = torch.from_numpy(_points(n, d, seed=n)).cuda()
    k = neighbour_count(n, perplexity)
    idx, d2 = knn_graph(x, k)
    pc, beta, rowptr, col, p, nnz = _affinities(idx, d2, perplexity)
    idx_h, d2_h = idx.cpu().numpy(), d2.cpu().numpy()
    p64 = pc.astype(np.float64)
    H = -(p64 * np.log(np.where(p64 > 0, p64, 1.0))).sum(1)
    h_err, row_err = float(np.abs(H - np.log(perplexity)).max()), float(np.abs(p64.sum(1) - 1.0).max())
    D = _check_csr(rowptr, col, p, nnz, n, idx_h)
    ref = R.joint(idx_h, R.calibrate(d2_h, perplexity)[0])
    bar = 4.0 * R.rel_l2(R.joint(idx_h, R.calibrate(d2_h, perplexity, f32=True)[0]), ref)
    err = R.rel_l2(D, ref)
    print(f"tsne affinities n {n} d {d} perplexity {perplexity:g} k {k}: max |H - log perplexity| {h_err:.3e}, max |row sum - 1| {row_err:.2e}, "
          f"|sum P - 1| {abs(D.sum() - 1.0):.2e}, P rel-L2 {err:.3e} / bar {bar:.3e} = {err / bar:.4f}, nnz {nnz}")
    assert np.isfinite(pc).all() and np.isfinite(beta).all() and (beta > 0).all()
    assert h_err <= 1e-5 and row_err <= 1e-6 and abs(D.sum() - 1.0) <= 1e-6
    assert err <= bar
    # the Python layer: the same bits, with its own graph or the caller's
    for P in (tsne_affinities(x, perplexity), tsne_affinities(x, perplexity, neighbours=(idx, d2))):
        assert P.n == n and int(P.nnz[0]) == nnz and P.w.dtype == torch.float32
        assert np.array_equal(P.rowptr.cpu().numpy(), rowptr) and np.array_equal(P.col[:nnz].cpu().numpy(), col)
        assert np.array_equal(P.w[:nnz].cpu().numpy(), p)


def test_affinities_of_duplicated_points():
    """70 copies of one point among 200 others, perplexity 20 (k = 61): a copy's 61 nearest are copies at distance exactly 0, its row
    cannot reach the entropy and ends after 100 doublings as the uniform row; everything stays finite."""
    from src.evaluation.graph import knn_graph
    x = _points(270, 12, seed=5)
    copies = np.random.RandomState(6).permutation(270)[:70]
    x[copies] = x[copies[0]]
    idx, d2 = knn_graph(torch.from_numpy(x).cuda(), 61)
    assert bool((d2[torch.from_numpy(copies).cuda()] == 0).all())
    pc, beta, rowptr, col, p, nnz = _affinities(idx, d2, 20.0)
    assert np.isfinite(pc).all() and np.isfinite(beta).all() and np.isfinite(p).all()
    idx_h, d2_h = idx.cpu().numpy(), d2.cpu().numpy()
    flat = d2_h.max(1) == d2_h.min(1)                                   # the copies, and any point whose 61 nearest are all copies
    assert flat[copies].all() and 70 <= int(flat.sum()) <= 80
    assert (pc[flat] == np.float32(1.0 / 61.0)).all() and (beta[flat] == np.float32(2.0 ** 100)).all()
    p64 = pc[~flat].astype(np.float64)
    H = -(p64 * np.log(np.where(p64 > 0, p64, 1.0))).sum(1)
    assert float(np.abs(H - np.log(20.0)).max()) <= 1e-5
    D = _check_csr(rowptr, col, p, nnz, 270, idx_h)
    assert abs(D.sum() - 1.0) <= 1e-6
    ref = R.joint(idx_h, R.calibrate(d2_h, 20.0)[0])
    bar = 4.0 * R.rel_l2(R.joint(idx_h, R.calibrate(d2_h, 20.0, f32=True)[0]), ref)
    print(f"tsne affinities with 70 duplicates: P rel-L2 {R.rel_l2(D, ref):.3e} / bar {bar:.3e}")
    assert R.rel_l2(D, ref) <= bar


# ---- gradient -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(n):
    """-> (x float32 [n, 16], the device Csr, dense P float64 of exactly the values the device holds)"""
    from src.evaluation.tsne import tsne_affinities
    x = _points(n, 16, seed=1000 + n)
    P = tsne_affinities(torch.from_numpy(x).cuda(), 20.0)
    m = int(P.nnz[0])
    D = R.csr_to_dense(P.rowptr.cpu().numpy(), P.col[:m].cpu().numpy(), P.w[:m].cpu().numpy(), n)
    return x, P, D


def _layout(name, x):
    from src.evaluation.tsne import pca_init
    if name == "pca":
        return pca_init(torch.from_numpy(x)).numpy()
    y = (3.0 * np.random.RandomState(len(x)).randn(len(x), 2)).astype(np.float32)
    if name == "coincident":
        y[1], y[3] = y[0], y[2]
    return y


def _gradient(P, y, exaggeration):
    """-> (grad [n, 2], rep [n, 2], Z, kl) on the CPU from the raw entries; guards, workspace end and inputs checked."""
    from src import _native as N
    n = P.n
    yd = torch.from_numpy(y).cuda()
    rep, grad = _guarded(2 * n, torch.float32, -7.5), _guarded(2 * n, torch.float32, -7.5)
    Z, kl = _guarded(1, torch.float64, -7.5), _guarded(1, torch.float64, -7.5)
    ws, nbytes = _workspace(n)
    N.call("tsne_repulsion", yd, n, rep, Z, ws, nbytes)
    N.call("tsne_gradient", P.rowptr, P.col, P.w, P.col.numel(), yd, rep, Z, n, float(exaggeration), grad, kl, ws, nbytes)
    torch.cuda.synchronize()
    assert _intact(rep, 2 * n, -7.5) and _intact(grad, 2 * n, -7.5) and _intact(Z, 1, -7.5) and _intact(kl, 1, -7.5), "guard entries overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "workspace overrun"
    assert torch.equal(yd.cpu(), torch.from_numpy(y))
    return grad[:2 * n].reshape(n, 2).cpu(), rep[:2 * n].reshape(n, 2).cpu(), Z[:1].cpu(), kl[:1].cpu()


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
@pytest.mark.parametrize("layout", ["pca", "random", "coincident"])
@pytest.mark.parametrize("n", [257, 600, 1030])
def test_gradient_against_the_restatement(n, layout, exaggeration):
    """n = 1030: five row blocks with a ragged tail, the walked range split five ways, so the fold of the partials runs.
    The layouts are not converged ones: there the two force sums cancel and float32 itself loses four digits."""
    from src.evaluation.tsne import tsne_gradient
    x, P, D = _problem(n)
    y = _layout(layout, x)
    grad, rep, Z, kl = _gradient(P, y, exaggeration)
    want, want_kl, want_z, want_rep = R.kl_and_gradient(D, y, exaggeration)
    bar = 4.0 * R.rel_l2(R.kl_and_gradient(D, y, exaggeration, f32=True)[0], want)
    err, rep_err = R.rel_l2(grad.numpy(), want), R.rel_l2(rep.numpy(), want_rep)
    z_err, kl_err = abs(float(Z) - want_z) / want_z, abs(float(kl) - want_kl)
    print(f"tsne gradient n {n} {layout} exaggeration {exaggeration:g}: grad rel-L2 {err:.3e} / bar {bar:.3e} = {err / bar:.4f}, "
          f"rep rel-L2 {rep_err:.3e}, Z rel {z_err:.2e}, |KL - ref| {kl_err:.2e} (KL {want_kl:.4f})")
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(rep).all()) and np.isfinite(float(Z)) and np.isfinite(float(kl))
    assert err <= bar
    assert z_err <= 1e-6 and kl_err <= 1e-6
    # a second call, and the Python layer: the same bits
    grad2, rep2, Z2, kl2 = _gradient(P, y, exaggeration)
    g3, kl3 = tsne_gradient(P, torch.from_numpy(y).cuda(), exaggeration)
    for a, b in ((grad, grad2), (rep, rep2), (grad, g3.cpu())):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in ((Z, Z2), (kl, kl2), (kl, kl3.cpu())):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_gradient_without_the_kl_is_the_same_gradient():
    from src import _native as N
    x, P, D = _problem(600)
    y = _layout("random", x)
    grad, rep, Z, _ = _gradient(P, y, 12.0)
    g = _guarded(2 * 600, torch.float32, -7.5)
    N.call("tsne_gradient", P.rowptr, P.col, P.w, P.col.numel(), torch.from_numpy(y).cuda(), rep.cuda().contiguous(), Z.cuda(), 600, 12.0, g,
           None, None, 0)
    assert _intact(g, 1200, -7.5) and torch.equal(g[:1200].cpu().view(torch.int32), grad.reshape(-1).view(torch.int32))


# ---- update -------------------------------------------------------------------------------------------------------------------
def test_update_rule():
    """gains exactly the rule in torch fp32; update and y within 1e-6 of their largest magnitude (a contracted fma saves one rounding
    of 2^-24 per operation)."""
    from src import _native as N
    n = 1030
    g = torch.Generator().manual_seed(3)
    y, upd, grad = (torch.randn(2 * n, generator=g) * s for s in (5.0, 0.3, 1e-3))
    gains = torch.rand(2 * n, generator=g) * 3.0 + 0.005
    gains[:40] = 0.011                                                  # 0.8 x: below the floor of 0.01
    upd[40:80] = 0.0                                                    # a product of 0 is not "< 0": the gain shrinks
    grad[80:100] = 0.0
    momentum, lr = 0.8, 85.75
    yd, ud, gd = (_guarded(2 * n, torch.float32, -7.5) for _ in range(3))
    yd[:2 * n], ud[:2 * n], gd[:2 * n] = y.cuda(), upd.cuda(), gains.cuda()
    gradd = grad.cuda()
    N.call("tsne_update", gradd, n, momentum, lr, yd, ud, gd)
    torch.cuda.synchronize()
    assert _intact(yd, 2 * n, -7.5) and _intact(ud, 2 * n, -7.5) and _intact(gd, 2 * n, -7.5) and torch.equal(gradd.cpu(), grad)
    inc = upd * grad < 0
    want_g = torch.where(inc, gains + 0.2, gains * 0.8).clamp_min(0.01)
    assert int(inc.sum()) > 500 and int((~inc).sum()) > 500 and bool((want_g[:40][~inc[:40]] == 0.01).all()) and int((~inc[:40]).sum()) > 5
    assert torch.equal(gd[:2 * n].cpu(), want_g)
    want_u = torch.from_numpy(R.update(y.double().numpy(), upd.double().numpy(), gains.double().numpy(), grad.double().numpy(), momentum, lr)[1])
    want_y = y.double() + want_u
    eu = float((ud[:2 * n].cpu().double() - want_u).abs().max() / want_u.abs().max())
    ey = float((yd[:2 * n].cpu().double() - want_y).abs().max() / want_y.abs().max())
    print(f"tsne update: max |update - ref| / max |update| {eu:.2e}, max |y - ref| / max |y| {ey:.2e}")
    assert eu <= 1e-6 and ey <= 1e-6


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_map_separates_blobs():
    """Six blobs of 100 points, d = 16, centre spread 4, perplexity 20, 500 iterations, PCA init.  The float64 restatement alone:
    purity 1.000 and a final KL of 0.27 - 0.30 of the initial one on three such sets.  No trajectory is compared: the gain rule is
    discontinuous and 500 steps amplify a rounding."""
    from src.evaluation.tsne import pca_init, tsne, tsne_affinities, tsne_gradient
    x, labels = R.blobs(100, 6, 16, 4.0, seed=8)
    xd = torch.from_numpy(x).cuda()
    y, kl = tsne(xd, perplexity=20.0, n_iter=500, return_kl=True)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (600, 2) and bool(torch.isfinite(y).all())
    kl0 = float(tsne_gradient(tsne_affinities(xd, 20.0), pca_init(xd).cuda())[1])
    purity = R.purity(y.cpu().numpy(), labels)
    print(f"tsne map of 6 x 100 blobs: purity {purity:.4f}, KL {kl0:.4f} -> {kl:.4f} ({kl / kl0:.3f} of the initial)")
    assert purity >= 0.99 and kl <= 0.5 * kl0
    y2 = tsne(xd, perplexity=20.0, n_iter=500)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32))
    # other initialisations run the same loop
    yr = tsne(xd, n_iter=3, init="random", seed=4)
    assert torch.equal(yr.view(torch.int32), tsne(xd, n_iter=3, init="random", seed=4).view(torch.int32))
    assert not torch.equal(yr, tsne(xd, n_iter=3, init="random", seed=5))
    y0 = torch.from_numpy(R.pca_init(x).astype(np.float32)).cuda()
    assert torch.equal(tsne(xd, n_iter=0, init=y0), y0)


# ---- the labeler --------------------------------------------------------------------------------------------------------------
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


def _write_wavs(tmp_path, lengths, salt):
    from scipy.io import wavfile
    files = []
    for i, L in enumerate(lengths):
        w = fill.uniform((L,), salt + i, -0.3, 0.3) + 0.2 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(L) / 16000).astype(np.float32)
        p = str(tmp_path / f"clip{salt}_{i}.wav")
        wavfile.write(p, 16000, (w * 32767).astype(np.int16))
        files.append(p)
    return files


def test_labeler_map(tmp_path, cfg_s, capsys):
    """The 12-clip checkpoint fixture of tests/test_gpu_silhouette.py, rebuilt here."""
    import pandas as pd
    from src.upstream.decar_v2 import store_clusters as sc
    ckpt = _checkpoint(tmp_path, cfg_s)
    files = _write_wavs(tmp_path, [16000 + 500 * (i % 3) for i in range(12)], salt=300)
    files_csv = str(tmp_path / "files.csv")
    pd.DataFrame({"files": files}).to_csv(files_csv, index=False)
    base = ["--checkpoint", ckpt, "--upstream", "delores_s", "--input", files_csv, "--pca", "8", "--window", "center", "--k", "3"]
    np.random.seed(2)
    plain_labels = sc.main(sc.get_args(base + ["--out", str(tmp_path / "plain.csv")]))
    plain = capsys.readouterr().out
    assert len(plain.splitlines()) == 1                                  # without --map the command prints what it printed
    np.random.seed(2)
    labels = sc.main(sc.get_args(base + ["--out", str(tmp_path / "out.csv"), "--map", str(tmp_path / "m.csv"), "--perplexity", "3",
                                         "--map_iters", "50"]))
    text = capsys.readouterr().out.splitlines()
    assert open(tmp_path / "out.csv", "rb").read() == open(tmp_path / "plain.csv", "rb").read()
    np.testing.assert_array_equal(labels, plain_labels)
    assert len(text) == 2 and text[0].replace("out.csv", "plain.csv") == plain.splitlines()[0]
    assert text[1].startswith("map of 12 files, perplexity 3, 50 iterations, KL ") and text[1].endswith(f"-> {tmp_path / 'm.csv'}")
    assert np.isfinite(float(text[1].split("KL ")[1].split(" ")[0]))
    assert open(tmp_path / "m.csv").readline().strip() == "files,label,x,y"
    m = pd.read_csv(tmp_path / "m.csv")
    assert list(m.columns) == ["files", "label", "x", "y"] and list(m["files"]) == files and len(m) == 12
    assert list(m["label"]) == list(pd.read_csv(tmp_path / "out.csv")["label"]) == [int(c) for c in labels]
    assert np.isfinite(m[["x", "y"]].to_numpy()).all() and m["x"].std() > 0
    # the default perplexity 20 does not fit 12 files: refused before the embedding, nothing written
    with pytest.raises(ValueError, match="below the 11 neighbours"):
        sc.main(sc.get_args(base + ["--out", str(tmp_path / "no.csv"), "--map", str(tmp_path / "no_map.csv")]))
    assert not (tmp_path / "no.csv").exists() and not (tmp_path / "no_map.csv").exists()
