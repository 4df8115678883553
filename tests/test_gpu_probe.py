"""Linear-probe grid on the GPU: `audiossl_probe_batch` / `_ce` / `_adamw` against the restatements of `tests/probe_ref.py`,
`LinearProbeGrid.fit` against `fit_ref` with the same permutations, one grid against separate fits, and the command.

Tolerances that cannot be derived are measured in place (probe_ref.bound): the restatement runs in fp32 on the CPU and in fp64 on
the same inputs; the kernel may differ from fp64 by 4 x that largest difference plus one fp32 ulp of the largest reference
magnitude.  For a relative L2 error the floor is one fp32 ulp of 1.0 (2^-23).  Every test prints kernel error / bound."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

import probe_ref as R

pytestmark = pytest.mark.gpu

GUARD = 2
POISON = -7777.5


# ---- 1. probe_batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,b", [(5, 8, 1), (300, 64, 257), (70, 2048, 64)])
@pytest.mark.parametrize("stats,extra", [(True, 0), (False, 0), (True, 12)])
def test_probe_batch_bit_equal_to_numpy(n, d, b, stats, extra):
    from src import _native as N
    g = torch.Generator().manual_seed(n + d + b)
    X = torch.randn(n, d, generator=g) * 2.0 + 0.3
    mean = torch.randn(d, generator=g) * 0.5
    rstd = 1.0 / (torch.rand(d, generator=g) + 0.5)
    if b == 1:
        idx = torch.tensor([n - 1], dtype=torch.int32)
    else:
        idx = torch.randint(0, n, (b,), generator=g).to(torch.int32)
        idx[:4] = torch.tensor([n - 1, n - 2, 1, 0], dtype=torch.int32)[:min(4, b)]      # descending
        idx[4:7] = idx[4]                                                                # repeated
        idx[b // 2], idx[b - 1] = -1, n                                                  # outside [0, N): never read
    ldo = d + 8 + extra
    out = torch.full((b + GUARD, ldo), POISON)
    Xd, out_d = X.cuda(), out.cuda()
    md, rd = (mean.cuda(), rstd.cuda()) if stats else (None, None)
    N.call("probe_batch", Xd, n, d, idx.cuda(), b, md, rd, out_d, ldo)
    torch.cuda.synchronize()
    got = out_d.cpu()
    assert bool((got[b:] == POISON).all()), "guard rows overwritten"
    assert torch.equal(Xd.cpu(), X)
    bad = (idx < 0) | (idx >= n)
    rows = idx[~bad].long().numpy()
    want = X.numpy()[rows]
    if stats:
        want = (want - mean.numpy()[None, :]) * rstd.numpy()[None, :]             # numpy fp32: subtract, then multiply
    good = got[:b][~bad].numpy()
    assert good[:, :d].tobytes() == want.astype(np.float32).tobytes()
    assert bool((good[:, d] == 1.0).all()) and bool((good[:, d + 1:] == 0.0).all())
    assert bool(torch.isnan(got[:b][bad]).all()) and int(bad.sum()) == (0 if b == 1 else 2)
    ref = R.batch_ref(X, idx, mean if stats else None, rstd if stats else None, ldo, dtype=torch.float32)
    assert torch.equal(torch.nan_to_num(ref, nan=123.0), torch.nan_to_num(got[:b], nan=123.0))


# ---- 2. probe_ce against fp64 -----------------------------------------------------------------------------------------------------
def _ce_launch(logits, label, H, C, Cp, gscale, train=True, loss0=None, correct0=None):
    """The C entry on a dlogits buffer poisoned everywhere, with guard rows -> (loss_sum, correct, dlogits | None) on the CPU."""
    from src import _native as N
    B, ld = logits.shape
    loss = (torch.zeros(H, dtype=torch.float64) if loss0 is None else loss0.clone()).cuda()
    correct = (torch.zeros(H, dtype=torch.int64) if correct0 is None else correct0.clone()).cuda()
    ld_d, lab_d = logits.cuda(), label.cuda()
    dl = torch.full((B + GUARD, ld), POISON).cuda() if train else None
    N.call("probe_ce", ld_d, ld, lab_d, B, H, C, Cp, float(gscale), loss, correct, dl)
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(ld_d.cpu(), nan=5.0), torch.nan_to_num(logits, nan=5.0)) and torch.equal(lab_d.cpu(), label)
    if train:
        dl = dl.cpu()
        assert bool((dl[B:] == POISON).all()), "guard rows overwritten"
        assert bool((dl[:B, H * Cp:] == POISON).all()), "columns at and beyond H Cp touched"
        dl = dl[:B, :H * Cp]
    return loss.cpu(), correct.cpu(), dl


def _ce_inputs(B, H, C, extra, seed):
    Cp = (C + 7) // 8 * 8
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, H * Cp + extra, generator=g) * 3.0
    for h in range(H):
        logits[:, h * Cp + C:(h + 1) * Cp] = float("nan")            # whatever the pad columns hold is never used
    label = torch.randint(0, C, (B,), generator=g)
    return Cp, logits, label


@pytest.mark.parametrize("B,H,C", [(1, 1, 2), (7, 3, 35), (64, 12, 37), (257, 2, 1251), (3, 1, 4096),
                                   (21, 2, 300),       # four waves per row (256 < C <= 1024), rows not a multiple of four
                                   (70, 2, 64),        # the widest row of 16 lanes, more than one pass of 64 rows
                                   (19, 2, 130)])      # a wave per row (64 < C <= 256)
@pytest.mark.parametrize("extra", [0, 12])
def test_probe_ce_against_fp64(B, H, C, extra):
    Cp, logits, label = _ce_inputs(B, H, C, extra, 100 + B + C)
    gscale = 1.0 / B
    clean = torch.nan_to_num(logits, nan=0.0)
    l64, c64, g64 = R.ce_heads_ref(clean, label, H, C, Cp, gscale, dtype=torch.float64)
    l32, _, g32 = R.ce_heads_ref(clean, label, H, C, Cp, gscale, dtype=torch.float32)
    loss, correct, dl = _ce_launch(logits, label, H, C, Cp, gscale)
    b_loss, b_grad = R.bound(l32, l64), R.bound(g32, g64)
    e_loss, e_grad = float((loss - l64).abs().max()), float((dl.double() - g64).abs().max())
    print(f"probe_ce B {B} H {H} C {C} ld+{extra}: loss err {e_loss:.3e} / bound {b_loss:.3e} = {e_loss / b_loss:.3f}; "
          f"dlogits err {e_grad:.3e} / bound {b_grad:.3e} = {e_grad / b_grad:.3f}")
    assert e_loss <= b_loss
    assert e_grad <= b_grad
    assert torch.equal(correct, c64)                                 # the arg-max is exact on the logits as given
    for h in range(H):
        assert bool((dl[:, h * Cp + C:(h + 1) * Cp] == 0).all()), "pad columns must be exactly 0"
    # the forward-only form: the same sums bit for bit
    loss_e, correct_e, _ = _ce_launch(logits, label, H, C, Cp, gscale, train=False)
    assert torch.equal(loss_e, loss) and torch.equal(correct_e, correct)
    # a second launch on the first one's sums accumulates, and repeats the first bit for bit
    loss2, correct2, dl2 = _ce_launch(logits, label, H, C, Cp, gscale, loss0=loss, correct0=correct)
    assert torch.equal(loss2, loss + loss) and torch.equal(correct2, 2 * correct)
    assert torch.equal(dl2, dl)


# ---- 3. probe_ce exact cases ----------------------------------------------------------------------------------------------------
def test_probe_ce_counts_first_argmax_with_planted_ties():
    B, H, C = 40, 3, 35
    Cp = 40
    g = torch.Generator().manual_seed(9)
    logits = torch.randint(-3, 3, (B, H * Cp), generator=g).float()              # many ties at the maximum already
    label = torch.randint(0, C, (B,), generator=g)
    for h in range(H):
        z = logits[:, h * Cp:h * Cp + C]
        z[0, :] = 1.0                                                            # everything ties: class 0 wins
        label[0] = 0
        z[1, :] = 1.0
        label[1] = 5                                                             # the label ties with lower classes: a miss
        z[2, :] = -2.0
        z[2, 7], z[2, 20] = 4.0, 4.0
        label[2] = 20                                                            # tie between the label and a lower class: a miss
        z[3, :] = -2.0
        z[3, 7], z[3, 20] = 4.0, 4.0
        label[3] = 7                                                             # ... and the lower one is the label: a hit
        z[4, :] = 0.0
        z[4, C - 1] = 2.0
        label[4] = C - 1                                                         # the last class alone
        logits[:, h * Cp + C:(h + 1) * Cp] = 100.0                               # pad columns larger than every class: ignored
    want = torch.zeros(H, dtype=torch.int64)
    for h in range(H):
        z = logits[:, h * Cp:h * Cp + C]
        first = torch.tensor([int(torch.nonzero(r == r.max())[0]) for r in z])
        assert torch.equal(first, z.argmax(dim=1))                               # torch.argmax: ties to the lowest index
        want[h] = int((first == label).sum())
    _, c64, _ = R.ce_heads_ref(logits, label, H, C, Cp, 1.0)
    assert torch.equal(c64, want)
    loss, correct, _ = _ce_launch(logits, label, H, C, Cp, 1.0)
    assert correct.dtype == torch.int64 and torch.equal(correct, want)
    assert bool(torch.isfinite(loss).all())


@pytest.mark.parametrize("C", [35, 1251])
def test_probe_ce_extreme_logits_stay_finite(C):
    B, H = 6, 2
    Cp = (C + 7) // 8 * 8
    logits = torch.full((B, H * Cp), -1e4)
    label = torch.tensor([0, 1, C - 1, 3, 2, C - 2])
    logits[0, 0], logits[0, Cp] = 1e4, 1e4                  # right with certainty: loss 0
    logits[1, 0], logits[1, Cp] = 1e4, 1e4                  # wrong with certainty: loss 2e4
    logits[2] = 1e4                                         # all equal and huge: loss log C
    logits[3, :] = torch.where(torch.arange(H * Cp) % 2 == 0, 1e4, -1e4)
    l64, c64, g64 = R.ce_heads_ref(logits, label, H, C, Cp, 0.5)
    loss, correct, dl = _ce_launch(logits, label, H, C, Cp, 0.5)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all())
    assert torch.equal(correct, c64)
    assert float((loss - l64).abs().max()) <= 1e-6 * float(l64.abs().max())          # 2e4 + ...: fp32 soft-max sums, fp64 row sums
    assert float((dl.double() - g64).abs().max()) <= 1e-6


def test_probe_ce_label_outside_the_classes_is_loud():
    B, H, C, Cp = 9, 3, 35, 40
    _, logits, label = _ce_inputs(B, H, C, 0, 77)
    good_loss, good_correct, good_dl = _ce_launch(logits, label, H, C, Cp, 0.25)
    for bad_value in (-1, C):
        lab = label.clone()
        lab[4] = bad_value
        loss, correct, dl = _ce_launch(logits, lab, H, C, Cp, 0.25)
        assert bool(torch.isnan(loss).all())                                     # every head's sum
        for h in range(H):
            assert bool(torch.isnan(dl[4, h * Cp:h * Cp + C]).all())
            assert bool((dl[4, h * Cp + C:(h + 1) * Cp] == 0).all())             # the pad columns stay zero: W's pad rows never move
        keep = [r for r in range(B) if r != 4]
        assert torch.equal(dl[keep], good_dl[keep])                              # the other rows are unaffected
        loss_e, correct_e, _ = _ce_launch(logits, lab, H, C, Cp, 0.25, train=False)
        assert bool(torch.isnan(loss_e).all()) and torch.equal(correct_e, correct)


# ---- 4. probe_adamw --------------------------------------------------------------------------------------------------------------
LRS3, WDS3 = [1e-2, 0.0, 1e-3], [0.0, 0.0, 0.1]


def _adamw_run(W0, grads, lrs, wds, seg, lr_scale):
    from src import _native as N
    H = len(lrs)
    pad = 8
    bufs = [torch.cat([t, torch.full((pad,), POISON)]).cuda() for t in (W0, torch.zeros_like(W0), torch.zeros_like(W0))]
    W, m, v = bufs
    lr, wd = torch.tensor(lrs, dtype=torch.float32).cuda(), torch.tensor(wds, dtype=torch.float32).cuda()
    step = torch.zeros(1, dtype=torch.int64).cuda()
    for g in grads:
        gd = g.cuda()
        step.add_(1)
        N.call("probe_adamw", W, gd, m, v, H, seg, lr, wd, float(lr_scale), R.BETAS[0], R.BETAS[1], R.EPS, step)
        torch.cuda.synchronize()
        assert torch.equal(gd.cpu(), g)
    for t in bufs:
        assert bool((t[H * seg:] == POISON).all()), "wrote beyond the last segment"
    return W[:H * seg].cpu(), m[:H * seg].cpu(), v[:H * seg].cpu()


@pytest.mark.parametrize("seg", [8 * 16, 40 * 72])
def test_probe_adamw_against_torch_adamw_per_head(seg):
    H, steps = 3, 5
    g = torch.Generator().manual_seed(seg)
    W0 = torch.randn(H * seg, generator=g)
    grads = [torch.randn(H * seg, generator=g) * 0.1 for _ in range(steps)]
    ref64 = R.adamw_heads_ref(W0, grads, LRS3, WDS3, seg, dtype=torch.float64)
    ref32 = R.adamw_heads_ref(W0, grads, LRS3, WDS3, seg, dtype=torch.float32)
    got = _adamw_run(W0, grads, LRS3, WDS3, seg, 1.0)
    for name, k, r32, r64 in zip(("W", "m", "v"), got, ref32, ref64):
        b, e = R.bound(r32, r64), float((k.double() - r64).abs().max())
        print(f"probe_adamw seg {seg} {name}: err {e:.3e} / bound {b:.3e} = {e / b:.3f}")
        assert e <= b, name
    assert torch.equal(got[0][seg:2 * seg], W0[seg:2 * seg]), "the head with lr = 0 and wd = 0 must stay bit-unchanged"
    assert not torch.equal(got[0][:seg], W0[:seg]) and not torch.equal(got[0][2 * seg:], W0[2 * seg:])
    # lr_scale = 0.5 is the halved learning rates, bit for bit
    half = _adamw_run(W0, grads, LRS3, WDS3, seg, 0.5)
    halved = _adamw_run(W0, grads, [0.5 * v for v in LRS3], WDS3, seg, 1.0)
    assert all(torch.equal(a, b) for a, b in zip(half, halved))
    assert not torch.equal(half[0], got[0])


# ---- 5 / 6. the grid ------------------------------------------------------------------------------------------------------------------
FIT = dict(n=520, n_val=200, d=64, c=5, lrs=[1e-3, 1e-2], wds=[0.0, 1e-2], epochs=3, batch=64, sep=1.2, seed=31, perm_seed=5)


def fit_data(cfg=FIT):
    """Gaussian classes: unit-variance noise around `c` random centres of norm `sep` * sqrt(d) / 2, an affine distortion on top so
    that the standardisation has something to do."""
    g = torch.Generator().manual_seed(cfg["seed"])
    centres = torch.randn(cfg["c"], cfg["d"], generator=g) * cfg["sep"] * 0.5
    scale, shift = torch.rand(cfg["d"], generator=g) * 3.0 + 0.2, torch.randn(cfg["d"], generator=g) * 2.0

    def draw(n):
        y = torch.randint(0, cfg["c"], (n,), generator=g)
        return ((centres[y] + torch.randn(n, cfg["d"], generator=g)) * scale + shift).contiguous(), y
    X, y = draw(cfg["n"])
    Xv, yv = draw(cfg["n_val"])
    return X, y, Xv, yv


@functools.lru_cache(maxsize=None)
def _fit_reference():
    """Computed once and shared (never modified): data, the stats the grid uses, fit_ref in fp64 and fp32 with the grid's permutations."""
    from src.evaluation import epoch_permutations, feature_stats
    X, y, Xv, yv = fit_data()
    stats = tuple(t.cpu() for t in feature_stats(X.cuda()))
    perms = epoch_permutations(FIT["n"], FIT["epochs"], torch.Generator().manual_seed(FIT["perm_seed"]))
    hparams = [(lr, wd) for lr in FIT["lrs"] for wd in FIT["wds"]]
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        heads = R.fit_ref(X, y, FIT["c"], hparams, perms, FIT["batch"], stats=stats, dtype=dt)
        loss, logits = R.eval_ref(heads, Xv, yv, stats=stats, dtype=dt)
        out[name] = dict(heads=heads, loss=loss, logits=logits)
    return X, y, Xv, yv, stats, hparams, out


def _stack(weight, bias):
    return torch.cat([weight.double(), bias.double()[:, None]], dim=1)


def _folded(head, stats):
    from src.evaluation import fold_standardisation
    return _stack(*fold_standardisation(head[0], head[1], stats[0], stats[1]))


def _fit_grid(X, y, stats, lrs, wds):
    from src.evaluation import LinearProbeGrid
    grid = LinearProbeGrid(FIT["d"], FIT["c"], lrs, wds, stats=tuple(t.cuda() for t in stats))
    return grid.fit(X.cuda(), y.cuda(), FIT["epochs"], FIT["batch"], generator=torch.Generator().manual_seed(FIT["perm_seed"]))


def test_grid_fit_against_fit_ref():
    """N = 520, batch 64: every epoch ends in a batch of 8.  On the CPU the fp64 reference's top-2 logit margin exceeds 10 x the
    logit bound on 100 % of the 200 validation rows of every head (checked when this test was written; the test asserts >= 95 %)."""
    X, y, Xv, yv, stats, hparams, ref = _fit_reference()
    grid = _fit_grid(X, y, stats, FIT["lrs"], FIT["wds"])
    assert grid.hparams == hparams and int(grid.steps) == FIT["epochs"] * 9
    val = grid.evaluate(Xv.cuda(), yv.cuda(), slab=96)                        # three slabs, the last one short
    for h, (lr, wd) in enumerate(hparams):
        f64, f32 = _folded(ref["f64"]["heads"][h], stats), _folded(ref["f32"]["heads"][h], stats)
        b_head = 4.0 * R.rel_l2(f32, f64) + 2.0 ** -23
        e_head = R.rel_l2(_stack(*[t.cpu() for t in grid.head(h)]), f64)
        l64, l32 = ref["f64"]["loss"][h], ref["f32"]["loss"][h]
        b_loss = 4.0 * abs(l32 - l64) + R.ulp32(l64)
        e_loss = abs(val[h]["loss"] - l64)
        z64, z32 = ref["f64"]["logits"][h], ref["f32"]["logits"][h]
        b_logit = R.bound(z32, z64)
        top2 = z64.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 10.0 * b_logit
        share = float(clear.float().mean())
        print(f"grid fit head {h} lr {lr} wd {wd}: head rel-L2 {e_head:.3e} / bound {b_head:.3e} = {e_head / b_head:.3f}; "
              f"val loss err {e_loss:.3e} / bound {b_loss:.3e} = {e_loss / b_loss:.3f}; logit bound {b_logit:.3e}, clear rows {share:.3f}")
        assert (val[h]["lr"], val[h]["wd"]) == (lr, wd)
        assert e_head <= b_head, h
        assert e_loss <= b_loss, h
        assert share >= 0.95, h
        pred = grid.predict(Xv.cuda(), h).cpu()
        assert torch.equal(pred[clear], z64.argmax(dim=1)[clear]), h
        assert val[h]["top1"] == int((pred == yv).sum()) / yv.numel()
    # nothing moved that must not: pad rows and the columns behind the bias are still zero
    W = grid.W.cpu().view(grid.H, grid.Cp, grid.Dp)
    assert bool((W[:, FIT["c"]:, :] == 0).all()) and bool((W[:, :, FIT["d"] + 1:] == 0).all())
    assert bool((W[:, :FIT["c"], :FIT["d"] + 1] != 0).any())
    best = grid.select(val)
    assert val[best]["top1"] == max(v["top1"] for v in val)


def test_one_grid_agrees_with_separate_fits():
    """The four heads trained together against each trained alone (H = 1): the same bound as against fit_ref; not bit equality, the
    GEMM's N differs."""
    X, y, Xv, yv, stats, hparams, ref = _fit_reference()
    grid = _fit_grid(X, y, stats, FIT["lrs"], FIT["wds"])
    for h, (lr, wd) in enumerate(hparams):
        alone = _fit_grid(X, y, stats, [lr], [wd])
        assert alone.H == 1
        f64, f32 = _folded(ref["f64"]["heads"][h], stats), _folded(ref["f32"]["heads"][h], stats)
        bound = 4.0 * R.rel_l2(f32, f64) + 2.0 ** -23
        a, b = _stack(*[t.cpu() for t in alone.head(0)]), _stack(*[t.cpu() for t in grid.head(h)])
        e = R.rel_l2(b, a)
        print(f"grid vs alone head {h}: rel-L2 {e:.3e} / bound {bound:.3e} = {e / bound:.3f}")
        assert e <= bound, h
        assert R.rel_l2(a, f64) <= bound, h


def test_grid_step_is_five_launches_and_allocates_no_n_by_hc_matrix():
    from src import _native as N
    from src.evaluation import LinearProbeGrid
    n, d, c = 16384, 64, 35
    g = torch.Generator().manual_seed(2)
    X, y = torch.randn(n, d, generator=g).cuda(), torch.randint(0, c, (n,), generator=g).cuda()
    grid = LinearProbeGrid(d, c, [1e-3, 1e-2, 1e-1], [0.0, 1e-2])
    idx = torch.arange(128, dtype=torch.int32).cuda()
    grid.step(X, idx, y[:128].contiguous(), 1.0)                  # buffers exist now
    N.PROFILE, N.PROFILE_ALL = {}, True
    try:
        grid.step(X, idx, y[:128].contiguous(), 1.0)
        torch.cuda.synchronize()
        calls = {k: len(v) for k, v in N.PROFILE.items()}
    finally:
        N.PROFILE, N.PROFILE_ALL = None, False
    assert calls == {"audiossl_probe_batch": 1, "audiossl_gemm": 2, "audiossl_probe_ce": 1, "audiossl_probe_adamw": 1}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    grid.fit(X, y, 1, 128)
    grid.evaluate(X, y, slab=512)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    full = n * grid.H * grid.Cp * 4
    print(f"grid footprint: peak growth {growth / 2 ** 10:.0f} KiB (an N x H Cp matrix: {full / 2 ** 10:.0f} KiB)")
    assert growth < full // 4


# ---- 7. the command -------------------------------------------------------------------------------------------------------------------
def test_evaluate_linear_command(tmp_path, cfg_s, capsys):
    import importlib.util

    import pandas as pd
    from test_gpu_knn import _checkpoint, _write_wavs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("evaluate_linear_hip", os.path.join(root, "audio-ssl_amd", "evaluate_linear.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    ckpt = _checkpoint(tmp_path, copy.deepcopy(cfg_s))
    files, _ = _write_wavs(tmp_path, [16000 + 500 * (i % 3) for i in range(16)], salt=400)
    labels = ["dog", "cat", "bird"]
    train = pd.DataFrame({"wav": files[:12], "label": [labels[i % 3] for i in range(12)]})
    test = pd.DataFrame({"wav": files[12:], "label": [labels[i % 3] for i in range(4)]})
    train_csv, test_csv = str(tmp_path / "train.csv"), str(tmp_path / "test.csv")
    train.to_csv(train_csv, index=False)
    test.to_csv(test_csv, index=False)
    dump, head_path = str(tmp_path / "dump"), str(tmp_path / "head.pt")
    grid_args = ["--lrs", "1e-3,1e-2", "--wds", "0,1e-2", "--epochs", "2", "--probe_batch", "4", "--holdout", "0.25"]
    capsys.readouterr()
    res = ev.main(ev.get_args(["--checkpoint", ckpt, "--upstream", "delores_s", "--train_csv", train_csv, "--test_csv", test_csv,
                               "--dump_embeddings", dump, "--save_head", head_path] + grid_args))
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out == res
    assert set(out) == {"top1", "lr", "wd", "val_top1", "heads", "N_train", "N_valid", "N_test", "d", "epochs"}
    assert (out["N_train"], out["N_valid"], out["N_test"], out["d"], out["epochs"]) == (9, 3, 4, 2048, 2)      # 1 of 4 rows per class held out
    assert [(h["lr"], h["wd"]) for h in out["heads"]] == [(1e-3, 0.0), (1e-3, 1e-2), (1e-2, 0.0), (1e-2, 1e-2)]
    assert all(0.0 <= h["val_top1"] <= 1.0 and 0.0 <= h["test_top1"] <= 1.0 for h in out["heads"])
    picked = [h for h in out["heads"] if (h["lr"], h["wd"]) == (out["lr"], out["wd"])][0]
    assert picked["val_top1"] == out["val_top1"] == max(h["val_top1"] for h in out["heads"]) and picked["test_top1"] == out["top1"]
    assert np.load(os.path.join(dump, "train_embeddings.npy")).shape == (12, 2048)
    assert np.load(os.path.join(dump, "test_labels.npy")).tolist() == [2, 1, 0, 2]                # sorted ids: bird 0, cat 1, dog 2
    # the same line from the dumped embeddings, without a checkpoint
    again = ev.main(ev.get_args(["--embeddings", dump] + grid_args))
    line2 = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    assert line2 == line and again == res
    # the saved head applies to RAW embeddings
    from src.evaluation import LinearProbeGrid, feature_stats, stratified_holdout
    head = torch.load(head_path)
    assert head["labels"] == ["bird", "cat", "dog"] and (head["lr"], head["wd"]) == (out["lr"], out["wd"])
    assert head["weight"].shape == (3, 2048) and head["bias"].shape == (3,)
    x_all = torch.from_numpy(np.load(os.path.join(dump, "train_embeddings.npy")))
    y_all = torch.from_numpy(np.load(os.path.join(dump, "train_labels.npy")))
    x_te = torch.from_numpy(np.load(os.path.join(dump, "test_embeddings.npy")))
    keep, _ = stratified_holdout(y_all, 0.25, 0)
    x_tr = x_all[keep].contiguous().cuda()
    grid = LinearProbeGrid(2048, 3, [1e-3, 1e-2], [0.0, 1e-2], stats=feature_stats(x_tr))
    grid.fit(x_tr, y_all[keep].cuda(), 2, 4, generator=torch.Generator().manual_seed(0))
    best = [h for h, p in enumerate(grid.hparams) if p == (out["lr"], out["wd"])][0]
    w, b = grid.head(best)
    assert torch.equal(w.cpu(), head["weight"]) and torch.equal(b.cpu(), head["bias"])
    z = x_te.double() @ head["weight"].double().T + head["bias"].double()
    top2 = z.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3 * float(z.abs().max())
    assert torch.equal(grid.predict(x_te.cuda(), best).cpu()[clear], z.argmax(dim=1)[clear])
