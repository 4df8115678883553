"""Audio tagging on the GPU: `audiossl_tagging_stats` / `audiossl_bce_rows` against the int64 / fp64 restatements of
`tests/tagging_ref.py` and the recorded results of the reference's `calculate_stats`, the Python layer above them, and
`train_tagging.py` end to end for both encoder families.

Largest errors seen on an MI355X (each test prints its own), beside their bars:
  tagging_stats  npos / auc_num2 equal everywhere; |auc - ref| 0 in every case (bar 2^-52 = 2.2e-16); |ap - ref| at most 1.1e-16
                 (bar N 2^-51: 1.1e-13 at N = 257, 9.1e-12 at N = 20,383); against the recorded calculate_stats AP 1.1e-16,
                 AUC 1.1e-16 (bar 1e-12)
  bce_rows       loss at most 2.4e-8 relative (bar 2^-20 = 9.5e-7); fp32 dlogits at most 0.56 of the bar 4 * 2^-24 / (N C);
                 bf16 dlogits at most 0.996 of theirs (bf16 rounding alone is up to 2^-8 relative, which is the bar's second term)
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import tagging_ref as R

pytestmark = pytest.mark.gpu

GUARD = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C entries on guarded buffers ----------------------------------------------------------------------------------------
def _launch_stats(s, t):
    """`audiossl_tagging_stats` on buffers with guard elements of a recognisable pattern behind them and an 0xA5-filled, over-long
    workspace -> (npos int64, auc_num2 int64, ap fp64, auc fp64) numpy [C]."""
    from src import _native as N
    from src.evaluation.tagging import workspace_bytes
    n, c = s.shape
    sd, td = torch.from_numpy(np.ascontiguousarray(s)).cuda(), torch.from_numpy(np.ascontiguousarray(t.astype(np.uint8))).cuda()
    npos = torch.full((c + GUARD,), -5, dtype=torch.int32, device="cuda")
    num2 = torch.full((c + GUARD,), -7, dtype=torch.int64, device="cuda")
    ap = torch.full((c + GUARD,), 1000.5, dtype=torch.float64, device="cuda")
    auc = torch.full((c + GUARD,), -1000.5, dtype=torch.float64, device="cuda")
    nbytes = workspace_bytes(n, c)
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")           # 0xA5A5A5A5 is a NaN pattern: nothing may rely on zeros
    N.call("tagging_stats", sd, td, n, c, npos, num2, ap, auc, ws, nbytes)
    torch.cuda.synchronize()
    assert npos[c:].tolist() == [-5] * GUARD and num2[c:].tolist() == [-7] * GUARD, "guard overwritten"
    assert ap[c:].tolist() == [1000.5] * GUARD and auc[c:].tolist() == [-1000.5] * GUARD, "guard overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "workspace overrun"
    assert np.array_equal(sd.cpu().numpy(), s) and np.array_equal(td.cpu().numpy(), t.astype(np.uint8))
    return npos[:c].cpu().numpy().astype(np.int64), num2[:c].cpu().numpy(), ap[:c].cpu().numpy(), auc[:c].cpu().numpy()


def _check_stats(s, t, tag, ref=None):
    """The bars of every tagging_stats case: npos and auc_num2 EQUAL to the int64 reference, auc within 2^-52 of the reference's
    quotient, ap within N 2^-51 (the reordering of at most N fp64 terms in [0, 1]; one count off by one moves AP by at least
    1 / N^3, far above it), NaN exactly where the reference has NaN, and two launches agree bit for bit."""
    n = s.shape[0]
    ref = ref or R.stats(s, t)
    npos, num2, ap, auc = _launch_stats(s, t)
    again = _launch_stats(s, t)
    assert np.array_equal(npos, ref["npos"]), tag
    assert np.array_equal(num2, ref["auc_num2"]), tag
    nan = np.isnan(ref["auc"])
    assert np.array_equal(np.isnan(ap), nan) and np.array_equal(np.isnan(auc), nan), tag
    e_auc = float(np.abs(auc - ref["auc"])[~nan].max()) if (~nan).any() else 0.0
    e_ap = float(np.abs(ap - ref["AP"])[~nan].max()) if (~nan).any() else 0.0
    print(f"tagging_stats {tag}: |auc - ref| {e_auc:.3e} (bar {2.0 ** -52:.3e}), |ap - ref| {e_ap:.3e} (bar {n * 2.0 ** -51:.3e})")
    assert e_auc <= 2.0 ** -52 and e_ap <= n * 2.0 ** -51, tag
    for a, b in zip((npos, num2, ap, auc), again):
        assert a.tobytes() == b.tobytes(), "two launches on the same inputs differ"
    return npos, num2, ap, auc


def test_stats_hand_written_column():
    """scores 3 2 2 1 0, labels + - + + - (worked out in test_host_tagging.py): AP = (1 + 2/3 + 3/4) / 3, auc_num2 = 9."""
    s = np.array([[3], [2], [2], [1], [0]], dtype=np.float32)
    t = np.array([[1], [0], [1], [1], [0]], dtype=np.uint8)
    npos, num2, ap, auc = _check_stats(s, t, "hand-written")
    assert (int(npos[0]), int(num2[0]), float(auc[0])) == (3, 9, 0.75)
    assert abs(float(ap[0]) - (1 + 2 / 3 + 3 / 4) / 3) <= 5 * 2.0 ** -51


@pytest.mark.parametrize("i", range(len(R.GOLDEN_CASES)), ids=lambda i: "x".join(str(v) for v in R.GOLDEN_CASES[i][:2]))
def test_stats_golden_matrices(i, golden):
    """One sample past a 256 tile (257), several tiles with a ragged end (1000, 2049), a class count that fills no 16-class tile,
    tie groups that span positives and negatives (scores in multiples of 1/8, 1/3, 1/2); row 0 all-positive, row 1 all-negative,
    so every class is scored.  Against the numpy reference at the bars of `_check_stats`, against what the reference project's
    `calculate_stats` recorded at 1e-12, and through the Python layer (d' included, 1e-9 relative)."""
    from src.evaluation.tagging import tagging_stats
    g = golden("tagging_stats")
    s, t = g[f"scores_{i}"], g[f"targets_{i}"]
    npos, num2, ap, auc = _check_stats(s, t, str(R.GOLDEN_CASES[i]))
    e_ap, e_auc = float(np.abs(ap - g[f"AP_{i}"]).max()), float(np.abs(auc - g[f"auc_{i}"]).max())
    print(f"tagging_stats vs calculate_stats: AP {e_ap:.3e}, AUC {e_auc:.3e} (bar 1e-12)")
    assert e_ap <= 1e-12 and e_auc <= 1e-12
    st = tagging_stats(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda())
    assert np.array_equal(st["AP"], ap) and np.array_equal(st["auc"], auc) and np.array_equal(st["npos"], npos)
    assert st["classes_scored"] == s.shape[1]
    assert float(np.abs(st["d_prime"] / g[f"dprime_{i}"] - 1.0).max()) <= 1e-9
    assert st["mAP"] == pytest.approx(float(g[f"AP_{i}"].mean()), abs=1e-12) and st["mAUC"] == pytest.approx(float(g[f"auc_{i}"].mean()), abs=1e-12)
    assert st["d_prime_mean"] == pytest.approx(float(np.sqrt(2.0)) * __import__("statistics").NormalDist().inv_cdf(st["mAUC"]), rel=1e-12)
    # float targets (what the trainer holds) and a bool matrix mean the same
    st2 = tagging_stats(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda().float())
    assert np.array_equal(st2["AP"], ap) and np.array_equal(st2["auc_num2"], num2)


def test_stats_degenerate_columns():
    """Columns: all positive; all negative; constant score (AP = npos / N, auc_num2 = npos * nneg); +0.0 / -0.0 only (one tie
    group: the same two identities); a single positive holding the lowest score (AP = 1 / N, AUC = 0)."""
    from src.evaluation.tagging import tagging_stats
    n = 300
    rng = np.random.default_rng(7)
    s = rng.standard_normal((n, 5)).astype(np.float32)
    t = (rng.random((n, 5)) < 0.3).astype(np.uint8)
    t[:, 0], t[:, 1] = 1, 0
    s[:, 2] = 0.625
    s[:, 3] = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0))
    assert np.signbit(s[:, 3]).any() and not np.signbit(s[:, 3]).all()
    t[:, 4] = 0
    t[17, 4] = 1
    s[17, 4] = s[:, 4].min() - 1.0
    npos, num2, ap, auc = _check_stats(s, t, "degenerate")
    assert np.isnan(ap[0]) and np.isnan(auc[0]) and np.isnan(ap[1]) and np.isnan(auc[1])
    assert (int(npos[0]), int(npos[1]), int(num2[0]), int(num2[1])) == (n, 0, 0, 0)
    for c in (2, 3):
        p = int(npos[c])
        assert 0 < p < n and int(num2[c]) == p * (n - p) and float(auc[c]) == 0.5
        assert abs(float(ap[c]) - p / n) <= n * 2.0 ** -51
    assert (int(npos[4]), int(num2[4]), float(auc[4]), float(ap[4])) == (1, 0, 0.0, 1.0 / n)
    st = tagging_stats(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda())
    assert st["classes_scored"] == 3
    assert st["mAP"] == pytest.approx(float(np.mean(ap[2:])), abs=1e-15) and st["mAUC"] == pytest.approx(float(np.mean(auc[2:])), abs=1e-15)
    assert np.isnan(st["d_prime"][0]) and st["d_prime"][2] == 0.0 and st["d_prime"][4] == -np.inf
    with pytest.raises(ValueError):
        tagging_stats(torch.from_numpy(np.where(s == s[0, 0], np.float32(np.inf), s)).cuda(), torch.from_numpy(t).cuda())


def test_stats_single_sample():
    s = np.array([[0.5, -1.0, 2.0]], dtype=np.float32)
    t = np.array([[1, 0, 1]], dtype=np.uint8)
    npos, num2, ap, auc = _check_stats(s, t, "N = 1")
    assert npos.tolist() == [1, 0, 1] and num2.tolist() == [0, 0, 0] and np.isnan(ap).all() and np.isnan(auc).all()


def test_stats_sparse_at_evaluation_size():
    """(20383, 64) at 0.5 % positives: 80 sample tiles, about 100 positives per class (one counting workgroup each; one class is
    given 700 so that three are used), scores in multiples of 1/64 so that every class has ties."""
    n, c = 20383, 64
    rng = np.random.default_rng(11)
    s = (np.round(rng.standard_normal((n, c)) * 64) / 64).astype(np.float32)
    t = (rng.random((n, c)) < 0.005).astype(np.uint8)
    t[:, 5] |= (rng.random(n) < 0.03).astype(np.uint8)
    ref = R.stats(s, t)
    assert ref["classes_scored"] == c and int(ref["npos"][5]) > 512 and int(ref["npos"].min()) > 0
    _check_stats(s, t, "(20383, 64, 0.005)", ref)


# ---- bce_rows ----------------------------------------------------------------------------------------------------------------
def _bce_case(n, c, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, c)) * 3.0).astype(np.float32)
    t = rng.random((n, c)).astype(np.float32)
    t[rng.random((n, c)) < 0.3] = 0.0
    t[rng.random((n, c)) < 0.2] = 1.0
    special = np.array([0.0, -0.0, 40.0, -40.0, 100.0, -100.0], dtype=np.float32)
    flat_x, flat_t = x.reshape(-1), t.reshape(-1)
    k = min(len(special), flat_x.size)
    if flat_x.size >= 2 * len(special):                           # every special logit once against target 0 and once against 1
        flat_x[:len(special)], flat_t[:len(special)] = special, 0.0
        flat_x[len(special):2 * len(special)], flat_t[len(special):2 * len(special)] = special, 1.0
        flat_x[2 * len(special):3 * len(special)] = special       # ... and against whatever soft target lies there
    else:
        flat_x[:k] = special[:k]
    return x, t


def _launch_bce(x, t, dtype):
    """`audiossl_bce_rows` on guarded buffers; dtype 0 / 1 = fp32 / bf16 dlogits, None = the NULL-gradient variant.
    -> (loss float, dlogits fp64 numpy or None)."""
    from src import _native as N
    n, c = x.shape
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    loss = torch.tensor([float("nan"), 77.25, -3.5], dtype=torch.float32, device="cuda")
    dl = None
    if dtype is not None:
        dl = torch.full((n * c + 8,), 5.0, dtype=torch.float32 if dtype == 0 else torch.bfloat16, device="cuda")
    N.call("bce_rows", dtype or 0, xd, td, n, c, loss, dl)
    torch.cuda.synchronize()
    assert loss[1:].tolist() == [77.25, -3.5], "loss_out is one float"
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(td.cpu().numpy(), t)
    if dl is None:
        return float(loss[0]), None
    assert dl[n * c:].float().tolist() == [5.0] * 8, "guard overwritten"
    return float(loss[0]), dl[:n * c].float().cpu().double().numpy().reshape(n, c)


@pytest.mark.parametrize("n,c", [(1, 1), (3, 527), (257, 7), (64, 200)])
def test_bce_rows_against_fp64(n, c):
    """Loss within 2^-20 relative of fp64 (terms good to a few fp32 ulp, fp64 accumulation, one final rounding); fp32 dlogits
    within 4 * 2^-24 / (N C) absolute (sigmoid to 2 * 2^-24, the subtraction, the scaling); bf16 adds 2^-8 relative; the three
    variants agree on the loss and two runs give equal bits."""
    x, t = _bce_case(n, c, 31 + n)
    want, dwant = R.bce(x, t)
    l32, d32 = _launch_bce(x, t, 0)
    l16, d16 = _launch_bce(x, t, 1)
    l0, _ = _launch_bce(x, t, None)
    l32b, d32b = _launch_bce(x, t, 0)
    bar = 4 * 2.0 ** -24 / (n * c)
    e_loss = abs(l32 - want) / abs(want)
    e32 = float(np.abs(d32 - dwant).max())
    r16 = float((np.abs(d16 - dwant) / (bar + 2.0 ** -8 * np.abs(dwant))).max())
    print(f"bce_rows ({n}, {c}): loss {l32:.7f} vs {want:.7f}, rel {e_loss:.3e} (bar {2.0 ** -20:.3e}); fp32 dlogits {e32 / bar:.3f} of the bar, "
          f"bf16 {r16:.3f} of its bar (the fp32 bar + 2^-8 relative)")
    assert np.isfinite(l32) and e_loss <= 2.0 ** -20
    assert e32 <= bar
    assert r16 <= 1.0
    assert l16 == l32 and l0 == l32 and l32b == l32 and d32b.tobytes() == d32.tobytes()


def test_bce_autograd_function():
    """backward = the kernel's dlogits times the upstream gradient; no gradient buffer without requires_grad."""
    from src.evaluation.tagging import bce_with_logits
    x, t = _bce_case(64, 200, 5)
    want, _ = R.bce(x, t)
    _, dl = _launch_bce(x, t, 0)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    loss = bce_with_logits(xd, torch.from_numpy(t).cuda())
    (loss * 2.5).backward()
    assert abs(float(loss.detach()) - want) <= 2.0 ** -20 * want
    assert torch.equal(xd.grad.cpu(), (torch.from_numpy(dl).float() * 2.5))
    with torch.no_grad():
        again = bce_with_logits(xd, torch.from_numpy(t).cuda())
    assert float(again) == float(loss.detach()) and not again.requires_grad


# ---- end to end ----------------------------------------------------------------------------------------------------------------
TONES = (("low", 440.0), ("mid", 1000.0), ("high", 2500.0))


def _tone_clips(tmp_path, n, salt):
    """n one-second clips, each a mixture of the tones of a non-empty subset of TONES (cycling through the seven subsets) plus a
    little seeded noise; the label cell names the tones present."""
    from scipy.io import wavfile
    rng = np.random.default_rng(salt)
    files, cells = [], []
    tt = np.arange(16000) / 16000.0
    for i in range(n):
        mask = (i % 7) + 1
        names = [nm for b, (nm, _) in enumerate(TONES) if mask >> b & 1]
        w = sum(0.2 * np.sin(2 * np.pi * f * tt + rng.uniform(0, 6.28)) for b, (_, f) in enumerate(TONES) if mask >> b & 1)
        w = w + 0.01 * rng.standard_normal(16000)
        p = str(tmp_path / f"tone{salt}_{i}.wav")
        wavfile.write(p, 16000, (w * 32767).astype(np.int16))
        files.append(p)
        cells.append(",".join(names))
    return files, cells


def _csvs(tmp_path, n_train=24, n_test=8):
    import pandas as pd
    ftr, ctr = _tone_clips(tmp_path, n_train, 1)
    fte, cte = _tone_clips(tmp_path, n_test, 2)
    train_csv, test_csv = str(tmp_path / "train.csv"), str(tmp_path / "test.csv")
    pd.DataFrame({"wav": ftr, "label": ctr}).to_csv(train_csv, index=False)
    pd.DataFrame({"wav": fte, "label": cte}).to_csv(test_csv, index=False)
    return train_csv, test_csv


def _command():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_tagging_hip", os.path.join(ROOT, "audio-ssl_amd", "train_tagging.py"))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)
    return tt


def _check_against_ref(stats, logits, targets):
    ref = R.stats(logits.cpu().numpy(), targets.cpu().numpy())
    n = logits.shape[0]
    assert stats["classes_scored"] == ref["classes_scored"]
    assert np.array_equal(stats["npos"], ref["npos"]) and np.array_equal(stats["auc_num2"], ref["auc_num2"])
    assert abs(stats["mAP"] - ref["mAP"]) <= n * 2.0 ** -51 and abs(stats["mAUC"] - ref["mAUC"]) <= 2.0 ** -52


def _fixed_batch_lowers_the_loss(trainer, loader, steps=20):
    from src.evaluation.tagging import bce_with_logits
    waves, target = next(iter(loader))
    trainer.model.train()
    x = trainer.eval_front(waves)                                    # no masks, no mix: the same input every step
    y = target.float().cuda()
    losses = [float(trainer.step(x, y)) for _ in range(steps)]
    with torch.no_grad():
        after = float(bce_with_logits(trainer.model(x), y))
    print(f"fixed batch: BCE {losses[0]:.4f} -> {after:.4f} after {steps} steps")
    assert np.isfinite(losses).all() and after < losses[0]


def test_train_tagging_conv_encoder_end_to_end(tmp_path):
    import yaml
    tt = _command()
    train_csv, test_csv = _csvs(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "audio-ssl_amd", "src", "downstream", "downstream_config.yaml")))
    cfg["run"].update(batch_size=8, epochs=2, duration=1, lr=2e-4)
    cfg_path = str(tmp_path / "tagging.yaml")
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    exp = tmp_path / "exp"
    torch.manual_seed(0)
    trainer, history = tt.main(tt.get_args(["--train_csv", train_csv, "--test_csv", test_csv, "--exp_dir", str(exp), "--task", "tones",
                                           "-c", cfg_path]))
    lines = [json.loads(ln) for ln in open(exp / "tones" / "tagging_stats.txt").read().splitlines()]
    assert len(lines) == 2 and [ln["epoch"] for ln in lines] == [0, 1]
    for ln, h in zip(lines, history):
        assert set(ln) == set(tt.STAT_KEYS) and ln == h
        assert ln["classes_scored"] == 3
        assert np.isfinite([ln["Train_loss"], ln["Test_Loss"], ln["mAP"], ln["mAUC"], ln["d_prime"]]).all()
        assert 0.0 <= ln["mAP"] <= 1.0 and 0.0 <= ln["mAUC"] <= 1.0
    assert lines[1]["Best_mAP"] == max(ln["mAP"] for ln in lines)
    assert trainer.class_index == {"high": 0, "low": 1, "mid": 2}
    assert [n for n, p in trainer.model.named_parameters() if p.requires_grad] == ["final.weight", "final.bias"]      # frozen
    stats, logits, targets = trainer.last_eval
    assert logits.is_cuda and tuple(logits.shape) == (8, 3) and (lines[1]["mAP"], lines[1]["mAUC"]) == (stats["mAP"], stats["mAUC"])
    _check_against_ref(stats, logits, targets)
    stats, logits, targets = trainer.eval(trainer.test_loader, epoch=9)
    assert stats["epoch"] == 9 and not trainer.model.training
    _check_against_ref(stats, logits, targets)
    _fixed_batch_lowers_the_loss(trainer, trainer.test_loader)


def test_ast_head_backward_with_a_class_count_that_is_no_multiple_of_8():
    """The closing Linear's backward zero-pads a class axis that is no multiple of 64 (`vit_engine.fc_backward`): a 3-class model
    must get the gradients of a 64-class model that shares its three rows and sees no gradient on the other 61.  Bar 1e-4
    relative L2: the two widths may run other GEMM variants and split-K orders, i.e. reorder fp32 sums of at most 512 products
    (512 * 2^-24 = 3e-5 in the worst case; a last-bit difference that flips a bf16 rounding of a gradient, one element in 2^16 at
    2^-8 each, adds 1.5e-5); a padding mistake is an error of order 1."""
    from helpers import rel_l2
    from src.encoder import ASTModel
    kw = dict(fstride=10, tstride=10, input_fdim=128, input_tdim=101, embed_dim=128, depth=2, num_heads=2)
    torch.manual_seed(11)
    small, wide = ASTModel(label_dim=3, **kw), ASTModel(label_dim=64, **kw)
    sd = {k: v for k, v in small.state_dict().items() if not k.startswith("fc.")}
    wide.load_state_dict(sd, strict=False)
    with torch.no_grad():
        wide.fc.weight[:3].copy_(small.fc.weight)
        wide.fc.bias[:3].copy_(small.fc.bias)
    small, wide = small.cuda().train(), wide.cuda().train()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(8, 1, 128, 101, generator=g).cuda()
    dout = torch.randn(8, 3, generator=g).cuda()
    out_s, out_w = small(x), wide(x)
    assert rel_l2(out_s.detach().cpu(), out_w[:, :3].detach().cpu()) <= 1e-4
    (out_s * dout).sum().backward()
    (out_w[:, :3] * dout).sum().backward()
    gs, gw = dict(small.named_parameters()), dict(wide.named_parameters())
    assert rel_l2(gs["fc.weight"].grad.cpu(), gw["fc.weight"].grad[:3].cpu()) <= 1e-4
    assert rel_l2(gs["fc.bias"].grad.cpu(), gw["fc.bias"].grad[:3].cpu()) <= 1e-4
    assert float(gs["fc.weight"].grad.abs().max()) > 0 and not bool(gw["fc.weight"].grad[3:].any())
    for n, p in gs.items():
        if not n.startswith("fc."):
            assert float(p.grad.abs().max()) > 0 and rel_l2(p.grad.cpu(), gw[n].grad.cpu()) <= 1e-4, n


MAST_CFG = {"run": {"batch_size": 8, "epochs": 1, "duration": 1, "lr": 2e-4},
            "pretrain": {"base_encoder": {"type": "MAST", "output_dim": 128, "depth": 2, "num_heads": 2, "fstride": 10, "tstride": 10,
                                          "return_all_layers": False},
                         "input": {"type": "raw_wav", "sampling_rate": 16000, "length_wave": 1.0, "n_mels": 128}},
            "tagging": {"freqm": 8, "timem": 10, "mixup": 0.6, "skip_norm": True}}


def test_train_tagging_ast_encoder_end_to_end(tmp_path, monkeypatch):
    """ASTModel (embed 128, 2 heads, depth 2, 128 mels, 101 frames): a checkpoint round trip that leaves `fc` alone, one epoch
    with mixup whose targets are `mix_labels` of the recorded draws, and the fixed-batch check."""
    import yaml
    from src.evaluation.tagging import mix_labels
    from src.upstream.ssmast.upstream_encoder import SSMAST
    tt = _command()
    train_csv, test_csv = _csvs(tmp_path)
    cfg_path = str(tmp_path / "mast.yaml")
    yaml.safe_dump(MAST_CFG, open(cfg_path, "w"))
    # a "pre-trained" checkpoint: the encoder of an SS-MAST expert with a 256-wide embedding head
    torch.manual_seed(1)
    pre = SSMAST(copy.deepcopy(MAST_CFG), emb_dim=256)
    with torch.no_grad():
        for p in pre.parameters():
            p.add_(0.01 * torch.randn_like(p))
    sd = {"encoder_q." + k: v.clone() for k, v in pre.state_dict().items()}
    sd.update({"encoder_k." + k: torch.zeros_like(v) for k, v in pre.state_dict().items()})
    sd["queue"] = torch.zeros(256, 16)
    ckpt = str(tmp_path / "ssmast.ckpt")
    torch.save({"state_dict": sd, "hyper_parameters": {}}, ckpt)

    seen = []
    real = tt.TaggingTrainer.train_targets

    def recording(self, target, device):
        out = real(self, target, device)
        seen.append((torch.as_tensor(target).clone(), tuple(t.clone() for t in self.front.last_plan), out.clone()))
        return out
    monkeypatch.setattr(tt.TaggingTrainer, "train_targets", recording)
    torch.manual_seed(2)
    import random
    random.seed(3)
    np.random.seed(4)
    exp = tmp_path / "exp"
    trainer, history = tt.main(tt.get_args(["--train_csv", train_csv, "--test_csv", test_csv, "--exp_dir", str(exp), "--task", "tones",
                                           "-c", cfg_path, "--encoder", "ASTModel", "--checkpoint", ckpt, "--freeze", "false"]))
    model = trainer.model
    assert repr(model) == "ASTModel" and tuple(model.fc.weight.shape) == (3, 128)
    assert all(p.requires_grad for p in model.parameters())
    # the round trip: a fresh model takes every tensor but fc from the checkpoint
    torch.manual_seed(5)
    fresh = SSMAST(copy.deepcopy(MAST_CFG), emb_dim=3)
    fc0 = {k: v.clone() for k, v in fresh.state_dict().items() if k.startswith("fc.")}
    tt.load_mast_encoder(fresh, ckpt)
    got = fresh.state_dict()
    assert set(got) == set(pre.state_dict())
    for k, v in pre.state_dict().items():
        if k.startswith("fc."):
            assert torch.equal(got[k], fc0[k]) and got[k].shape != v.shape
        else:
            assert torch.equal(got[k], v), k
    bad = {k: v for k, v in sd.items() if "blocks.1.mlp.fc1.weight" not in k}
    torch.save({"state_dict": bad}, str(tmp_path / "bad.ckpt"))
    with pytest.raises(RuntimeError, match="does not fit"):
        tt.load_mast_encoder(SSMAST(copy.deepcopy(MAST_CFG), emb_dim=3), str(tmp_path / "bad.ckpt"))
    # one epoch with mixup: three batches, the targets follow the recorded plan
    assert len(seen) == 3 and len(history) == 1
    mixed_rows = 0
    for y, (partner, lam, _), out in seen:
        want = mix_labels(y.float(), partner, lam)
        assert torch.equal(out.cpu(), want)
        names = [[nm for j, nm in enumerate(("high", "low", "mid")) if row[j] > 0] for row in y.tolist()]
        assert np.array_equal(out.cpu().numpy(), R.mix_rows(names, partner.tolist(), lam.tolist(), trainer.class_index))
        mixed_rows += int((partner >= 0).sum())
    assert mixed_rows > 0, "mixup 0.6 over 24 clips drew no partner"
    assert any(bool(((o > 0) & (o < 1)).any()) for _, _, o in seen), "no soft target reached the loss"
    ln = history[0]
    assert set(ln) == set(tt.STAT_KEYS) and ln["classes_scored"] == 3 and np.isfinite([ln["Train_loss"], ln["Test_Loss"], ln["mAP"]]).all()
    assert trainer.eval_front.mixup == 0.0 and trainer.eval_front.freqm == 0 and trainer.front.mixup == 0.6
    stats, logits, targets = trainer.last_eval
    _check_against_ref(stats, logits, targets)
    _fixed_batch_lowers_the_loss(trainer, trainer.test_loader)
    # --freeze: only the head trains
    frozen, _, _ = tt.build_model(tt.get_args(["--train_csv", train_csv, "--test_csv", test_csv, "--encoder", "ASTModel"]),
                                  copy.deepcopy(MAST_CFG), 3)
    assert [n for n, p in frozen.named_parameters() if p.requires_grad] == ["fc.weight", "fc.bias"]
