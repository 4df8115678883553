"""CPU: the linear-probe grid's C ABI (declared, exported, arguments refused before any launch), the tests' own restatement
against torch's cross-entropy and autograd, and the host logic of `src/evaluation/probe.py` and `evaluate_linear.py`."""
import ctypes
import importlib.util
import os

import pytest
import torch

import probe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("audiossl_probe_batch", "audiossl_probe_ce", "audiossl_probe_adamw")


def test_probe_entry_points_are_declared_and_exported():
    from src import _native as N
    protos = N.parse_header()
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in NEW:
        assert name in protos, name
        assert hasattr(lib, name), name
        assert protos[name][-1][0] == "stream"
    assert [a for a, _ in protos["audiossl_probe_batch"]] == ["X", "N", "D", "idx", "B", "mean", "rstd", "out", "ldo", "stream"]
    assert [a for a, _ in protos["audiossl_probe_ce"]] == ["logits", "ld", "label", "B", "H", "C", "Cp", "gscale", "loss_sum", "correct",
                                                           "dlogits", "stream"]
    assert [a for a, _ in protos["audiossl_probe_adamw"]] == ["W", "dW", "m", "v", "H", "seg", "lr", "wd", "lr_scale", "beta1", "beta2",
                                                              "eps", "step", "stream"]


def test_probe_arguments_are_refused_before_any_launch():
    from src import _native as N
    lib = N.lib()
    P = 256                                        # a non-null, 16-byte aligned address that is never dereferenced: every call returns first

    def batch(X=P, N_=10, D=64, idx=P, B=4, mean=P, rstd=P, out=P, ldo=72):
        return lib.audiossl_probe_batch(X, N_, D, idx, B, mean, rstd, out, ldo, None)
    assert batch(X=None) == -1 and batch(idx=None) == -1 and batch(out=None) == -1
    assert batch(mean=None) == -1 and batch(rstd=None) == -1              # nullable together only
    assert batch(D=60, ldo=68) == -1 and batch(D=4, ldo=12) == -1         # D % 8, D < 8
    assert batch(D=4104, ldo=4112) == -1                                  # D > 4096
    assert batch(ldo=71) == -1 and batch(ldo=64) == -1 and batch(ldo=70) == -1        # ldo < D + 8, ldo % 4
    assert batch(B=0) == -1 and batch(N_=0) == -1
    assert batch(X=P + 4) == -3 and batch(out=P + 8) == -3

    def ce(logits=P, ld=80, label=P, B=4, H=2, C=35, Cp=40, loss=P, correct=P, dl=P):
        return lib.audiossl_probe_ce(logits, ld, label, B, H, C, Cp, 0.25, loss, correct, dl, None)
    assert ce(logits=None) == -1 and ce(label=None) == -1 and ce(loss=None) == -1 and ce(correct=None) == -1
    assert ce(C=1, Cp=8) == -1                                            # C < 2
    assert ce(C=4097, Cp=4104, ld=8208) == -1                             # C > 4096
    assert ce(C=35, Cp=32) == -1                                          # Cp < C
    assert ce(ld=72) == -1                                                # ld < H Cp
    assert ce(ld=82) == -1                                                # ld % 4
    assert ce(H=0) == -1 and ce(B=0) == -1
    assert ce(logits=P + 4) == -3 and ce(dl=P + 4) == -3

    def adamw(W=P, dW=P, m=P, v=P, H=3, seg=128, lr=P, wd=P, step=P):
        return lib.audiossl_probe_adamw(W, dW, m, v, H, seg, lr, wd, 1.0, 0.9, 0.999, 1e-8, step, None)
    for k in ("W", "dW", "m", "v", "lr", "wd", "step"):
        assert adamw(**{k: None}) == -1, k
    assert adamw(H=0) == -1 and adamw(seg=0) == -1 and adamw(seg=126) == -1
    assert adamw(W=P + 4) == -3


@pytest.mark.parametrize("B,H,C", [(7, 3, 35), (16, 2, 130)])
def test_ce_heads_ref_equals_torch_cross_entropy_and_its_autograd(B, H, C):
    Cp = (C + 7) // 8 * 8
    g = torch.Generator().manual_seed(B + C)
    logits = torch.randn(B, H * Cp + 4, generator=g, dtype=torch.float64) * 3.0
    label = torch.randint(0, C, (B,), generator=g)
    gscale = 1.0 / B
    loss, correct, grad = R.ce_heads_ref(logits, label, H, C, Cp, gscale)
    for h in range(H):
        z = logits[:, h * Cp:h * Cp + C].clone().requires_grad_(True)
        want = torch.nn.functional.cross_entropy(z, label, reduction="sum")
        (want * gscale).backward()
        want = want.detach()
        assert abs(float(loss[h]) - float(want)) <= 1e-12 * abs(float(want))
        assert float((grad[:, h * Cp:h * Cp + C] - z.grad).abs().max()) <= 1e-15
        assert bool((grad[:, h * Cp + C:(h + 1) * Cp] == 0).all())
        assert int(correct[h]) == int((z.argmax(dim=1) == label).sum())


def test_adamw_heads_ref_keeps_a_head_with_zero_lr_and_wd():
    g = torch.Generator().manual_seed(3)
    W = torch.randn(3 * 16, generator=g, dtype=torch.float64)
    grads = [torch.randn(3 * 16, generator=g, dtype=torch.float64) for _ in range(3)]
    out, m, v = R.adamw_heads_ref(W, grads, [1e-2, 0.0, 1e-3], [0.0, 0.0, 0.1], 16)
    assert torch.equal(out[16:32], W[16:32]) and not torch.equal(out[:16], W[:16]) and not torch.equal(out[32:], W[32:])
    assert bool((v[16:32] > 0).all())


def test_head_index_order_of_the_grid():
    from src.evaluation.probe import head_index
    lrs, wds = [1e-3, 1e-2], [0.0, 1e-4, 1e-2]
    order = [(lr, wd) for lr in lrs for wd in wds]
    for i, lr in enumerate(lrs):
        for j, wd in enumerate(wds):
            assert order[head_index(i, j, len(wds))] == (lr, wd)
    assert [head_index(i, j, 3) for i in range(2) for j in range(3)] == list(range(6))


def test_holdout_is_stratified_deterministic_and_disjoint():
    from src.evaluation import stratified_holdout
    g = torch.Generator().manual_seed(0)
    counts = {0: 50, 1: 23, 2: 4, 3: 1, 4: 2, 7: 96}                      # class 3 has a single row; ids need not be dense
    y = torch.cat([torch.full((n,), c) for c, n in counts.items()])
    y = y[torch.randperm(y.numel(), generator=g)]
    keep, held = stratified_holdout(y, 0.1, seed=0)
    assert sorted(torch.cat([keep, held]).tolist()) == list(range(y.numel()))          # a partition: disjoint and complete
    want = {0: 5, 1: 2, 2: 1, 3: 0, 4: 1, 7: 10}                                       # max(1, round(0.1 n)); the single row stays
    for c, k in want.items():
        assert int((y[held] == c).sum()) == k, c
        assert int((y[keep] == c).sum()) == counts[c] - k
    keep2, held2 = stratified_holdout(y, 0.1, seed=0)
    assert torch.equal(held, held2) and torch.equal(keep, keep2)
    _, held3 = stratified_holdout(y, 0.1, seed=1)
    assert not torch.equal(held, held3) and held3.numel() == held.numel()
    with pytest.raises(ValueError):
        stratified_holdout(y, 1.0, seed=0)


def test_select_prefers_top1_then_loss_then_index():
    from src.evaluation import select_head
    r = lambda top1, loss: dict(lr=0.0, wd=0.0, top1=top1, loss=loss)     # noqa: E731
    assert select_head([r(0.5, 1.0), r(0.7, 2.0), r(0.6, 0.1)]) == 1
    assert select_head([r(0.7, 1.0), r(0.7, 0.5), r(0.6, 0.1)]) == 1
    assert select_head([r(0.7, 0.5), r(0.7, 0.5), r(0.7, 0.5)]) == 0
    assert select_head([r(0.1, 0.5), r(0.7, 0.5), r(0.7, 0.5)]) == 1
    with pytest.raises(ValueError):
        select_head([])


def test_folding_the_standardisation_reproduces_the_logits():
    from src.evaluation import fold_standardisation
    g = torch.Generator().manual_seed(5)
    x = torch.randn(40, 24, generator=g, dtype=torch.float64) * 3.0 + 1.5
    mean, std = x.mean(0), x.std(0, unbiased=False)
    rstd = 1.0 / (std + 1e-6)
    w, b = torch.randn(7, 24, generator=g, dtype=torch.float64), torch.randn(7, generator=g, dtype=torch.float64)
    want = ((x - mean) * rstd) @ w.T + b
    w2, b2 = fold_standardisation(w, b, mean, rstd)
    assert w2.dtype == torch.float64
    assert float((x @ w2.T + b2 - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_cosine_scale_and_permutations():
    from src.evaluation import cosine_scale, epoch_permutations
    assert cosine_scale(0, 10) == 1.0 and 0.0 < cosine_scale(9, 10) < 0.03 and cosine_scale(5, 10) == pytest.approx(0.5)
    assert [cosine_scale(k, 7) for k in range(7)] == [R.cosine_scale(k, 7) for k in range(7)]
    a = epoch_permutations(11, 3, torch.Generator().manual_seed(4))
    g = torch.Generator().manual_seed(4)
    assert all(torch.equal(p, torch.randperm(11, generator=g)) for p in a)


def test_grid_refuses_cpu_tensors_and_bad_shapes():
    from src.evaluation import LinearProbeGrid, feature_stats
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        feature_stats(torch.zeros(4, 8))
    with pytest.raises(ValueError):
        LinearProbeGrid(12, 3, [1e-3], [0.0], device="cpu")               # D % 8
    with pytest.raises(ValueError):
        LinearProbeGrid(16, 1, [1e-3], [0.0], device="cpu")               # C < 2
    with pytest.raises(ValueError):
        LinearProbeGrid(16, 3, [], [0.0], device="cpu")
    grid = LinearProbeGrid(16, 3, [1e-3, 1e-2], [0.0, 0.1, 0.2], device="cpu")          # buffers only: nothing is launched
    assert grid.H == 6 and grid.hparams[4] == (1e-2, 0.1) and grid.W.shape == (6 * 8, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid.step(torch.zeros(4, 16), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid.evaluate(torch.zeros(4, 16), torch.zeros(4, dtype=torch.int64))


def test_evaluate_linear_parses_its_arguments():
    spec = importlib.util.spec_from_file_location("evaluate_linear_args", os.path.join(ROOT, "audio-ssl_amd", "evaluate_linear.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    base = ["--checkpoint", "c", "--train_csv", "a", "--test_csv", "b"]
    a = ev.get_args(base)
    assert a.lrs == [1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2] and a.wds == [0.0, 1e-4, 1e-2]
    assert (a.epochs, a.probe_batch, a.holdout, a.seed, a.valid_csv, a.window, a.layer, a.max_duration, a.batch_size) == \
        (100, 1024, 0.1, 0, None, "center", "backbone", 30.0, 64)
    assert a.embeddings is None and a.save_head is None and a.dump_embeddings is None
    a = ev.get_args(base + ["--lrs", "1e-3,0.5", "--wds", "0", "--epochs", "2", "--probe_batch", "8", "--valid_csv", "v", "--holdout", "0.25",
                            "--seed", "3", "--save_head", "h.pt", "--window", "whole"])
    assert (a.lrs, a.wds, a.epochs, a.probe_batch, a.valid_csv, a.holdout, a.seed, a.save_head, a.window) == \
        ([1e-3, 0.5], [0.0], 2, 8, "v", 0.25, 3, "h.pt", "whole")
    a = ev.get_args(["--embeddings", "dir"])                              # no checkpoint or CSVs needed
    assert a.embeddings == "dir" and a.checkpoint is None
    for bad in (["--train_csv", "a"], base + ["--lrs", "x"], base + ["--lrs", "-1"], base + ["--epochs", "0"], base + ["--holdout", "1.5"]):
        with pytest.raises(SystemExit):
            ev.get_args(bad)
