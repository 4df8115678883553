"""GPU: batch statistics of the stem (csrc/conv1.hip) - the tap-moments kernel that takes up to two views per launch and leaves
replica sets in per-view moment slots, and the MFMA stem forward that finalizes BatchNorm in its own prologue.

A moment slot is AUDIOSSL_CONV1_MOM_SLOT = 17 * 54 doubles: [0:54] the totals (written by whoever finalizes), then 16 replica sets of
54 that the kernel adds into; the consumer folds the replicas, and so do these tests.
Tolerances: moments against the float64 `unfold` reference rtol 2e-5, atol 1e-3 (those of test_conv1_tap_moments); the fused forward
against conv1_finalize + conv1_fwd bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import fill
from helpers import rel_l2, views

pytestmark = pytest.mark.gpu

SLOT, NMOM, REPL = 17 * 54, 54, 16
SHAPES = [(1, 2, 2), (3, 8, 2), (2, 64, 129), (5, 40, 300), (2, 120, 128), (7, 62, 101), (64, 64, 101)]


@pytest.fixture(scope="module")
def N():
    from src import _native
    _native.lib()
    assert torch.cuda.is_available()
    return _native


@functools.lru_cache(maxsize=None)
def _view(shape, salt):
    """(image batch [N][F][T] fp32 on the CPU, its 54 tap moments in float64) - computed once per (shape, salt), never modified."""
    import torch.nn.functional as Fnn
    Nimg, F_, T = shape
    x = torch.from_numpy(fill.normalish((Nimg, 1, F_, T), salt)).double()
    taps = Fnn.unfold(x, 3, padding=1)                               # [N, 9, F*T], tap order kh*3+kw
    s1 = taps.sum((0, 2))
    s2 = torch.einsum("nap,nbp->ab", taps, taps)
    want = torch.cat([s1, torch.stack([s2[a, b] for a in range(9) for b in range(a, 9)])])
    return x[:, 0].float().contiguous(), want.numpy()


def _fold(slot):
    """What the consumer of a slot does: the 16 replica sets added in replica order."""
    rep = slot[NMOM:].view(REPL, NMOM).cpu()
    tot = torch.zeros(NMOM, dtype=torch.float64)
    for r in range(REPL):
        tot += rep[r]
    return tot.numpy()


def _check(slot, want):
    got = _fold(slot)
    print("max |err| / (atol + rtol |want|):", float(np.max(np.abs(got - want) / (1e-3 + 2e-5 * np.abs(want)))))
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-3)


@pytest.mark.parametrize("shape", SHAPES)
def test_moments_one_view(N, shape):
    """Single-view call: slot 0 filled, and the second slot of the buffer (img_b = NULL) left exactly as it was."""
    Nimg, F_, T = shape
    a, want = _view(shape, 7 + T)
    slots = torch.full((2, SLOT), float("nan"), dtype=torch.float64, device="cuda")
    N.call("conv1_moments_pair", a.cuda(), None, Nimg, F_, T, slots)
    torch.cuda.synchronize()
    _check(slots[0], want)
    assert float(slots[0, :NMOM].abs().max()) == 0.0                  # the totals are the finalizer's to write
    assert bool(torch.isnan(slots[1]).all())
    # the existing entry runs on the same kernel: 16 x 54 doubles, totals in [0:54]
    mom = torch.full((REPL * NMOM,), float("nan"), dtype=torch.float64, device="cuda")
    N.call("conv1_moments", a.cuda(), Nimg, F_, T, mom)
    torch.cuda.synchronize()
    np.testing.assert_allclose(mom[:NMOM].cpu().numpy(), want, rtol=2e-5, atol=1e-3)


@pytest.mark.parametrize("shape", SHAPES)
def test_moments_two_views(N, shape):
    """Pair call on two DIFFERENT views: each slot holds its own view's moments."""
    Nimg, F_, T = shape
    a, want_a = _view(shape, 7 + T)
    b, want_b = _view(shape, 1007 + T)
    assert not np.allclose(want_a, want_b, rtol=1e-3, atol=0)
    slots = torch.full((2, SLOT), float("nan"), dtype=torch.float64, device="cuda")
    N.call("conv1_moments_pair", a.cuda(), b.cuda(), Nimg, F_, T, slots)
    torch.cuda.synchronize()
    _check(slots[0], want_a)
    _check(slots[1], want_b)


@pytest.mark.parametrize("prezeroed", [False, True])
def test_moments_reuse_of_caller_buffers(N, prezeroed):
    """Three calls in a row on the same caller buffers (outside the arena): nothing survives from one call to the next.  Without
    `set_prezeroed` the entry clears the slots itself (NaN in them before the first call); with it the caller does."""
    shape = (7, 62, 101)
    Nimg, F_, T = shape
    a, want_a = _view(shape, 7 + T)
    b, want_b = _view(shape, 1007 + T)
    ad, bd = a.cuda(), b.cuda()
    slots = torch.full((2, SLOT), float("nan"), dtype=torch.float64, device="cuda")
    try:
        if prezeroed:
            N.call_host("set_prezeroed", 1)
        for _ in range(3):
            if prezeroed:
                slots.zero_()
            N.call("conv1_moments_pair", ad, bd, Nimg, F_, T, slots)
            torch.cuda.synchronize()
            _check(slots[0], want_a)
            _check(slots[1], want_b)
    finally:
        N.call_host("set_prezeroed", 0)


@pytest.mark.parametrize("running", [True, False])
@pytest.mark.parametrize("with_xl", [True, False])
@pytest.mark.parametrize("shape", [(3, 64, 101), (3, 64, 96), (2, 40, 10)])
def test_fused_forward_equals_finalize_plus_forward(N, shape, with_xl, running):
    """conv1_fwd_train against conv1_finalize + conv1_fwd(dtype 1) on the same totals: every output bit for bit.  The slot handed to
    the fused launch carries the totals as replica 0 and zeros in the other fifteen, so its fold reproduces them exactly."""
    Nimg, F_, T = shape
    a, _ = _view(shape, 7 + T)
    img = a.cuda()
    w = torch.from_numpy(fill.uniform((64, 9), 31, -0.4, 0.4)).cuda()
    bias, beta = (torch.from_numpy(fill.uniform((64,), 32 + i)).cuda() for i in range(2))
    gamma = torch.from_numpy(fill.uniform((64,), 34, 0.5, 1.5)).cuda()
    mom = torch.empty(REPL * NMOM, dtype=torch.float64, device="cuda")
    N.call("conv1_moments", img, Nimg, F_, T, mom)
    totals = mom[:NMOM].clone()
    count = float(Nimg * F_ * T)

    def outputs():
        st = [torch.zeros(64, device="cuda") for _ in range(4)]
        rm = torch.from_numpy(fill.uniform((64,), 35)).cuda() if running else None
        rv = torch.from_numpy(fill.uniform((64,), 36, 0.5, 1.5)).cuda() if running else None
        P = torch.zeros(Nimg, T // 2, F_ // 2, 64, device="cuda", dtype=torch.bfloat16)
        xl = torch.zeros(4, Nimg, (F_ // 2) * 64, device="cuda") if with_xl else None
        return st, rm, rv, P, xl

    st0, rm0, rv0, P0, xl0 = outputs()
    tot0 = totals.clone()
    N.call("conv1_finalize", tot0, w, bias, gamma, beta, rm0, rv0, 0.1, 1e-5, count, *st0)
    N.call("conv1_fwd", 1, img, Nimg, F_, T, w, bias, st0[0], st0[1], P0, xl0)
    st1, rm1, rv1, P1, xl1 = outputs()
    slot = torch.zeros(SLOT, dtype=torch.float64, device="cuda")
    slot[NMOM:2 * NMOM] = totals
    N.call("conv1_fwd_train", img, Nimg, F_, T, slot, count, w, bias, gamma, beta, rm1, rv1, 0.1, 1e-5, *st1, P1, xl1)
    torch.cuda.synchronize()
    for name, x0, x1 in zip(("scale", "shift", "mean", "rstd"), st0, st1):
        assert torch.isfinite(x0).all() and torch.equal(x0, x1), name
    assert float(st0[3].min()) > 0.0
    if running:
        assert torch.equal(rm0, rm1) and torch.equal(rv0, rv1)
    assert float(P0.float().abs().max()) > 0.0 and torch.equal(P0, P1)
    if with_xl:
        assert torch.equal(xl0, xl1)
    assert torch.equal(slot[:NMOM], totals) and torch.equal(tot0, totals)


@pytest.mark.parametrize("T", [96, 101])
def test_encoder_forward_with_precomputed_pair_moments(N, T):
    """engine.encoder_forward handed its row of a two-view moments launch against the same call taking its own moments.  The pair
    launch and the single-view launch split the work over different grids (and both add through atomics), so the totals may
    differ in their last bits: the pooled stem output is compared within bf16 rounding (rel-L2 < 1e-3), the totals at the tolerance
    of the moments themselves."""
    from src import engine as E
    from src.encoder import AudioNTT2020Task6
    enc = AudioNTT2020Task6(64, 2048, True)
    fill.fill_state_dict_(enc, seed=1)
    enc = enc.cuda().train()
    E.set_high_precision(False)
    assert E.stem_fused(N.BF16, True)
    P = enc.param_dict()
    xq, xk = views(4, T, 5000 + T).cuda(), views(4, T, 6000 + T).cuda()
    moms = E.stem_moments_pair(xq, xk)
    assert moms.shape == (2, SLOT)
    for x, row in ((xq, moms[0]), (xk, moms[1])):
        own = E.encoder_forward(P, x, N.BF16, train=True, update_running=False)
        pre = E.encoder_forward(P, x, N.BF16, train=True, update_running=False, stem_moments=row)
        torch.cuda.synchronize()
        c0, c1 = own[4], pre[4]
        assert c1.mom1.data_ptr() == row.data_ptr()
        np.testing.assert_allclose(c1.mom1[:NMOM].cpu().numpy(), c0.mom1[:NMOM].cpu().numpy(), rtol=2e-5, atol=1e-3)
        assert float(c0.mom1[:NMOM].abs().max()) > 0.0
        assert rel_l2(c1.P1.float().cpu(), c0.P1.float().cpu()) < 1e-3
        for got, want in zip(pre[:4], own[:4]):
            assert rel_l2(got.float().cpu(), want.float().cpu()) < 2e-2          # ACT_TOL of the bf16 path (test_gpu_model.py)


def test_step_with_pair_launch_matches_per_encoder_moments(N, monkeypatch):
    """The DeLoRes-M step with both views' stem moments taken by one launch ahead of the key stream (AUDIOSSL_STEM_PAIR=1) against the
    default, where each encoder takes its own: same loss and query-encoder gradient within the bf16 path's tolerances (LOSS_TOL 2e-2 of
    test_gpu_model.py; gradients 5e-2 rel-L2 - the two differ by the last bits of the moment totals only)."""
    import copy
    from conftest import CFG_M
    from helpers import closed_queue, drop_mask
    from src.encoder import AudioNTT2020Task6
    from src.upstream.delores_m import upstream_expert as UE
    B, T, K = 8, 101, 1024            # the shapes of test_delores_m_steps_vs_reference_golden (the grouped heads need 2 B >= 16 rows)
    cfg = copy.deepcopy(CFG_M)
    cfg["run"]["precision"] = "bf16"
    out = []
    for pair in (False, True):
        monkeypatch.setattr(UE, "_STEM_PAIR", pair)
        em = UE.Upstream_Expert(cfg, base_encoder=AudioNTT2020Task6, num_negatives=K)
        fill.fill_state_dict_(em, seed=4)
        for pq, pk in zip(em.encoder_q.parameters(), em.encoder_k.parameters()):
            pk.data.copy_(pq.data)
        em.queue.copy_(closed_queue(128, K))
        em = em.cuda().train()
        em.encoder_q.encoder.dropout_masks.queue = [drop_mask((B, 12, 2048), 3)]
        em.encoder_k.encoder.dropout_masks.queue = [drop_mask((B, 12, 2048), 4)]
        loss = em.training_step((views(B, T, 1).cuda(), views(B, T, 2).cuda()), 0)
        loss.backward()
        torch.cuda.synchronize()
        g = dict(em.named_parameters())
        out.append((float(loss), g["encoder_q.encoder.features_1.0.weight"].grad.float().cpu(),
                    g["encoder_q.encoder.fc.3.weight"].grad.float().cpu(), em.encoder_k.encoder.features_1[1].running_mean.cpu()))
    (l0, gw0, gf0, rm0), (l1, gw1, gf1, rm1) = out
    print("loss", l0, l1, "stem dW rel-L2", rel_l2(gw1, gw0), "fc dW rel-L2", rel_l2(gf1, gf0))
    assert np.isfinite(l0) and abs(l1 - l0) <= 2e-2 * abs(l0)
    assert rel_l2(gw1, gw0) < 5e-2 and rel_l2(gf1, gf0) < 5e-2
    np.testing.assert_allclose(rm1.numpy(), rm0.numpy(), rtol=1e-4, atol=1e-6)   # the key encoder's stem statistics: from slot 1
