"""GPU: the conv blocks with the 2x2 max-pool taken in the convolution's epilogue (conv3x3_pool_fwd) and BatchNorm + ReLU on the
pooled map (bn_relu_pooled_fwd / bn_relu_pooled_train_fwd), held to EXACT equality with the path they replace:

  conv3x3_pool_fwd      Y (where kept) and the fp64 sums bit for bit those of conv3x3_fwd; Praw bit for bit the per-channel window
                        maximum (gamma >= 0) / minimum (gamma < 0) of that Y, taken with torch.
                        The sums: the pooled forms keep the accumulation order (same per-lane order over the same values, same
                        per-workgroup fold, same replica per workgroup), and a replica adds at most 32 doubles that were fp32
                        values - exact in fp64, so the order of the atomics does not show.  The test asserts BITWISE equality.
  bn_relu_pooled_*_fwd  P, scale, shift, mean, rstd and the running buffers bit for bit those of bn_relu_pool_(train_)fwd on the
                        whole of Y: BN + ReLU is monotone with the sign of gamma, so it commutes with the window extremum.
  engine                encoder_forward with the new path against AUDIOSSL_CONV_POOL=0 (the module switch is flipped the way the
                        other engine switches are, by monkeypatch): hard limit rel-L2 4e-3 (the bf16 bound of test_gpu_bn_chain.py),
                        the number of differing elements is printed (zero is expected); parameter gradients rel-L2 1e-4 (that
                        file's bound for fp32 outputs).
Outputs documented as written are pre-filled with NaN."""
import functools

import pytest
import torch

from oracle import fill
from helpers import rel_l2, views

pytestmark = pytest.mark.gpu

BF16_TOL = 4.0e-3            # test_gpu_bn_chain.py: one bf16 output rounding on top of 1e-4
F32_TOL = 1e-4
EPS = 1e-5
REP = 8


@pytest.fixture(scope="module")
def N():
    from src import _native
    _native.lib()
    assert torch.cuda.is_available()
    return _native


def nan_bf16(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else (torch.int32 if t.dtype == torch.float32 else torch.int64))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def mixed_gamma(seed):
    g = torch.Generator().manual_seed(seed)
    gamma = torch.rand(64, generator=g) + 0.5
    gamma[torch.randperm(64, generator=g)[:24]] *= -1.0            # 24 channels pool by the minimum
    gamma[5], gamma[6], gamma[37], gamma[38] = 0.0, -0.0, -0.0, 0.0
    return gamma


def window_extrema(Y, gamma):
    """Y [N][Ti][Fi][64] bf16 -> [N][Ti/2][Fi/2][64] bf16: per channel the window's max where gamma >= 0, its min where gamma < 0"""
    n, Ti, Fi, c = Y.shape
    w = Y.float()[:, :Ti // 2 * 2].reshape(n, Ti // 2, 2, Fi // 2, 2, c)
    hi, lo = w.amax((2, 4)), w.amin((2, 4))
    return torch.where((gamma >= 0).to(Y.device), hi, lo).bfloat16()


# ======================================================================================== 1. the convolution
CONV_SHAPES = [(3, 6, 32),        # 18 rows: a partial last tile, image borders inside a tile
               (3, 10, 16),       # the same for the 16-wide form
               (64, 50, 32),      # 400 tiles on at most 256 persistent workgroups: double-buffered second tile, block 2's own Ti
               (172, 24, 16)]     # 258 tiles: the 16-wide form past one round


@functools.lru_cache(maxsize=None)
def conv_case(shape):
    """inputs and what conv3x3_fwd makes of them (stats, 8 replicas), computed once per shape and left unchanged"""
    from src import _native as N
    Nimg, Ti, Fi = shape
    x = torch.from_numpy(fill.normalish((Nimg, Ti, Fi, 64), 7100 + Ti + Fi)).cuda().bfloat16()
    w = torch.from_numpy(fill.uniform((64, 64, 3, 3), 7200 + Ti, -0.05, 0.05)).cuda()
    b = torch.from_numpy(fill.uniform((64,), 7300 + Ti)).cuda()
    Wf, Wd = torch.empty(64, 576, device="cuda", dtype=torch.bfloat16), torch.empty(64, 576, device="cuda", dtype=torch.bfloat16)
    N.call("pack_conv_w", 1, w, Wf, Wd)
    gamma = mixed_gamma(7400 + Ti).cuda()
    Y = nan_bf16(Nimg, Ti, Fi, 64)
    sq = torch.full((REP, 2, 64), float("nan"), dtype=torch.float64, device="cuda")
    N.call("conv3x3_fwd", x, Wf, b, Y, 0, sq[0, 0], sq[0, 1], REP, Nimg, Ti, Fi)
    torch.cuda.synchronize()
    assert torch.isfinite(Y.float()).all() and torch.isfinite(sq).all()
    return x, Wf, b, gamma, Y, sq


@pytest.mark.parametrize("keep_y", [True, False])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_conv_pool_fwd_equals_conv_fwd_and_torch_window_extrema(N, shape, keep_y):
    Nimg, Ti, Fi = shape
    x, Wf, b, gamma, Y0, sq0 = conv_case(shape)
    npool = Nimg * (Ti // 2) * (Fi // 2) * 64
    guard = 4096                                                     # elements before and behind every output
    pbuf = nan_bf16(npool + 2 * guard)
    sbuf = torch.full((REP * 128 + 2 * 64,), float("nan"), dtype=torch.float64, device="cuda")
    Praw = pbuf[guard:guard + npool].view(Nimg, Ti // 2, Fi // 2, 64)
    sq = sbuf[64:64 + REP * 128].view(REP, 2, 64)
    ybuf = nan_bf16(Y0.numel() + 2 * guard)
    Y = ybuf[guard:guard + Y0.numel()].view(Y0.shape) if keep_y else None
    N.call("conv3x3_pool_fwd", x, Wf, b, gamma, Y, Praw, sq[0, 0], sq[0, 1], REP, Nimg, Ti, Fi)
    torch.cuda.synchronize()
    if keep_y:
        assert same_bits(Y, Y0)
        assert torch.isnan(ybuf[:guard].float()).all() and torch.isnan(ybuf[-guard:].float()).all()
    else:
        assert torch.isnan(ybuf.float()).all()                       # a buffer the call was not given stays as it was
    want = window_extrema(Y0, gamma)
    ndiff = int((bits(Praw) != bits(want)).sum())
    print(f"{shape} keep_y={keep_y}: Praw elements that differ {ndiff} of {npool}; "
          f"sums max |diff| {float((sq - sq0).abs().max()):.3e}")
    assert ndiff == 0
    assert same_bits(sq, sq0)                                        # the accumulation order was kept: bitwise
    assert torch.isnan(pbuf[:guard].float()).all() and torch.isnan(pbuf[-guard:].float()).all()
    assert torch.isnan(sbuf[:64]).all() and torch.isnan(sbuf[-64:]).all()
    # the minimum really differs from the maximum on the channels that take it
    neg = (gamma < 0).cpu()
    hi = window_extrema(Y0, torch.ones(64).cuda()).float().cpu()
    assert float((hi - Praw.float().cpu())[..., neg].abs().max()) > 0.0


# ======================================================================================== 2. BatchNorm + ReLU on the pooled map
BN_SHAPES = [(3, 6, 32), (3, 10, 16)]


def bn_case(shape):
    Nimg, Ti, Fi = shape
    g = torch.Generator().manual_seed(8000 + Ti + Fi)
    Y = (torch.randn(Nimg, Ti, Fi, 64, generator=g) * 1.5 + 0.25).bfloat16().cuda()
    gamma = mixed_gamma(8100 + Ti).cuda()
    beta = (torch.randn(64, generator=g) * 0.3).cuda()
    Yd = Y.double().reshape(-1, 64)
    sq = torch.zeros(REP, 2, 64, dtype=torch.float64, device="cuda")
    for r in range(REP):                                             # the sums spread over the replicas, as the convolution leaves them
        part = Yd[r::REP]
        sq[r, 0], sq[r, 1] = part.sum(0), (part * part).sum(0)
    return Y, gamma, beta, sq, window_extrema(Y, gamma)


def run_old_train(N, Y, sq, gamma, beta, running, shape):
    Nimg, Ti, Fi = shape
    P = nan_bf16(Nimg, Ti // 2, Fi // 2, 64)
    st = torch.full((4, 64), float("nan"), device="cuda")
    rm, rv = (torch.linspace(-1, 1, 64).cuda(), torch.linspace(0.5, 2, 64).cuda()) if running else (None, None)
    N.call("bn_relu_pool_train_fwd", 1, 1, Y, sq[0, 0], sq[0, 1], REP, float(Nimg * Ti * Fi), gamma, beta, rm, rv, 0.1, EPS, P, st[0],
           st[1], st[2], st[3], Nimg, Ti, Fi)
    return P, st, rm, rv


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("running", [True, False])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=str)
def test_bn_relu_pooled_train_fwd_equals_bn_relu_pool_train_fwd(N, shape, running, in_place):
    Nimg, Ti, Fi = shape
    Y, gamma, beta, sq, Praw = bn_case(shape)
    P0, st0, rm0, rv0 = run_old_train(N, Y, sq, gamma, beta, running, shape)
    src = Praw.clone()
    P = src if in_place else nan_bf16(*Praw.shape)
    st = torch.full((4, 64), float("nan"), device="cuda")
    rm, rv = (torch.linspace(-1, 1, 64).cuda(), torch.linspace(0.5, 2, 64).cuda()) if running else (None, None)
    N.call("bn_relu_pooled_train_fwd", 1, src, sq[0, 0], sq[0, 1], REP, float(Nimg * Ti * Fi), gamma, beta, rm, rv, 0.1, EPS, P, st[0],
           st[1], st[2], st[3], Nimg, Ti // 2, Fi // 2)
    torch.cuda.synchronize()
    assert torch.isfinite(P0.float()).all() and float(P0.float().max()) > 0.0 and float((P0.float() == 0).float().mean()) > 0.05
    print(f"{shape}: P elements that differ {int((bits(P) != bits(P0)).sum())}")
    assert same_bits(P, P0)
    for name, a, b in zip(("scale", "shift", "mean", "rstd"), st, st0):
        assert torch.isfinite(b).all() and same_bits(a, b), name
    if running:
        assert same_bits(rm, rm0) and same_bits(rv, rv0)
        assert not torch.equal(rm0, torch.linspace(-1, 1, 64).cuda())
    if not in_place:
        assert same_bits(src, Praw)                                  # the input is only read


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=str)
def test_bn_relu_pooled_fwd_equals_bn_relu_pool_fwd(N, shape, in_place):
    Nimg, Ti, Fi = shape
    Y, gamma, beta, sq, Praw = bn_case(shape)
    _, st0, _, _ = run_old_train(N, Y, sq, gamma, beta, False, shape)          # a realistic scale / shift, signs from gamma
    scale, shift = st0[0].clone(), st0[1].clone()
    P0 = nan_bf16(Nimg, Ti // 2, Fi // 2, 64)
    N.call("bn_relu_pool_fwd", 1, 1, Y, scale, shift, P0, Nimg, Ti, Fi)
    src = Praw.clone()
    P = src if in_place else nan_bf16(*Praw.shape)
    N.call("bn_relu_pooled_fwd", 1, src, scale, shift, P, Nimg, Ti // 2, Fi // 2)
    torch.cuda.synchronize()
    assert torch.isfinite(P0.float()).all() and float(P0.float().max()) > 0.0
    print(f"{shape}: P elements that differ {int((bits(P) != bits(P0)).sum())}")
    assert same_bits(P, P0)


# ======================================================================================== 4. the engine
RUNNING = ["features_2.1.running_mean", "features_2.1.running_var", "features_3.1.running_mean", "features_3.1.running_var"]


@functools.lru_cache(maxsize=None)
def encoder_params():
    from src.encoder import AudioNTT2020Task6
    enc = AudioNTT2020Task6(64, 2048, True)
    fill.fill_state_dict_(enc, seed=1)
    enc = enc.cuda().train()
    P = {k: v.detach().clone() for k, v in enc.param_dict().items()}
    g = torch.Generator().manual_seed(9)
    for blk in ("features_2.1", "features_3.1"):                     # some channels pool by the minimum
        P[blk + ".weight"][torch.randperm(64, generator=g)[:16].cuda()] *= -1.0
    return P, [n for n in enc.engine_param_names()]


def run_encoder(monkeypatch, pool, T, need_bwd):
    from src import _native as N
    from src import engine as E
    monkeypatch.setattr(E, "_CONV_POOL", pool)
    E.set_high_precision(False)
    P0, names = encoder_params()
    P = {k: v.clone() for k, v in P0.items()}
    x = views(4, T, 7000 + T).cuda()
    x1, x2, x3, H2, c = E.encoder_forward(P, x, N.BF16, train=True, update_running=True, need_bwd=need_bwd)
    out = {"x1": x1, "x2": x2, "x3": x3, "H2": H2, **{k: P[k] for k in RUNNING}}
    G = None
    if need_bwd:
        G = {n: torch.zeros_like(P[n], dtype=torch.float32) for n in names}
        g = torch.Generator().manual_seed(70 + T)
        dH2 = torch.randn(c.M, c.d, generator=g).cuda().bfloat16()
        dx = [torch.randn(tuple(v.shape), generator=g).cuda() for v in (x1, x2, x3)]
        E.encoder_backward(c, G, dH2=dH2, dx1=dx[0], dx2=dx[1], dx3=dx[2])
    torch.cuda.synchronize()
    return out, c, G


@pytest.mark.parametrize("need_bwd", [False, True])
@pytest.mark.parametrize("T", [96, 101])        # 96: both blocks take the new path; 101: block 2 does, block 3 (Ti = 25) falls back
def test_encoder_with_pooled_conv_equals_switch_off(monkeypatch, T, need_bwd):
    old, c_old, G_old = run_encoder(monkeypatch, False, T, need_bwd)
    new, c, G = run_encoder(monkeypatch, True, T, need_bwd)
    assert c_old.Y2 is not None and c_old.Y3 is not None
    for k in old:
        a, b = new[k].float().cpu(), old[k].float().cpu()
        err = rel_l2(a, b)
        print(f"T={T} need_bwd={need_bwd} {k}: differing elements {int((a != b).sum())} of {a.numel()}, rel-L2 {err:.3e}")
        assert torch.isfinite(a).all() and float(b.abs().max()) > 0.0
        assert err < BF16_TOL, k
    if not need_bwd:
        assert c.Y2 is None
        assert (c.Y3 is None) == (T == 96)                           # Ti = 25 keeps the old launches, which store Y
        return
    assert c.Y2 is not None and c.Y3 is not None
    for n in G:
        a, b = G[n].cpu(), G_old[n].cpu()
        if n.startswith("features") and n.endswith(".0.bias"):      # conv bias under train-mode BatchNorm: zero up to rounding noise
            scale = max(float(G_old[n.replace(".0.bias", ".1.bias")].abs().max()), 1.0)
            assert float((a - b).abs().max()) <= 1e-3 * scale, n
            continue
        err = rel_l2(a, b)
        print(f"T={T} grad {n}: rel-L2 {err:.3e}")
        assert float(b.abs().max()) > 0.0 and err < F32_TOL, n
