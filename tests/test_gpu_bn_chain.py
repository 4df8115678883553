"""GPU: the BatchNorm chain of the conv encoder and the projector, kernel by kernel through the C ABI, and the two halves
("sums" and "apply / finalize") of every SyncBatchNorm kernel on ONE GPU: a batch is split in two, the sums half runs on each
part, the test adds the sums as the all-reduce would, the apply half runs on each part with the global count, and the
concatenated result is compared with an fp64 reference of the whole batch.

The reference sees what the kernel sees: fp64 torch autograd on the inputs as stored (bf16 tensors are rounded first, then cast
to fp64), so only the output rounding and the fp32 accumulation separate the two:
  fp32 outputs              rel-L2 <= 1e-4   (the project's fp32 bound, TOL[0] of test_gpu_kernels.py)
  bf16 outputs              rel-L2 <= 4.0e-3 (one output rounding, 2^-8 per element, on top of 1e-4)
  fp64 / fp32 sums          rel-L2 <= 1e-4   (fp64 sums and the statistics derived from fp64 sums: 1e-6, element-wise)
  integer / arg outputs     bit-exact
Max-pool routing and ReLU gates flip when fp32 and fp64 disagree about a comparison, so the inputs leave no near-ties: the conv
outputs of the pooled blocks lie on a grid of 1/32 (exact in bf16: window ties are exact ties and go to the first maximum in
(f, t) order on both sides, every other gap is at least |scale| / 32), and every test asserts the margins of its own reference
before it compares (the assertion guards the input, it excludes nothing).
Outputs documented as written are pre-filled with NaN, accumulated ones (dgamma, dbeta, dW) with non-zero values."""
import functools

import numpy as np
import pytest
import torch

from oracle import fill
from helpers import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    from src import _native
    _native.lib()
    assert torch.cuda.is_available()
    return _native


def dev(x):
    return torch.as_tensor(x).cuda().contiguous()


F32_TOL = 1e-4
BF16_TOL = 4.0e-3            # 2^-8 + 1e-4
EPS = 1e-5


def tol_of(dtype):
    return F32_TOL if dtype == 0 else BF16_TOL


def tdt(dtype):
    return torch.float32 if dtype == 0 else torch.bfloat16


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), device="cuda", dtype=tdt(dtype))


def prefill(n, k=0):
    """non-zero start values of an accumulated output"""
    return torch.linspace(-1.0, 1.0, n) * (1.0 + 0.25 * k) + 0.125


def show(name, **figures):
    print(name, " ".join(f"{k}={v:.3e}" for k, v in figures.items()))


# ====================================================================================== 1. pooled conv blocks (csrc/bnpool.hip)
POOL_SHAPES = [(2, 2, 2), (3, 5, 6), (5, 24, 16), (3, 25, 32)]
POOL_TYPES3 = [(0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]        # (dtype, ydtype, gdtype)
POOL_BWD_CASES = ([(s, t) for s in [(3, 5, 6), (5, 24, 16)] for t in POOL_TYPES3] +
                  [(s, (1, 1, 0)) for s in [(2, 2, 2), (3, 25, 32)]])


def pool_inputs(shape):
    Nimg, Ti, Fi = shape
    To, Fo = Ti // 2, Fi // 2
    g = torch.Generator().manual_seed(1000 + 100 * Ti + Fi)
    Y = torch.randint(-128, 129, (Nimg, Ti, Fi, 64), generator=g).float() / 32        # multiples of 1/32, |y| <= 4: exact in bf16
    gamma = torch.rand(64, generator=g) + 0.5
    gamma[3] = -0.7                                                  # the window's arg-max is the conv output's arg-min
    beta = torch.randn(64, generator=g) * 0.3
    dP = torch.randn(Nimg, To, Fo, 64, generator=g)
    dxl = torch.randn(Nimg, Fo, 64, generator=g)
    return Y, gamma, beta, dP, dxl


def bn_stats64(y64, gamma, beta, dims):
    """fp64 train-mode statistics -> the fp32 (scale, shift, mean, rstd) a kernel is handed"""
    mean, var = y64.mean(dims), y64.var(dims, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    g, b = gamma.double(), beta.double()
    return (g * rstd).float(), (b - mean * g * rstd).float(), mean.float(), rstd.float()


def windows(a, To, Fo):
    """a [N][Ti][Fi][C] -> [N][To][Fo][C][4], the window in (f, t) order"""
    n, _, _, c = a.shape
    w = a[:, :2 * To].reshape(n, To, 2, Fo, 2, c)                    # [n][to][dt][fo][df][c]
    return w.permute(0, 1, 3, 5, 4, 2).reshape(n, To, Fo, c, 4)


@functools.lru_cache(maxsize=None)
def pool_ref(shape, gdtype=0, with_dxl=True):
    """fp64 autograd through BatchNorm2d(train) -> ReLU -> MaxPool2d(2) (+ the mean over pooled time) on the stored inputs"""
    Nimg, Ti, Fi = shape
    To, Fo = Ti // 2, Fi // 2
    Y, gamma, beta, dP, dxl = pool_inputs(shape)
    if gdtype == 1:
        dP, dxl = dP.bfloat16().float(), dxl.bfloat16().float()
    assert torch.equal(Y.bfloat16().float(), Y)
    y = Y.double().requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2), unbiased=False)
    a = (y - mean) / torch.sqrt(var + EPS) * ga + be
    a.retain_grad()
    # torch's layout is [N][C][F][T]: a tie inside a window goes to the first maximum in (f, t) order
    P = torch.nn.functional.max_pool2d(torch.relu(a).permute(0, 3, 2, 1), 2).permute(0, 3, 2, 1)        # [N][To][Fo][64]
    loss = (P * dP.double()).sum()
    if with_dxl:
        loss = loss + (P.mean(1) * dxl.double()).sum()
    loss.backward()
    scale, shift, mean32, rstd32 = bn_stats64(y.detach(), gamma, beta, (0, 1, 2))
    # margins of the reference itself, on the affine map the kernel evaluates
    ah = scale.double() * y.detach() + shift.double()
    w = windows(ah, To, Fo)
    top = w.max(-1).values
    gaps = top[..., None] - w
    min_gap = float(gaps[gaps > 0].min()) if bool((gaps > 0).any()) else float("inf")
    assert min_gap >= 1e-4, min_gap
    assert float(top.abs().min()) >= 1e-5, float(top.abs().min())
    assert torch.equal(windows(a.detach(), To, Fo).argmax(-1), w.argmax(-1))
    assert torch.equal(windows(a.detach(), To, Fo).max(-1).values > 0, top > 0)
    xhat = (y.detach() - mean32.double()) * rstd32.double()
    return dict(Y=Y, gamma=gamma, beta=beta, dP=dP, dxl=dxl if with_dxl else None, scale=scale, shift=shift, mean=mean32,
                rstd=rstd32, P=P.detach(), dY=y.grad, dgamma=ga.grad, dbeta=be.grad, da=a.grad, xhat=xhat)


def pool_args(r, ydtype, gdtype):
    Y = dev(r["Y"]).to(tdt(ydtype))
    dP = dev(r["dP"]).to(tdt(gdtype))
    dxl = dev(r["dxl"]).to(tdt(gdtype)) if r["dxl"] is not None else None
    st = tuple(dev(r[k]) for k in ("scale", "shift", "mean", "rstd"))
    return Y, dP, dxl, st


def check_pool_bwd(name, r, dtype, dY, dg, db, dg0, db0, stat_tol=F32_TOL):
    Ti = r["Y"].shape[1]
    e = dict(dY=rel_l2(dY.float().cpu(), r["dY"]), dgamma=rel_l2(dg.cpu().double() - dg0.double(), r["dgamma"]),
             dbeta=rel_l2(db.cpu().double() - db0.double(), r["dbeta"]))
    if Ti % 2:
        # the unpooled last time row, scale * (-dbeta/n - xhat*dgamma/n): 1/Ti of the tensor, a whole-tensor rel-L2 would hide it
        assert float(r["dY"][:, Ti - 1].abs().min()) > 0.0
        e["dY_last_row"] = rel_l2(dY[:, Ti - 1].float().cpu(), r["dY"][:, Ti - 1])
    show(name, **e)
    assert torch.isfinite(dY.float()).all()
    assert e["dY"] <= tol_of(dtype) and e.get("dY_last_row", 0.0) <= tol_of(dtype)
    assert e["dgamma"] <= stat_tol and e["dbeta"] <= stat_tol


@pytest.mark.parametrize("dtype,ydtype", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_bn_relu_pool_fwd(N, shape, dtype, ydtype):
    """BN -> ReLU -> MaxPool2d(2) of a conv block; with odd Ti the last time row reaches no output."""
    Nimg, Ti, Fi = shape
    r = pool_ref(shape)
    Y, _, _, st = pool_args(r, ydtype, 0)
    P = nan_like((Nimg, Ti // 2, Fi // 2, 64), dtype)
    N.call("bn_relu_pool_fwd", dtype, ydtype, Y, st[0], st[1], P, Nimg, Ti, Fi)
    torch.cuda.synchronize()
    e = rel_l2(P.float().cpu(), r["P"])
    show(f"pool_fwd {shape} {dtype}{ydtype}", P=e)
    assert torch.isfinite(P.float()).all() and e <= tol_of(dtype)


def _stat_rows(Y):
    return Y.double().reshape(-1, 64)


def _lay_out_sums(rows, layout):
    """fp64 column sums of `rows` in one of the three layouts train_fwd reads -> (sum, sumsq, stat_replicas, folded [2][64])"""
    tot = torch.stack([rows.sum(0), (rows * rows).sum(0)])
    if layout == "separate":
        return dev(tot[0].clone()), dev(tot[1].clone()), 1, tot
    if layout == "contiguous":
        buf = dev(tot.reshape(128).clone())
        return buf, buf[64:], 1, tot
    # eight replicas holding the sums of uneven row ranges: sums at r*128, squares at r*128 + 64
    n = rows.shape[0]
    cuts = sorted({0, n} | {min(n, max(0, int(n * f))) for f in (0.03, 0.1, 0.11, 0.4, 0.55, 0.8, 0.97)})
    cuts = cuts + [n] * (9 - len(cuts))
    buf = torch.zeros(8, 128, dtype=torch.float64)
    for k in range(8):
        part = rows[cuts[k]:cuts[k + 1]]
        buf[k, :64], buf[k, 64:] = part.sum(0), (part * part).sum(0)
    buf = dev(buf.reshape(-1))
    return buf, buf[64:], 8, tot


@pytest.mark.parametrize("layout", ["separate", "contiguous", "replicas8"])
@pytest.mark.parametrize("dtype,ydtype", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_bn_relu_pool_train_fwd(N, shape, dtype, ydtype, layout):
    """bn_finalize + the pooled forward in one launch, from fp64 sums the test lays out itself: the statistics against fp64 and
    against bn_finalize on the folded sums, the running buffers after one update from non-trivial values."""
    Nimg, Ti, Fi = shape
    r = pool_ref(shape)
    Y, _, _, _ = pool_args(r, ydtype, 0)
    rows = _stat_rows(r["Y"])
    count = float(rows.shape[0])
    s, q, rep, tot = _lay_out_sums(rows, layout)
    gamma, beta = dev(r["gamma"]), dev(r["beta"])
    rm0, rv0 = prefill(64, 1), prefill(64, 2).abs() + 0.5
    rm, rv = dev(rm0.clone()), dev(rv0.clone())
    P = nan_like((Nimg, Ti // 2, Fi // 2, 64), dtype)
    st = [nan_like((64,), 0) for _ in range(4)]
    N.call("bn_relu_pool_train_fwd", dtype, ydtype, Y, s, q, rep, count, gamma, beta, rm, rv, 0.1, EPS, P, *st, Nimg, Ti, Fi)
    torch.cuda.synchronize()
    for got, name in zip(st, ("scale", "shift", "mean", "rstd")):
        np.testing.assert_allclose(got.cpu().numpy(), r[name].numpy(), rtol=1e-6, atol=0, err_msg=name)
    st2 = [nan_like((64,), 0) for _ in range(4)]
    tot_d = dev(tot)
    N.call("bn_finalize", tot_d[0], tot_d[1], 1, count, 64, gamma, beta, None, None, 0.1, EPS, *st2)
    torch.cuda.synchronize()
    for got, want in zip(st, st2):
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=0)
    mean = rows.mean(0)
    var = (rows * rows).mean(0) - mean * mean
    # this test's own bound: 0.9 * old + 0.1 * new is three fp32 roundings (2e-7 relative); atol 1e-7 covers a running mean that the
    # update leaves near zero, where the two addends of order 0.1 cancel
    np.testing.assert_allclose(rm.cpu().numpy(), (0.9 * rm0.double() + 0.1 * mean).numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(rv.cpu().numpy(), (0.9 * rv0.double() + 0.1 * var * count / (count - 1.0)).numpy(), rtol=1e-6, atol=1e-7)
    e = rel_l2(P.float().cpu(), r["P"])
    show(f"pool_train_fwd {shape} {dtype}{ydtype} {layout}", P=e)
    assert torch.isfinite(P.float()).all() and e <= tol_of(dtype)


@pytest.mark.parametrize("shape", [(3, 5, 6), (5, 24, 16)])
def test_bn_relu_pool_train_fwd_null_running_and_count(N, shape):
    """NULL running buffers are accepted, and `count` is what divides the sums: with the sums of a batch twice as large and
    count = 2*N*Ti*Fi the statistics (and the pooled output) are the larger batch's."""
    Nimg, Ti, Fi = shape
    r = pool_ref(shape)
    dtype = ydtype = 1
    Y, _, _, _ = pool_args(r, ydtype, 0)
    gamma, beta = dev(r["gamma"]), dev(r["beta"])
    g = torch.Generator().manual_seed(77 + Ti)
    other = torch.randint(-128, 129, tuple(r["Y"].shape), generator=g).float() / 32 * 0.5 + 1.0
    rows = torch.cat([_stat_rows(r["Y"]), _stat_rows(other)])
    want = bn_stats64(rows, r["gamma"], r["beta"], (0,))
    for layout in ("separate", "replicas8"):
        s, q, rep, _ = _lay_out_sums(rows, layout)
        P = nan_like((Nimg, Ti // 2, Fi // 2, 64), dtype)
        st = [nan_like((64,), 0) for _ in range(4)]
        N.call("bn_relu_pool_train_fwd", dtype, ydtype, Y, s, q, rep, float(rows.shape[0]), gamma, beta, None, None, 0.1, EPS, P, *st,
               Nimg, Ti, Fi)
        torch.cuda.synchronize()
        for got, w, name in zip(st, want, ("scale", "shift", "mean", "rstd")):
            np.testing.assert_allclose(got.cpu().numpy(), w.numpy(), rtol=1e-6, atol=0, err_msg=name)
        a = want[0].double() * r["Y"].double() + want[1].double()
        Pw = torch.nn.functional.max_pool2d(torch.relu(a).permute(0, 3, 2, 1), 2).permute(0, 3, 2, 1)
        assert rel_l2(P.float().cpu(), Pw) <= BF16_TOL


@pytest.mark.parametrize("with_dxl", [True, False])
@pytest.mark.parametrize("shape,types", POOL_BWD_CASES)
def test_bn_relu_pool_bwd(N, shape, types, with_dxl):
    """One-launch backward, statistics from a sweep over Y (`bn_relu_pool_bwd`) and from the pooled output (`_bwd_p`)."""
    dtype, ydtype, gdtype = types
    Nimg, Ti, Fi = shape
    r = pool_ref(shape, gdtype, with_dxl)
    Y, dP, dxl, st = pool_args(r, ydtype, gdtype)
    Pst = dev(r["P"].to(tdt(dtype)))                                 # what the forward stores
    for entry in ("bn_relu_pool_bwd", "bn_relu_pool_bwd_p"):
        stat = nan_like((33 * 128,), 0)
        dY = nan_like((Nimg, Ti, Fi, 64), dtype)
        dg0, db0 = prefill(64, 1), prefill(64, 2)
        dg, db = dev(dg0.clone()), dev(db0.clone())
        args = (dtype, ydtype, gdtype, Y) + ((Pst,) if entry.endswith("_p") else ()) + (dP, dxl, *st, stat, dY, dg, db, Nimg, Ti, Fi)
        N.call(entry, *args)
        torch.cuda.synchronize()
        # _p recomputes xhat from P: one bf16 rounding of the activation in every term of the sums (4e-3 as in
        # test_bn_relu_pool_bwd_sums_from_the_pooled_output); an fp32 P leaves fp32 arithmetic only
        stat_tol = BF16_TOL if (entry.endswith("_p") and dtype == 1) else F32_TOL
        check_pool_bwd(f"{entry} {shape} {types} dxl={with_dxl}", r, dtype, dY, dg, db, dg0, db0, stat_tol)


@pytest.mark.parametrize("with_dxl", [True, False])
@pytest.mark.parametrize("types", POOL_TYPES3)
@pytest.mark.parametrize("shape,split", [((5, 24, 16), 3), ((3, 5, 6), 2)])
def test_bn_relu_pool_bwd_halves(N, shape, split, types, with_dxl):
    """SyncBatchNorm halves on one GPU: `_stats` on each part of the batch, the sums added as the all-reduce would, `_apply`
    on each part with the global count; both applies add into the same dgamma / dbeta."""
    dtype, ydtype, gdtype = types
    Nimg, Ti, Fi = shape
    r = pool_ref(shape, gdtype, with_dxl)
    Y, dP, dxl, st = pool_args(r, ydtype, gdtype)
    parts = [slice(0, split), slice(split, Nimg)]
    stats = []
    for p in parts:
        stat = nan_like((33 * 128,), 0)
        n = p.stop - p.start
        N.call("bn_relu_pool_bwd_stats", dtype, ydtype, gdtype, Y[p].contiguous(), dP[p].contiguous(),
               dxl[p].contiguous() if dxl is not None else None, *st, stat, n, Ti, Fi)
        torch.cuda.synchronize()
        want = torch.cat([r["da"][p].sum((0, 1, 2)), (r["da"][p] * r["xhat"][p]).sum((0, 1, 2))])
        e = rel_l2(stat[:128].cpu(), want)
        show(f"pool_bwd_stats {shape} {types} part {p.start}:{p.stop}", stat=e)
        assert e <= F32_TOL
        stats.append(stat)
    gstat = (stats[0][:128] + stats[1][:128]).contiguous()
    dY = nan_like((Nimg, Ti, Fi, 64), dtype)
    dg0, db0 = prefill(64, 1), prefill(64, 2)
    dg, db = dev(dg0.clone()), dev(db0.clone())
    for p, stat in zip(parts, stats):
        n = p.stop - p.start
        dYp = nan_like((n, Ti, Fi, 64), dtype)
        N.call("bn_relu_pool_bwd_apply", dtype, ydtype, gdtype, Y[p].contiguous(), dP[p].contiguous(),
               dxl[p].contiguous() if dxl is not None else None, *st, stat, gstat, float(Nimg * Ti * Fi), dYp, dg, db, n, Ti, Fi)
        dY[p] = dYp
    torch.cuda.synchronize()
    check_pool_bwd(f"pool_bwd_halves {shape} {types} dxl={with_dxl}", r, dtype, dY, dg, db, dg0, db0)


@pytest.mark.parametrize("types", POOL_TYPES3)
def test_bn_relu_pool_bwd_world_of_one_is_the_one_launch_entry(N, types):
    """(3, 5, 6) is one workgroup, so every replica of the statistics receives one add and nothing depends on atomic order:
    stats + apply(gstat = own sums, count = N*Ti*Fi) gives the bits of `bn_relu_pool_bwd` (both fold the replicas in replica
    order and multiply by the same inv_count)."""
    dtype, ydtype, gdtype = types
    shape = (3, 5, 6)
    Nimg, Ti, Fi = shape
    r = pool_ref(shape, gdtype, True)
    Y, dP, dxl, st = pool_args(r, ydtype, gdtype)
    out = []
    for halves in (False, True):
        stat = nan_like((33 * 128,), 0)
        dY = nan_like((Nimg, Ti, Fi, 64), dtype)
        dg, db = dev(prefill(64, 1)), dev(prefill(64, 2))
        if halves:
            N.call("bn_relu_pool_bwd_stats", dtype, ydtype, gdtype, Y, dP, dxl, *st, stat, Nimg, Ti, Fi)
            N.call("bn_relu_pool_bwd_apply", dtype, ydtype, gdtype, Y, dP, dxl, *st, stat, stat[:128].clone(), float(Nimg * Ti * Fi),
                   dY, dg, db, Nimg, Ti, Fi)
        else:
            N.call("bn_relu_pool_bwd", dtype, ydtype, gdtype, Y, dP, dxl, *st, stat, dY, dg, db, Nimg, Ti, Fi)
        torch.cuda.synchronize()
        out.append((dY, dg, db))
    assert torch.isfinite(out[0][0].float()).all()
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ====================================================================================== 2. projector BatchNorm1d (csrc/heads.hip)
COLBN_TYPES3 = [(0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]      # (dtype, adtype, gdtype)
COLBN_CASES = ([(M, C, relu, aff, (1, 0, 0)) for M in (1100, 4100) for C in (64, 192) for relu in (0, 1) for aff in (True, False)] +
               [(1100, 64, 1, True, t) for t in COLBN_TYPES3 if t != (1, 0, 0)])
G = 2
COLBN_SEEDS = {(4100, 192): 27}             # (M, C) -> seed, where 3 + M + C leaves a pre-activation closer than 1e-6 to the ReLU gate


@functools.lru_cache(maxsize=4)
def colbn_inputs(M, C, adtype, gdtype):
    g = torch.Generator().manual_seed(COLBN_SEEDS.get((M, C), 3 + M + C))
    a = torch.randn(G, M, C, generator=g) * 1.7 + 0.4
    dh = torch.randn(G, M, C, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[5] = -0.8
    beta = torch.randn(C, generator=g) * 0.1
    if adtype == 1:
        a = a.bfloat16().float()
    if gdtype == 1:
        dh = dh.bfloat16().float()
    return a, dh, gamma, beta


@functools.lru_cache(maxsize=4)
def colbn_ref(M, C, relu, affine, adtype, gdtype):
    """torch batch_norm(training=True) per group, fp64 autograd on the stored inputs; the statistics the kernels are handed"""
    a32, dh, gamma, beta = colbn_inputs(M, C, adtype, gdtype)
    a = a32.double().requires_grad_(True)
    ga = gamma.double().requires_grad_(True) if affine else None
    be = beta.double().requires_grad_(True) if affine else None
    pre = torch.stack([torch.nn.functional.batch_norm(a[k], None, None, ga, be, True, 0.1, EPS) for k in range(G)])
    pre.retain_grad()
    h = torch.relu(pre) if relu else pre
    h.backward(dh.double())
    ones, zeros = torch.ones(C), torch.zeros(C)
    st = [torch.stack(x) for x in zip(*[bn_stats64(a[k].detach(), gamma if affine else ones, beta if affine else zeros, (0,))
                                         for k in range(G)])]               # scale, shift, mean, rstd [G][C]
    handed = st[0].double()[:, None] * a.detach() + st[1].double()[:, None]
    if relu:
        m = min(float(handed.abs().min()), float(pre.detach().abs().min()))
        assert m >= 1e-6, m
        assert torch.equal(handed > 0, pre.detach() > 0)
    xhat = (a.detach() - st[2].double()[:, None]) * st[3].double()[:, None]
    return dict(a=a32, dh=dh, gamma=gamma if affine else None, beta=beta if affine else None, st=st, da=a.grad,
                dgamma=ga.grad if affine else None, dbeta=be.grad if affine else None, g=pre.grad, xhat=xhat)


def colbn_args(r, adtype, gdtype):
    return (dev(r["a"]).to(tdt(adtype)), dev(r["dh"]).to(tdt(gdtype)), tuple(dev(s.reshape(-1)) for s in r["st"]))


@pytest.mark.parametrize("M,C,relu,affine,types", COLBN_CASES)
def test_colbn_bwd_two_kernel_path(N, M, C, relu, affine, types):
    """M > 1024: `colbn_bwd` is colbn_bwd_stats_kernel + colbn_bwd_apply_kernel over several row blocks - 1100 rows = 17 blocks
    of 64 + 12 rows, 4100 rows = 16 blocks of 256 + 4 rows (what `BatchNorm1dFn` reaches for any batch above 1024 rows)."""
    dtype, adtype, gdtype = types
    r = colbn_ref(M, C, relu, affine, adtype, gdtype)
    a, dh, st = colbn_args(r, adtype, gdtype)
    da = nan_like((G, M, C), dtype)
    tmp = torch.full((2 * G * C,), float("nan"), device="cuda", dtype=torch.float64)
    dg0, db0 = prefill(C, 1), prefill(C, 2)
    dg, db = (dev(dg0.clone()), dev(db0.clone())) if affine else (None, None)
    N.call("colbn_bwd", dtype, adtype, gdtype, a, dh, *st, relu, G, M, C, tmp, da, dg, db)
    torch.cuda.synchronize()
    e = dict(da=rel_l2(da.float().cpu(), r["da"]))
    if affine:
        e["dgamma"] = rel_l2(dg.cpu().double() - dg0.double(), r["dgamma"])
        e["dbeta"] = rel_l2(db.cpu().double() - db0.double(), r["dbeta"])
    show(f"colbn_bwd M={M} C={C} relu={relu} affine={affine} {types}", **e)
    assert torch.isfinite(da.float()).all() and e["da"] <= tol_of(dtype)
    assert e.get("dgamma", 0.0) <= F32_TOL and e.get("dbeta", 0.0) <= F32_TOL


@pytest.mark.parametrize("types", COLBN_TYPES3)
def test_colbn_bwd_halves(N, types):
    """SyncBatchNorm halves of the projector: 1100 rows as 700 + 400.  `colbn_bwd_stats` leaves each part's sums in
    tmp [2][G*C] (fp64); `colbn_bwd_apply` takes the added sums and count = 1100; the parameter gradients are each part's own
    sums through `add_d2f`, as `engine.projector_backward` takes them.
    The sums are compared element-wise, each column within 1e-6 of the sum of the magnitudes of its own terms: every thread of
    colbn_bwd_stats_kernel adds its rows of a row block (2 of 64 here) in fp32 before the fp64 fold, so a column's error is a few
    2^-24 of sum |term| (three roundings in g * (x - mean) * rstd and one add: <= 2.4e-7), whatever the signed terms cancel to;
    a wrong or missing row is of the order of one term, 1 / 700 of that sum."""
    dtype, adtype, gdtype = types
    M, C, relu = 1100, 64, 1
    r = colbn_ref(M, C, relu, True, adtype, gdtype)
    a, dh, st = colbn_args(r, adtype, gdtype)
    parts = [slice(0, 700), slice(700, M)]
    tmps = []
    for p in parts:
        tmp = torch.full((2, G * C), float("nan"), device="cuda", dtype=torch.float64)
        N.call("colbn_bwd_stats", dtype, adtype, gdtype, a[:, p].contiguous(), dh[:, p].contiguous(), *st, relu, G, p.stop - p.start, C, tmp)
        torch.cuda.synchronize()
        terms = torch.stack([r["g"][:, p], r["g"][:, p] * r["xhat"][:, p]])              # [2][G][rows][C]
        want, mag = terms.sum(2).reshape(2, -1), terms.abs().sum(2).reshape(2, -1)
        err = (tmp.cpu() - want).abs() / mag
        e = dict(sg=float(err[0].max()), sgx=float(err[1].max()))
        show(f"colbn_bwd_stats {types} rows {p.start}:{p.stop} (worst column, error / sum |term|)", **e)
        assert torch.isfinite(tmp).all() and float(mag.min()) > 0.0 and e["sg"] <= 1e-6 and e["sgx"] <= 1e-6
        tmps.append(tmp)
    sums = (tmps[0] + tmps[1]).contiguous()
    da = nan_like((G, M, C), dtype)
    dg0, db0 = prefill(C, 1), prefill(C, 2)
    dg, db = dev(dg0.clone()), dev(db0.clone())
    for p, tmp in zip(parts, tmps):
        dap = nan_like((G, p.stop - p.start, C), dtype)
        N.call("colbn_bwd_apply", dtype, adtype, gdtype, a[:, p].contiguous(), dh[:, p].contiguous(), *st, relu, G, p.stop - p.start, C,
               sums, float(M), dap)
        da[:, p] = dap
        flat = tmp.reshape(-1)                                       # [dbeta sums: G x C][dgamma sums: G x C]
        for k in range(G):
            N.call("add_d2f", flat[k * C:(k + 1) * C], db, C)
            N.call("add_d2f", flat[(G + k) * C:(G + k + 1) * C], dg, C)
    torch.cuda.synchronize()
    e = dict(da=rel_l2(da.float().cpu(), r["da"]), dgamma=rel_l2(dg.cpu().double() - dg0.double(), r["dgamma"]),
             dbeta=rel_l2(db.cpu().double() - db0.double(), r["dbeta"]))
    show(f"colbn_bwd_halves {types}", **e)
    assert torch.isfinite(da.float()).all() and e["da"] <= tol_of(dtype)
    assert e["dgamma"] <= F32_TOL and e["dbeta"] <= F32_TOL


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dtype,adtype", [(0, 0), (1, 0), (1, 1)])
def test_colbn_eval_mode(N, dtype, adtype, relu):
    """Eval-mode BatchNorm1d: `bn_eval_affine` folds the running statistics of each group's layer into scale / shift,
    `colbn_fwd` applies them per group."""
    M, C = 37, 72
    g = torch.Generator().manual_seed(19)
    a = (torch.randn(G, M, C, generator=g) * 1.7 + 0.4).to(tdt(adtype)).float()
    gamma, beta, rm = (torch.randn(G, C, generator=g) for _ in range(3))
    rv = torch.rand(G, C, generator=g) + 0.2
    scale, shift = nan_like((G, C), 0), nan_like((G, C), 0)
    gd, bd, rmd, rvd = dev(gamma), dev(beta), dev(rm), dev(rv)
    for k in range(G):
        N.call("bn_eval_affine", gd[k], bd[k], rmd[k], rvd[k], EPS, C, scale[k], shift[k])
    h = nan_like((G, M, C), dtype)
    N.call("colbn_fwd", dtype, adtype, dev(a).to(tdt(adtype)), scale, shift, relu, h, G, M, C)
    torch.cuda.synchronize()
    want = gamma.double()[:, None] * (a.double() - rm.double()[:, None]) / torch.sqrt(rv.double()[:, None] + EPS) + beta.double()[:, None]
    want = torch.relu(want) if relu else want
    e = rel_l2(h.float().cpu(), want)
    show(f"colbn_eval {dtype}{adtype} relu={relu}", h=e)
    assert torch.isfinite(h.float()).all() and e <= tol_of(dtype)


# ====================================================================================== 3. stem backward (csrc/conv1.hip)
STEM_SHAPES = [(3, 32, 11), (3, 64, 10)]
STEM_SALT = 100              # salt of the image: at both shapes it leaves every window gap and every ReLU gate wider than 1e-5


@functools.lru_cache(maxsize=None)
def stem_ref(shape, round_bf16=False, gdtype=0):
    """fp64 autograd through Conv2d(1,64,3,p=1) -> BatchNorm2d(train) -> ReLU -> MaxPool2d(2) and the mean over pooled time;
    gdtype 1: the incoming gradients as a bf16 caller stores them"""
    import torch.nn as nn
    Nimg, F_, T = shape
    To, Fo = T // 2, F_ // 2
    blk = nn.Sequential(nn.Conv2d(1, 64, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU(), nn.MaxPool2d(2, 2))
    fill.fill_state_dict_(blk, seed=5)
    blk.train()
    x = torch.from_numpy(fill.normalish((Nimg, 1, F_, T), STEM_SALT))
    conv, bn = blk[0], blk[1]
    w32, b32 = conv.weight.detach().clone(), conv.bias.detach().clone()
    gamma, beta = bn.weight.detach().clone(), bn.bias.detach().clone()
    gP = torch.from_numpy(fill.uniform((Nimg, 64, Fo, To), 42))
    gX1 = torch.from_numpy(fill.uniform((Nimg, Fo * 64), 43))
    if gdtype == 1:
        gP, gX1 = gP.bfloat16().float(), gX1.bfloat16().float()
    xin = (x.bfloat16().float() if round_bf16 else x).double()
    w = (w32.bfloat16().float() if round_bf16 else w32).double().requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = torch.nn.functional.conv2d(xin, w, b32.double(), padding=1)                       # [N][64][F][T]
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    a = (y - mean[None, :, None, None]) * (rstd * ga)[None, :, None, None] + be[None, :, None, None]
    a.retain_grad()
    P = torch.nn.functional.max_pool2d(torch.relu(a), 2)                                   # [N][64][Fo][To]
    x1 = P.permute(0, 3, 2, 1).reshape(Nimg, To, -1).mean(1)
    ((P * gP.double()).sum() + (x1 * gX1.double()).sum()).backward()
    xhat = ((y - mean[None, :, None, None]) * rstd[None, :, None, None]).detach()
    if not round_bf16:
        # margins of the reference itself: the fp32 VALU flavour evaluates nine FMAs per pixel, |a| of order one - 1e-5 is some ten
        # times its error, so both sides route every window alike and open the same ReLU gates
        ad = a.detach()
        win = ad[:, :, :, :2 * To].reshape(Nimg, 64, Fo, 2, To, 2).permute(0, 1, 2, 4, 3, 5).reshape(Nimg, 64, Fo, To, 4)
        srt = win.sort(-1, descending=True).values
        assert float((srt[..., 0] - srt[..., 1]).min()) >= 1e-5, float((srt[..., 0] - srt[..., 1]).min())
        assert float(srt[..., 0].abs().min()) >= 1e-5, float(srt[..., 0].abs().min())
    return dict(x=x[:, 0].contiguous(), w=w32.reshape(64, 9), b=b32, gamma=gamma, beta=beta, dP=gP.permute(0, 3, 2, 1).contiguous(),
                dxl=gX1, P=P.detach().permute(0, 3, 2, 1), dW=w.grad.reshape(64, 9), dgamma=ga.grad, dbeta=be.grad,
                mean=mean.detach(), rstd=rstd.detach(), scale=(gamma.double() * rstd).detach(),
                shift=(beta.double() - mean * gamma.double() * rstd).detach(), da=a.grad, xhat=xhat)


def stem_forward(N, r, shape, flavour):
    """conv1_stats + conv1_fwd of the whole batch -> (img, parameters, (scale, shift, mean, rstd), mom, P)"""
    Nimg, F_, T = shape
    img = dev(r["x"])
    par = tuple(dev(r[k]) for k in ("w", "b", "gamma", "beta"))
    mom = torch.full((16 * 54,), float("nan"), device="cuda", dtype=torch.float64)
    st = tuple(nan_like((64,), 0) for _ in range(4))
    N.call("conv1_stats", img, Nimg, F_, T, *par, None, None, 0.1, EPS, mom, *st)
    P = nan_like((Nimg, T // 2, F_ // 2, 64), flavour)
    N.call("conv1_fwd", flavour, img, Nimg, F_, T, par[0], par[1], st[0], st[1], P, None)
    torch.cuda.synchronize()
    return img, par, st, mom, P


def stem_bwd(N, shape, flavour, img, par, st, mom, dP, dxl, dp_dtype=0):
    Nimg, F_, T = shape
    w, b, gamma, _ = par
    acc = nan_like((32 * 64 * 11,), 0)
    start = [prefill(576, 1).reshape(64, 9), prefill(64, 2), prefill(64, 3)]
    dW, dg, dbt = (dev(s.clone()) for s in start)
    dbias = torch.zeros(64, device="cuda")
    N.call("conv1_bwd", dp_dtype, flavour, img, Nimg, F_, T, w, b, gamma, *st, mom, dP, dxl, acc, dW, dbias, dg, dbt)
    torch.cuda.synchronize()
    assert float(dbias.abs().max()) == 0.0
    return [(o.cpu().double() - s.double()) for o, s in zip((dW, dg, dbt), start)]


@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_conv1_bwd_whole_batch(N, shape, flavour):
    """conv1_stats -> conv1_fwd -> conv1_bwd against fp64 autograd, the dxl term included.  F = 32 is the general MFMA
    instantiation (conv1_bwd_mfma_kernel<false, ...>) and the VALU kernel below F = 64; T = 11 leaves the last column unpooled.
    Flavour 0: 2e-4 as test_conv1_block_fwd_bwd.  Flavour 1 recomputes the conv on bf16 operands, so a share of near-tied
    windows route elsewhere: that test's 8e-2, next to the reference's own figure for the shape (fp64 autograd on bf16-rounded
    image and weights against the unrounded ones), as (dW, dgamma, dbeta):
      (3, 32, 11)  kernel, flavour 1 4.3e-2, 1.9e-3, 1.1e-2    reference's own 4.3e-2, 1.7e-3, 1.1e-2
      (3, 64, 10)  kernel, flavour 1 3.5e-2, 2.2e-3, 1.7e-2    reference's own 3.5e-2, 2.0e-3, 1.7e-2
    (measured on an MI355X; flavour 0 gives 1e-7 on all three at both shapes).  The kernel's error is the rounding of its operands
    and no more: at F = 32 the general MFMA instantiation sits at half the bound, as the F = 64 one does.  Both sets of figures are
    printed on every run (pytest -s)."""
    Nimg, F_, T = shape
    r = stem_ref(shape)
    img, par, st, mom, P = stem_forward(N, r, shape, flavour)
    for got, name in zip(st, ("scale", "shift", "mean", "rstd")):
        assert rel_l2(got.cpu(), r[name]) <= F32_TOL, name
    assert rel_l2(P.float().cpu(), r["P"]) < (1e-5 if flavour == 0 else 1e-2)
    dP, dxl = dev(r["dP"]), dev(r["dxl"])
    got = stem_bwd(N, shape, flavour, img, par, st, mom, dP, dxl)
    e = {k: rel_l2(g, r[k]) for g, k in zip(got, ("dW", "dgamma", "dbeta"))}
    show(f"conv1_bwd {shape} flavour {flavour}", **e)
    if flavour == 1:
        rb = stem_ref(shape, True)
        show(f"conv1_bwd {shape} reference's own bf16 figure", **{k: rel_l2(rb[k], r[k]) for k in ("dW", "dgamma", "dbeta")})
    tol = 2e-4 if flavour == 0 else 8e-2
    assert all(v < tol for v in e.values()), e
    if flavour == 1:
        # the MFMA flavour also takes the pooled gradient in bf16 (dxl stays fp32): same result up to the rounding of dP
        got2 = stem_bwd(N, shape, 1, img, par, st, mom, dP.bfloat16().contiguous(), dxl, dp_dtype=1)
        assert all(rel_l2(a, b) < 5e-3 for a, b in zip(got2, got))


@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_conv1_halves(N, shape, flavour):
    """SyncBatchNorm halves of the stem on a 2 + 1 split; both parts use the whole batch's scale / shift / mean / rstd, so the
    routing is the one-launch run's.  conv1_moments per part -> totals add up; conv1_finalize on the sum == conv1_stats;
    conv1_bwd_sums per part -> lstat; conv1_bwd_finalize per part with THAT PART'S OWN mom, the added lstat and the global
    count -> dW, dgamma, dbeta accumulated over the parts == the one-launch conv1_bwd."""
    Nimg, F_, T = shape
    r = stem_ref(shape)
    img, par, st, mom, _ = stem_forward(N, r, shape, flavour)
    w, b, gamma, beta = par
    dP, dxl = dev(r["dP"]), dev(r["dxl"])
    whole = stem_bwd(N, shape, flavour, img, par, st, mom, dP, dxl)
    parts = [slice(0, 2), slice(2, Nimg)]
    moms = []
    for p in parts:
        m = torch.full((16 * 54,), float("nan"), device="cuda", dtype=torch.float64)
        N.call("conv1_moments", img[p].contiguous(), p.stop - p.start, F_, T, m)
        moms.append(m)
    torch.cuda.synchronize()
    tot = moms[0][:54] + moms[1][:54]
    np.testing.assert_allclose(tot.cpu().numpy(), mom[:54].cpu().numpy(), rtol=1e-12, atol=0)
    mt = torch.zeros(16 * 54, device="cuda", dtype=torch.float64)
    mt[:54] = tot
    st2 = tuple(nan_like((64,), 0) for _ in range(4))
    N.call("conv1_finalize", mt, w, b, gamma, beta, None, None, 0.1, EPS, float(Nimg * F_ * T), *st2)
    torch.cuda.synchronize()
    for got, want in zip(st2, st):
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=0)
    accs, lstats = [], []
    for p, m in zip(parts, moms):
        acc, lstat = nan_like((32 * 64 * 11,), 0), nan_like((128,), 0)
        N.call("conv1_bwd_sums", 0, flavour, img[p].contiguous(), p.stop - p.start, F_, T, w, b, gamma, *st, m, dP[p].contiguous(),
               dxl[p].contiguous(), acc, lstat)
        torch.cuda.synchronize()
        if flavour == 0:
            da, xhat = r["da"][p], r["xhat"][p]
            want = torch.cat([da.sum((0, 2, 3)), (da * xhat).sum((0, 2, 3))])
            e = rel_l2(lstat.cpu(), want)
            show(f"conv1_bwd_sums {shape} part {p.start}:{p.stop}", lstat=e)
            assert e <= F32_TOL
        accs.append(acc)
        lstats.append(lstat)
    gstat = (lstats[0] + lstats[1]).contiguous()
    start = [prefill(576, 1).reshape(64, 9), prefill(64, 2), prefill(64, 3)]
    dW, dg, dbt = (dev(s.clone()) for s in start)
    dbias = torch.zeros(64, device="cuda")
    for acc, m in zip(accs, moms):
        N.call("conv1_bwd_finalize", acc, m, w, b, gamma, st[2], st[3], float(Nimg * F_ * T), gstat, dW, dbias, dg, dbt)
    torch.cuda.synchronize()
    got = [(o.cpu().double() - s.double()) for o, s in zip((dW, dg, dbt), start)]
    e = {k: rel_l2(g, wh) for g, wh, k in zip(got, whole, ("dW", "dgamma", "dbeta"))}
    show(f"conv1_halves {shape} flavour {flavour} vs one launch", **e)
    assert all(v < 2e-4 for v in e.values()), e
    if flavour == 0:
        e = {k: rel_l2(g, r[k]) for g, k in zip(got, ("dW", "dgamma", "dbeta"))}
        show(f"conv1_halves {shape} flavour 0 vs fp64", **e)
        assert all(v < 2e-4 for v in e.values()), e


# ====================================================================================== 4. encoder tail (maxmean)
MAXMEAN_SHAPES = [(3, 1, 8), (2, 12, 2048), (2, 255, 64), (5, 7, 24)]


@functools.lru_cache(maxsize=None)
def maxmean_inputs(shape):
    """a ReLU output rounded to bf16, with whole columns of zeros and repeated maxima"""
    Nimg, Tt, D = shape
    g = torch.Generator().manual_seed(7 + Tt + D)
    H = torch.relu(torch.randn(Nimg, Tt, D, generator=g)).bfloat16().float()
    H[:, :, 1::8] = 0.0                                              # whole columns of zeros: the first arg-max is 0
    if Tt > 1:
        top = H.max(1).values
        H[:, Tt - 1, 2::8] = top[:, 2::8]                            # the maximum again in the last row
        H[:, Tt // 2, 4::8] = top[:, 4::8]                           # ... and in the middle
    nz = H[H > 0]
    assert float(nz.min()) >= 1e-6
    dy = torch.randn(Nimg, D, generator=g)
    arg = np.argmax(H.numpy(), axis=1).astype(np.uint8)              # numpy: the first maximum
    return H, dy, arg


@pytest.mark.parametrize("dtype,out_f32", [(0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize("shape", MAXMEAN_SHAPES)
def test_maxmean_fwd(N, shape, dtype, out_f32):
    Nimg, Tt, D = shape
    H, _, arg_want = maxmean_inputs(shape)
    odt = 0 if out_f32 else 1
    y = nan_like((Nimg, D), odt)
    arg = torch.full((Nimg, D), 255, device="cuda", dtype=torch.uint8)
    N.call("maxmean_fwd", dtype, out_f32, dev(H).to(tdt(dtype)), y, arg, Nimg, Tt, D)
    torch.cuda.synchronize()
    assert np.array_equal(arg.cpu().numpy(), arg_want)
    want = H.double().max(1).values + H.double().mean(1)
    e = rel_l2(y.float().cpu(), want)
    show(f"maxmean_fwd {shape} {dtype} out_f32={out_f32}", y=e)
    assert torch.isfinite(y.float()).all() and e <= tol_of(odt)


@pytest.mark.parametrize("dtype,gdtype", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", MAXMEAN_SHAPES)
def test_maxmean_bwd(N, shape, dtype, gdtype):
    Nimg, Tt, D = shape
    H, dy, arg = maxmean_inputs(shape)
    if gdtype == 1:
        dy = dy.bfloat16().float()
    dA = nan_like((Nimg, Tt, D), dtype)
    N.call("maxmean_bwd", dtype, gdtype, dev(dy).to(tdt(gdtype)), dev(arg), dev(H).to(tdt(dtype)), dA, Nimg, Tt, D)
    torch.cuda.synchronize()
    onehot = torch.from_numpy(arg.astype(np.int64))[:, None, :] == torch.arange(Tt)[None, :, None]
    want = (dy.double()[:, None, :] / Tt + dy.double()[:, None, :] * onehot) * (H > 0)
    e = rel_l2(dA.float().cpu(), want)
    show(f"maxmean_bwd {shape} {dtype}{gdtype}", dA=e)
    assert torch.isfinite(dA.float()).all() and e <= tol_of(dtype)


def test_maxmean_refuses_256_time_steps(N):
    """`arg` is a uint8 time index: Tt = 256 is AUDIOSSL_EINVAL"""
    H = torch.zeros(1, 256, 8, device="cuda")
    y, arg = torch.zeros(1, 8, device="cuda"), torch.zeros(1, 8, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="EINVAL"):
        N.call("maxmean_fwd", 0, 1, H, y, arg, 1, 256, 8)
