"""GPU: every storage-type combination of the launchers written on csrc/dispatch.h that no other GPU test calls through the
C ABI (the rule: `dtype` is the path, each wide code is 0 or `dtype`; 2, 3 or 5 instantiations per entry point), and both
halves of the 8 / 16 rows-per-thread split (M <= 512 / M <= 1024) where the other tests reach one only.

Conventions of test_gpu_bn_chain.py, whose helpers are used: the reference is fp64 torch on the inputs as stored, written
outputs start as NaN and accumulated ones non-zero, fp32 outputs and sums are within rel-L2 1e-4, bf16 outputs within 4.0e-3,
integers, copies and roundings are compared bit for bit, and a reference with a ReLU gate asserts its own margin first."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import rel_l2
from test_gpu_bn_chain import (N, dev, F32_TOL, EPS, G, tol_of, tdt, nan_like, prefill, show, bn_stats64,     # noqa: F401 (N: fixture)
                               stem_ref, stem_forward, stem_bwd)

pytestmark = pytest.mark.gpu

PAIRS = [(0, 0), (1, 0), (1, 1)]                                         # (dtype, wide code)
TRIPLES = [(0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]        # (dtype, adtype, gdtype)
ROWS = [40, 520]                                                         # 8 and 16 rows per thread


def harr(ctype, xs):
    """host array of device pointers / scalars for a multi-problem entry point (None -> null pointer)"""
    return (ctype * len(xs))(*[x.data_ptr() if isinstance(x, torch.Tensor) else x for x in xs])


def scalar_err(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


# ====================================================================================== 1. one-launch BatchNorm1d (csrc/heads.hip)
HEAD_SEEDS = {(520, 32, 2): 1}              # (M, C, salt) -> seed, where the default leaves a pre-activation within 1e-6 of the gate


@functools.lru_cache(maxsize=None)
def head_ref(M, C, adtype, gdtype, salt=0, affine=True):
    """train-mode batch_norm -> ReLU per group on the stored inputs, fp64 autograd; running buffers updated group after group"""
    g = torch.Generator().manual_seed(HEAD_SEEDS.get((M, C, salt), 11 + M + C + 1000 * salt))
    a32 = (torch.randn(G, M, C, generator=g) * 1.7 + 0.4).to(tdt(adtype)).float()
    dh = torch.randn(G, M, C, generator=g).to(tdt(gdtype)).float()
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[5] = -0.8
    beta = torch.randn(C, generator=g) * 0.1
    rm0, rv0 = prefill(C, 1), prefill(C, 2).abs() + 0.5
    rm, rv = rm0.double(), rv0.double()
    a = a32.double().requires_grad_(True)
    ga = gamma.double().requires_grad_(True) if affine else None
    be = beta.double().requires_grad_(True) if affine else None
    pre = torch.stack([torch.nn.functional.batch_norm(a[k], rm, rv, ga, be, True, 0.1, EPS) for k in range(G)])
    h = torch.relu(pre)
    h.backward(dh.double())
    ones, zeros = torch.ones(C), torch.zeros(C)
    st = [torch.stack(x) for x in zip(*[bn_stats64(a[k].detach(), gamma if affine else ones, beta if affine else zeros, (0,))
                                         for k in range(G)])]               # scale, shift, mean, rstd [G][C]
    handed = st[0].double()[:, None] * a.detach() + st[1].double()[:, None]
    m = min(float(handed.abs().min()), float(pre.detach().abs().min()))
    assert m >= 1e-6, m
    assert torch.equal(handed > 0, pre.detach() > 0)
    return dict(a=a32, dh=dh, gamma=gamma if affine else None, beta=beta if affine else None, rm0=rm0, rv0=rv0, rm=rm, rv=rv, st=st,
                h=h.detach(), da=a.grad, dgamma=ga.grad if affine else None, dbeta=be.grad if affine else None)


def check_stats(name, got, r):
    e = {k: rel_l2(x.cpu().reshape(G, -1), w) for k, x, w in zip(("scale", "shift", "mean", "rstd"), got, r["st"])}
    show(name + " statistics", **e)
    assert all(v <= F32_TOL for v in e.values()), e


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("dtype,adtype", PAIRS)
def test_colbn_train_fwd(N, dtype, adtype, M):
    C = 32
    r = head_ref(M, C, adtype, 0)
    h = nan_like((G, M, C), dtype)
    st = [nan_like((G * C,), 0) for _ in range(4)]
    rm, rv = dev(r["rm0"].clone()), dev(r["rv0"].clone())
    N.call("colbn_train_fwd", dtype, adtype, dev(r["a"]).to(tdt(adtype)), dev(r["gamma"]), dev(r["beta"]), rm, rv, 0.1, EPS, 1, G, M, C,
           h, *st)
    torch.cuda.synchronize()
    check_stats(f"colbn_train_fwd {dtype}{adtype} M={M}", st, r)
    e = dict(h=rel_l2(h.float().cpu(), r["h"]), rm=rel_l2(rm.cpu(), r["rm"]), rv=rel_l2(rv.cpu(), r["rv"]))
    show(f"colbn_train_fwd {dtype}{adtype} M={M}", **e)
    assert torch.isfinite(h.float()).all() and e["h"] <= tol_of(dtype) and e["rm"] <= F32_TOL and e["rv"] <= F32_TOL


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("types", TRIPLES)
def test_colbn_bwd_one_launch(N, types, M):
    """M <= 1024: `colbn_bwd` is colbn_bwd_fused_kernel and leaves its scratch alone."""
    dtype, adtype, gdtype = types
    C = 64
    r = head_ref(M, C, adtype, gdtype)
    da = nan_like((G, M, C), dtype)
    tmp = torch.full((2 * G * C,), float("nan"), device="cuda", dtype=torch.float64)
    dg0, db0 = prefill(C, 1), prefill(C, 2)
    dg, db = dev(dg0.clone()), dev(db0.clone())
    N.call("colbn_bwd", dtype, adtype, gdtype, dev(r["a"]).to(tdt(adtype)), dev(r["dh"]).to(tdt(gdtype)),
           *(dev(s.reshape(-1)) for s in r["st"]), 1, G, M, C, tmp, da, dg, db)
    torch.cuda.synchronize()
    e = dict(da=rel_l2(da.float().cpu(), r["da"]), dgamma=rel_l2(dg.cpu().double() - dg0.double(), r["dgamma"]),
             dbeta=rel_l2(db.cpu().double() - db0.double(), r["dbeta"]))
    show(f"colbn_bwd one launch {types} M={M}", **e)
    assert torch.isnan(tmp).all()
    assert torch.isfinite(da.float()).all() and e["da"] <= tol_of(dtype) and e["dgamma"] <= F32_TOL and e["dbeta"] <= F32_TOL


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("adtype,gdtype", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_colbn_multi(N, adtype, gdtype, M):
    """Two layers per launch, bf16 out: problem 0 affine with running buffers and parameter gradients, problem 1 without any."""
    C, vp, adr = 32, ctypes.c_void_p, ctypes.addressof
    rs = [head_ref(M, C, adtype, gdtype, 1, True), head_ref(M, C, adtype, gdtype, 2, False)]
    a = [dev(r["a"]).to(tdt(adtype)) for r in rs]
    h = [nan_like((G, M, C), 1) for _ in rs]
    st = [nan_like((4, G * C), 0) for _ in rs]
    rm, rv, gamma, beta = (dev(rs[0][k].clone()) for k in ("rm0", "rv0", "gamma", "beta"))
    arrs = (harr(vp, a), harr(vp, [gamma, None]), harr(vp, [beta, None]), harr(vp, [rm, None]), harr(vp, [rv, None]), harr(vp, h),
            harr(vp, st))
    N.call("colbn_train_fwd_multi", 2, adtype, *(adr(x) for x in arrs[:5]), 0.1, EPS, 1, G, M, C, adr(arrs[5]), adr(arrs[6]))
    torch.cuda.synchronize()
    for p, r in enumerate(rs):
        check_stats(f"colbn_train_fwd_multi a={adtype} M={M} problem {p}", st[p], r)
        e = rel_l2(h[p].float().cpu(), r["h"])
        show(f"colbn_train_fwd_multi a={adtype} M={M} problem {p}", h=e)
        assert torch.isfinite(h[p].float()).all() and e <= tol_of(1)
    assert rel_l2(rm.cpu(), rs[0]["rm"]) <= F32_TOL and rel_l2(rv.cpu(), rs[0]["rv"]) <= F32_TOL
    dh = [dev(r["dh"]).to(tdt(gdtype)) for r in rs]
    handed = [dev(torch.stack([s.reshape(-1) for s in r["st"]])) for r in rs]
    da = [nan_like((G, M, C), 1) for _ in rs]
    dg0, db0 = prefill(C, 1), prefill(C, 2)
    dg, db = dev(dg0.clone()), dev(db0.clone())
    arrs = (harr(vp, a), harr(vp, dh), harr(vp, handed), harr(vp, da), harr(vp, [dg, None]), harr(vp, [db, None]))
    N.call("colbn_bwd_multi", 2, adtype, gdtype, adr(arrs[0]), adr(arrs[1]), adr(arrs[2]), 1, G, M, C, *(adr(x) for x in arrs[3:]))
    torch.cuda.synchronize()
    e = dict(da0=rel_l2(da[0].float().cpu(), rs[0]["da"]), da1=rel_l2(da[1].float().cpu(), rs[1]["da"]),
             dgamma=rel_l2(dg.cpu().double() - dg0.double(), rs[0]["dgamma"]), dbeta=rel_l2(db.cpu().double() - db0.double(), rs[0]["dbeta"]))
    show(f"colbn_bwd_multi a={adtype} g={gdtype} M={M}", **e)
    assert all(torch.isfinite(x.float()).all() for x in da)
    assert e["da0"] <= tol_of(1) and e["da1"] <= tol_of(1) and e["dgamma"] <= F32_TOL and e["dbeta"] <= F32_TOL


def test_center_cast_multi_16_rows_per_thread(N):
    """520 rows: the <16> instantiation, equal to the single-problem launches bit for bit and within one rounding of fp64."""
    M, Cs, vp, adr = 520, [32, 64], ctypes.c_void_p, ctypes.addressof
    g = torch.Generator().manual_seed(520)
    ys = [dev(torch.rand(G, M, C, generator=g) * 0.3 + 5.0 * torch.rand(C, generator=g)) for C in Cs]
    one = [(nan_like((G, M, C), 1), nan_like((G, C), 0)) for C in Cs]
    for y, (yc, cm), C in zip(ys, one, Cs):
        N.call("center_cast", y, yc, cm, G, M, C)
    ycs, cms = [nan_like((G, M, C), 1) for C in Cs], [nan_like((G, C), 0) for C in Cs]
    arrs = (harr(vp, ys), harr(vp, ycs), harr(vp, cms), harr(ctypes.c_int, Cs))
    N.call("center_cast_multi", 2, *(adr(x) for x in arrs), G, M)
    torch.cuda.synchronize()
    for y, (yc, cm), yc2, cm2 in zip(ys, one, ycs, cms):
        assert torch.equal(yc, yc2) and torch.equal(cm, cm2)
        mu = y.double().mean(1)
        assert rel_l2(cm2.cpu(), mu.cpu()) <= F32_TOL and rel_l2(yc2.float().cpu(), (y.double() - mu[:, None]).cpu()) <= tol_of(1)


# ====================================================================================== 2. conv blocks (csrc/bnpool.hip, conv1.hip)
@pytest.mark.parametrize("want_sq", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1])
def test_colstats(N, dtype, want_sq):
    M, C = 40, 64
    g = torch.Generator().manual_seed(40 + dtype)
    x = (torch.randn(G, M, C, generator=g) * 1.7 + 0.4).to(tdt(dtype))
    s = torch.full((2, G * C), float("nan"), device="cuda", dtype=torch.float64)
    N.call("colstats", dtype, dev(x), G, M, C, C, want_sq, s[0], s[1] if want_sq else None)
    torch.cuda.synchronize()
    x64 = x.double()
    e = dict(sum=rel_l2(s[0].cpu(), x64.sum(1)), sumsq=rel_l2(s[1].cpu(), (x64 * x64).sum(1)) if want_sq else 0.0)
    show(f"colstats {dtype} want_sq={want_sq}", **e)
    assert e["sum"] <= F32_TOL and e["sumsq"] <= F32_TOL
    assert want_sq or torch.isnan(s[1]).all()


@pytest.mark.parametrize("dtype", [0, 1])
def test_pack_conv_w_and_im2col3x3(N, dtype):
    """copies and roundings: Wf [co][tap*64+ci], Wd [ci][tap*64+co] with the taps flipped, col[pix][tap*64+c] with zero padding"""
    g = torch.Generator().manual_seed(9)
    ws = [torch.randn(64, 64, 3, 3, generator=g) * 0.05 for _ in range(2)]
    out = [nan_like((64, 576), dtype) for _ in range(8)]
    for k, w in enumerate(ws):
        N.call("pack_conv_w", dtype, dev(w), out[2 * k], out[2 * k + 1])
    N.call("pack_conv_w2", dtype, dev(ws[0]), out[4], out[5], dev(ws[1]), out[6], out[7])
    Nimg, Ti, Fi = 2, 3, 4
    X = torch.randn(Nimg, Ti, Fi, 64, generator=g).to(tdt(dtype))
    col = nan_like((Nimg * Ti * Fi, 576), dtype)
    N.call("im2col3x3", dtype, dev(X), col, Nimg, Ti, Fi)
    torch.cuda.synchronize()
    for k, w in enumerate(ws):
        taps = w.reshape(64, 64, 9)                                      # [co][ci][tap]
        Wf = taps.permute(0, 2, 1).reshape(64, 576).to(tdt(dtype))
        Wd = taps.flip(2).permute(1, 2, 0).reshape(64, 576).to(tdt(dtype))
        for got in (out[2 * k], out[4 + 2 * k]):
            assert torch.equal(got.cpu(), Wf)
        for got in (out[2 * k + 1], out[5 + 2 * k]):
            assert torch.equal(got.cpu(), Wd)
    pad = torch.zeros(Nimg, Ti + 2, Fi + 2, 64, dtype=X.dtype)
    pad[:, 1:-1, 1:-1] = X
    want = torch.stack([pad[:, kw:kw + Ti, kh:kh + Fi] for kh in range(3) for kw in range(3)], 3)         # [n][t][f][tap][c]
    assert torch.equal(col.cpu(), want.reshape(Nimg * Ti * Fi, 576))


def test_conv1_bwd_valu_kernel_with_bf16_gradients(N):
    """conv_dtype 0 with dtype 1: conv1_bwd_kernel<bf16> reads dP AND dxl as bf16 (the MFMA flavour keeps dxl in fp32)."""
    shape = (3, 32, 11)
    r = stem_ref(shape, False, 1)
    img, par, st, mom, _ = stem_forward(N, r, shape, 0)
    got = stem_bwd(N, shape, 0, img, par, st, mom, dev(r["dP"]).bfloat16(), dev(r["dxl"]).bfloat16(), dp_dtype=1)
    e = {k: rel_l2(x, r[k]) for x, k in zip(got, ("dW", "dgamma", "dbeta"))}
    show("conv1_bwd flavour 0, bf16 gradients", **e)
    assert all(v <= F32_TOL for v in e.values()), e


# ====================================================================================== 3. losses and the MoCo head
@pytest.mark.parametrize("dtype", [0, 1])
def test_barlow_loss(N, dtype):
    D, coef, dscale = 64, 5e-3, 0.25
    g = torch.Generator().manual_seed(64)
    c = torch.randn(D, D, generator=g) * 0.2 + torch.eye(D) * 0.9
    dc = nan_like((D, D), dtype)
    loss = dev(torch.tensor([0.375]))
    N.call("barlow_loss", dtype, dev(c), D, coef, dscale, dc, loss)
    torch.cuda.synchronize()
    d = c.double() - torch.eye(D, dtype=torch.float64)
    e = dict(loss=scalar_err(loss.item() - 0.375, coef * (d * d).sum()), dc=rel_l2(dc.float().cpu(), dscale * d))
    show(f"barlow_loss {dtype}", **e)
    assert torch.isfinite(dc.float()).all() and e["loss"] <= F32_TOL and e["dc"] <= tol_of(dtype)


@pytest.mark.parametrize("dtype", [0, 1])
def test_moco_head_rows(N, dtype):
    """l2norm_fwd, moco_prep and l2norm_bwd (B = 3, D = 128) against fp64 autograd; moco_ce_bwd on its scalar path (K = 300,
    K % 8 != 0) and its vector path (K = 304)."""
    B, D, scale = 3, 128, 5.0
    g = torch.Generator().manual_seed(128)
    q32, k32 = torch.randn(B, D, generator=g) * 3, torch.randn(B, D, generator=g)
    dqn, dlpos = torch.randn(B, D, generator=g), torch.randn(B, generator=g)
    q = q32.double().requires_grad_(True)
    qn, kn = q / q.norm(dim=1, keepdim=True), k32.double() / k32.double().norm(dim=1, keepdim=True)
    ((qn * dqn.double()).sum() + ((qn * kn).sum(1) * dlpos.double()).sum()).backward()
    o = [nan_like((B, D), dtype), nan_like((B, D), 0), nan_like((B,), 0)]
    N.call("l2norm_fwd", dtype, dev(q32), B, D, *o)
    p = [nan_like((B, D), dtype), nan_like((B, D), 0), nan_like((B,), 0), nan_like((B, D), dtype), nan_like((B, D), 0), nan_like((B,), 0),
         nan_like((B,), 0)]
    N.call("moco_prep", dtype, dev(q32), dev(k32), B, D, scale, *p)
    dq = nan_like((B, D), dtype)
    inv = (1.0 / q.detach().norm(dim=1)).float()
    N.call("l2norm_bwd", dtype, dev(dqn), dev(dlpos), dev(kn.float()), dev(qn.detach().float()), dev(inv), B, D, dq)
    torch.cuda.synchronize()
    for u, v in zip(o, p[:3]):
        assert torch.equal(u, v)
    assert torch.equal(p[0].float(), p[1].to(tdt(dtype)).float()) and torch.equal(p[3].float(), p[4].to(tdt(dtype)).float())
    e = dict(qn=rel_l2(p[1].cpu(), qn.detach()), kn=rel_l2(p[4].cpu(), kn), qinv=rel_l2(p[2].cpu(), inv.double()),
             lpos=rel_l2(p[6].cpu(), (qn.detach() * kn).sum(1) * scale), dq=rel_l2(dq.float().cpu(), q.grad))
    show(f"moco head {dtype}", **e)
    assert all(e[k] <= F32_TOL for k in ("qn", "kn", "qinv", "lpos")) and e["dq"] <= tol_of(dtype)
    for K in (300, 304):
        Bc, gscale = 4, 0.25
        lpos, lneg = torch.randn(Bc, generator=g), torch.randn(Bc, K, generator=g)
        lse = torch.logsumexp(torch.cat([lpos[:, None], lneg], 1).double(), 1).float()
        P, dl = nan_like((Bc, K), dtype), nan_like((Bc,), 0)
        N.call("moco_ce_bwd", dtype, dev(lpos), dev(lneg), dev(lse), Bc, K, gscale, P, dl)
        torch.cuda.synchronize()
        e = dict(P=rel_l2(P.float().cpu(), torch.exp(lneg.double() - lse.double()[:, None]) * gscale),
                 dlpos=rel_l2(dl.cpu(), (torch.exp(lpos.double() - lse.double()) - 1) * gscale))
        show(f"moco_ce_bwd {dtype} K={K}", **e)
        assert torch.isfinite(P.float()).all() and e["P"] <= tol_of(dtype) and e["dlpos"] <= F32_TOL


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("dtype", [0, 1])
def test_enqueue(N, dtype, on_device):
    """queue[:, ptr:ptr+B] = keys^T in the fp32 master and its shadow copy; the write position from the host or from the device"""
    B, D, K, ptr = 3, 70, 10, 4                                              # B * D = 210: one partial workgroup
    g = torch.Generator().manual_seed(70)
    keys, q0 = torch.randn(B, D, generator=g), torch.randn(D, K, generator=g)
    queue, shadow = dev(q0.clone()), dev(q0.to(tdt(dtype)))
    pd = dev(torch.tensor([ptr], dtype=torch.int64)) if on_device else None
    N.call("enqueue", dtype, dev(keys), B, D, K, -1 if on_device else ptr, pd, queue, shadow)
    torch.cuda.synchronize()
    want = q0.clone()
    want[:, ptr:ptr + B] = keys.T
    assert torch.equal(queue.cpu(), want) and torch.equal(shadow.cpu(), want.to(tdt(dtype)))
    assert pd is None or int(pd.item()) == (ptr + B) % K


@pytest.mark.parametrize("dtype", [0, 1])
def test_cast_cast_back_relu_bwd(N, dtype):
    """n = 8 * 33 ends inside a workgroup; a destination 4 (2) bytes past a 16-byte boundary takes `cast` off its vector path"""
    n = 8 * 33
    g = torch.Generator().manual_seed(33)
    src = torch.randn(n, generator=g)
    for off in (0, 1):
        dst = nan_like((n + 8,), dtype)
        N.call("cast", dtype, dev(src), dst[off:off + n], n)
        torch.cuda.synchronize()
        assert torch.equal(dst[off:off + n].cpu(), src.to(tdt(dtype))) and torch.isnan(dst[off + n:].float()).all()
    stored = src.to(tdt(dtype))
    back = nan_like((n,), 0)
    N.call("cast_back", dtype, dev(stored), back, n)
    h = torch.relu(torch.randn(n, generator=g)).to(tdt(dtype))                # a ReLU output: zeros where the gate is closed
    h[::7] = -h[::7] - 0.5                                                   # relu_bwd also takes a pre-activation
    assert float(h.float()[h != 0].abs().min()) >= 1e-6
    out = nan_like((n,), dtype)
    N.call("relu_bwd", dtype, dev(stored), dev(h), out, n)
    torch.cuda.synchronize()
    assert torch.equal(back.cpu(), stored.float())
    assert torch.equal(out.cpu(), torch.where(h > 0, stored, torch.zeros_like(stored)))


@pytest.mark.parametrize("dtype", [0, 1])
def test_ntxent_bwd_and_ce_rows(N, dtype):
    """300 columns: a second 256-thread sweep (ce_rows) / a second workgroup per row (ntxent_bwd) with 44 live threads"""
    g = torch.Generator().manual_seed(300)
    Nr, B, gscale = 300, 4, 0.125
    sim = torch.randn(Nr, Nr, generator=g)
    off = ~torch.eye(Nr, dtype=torch.bool)
    lse = torch.logsumexp(sim.double().masked_fill(~off, float("-inf")), 1).float()
    dsim = nan_like((Nr, Nr), dtype)
    N.call("ntxent_bwd", dtype, dev(sim), dev(lse), Nr, B, gscale, dsim)
    pos = torch.zeros(Nr, Nr, dtype=torch.float64)
    pos[torch.arange(Nr), (torch.arange(Nr) + B) % Nr] = 1.0
    want = (torch.exp(sim.double() - lse.double()[:, None]) - pos) * gscale * off
    Bc, K, ignore = 4, 300, -100
    logits = torch.randn(Bc, K, generator=g) * 2
    target = torch.tensor([7, ignore, 299, 256])
    x = logits.double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(x, target, ignore_index=ignore)
    ce.backward()
    outs = []
    for with_grad in (True, False):
        cnt = dev(torch.tensor([12345], dtype=torch.int32))
        loss = dev(torch.tensor([0.375]))
        dl = nan_like((Bc, K), dtype) if with_grad else None
        N.call("ce_rows", dtype, dev(logits), dev(target), Bc, K, ignore, cnt, loss, dl)
        outs.append((cnt, loss, dl))
    torch.cuda.synchronize()
    e = dict(dsim=rel_l2(dsim.float().cpu(), want), loss=scalar_err(outs[0][1].item() - 0.375, ce.item()),
             loss_fwd_only=scalar_err(outs[1][1].item() - 0.375, ce.item()), dlogits=rel_l2(outs[0][2].float().cpu(), x.grad))
    show(f"ntxent_bwd / ce_rows {dtype}", **e)
    assert torch.isfinite(dsim.float()).all() and float(dsim.float().diagonal().abs().max()) == 0.0 and e["dsim"] <= tol_of(dtype)
    assert int(outs[0][0].item()) == 3 and int(outs[1][0].item()) == 3
    assert e["loss"] <= F32_TOL and e["loss_fwd_only"] <= F32_TOL and e["dlogits"] <= tol_of(dtype)
    assert float(outs[0][2][1].float().abs().max()) == 0.0                   # the ignored row
