"""CPU: the references, emulations and inputs of tests/vit_ref.py (what tests/test_gpu_vit_kernels.py compares the transformer
kernels with) checked against torch's own fp64 operators, and the properties the input families are chosen for."""
import math

import pytest
import torch

import vit_ref as R


def show(name, **figures):
    print(name, " ".join(f"{k}={v:.3e}" for k, v in figures.items()))


# ------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("family,B,H,S", [("plain", 2, 2, 33), ("offset", 2, 2, 129), ("peaked", 2, 2, 128), ("plain", 3, 5, 37), ("plain", 2, 2, 1)])
def test_attention64_matches_autograd(family, B, H, S):
    qkv, dout = R.attn_inputs(family, B, S, H)
    ref = R.attention64(qkv, dout, B, S, H)
    C = H * 64
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, i * C:(i + 1) * C].view(B, S, H, 64).permute(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * R.SCALE
    out = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B * S, C)
    out.backward(dout.double())
    figs = dict(out=R.rel_all(ref["out"], out.detach()), lse=R.rel_all(ref["lse"], torch.logsumexp(s, -1).reshape(B * H, S).detach()))
    for i, n in enumerate(("dq", "dk", "dv")):
        figs[n] = R.rel_all(ref[n], x.grad[:, i * C:(i + 1) * C])
    show(f"attention64 {family} B{B} H{H} S{S}", **figs)
    assert max(figs.values()) <= 1e-12, figs


@pytest.mark.parametrize("family,B,H,S", R.ATTN_CASES)
def test_attention_emulation_stays_under_the_cap(family, B, H, S):
    """the reference's own figure for every case of the GPU matrix: the kernels are allowed ATTN_MARGIN x these, so they must
    stay small enough that the allowance is far from the 100 % of a wrong row"""
    qkv, dout, ref, fig = R.attn_case(family, B, S, H)
    assert torch.equal(qkv.float().bfloat16(), qkv) and qkv.shape == (B * S, 3 * H * 64) and dout.shape == (B * S, H * 64)
    for n, (row, head, whole) in fig.items():
        show(f"attention_emulated {family} B{B} H{H} S{S} {n}", row=row, row_head=head, all=whole)
        assert row <= R.ATTN_EMU_ROW_CAP and head <= R.ATTN_EMU_HEAD_CAP and whole <= R.ATTN_EMU_ALL_CAP, (n, row, head, whole)
        assert R.ATTN_MARGIN * max(row, head) < 0.25
    if S > 1:
        assert min(fig[n][2] for n in fig) > 0.0                 # the roundings are really in


@pytest.mark.parametrize("S", R.ATTN_ALL_FAMILIES_AT)
def test_attention_offset_family_needs_the_max_subtraction(S):
    """every score is 100 + noise: exp(score) overflows fp32 (exp(88.7) is the largest finite value).  Soft-max ignores a constant
    added to a row, and the constant here is exactly scale * 40 * 20 = 100 in place of the column-0 product: the probabilities
    are those of the plain draw with column 0 of q taken out, to fp64 rounding of scores near 100"""
    B = H = 2
    C = H * 64
    qo, _ = R.attn_inputs("offset", B, S, H)
    qp, _ = R.attn_inputs("plain", B, S, H)
    so = R.attn_scores(qo, B, S, H)
    assert float(so.min()) > 89.0
    assert not bool(torch.isfinite(torch.exp(so.float())).any())
    q0 = qp.float().clone()
    q0[:, 0:C:64] = 0.0
    sp = R.attn_scores(q0, B, S, H)
    diff = float((torch.softmax(so, -1) - torch.softmax(sp, -1)).abs().max())
    show(f"offset S{S}", min_score=float(so.min()), softmax_diff=diff)
    assert diff < 1e-9


@pytest.mark.parametrize("S", R.ATTN_ALL_FAMILIES_AT)
def test_attention_peaked_family_is_peaked(S):
    """q and k doubled: a few keys carry each row (mean row maximum of P above 0.3), and for S > 128 the running maximum of
    sweep 1 rises at a later key block on a good part of the rows, by more than one unit on average - a sum that is not
    rescaled by exp(m - mn) there is off by a factor of e or more"""
    B = H = 2
    qkv, _ = R.attn_inputs("peaked", B, S, H)
    s = R.attn_scores(qkv, B, S, H)
    P = torch.softmax(s, -1)
    mean_max = float(P.max(-1).values.mean())
    show(f"peaked S{S}", max_abs_score=float(s.abs().max()), mean_row_max_P=mean_max)
    assert mean_max > 0.3
    assert 10.0 < float(s.abs().max()) < 20.0
    if S > R.SP:
        nb = -(-S // R.SP)
        bm = torch.stack([s[..., kb * R.SP:(kb + 1) * R.SP].max(-1).values for kb in range(nb)], -1)       # [B][H][S][nb]
        run = torch.cummax(bm, -1).values
        rise = (run[..., 1:] - run[..., :-1]).sum(-1)              # total rise of the running maximum after block 0
        spread = float((bm.max(-1).values - bm.min(-1).values).mean())
        frac = float((rise > 0).float().mean())
        mean_rise = float(rise[rise > 0].mean())
        show(f"peaked S{S} blocks", spread=spread, rows_rising=frac, mean_rise=mean_rise)
        assert spread > 2.0                                      # block maxima differ by several units
        if nb * R.SP - S < R.SP // 2:                            # a last block of one key rarely holds the row maximum
            assert frac > 0.25 and mean_rise > 1.0


# ------------------------------------------------------------------------------------------------------ LayerNorm
def test_layernorm_inputs_and_reference():
    x, gamma, beta, dy, base = R.ln_inputs(9, 40)
    assert float(gamma.min()) < 0 and int((gamma == 0).sum()) == 1
    assert abs(float(x.mean()) - 0.5) < 0.2 and float(x.min()) >= -1.5 and float(x.max()) <= 2.5
    xo = R.ln_inputs(9, 40, 100.0)[0]
    assert float(xo.min()) >= 98.0 and float(xo.max()) <= 102.0
    r = R.ln_ref64(9, 40)
    xd = x.double()
    xh = (xd - r["mean"][:, None]) * r["rstd"][:, None]
    assert R.rel_all(xh * gamma.double() + beta.double(), r["y"]) < 1e-13
    g = dy.double() * gamma.double()
    dx = r["rstd"][:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    assert R.rel_all(dx, r["dx"]) < 1e-12
    assert R.rel_all((dy.double() * xh).sum(0), r["dgamma"]) < 1e-12 and R.rel_all(dy.double().sum(0), r["dbeta"]) < 1e-12


@pytest.mark.parametrize("C", R.LN_C_VEC + R.LN_C_SCALAR)
def test_layernorm_base_family_leaves_room_under_the_bounds(C):
    """the kernels' arithmetic (fp32, two passes, lane-strided sums) on the very inputs of the GPU matrix: per-row y32 <= 1e-6,
    mean rtol 1e-5 / atol 1e-6, rstd rtol 1e-5 and per-row dres - base <= 1e-5 must hold for it with room (0.7 of the bound at
    the worst, C = 3, see vit_ref.LN_SEED; 0.2 from C = 40 on), so that a failure on the GPU is the kernel's"""
    worst = dict(y32=0.0, mean=0.0, rstd=0.0, dres=0.0)
    for M in R.LN_M:
        x, gamma, beta, dy, base = R.ln_inputs(M, C)
        ref = R.ln_ref64(M, C)
        y, mu, rs = R.layernorm_fp32(x, gamma, beta)
        dres = R.layernorm_bwd_fp32(x, gamma, dy, base, mu, rs)
        worst["y32"] = max(worst["y32"], R.rel_rows(y, ref["y"]))
        worst["mean"] = max(worst["mean"], float(((mu.double() - ref["mean"]).abs() / (1e-5 * ref["mean"].abs() + 1e-6)).max()))
        worst["rstd"] = max(worst["rstd"], float(((rs.double() - ref["rstd"]).abs() / ref["rstd"]).max()))
        worst["dres"] = max(worst["dres"], R.rel_rows(dres.double() - base.double(), ref["dx"]))
    show(f"layernorm_fp32 base C{C}", **worst)
    room = 0.7 if C < 40 else 0.2
    assert worst["y32"] <= room * 1e-6 and worst["mean"] <= 0.5 and worst["rstd"] <= 5e-6 and worst["dres"] <= room * 1e-5, worst


@pytest.mark.parametrize("C", R.LN_OFFSET_C)
def test_layernorm_offset_family_separates_two_pass_from_one_pass(C):
    """x = uniform +-2 + 100: the 1e-4 bound of the GPU test sits between the two-pass form the kernels have and the one-pass
    E[x^2] - E[x]^2 form, which loses 100^2 / var ~ 1e4 of its fp32 digits"""
    for M in R.LN_OFFSET_M:
        x, gamma, beta, _, _ = R.ln_inputs(M, C, 100.0)
        ref = R.ln_ref64(M, C, 100.0)
        y2, _, rs2 = R.layernorm_fp32(x, gamma, beta)
        y1, _, rs1 = R.layernorm_fp32(x, gamma, beta, one_pass=True)
        two, one = R.rel_rows(y2, ref["y"]), R.rel_rows(y1, ref["y"])
        show(f"layernorm_fp32 offset M{M} C{C}", two_pass=two, one_pass=one,
             rstd_two=float(((rs2.double() - ref["rstd"]).abs() / ref["rstd"]).max()),
             rstd_one=float(((rs1.double() - ref["rstd"]).abs() / ref["rstd"]).max()))
        assert two <= 2.5e-5 and one >= 4e-4, (M, C, two, one)


# ------------------------------------------------------------------------------------------------------ GELU
def test_gelu_reference():
    x = R.all_finite_bf16()
    xf = x.float()
    assert x.numel() % 8 == 0 and bool(torch.isfinite(xf).all()) and xf.unique().numel() == 65280 - 1       # +0 and -0 compare equal
    y, d = R.gelu64(x), R.gelu_grad64(x)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(d).all())
    mid = xf.abs() <= 6
    xm = x.double()[mid].requires_grad_(True)
    t = torch.nn.functional.gelu(xm)
    t.backward(torch.ones_like(t))
    assert float((y[mid] - t.detach()).abs().max()) < 1e-15 and float((d[mid] - xm.grad).abs().max()) < 1e-14
    big = xf >= 8
    assert torch.equal(R.bf16r(y[big]), x.double()[big])          # Phi(8) = 1 - 6e-16: x itself once stored as bf16
    assert float(y[xf <= -8].abs().max()) < 1e-13 and float(d[xf <= -8].abs().max()) < 1e-12
    assert float(y[xf == -5.0][0]) == pytest.approx(-5 * 2.866515718791939e-07, rel=1e-9)


# ------------------------------------------------------------------------------------------------------ patch_unfold, tile_rows
@pytest.mark.parametrize("F,T,fs,ts", R.PATCH_CASES)
def test_patch_unfold_reference_is_the_conv2d_operand(F, T, fs, ts):
    B = 3
    g = torch.Generator().manual_seed(500 + F)
    x = (torch.rand(B, F, T, generator=g) * 2 - 1).bfloat16().float()           # bf16-exact: the rounding drops out
    w = torch.rand(5, 1, 16, 16, generator=g).double()
    nf, nt = R.patch_grid(F, T, fs, ts)
    conv = torch.nn.functional.conv2d(x[:, None].double(), w, stride=(fs, ts))
    assert tuple(conv.shape[2:]) == (nf, nt)
    rows = R.patch_unfold_ref(x, fs, ts)
    assert rows.shape == (B * nf * nt, 256) and rows.dtype == torch.bfloat16
    want = conv.flatten(2).transpose(1, 2).reshape(B * nf * nt, 5)
    assert R.rel_all(rows.double() @ w.view(5, 256).T, want) < 1e-14


def test_tile_rows_reference():
    src = torch.arange(12.0).reshape(3, 4)
    assert torch.equal(R.tile_rows_ref(src, 6, 3, 1, 1.0), torch.cat([src, src]))
    got = R.tile_rows_ref(src, 6, 3, 2, 0.5)
    assert torch.equal(got, 0.5 * src[[0, 0, 1, 1, 2, 2]])
    x = torch.rand(2, 7, 4, dtype=torch.float64, requires_grad=True)             # token-mean backward: dpooled / Ntok on every token
    dp = torch.rand(2, 4)
    x.mean(1).backward(dp.double())
    assert torch.allclose(R.tile_rows_ref(dp, 14, 2, 7, 1.0 / 7).double(), x.grad.reshape(14, 4), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("n,t0,gscale", [c for c in R.ADAMW_CASES if c[0] <= 4003])
def test_adamw64_matches_torch_optim(n, t0, gscale):
    hp = {k: R.f32(v) for k, v in R.ADAMW_HP.items()}
    p0, grads, m0, v0 = R.adamw_inputs(n, t0)
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    if t0 != 1:
        opt.state[p] = dict(step=torch.tensor(float(t0 - 1)), exp_avg=m0.double().clone(), exp_avg_sq=v0.double().clone())
    for g in grads:
        p.grad = g.double() * gscale
        opt.step()
    rp, rm, rv = R.adamw_ref(n, t0, gscale)
    st = opt.state[p]
    assert float(st["step"]) == t0 + 2
    figs = dict(p=R.rel_all(rp, p.detach()), m=R.rel_all(rm, st["exp_avg"]), v=R.rel_all(rv, st["exp_avg_sq"]))
    show(f"adamw64 n{n} t0={t0} gscale={gscale}", **figs)
    assert max(figs.values()) < 1e-13
    assert not torch.equal(rp.float(), p0)
    assert math.isclose(hp["b2"], 0.999, rel_tol=1e-7) and hp["b2"] != 0.999      # the fp32 value the kernel is handed, not 0.999
