"""GPU: every kernel and instantiation of the transformer path (csrc/attention.hip, csrc/vit.hip) through the C ABI against the
fp64 references of tests/vit_ref.py, at the row, wave and tile edges where such kernels go wrong.

Conventions (those of test_gpu_bn_chain.py):
  * references are fp64 on the inputs as stored (bf16 tensors are rounded first, then cast to fp64);
  * outputs documented as written start as NaN, accumulated ones (dgamma, dbeta) from `prefill` values, and every test asserts
    that all of them are finite afterwards;
  * every measured error goes through `show`, so `pytest -s` lists it.
Guard rows: every device tensor a kernel reads or writes is a contiguous slice of a larger buffer (`Buf`) with at least 128 rows
on each side; the slice starts 16-byte aligned unless the case is about misalignment.  Guards of pure inputs hold NaN (a read
that escapes a mask poisons an output), guards of written tensors hold 512.0 and must be bit-identical after the call.  A
tensor one kernel writes and the next one reads (out, lse, mean, rstd) is copied between NaN guards for the second call.

Attention.  `vit_ref.attention_emulated` is attention64 with the kernels' bf16 roundings; its per-row rel-L2 against attention64
is the reference's own figure of a case, and the kernels must stay within 4 x that figure per token row and per (row, head) -
the emulation leaves out fp32 accumulation order, __expf and __logf - and within the whole-tensor 1e-2 (out) / 2e-2 (gradients)
of test_gpu_vit.py.  A (row, head) segment is measured against its own norm or a quarter of the mean segment norm, whichever is
larger (vit_ref.rel_rows: a one-hot soft-max row has no dq / dk to speak of); whole rows are not floored.  Worst per-row figures over (out, dq, dk, dv), emulation | kernels as measured on an MI355X, B = H = 2
unless (B, H, S) is given:
  plain  S = 1       out 0.0e+00 | 0.0e+00 dq 0.0e+00 | 0.0e+00 dk 0.0e+00 | 0.0e+00 dv 0.0e+00 | 0.0e+00 (row, head) 0.0e+00 | 0.0e+00
  plain  S = 31      out 2.9e-03 | 2.9e-03 dq 3.1e-03 | 3.1e-03 dk 3.0e-03 | 3.0e-03 dv 2.9e-03 | 2.9e-03 (row, head) 3.6e-03 | 3.6e-03
  plain  S = 32      out 2.5e-03 | 2.5e-03 dq 3.1e-03 | 3.1e-03 dk 3.0e-03 | 3.0e-03 dv 2.9e-03 | 2.9e-03 (row, head) 3.6e-03 | 3.6e-03
  plain  S = 33      out 2.8e-03 | 2.8e-03 dq 3.0e-03 | 3.0e-03 dk 2.9e-03 | 2.9e-03 dv 2.9e-03 | 2.9e-03 (row, head) 3.7e-03 | 3.7e-03
  offset S = 33      out 2.5e-03 | 2.5e-03 dq 1.0e-02 | 1.0e-02 dk 8.9e-03 | 8.9e-03 dv 3.0e-03 | 3.0e-03 (row, head) 1.8e-02 | 1.8e-02
  peaked S = 33      out 2.2e-03 | 2.2e-03 dq 3.4e-03 | 3.4e-03 dk 3.4e-03 | 3.4e-03 dv 3.0e-03 | 3.0e-03 (row, head) 3.9e-03 | 3.9e-03
  plain  S = 64      out 2.7e-03 | 2.7e-03 dq 3.2e-03 | 3.2e-03 dk 3.2e-03 | 3.2e-03 dv 3.4e-03 | 3.4e-03 (row, head) 4.3e-03 | 4.3e-03
  plain  S = 96      out 2.8e-03 | 2.8e-03 dq 2.9e-03 | 2.9e-03 dk 3.0e-03 | 3.0e-03 dv 3.0e-03 | 3.0e-03 (row, head) 3.3e-03 | 3.3e-03
  plain  S = 127     out 2.8e-03 | 2.8e-03 dq 2.9e-03 | 2.9e-03 dk 2.9e-03 | 2.9e-03 dv 3.0e-03 | 3.0e-03 (row, head) 3.4e-03 | 3.4e-03
  plain  S = 128     out 2.7e-03 | 2.7e-03 dq 3.2e-03 | 3.2e-03 dk 3.3e-03 | 3.3e-03 dv 3.1e-03 | 3.1e-03 (row, head) 3.8e-03 | 3.8e-03
  offset S = 128     out 2.8e-03 | 2.8e-03 dq 1.1e-02 | 1.1e-02 dk 1.4e-02 | 1.4e-02 dv 2.9e-03 | 2.9e-03 (row, head) 1.7e-02 | 1.7e-02
  peaked S = 128     out 2.4e-03 | 2.4e-03 dq 3.8e-03 | 3.8e-03 dk 3.4e-03 | 3.4e-03 dv 3.7e-03 | 3.7e-03 (row, head) 4.1e-03 | 4.1e-03
  plain  S = 129     out 2.9e-03 | 2.9e-03 dq 3.1e-03 | 3.1e-03 dk 3.1e-03 | 3.1e-03 dv 2.7e-03 | 2.7e-03 (row, head) 3.5e-03 | 3.5e-03
  offset S = 129     out 2.9e-03 | 2.9e-03 dq 2.3e-02 | 2.3e-02 dk 1.2e-02 | 1.2e-02 dv 2.9e-03 | 2.9e-03 (row, head) 3.2e-02 | 3.2e-02
  peaked S = 129     out 3.3e-03 | 3.3e-03 dq 1.6e-02 | 1.6e-02 dk 1.4e-02 | 1.4e-02 dv 4.3e-03 | 4.3e-03 (row, head) 4.7e-02 | 4.7e-02
  plain  S = 160     out 2.8e-03 | 2.8e-03 dq 3.1e-03 | 3.1e-03 dk 3.1e-03 | 3.1e-03 dv 3.1e-03 | 3.1e-03 (row, head) 3.7e-03 | 3.7e-03
  plain  S = 255     out 2.9e-03 | 2.9e-03 dq 3.1e-03 | 3.1e-03 dk 3.0e-03 | 3.0e-03 dv 3.2e-03 | 3.2e-03 (row, head) 3.7e-03 | 3.6e-03
  plain  S = 256     out 3.0e-03 | 3.0e-03 dq 3.1e-03 | 3.1e-03 dk 3.1e-03 | 3.1e-03 dv 3.1e-03 | 3.1e-03 (row, head) 3.8e-03 | 3.8e-03
  plain  S = 257     out 2.9e-03 | 2.9e-03 dq 3.2e-03 | 3.2e-03 dk 3.2e-03 | 3.2e-03 dv 3.0e-03 | 3.0e-03 (row, head) 3.8e-03 | 3.8e-03
  offset S = 257     out 3.1e-03 | 3.1e-03 dq 2.3e-02 | 2.3e-02 dk 1.6e-02 | 1.6e-02 dv 2.8e-03 | 2.9e-03 (row, head) 3.4e-02 | 3.4e-02
  peaked S = 257     out 4.1e-03 | 4.1e-03 dq 1.7e-02 | 1.7e-02 dk 1.4e-02 | 1.4e-02 dv 3.8e-03 | 3.8e-03 (row, head) 4.8e-02 | 4.8e-02
  plain  S = 385     out 3.0e-03 | 3.0e-03 dq 3.2e-03 | 3.2e-03 dk 3.2e-03 | 3.2e-03 dv 3.0e-03 | 3.0e-03 (row, head) 3.6e-03 | 3.6e-03
  plain  (3, 5, 37)  out 2.6e-03 | 2.6e-03 dq 3.0e-03 | 3.0e-03 dk 3.0e-03 | 3.0e-03 dv 2.8e-03 | 2.8e-03 (row, head) 4.2e-03 | 4.2e-03
  plain  (1, 3, 300) out 2.8e-03 | 2.8e-03 dq 2.9e-03 | 2.9e-03 dk 2.9e-03 | 2.9e-03 dv 2.9e-03 | 2.9e-03 (row, head) 3.7e-03 | 3.7e-03
  (S = 1 is exact on both sides.  lse: worst |error| 9.0e-7 in the plain family, 5.9e-6 over all cases.)

LayerNorm.  Which kernel a case ran follows from the dispatch rule of audiossl_layernorm_fwd / _bwd, which nothing reports at
run time: the 16-byte `_vec` kernels run iff C % 4 == 0 and x, gamma, beta (and y32, when given) are 16-byte aligned and y is
8-byte aligned (forward), or dy, x, dres and gamma are 16-byte aligned (backward), with NV = ceil(C / 256) float4 chunks per
lane; any other call runs the scalar one-dword-per-lane kernels.  So C in LN_C_VEC on aligned slices covers the eight vec
instantiations (NV = 1: 4, 40, 256; NV = 2: 260, 384, 512; NV = 3: 516, 768; NV = 4: 772, 1024), C in LN_C_SCALAR the scalar
pair through C % 4 != 0, and C = 768 with x (forward) / dy (backward) one float into its buffer the scalar pair through alignment.
Offset family (x = uniform +-2 + 100), worst per-row rel-L2 of y32: fp32 two-pass emulation | one-pass emulation | kernel as
measured on an MI355X (bound 1e-4):
  M = 9   C = 40    5.8e-06 | 6.4e-04 | 5.8e-06    (kernel: rstd 7.7e-08, dres - base per row 1.0e-06)
  M = 65  C = 40    8.4e-06 | 8.1e-04 | 8.4e-06    (kernel: rstd 9.8e-08, dres - base per row 4.7e-06)
  M = 9   C = 384   7.9e-06 | 8.9e-04 | 7.9e-06    (kernel: rstd 4.8e-08, dres - base per row 7.2e-07)
  M = 65  C = 384   1.1e-05 | 1.1e-03 | 1.1e-05    (kernel: rstd 8.9e-08, dres - base per row 8.4e-07)
  M = 9   C = 768   7.5e-06 | 7.6e-04 | 7.5e-06    (kernel: rstd 7.7e-08, dres - base per row 7.9e-07)
  M = 65  C = 768   1.2e-05 | 1.2e-03 | 1.2e-05    (kernel: rstd 7.1e-08, dres - base per row 1.1e-06)
  M = 9   C = 1023  4.9e-06 | 7.9e-04 | 4.9e-06    (kernel: rstd 5.8e-08, dres - base per row 2.7e-07)
  M = 65  C = 1023  9.0e-06 | 8.3e-04 | 9.0e-06    (kernel: rstd 9.0e-08, dres - base per row 3.7e-07)

GELU, all 65,280 finite bf16 inputs, worst element in units of the bound 2^-8 |ref| + 1e-6, as measured on an MI355X:
  gelu_fwd               0.967 at x = 2.078    (0.5 ulp of bf16 at the bottom of a binade is 2^-8 |ref|: the rounding itself)
  gelu_bwd, dh = 1       0.993 at x = 2.44e-3
  gelu_bwd, dh uniform   0.972 at x = -0.201"""
import functools

import numpy as np
import pytest
import torch

import vit_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 512.0
GUARD = 128
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def N():
    from src import _native
    _native.lib()
    assert torch.cuda.is_available()
    return _native


def prefill(n, k=0):
    """non-zero start values of an accumulated output"""
    return torch.linspace(-1.0, 1.0, n) * (1.0 + 0.25 * k) + 0.125


def show(name, **figures):
    print(name, " ".join(f"{k}={v:.3e}" for k, v in figures.items()))


class Buf:
    """`body` (a CPU tensor) as a contiguous slice `.t` of a device buffer with GUARD rows of `guard` on each side (a row is the
    last dimension; 1-D tensors get GUARD elements).  shift: elements by which the slice is moved off its 16-byte alignment."""

    def __init__(self, body, guard, shift=0):
        body = body.contiguous()
        row = body.shape[-1] if body.dim() > 1 else 1
        pad = GUARD * row
        assert (pad * body.element_size()) % 16 == 0
        flat = torch.full((2 * pad + shift + body.numel(),), guard, dtype=body.dtype)
        self.lo, self.hi = pad + shift, pad + shift + body.numel()
        flat[self.lo:self.hi] = body.flatten()
        self.flat = flat.cuda()
        self.t = self.flat[self.lo:self.hi].view(body.shape)
        self.guard = guard
        assert self.t.is_contiguous() and (self.t.data_ptr() % 16 == 0) == (shift * body.element_size() % 16 == 0)

    @classmethod
    def out(cls, shape, dtype, shift=0):
        """a written output: NaN inside, SENTINEL around"""
        return cls(torch.full(shape, NAN, dtype=dtype), SENTINEL, shift)

    def cpu(self):
        return self.t.cpu()

    def check(self, name):
        """guards bit-identical, everything inside finite"""
        flat = self.flat.cpu()
        g = torch.cat([flat[:self.lo], flat[self.hi:]])
        assert bool((g == self.guard).all()), f"{name}: guard rows were written"
        assert bool(torch.isfinite(flat[self.lo:self.hi].double()).all()), f"{name}: NaN / Inf or unwritten elements"

    def renan(self):
        """the same values between NaN guards: the input of the next kernel"""
        return Buf(self.cpu(), NAN)


def sync():
    torch.cuda.synchronize()


# ====================================================================================================== attention
def run_attention(N, qkv, dout, B, S, H):
    C = H * R.DH
    q, g = Buf(qkv, NAN), Buf(dout, NAN)
    out, lse, dqkv = Buf.out((B * S, C), BF16), Buf.out((B * H, S), F32), Buf.out((B * S, 3 * C), BF16)
    N.call("attn_fwd", q.t, out.t, lse.t, B, S, H, R.SCALE)
    sync()
    out_in, lse_in = out.renan(), lse.renan()
    N.call("attn_bwd", q.t, out_in.t, g.t, lse_in.t, dqkv.t, B, S, H, R.SCALE)
    sync()
    for name, b in (("out", out), ("lse", lse), ("dqkv", dqkv)):
        b.check(name)
    d = dqkv.cpu()
    return dict(out=out.cpu(), lse=lse.cpu(), dq=d[:, :C], dk=d[:, C:2 * C], dv=d[:, 2 * C:])


@pytest.mark.parametrize("family,B,H,S", R.ATTN_CASES)
def test_attention_vs_fp64_per_row(N, family, B, H, S):
    """one forward and one backward launch per case: S <= 128 the single-tile pair, longer the two-sweep forward and the dQ and
    dK / dV kernels; S on wave (31 / 32 / 33, 64, 96) and tile (127 / 128 / 129, 255 / 256 / 257, 385) boundaries, (3, 5, 37) for the
    bh / H, h * 64 and ld = 3 * H * 64 indexing.  offset: no result without the max subtraction; peaked: nor without the rescale of
    the running sum in sweep 1."""
    qkv, dout, ref, emu = R.attn_case(family, B, S, H)
    got = run_attention(N, qkv, dout, B, S, H)
    bad = []
    for n in ("out", "dq", "dk", "dv"):
        row, head, whole = R.rel_rows(got[n], ref[n]), R.rel_rows(got[n], ref[n], R.DH), R.rel_all(got[n], ref[n])
        show(f"attention {family} B{B} H{H} S{S} {n}", row=row, emu_row=emu[n][0], row_head=head, emu_row_head=emu[n][1], all=whole)
        if not (row <= R.ATTN_MARGIN * emu[n][0] and head <= R.ATTN_MARGIN * emu[n][1] and whole <= (1e-2 if n == "out" else 2e-2)):
            bad.append((n, row, emu[n][0], head, emu[n][1], whole))
    err = (got["lse"].double() - ref["lse"]).abs()
    show(f"attention {family} B{B} H{H} S{S} lse", max_abs=float(err.max()))
    assert not bad, bad
    np.testing.assert_allclose(got["lse"].numpy(), ref["lse"].numpy(), rtol=2e-3, atol=2e-3)
    if family == "plain":
        assert float(err.max()) <= 1e-4


def test_attention_single_token_is_exact(N):
    """S = 1: the soft-max is 1, so out == v and dv == dout bit for bit, dq and dk are exactly 0, lse is the score itself"""
    B, H, S = 2, 2, 1
    C = H * R.DH
    qkv, dout = R.attn_inputs("plain", B, S, H)
    got = run_attention(N, qkv, dout, B, S, H)
    assert torch.equal(got["out"], qkv[:, 2 * C:]) and torch.equal(got["dv"], dout)
    assert bool((got["dq"] == 0).all()) and bool((got["dk"] == 0).all())
    score = R.attn_scores(qkv, B, S, H).reshape(B * H, S)
    err = float((got["lse"].double() - score).abs().max())
    show("attention S1", lse_abs=err)
    assert err <= 1e-6


@pytest.mark.parametrize("S", [33, 129])
def test_attention_zero_dout_gives_zero_gradient(N, S):
    B = H = 2
    qkv, dout = R.attn_inputs("plain", B, S, H)
    got = run_attention(N, qkv, torch.zeros_like(dout), B, S, H)
    for n in ("dq", "dk", "dv"):
        assert bool((got[n] == 0).all()), n


@pytest.mark.parametrize("S", [33, 129])
@pytest.mark.parametrize("which", ["qkv", "out", "dout", "dqkv"])
def test_attention_rejects_misaligned_pointers(N, S, which):
    B = H = 2
    C = H * R.DH
    qkv, dout = R.attn_inputs("plain", B, S, H)
    sh = {n: int(n == which) for n in ("qkv", "out", "dout", "dqkv")}
    q, g = Buf(qkv, NAN, sh["qkv"]), Buf(dout, NAN, sh["dout"])
    out, lse, dqkv = Buf.out((B * S, C), BF16, sh["out"]), Buf.out((B * H, S), F32), Buf.out((B * S, 3 * C), BF16, sh["dqkv"])
    if which in ("qkv", "out"):
        with pytest.raises(RuntimeError, match="EALIGN"):
            N.call("attn_fwd", q.t, out.t, lse.t, B, S, H, R.SCALE)
    with pytest.raises(RuntimeError, match="EALIGN"):
        N.call("attn_bwd", q.t, out.t, g.t, lse.t, dqkv.t, B, S, H, R.SCALE)
    sync()
    for b in (out, lse, dqkv):                                  # rejected before any launch: nothing was written at all
        assert bool(torch.isnan(b.cpu().float()).all())


# ====================================================================================================== LayerNorm
def run_layernorm(N, M, C, offset, misaligned):
    """forward + backward at one (M, C) -> figures; asserts guards, finiteness and the exact-type checks"""
    x, gamma, beta, dy, base = R.ln_inputs(M, C, offset)
    ref = R.ln_ref64(M, C, offset)
    shift = 1 if misaligned else 0
    xs, gm, bt = Buf(x, NAN, shift), Buf(gamma, NAN), Buf(beta, NAN)
    y, y32, mean, rstd = Buf.out((M, C), BF16), Buf.out((M, C), F32), Buf.out((M,), F32), Buf.out((M,), F32)
    N.call("layernorm_fwd", xs.t, gm.t, bt.t, y.t, y32.t, mean.t, rstd.t, M, C, R.LN_EPS)
    sync()
    xb, dyb, mean_in, rstd_in = Buf(x, NAN), Buf(dy, NAN, shift), mean.renan(), rstd.renan()
    dres, dg, db = Buf(base, SENTINEL), Buf(prefill(C, 0), SENTINEL), Buf(prefill(C, 1), SENTINEL)
    N.call("layernorm_bwd", dyb.t, xb.t, mean_in.t, rstd_in.t, gm.t, dres.t, dg.t, db.t, M, C)
    sync()
    for name, b in (("y", y), ("y32", y32), ("mean", mean), ("rstd", rstd), ("dres", dres), ("dgamma", dg), ("dbeta", db)):
        b.check(f"{name} M{M} C{C}")                            # the row after the last one is the first guard row
    yd = y.cpu().double()
    fig = dict(y32=R.rel_rows(y32.cpu(), ref["y"]),
               y_ulp=float(((yd - ref["y"]).abs() / (R.bf16_ulp(ref["y"]) + 1e-6)).max()),
               mean=float(((mean.cpu().double() - ref["mean"]).abs() / (1e-5 * ref["mean"].abs() + 1e-6)).max()),
               rstd=float(((rstd.cpu().double() - ref["rstd"]).abs() / ref["rstd"]).max()),
               dres=R.rel_rows(dres.cpu().double() - base.double(), ref["dx"]),
               dgamma=R.rel_all(dg.cpu().double() - prefill(C, 0).double(), ref["dgamma"]),
               dbeta=R.rel_all(db.cpu().double() - prefill(C, 1).double(), ref["dbeta"]))
    return fig


LN_PATHS = ([(C, "vec") for C in R.LN_C_VEC] + [(C, "scalar") for C in R.LN_C_SCALAR] + [(768, "misaligned")])


@pytest.mark.parametrize("C,path", LN_PATHS)
def test_layernorm_vs_fp64_every_m(N, C, path):
    """M = 1 ... 130 against the forward's two rows per wave / eight per workgroup and the backward's pairs of rows, 16 per wave,
    64 per workgroup: odd M leaves a dead second row, 65 a one-row workgroup, 130 a third workgroup for the dgamma / dbeta atomics.
    gamma has a negative entry and an exact zero; dgamma and dbeta must ACCUMULATE onto their start values."""
    assert (C % 4 == 0) == (path != "scalar")
    bad = []
    for M in R.LN_M:
        f = run_layernorm(N, M, C, 0.5, path == "misaligned")
        show(f"layernorm {path} M{M} C{C}", **f)
        ok = (f["y32"] <= 1e-6 and f["y_ulp"] <= 1.0 and f["mean"] <= 1.0 and f["rstd"] <= 1e-5 and
              f["dres"] <= 1e-5 and f["dgamma"] <= 1e-5 and f["dbeta"] <= 1e-5)
        if not ok:
            bad.append((M, f))
    assert not bad, bad


@pytest.mark.parametrize("C", R.LN_OFFSET_C)
def test_layernorm_offset_100_is_two_pass(N, C):
    """x = uniform +-2 + 100: a one-pass variance is 4e-4 or worse here (test_host_vit_ref.py), two passes in fp32 2.5e-5 or better"""
    bad = []
    for M in R.LN_OFFSET_M:
        f = run_layernorm(N, M, C, 100.0, False)
        show(f"layernorm offset100 M{M} C{C}", **f)
        if not (f["y32"] <= 1e-4 and f["rstd"] <= 1e-4 and f["mean"] <= 1.0 and f["dres"] <= 1e-4 and f["dgamma"] <= 1e-4 and f["dbeta"] <= 1e-4):
            bad.append((M, f))
    assert not bad, bad


# ====================================================================================================== GELU
@functools.lru_cache(maxsize=None)
def gelu_case():
    x = R.all_finite_bf16()
    return x, R.gelu64(x), R.gelu_grad64(x)


def gelu_bound(ref):
    """one bf16 rounding plus a crossed rounding boundary, and the fp32 cancellation of 1 + erff on the negative tail"""
    return 2.0 ** -8 * ref.abs() + 1e-6


def test_gelu_forward_every_bf16_value(N):
    x, ref, _ = gelu_case()
    xs, h = Buf(x, NAN), Buf.out(tuple(x.shape), BF16)
    N.call("gelu_fwd", xs.t, h.t, x.numel())
    sync()
    h.check("h")
    got, xf = h.cpu().double(), x.double()
    ratio = (got - ref).abs() / gelu_bound(ref)
    i = int(ratio.argmax())
    show("gelu_fwd", worst=float(ratio.max()), at_x=float(xf[i]))
    assert float(ratio.max()) <= 1.0
    assert torch.equal(got[xf >= 8], xf[xf >= 8])
    assert float(got[xf <= -8].abs().max()) <= 1e-6


@pytest.mark.parametrize("dh_kind", ["ones", "uniform"])
def test_gelu_backward_every_bf16_value(N, dh_kind):
    x, _, dref = gelu_case()
    if dh_kind == "ones":
        dh = torch.ones(x.numel()).bfloat16()
    else:
        dh = (torch.rand(x.numel(), generator=torch.Generator().manual_seed(401)) * 2 - 1).bfloat16()
    xs, g, da = Buf(x, NAN), Buf(dh, NAN), Buf.out(tuple(x.shape), BF16)
    N.call("gelu_bwd", xs.t, g.t, da.t, x.numel())
    sync()
    da.check("da")
    got, s = da.cpu().double(), dh.double().abs()
    ratio = (got - dh.double() * dref).abs() / (s * gelu_bound(dref)).clamp_min(1e-300)
    ratio = torch.where((s == 0) & (got == 0), torch.zeros_like(ratio), ratio)
    i = int(ratio.argmax())
    show(f"gelu_bwd dh={dh_kind}", worst=float(ratio.max()), at_x=float(x.double()[i]))
    assert float(ratio.max()) <= 1.0


# ====================================================================================================== patch_unfold, tile_rows
@pytest.mark.parametrize("F,T,fs,ts", R.PATCH_CASES)
def test_patch_unfold_bit_exact(N, F, T, fs, ts):
    """a gather plus one rounding: overlapping patches, exact tiling, a single patch, strides that leave a remainder"""
    B = 3
    x = torch.rand(B, F, T, generator=torch.Generator().manual_seed(500 + F)) * 2 - 1
    nf, nt = R.patch_grid(F, T, fs, ts)
    assert (nf, nt) == tuple(torch.nn.functional.conv2d(torch.zeros(1, 1, F, T), torch.zeros(1, 1, 16, 16), stride=(fs, ts)).shape[2:])
    xs, rows = Buf(x, NAN), Buf.out((B * nf * nt, 256), BF16)
    N.call("patch_unfold", xs.t, rows.t, B, F, T, fs, ts)
    sync()
    rows.check("rows")
    assert torch.equal(rows.cpu(), R.patch_unfold_ref(x, fs, ts))


@pytest.mark.parametrize("rows,Ntok,B,C", R.TILE_CASES)
@pytest.mark.parametrize("form", ["pos_embed", "token_mean_bwd"])
def test_tile_rows_bit_exact(N, rows, Ntok, B, C, form):
    """group 1, period Ntok: the position embedding over the batch; group Ntok, period B, scale 1 / Ntok: token-mean backward"""
    period, group, scale = (Ntok, 1, 1.0) if form == "pos_embed" else (B, Ntok, R.f32(1.0 / Ntok))
    src = torch.rand(period, C, generator=torch.Generator().manual_seed(800 + C + period)) * 2 - 1
    s, out = Buf(src, NAN), Buf.out((rows, C), F32)
    N.call("tile_rows", s.t, out.t, rows, period, group, scale, C)
    sync()
    out.check("out")
    assert torch.equal(out.cpu(), R.tile_rows_ref(src, rows, period, group, scale))
    for sh_src, sh_out in ((1, 0), (0, 1)):
        s2, o2 = Buf(src, NAN, sh_src), Buf.out((rows, C), F32, sh_out)
        with pytest.raises(RuntimeError, match="EALIGN"):
            N.call("tile_rows", s2.t, o2.t, rows, period, group, scale, C)


# ====================================================================================================== AdamW
@pytest.mark.parametrize("n,t0,gscale", R.ADAMW_CASES)
def test_adamw_vs_fp64(N, n, t0, gscale):
    """three steps from step count t0 (1: fresh moments, 1000: a running state) with grad_scale 1 or 1 / 32; n = 3 is the scalar
    tail alone, 2048 * 1024 + 4003 the second grid-stride trip and then a tail.  Buffers are padded to a multiple of 4; the
    padding must come back bit for bit."""
    hp = R.ADAMW_HP
    p0, grads, m0, v0 = R.adamw_inputs(n, t0)
    pad = (-n) % 4
    padded = lambda t, fillv: torch.cat([t, torch.full((pad,), fillv)])
    p, m, v = Buf(padded(p0, 7.0), SENTINEL), Buf(padded(m0, 5.0), SENTINEL), Buf(padded(v0, 3.0), SENTINEL)
    step = Buf(torch.tensor([t0 - 1], dtype=torch.int64), -7)
    for g in grads:
        gb = Buf(padded(g, 9.0), NAN)
        step.t.add_(1)
        N.call("adamw", p.t, gb.t, m.t, v.t, n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], gscale, step.t)
    sync()
    rp, rm, rv = R.adamw_ref(n, t0, gscale)
    assert int(step.cpu()[0]) == t0 + 2
    step.check("step")
    for name, b, ref, fillv in (("p", p, rp, 7.0), ("m", m, rm, 5.0), ("v", v, rv, 3.0)):
        b.check(name)
        got = b.cpu()
        assert bool((got[n:] == fillv).all()), f"{name}: padding changed"
        err = (got[:n].double() - ref).abs() / (1e-7 + 2e-5 * ref.abs())
        show(f"adamw n{n} t0={t0} gscale={gscale} {name}", worst_in_tol=float(err.max()))
        np.testing.assert_allclose(got[:n].numpy(), ref.numpy(), rtol=2e-5, atol=1e-7, err_msg=name)
    p2 = Buf(padded(p0, 7.0), SENTINEL, 1)
    with pytest.raises(RuntimeError, match="EALIGN"):
        N.call("adamw", p2.t, gb.t, m.t, v.t, n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], gscale, step.t)
