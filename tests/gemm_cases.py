"""The GEMM case matrix: cases, operands, the float64 reference and the per-element bound (plain Python, runs on the CPU).

Every operand sits inside a larger allocation - leading dimension 8 past its width, three rows past its end - whose
surplus is NaN, and so does C (guard columns up to ldc, two guard rows): a kernel that reads or writes outside the logical
matrices shows up either as a NaN in the result or as a guard element that changed.

The reference restates the epilogue order of include/audiossl_hip.h in float64, from the operands AS STORED:
    x = alpha * op(A) op(B);  + bias (once, also under split-K);  ReLU;  * keep * keep_scale;  0 where gate <= 0;  + resid;
    store x, or C0 + x.
Bound, element by element (derived, not tuned):  |C - ref| <= f * (K + 8) * 2^-24 * S,
    S = |alpha| * (|op(A)| |op(B)|) + |bias| + |resid| + |C0|.
(K + 8) * 2^-24 * S is the worst case of round-to-nearest fp32 accumulation, in any order, of products that are exact in fp32
(bf16 x bf16: 16 significand bits), the 8 covering the epilogue's handful of operations; f = 2 covers accumulators that truncate
(up to one ulp per add), f = 4 the fp32 operands, whose products round as well.  A bf16 result adds 2^-8 * |ref| for its one
rounding.  ReLU is a contraction and the keep / gate zeros are exact, so neither enters; keep_scale is left out of S as well, which
makes the bound stricter than the derivation by that factor (1 / 0.7) - rounding errors grow like sqrt(K) and stay far below it."""
import math
import zlib

import numpy as np
import torch

from oracle import fill

NAN = float("nan")
PAD_COLS, PAD_ROWS, GUARD_ROWS = 8, 3, 2
KEEP_SCALE = 1.0 / 0.7
LAYOUTS = ((0, 0), (0, 1), (1, 1), (1, 0))                    # (trans_a, trans_b): NT, NN, TN and the fourth one
VARIANTS = ("reg64x128", "reg128_k64", "reg128_k128", "ring64", "ring128", "bk32", "p8", "pk5", "sp5", "sp6", "sp8")
MULTI_VARIANTS = ("reg64x128", "reg128_k64", "reg128_k128", "p8", "pk5", "sp5", "sp6", "sp8")
_REG = {"reg64x128": (64, 1), "reg128_k64": (64, 2), "reg128_k128": (128, 2)}
_TF = ("false", "true")

# mode -> epilogue and output of audiossl_gemm (section "Output and epilogue modes" of the matrix)
MODES = {
    "a": dict(out_f32=1),
    "b": dict(out_f32=0, bias=1, relu=1, keep=1, gate=1),
    "c": dict(out_f32=0, bias=1, relu=1, keep=1, gate=1, odd_ldc=1),
    "d": dict(out_f32=1, alpha=0.5, bias=1, resid=1),
    "do": dict(out_f32=1, alpha=0.5, bias=1, resid=1, odd_ldc=1),  # (d) through the one-column-per-lane epilogue
    "e": dict(out_f32=1, atomic=2),
    "f": dict(out_f32=1, atomic=1, bias=1),                   # + ksplit
}


def cdiv(a, b):
    return (a + b - 1) // b


def up8(n):
    return cdiv(n, 8) * 8


def legal(v, ta, tb, M, Ns, Ks, ksplit=1, multi=False, lse=False):
    """`legal()` of csrc/gemm.hip: where AUDIOSSL_GEMM_FORCE=<v> takes effect.  The generator emits only legal cases, so a launch
    that reports another kernel than the forced one is a failure."""
    N, kmin, count = max(Ns), min(Ks), len(Ns)
    blocks = cdiv(M, 128) * cdiv(N, 128) * ksplit * count
    hs = M >= 128 and N >= 128 and (not ta or M % 8 == 0) and all(k % 64 == 0 for k in Ks) and (not tb or all(n % 8 == 0 for n in Ns))
    if v == "reg64x128":
        return blocks <= 128 and M > 64
    if v == "reg128_k64":
        return True
    if v == "reg128_k128":
        return blocks <= 256 and kmin >= 512
    if v in ("ring64", "ring128"):
        return not multi and kmin % 64 == 0 and M >= 8 and N >= 8
    if v == "bk32":
        return not multi and blocks >= 512
    if v in ("p8", "sp8"):
        return hs and M >= 256 and N >= 256
    if v == "sp6":
        return hs and not lse and M >= 256
    if v in ("pk5", "sp5"):
        return hs and not lse
    raise KeyError(v)


def kernel_name(v, ta, tb, entry="gemm"):
    """What audiossl_last_kernel reports for variant v (None: the fp32 kernel) in layout (ta, tb)."""
    multi, sgd = entry.startswith("gemm_multi"), entry == "gemm_multi_sgd"
    m, a, b = ("_multi" if multi else ""), _TF[ta], _TF[tb]
    if v is None:
        return f"gemm_kernelIfLb{ta}ELb{tb}ELi32ELi2ELi4E"
    if v in _REG:
        return f"gemm{m}_kernelIDF16bLb{ta}ELb{tb}ELi{_REG[v][0]}ELi{_REG[v][1]}ELi4E"
    if v in ("ring64", "ring128"):
        return f"gemm_ring_kernel<{a}, {b}, {1 if v == 'ring64' else 2}, 4>"
    if v == "bk32":
        return f"gemm_bk32_kernel<{a}, {b}>"
    if v == "p8":
        return f"gemm_p8_multi{'_sgd' if sgd else ''}_kernel<{a}, {b}>" if multi else f"gemm_p8_kernel<{a}, {b}, 0>"
    if v == "pk5":
        return f"gemm_pk{m}_kernel<{a}, {b}, 5>"
    return f"gemm_sp{m}{'_sgd' if sgd else ''}_kernel<{a}, {b}, {v[2]}>"


def fit(ta, tb, M, N):
    """M is odd only when trans_a = 0, N only when trans_b = 0 (the vector dimension of an operand is a multiple of 8)."""
    return (up8(M) if ta else M), (up8(N) if tb else N)


# ---------------------------------------------------------------------------------------------------------- the single-problem matrix
_PIPE_SHAPES = {"p8": ((300, 520), (520, 520)), "sp8": ((300, 520), (520, 520)), "sp6": ((300, 136), (520, 264)),
                "pk5": ((136, 200), (264, 328)), "sp5": ((136, 200), (264, 328)),
                "ring64": ((8, 8), (72, 136), (136, 137)), "ring128": ((8, 8), (72, 136), (136, 137))}
_PIPE_K = (64, 128, 192, 448)
# (ksplit, K) of mode (f) on the pipelined kernels: one K-tile per split, fewer than the ring depth, none (ksplit > K-tiles)
_PIPE_SPLITS = ((8, 64), (8, 192), (8, 448), (2, 192), (3, 448), (2, 448))


def _case(v, dtype, ta, tb, M, N, K, mode, ksplit=1):
    M, N = fit(ta, tb, M, N)
    tag = "f32" if dtype == 0 else v
    return dict(entry="gemm", id=f"{tag}-{_TF[ta][0]}{_TF[tb][0]}-{M}x{N}x{K}-{mode}{ksplit if mode == 'f' else ''}", variant=v, dtype=dtype,
                ta=ta, tb=tb, M=M, N=N, K=K, mode=mode, ksplit=ksplit,
                expect=kernel_name(v if dtype else None, ta, tb))


def _reg_cases(v, dtype):
    """The register-staged kernels, bf16 (forced variant v) or fp32 (dtype 0, default path: one kernel)."""
    ks = (520, 512) if v == "reg128_k128" else (8, 40, 72, 520)
    shapes = ((1, 1), (7, 5), (72, 105), (200, 136))
    out = []
    for ta, tb in LAYOUTS:
        def ok(M, N, K, s=1, ta=ta, tb=tb):
            M, N = fit(ta, tb, M, N)
            return dtype == 0 or legal(v, ta, tb, M, [N], [K], s)
        for i, (M, N) in enumerate(shapes):                          # (a) on every shape, the K set dealt over them
            for K in {ks[i % len(ks)], ks[(i + 1) % len(ks)]}:
                if ok(M, N, K):
                    out.append(_case(v, dtype, ta, tb, M, N, K, "a"))
        if ok(1024, 1024, ks[1]):                                    # 64 tiles (reg64x128: 128): the xcd_remap branch
            out.append(_case(v, dtype, ta, tb, 1024, 1024, ks[1], "a"))
        for mode in "bcde" if dtype else "cde":
            for (M, N), K in (((72, 105), ks[1]), ((200, 136), ks[-2] if len(ks) > 2 else ks[0])):
                if ok(M, N, K):
                    out.append(_case(v, dtype, ta, tb, M, N, K, mode))
        # (f): K-steps of 64 (fp32: 32; reg128_k128: 128) against 2, 3 and 8 splits: one step per split, empty splits
        for s, K in ((2, ks[0]), (3, ks[0]), (8, ks[0]), (8, ks[-1]), (2, ks[-1])) if v == "reg128_k128" else ((2, 72), (3, 72), (8, 8), (8, 520), (3, 520)):
            for M, N in ((72, 105), (200, 136)):
                if ok(M, N, K, s):
                    out.append(_case(v, dtype, ta, tb, M, N, K, "f", s))
                    break
    return out


def _pipe_cases(v):
    small, nine_ = _PIPE_SHAPES[v][-2 if v.startswith("ring") else 0], _PIPE_SHAPES[v][-1]
    out = []
    for ta, tb in LAYOUTS:
        nine = nine_ if tb or nine_[1] % 8 else (nine_[0], nine_[1] + 1)      # N % 8 != 0 wherever B is [N][K]; the tile count stays
        for K in _PIPE_K:
            out.append(_case(v, 1, ta, tb, *small, K, "a"))
        if v.startswith("ring"):
            out.append(_case(v, 1, ta, tb, 8, 8, 64, "a"))
            out.append(_case(v, 1, ta, tb, 8, 8, 192, "d"))
        for mode in "bcde":
            out.append(_case(v, 1, ta, tb, *small, 192, mode))
        for s, K in _PIPE_SPLITS:
            out.append(_case(v, 1, ta, tb, *small, K, "f", s))
        out.append(_case(v, 1, ta, tb, *nine, 128, "a"))              # tile counts congruent to 1 mod 8: xcd_contiguous's remainder branch
        out.append(_case(v, 1, ta, tb, *nine, 64, "b"))
        out.append(_case(v, 1, ta, tb, *nine, 128, "do"))             # the residual line of epilogue_lds (odd ldc, and N % 8 != 0 where legal)
        out.append(_case(v, 1, ta, tb, *nine, 448, "f", 2))
    return out


def _bk32_cases():
    """The only large cases (its rule is >= 512 workgroups), five of them: every layout once, the epilogues dealt over them."""
    big = (2040, 4104)
    return [_case("bk32", 1, 0, 0, *big, 96, "b"), _case("bk32", 1, 0, 1, *big, 72, "d"), _case("bk32", 1, 1, 1, *big, 40, "e"),
            _case("bk32", 1, 1, 0, *big, 96, "c"), _case("bk32", 1, 1, 0, 1024, 2048, 96, "f", 4)]


def single_cases(v):
    """v: a variant name, or None for the fp32 kernel."""
    if v is None:
        cases = _reg_cases("reg128_k64", 0)
    elif v in _REG:
        cases = _reg_cases(v, 1)
    elif v == "bk32":
        cases = _bk32_cases()
    else:
        cases = _pipe_cases(v)
    cases = list({c["id"]: c for c in cases}.values())            # (1, 1) and (7, 5) meet at (8, 8) when both operands are transposed
    for c in cases:
        assert c["dtype"] == 0 or legal(v, c["ta"], c["tb"], c["M"], [c["N"]], [c["K"]], c["ksplit"]), c["id"]
        assert c["K"] <= 520
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


# ---------------------------------------------------------------------------------------------------------- the other entry points
def multi_cases(v):
    """audiossl_gemm_multi: two and three problems of different N and K, partial tiles, every layout; store (bf16, fp32), atomic = 2,
    atomic = 1 with two splits (one problem has a single K-tile: its second split is empty)."""
    if v not in MULTI_VARIANTS:
        return []
    out = []
    for ta, tb in LAYOUTS:
        M = 296 if ta else 300
        Ns = [264, 136, 200] if tb else [264, 137, 200]
        Ks = [520, 512, 520] if v == "reg128_k128" else [192, 64, 128]
        for count, f32, atomic, ks in ((2, 0, 0, 1), (3, 1, 0, 1), (3, 1, 2, 1), (2, 1, 1, 2)):
            assert legal(v, ta, tb, M, Ns[:count], Ks[:count], ks, multi=True)
            out.append(dict(entry="gemm_multi", id=f"multi-{v}-{_TF[ta][0]}{_TF[tb][0]}-{count}-{'f32' if f32 else 'bf16'}-a{atomic}k{ks}", variant=v,
                            ta=ta, tb=tb, M=M, Ns=Ns[:count], Ks=Ks[:count], out_f32=f32, atomic=atomic, ksplit=ks, alpha=0.5 if atomic else 1.0,
                            expect=kernel_name(v, ta, tb, "gemm_multi")))
    return out


def sgd_case(v):
    """audiossl_gemm_multi_sgd against gemm_multi + sgd_momentum (bit for bit) at one small ragged shape, the weight-gradient layout."""
    if v not in MULTI_VARIANTS:
        return []
    K = 520 if v == "reg128_k128" else 192
    assert legal(v, 1, 1, 264, [264, 136], [K, K], multi=True)
    return [dict(entry="gemm_multi_sgd", id=f"sgd-{v}", variant=v, M=264, Ns=[264, 136], K=K, expect=kernel_name(v, 1, 1, "gemm_multi_sgd"),
                 expect_plain=kernel_name(v, 1, 1, "gemm_multi"))]


def barlow_cases(v):
    if v not in MULTI_VARIANTS:
        return []
    out = []
    for D in (128, 256):
        Ks = [64, 192]
        if legal(v, 1, 1, D, [D, D], Ks, multi=True):
            out.append(dict(entry="gemm_multi_barlow", id=f"barlow-{v}-{D}", variant=v, D=D, Ks=Ks, expect=kernel_name(v, 1, 1, "gemm_multi_barlow")))
    return out


def dropout_cases(v):
    """audiossl_gemm_dropout against gemm + dropout_mask (bit for bit): one aligned and one ragged shape."""
    if v == "bk32":
        return []                                                    # large grids only; the existing test runs its fc.0 shape
    K = 520 if v == "reg128_k128" else 192
    shapes = ((128, 128), (72, 137)) if v.startswith("ring") or v in _REG else ((256, 256), (300, 521))
    return [dict(entry="gemm_dropout", id=f"dropout-{v}-{M}x{N}", variant=v, M=M, N=N, K=K, expect=kernel_name(v, 0, 0))
            for M, N in shapes if legal(v, 0, 0, M, [N], [K])]


def moco_cases(v):
    """audiossl_moco_logits modes 1 + 2 (v: p8, sp8, or None = the default choice, which is the 64 x 128 register-staged kernel at
    these sizes: nine 128 x 128 tiles, M > 64, a transposed B).  Slabs (64 columns) and tiles end inside the [B][K] matrix."""
    if v not in (None, "p8", "sp8"):
        return []
    return [dict(entry="moco_logits", id=f"moco-{v or 'default'}-{K}-{dim}", variant=v, B=264, K=K, dim=dim,
                 expect=kernel_name(v or "reg64x128", 0, 1))
            for K in (328, 520) for dim in (64, 128) if v is None or legal(v, 0, 1, 264, [K], [dim], lse=True)]


def all_cases(v):
    """Everything one child runs: v = a variant name (AUDIOSSL_GEMM_FORCE) or None (default choice: the fp32 kernel, moco_logits)."""
    if v is None:
        return single_cases(None) + moco_cases(None)
    return single_cases(v) + multi_cases(v) + sgd_case(v) + barlow_cases(v) + dropout_cases(v) + moco_cases(v)


def result_kind(c):
    """"fp32" / "bf16": what the case stores (a bf16 store spends up to the whole 2^-8 term of its bound on its own rounding); "tol": checked
    against fixed tolerances or bit for bit, not against the derived bound"""
    if c["entry"] == "gemm":
        return "bf16" if c["dtype"] == 1 and not MODES[c["mode"]].get("out_f32", 1) else "fp32"
    if c["entry"] == "gemm_multi":
        return "fp32" if c["out_f32"] else "bf16"
    return "bf16" if c["entry"] == "gemm_multi_barlow" else "tol"


# ---------------------------------------------------------------------------------------------------------- operands
def salt(case_id, k):
    return (zlib.crc32(case_id.encode()) + 0x9E3779B1 * k) & 0xFFFFFFFF


def padded(rows, width, values, td, pad_cols=PAD_COLS, pad_rows=PAD_ROWS, junk=NAN):
    """[rows][width] `values` inside a [rows + pad_rows][width + pad_cols] buffer of `junk`; -> (buffer, leading dimension)"""
    buf = torch.full((rows + pad_rows, width + pad_cols), junk, dtype=td)
    buf[:rows, :width] = torch.as_tensor(values).to(td)
    return buf, width + pad_cols


def gate_values(M, N, s):
    """gate operand: uniform, with exact +0.0, -0.0 (both must zero the output) and negative entries at known places"""
    g = fill.uniform((M, N), s).astype(np.float64)
    flat = g.reshape(-1)
    flat[0::7] = 0.0
    flat[3::7] = -0.0
    flat[5::7] = -np.abs(flat[5::7]) - 2.0 ** -20
    assert (g == 0).any() and np.signbit(g[g == 0]).any() and (g < 0).any() and (g > 0).any()
    return g


def build_problem(pid, dtype, ta, tb, M, N, K, out_f32=1, alpha=1.0, bias=0, relu=0, keep=0, gate=0, resid=0, atomic=0, odd_ldc=0, **_):
    """Host side of one problem: the padded buffers a kernel gets (torch CPU tensors) and the logical operands in float64."""
    td = torch.float32 if dtype == 0 else torch.bfloat16
    out_td = torch.float32 if (out_f32 or dtype == 0) else torch.bfloat16
    p = dict(dtype=dtype, ta=ta, tb=tb, M=M, N=N, K=K, alpha=alpha, relu=relu, atomic=atomic, out_td=out_td, keep_scale=KEEP_SCALE if keep else 1.0)
    ar, aw = (K, M) if ta else (M, K)
    br, bw = (K, N) if tb else (N, K)
    p["A"], p["lda"] = padded(ar, aw, fill.uniform((ar, aw), salt(pid, 1)), td)
    p["B"], p["ldb"] = padded(br, bw, fill.uniform((br, bw), salt(pid, 2)), td)
    A, B = p["A"][:ar, :aw].double(), p["B"][:br, :bw].double()
    p["opA"], p["opB"] = (A.T if ta else A), (B if tb else B.T)
    ldc = up8(N) + 8 + (1 if odd_ldc else 0)
    # C with guard columns and rows: NaN for the store modes, a known C0 for the accumulating ones (guards included)
    if atomic:
        p["C0"] = torch.from_numpy(fill.uniform((M + GUARD_ROWS, ldc), salt(pid, 3))).to(out_td)
    else:
        p["C0"] = torch.full((M + GUARD_ROWS, ldc), NAN, dtype=out_td)
    p["ldc"] = ldc
    p["bias"] = torch.from_numpy(fill.uniform((N,), salt(pid, 4))) if bias else None
    p["keep"] = p["gate"] = p["resid"] = None
    p["ldk"] = p["ldg"] = p["ldr"] = 0
    if keep:
        kv = (fill.uniform01((M, N), salt(pid, 5)) >= 0.3).astype(np.uint8)
        assert (kv == 0).any() and (kv == 1).any()
        p["keep"], p["ldk"] = padded(M, N, kv, torch.uint8, pad_cols=up8(N) - N + 8, pad_rows=0, junk=1)
    if gate:
        p["gate"], p["ldg"] = padded(M, N, gate_values(M, N, salt(pid, 6)), td, pad_cols=up8(N) - N + 8, pad_rows=0)
    if resid:
        p["resid"], p["ldr"] = padded(M, N, fill.uniform((M, N), salt(pid, 7)), torch.float32, pad_cols=up8(N) - N + 8, pad_rows=0)
    return p


def reference(p):
    """-> (ref, bound), float64 [M][N]"""
    M, N, K = p["M"], p["N"], p["K"]
    x = p["alpha"] * (p["opA"] @ p["opB"])
    S = abs(p["alpha"]) * (p["opA"].abs() @ p["opB"].abs())
    if p["bias"] is not None:
        x = x + p["bias"].double()
        S = S + p["bias"].double().abs()
    if p["relu"]:
        x = x.clamp_min(0.0)
    if p["keep"] is not None:
        x = torch.where(p["keep"][:M, :N] != 0, x * p["keep_scale"], torch.zeros_like(x))
    if p["gate"] is not None:
        x = torch.where(p["gate"][:M, :N].double() > 0, x, torch.zeros_like(x))
    if p["resid"] is not None:
        x = x + p["resid"][:M, :N].double()
        S = S + p["resid"][:M, :N].double().abs()
    if p["atomic"]:
        x = p["C0"][:M, :N].double() + x
        S = S + p["C0"][:M, :N].double().abs()
    bound = (4.0 if p["dtype"] == 0 else 2.0) * (K + 8) * 2.0 ** -24 * S
    if p["out_td"] == torch.bfloat16:
        bound = bound + 2.0 ** -8 * x.abs()
    return x, bound


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over every element; inf where the result is not finite or a zero bound is missed"""
    err = (got.double() - ref).abs()
    inf = torch.full_like(err, math.inf)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    r = torch.where(torch.isfinite(err), r, inf)
    return float(r.max()), int((r > 1).sum())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def guards_intact(C, C0, M, N):
    """every element of the C allocation outside [0:M, 0:N] is bit-identical to its prefill"""
    same = _bits(C) == _bits(C0)
    same[:M, :N] = True
    return bool(same.all())


def check(p, C):
    """C: the whole allocation after the launch (CPU).  -> (worst ratio, elements over their bound, guards intact)"""
    ref, bound = reference(p)
    ratio, nbad = worst_ratio(C[:p["M"], :p["N"]], ref, bound)
    return ratio, nbad, guards_intact(C, p["C0"], p["M"], p["N"])
