"""Exact cases for the 3x3 / 64 -> 64 convolution (csrc/conv.hip): inputs whose convolution, data gradient and weight gradient are
EXACT in fp32, so that a kernel is compared with the float64 reference by equality of bits and not by a tolerance.

  x, dy   integers in [-2, 2]                 (bf16-exact)
  w       integers in [-16, 16] / 64          (bf16-exact)
  bias    integers in [-32, 32] / 64
  dW0     integers in [-1000, 1000]           (what dWp holds before the weight gradient adds to it)

Every product is a multiple of 2^-6 and |y| <= 576 * 2 * 0.25 + 0.5 = 288.5: 15 significant bits.  |dW| <= 4 * pixels + 1000 < 2^24
for every shape below (at most 8200 * 16 pixels).  So every partial sum, in whatever order the MFMA, the waves and the atomics take
them, is an fp32 number and the result does not depend on the order.  About a quarter of the outputs need bf16 rounding (8
significant bits; |y| is mostly below 4, where the 1/64 grid is bf16-exact), and those between 4 and 8 are all ties.
`fwd_ref()` / `wgrad_ref()` assert the premise on the reference itself: every float64 result is an fp32 number, an fp32
convolution on the CPU gives the same numbers, and no result is a negative zero (equality of bits would otherwise depend on the
sign an implementation gives a zero sum).

Layout: activations [N][Ti][Fi][64] (channels last, kh walks Fi, kw walks Ti); the reference is torch's conv2d on [N][C][Fi][Ti]."""
import functools

import torch
import torch.nn.functional as Fnn

# (N, Ti, Fi): tiles are 256 pixels - 8 rows at Fi = 32, 16 rows at Fi = 16 - rows are counted across images (g = n * Ti + t), and at
# most 256 persistent workgroups walk them (workgroup i: tiles i, i + 256, ...)
SHAPES = [
    (1, 1, 32),        # single partial tile; the one row is top and bottom border
    (3, 1, 32),        # all rows are borders (every row is a whole image)
    (2, 2, 32),        # all rows are borders (top or bottom)
    (5, 3, 32),        # border inside a tile, 15 rows: two tiles, the second partial
    (1, 8, 32),        # exactly one tile
    (1, 9, 32),        # a one-row last tile
    (2, 7, 32),        # border inside a tile, partial last tile
    (3, 8, 32),        # border on a tile border: the halo rows belong to the neighbouring images
    (32, 64, 32),      # 256 tiles: the last launch where every workgroup walks one tile
    (257, 8, 32),      # 257 tiles aligned with images: workgroup 0 walks two tiles, the rest one
    (1, 2049, 32),     # 257 tiles with a one-row last tile and an odd row count
    (1, 4100, 32),     # 513 tiles: three for workgroup 0 (the double buffer flips twice), a half-filled last tile
    (1, 1, 16),        # single partial tile; the one row is top and bottom border
    (3, 1, 16),        # all rows are borders; an odd row count: the second row of the last row pair is past the end
    (2, 2, 16),        # all rows are borders
    (5, 3, 16),        # border inside a tile and inside a wave's row pair, 15 rows
    (1, 16, 16),       # exactly one tile
    (1, 17, 16),       # a one-row last tile: the second row of its first row pair is past the end
    (2, 15, 16),       # border inside a tile, partial last tile
    (3, 16, 16),       # border on a tile border
    (2, 32, 16),       # border on a tile border, images of two tiles
    (128, 32, 16),     # 256 tiles
    (257, 16, 16),     # 257 tiles aligned with images
    (1, 4097, 16),     # 257 tiles with a one-row last tile and an odd row count
    (1, 8200, 16),     # 513 tiles: three for workgroup 0, a half-filled last tile
]
ISOLATION_SHAPES = [(3, 8, 32), (3, 16, 16), (2, 7, 32), (2, 15, 16), (5, 3, 16)]
WS_FLOATS = 64 * 576                     # one workgroup's partial result in the weight gradient's workspace


def tiles(shape):
    n, ti, fi = shape
    tt = 256 // fi
    return (n * ti + tt - 1) // tt


def shape_id(shape):
    return "%dx%dx%d" % shape


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def to_nchw(a):
    """[N][Ti][Fi][C] -> [N][C][Fi][Ti] float64"""
    return a.double().permute(0, 3, 2, 1).contiguous()


def from_nchw(a):
    return a.permute(0, 3, 2, 1).contiguous()


def unpacked(dwp):
    """packed [co][tap * 64 + ci] -> [co][ci][kh][kw], tap = kh * 3 + kw (what unpack_conv_dw adds into its output)"""
    return dwp.view(64, 9, 64).permute(0, 2, 1).reshape(64, 64, 3, 3).contiguous()


def _is_f32(t):
    return bool(torch.equal(t.float().double(), t))


def _no_negative_zero(t):
    return not bool((torch.signbit(t) & (t == 0)).any())


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """CPU tensors of one shape, made once and left unchanged: x, dy (bf16, channels last), w [co][ci][kh][kw], bias, dw0 (fp32)"""
    n, ti, fi = shape
    gen = torch.Generator().manual_seed(9000 + 97 * n + 13 * ti + fi)
    x = _ints(gen, (n, ti, fi, 64), -2, 2)
    dy = _ints(gen, (n, ti, fi, 64), -2, 2)
    w = _ints(gen, (64, 64, 3, 3), -16, 16) / 64
    bias = _ints(gen, (64,), -32, 32) / 64
    dw0 = _ints(gen, (64, 576), -1000, 1000)
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(dy.bfloat16().float(), dy) and torch.equal(w.bfloat16().float(), w)
    return dict(shape=shape, x=x.bfloat16(), dy=dy.bfloat16(), w=w, bias=bias, dw0=dw0)


def _premise(shape, name, t):
    assert _is_f32(t), f"{shape}: the float64 {name} is not an fp32 tensor"
    assert _no_negative_zero(t), f"{shape}: the float64 {name} holds a negative zero"


@functools.lru_cache(maxsize=None)
def fwd_ref(shape, fp32_too=True):
    """float64 references of the forward and the data gradient, stored as the fp32 numbers they are, channels last: y (with bias),
    y0 (without), dx.  fp32_too: also assert that the CPU's fp32 convolution gives the same numbers (the child processes leave that
    half of the premise to the parent, which asserts it for every shape)."""
    c = inputs(shape)
    xn, dyn, wd = to_nchw(c["x"]), to_nchw(c["dy"]), c["w"].double()
    y0 = Fnn.conv2d(xn, wd, None, padding=1)
    y = y0 + c["bias"].double().view(1, 64, 1, 1)
    dx = torch.nn.grad.conv2d_input(xn.shape, wd, dyn, padding=1)
    for name, t in (("y", y), ("y0", y0), ("dx", dx)):
        _premise(shape, name, t)
    assert float(y.abs().max()) <= 288.5 and float(dx.abs().max()) <= 288.0
    if fp32_too:
        assert torch.equal(Fnn.conv2d(xn.float(), c["w"], c["bias"], padding=1).double(), y)
        assert torch.equal(torch.nn.grad.conv2d_input(xn.shape, c["w"], dyn.float(), padding=1).double(), dx)
    return dict(y=from_nchw(y).float(), y0=from_nchw(y0).float(), dx=from_nchw(dx).float())


@functools.lru_cache(maxsize=None)
def wgrad_ref(shape, fp32_too=True):
    """float64 reference of what the weight gradient leaves behind: unpacked(dw0) + conv2d_weight, [co][ci][kh][kw], as fp32"""
    c = inputs(shape)
    xn, dyn = to_nchw(c["x"]), to_nchw(c["dy"])
    dw = torch.nn.grad.conv2d_weight(xn, c["w"].shape, dyn, padding=1)
    total = unpacked(c["dw0"]).double() + dw
    _premise(shape, "dw", dw)
    _premise(shape, "dw0 + dw", total)
    assert float(total.abs().max()) < 2 ** 24
    if fp32_too:
        assert torch.equal(torch.nn.grad.conv2d_weight(xn.float(), c["w"].shape, dyn.float(), padding=1).double(), dw)
    return total.float()


def bits(t):
    return t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def mismatches(got, want):
    """number of elements of `got` whose bits differ from `want` (same shape and type required)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((bits(got) != bits(want)).sum())


def fwd_name(fi, stats, f32):
    return f"conv3x3_ws_kernel<{fi}, {'true' if stats else 'false'}, {'true' if f32 else 'false'}>"


def wgrad_name(fi, kg, fold):
    return f"conv3x3_wgrad_kernel<{fi}, {kg}>" + ("+reduce" if fold else "")
