"""GPU: every instantiation of the 3x3 convolution kernels (csrc/conv.hip) against float64, BIT FOR BIT, at the tile edges.

The inputs (tests/conv_cases.py) are small integers and multiples of 1/64, so that the convolution, the data gradient and the weight
gradient are exact in fp32 in whatever order they are summed: the expected fp32 output is the float64 reference itself, the expected
bf16 output its round-to-nearest-even, and the comparison is equality of bits.  One wrong pixel, one wrong channel quad or a
truncating conversion fails it.  The reference takes the ORIGINAL weights; the kernels take them through pack_conv_w.

  forward          conv3x3_ws_kernel<Fi, STATS, F32OUT>, all eight, every shape; statistics as sq[0], sq[1] of one allocation, as two
                   allocations (the other zeroing branch), as 8 replicas; with and without bias
  pooled forward   conv3x3_pool_fwd: the kernel it reports with and without Y, Y and Praw bit for bit on the exact inputs
  data gradient    the same kernels on dy with Wd, fp32 and bf16 output
  weight gradient  conv3x3_wgrad_kernel<Fi, 1> (atomics), <Fi, 2>+reduce (workspace), and the silent fall-back to atomics when the
                   workspace is one float short; dWp starts from non-zero values ("+=")
  children         conv3x3_kernel<Fi, 8>, <Fi, 4> (AUDIOSSL_CONV_WS=0), conv3x3_wgrad_kernel<Fi, 2> with atomics and <Fi, 1>+reduce
                   (AUDIOSSL_WGRAD_KG): the switches are read once per process, so one child process per environment
  isolation        tensors inside larger allocations with NaN (inputs) or a bit pattern (outputs) around them; one NaN image among
                   finite ones

Every launch must report the kernel it is meant to run (audiossl_last_kernel).  The launches and verdicts live in
tests/conv_matrix_child.py.  A child that dies - by a signal, an abort, at its time limit, or with its own exit status 70 for an error
of the HIP runtime - trips a latch: the later child tests fail at once without starting another GPU process.  No retries."""
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_cases as C

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SWITCHES = ("AUDIOSSL_CONV_WS", "AUDIOSSL_CONV_WAVES", "AUDIOSSL_WGRAD_KG")
_DEAD_STATUS = (134, 139, 124, 137, 70)
_dead = []
SHAPE_IDS = [C.shape_id(s) for s in C.SHAPES]


@pytest.fixture(scope="module")
def N():
    from src import _native
    _native.lib()
    assert torch.cuda.is_available()
    assert not any(os.environ.get(k) for k in _SWITCHES), "the default kernels need the conv switches unset"
    return _native


def default_wgrad_modes(fi):
    return [(None, C.wgrad_name(fi, 1, False)), ("full", C.wgrad_name(fi, 2, True)), ("short", C.wgrad_name(fi, 1, False))]


# ================================================================================= 1 - 3. the default kernels, in this process
@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_conv3x3_matrix_forward(N, shape):
    """conv3x3_ws_kernel<Fi, true | false, true | false>: Y bit for bit float64 (bf16: its round-to-nearest-even), the statistics
    the float64 sums of the stored tensor (rtol 1e-5, atol 1e-2 on the plain sum) in all three buffer flavours."""
    import conv_matrix_child as K
    names, bad, why = K.run_forward(N, shape, C.fwd_name)
    assert not why, "\n".join(why)
    assert bad == 0
    fi = shape[2]
    assert set(names) == {C.fwd_name(fi, st, f32) for st in (False, True) for f32 in (False, True)}


@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_conv3x3_matrix_data_gradient(N, shape):
    """conv3x3_ws_kernel<Fi, false, true> and <Fi, false, false> (dx_bf16) on dy with Wd: bit for bit conv2d_input in float64"""
    import conv_matrix_child as K
    names, bad, why = K.run_dgrad(N, shape, C.fwd_name)
    assert not why, "\n".join(why)
    assert bad == 0
    assert names == [C.fwd_name(shape[2], False, True), C.fwd_name(shape[2], False, False)]


@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_conv3x3_matrix_weight_gradient(N, shape):
    """conv3x3_wgrad_kernel<Fi, 1> (no workspace; a workspace one float short), <Fi, 2>+reduce (full workspace): dWp afterwards is
    bit for bit its starting value + conv2d_weight in float64; the workspace holds NaN wherever the launch has no business."""
    import conv_matrix_child as K
    fi = shape[2]
    names, bad, why = K.run_wgrad(N, shape, default_wgrad_modes(fi))
    assert not why, "\n".join(why)
    assert bad == 0
    assert names == [C.wgrad_name(fi, 1, False), C.wgrad_name(fi, 2, True), C.wgrad_name(fi, 1, False)]


@pytest.mark.parametrize("shape", [(2, 2, 32), (3, 8, 32), (2, 2, 16), (3, 16, 16)], ids=C.shape_id)
def test_conv3x3_matrix_pooled_forward(N, shape):
    """conv3x3_pool_fwd reports conv3x3_ws_kernel<Fi, true, false, 2, true, KEEP_Y> for the Y it is given or not; on the exact inputs Y
    is bit for bit the rounded float64 reference and Praw its 2x2 window maximum (gamma >= 0) or minimum (gamma < 0).  What else the
    pooled forms owe - sums, BatchNorm on the pooled map - is held to conv3x3_fwd by tests/test_gpu_conv_pool.py."""
    import conv_matrix_child as K
    n, ti, fi = shape
    c, r = C.inputs(shape), C.fwd_ref(shape, fp32_too=True)
    Wf, _ = K.packed_weights(N, c["w"])
    x, bias = c["x"].cuda(), c["bias"].cuda()
    gamma = torch.where(torch.arange(64) % 3 == 0, -1.0, 1.0)
    want = r["y"].bfloat16()
    win = want.float().view(n, ti // 2, 2, fi // 2, 2, 64)
    want_p = torch.where(gamma >= 0, win.amax((2, 4)), win.amin((2, 4))).bfloat16()
    for keep in (True, False):
        Y = K.nan_full((n, ti, fi, 64), torch.bfloat16) if keep else None
        Praw = K.nan_full((n, ti // 2, fi // 2, 64), torch.bfloat16)
        sq = K.nan_full((8, 128), torch.float64)
        N.call("conv3x3_pool_fwd", x, Wf, bias, gamma.cuda(), Y, Praw, sq[0], sq[0, 64:], 8, n, ti, fi)
        assert N.last_kernel() == f"conv3x3_ws_kernel<{fi}, true, false, 2, true, {'true' if keep else 'false'}>"
        torch.cuda.synchronize()
        assert Y is None or C.mismatches(Y, want.cuda()) == 0
        assert C.mismatches(Praw, want_p.cuda()) == 0, keep


# ================================================================================= 4. the kernels a switch selects: child processes
def _child(what, arg, env_set):
    if _dead:
        pytest.fail(f"not started: an earlier conv matrix child died ({_dead[0]})", pytrace=False)
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env.update(env_set)
    try:
        out = subprocess.run([sys.executable, os.path.join(_HERE, "conv_matrix_child.py"), what, str(arg)], env=env, capture_output=True,
                             text=True, timeout=180)
    except subprocess.TimeoutExpired:
        _dead.append(f"{what} {arg}: time limit")
        raise
    if out.returncode < 0 or out.returncode in _DEAD_STATUS:
        _dead.append(f"{what} {arg}: exit status {out.returncode}")
    assert out.returncode == 0, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
    rows = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    done = [r for r in rows if "done" in r]
    cases = [r for r in rows if "shape" in r]
    import conv_matrix_child as K
    want = [list(s) for s in K.child_shapes(what)]
    assert len(done) == 1 and [r["shape"] for r in cases] == want, "the child did not run to the end"
    print(f"{what} {arg}: {len(cases)} shapes, {sum(r['bad'] for r in cases)} mismatching elements, {done[0]['seconds']} s")
    return cases


@pytest.mark.parametrize("waves", [8, 4])
def test_conv3x3_matrix_lds_weights_kernel(waves):
    """AUDIOSSL_CONV_WS=0 (and AUDIOSSL_CONV_WAVES=4): conv3x3_kernel<Fi, 8> / <Fi, 4>, the fall-back of inputs past 2 GB - forward
    (both output types, with and without statistics) and data gradient, bit for bit float64."""
    env = {"AUDIOSSL_CONV_WS": "0"}
    if waves == 4:
        env["AUDIOSSL_CONV_WAVES"] = "4"
    cases = _child("fwd", waves, env)
    bad = [r for r in cases if r["bad"] or r["why"]]
    assert not bad, "\n".join(f"{r['shape']}: {r['why']}" for r in bad)
    for r in cases:
        assert r["kernels"] == [f"conv3x3_kernel<{r['shape'][2]}, {waves}>"] and r["bad"] == 0
    assert {k for r in cases for k in r["kernels"]} == {f"conv3x3_kernel<32, {waves}>", f"conv3x3_kernel<16, {waves}>"}


@pytest.mark.parametrize("kg", [2, 1])
def test_conv3x3_matrix_weight_gradient_forced_split(kg):
    """AUDIOSSL_WGRAD_KG=2 without a workspace: conv3x3_wgrad_kernel<Fi, 2>, both pixel halves through atomics;
    AUDIOSSL_WGRAD_KG=1 with one: conv3x3_wgrad_kernel<Fi, 1>+reduce, the fold of unsplit partial results."""
    cases = _child("wgrad", kg, {"AUDIOSSL_WGRAD_KG": str(kg)})
    bad = [r for r in cases if r["bad"] or r["why"]]
    assert not bad, "\n".join(f"{r['shape']}: {r['why']}" for r in bad)
    for r in cases:
        assert r["kernels"] == [C.wgrad_name(r["shape"][2], kg, kg == 1)] and r["bad"] == 0
    assert {k for r in cases for k in r["kernels"]} == {C.wgrad_name(fi, kg, kg == 1) for fi in (32, 16)}


# ================================================================================= 5. isolation
TILE = 256 * 64                       # elements of one tile
SENTINEL = {torch.bfloat16: 0x5A5A, torch.float32: 0x5A5A5A5A}


def _inside(t, fill):
    """-> (big, view): a copy of t (or, t = (shape, dtype), an output) that starts 16 bytes past a whole tile into a larger allocation and
    ends as far before its end.  fill = "nan": NaN around it (an input); "bits": the sentinel pattern around and in it (an output)."""
    shape, dtype = (t.shape, t.dtype) if isinstance(t, torch.Tensor) else t
    n = 1
    for d in shape:
        n *= d
    margin = TILE + 16 // torch.empty(0, dtype=dtype).element_size()
    big = torch.empty(n + 2 * margin, device="cuda", dtype=dtype)
    if fill == "nan":
        big.fill_(float("nan"))
    else:
        C.bits(big).fill_(SENTINEL[dtype])
    view = big[margin:margin + n].view(shape)
    if isinstance(t, torch.Tensor):
        view.copy_(t)
    assert view.data_ptr() % 16 == 0 and view.data_ptr() % 256 != 0 and view.is_contiguous()
    return big, view


def _margins_intact(big, view):
    n, margin = view.numel(), (big.numel() - view.numel()) // 2
    b = C.bits(big)
    return bool((b[:margin] == SENTINEL[big.dtype]).all() and (b[margin + n:] == SENTINEL[big.dtype]).all())


@pytest.mark.parametrize("shape", C.ISOLATION_SHAPES, ids=[C.shape_id(s) for s in C.ISOLATION_SHAPES])
def test_conv3x3_matrix_stays_inside_its_tensors(N, shape):
    """x, dy, Y and dWp as 16-byte-aligned interior slices of larger allocations - NaN around the inputs for more than a tile on
    each side, a bit pattern around the outputs: the results are those of the float64 reference (which the plain runs above equal)
    and the pattern is untouched.  Everything stays inside its own allocation."""
    import conv_matrix_child as K
    n, ti, fi = shape
    c, r, dw = C.inputs(shape), C.fwd_ref(shape, fp32_too=True), C.wgrad_ref(shape, fp32_too=True)
    Wf, Wd = K.packed_weights(N, c["w"])
    _, x = _inside(c["x"].cuda(), "nan")
    _, dy = _inside(c["dy"].cuda(), "nan")
    bias = c["bias"].cuda()
    for f32 in (0, 1):
        dt = torch.float32 if f32 else torch.bfloat16
        for stats in (False, True):
            big, Y = _inside(((n, ti, fi, 64), dt), "bits")
            sq = K.nan_full((2, 64), torch.float64)
            N.call("conv3x3_fwd", x, Wf, bias, Y, f32, sq[0] if stats else None, sq[1] if stats else None, 1, n, ti, fi)
            assert N.last_kernel() == C.fwd_name(fi, stats, bool(f32))
            torch.cuda.synchronize()
            assert C.mismatches(Y, r["y"].to(dt).cuda()) == 0, (dt, stats)
            assert _margins_intact(big, Y), (dt, stats)
        big, dx = _inside(((n, ti, fi, 64), dt), "bits")
        N.call("conv3x3_fwd", dy, Wd, None, dx, f32, None, None, 1, n, ti, fi)
        torch.cuda.synchronize()
        assert C.mismatches(dx, r["dx"].to(dt).cuda()) == 0, dt
        assert _margins_intact(big, dx), dt
    for flavour, expect in default_wgrad_modes(fi)[:2]:
        big, dWp = _inside(c["dw0"].cuda(), "bits")
        ws = None if flavour is None else K.nan_full((256 * C.WS_FLOATS,), torch.float32)
        N.call("conv3x3_wgrad", dy, x, dWp, ws, 0 if ws is None else ws.numel(), n, ti, fi)
        assert N.last_kernel() == expect
        dW = torch.zeros(64, 64, 3, 3, device="cuda")
        N.call("unpack_conv_dw", dWp.clone(), dW)
        torch.cuda.synchronize()
        assert C.mismatches(dW, dw.cuda()) == 0, flavour
        assert _margins_intact(big, dWp), flavour


@pytest.mark.parametrize("shape", C.ISOLATION_SHAPES, ids=[C.shape_id(s) for s in C.ISOLATION_SHAPES])
def test_conv3x3_matrix_one_nan_image_stays_alone(N, shape):
    """One image all NaN among finite neighbours, in the forward and the data gradient: every other image is bit for bit what the
    clean run gives (the halo rows a tile shares with the neighbouring image must be masked, not multiplied by zero), and the NaN
    image's own output is NaN throughout (it was read)."""
    import conv_matrix_child as K
    n, ti, fi = shape
    c = C.inputs(shape)
    Wf, Wd = K.packed_weights(N, c["w"])
    bias = c["bias"].cuda()
    for src, W, b in ((c["x"].cuda(), Wf, bias), (c["dy"].cuda(), Wd, None)):
        for f32 in (0, 1):
            dt = torch.float32 if f32 else torch.bfloat16
            clean = K.nan_full((n, ti, fi, 64), dt)
            N.call("conv3x3_fwd", src, W, b, clean, f32, None, None, 1, n, ti, fi)
            for sick in sorted({0, n // 2, n - 1}):
                xs = src.clone()
                xs[sick] = float("nan")
                Y = torch.zeros((n, ti, fi, 64), device="cuda", dtype=dt)
                N.call("conv3x3_fwd", xs, W, b, Y, f32, None, None, 1, n, ti, fi)
                assert N.last_kernel() == C.fwd_name(fi, False, bool(f32))
                torch.cuda.synchronize()
                others = [i for i in range(n) if i != sick]
                assert C.mismatches(Y[others], clean[others]) == 0, (dt, sick)
                assert bool(Y[sick].isnan().all()), (dt, sick)
