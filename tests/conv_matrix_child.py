"""The launches of the exact 3x3 convolution cases (conv_cases.py) and their verdicts, shared by tests/test_gpu_conv_matrix.py (in
its own process: the default kernels) and by the child processes it starts for the kernels that a switch selects - the switches are
read once per process:

    python conv_matrix_child.py fwd <waves>      AUDIOSSL_CONV_WS=0 [AUDIOSSL_CONV_WAVES=4]: conv3x3_kernel<Fi, waves>, forward and
                                                 data gradient, both output types, with and without statistics
    python conv_matrix_child.py wgrad <kg>       AUDIOSSL_WGRAD_KG=2: atomics with the pixel split; =1: two-stage without it

One JSON line per shape - the kernels the launches reported and the number of elements whose bits differ from the float64 reference -
and a closing line {"done": shapes, "seconds": t}.  Exit status 0 means "ran to the end", whatever the verdicts; an error of the HIP
runtime ends the run at once with status 70 (nothing more is started on a GPU that has reported a fault).

Every run_* function returns (kernel names, mismatching elements, other complaints as strings)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "audio-ssl_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import torch

import conv_cases as C

FATAL_STATUS = 70
NAN = float("nan")


def nan_full(shape, dtype):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


def packed_weights(N, w):
    """-> Wf, Wd (bf16 [64][576]) from the ORIGINAL weights, through pack_conv_w (dtype 1 = bf16)"""
    Wf = torch.empty(64, 576, device="cuda", dtype=torch.bfloat16)
    Wd = torch.empty_like(Wf)
    N.call("pack_conv_w", 1, w.cuda(), Wf, Wd)
    return Wf, Wd


def _stats_complaints(tag, s, q, Y):
    """the statistics against float64 sums of the tensor as stored (tolerances of test_conv3x3_implicit_gemm_fwd_dgrad_wgrad)"""
    Yd = Y.double()
    out = []
    try:
        np.testing.assert_allclose(s.cpu().numpy(), Yd.sum((0, 1, 2)).cpu().numpy(), rtol=1e-5, atol=1e-2)
        np.testing.assert_allclose(q.cpu().numpy(), (Yd ** 2).sum((0, 1, 2)).cpu().numpy(), rtol=1e-5)
    except AssertionError as e:
        out.append(f"{tag}: statistics {' '.join(str(e).split())[:300]}")
    return out


def stat_buffers(mode):
    """-> (sum, sumsq, stat_replicas, fold, guards): NaN-filled statistics buffers of one flavour; fold() -> (sums, sums of squares)
    after the launch; guards() -> True while the doubles next to the buffers still hold their NaN"""
    if mode == "pair":                       # sq[0], sq[1] of one allocation: sumsq == sum + 64, zeroed in one piece
        sq = nan_full((4, 64), torch.float64)
        return sq[1], sq[2], 1, lambda: (sq[1], sq[2]), lambda: bool(sq[0].isnan().all() and sq[3].isnan().all())
    if mode == "split":                      # two allocations: the other zeroing branch
        s, q = nan_full((3, 64), torch.float64), nan_full((3, 64), torch.float64)
        assert q[1].data_ptr() != s[1].data_ptr() + 512
        return s[1], q[1], 1, lambda: (s[1], q[1]), lambda: bool(s[0].isnan().all() and s[2].isnan().all() and q[0].isnan().all() and q[2].isnan().all())
    assert mode == "rep8"                    # 8 replicas [8][128], folded in float64
    sq = nan_full((10, 128), torch.float64)
    return sq[1], sq[1, 64:], 8, lambda: (sq[1:9, :64].sum(0), sq[1:9, 64:].sum(0)), lambda: bool(sq[0].isnan().all() and sq[9].isnan().all())


def run_forward(N, shape, name_of, fp32_too=True):
    """conv3x3_fwd on x with Wf: {bf16, fp32 output} x {no statistics, the three statistics flavours} with bias, and without bias
    with and without statistics.  Y is pre-filled with NaN.  name_of(fi, stats, f32) = the kernel the launch must report."""
    n, ti, fi = shape
    c, r = C.inputs(shape), C.fwd_ref(shape, fp32_too=fp32_too)
    x, bias = c["x"].cuda(), c["bias"].cuda()
    Wf, _ = packed_weights(N, c["w"])
    names, bad, why = [], 0, []
    for f32 in (0, 1):
        dt = torch.float32 if f32 else torch.bfloat16
        for b, ref in ((bias, r["y"]), (None, r["y0"])):
            want = ref.to(dt).cuda()                                   # bf16: round to nearest even
            for mode in (None, "pair", "split", "rep8") if b is not None else (None, "pair"):
                tag = f"{'fp32' if f32 else 'bf16'} {'bias' if b is not None else 'no bias'} {mode or 'no statistics'}"
                Y = nan_full((n, ti, fi, 64), dt)
                s, q, rep, fold, guards = stat_buffers(mode) if mode else (None, None, 1, None, None)
                N.call("conv3x3_fwd", x, Wf, b, Y, f32, s, q, rep, n, ti, fi)
                name = N.last_kernel()
                torch.cuda.synchronize()
                names.append(name)
                if name != name_of(fi, mode is not None, bool(f32)):
                    why.append(f"{tag}: ran {name}")
                k = C.mismatches(Y, want)
                if k:
                    bad += k
                    why.append(f"{tag}: {k} elements differ")
                if mode:
                    if not guards():
                        why.append(f"{tag}: doubles next to the statistics were written")
                    why += _stats_complaints(tag, *fold(), Y)
    return names, bad, why


def run_dgrad(N, shape, name_of, fp32_too=True):
    """the data gradient: conv3x3_fwd on dy with Wd, no bias, fp32 and bf16 (dx_bf16) output, against conv2d_input"""
    n, ti, fi = shape
    c, r = C.inputs(shape), C.fwd_ref(shape, fp32_too=fp32_too)
    dy = c["dy"].cuda()
    _, Wd = packed_weights(N, c["w"])
    names, bad, why = [], 0, []
    for f32 in (1, 0):
        dt = torch.float32 if f32 else torch.bfloat16
        dx = nan_full((n, ti, fi, 64), dt)
        N.call("conv3x3_fwd", dy, Wd, None, dx, f32, None, None, 1, n, ti, fi)
        name = N.last_kernel()
        torch.cuda.synchronize()
        names.append(name)
        if name != name_of(fi, False, bool(f32)):
            why.append(f"dgrad {dt}: ran {name}")
        k = C.mismatches(dx, r["dx"].to(dt).cuda())
        if k:
            bad += k
            why.append(f"dgrad {dt}: {k} elements differ")
    return names, bad, why


def run_wgrad(N, shape, modes, fp32_too=True):
    """conv3x3_wgrad into a dWp that starts from dw0.  modes: (workspace flavour, kernel the launch must report) with the flavours
    None (fp32 atomics), "full" (256 partial results, NaN-filled: what the launch does not use must stay NaN) and "short" (one float
    less than the launch needs, NaN-filled: the launch must fall back to atomics and leave it alone)."""
    n, ti, fi = shape
    c, want = C.inputs(shape), C.wgrad_ref(shape, fp32_too=fp32_too).cuda()
    x, dy = c["x"].cuda(), c["dy"].cuda()
    grid = min(C.tiles(shape), 256)
    names, bad, why = [], 0, []
    for flavour, expect in modes:
        ws = None if flavour is None else nan_full((256 * C.WS_FLOATS if flavour == "full" else grid * C.WS_FLOATS - 1,), torch.float32)
        dWp = c["dw0"].cuda().clone()
        N.call("conv3x3_wgrad", dy, x, dWp, ws, 0 if ws is None else ws.numel(), n, ti, fi)
        name = N.last_kernel()
        dW = torch.zeros(64, 64, 3, 3, device="cuda")
        N.call("unpack_conv_dw", dWp, dW)
        torch.cuda.synchronize()
        names.append(name)
        tag = f"workspace {flavour}"
        if name != expect:
            why.append(f"{tag}: ran {name}, expected {expect}")
        k = C.mismatches(dW, want)
        if k:
            bad += k
            why.append(f"{tag}: {k} elements differ")
        if flavour == "short" and not bool(ws.isnan().all()):
            why.append(f"{tag}: the workspace that is too small was written")
        if flavour == "full" and expect.endswith("+reduce"):
            if not bool(ws[grid * C.WS_FLOATS:].isnan().all()):
                why.append(f"{tag}: floats past the {grid} partial results were written")
            if bool(ws[:grid * C.WS_FLOATS].isnan().any()):
                why.append(f"{tag}: a partial result was left unwritten")
    return names, bad, why


def child_shapes(what):
    """the forward children leave out the two 513-tile shapes (their references alone take as long as the rest together)"""
    return [s for s in C.SHAPES if what == "wgrad" or C.tiles(s) <= 257]


def main(what, arg):
    from src import _native as N
    N.lib()
    t0 = time.time()
    done = 0
    for shape in child_shapes(what):
        if what == "fwd":
            name_of = lambda fi, stats, f32: f"conv3x3_kernel<{fi}, {arg}>"
            n1, b1, w1 = run_forward(N, shape, name_of, fp32_too=False)
            n2, b2, w2 = run_dgrad(N, shape, name_of, fp32_too=False)
            names, bad, why = n1 + n2, b1 + b2, w1 + w2
        else:
            kg = int(arg)
            mode = (None, C.wgrad_name(shape[2], 2, False)) if kg == 2 else ("full", C.wgrad_name(shape[2], 1, True))
            names, bad, why = run_wgrad(N, shape, [mode], fp32_too=False)
        print(json.dumps(dict(shape=list(shape), kernels=sorted(set(names)), bad=bad, why=why)), flush=True)
        done += 1
    print(json.dumps(dict(done=done, seconds=round(time.time() - t0, 1))), flush=True)


if __name__ == "__main__":
    try:
        main(sys.argv[1], sys.argv[2])
    except RuntimeError as e:                     # a failed launch, a HIP error at the synchronize: nothing more on this GPU
        print(json.dumps(dict(fatal=" ".join(str(e).split())[:500])), flush=True)
        sys.exit(FATAL_STATUS)
