"""Diagnostic (GPU box): what the packed PCM upload (`run.pcm_upload`) costs and saves against the float32 batch, part by part.

  collate   host time to build one batch from decoded clips: zeroed float32 [B, unit] filled clip by clip and pinned (WindowCollate)
            against `PcmBatch.pack` into one pinned buffer
  upload    pinned host -> device copy of either batch (device events around the copy)
  kernel    `audiossl_pcm_window` at B = 512 x 16000 mono s16, B = 256 x 160000 mono s16 and B = 512 x 16000 stereo s16, each next
            to `audiossl_cast` (F32 -> BF16: the project's streaming yardstick, 4 bytes in and 2 out per element where the mono
            kernel has 2 in and 4 out) over the same number of output elements
  both      upload + convert against the float32 upload, each as one event-timed sequence on one stream

Every pair is measured in alternation, `--runs` times (default 5); a line gives the median and the min / max over the runs.

    python tools/ingest_bench.py [--runs N] [--skip-host]
    rocprofv3 --kernel-trace --stats -d out -- python tools/ingest_bench.py --once     # one launch of each kernel shape, no graphs
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd"), os.path.join(ROOT, "tools")]
import numpy as np, torch
from src import _native as N
from src.dataset import ingest
from gemm_shapes import timeit

runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 5
once = "--once" in sys.argv
HBM = 8000.0   # GB/s


def clips(B, n, C, seed=0):
    g = np.random.RandomState(seed)
    return [ingest.PcmClip(g.randint(-32768, 32768, (n,) if C == 1 else (n, C)).astype(np.int16), 16000) for _ in range(B)]


def line(name, us, extra=""):
    us = sorted(us)
    med = us[len(us) // 2]
    print(f"{name}: {med:.1f} us (min {us[0]:.1f} max {us[-1]:.1f} over {len(us)}, spread {(us[-1] - us[0]) / med:.3f}){extra}", flush=True)
    return med


def float_collate(waves, starts, unit):
    """`WindowCollate.__call__`'s batch assembly plus `_CollatedLoader`'s pinning."""
    out = torch.zeros(len(waves), unit, dtype=torch.float32)
    for b, w in enumerate(waves):
        n = len(w)
        if n >= unit:
            out[b] = w[starts[b]:starts[b] + unit]
        else:
            left = (unit - n) // 2
            out[b, left:left + n] = w
    return out.pin_memory()


def events(fn, reps=10):
    """Mean time of fn() over `reps` calls between two device events on the current stream, in us."""
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


# ---- kernel: pcm_window next to cast over the same number of output elements
for name, B, unit, C in (("mono s16", 512, 16000, 1), ("mono s16", 256, 160000, 1), ("stereo s16", 512, 16000, 2)):
    one = clips(1, unit, C)[0]
    batch = ingest.PcmBatch.pack([one] * B, [0] * B, unit).cuda()
    out = torch.empty(B, unit, dtype=torch.float32, device="cuda")
    src = torch.randn(B * unit, device="cuda")
    dst = torch.empty(B * unit, dtype=torch.bfloat16, device="cuda")
    tb, dev = ingest.PcmBatch.table_bytes(B), batch._dev           # the bare entry point inside the graph, as the yardstick
    k_pcm = lambda: N.call("pcm_window", dev.data_ptr() + tb, dev.numel() - tb, dev.data_ptr(), batch._host.data_ptr(), out, B, unit, 0)
    k_cast = lambda: N.call("cast", N.BF16, src, dst, B * unit)
    k_pcm(); k_cast(); torch.cuda.synchronize()
    if once:
        continue
    want = torch.from_numpy(one.to_float()).cuda()
    assert torch.equal(out[0], want) and torch.equal(out[B - 1], want)
    t_pcm, t_cast = [], []
    for _ in range(runs):
        t_pcm.append(timeit(k_pcm)); t_cast.append(timeit(k_cast))
    by_pcm, by_cast = B * unit * (2.0 * C + 4.0), B * unit * 6.0
    m = line(f"pcm_window {name} B={B} unit={unit}", t_pcm, f"  {by_pcm / 1e6:.1f} MB")
    print(f"    {by_pcm / m / 1e3:.0f} GB/s ({by_pcm / m / 1e3 / HBM:.3f} of 8 TB/s)")
    m = line(f"cast f32->bf16 n={B * unit}", t_cast, f"  {by_cast / 1e6:.1f} MB")
    print(f"    {by_cast / m / 1e3:.0f} GB/s ({by_cast / m / 1e3 / HBM:.3f} of 8 TB/s)")
    del batch, out, src, dst
if once:
    sys.exit(0)

# ---- upload, and upload + convert, B = 512 x 1 s and B = 256 x 10 s
for B, unit in ((512, 16000), (256, 160000)):
    cl = clips(B, unit, 1, seed=1)
    batch = ingest.PcmBatch.pack(cl, [0] * B, unit)
    fl = torch.stack([torch.from_numpy(c.to_float()) for c in cl]).pin_memory()
    out = torch.empty(B, unit, dtype=torch.float32, device="cuda")
    up_f = lambda: fl.to("cuda", non_blocking=True)
    up_p = lambda: batch.to("cuda", non_blocking=True)
    both = lambda: ingest.pcm_window(batch.to("cuda", non_blocking=True), out=out)
    t = {"f": [], "p": [], "b": []}
    for _ in range(runs):
        t["f"].append(events(up_f)); t["p"].append(events(up_p)); t["b"].append(events(both))
    assert torch.equal(out, fl.cuda())
    mf = line(f"upload float32 B={B} unit={unit}", t["f"], f"  {fl.numel() * 4 / 1e6:.1f} MB")
    mp = line(f"upload packed  B={B} unit={unit}", t["p"], f"  {batch.nbytes / 1e6:.1f} MB")
    mb = line(f"upload packed + pcm_window B={B} unit={unit}", t["b"])
    print(f"    packed / float32 upload {mp / mf:.3f}, upload + convert / float32 upload {mb / mf:.3f}")
    del batch, fl, out

# ---- host collate, B = 512 windows of 1 s cut from 4 s clips
if "--skip-host" not in sys.argv:
    B, unit = 512, 16000
    cl = clips(B, 4 * unit, 1, seed=2)
    fw = [torch.from_numpy(c.to_float()) for c in cl]
    starts = np.random.RandomState(3).randint(0, 3 * unit, B)
    t_f, t_p = [], []
    for _ in range(runs):
        for fn, acc in ((lambda: float_collate(fw, starts, unit), t_f), (lambda: ingest.PcmBatch.pack(cl, starts, unit), t_p)):
            fn()
            t0 = time.perf_counter()
            for _ in range(5): fn()
            acc.append((time.perf_counter() - t0) / 5 * 1e6)
    mf = line(f"collate float32 B={B} unit={unit} (zeros, fill, pin)", t_f)
    mp = line(f"collate packed  B={B} unit={unit} (PcmBatch.pack)", t_p)
    print(f"    packed / float32 collate {mp / mf:.3f}")
