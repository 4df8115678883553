"""Diagnostic (GPU box): time the Kaldi fbank front end alone at B = 256 for 1 s and 10 s clips (128 mel bins, the finished
[B, 1, 128, T] network input: padding, masks and normalisation included), and - with --yardstick - the log-mel kernel at the same
B and 128 mel rows on 1 s clips, five times, for the per-frame comparison of DESIGN.md.

    python tools/fbank_bench.py [B] [--yardstick] [--runs N]
    rocprofv3 --kernel-trace --stats -d out -- python tools/fbank_bench.py --once     # one launch of each shape, no graphs
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd"), os.path.join(ROOT, "tools")]
import numpy as np, torch
from src import _native as N
from src.dataset.mast_dataset import KaldiFbank, plan_masks, AUDIOSET_MEAN, AUDIOSET_STD, PADDED, PREEMPH, EPS
from src.utils import MelSpectrogramLibrosa
from gemm_shapes import timeit

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args else 256
runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 5
once = "--once" in sys.argv
HBM = 8000.0   # GB/s


def waves(L):
    g = np.random.RandomState(0)
    t = np.arange(L) / 16000.0
    return torch.from_numpy((g.uniform(-0.1, 0.1, (B, L)) + 0.3 * np.sin(2 * np.pi * 440 * t)).astype(np.float32)).cuda()


fb = KaldiFbank(128)
win, tw, packed, starts = fb._tables(torch.device("cuda", torch.cuda.current_device()))
torch.manual_seed(0)
for L, T in ((16000, 98), (160000, 1024)):
    w = waves(L)
    out = torch.empty(B, 1, 128, T, device="cuda")
    bands_h = plan_masks(B, 128, T, 24, min(192, T // 4))
    bands = bands_h.cuda()
    launch = lambda: N.call("fbank_fwd", w, None, None, None, None, bands, bands_h.data_ptr(), out, B, L, fb.win_len, fb.shift, PADDED,
                            128, packed.shape[1], T, win, tw, packed, starts, PREEMPH, EPS, AUDIOSET_MEAN, AUDIOSET_STD, 0, 0)
    launch()
    torch.cuda.synchronize()
    if once:
        continue
    frames = B * min(T, fb.n_frames(L))
    byt = B * (4.0 * L + 4.0 * 128 * T)
    us = sorted(timeit(launch) for _ in range(runs))
    med = us[len(us) // 2]
    print(f"fbank B={B} L={L} T={T}: {med:.1f} us (min {us[0]:.1f} max {us[-1]:.1f} over {runs})  {med * 1e3 / frames:.2f} ns/frame  "
          f"{byt / med / 1e3:.1f} GB/s algorithmic ({byt / med / 1e3 / HBM:.4f} of 8 TB/s)  checksum {float(out.double().sum()):.6f}")

if "--yardstick" in sys.argv or once:
    # the yardstick timed the same way: tables and output allocated once, the bare entry point inside the graph
    mel = MelSpectrogramLibrosa(n_mels=128)
    w = waves(16000)
    T = mel.n_frames(16000)
    mwin, mtw, mpacked, mstarts = mel._tables(w.device)
    mout = torch.empty(B, 128, T, device="cuda")
    from src.utils.utils import F32_EPS, F64_EPS
    mlaunch = lambda: N.call("logmel_fwd", w, mout, B, 16000, T, mel.n_fft, mel.shift, 128, mpacked.shape[1], mwin, mtw, mpacked,
                             mstarts, np.float32(F64_EPS).item(), F32_EPS, 1)
    mlaunch()
    torch.cuda.synchronize()
    if not once:
        frames = B * T
        us = sorted(timeit(mlaunch) for _ in range(runs))
        med = us[len(us) // 2]
        print(f"logmel (yardstick) B={B} L=16000 n_mels=128 T={T} taps={mpacked.shape[1]}: {med:.1f} us "
              f"(min {us[0]:.1f} max {us[-1]:.1f} over {runs}, spread {(us[-1] - us[0]) / med:.3f})  {med * 1e3 / frames:.2f} ns/frame")
