"""Diagnostic (GPU box): the UnFuSeD step next to the DeLoRes-S step (one more encoder pass, a 2048-wide Barlow head) in the same
process, both as graph replays at the same B and T, alternating run by run; median and min / max of the runs.

    python tools/unfused_bench.py [--batch 512] [--classes 585] [--steps 100] [--runs 5] [--only unfused]

`--only unfused` runs that step alone (for a `rocprofv3 --kernel-trace --stats -- python tools/unfused_bench.py --only unfused
--runs 1` trace: per-launch time of `unfused_loss_kernel` next to its algorithmic bytes, which this prints, and whatever
`at::native` kernels are left inside the replayed step)."""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import torch  # noqa: E402
from src.encoder import AudioNTT2020Task6  # noqa: E402

PRE = {"base_encoder": {"type": "AudioNTT2020Task6", "output_dim": 2048, "return_all_layers": True}, "projection_dim": 2048,
       "normalization": "mean_var", "input": {"type": "raw_wav", "sampling_rate": 16000, "length_wave": 0.95, "n_mels": 64}}


def make(which, C, prec):
    run = {"batch_size": 8, "precision": prec}
    if which == "unfused":
        from src.upstream.unfused.upstream_expert import Upstream_Expert
        cfg = {"run": run, "pretrain": dict(copy.deepcopy(PRE), task_label=C, alpha=0.7, beta=0.3, gamma=0.003)}
    else:
        from src.upstream.delores_s.upstream_expert import Upstream_Expert
        cfg = {"run": run, "pretrain": dict(copy.deepcopy(PRE), lambda_barlow=5e-5)}
        cfg["pretrain"]["base_encoder"]["return_all_layers"] = False
    torch.manual_seed(0)
    ex = Upstream_Expert(cfg, base_encoder=AudioNTT2020Task6).cuda().train()
    return ex, ex.graphed_step(ex.configure_optimizers(), eager_steps=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--classes", type=int, default=585)
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--only", default=None, choices=[None, "unfused", "delores_s"])
    a = ap.parse_args()
    B, C, T = a.batch, a.classes, a.frames
    x1, x2 = torch.randn(B, 1, 64, T, device="cuda"), torch.randn(B, 1, 64, T, device="cuda")
    names = [a.only] if a.only else ["unfused", "delores_s"]
    steps = {}
    for n in names:
        ex, st = make(n, C, a.precision)
        if n == "unfused":
            ex.set_labels(torch.randint(0, C, (B,)))
        for _ in range(a.warmup):
            loss = st(x1, x2)
        torch.cuda.synchronize()
        steps[n] = (ex, st, float(loss))
    times = {n: [] for n in names}
    for _ in range(a.runs):
        for n in names:
            st = steps[n][1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                st(x1, x2)
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / a.steps * 1e3)
    for n in names:
        ts = times[n]
        print(f"{n}: B={B} T={T} {a.precision} graph replay  median {statistics.median(ts):.3f} ms/step  "
              f"min {min(ts):.3f}  max {max(ts):.3f}  ({B / statistics.median(ts) * 1e3:.0f} clips/s, loss {steps[n][2]:.4f})")
    if "unfused" in names:
        ld = (C + 63) // 64 * 64
        gb = 2 if a.precision == "bf16" else 4
        print(f"unfused_loss_kernel algorithmic bytes: {4 * B * C * 4 / 1e6:.2f} MB read, {4 * B * ld * gb / 1e6:.2f} MB written "
              f"(C={C}, ld={ld}, {gb}-byte gradients)")


if __name__ == "__main__":
    main()
