"""Diagnostic (GPU box): the fused silhouette (`silhouette_samples`: all pairs on the fp32 MFMA pipe, the per-cluster sums folded in
the kernel, nothing of size n x n or n x K stored) next to the obvious torch composition in the same process, alternating run by
run, with the peak allocator growth of each.

    python tools/silhouette_bench.py [--n 65536] [--d 128] [--centres 512] [--runs 5] [--slab 4096]

Baseline: slabs of `slab` rows, torch fp32 `mm` against all points, distances from the norms (clamped, the diagonal zeroed by
index, `sqrt`), then slab x one-hot [n, K] in float64 for the per-cluster sums - the slab's [slab, n] matrix and the [n, K] one-hot
are stored; a, b and s in float64 as the fused path forms them.  Labels: the nearest of `centres` random unit centres.
Prints one line per path: median / min / max ms, peak MiB; then the largest difference between the two results."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import torch  # noqa: E402
from src.evaluation import graph as G  # noqa: E402


def torch_silhouette(x, labels, slab):
    n = x.shape[0]
    _, inv, counts = torch.unique(labels, return_inverse=True, return_counts=True)
    K = counts.numel()
    onehot = torch.zeros(n, K, dtype=torch.float64, device=x.device)
    onehot[torch.arange(n, device=x.device), inv] = 1.0
    norms = (x * x).sum(1)
    sums = torch.empty(n, K, dtype=torch.float64, device=x.device)
    for i in range(0, n, slab):
        xs = x[i:i + slab]
        dist = (norms[i:i + slab, None] + norms[None, :] - 2.0 * (xs @ x.T)).clamp_(min=0).sqrt_()
        r = torch.arange(xs.shape[0], device=x.device)
        dist[r, r + i] = 0.0
        sums[i:i + slab] = dist.double() @ onehot
    rows = torch.arange(n, device=x.device)
    size = counts[inv]
    a = sums[rows, inv] / (size - 1).clamp_min(1)
    other = sums / counts[None, :]
    other[rows, inv] = float("inf")
    b = other.min(1).values
    s = torch.nan_to_num((b - a) / torch.maximum(a, b))
    s[size == 1] = 0.0
    return s


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del out
    return grown / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--centres", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--slab", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("silhouette_bench.py measures on the GPU; there is nothing to measure without one")
    g = torch.Generator(device="cuda").manual_seed(a.n)
    c = torch.nn.functional.normalize(torch.randn(a.centres, a.d, device="cuda", generator=g), dim=1)
    x = c[torch.randint(a.centres, (a.n,), device="cuda", generator=g)] + 0.15 * torch.randn(a.n, a.d, device="cuda", generator=g) / a.d ** 0.5
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    labels = (x @ c.T).argmax(1)
    sizes = torch.unique(labels, return_counts=True)[1]

    paths = {"fused": lambda: G.silhouette_samples(x, labels), "torch": lambda: torch_silhouette(x, labels, a.slab)}
    outs = {p: timed(fn)[1] for p, fn in paths.items()}                # warm-up of every shape the timed window uses
    print(f"n={a.n} d={a.d}: {sizes.numel()} clusters of {int(sizes.min())} .. {int(sizes.max())} members, "
          f"silhouette {float(outs['fused'].mean()):.6f}")
    times = {p: [] for p in paths}
    for _ in range(a.runs):
        for p, fn in paths.items():
            times[p].append(timed(fn)[0])
    for p, fn in paths.items():
        ts = times[p]
        print(f"  silhouette {p:6s} median {statistics.median(ts):10.3f} ms  min {min(ts):10.3f}  max {max(ts):10.3f}  peak {peak(fn):9.1f} MiB")
    print(f"  max |s_fused - s_torch| = {float((outs['fused'] - outs['torch']).abs().max()):.3e}")


if __name__ == "__main__":
    main()
