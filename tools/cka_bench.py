"""Diagnostic (GPU box): the fused CKA path (`src.evaluation.cka.hsic_terms`: column centring, the median rule, one sweep over
the Gram tiles on the fp32 MFMA pipe, no n x n matrix) next to the obvious composition in the same process - torch fp32 `mm`
for both Gram matrices, centring, product-sum - alternating run by run, with the peak allocator growth of each.

    python tools/cka_bench.py [--n 8192] [--p 2048] [--q 512] [--runs 5] [--iters 3]

Prints one line per path and kernel: median / min / max ms per call, algorithmic TFLOP/s of one pass over both Gram matrices
(2 n^2 (p + q) over the time; the RBF median rule recomputes the tiles in its three select passes, which this figure does not
count), peak MiB, and the difference between the two CKA values."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import torch  # noqa: E402
from src.evaluation.cka import hsic_terms  # noqa: E402


def _center_gram(k):
    return k - k.mean(0, keepdim=True) - k.mean(1, keepdim=True) + k.mean()


def _rbf(g, sigma):
    d = torch.diagonal(g)
    dist = (d[:, None] + d[None, :] - 2.0 * g).clamp_(min=0)
    if sigma is None:
        v = torch.sort(dist[dist != 0]).values
        m = v.numel()
        s2 = (v[(m - 1) // 2].double() + v[m // 2].double()) / 2
    else:
        s2 = torch.tensor(float(sigma) ** 2, dtype=torch.float64, device=g.device)
    return torch.exp(dist * (-0.5 / s2).float())


def baseline(x, y, kernel, sigma=None):
    """torch fp32: both n x n matrices stored, centred, multiplied and summed (fp64 sums)."""
    x, y = x - x.mean(0, keepdim=True), y - y.mean(0, keepdim=True)
    k, l = x @ x.T, y @ y.T
    if kernel == "rbf":
        k, l = _rbf(k, sigma), _rbf(l, sigma)
    k, l = _center_gram(k), _center_gram(l)
    xy, xx, yy = (k * l).sum(dtype=torch.float64), (k * k).sum(dtype=torch.float64), (l * l).sum(dtype=torch.float64)
    return xy / torch.sqrt(xx * yy)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


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
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--p", type=int, default=2048)
    ap.add_argument("--q", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cka_bench.py measures on the GPU; there is nothing to measure without one")
    g = torch.Generator(device="cuda").manual_seed(a.n)
    z = torch.randn(a.n, 16, device="cuda", generator=g)
    x = z @ torch.randn(16, a.p, device="cuda", generator=g) + torch.randn(a.n, a.p, device="cuda", generator=g) + 1.0
    y = z @ torch.randn(16, a.q, device="cuda", generator=g) + torch.randn(a.n, a.q, device="cuda", generator=g) - 0.5
    flop = 2.0 * a.n * a.n * (a.p + a.q)
    for kernel in ("linear", "rbf"):
        paths = {"fused hsic_terms": lambda: hsic_terms(x, y, kernel)[0], "torch mm + centring": lambda: baseline(x, y, kernel)}
        f, b = float(paths["fused hsic_terms"]()), float(paths["torch mm + centring"]())
        print(f"n={a.n} p={a.p} q={a.q} {kernel}: cka fused {f:.9f} torch {b:.9f} diff {abs(f - b):.2e}")
        for fn in paths.values():                     # warm-up of every shape the timed window uses
            timed(fn, 1)
        times = {n: [] for n in paths}
        for _ in range(a.runs):
            for n, fn in paths.items():
                times[n].append(timed(fn, a.iters))
        for n, fn in paths.items():
            ts = times[n]
            med = statistics.median(ts)
            print(f"  {n:20s} median {med:9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}  {flop / med / 1e9:7.1f} TFLOP/s  "
                  f"peak {peak(fn):8.1f} MiB")


if __name__ == "__main__":
    main()
