"""Diagnostic (GPU box): the linear-probe grid (`src.evaluation.probe.LinearProbeGrid`: H heads trained together, five launches per
step) next to the obvious loop - per head one `nn.Linear`, `F.cross_entropy` and `torch.optim.AdamW` on the same device, the
standardised batch gathered once per step and shared by the heads.  Same data, same permutations, same cosine schedule.

    python tools/probe_bench.py --leg grid  [--n 65536 --d 2048 --classes 35 --epochs 10 --batch 1024 --runs 3]
    python tools/probe_bench.py --leg loop
    python tools/probe_bench.py --leg split          # the grid's step, split by launch (device events around every entry point)

One leg per process (from a job script: one `timeout`-bounded command each).  `grid` and `loop` print the wall time of a whole fit
(host clock, ends in a device synchronise; the first run is the warm-up and is listed apart), the allocator peak above the resident
[N, D] matrix, and the validation accuracy of every head, so that the two legs can be compared by eye: they train the same heads.
`split` prints median / min / max microseconds per launch over the steps of one epoch.  Nothing is asserted about which is faster."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import torch  # noqa: E402
from src import _native as N  # noqa: E402
from src.evaluation.probe import LinearProbeGrid, cosine_scale, epoch_permutations, feature_stats  # noqa: E402

LRS = [1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2]
WDS = [0.0, 1e-4, 1e-2]


def data(n, d, c, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn(c, d, device="cuda", generator=g) * 0.08
    y = torch.randint(0, c, (n + 4096,), device="cuda", generator=g)
    x = torch.randn(n + 4096, d, device="cuda", generator=g) + centres[y]
    return x[:n].contiguous(), y[:n].contiguous(), x[n:].contiguous(), y[n:].contiguous()


def fit_loop(X, y, stats, c, epochs, batch, seed):
    """The baseline: H separate torch heads.  -> list of (weight, bias) on the standardised features."""
    n, d = X.shape
    mean, rstd = stats
    hp = [(lr, wd) for lr in LRS for wd in WDS]
    heads = [torch.nn.Linear(d, c, device="cuda") for _ in hp]
    for h in heads:
        torch.nn.init.zeros_(h.weight)
        torch.nn.init.zeros_(h.bias)
    opts = [torch.optim.AdamW(h.parameters(), lr=lr, weight_decay=wd) for h, (lr, wd) in zip(heads, hp)]
    total, k = epochs * ((n + batch - 1) // batch), 0
    for perm in epoch_permutations(n, epochs, torch.Generator().manual_seed(seed)):
        order = perm.cuda()
        for i in range(0, n, batch):
            rows = order[i:i + batch]
            xb, yb = (X[rows] - mean) * rstd, y[rows]
            s = cosine_scale(k, total)
            for head, opt, (lr, _) in zip(heads, opts, hp):
                opt.param_groups[0]["lr"] = lr * s
                opt.zero_grad(set_to_none=True)
                torch.nn.functional.cross_entropy(head(xb), yb).backward()
                opt.step()
            k += 1
    return heads


def accuracy_loop(heads, Xv, yv, stats):
    xs = (Xv - stats[0]) * stats[1]
    with torch.no_grad():
        return [float((h(xs).argmax(1) == yv).float().mean()) for h in heads]


def measure(fn, runs):
    times, peak, out = [], 0, None
    for _ in range(runs + 1):
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        peak = max(peak, torch.cuda.max_memory_allocated() - before)
    return times, peak / 2 ** 20, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("grid", "loop", "split"), required=True)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=35)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_bench.py measures on the GPU; there is nothing to measure without one")
    X, y, Xv, yv = data(a.n, a.d, a.classes)
    stats = feature_stats(X)
    steps = a.epochs * ((a.n + a.batch - 1) // a.batch)
    print(f"N={a.n} D={a.d} C={a.classes} heads={len(LRS) * len(WDS)} epochs={a.epochs} batch={a.batch} ({steps} steps per fit)")
    if a.leg == "grid":
        def run():
            grid = LinearProbeGrid(a.d, a.classes, LRS, WDS, stats=stats)
            return grid.fit(X, y, a.epochs, a.batch, generator=torch.Generator().manual_seed(1))
        times, peak, grid = measure(run, a.runs)
        acc = [r["top1"] for r in grid.evaluate(Xv, yv)]
    elif a.leg == "loop":
        times, peak, heads = measure(lambda: fit_loop(X, y, stats, a.classes, a.epochs, a.batch, 1), a.runs)
        acc = accuracy_loop(heads, Xv, yv, stats)
    else:
        grid = LinearProbeGrid(a.d, a.classes, LRS, WDS, stats=stats)
        grid.fit(X, y, 1, a.batch, generator=torch.Generator().manual_seed(1))           # warm-up of every shape
        N.PROFILE, N.PROFILE_ALL = {}, True
        grid.fit(X, y, 1, a.batch, generator=torch.Generator().manual_seed(2))
        torch.cuda.synchronize()
        prof, N.PROFILE, N.PROFILE_ALL = N.PROFILE, None, False
        rows = {}
        for name, evs in prof.items():
            if name == "audiossl_gemm":                       # the two GEMMs alternate: logits first, dW second
                rows["gemm logits"] = [e0.elapsed_time(e1) for e0, e1, *_ in evs[0::2]]
                rows["gemm dW"] = [e0.elapsed_time(e1) for e0, e1, *_ in evs[1::2]]
            else:
                rows[name[len("audiossl_"):]] = [e0.elapsed_time(e1) for e0, e1, *_ in evs]
        total = sum(statistics.median(v) for v in rows.values())
        for name, v in rows.items():
            print(f"  {name:14s} median {1e3 * statistics.median(v):8.1f} us  min {1e3 * min(v):8.1f}  max {1e3 * max(v):8.1f}  "
                  f"({100 * statistics.median(v) / total:4.1f} % of the medians' sum, {len(v)} launches)")
        print(f"  sum of medians {1e3 * total:8.1f} us per step (device events around each entry point; host gaps not included)")
        return
    print(f"  {a.leg}: warm-up fit {times[0]:.3f} s; fits " + ", ".join(f"{t:.3f}" for t in times[1:]) +
          f" s (median {statistics.median(times[1:]):.3f} s, {1e3 * statistics.median(times[1:]) / steps:.3f} ms per step); "
          f"allocator peak above the resident data {peak:.1f} MiB")
    print("  validation top1 per head: " + " ".join(f"{v:.4f}" for v in acc))


if __name__ == "__main__":
    main()
