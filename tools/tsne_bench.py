"""Diagnostic (GPU box): one t-SNE gradient evaluation of the fused path (`tsne_gradient`: exact repulsion over all pairs in one
kernel, nothing of size n x n stored) next to slabbed torch fp32 that forms w slab by slab on the same device, alternating run by
run, with the peak allocator growth of each; then the stages of the affinities and the wall time of a whole map.

    python tools/tsne_bench.py [--n 65536] [--d 128] [--centres 64] [--runs 5] [--slab 4096] [--iters 1000] [--perplexity 20]

Baseline: slabs of `slab` rows: y_slab against all of y by broadcasting (the [slab, n] matrices d2, w and w^2 are stored), Z in
float64 from the slab sums, the attraction through the same CSR with torch `index_add_`.  Points: `centres` Gaussian blobs,
PCA-whitened and L2-normalised the way the labeler prepares them (`preprocess_features`).  Prints one line per path: median / min /
max ms, peak MiB; the largest difference between the two gradients; the time of each stage of the affinities; the wall time of
`tsne` and what that is per iteration."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import torch  # noqa: E402
from src.evaluation.tsne import (_Stepper, neighbour_count, tsne, tsne_affinities, tsne_calibrate, tsne_symmetrize,  # noqa: E402
                                 tsne_workspace_bytes)
from src.evaluation.graph import knn_graph  # noqa: E402


def torch_gradient(P, y, exaggeration, slab):
    n = y.shape[0]
    rep = torch.empty_like(y)
    z = torch.zeros((), dtype=torch.float64, device=y.device)
    for i in range(0, n, slab):
        ys = y[i:i + slab]
        dx, dy = ys[:, None, 0] - y[None, :, 0], ys[:, None, 1] - y[None, :, 1]
        w = 1.0 / (1.0 + dx * dx + dy * dy)
        r = torch.arange(ys.shape[0], device=y.device)
        w[r, r + i] = 0.0
        z += w.sum(dtype=torch.float64)
        w2 = w * w
        rep[i:i + slab, 0], rep[i:i + slab, 1] = (w2 * dx).sum(1), (w2 * dy).sum(1)
    m = int(P.nnz[0])
    rows = torch.repeat_interleave(torch.arange(n, device=y.device), (P.rowptr[1:] - P.rowptr[:-1]).long())
    cols = P.col[:m].long()
    diff = y[rows] - y[cols]
    pw = P.w[:m] / (1.0 + (diff * diff).sum(1))
    att = torch.zeros_like(y).index_add_(0, rows, pw[:, None] * diff)
    return 4.0 * (exaggeration * att - (rep.double() / z).float())


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
    ap.add_argument("--centres", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--slab", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--perplexity", type=float, default=20.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench.py measures on the GPU; there is nothing to measure without one")
    from src.upstream.decar_v2.clustering import preprocess_features
    g = torch.Generator(device="cuda").manual_seed(a.n)
    c = 4.0 * torch.randn(a.centres, a.d, device="cuda", generator=g)
    x = c[torch.randint(a.centres, (a.n,), device="cuda", generator=g)] + torch.randn(a.n, a.d, device="cuda", generator=g)
    x = preprocess_features(x, pca=a.d)
    k = neighbour_count(a.n, a.perplexity)

    timed(lambda: tsne_affinities(x, a.perplexity))                  # warm-up
    t_graph, (idx, d2) = timed(lambda: knn_graph(x, k))
    t_cal, (pc, _) = timed(lambda: tsne_calibrate(d2, a.perplexity))
    t_sym, P = timed(lambda: tsne_symmetrize(idx, pc))
    print(f"n={a.n} d={a.d} perplexity={a.perplexity:g} k={k}: knn_graph {t_graph:.1f} ms, calibrate {t_cal:.1f} ms, symmetrize {t_sym:.1f} ms, "
          f"nnz {int(P.nnz[0])}, workspace {tsne_workspace_bytes(a.n, k) / 2 ** 20:.1f} MiB (affinities) / "
          f"{tsne_workspace_bytes(a.n) / 2 ** 20:.1f} MiB (iterations)")

    y = (3.0 * torch.randn(a.n, 2, generator=torch.Generator().manual_seed(1))).cuda()
    st = _Stepper(P, a.n, y.device)
    paths = {"fused": lambda: st.gradient(y, 1.0, False).clone(), "torch": lambda: torch_gradient(P, y, 1.0, a.slab)}
    outs = {p: timed(fn)[1] for p, fn in paths.items()}                # warm-up of every shape the timed window uses
    times = {p: [] for p in paths}
    for _ in range(a.runs):
        for p, fn in paths.items():
            times[p].append(timed(fn)[0])
    for p, fn in paths.items():
        ts = times[p]
        print(f"  gradient {p:6s} median {statistics.median(ts):10.3f} ms  min {min(ts):10.3f}  max {max(ts):10.3f}  peak {peak(fn):9.1f} MiB")
    rel = float((outs["fused"] - outs["torch"]).norm() / outs["torch"].norm())
    print(f"  |grad_fused - grad_torch| / |grad_torch| = {rel:.3e}")
    # the repulsion alone, by device events over `reps` back-to-back calls
    from src import _native as N
    reps = 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        N.call("tsne_repulsion", y, a.n, st.rep, st.z, st.ws, st.nbytes)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    pairs = float(a.n) * (a.n - 1)
    print(f"  repulsion alone {ms:.3f} ms per call ({reps} calls): {pairs / ms / 1e6:.1f} G pairs/s")

    runs = []
    for _ in range(max(1, min(a.runs, 3))):
        t, (_, kl) = timed(lambda: tsne(x, perplexity=a.perplexity, n_iter=a.iters, return_kl=True))
        runs.append(t)
    print(f"  tsne {a.iters} iterations: wall {statistics.median(runs) / 1e3:.3f} s median of {len(runs)} (min {min(runs) / 1e3:.3f}, max "
          f"{max(runs) / 1e3:.3f}), {statistics.median(runs) / max(a.iters, 1):.3f} ms per iteration all included, final KL {kl:.4f}")


if __name__ == "__main__":
    main()
