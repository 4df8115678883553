"""Diagnostic (GPU box): the fused graph + PIC path (`knn_graph` on the fp32 MFMA pipe with the top-k reduced in the kernel, then
`pic_build` / `pic_power` / `pic_assign`) next to the obvious torch composition in the same process, alternating run by run,
with the peak allocator growth of each.

    python tools/pic_bench.py [--n 65536] [--d 128] [--nnn 5] [--centres 512] [--runs 5] [--slab 4096]

Baseline.  Graph: slabs of `slab` rows, torch fp32 `mm` against all points, distances from the norms, the diagonal masked by
index, `topk(nnn, largest=False)` - the slab's [slab, n] matrix is stored.  Iteration: W = A + A^T as a coalesced torch sparse
CSR tensor in float64, 200 rounds of `torch.mv`, the shift and the normalisation as torch ops.  There is no torch counterpart of
the walk to the maxima short of Python loops, so `pic_assign` is timed alone and the baseline column is empty for it.
Prints one line per stage and path: median / min / max ms, peak MiB; then the share of rows whose neighbour lists agree and the
largest relative difference of v."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import torch  # noqa: E402
from src.evaluation import graph as G  # noqa: E402

SIGMA, ALPHA, ITERS = 0.2, 0.001, 200


def torch_graph(x, k, slab):
    n = x.shape[0]
    norms = (x * x).sum(1)
    idx = torch.empty(n, k, dtype=torch.int64, device=x.device)
    d2 = torch.empty(n, k, dtype=torch.float32, device=x.device)
    for i in range(0, n, slab):
        xs = x[i:i + slab]
        dist = (norms[i:i + slab, None] + norms[None, :] - 2.0 * (xs @ x.T)).clamp_(min=0)
        r = torch.arange(xs.shape[0], device=x.device)
        dist[r, r + i] = float("inf")
        v, j = dist.topk(k, dim=1, largest=False)
        idx[i:i + slab], d2[i:i + slab] = j, v
    return idx, d2


def torch_matrix(idx, d2):
    n, k = idx.shape
    a = torch.exp(-d2.double() / SIGMA ** 2).reshape(-1)
    rows = torch.arange(n, device=idx.device).repeat_interleave(k)
    cols = idx.reshape(-1)
    w = torch.sparse_coo_tensor(torch.stack([torch.cat([rows, cols]), torch.cat([cols, rows])]), torch.cat([a, a]), (n, n))
    return w.coalesce().to_sparse_csr()


def torch_power(w):
    n = w.shape[0]
    v = torch.full((n,), 1.0 / n, dtype=torch.float64, device=w.device)
    for _ in range(ITERS):
        u = ALPHA * torch.mv(w, v) + (1.0 - ALPHA) / n
        v = u / u.sum()
    return v


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
    ap.add_argument("--nnn", type=int, default=5)
    ap.add_argument("--centres", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--slab", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pic_bench.py measures on the GPU; there is nothing to measure without one")
    g = torch.Generator(device="cuda").manual_seed(a.n)
    c = torch.nn.functional.normalize(torch.randn(a.centres, a.d, device="cuda", generator=g), dim=1)
    x = c[torch.randint(a.centres, (a.n,), device="cuda", generator=g)] + 0.15 * torch.randn(a.n, a.d, device="cuda", generator=g) / a.d ** 0.5
    x = torch.nn.functional.normalize(x, dim=1).contiguous()

    idx, d2 = G.knn_graph(x, a.nnn)
    W = G.pic_build(idx, d2, SIGMA)
    v = G.pic_power(W, ALPHA, ITERS)
    tw = torch_matrix(idx, d2)
    stages = [
        ("graph", lambda: G.knn_graph(x, a.nnn), lambda: torch_graph(x, a.nnn, a.slab)),
        ("matrix W", lambda: G.pic_build(idx, d2, SIGMA), lambda: torch_matrix(idx, d2)),
        ("200 iterations", lambda: G.pic_power(W, ALPHA, ITERS), lambda: torch_power(tw)),
        ("assign", lambda: G.pic_assign(W, v), None),
    ]
    print(f"n={a.n} d={a.d} nnn={a.nnn}: nnz {int(W.nnz)}, {int(G.pic_assign(W, v)[1])} raw clusters")
    for name, fused, base in stages:
        paths = {"fused": fused} if base is None else {"fused": fused, "torch": base}
        for fn in paths.values():
            timed(fn)                                 # warm-up of every shape the timed window uses
        times = {p: [] for p in paths}
        for _ in range(a.runs):
            for p, fn in paths.items():
                times[p].append(timed(fn)[0])
        for p, fn in paths.items():
            ts = times[p]
            print(f"  {name:15s} {p:6s} median {statistics.median(ts):10.3f} ms  min {min(ts):10.3f}  max {max(ts):10.3f}  "
                  f"peak {peak(fn):9.1f} MiB")
    ti, _ = torch_graph(x, a.nnn, a.slab)
    same = (idx.sort(1).values == ti.sort(1).values).all(1).float().mean()
    tv = torch_power(tw)
    print(f"  neighbour lists equal as sets in {float(same) * 100:.3f} % of rows; max |v - v_torch| / v = {float(((v - tv).abs() / tv).max()):.2e}")


if __name__ == "__main__":
    main()
