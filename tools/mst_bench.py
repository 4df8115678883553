"""Diagnostic (GPU box): the mutual-reachability spanning tree (`audiossl_mreach_mst`) next to its yardstick, one `knn_graph_l2`
call with k = 1 on the same input - the same pass over the Gram tiles, once - alternating run by run; then the whole `hdbscan`
call with its host stage.

    python tools/mst_bench.py [--n 65536] [--d 128 2048] [--centres 512] [--planted 2000] [--min_samples 1 5] [--runs 5]
                              [--min_cluster_size 25]

Data.  Unit rows around `centres` centres, every row with its own noise scale (clusters of different density), plus a planted
block of `planted` identical rows (every weight inside it is 0: the heaviest tie there is).
Prints per (d, min_samples): the Boruvka rounds that did work of the ceil(log2 n) issued, the entry point's time (median / min /
max ms), the time per working round (total / rounds: every working round walks all tiles, so the rounds cost the same), the
yardstick, the ratio round / yardstick, the fp32 MFMA rate of a round (2 n^2 d flop), the allocator's peak growth over one
`mutual_reachability_mst` call, and the time of `hdbscan` end to end with what it found."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import torch  # noqa: E402
from src import _native as N  # noqa: E402
from src.evaluation import graph as G  # noqa: E402
from src.evaluation import hdbscan as H  # noqa: E402

PEAK_F32_MFMA_TF = 155.0


def make_data(n, d, centres, planted):
    g = torch.Generator(device="cuda").manual_seed(n + d)
    c = torch.nn.functional.normalize(torch.randn(centres, d, device="cuda", generator=g), dim=1)
    scale = 0.05 + 0.25 * torch.rand(n, 1, device="cuda", generator=g)
    x = c[torch.randint(centres, (n,), device="cuda", generator=g)] + scale * torch.randn(n, d, device="cuda", generator=g) / d ** 0.5
    x = torch.nn.functional.normalize(x, dim=1)
    where = torch.randperm(n, device="cuda", generator=g)[:planted]
    x[where] = x[where[:1]]
    return x.contiguous()


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


def bench(n, d, min_samples, a):
    x = make_data(n, d, a.centres, a.planted)
    core2 = None if min_samples == 1 else H.core_distances2(x, min_samples)
    eu = torch.empty(n - 1, dtype=torch.int32, device="cuda")
    ev = torch.empty(n - 1, dtype=torch.int32, device="cuda")
    ew2 = torch.empty(n - 1, dtype=torch.float32, device="cuda")
    rounds = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = H.mst_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    idx = torch.empty(n, 1, dtype=torch.int32, device="cuda")
    nd2 = torch.empty(n, 1, dtype=torch.float32, device="cuda")
    kbytes = G.graph_workspace_bytes(n, 1)
    kws = torch.empty(kbytes, dtype=torch.uint8, device="cuda")

    def mst():
        N.call("mreach_mst", x, n, d, core2, 0, eu, ev, ew2, rounds, ws, nbytes)

    def yard():
        N.call("knn_graph_l2", x, n, d, 1, idx, nd2, kws, kbytes)
    for fn in (mst, yard):
        timed(fn)                                     # warm-up of every shape the timed window uses
    mt, yt = [], []
    for _ in range(a.runs):                           # strictly alternating
        mt.append(timed(mst)[0])
        yt.append(timed(yard)[0])
    used = int(rounds.item())
    issued = (n - 1).bit_length()
    m, y = statistics.median(mt), statistics.median(yt)
    per_round = m / max(used, 1)
    tf = 2.0 * n * n * d / (per_round * 1e-3) / 1e12
    print(f"n={n} d={d} min_samples={min_samples}: {used} rounds of {issued} issued, {int((ew2 == 0).sum())} edges at 0, workspace "
          f"{nbytes / 2 ** 20:.1f} MiB")
    print(f"  mreach_mst        median {m:10.3f} ms  min {min(mt):10.3f}  max {max(mt):10.3f}  = {per_round:.3f} ms per working round")
    print(f"  knn_graph_l2 k=1  median {y:10.3f} ms  min {min(yt):10.3f}  max {max(yt):10.3f}")
    print(f"  round / yardstick {per_round / y:.3f}; a round = {tf:.1f} TF fp32 = {100 * tf / PEAK_F32_MFMA_TF:.1f} % of {PEAK_F32_MFMA_TF:.0f} TF")
    print(f"  mutual_reachability_mst (core distances, tree, sort): peak {peak(lambda: H.mutual_reachability_mst(x, min_samples)):.1f} MiB")
    if min_samples == a.min_samples[-1]:
        ms, res = timed(lambda: H.hdbscan(x, min_cluster_size=a.min_cluster_size, min_samples=min_samples))
        print(f"  hdbscan min_cluster_size {a.min_cluster_size}: {ms:.1f} ms end to end (host stage included), {res.n_clusters} clusters, "
              f"{int((res.labels < 0).sum())} noise")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--centres", type=int, default=512)
    ap.add_argument("--planted", type=int, default=2000)
    ap.add_argument("--min_samples", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--min_cluster_size", type=int, default=25)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mst_bench.py measures on the GPU; there is nothing to measure without one")
    for d in a.d:
        for min_samples in a.min_samples:
            bench(a.n, d, min_samples, a)


if __name__ == "__main__":
    main()
