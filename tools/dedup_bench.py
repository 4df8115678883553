"""Diagnostic (GPU box): the duplicate search (`range_count`, `range_fill`, `graph_components` and the whole `near_duplicates` call)
next to the obvious torch composition in the same process, alternating run by run, with the peak allocator growth of each; and
the count pass next to `knn_graph_l2` (k = 5), which walks the same tiles.

    python tools/dedup_bench.py [--n 65536] [--d 128 2048] [--centres 512] [--planted 2000] [--matches 16] [--runs 5] [--slab 4096]

Data.  Unit rows around `centres` centres, every row with its own noise scale (so that the number of matches varies from row to
row), plus a planted block of `planted` identical rows.  The threshold is the one radius at which a sample of ordinary rows has
`matches` matches on average (a quantile of the sample's distances).
Baseline.  Slabs of `slab` rows: torch fp32 `mm` against all rows, distances from the norms, compare, diagonal cleared by index,
`nonzero` - the slab's [slab, n] matrix is stored; then the edges go to the host and scipy's `connected_components` labels them.
Prints one line per stage and path: median / min / max ms, peak MiB; the fp32 MFMA rate of the count pass (2 n^2 d flop); whether
the two edge sets agree (the baseline rounds differently: pairs within rounding of the radius may differ) and the groups."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from src import _native as N  # noqa: E402
from src.evaluation import dedup as D  # noqa: E402
from src.evaluation import graph as G  # noqa: E402

PEAK_F32_MFMA_TF = 155.0


def make_data(n, d, centres, planted):
    g = torch.Generator(device="cuda").manual_seed(n + d)
    c = torch.nn.functional.normalize(torch.randn(centres, d, device="cuda", generator=g), dim=1)
    scale = 0.05 + 0.25 * torch.rand(n, 1, device="cuda", generator=g)
    x = c[torch.randint(centres, (n,), device="cuda", generator=g)] + scale * torch.randn(n, d, device="cuda", generator=g) / d ** 0.5
    x = torch.nn.functional.normalize(x, dim=1)
    where = torch.randperm(n, device="cuda", generator=g)[:planted]
    x[where] = x[where[:1]]
    return x.contiguous(), where


def pick_radius2(x, where, matches, sample=512):
    ordinary = torch.ones(x.shape[0], dtype=torch.bool, device=x.device)
    ordinary[where] = False
    rows = ordinary.nonzero().reshape(-1)[:sample]
    dist = (2.0 - 2.0 * (x[rows] @ x.T)).clamp_(min=0)
    dist[torch.arange(len(rows), device=x.device), rows] = float("inf")
    return float(dist.reshape(-1).kthvalue(matches * len(rows)).values)


def torch_edges(x, r2, slab):
    n = x.shape[0]
    norms = (x * x).sum(1)
    out = []
    for i in range(0, n, slab):
        xs = x[i:i + slab]
        hit = (norms[i:i + slab, None] + norms[None, :] - 2.0 * (xs @ x.T)).clamp_(min=0) <= r2
        r = torch.arange(xs.shape[0], device=x.device)
        hit[r, r + i] = False
        e = hit.nonzero()
        e[:, 0] += i
        out.append(e)
    return torch.cat(out)


def scipy_components(edges, n):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    e = edges.cpu().numpy()
    m = csr_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(n, n))
    return connected_components(m, directed=True, connection="weak")


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


def bench(n, d, a):
    x, where = make_data(n, d, a.centres, a.planted)
    r2 = float(np.float32(pick_radius2(x, where, a.matches)))
    max_edges = 2 ** 31 - 1
    nbytes = D.range_workspace_bytes(n, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rowptr = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    total_d = torch.empty(1, dtype=torch.int64, device="cuda")
    geometry = (x, n, d, 0, n, 0, n, r2, 0)
    N.call("range_count", *geometry, rowptr, total_d, ws, nbytes)
    total = int(total_d.item())
    col = torch.empty(total, dtype=torch.int32, device="cuda")
    d2 = torch.empty(total, dtype=torch.float32, device="cuda")
    csr = D.range_graph(x, r2, max_edges=max_edges)
    te = torch_edges(x, r2, a.slab)
    stages = [
        ("count", lambda: N.call("range_count", *geometry, rowptr, total_d, ws, nbytes), None),
        ("knn_graph k=5", lambda: G.knn_graph(x, 5), None),
        ("fill", lambda: N.call("range_fill", *geometry, rowptr, total, col, d2, total, ws, nbytes), None),
        ("count+read+fill", lambda: D.range_graph(x, r2, max_edges=max_edges), lambda: torch_edges(x, r2, a.slab)),
        ("components", lambda: D.graph_components(csr.rowptr, csr.col, n), lambda: scipy_components(te, n)),
        ("near_duplicates", lambda: D.near_duplicates(x, r2, metric="l2", max_edges=max_edges),
         lambda: scipy_components(torch_edges(x, r2, a.slab), n)),
    ]
    ordinary = (total - a.planted * (a.planted - 1)) / (n - a.planted)
    print(f"n={n} d={d}: r2 {r2:.6f} (cosine {1 - r2 / 2:.4f}), {total} entries, {ordinary:.1f} per ordinary row, "
          f"max degree {int((csr.rowptr[1:] - csr.rowptr[:-1]).max())}")
    medians = {}
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
            medians[name, p] = statistics.median(ts)
            print(f"  {name:16s} {p:6s} median {statistics.median(ts):10.3f} ms  min {min(ts):10.3f}  max {max(ts):10.3f}  "
                  f"peak {peak(fn):9.1f} MiB")
    # count and knn_graph once more, strictly alternating
    ct, kt = [], []
    for _ in range(a.runs):
        ct.append(timed(stages[0][1])[0])
        kt.append(timed(stages[1][1])[0])
    tf = 2.0 * n * n * d / (statistics.median(ct) * 1e-3) / 1e12
    print(f"  alternating: count median {statistics.median(ct):.3f} ms, knn_graph_l2 (k = 5) median {statistics.median(kt):.3f} ms; "
          f"count = {tf:.1f} TF fp32 = {100 * tf / PEAK_F32_MFMA_TF:.1f} % of {PEAK_F32_MFMA_TF:.0f} TF")
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (csr.rowptr[1:] - csr.rowptr[:-1]).long())
    mine = rows * n + csr.col.long()
    theirs = te[:, 0] * n + te[:, 1]
    only_mine = int((~torch.isin(mine, theirs)).sum())
    only_theirs = int((~torch.isin(theirs, mine)).sum())
    label, count = D.graph_components(csr.rowptr, csr.col, n)
    tcount, tlabel = scipy_components(te, n)
    print(f"  edge sets: {len(mine)} fused, {len(theirs)} torch, {only_mine} only fused, {only_theirs} only torch; "
          f"groups {count} fused, {tcount} torch; largest group {int(torch.bincount(label.long()).max())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--centres", type=int, default=512)
    ap.add_argument("--planted", type=int, default=2000)
    ap.add_argument("--matches", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--slab", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dedup_bench.py measures on the GPU; there is nothing to measure without one")
    for d in a.d:
        bench(a.n, d, a)


if __name__ == "__main__":
    main()
