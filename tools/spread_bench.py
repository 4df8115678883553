"""Diagnostic (GPU box): `audiossl_spread_run` (csrc/spread.hip: one launch per iteration, Y never stored) next to the obvious torch
composition in the same process - `torch.sparse` CSR fp32 `S @ F`, then the scale and the add of a dense Y - alternating run by
run, with the peak allocator growth of each.

    python tools/spread_bench.py [--n 65536] [--d 128] [--k 10] [--centres 512] [--classes 35] [--iters 100] [--runs 5]

One graph (`knn_graph` -> `pic_build` -> `spread_normalize` on whitened-like unit-norm features), m = classes + 1 rounded up to
a multiple of 4 (36) and m = classes x 15 rounded up (528).  For every m: both workgroup-id mappings of the kernel
(AUDIOSSL_SPREAD_MAP=0: a row block's column slices on consecutive ids; 1, the default: one slice's row blocks first) and the
torch path.  Prints per path: median / min / max ms per iteration, bytes gathered per second (nnz m 4 / t), peak MiB; then the
largest difference between the two results and the longest row of the matrix.  Last, the wall time of one `lowshot_evaluate`
(3 shots values x 5 trials) on the same points."""
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
from src.evaluation import spread as SP  # noqa: E402

ALPHA = 0.99


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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--centres", type=int, default=512)
    ap.add_argument("--classes", type=int, default=35)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no_lowshot", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spread_bench.py measures on the GPU; there is nothing to measure without one")
    g = torch.Generator(device="cuda").manual_seed(a.n)
    c = torch.nn.functional.normalize(torch.randn(a.centres, a.d, device="cuda", generator=g), dim=1)
    member = torch.randint(a.centres, (a.n,), device="cuda", generator=g)
    x = c[member] + 0.15 * torch.randn(a.n, a.d, device="cuda", generator=g) / a.d ** 0.5
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    n = a.n
    idx, d2 = G.knn_graph(x, a.k)
    sigma = float(d2.median().sqrt())
    W = G.pic_build(idx, d2, sigma)
    s, deg = SP.spread_normalize(W)
    nnz = int(W.nnz)
    lengths = (W.rowptr[1:] - W.rowptr[:-1])
    print(f"n={n} d={a.d} k={a.k} sigma={sigma:.4f}: nnz {nnz} ({nnz / n:.1f} per row), longest row {int(lengths.max())}, "
          f"{int((deg == 0).sum())} rows of degree 0")
    S = torch.sparse_csr_tensor(W.rowptr.long(), W.col[:nnz].long(), s[:nnz], size=(n, n))

    for m in ((a.classes + 1 + 3) // 4 * 4, (a.classes * 15 + 3) // 4 * 4):
        gen = torch.Generator().manual_seed(m)
        rows = torch.randint(n, (m * 5,), generator=gen)
        cols = torch.arange(m).repeat_interleave(5)
        keys = torch.unique(rows * m + cols)
        rows, cols = keys // m, keys % m
        seed_ptr, seed_col = SP._seed_lists(rows, cols, n, m, x.device)
        f = torch.empty(n, m, dtype=torch.float32, device="cuda")
        nbytes = SP.spread_workspace_bytes(n, m)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def fused(mapping):
            def run():
                os.environ["AUDIOSSL_SPREAD_MAP"] = str(mapping)
                N.call("spread_run", W.rowptr, W.col, s, n, W.col.numel(), seed_ptr, seed_col, seed_col.numel(), m, ALPHA, a.iters, f, ws, nbytes)
                return f
            return run

        def fused_alloc():
            f2 = torch.empty(n, m, dtype=torch.float32, device="cuda")
            w2 = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            N.call("spread_run", W.rowptr, W.col, s, n, W.col.numel(), seed_ptr, seed_col, seed_col.numel(), m, ALPHA, a.iters, f2, w2, nbytes)
            return f2

        def torch_path():
            Y = torch.zeros(n, m, dtype=torch.float32, device="cuda")
            Y[rows.cuda(), cols.cuda()] = 1.0
            F = Y.clone()
            for _ in range(a.iters):
                F = ALPHA * (S @ F) + (1.0 - ALPHA) * Y
            return F

        paths = {"fused map 0": fused(0), "fused map 1": fused(1), "torch": torch_path}
        for fn in paths.values():
            timed(fn)                                 # warm-up of every shape the timed window uses
        times = {p: [] for p in paths}
        for _ in range(a.runs):
            for p, fn in paths.items():
                times[p].append(timed(fn)[0] / a.iters)
        print(f"m={m}: {a.iters} iterations, F {n * m * 4 / 2 ** 20:.0f} MiB per copy")
        for p, fn in paths.items():
            ts = times[p]
            med = statistics.median(ts)
            print(f"  {p:12s} median {med:9.4f} ms/iter  min {min(ts):9.4f}  max {max(ts):9.4f}  "
                  f"gathered {nnz * m * 4 / (med * 1e-3) / 1e12:6.3f} TB/s  peak {peak(fused_alloc if p.startswith('fused') else fn):9.1f} MiB")
        os.environ.pop("AUDIOSSL_SPREAD_MAP", None)
        ours = fused(1)().clone()
        theirs = torch_path()
        print(f"  max |fused - torch| = {float((ours - theirs).abs().max()):.3e} (largest value {float(theirs.max()):.3e}); "
              f"map 0 and map 1 bit-identical: {bool(torch.equal(fused(0)(), ours))}")
        os.environ.pop("AUDIOSSL_SPREAD_MAP", None)
        del f, ws, ours, theirs

    # what a hub row costs: rows are not split, so one wave per column slice walks the whole row.  A star (every node's only
    # neighbour is node 0) makes that row the critical path of the launch: time per iteration / entries = cost per entry.
    star = torch.zeros(n, 1, dtype=torch.int64, device="cuda")
    star[0, 0] = 1
    Ws = G.pic_build(star, 0.02 + 0.3 * torch.rand(n, 1, device="cuda", generator=g), 0.5)
    ss, _ = SP.spread_normalize(Ws)
    m = (a.classes * 15 + 3) // 4 * 4
    seed_ptr, seed_col = SP._seed_lists(torch.arange(m) * 7, torch.arange(m), n, m, x.device)
    f = torch.empty(n, m, dtype=torch.float32, device="cuda")
    nbytes = SP.spread_workspace_bytes(n, m)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hub = lambda: N.call("spread_run", Ws.rowptr, Ws.col, ss, n, Ws.col.numel(), seed_ptr, seed_col, m, m, ALPHA, 20, f, ws, nbytes)   # noqa: E731
    timed(hub)
    ts = [timed(hub)[0] / 20 for _ in range(a.runs)]
    med = statistics.median(ts)
    print(f"hub row of {n - 1} entries, m={m}: median {med:.4f} ms/iter (min {min(ts):.4f}, max {max(ts):.4f}) = {med * 1e6 / (n - 1):.1f} ns per entry; "
          f"the longest row of the k-NN graph above ({int(lengths.max())} entries) costs {med * 1e3 / (n - 1) * int(lengths.max()):.2f} us at that rate")
    del f, ws

    if not a.no_lowshot:
        y = (member % a.classes).cpu()
        n_train = n * 3 // 4
        args = (x[:n_train], y[:n_train], x[n_train:], y[n_train:])
        kw = dict(shots=(1, 5, 10), trials=5, k=a.k)
        timed(lambda: SP.lowshot_evaluate(*args, **kw))
        ts = [timed(lambda: SP.lowshot_evaluate(*args, **kw)) for _ in range(3)]
        out = ts[0][1]
        print(f"lowshot_evaluate: {out['columns']} columns, {out['iters']} iterations: median {statistics.median(t for t, _ in ts) / 1e3:.3f} s "
              f"(min {min(t for t, _ in ts) / 1e3:.3f}, max {max(t for t, _ in ts) / 1e3:.3f}); top1 {out['top1']}, unreached {out['unreached']}")


if __name__ == "__main__":
    main()
