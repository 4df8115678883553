"""Diagnostic (GPU box): the fused k-NN top-k (`audiossl_knn_topk`) next to the materialising baseline in the same process -
`E.gemm` bf16 -> fp32 [Nq, Nb] followed by `torch.topk` - alternating run by run, with the peak allocator growth of each; then
one embedding pass (front end + encoder in eval mode + time mean) beside the linear probe's forward on the same batches.

    python tools/knn_bench.py [--nq 4096] [--nb 65536] [--k 20] [--dims 2048 768] [--runs 5] [--iters 10]

Prints one line per path and shape: median / min / max ms per call, algorithmic TFLOP/s (2 Nq Nb D over the time), peak MiB."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import torch  # noqa: E402
from src import _native as N  # noqa: E402
from src import engine as E  # noqa: E402
from src.evaluation.knn import knn_topk_bf16  # noqa: E402


def baseline(q, bank, k):
    nq, d = q.shape
    nb = bank.shape[0]
    sim = torch.empty(nq, nb, dtype=torch.float32, device=q.device)
    E.gemm(N.BF16, 0, 0, nq, nb, d, q, d, bank, d, sim, nb, out_f32=1)
    return sim.topk(k, dim=1)


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


def bench_topk(nq, nb, d, k, runs, iters):
    g = torch.Generator(device="cuda").manual_seed(d)
    q = torch.nn.functional.normalize(torch.randn(nq, d, device="cuda", generator=g), dim=1).to(torch.bfloat16)
    bank = torch.nn.functional.normalize(torch.randn(nb, d, device="cuda", generator=g), dim=1).to(torch.bfloat16)
    paths = {"fused knn_topk": lambda: knn_topk_bf16(q, bank, k), "gemm + torch.topk": lambda: baseline(q, bank, k)}
    fs, fi = paths["fused knn_topk"]()
    bs, bi = paths["gemm + torch.topk"]()
    agree = float((fi.long() == bi).float().mean())
    print(f"Nq={nq} Nb={nb} D={d} k={k}: index agreement with the baseline {agree:.6f}, max |sim diff| {float((fs - bs).abs().max()):.2e}")
    for fn in paths.values():                       # warm-up of every shape the timed window uses
        timed(fn, 2)
    times = {n: [] for n in paths}
    for _ in range(runs):
        for n, fn in paths.items():
            times[n].append(timed(fn, iters))
    for n, fn in paths.items():
        ts = times[n]
        med = statistics.median(ts)
        print(f"  {n:18s} median {med:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  "
              f"{2.0 * nq * nb * d / med / 1e9:7.1f} TFLOP/s  peak {peak(fn):8.1f} MiB")


def bench_embed(batch, batches, runs):
    from src.dataset.downstream_dataset import DownstreamFrontEnd
    from src.downstream import DownstreamEncoder
    from src.encoder import AudioNTT2020Task6
    from src.evaluation import Embedder
    dcfg = {"downstream": {"finetune_layer": -1, "base_encoder": {"return_all_layers": False, "output_dim": 2048},
                           "input": {"n_mels": 64}}}
    torch.manual_seed(0)
    model = DownstreamEncoder(dcfg, None, AudioNTT2020Task6, 35).cuda().eval()
    emb = Embedder(model.encoder, layer="backbone")
    front = DownstreamFrontEnd()
    waves = [torch.randn(batch, 16000, device="cuda") * 0.1 for _ in range(batches)]

    def embed_pass():
        return [emb(front(w)) for w in waves]

    @torch.no_grad()
    def probe_pass():
        return [model(front(w)) for w in waves]
    for fn in (embed_pass, probe_pass):
        timed(fn, 1)
    for name, fn in (("embedding pass (eval, time mean)", embed_pass), ("probe forward (eval)", probe_pass)):
        ts = [timed(fn, 1) for _ in range(runs)]
        med = statistics.median(ts)
        print(f"{name:34s} B={batch} x {batches}: median {med:8.2f} ms  min {min(ts):8.2f}  max {max(ts):8.2f}  "
              f"{batch * batches / med * 1e3:9.0f} clips/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--nb", type=int, default=65536)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--dims", type=int, nargs="+", default=[2048, 768])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--embed_batch", type=int, default=256)
    ap.add_argument("--embed_batches", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench.py measures on the GPU; there is nothing to measure without one")
    for d in a.dims:
        bench_topk(a.nq, a.nb, d, a.k, a.runs, a.iters)
    if a.embed_batches:
        bench_embed(a.embed_batch, a.embed_batches, a.runs)


if __name__ == "__main__":
    main()
