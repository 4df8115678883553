"""Diagnostic (GPU box): whole-clip embeddings in ragged batches (`Embedder.embed_ragged` on the plan of `plan_ragged_batches`)
next to what gives the same result without them - one clip per call through the rectangular path at the clip's own length - and
next to the `center` window (one fixed window per file, the per-file yardstick), in one process, alternating pass by pass after
every shape has run once.

    python tools/whole_clip_bench.py [--clips 2048] [--passes 3] [--batch_size 64] [--max_frames 65536] [--precision bf16]

Clips: a seeded set, log-uniform in 1 .. 30 s, cut from one buffer of noise on the device; every variant finds its inputs on the
device already (no decoding, no upload in the timings).  A randomly initialised conv encoder in eval mode, layer `backbone`.
Prints one line per variant: median / min / max seconds per pass over all clips, clips per second, peak allocator MiB above the
resident inputs; then the padded share of frames of the plan and the largest rel-L2 between the two whole-clip results."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--max_frames", type=int, default=65536)
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from src.encoder import AudioNTT2020Task6
    from src.evaluation.embed import Embedder, plan_ragged_batches, take_window
    torch.manual_seed(a.seed)
    rng = np.random.default_rng(a.seed)
    lengths = [int(16000 * 30.0 ** u) for u in rng.uniform(0.0, 1.0, a.clips)]
    starts = [int(s) for s in rng.integers(0, 16000 * 30, a.clips)]
    noise = (torch.rand(16000 * 60, device="cuda") - 0.5) * 0.6
    clips = [noise[s:s + n] for s, n in zip(starts, lengths)]                  # views: nothing is copied
    model = AudioNTT2020Task6(64, 2048, False).cuda()
    emb = Embedder(model, layer="backbone", precision=a.precision)
    front = emb.front_end()
    plan = plan_ragged_batches(lengths, a.batch_size, a.max_frames)
    batches = []
    for idx, tmax in plan:
        lmax = lengths[idx[-1]] + lengths[idx[-1]] % 2
        w = torch.zeros(len(idx), lmax, device="cuda")
        for r, i in enumerate(idx):
            w[r, :lengths[i]] = clips[i]
        batches.append((idx, w, torch.tensor([lengths[i] for i in idx], dtype=torch.int32)))
    centre = [torch.stack([take_window(c, 16000, "center") for c in clips[i:i + a.batch_size]]) for i in range(0, a.clips, a.batch_size)]
    padded = 1.0 - sum(1 + n // 160 for n in lengths) / sum(len(idx) * tmax for idx, tmax in plan)

    def ragged():
        out = torch.empty(a.clips, 2048, device="cuda")
        for idx, w, lens in batches:
            out[torch.tensor(idx, device="cuda")] = emb.embed_ragged(w, lens)
        return out

    def one_by_one():
        out = torch.empty(a.clips, 2048, device="cuda")
        for i, c in enumerate(clips):
            out[i] = emb(front(c[None]))[0]
        return out

    def center():
        return torch.cat([emb(front(w)) for w in centre])

    variants = (("ragged batches", ragged), ("one clip per call", one_by_one), ("center window", center))
    results, times, peaks = {}, {n: [] for n, _ in variants}, {}
    for name, fn in variants:                                                  # every shape once: allocator, tables, code objects
        results[name] = fn()
    torch.cuda.synchronize()
    for _ in range(a.passes):
        for name, fn in variants:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            peaks[name] = max(peaks.get(name, 0), torch.cuda.max_memory_allocated() - base)
    for name, _ in variants:
        t = times[name]
        print(f"{name:18s} median {statistics.median(t):8.3f} s  min {min(t):8.3f}  max {max(t):8.3f}  "
              f"{a.clips / statistics.median(t):9.1f} clips/s  peak {peaks[name] / 2 ** 20:9.1f} MiB")
    r, o = results["ragged batches"].double(), results["one clip per call"].double()
    rel = float(((r - o).norm(dim=1) / o.norm(dim=1).clamp_min(1e-30)).max())
    print(f"{len(plan)} ragged batches, padded share of frames {padded:.4f}; largest rel-L2 ragged vs one clip per call {rel:.3e}")
    print(json.dumps(dict(clips=a.clips, precision=a.precision, audio_seconds=sum(lengths) / 16000.0, batches=len(plan), padded_share=padded,
                          seconds={n: statistics.median(t) for n, t in times.items()}, peak_mib={n: p / 2 ** 20 for n, p in peaks.items()},
                          rel_l2=rel)))


if __name__ == "__main__":
    main()
