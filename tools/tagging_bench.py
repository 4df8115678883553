"""Diagnostic (GPU box): the pair-count tagging metrics (`src.evaluation.tagging.tagging_counts`: transpose, compaction of each
class's positives, integer pair counts, one fp64 sum per class - no sort) next to the obvious device composition in the same
process - torch `sort` of every class column, `cumsum` of the sorted labels, tie groups closed with `cummin` / `cummax` -
alternating run by run, timed with device events, with the peak allocator growth of each.  No sklearn, no host round trip on
either side.

    python tools/tagging_bench.py [--runs 7] [--iters 3] [--sizes 20383x527x0.005,20383x527x0.5,10231x200x0.02]

Per size: the two results are compared first at the bars of tests/test_gpu_tagging.py (npos and the integer AUC numerator equal,
AUC within 2^-52, AP within N 2^-51) - a mismatch ends the run - then one line per path: median / min / max ms per call and
peak MiB.  Nothing is asserted about which path is faster."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-ssl_amd")]
import torch  # noqa: E402
from src.evaluation.tagging import tagging_counts  # noqa: E402

DEFAULT_SIZES = "20383x527x0.005,20383x527x0.5,10231x200x0.02"


def baseline(scores, targets):
    """Per-class sort + cumsum on the device -> (npos int64, auc_num2 int64, ap fp64, auc fp64), ties as sklearn treats them:
    every member of a tie group sees the counts at the END of its group.  Class-major first, so that the sort and the scans run
    along the contiguous axis (torch's segmented sort; sorting the [N, C] matrix along dim 0 took 11 to 15 times as long)."""
    n, c = scores.shape
    dev = scores.device
    vals, order = scores.t().contiguous().sort(dim=1, descending=True)
    lab = targets.t().contiguous().gather(1, order).to(torch.int64)
    cum_pos = lab.cumsum(1)
    rank = torch.arange(1, n + 1, device=dev, dtype=torch.int64)[None, :].expand(c, n)
    cum_neg = rank - cum_pos
    edge = vals[:, 1:] != vals[:, :-1]
    true_col = torch.ones(c, 1, dtype=torch.bool, device=dev)
    is_end, is_start = torch.cat([edge, true_col], 1), torch.cat([true_col, edge], 1)
    big = torch.iinfo(torch.int64).max

    def at_group_end(x):                                      # x non-decreasing along dim 1
        return torch.where(is_end, x, big).flip(1).cummin(1).values.flip(1)
    pos_end, all_end = at_group_end(cum_pos), at_group_end(rank)
    neg_before = torch.where(is_start, cum_neg - (1 - lab), -1).cummax(1).values          # negatives strictly above the group
    npos = cum_pos[:, -1]
    nneg = n - npos
    ge_neg = all_end - pos_end
    ap_terms = pos_end.double() / all_end.double()
    num2 = (lab * (2 * (nneg[:, None] - ge_neg) + (ge_neg - neg_before))).sum(1)
    scored = (npos > 0) & (nneg > 0)
    nan = torch.full((c,), float("nan"), dtype=torch.float64, device=dev)
    ap = torch.where(scored, (lab * ap_terms).sum(1) / npos.double(), nan)
    auc = torch.where(scored, num2.double() / (2.0 * npos.double() * nneg.double()), nan)
    return npos, num2, ap, auc


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del out
    return grown / 2 ** 20


def compare(ours, base, n):
    npos, num2, ap, auc = (t.cpu() for t in ours)
    bnpos, bnum2, bap, bauc = (t.cpu() for t in base)
    if not (torch.equal(npos.long(), bnpos) and torch.equal(num2, bnum2)):
        raise SystemExit("the two paths disagree on an integer count")
    keep = ~torch.isnan(bauc)
    if not torch.equal(torch.isnan(auc), ~keep) or not torch.equal(torch.isnan(ap), ~keep):
        raise SystemExit("the two paths disagree on which classes are scored")
    e_ap = float((ap - bap)[keep].abs().max()) if keep.any() else 0.0
    e_auc = float((auc - bauc)[keep].abs().max()) if keep.any() else 0.0
    if e_auc > 2.0 ** -52 or e_ap > n * 2.0 ** -51:
        raise SystemExit(f"the two paths differ: AP {e_ap:.3e} (bar {n * 2.0 ** -51:.3e}), AUC {e_auc:.3e} (bar {2.0 ** -52:.3e})")
    return e_ap, e_auc, int(keep.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=DEFAULT_SIZES, help="comma-separated NxCxdensity")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tagging_bench.py measures on the GPU; there is nothing to measure without one")
    for spec in a.sizes.split(","):
        n, c, dens = spec.split("x")
        n, c, dens = int(n), int(c), float(dens)
        g = torch.Generator(device="cuda").manual_seed(n + c)
        targets = (torch.rand(n, c, device="cuda", generator=g) < dens).to(torch.uint8)
        scores = torch.randn(n, c, device="cuda", generator=g) + 1.5 * targets.float()          # a classifier that has learnt something
        paths = {"pair counts (HIP)": lambda: tagging_counts(scores, targets), "torch sort + cumsum": lambda: baseline(scores, targets)}
        e_ap, e_auc, scored = compare(paths["pair counts (HIP)"](), paths["torch sort + cumsum"](), n)
        print(f"N={n} C={c} density={dens}: {scored} classes scored, |AP diff| {e_ap:.2e}, |AUC diff| {e_auc:.2e}, integer counts equal")
        for fn in paths.values():                             # warm-up of every shape the timed window uses
            timed(fn, 1)
        times = {k: [] for k in paths}
        for _ in range(a.runs):
            for k, fn in paths.items():
                times[k].append(timed(fn, a.iters))
        for k, fn in paths.items():
            ts = times[k]
            print(f"  {k:20s} median {statistics.median(ts):9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}  peak {peak(fn):8.1f} MiB")


if __name__ == "__main__":
    main()
