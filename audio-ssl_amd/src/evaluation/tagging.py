"""Audio tagging (multi-label) downstream: the labels, the loss and the metrics of the reference's AudioSet / FSD50K path.

  parse_labels / build_class_index / multi_hot / mix_labels   `extras/mast_new/mast/dataloader.py:21-29, 157-184`: a label cell
                                                              holds several names; with a two-file mix the target is
                                                              lam * y + (1 - lam) * y[partner]
  bce_with_logits                                             nn.BCEWithLogitsLoss() on soft targets (`audiossl_bce_rows`)
  tagging_stats                                               `extras/mast_new/mast/utilities/stats.py:11-57` (`calculate_stats`,
                                                              `d_prime`): per-class AP / ROC-AUC / d' (`audiossl_tagging_stats`)

The reference computes the metrics on the host with sklearn, class by class; here the logits stay on the device, the pass is
integer pair counts of each class's positives (no sort; csrc/tagging.hip) and only the [C] results come back.  Everything here
allocates through torch (outputs and the kernel's workspace), so torch's memory statistics see every byte.  Single GPU.
"""
import csv
import math
import statistics

import numpy as np
import torch

from src import _native as N


# ---------------------------------------------------------------------------------------------------------------- labels
def parse_labels(cell, sep=","):
    """One CSV label cell -> the list of names in it, in order ("dog,bark" -> ["dog", "bark"]); blanks around a name and
    quotes around the cell are dropped."""
    names = [s.strip() for s in str(cell).strip().strip('"').split(sep)]
    names = [s for s in names if s]
    if not names:
        raise ValueError(f"empty label cell {cell!r}")
    return names


def build_class_index(train_cells, label_csv=None, sep=","):
    """name -> column.  Default: the sorted unique names of the train split (as `DownstreamDataset.get_label2id` sorts).  With
    `label_csv`: the `index,mid,display_name` file of `dataloader.py:21-29`, mid -> index."""
    if label_csv is not None:
        with open(label_csv, "r", newline="") as f:
            index = {row["mid"]: int(row["index"]) for row in csv.DictReader(f)}
        if sorted(index.values()) != list(range(len(index))):
            raise ValueError(f"{label_csv}: the index column is not 0..{len(index) - 1}")
        return index
    names = sorted({n for cell in train_cells for n in parse_labels(cell, sep)}, key=str)
    return {n: i for i, n in enumerate(names)}


def multi_hot(list_of_name_lists, index):
    """[[name, ...], ...] -> float32 [B, C] with ones at the named columns; a name outside the index raises."""
    y = torch.zeros(len(list_of_name_lists), len(index), dtype=torch.float32)
    for r, names in enumerate(list_of_name_lists):
        for n in names:
            if n not in index:
                raise ValueError(f"label {n!r} is not in the class index ({len(index)} classes)")
            y[r, index[n]] = 1.0
    return y


def mix_labels(y, partner, lam):
    """`dataloader.py:167-175` for a batch: lam * y + (1 - lam) * y[partner] where partner >= 0, y unchanged where partner == -1
    (`MastFrontEnd.last_plan` holds the draws the audio was mixed with).  Formed in float64 and rounded to float32 once, as the
    reference's numpy row is."""
    partner = torch.as_tensor(partner).to(device=y.device, dtype=torch.int64)
    lam = torch.as_tensor(lam).to(device=y.device, dtype=torch.float64)[:, None]
    y64 = y.double()
    mixed = lam * y64 + (1.0 - lam) * y64[partner.clamp(min=0)]
    return torch.where((partner >= 0)[:, None], mixed, y64).to(torch.float32)


# ------------------------------------------------------------------------------------------------------------------ loss
class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        n, c = logits.shape
        lg = logits.float().contiguous()
        tg = targets.to(device=lg.device, dtype=torch.float32).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=lg.device)
        need = ctx.needs_input_grad[0]
        dl = torch.empty(n, c, dtype=torch.float32, device=lg.device) if need else None
        N.call("bce_rows", N.F32, lg, tg, n, c, loss, dl)
        if need:
            ctx.save_for_backward(dl)
        ctx.in_dtype = logits.dtype
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl * g).to(ctx.in_dtype), None


def bce_with_logits(logits, targets):
    """nn.BCEWithLogitsLoss()(logits, targets): logits [N, C], targets [N, C] in [0, 1] (soft after a mix), mean over N*C."""
    if logits.dim() != 2 or tuple(targets.shape) != tuple(logits.shape):
        raise ValueError(f"logits {tuple(logits.shape)} and targets {tuple(targets.shape)} must be the same [N, C]")
    return _BCEFn.apply(logits, targets)


# --------------------------------------------------------------------------------------------------------------- metrics
def workspace_bytes(n, c):
    return N.workspace_bytes("tagging_workspace", n, c)


def tagging_counts(scores, targets):
    """The kernel as it is: scores fp32 [N, C], targets [N, C] (non-zero = positive), both on the device ->
    (npos int32 [C], auc_num2 int64 [C], ap float64 [C], auc float64 [C]) on the device."""
    if scores.dim() != 2 or tuple(targets.shape) != tuple(scores.shape):
        raise ValueError(f"scores {tuple(scores.shape)} and targets {tuple(targets.shape)} must be the same [N, C]")
    n, c = scores.shape
    dev = scores.device
    sc = scores.float().contiguous()
    if sc.data_ptr() % 16:
        sc = sc.clone()
    tg = (targets.to(dev) != 0).to(torch.uint8).contiguous()
    npos = torch.empty(c, dtype=torch.int32, device=dev)
    num2 = torch.empty(c, dtype=torch.int64, device=dev)
    ap = torch.empty(c, dtype=torch.float64, device=dev)
    auc = torch.empty(c, dtype=torch.float64, device=dev)
    nbytes = workspace_bytes(n, c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    N.call("tagging_stats", sc, tg, n, c, npos, num2, ap, auc, ws, nbytes)
    return npos, num2, ap, auc


_NORMAL = statistics.NormalDist()


def d_prime(auc):
    """`stats.py:6-9`: sqrt(2) * inverse normal CDF of the AUC, in float64 on the host (1 -> inf, 0 -> -inf, NaN -> NaN)."""
    auc = float(auc)
    if math.isnan(auc):
        return float("nan")
    if auc >= 1.0:
        return float("inf")
    if auc <= 0.0:
        return float("-inf")
    return math.sqrt(2.0) * _NORMAL.inv_cdf(auc)


def _nanmean(a):
    keep = a[~np.isnan(a)]
    return float(keep.mean()) if keep.size else float("nan")


def tagging_stats(scores, targets):
    """`calculate_stats` for the whole matrix in one device pass: scores [N, C] (finite; pass the raw logits - they rank at
    least as finely as their sigmoid, which merges large logits into ties at 1.0), targets [N, C] in {0, 1}.
    -> dict: AP, auc, d_prime, npos (numpy [C]; NaN where a class has no positive or no negative), auc_num2 (the exact integer
    numerator), mAP, mAUC (means over the scored classes), d_prime_mean = sqrt(2) ndtri(mAUC), classes_scored."""
    if not scores.is_cuda:
        raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")
    if not bool(torch.isfinite(scores).all()):
        raise ValueError("tagging_stats needs finite scores")
    npos, num2, ap, auc = (t.cpu().numpy() for t in tagging_counts(scores, targets))
    m_ap, m_auc = _nanmean(ap), _nanmean(auc)
    return {"AP": ap, "auc": auc, "d_prime": np.array([d_prime(a) for a in auc], dtype=np.float64), "npos": npos, "auc_num2": num2,
            "mAP": m_ap, "mAUC": m_auc, "d_prime_mean": d_prime(m_auc), "classes_scored": int((~np.isnan(auc)).sum())}
