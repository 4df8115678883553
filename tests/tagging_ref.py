"""numpy restatements for the tagging tests: int64 pair counts -> fp64 AP / AUC (sklearn's average_precision_score and
roc_auc_score, ties included), fp64 BCE-with-logits and its gradient, and the literal label mix of
`extras/mast_new/mast/dataloader.py:167-175`.  Nothing here touches the GPU or the product code."""
import numpy as np

BLOCK = 512          # positives per comparison block: bounds the boolean matrices at BLOCK x N


def class_counts(s, t):
    """s [N] scores, t [N] {0,1} -> (ge_all, gt_all, ge_pos, gt_pos) int64 [npos], one row per positive in sample order."""
    s = np.asarray(s)
    pos = np.nonzero(np.asarray(t))[0]
    sp = s[pos]
    out = [np.zeros(len(pos), dtype=np.int64) for _ in range(4)]
    for b in range(0, len(pos), BLOCK):
        q = sp[b:b + BLOCK, None]
        out[0][b:b + BLOCK] = (s[None, :] >= q).sum(1)
        out[1][b:b + BLOCK] = (s[None, :] > q).sum(1)
        out[2][b:b + BLOCK] = (sp[None, :] >= q).sum(1)
        out[3][b:b + BLOCK] = (sp[None, :] > q).sum(1)
    return tuple(out)


def class_stats(s, t):
    """-> (npos, auc_num2 (python int), ap, auc); ap and auc are NaN without a positive or without a negative."""
    n = len(s)
    ge_all, gt_all, ge_pos, gt_pos = class_counts(s, t)
    npos = len(ge_all)
    nneg = n - npos
    ge_neg, gt_neg = ge_all - ge_pos, gt_all - gt_pos
    num2 = int(np.sum(2 * (nneg - ge_neg) + (ge_neg - gt_neg), dtype=np.int64))
    if npos == 0 or nneg == 0:
        return npos, num2, float("nan"), float("nan")
    ap = float(np.sum(ge_pos.astype(np.float64) / ge_all.astype(np.float64))) / npos
    return npos, num2, ap, num2 / (2.0 * npos * nneg)


def stats(scores, targets):
    """scores [N, C], targets [N, C] -> dict of npos int64 [C], auc_num2 int64 [C], AP / auc float64 [C], mAP, mAUC (NaN-skipping
    means), classes_scored."""
    scores, targets = np.asarray(scores), np.asarray(targets)
    rows = [class_stats(scores[:, c], targets[:, c]) for c in range(scores.shape[1])]
    ap = np.array([r[2] for r in rows], dtype=np.float64)
    auc = np.array([r[3] for r in rows], dtype=np.float64)
    scored = ~np.isnan(auc)
    return {"npos": np.array([r[0] for r in rows], dtype=np.int64), "auc_num2": np.array([r[1] for r in rows], dtype=np.int64),
            "AP": ap, "auc": auc, "mAP": float(ap[scored].mean()) if scored.any() else float("nan"),
            "mAUC": float(auc[scored].mean()) if scored.any() else float("nan"), "classes_scored": int(scored.sum())}


def bce(logits, targets):
    """fp64 nn.BCEWithLogitsLoss() (mean over every element) of the given values -> (loss, dlogits [N, C])."""
    x = np.asarray(logits, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float64)
    e = np.exp(-np.abs(x))
    loss = float(np.mean(np.maximum(x, 0.0) - x * t + np.log1p(e)))
    sig = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return loss, (sig - t) / x.size


def mix_rows(labels, partner, lam, index):
    """The literal loops of dataloader.py:167-175 / 179-182: labels = one list of names per clip, partner [B] (-1 = no mix),
    lam [B] -> float32 [B, C]."""
    out = np.zeros((len(labels), len(index)), dtype=np.float32)
    for i, names in enumerate(labels):
        row = np.zeros(len(index))
        if partner[i] >= 0:
            mix_lambda = float(lam[i])
            for name in names:
                row[index[name]] += mix_lambda
            for name in labels[int(partner[i])]:
                row[index[name]] += 1.0 - mix_lambda
        else:
            for name in names:
                row[index[name]] = 1.0
        out[i] = row.astype(np.float32)
    return out


# ---- the matrices of tests/golden/tagging_stats.npz (make_tagging_golden.py writes them, the GPU tests run on them) ----------
GOLDEN_CASES = [(257, 5, 0.3, None), (1000, 7, 0.02, 8), (513, 4, 0.5, 3), (2049, 6, 0.004, None), (300, 3, 0.9, 2)]


def golden_matrix(i):
    """Case i: float32 standard-normal scores, rounded to multiples of 1/q where q is given (heavy ties); Bernoulli(density)
    targets with row 0 all-positive and row 1 all-negative, so every class has both kinds."""
    n, c, dens, q = GOLDEN_CASES[i]
    rng = np.random.default_rng(100 + i)
    s = rng.standard_normal((n, c)).astype(np.float32)
    if q:
        s = (np.round(s * q) / q).astype(np.float32)
    t = (rng.random((n, c)) < dens).astype(np.uint8)
    t[0, :] = 1
    t[1, :] = 0
    return s, t
