"""CPU restatements the k-NN tests compare against: plain torch in int64 / float64, independent of the product code."""
import torch


def topk_exact_int(q, bank, k):
    """Integer-valued q [Nq, D], bank [Nb, D] -> (dots int64 [Nq, k] descending, rows int64 [Nq, k]); equal dots in ascending
    bank row.  The composite key dot * Nb + (Nb - 1 - row) is unique per row of the similarity matrix, so `topk` of it is the
    specified order whatever `topk` does with ties.  The products are formed in float64 (BLAS), which is exact for these
    integers (|dot| < 2^53, asserted), and converted to int64."""
    q, bank = q.double(), bank.double()
    assert torch.equal(q, q.round()) and torch.equal(bank, bank.round())
    assert float(q.abs().max()) * float(bank.abs().max()) * q.shape[1] < 2.0 ** 53
    nb = bank.shape[0]
    out_d, out_i = [], []
    rows = torch.arange(nb, dtype=torch.int64)
    for s in range(0, q.shape[0], 64):                     # slabs: the int64 similarity block stays small
        dot = (q[s:s + 64] @ bank.T).to(torch.int64)
        key = dot * nb + (nb - 1 - rows)[None, :]
        idx = key.topk(k, dim=1).indices
        out_d.append(dot.gather(1, idx))
        out_i.append(idx)
    return torch.cat(out_d), torch.cat(out_i)


def sims_f64(q, bank):
    """fp64 dot products of the given (already rounded) rows."""
    return q.double() @ bank.double().T


def vote(top_sim, top_idx, labels, inv_t):
    """fp64 weighted vote: (pred int64 [Nq], conf float64 [Nq], per-row sorted class weights).  Neighbour j weighs
    exp((s_j - max_j s) * inv_t); the label with the largest sum wins, ties to the smaller label; conf = that sum / the total.
    A row with an index outside [0, len(labels)) gives pred -1, conf NaN."""
    top_sim, top_idx = top_sim.double(), top_idx.to(torch.int64)
    nb = labels.shape[0]
    pred, conf, margins = [], [], []
    for r in range(top_sim.shape[0]):
        idx = top_idx[r]
        if bool(((idx < 0) | (idx >= nb)).any()):
            pred.append(-1)
            conf.append(float("nan"))
            margins.append(None)
            continue
        w = torch.exp((top_sim[r] - top_sim[r].max()) * inv_t)
        lab = labels[idx]
        sums = {}
        for l, x in zip(lab.tolist(), w.tolist()):
            sums[l] = sums.get(l, 0.0) + x
        best = max(sums.items(), key=lambda kv: (kv[1], -kv[0]))
        pred.append(best[0])
        conf.append(best[1] / float(w.sum()))
        margins.append(sorted(sums.values(), reverse=True))
    return torch.tensor(pred, dtype=torch.int64), torch.tensor(conf, dtype=torch.float64), margins
