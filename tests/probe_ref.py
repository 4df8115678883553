"""Torch restatement of the linear-probe grid (csrc/probe.hip, src/evaluation/probe.py) for the tests.  Every function takes a
`dtype`: torch.float64 is the reference, torch.float32 on the CPU is the yardstick the fp32 kernels are held against
(`bound`: 4 x the largest fp32-vs-fp64 difference of the restatement on the same inputs, plus one fp32 ulp of the largest
reference magnitude)."""
import math

import torch

BETAS = (0.9, 0.999)
EPS = 1e-8


def ulp32(x):
    """One fp32 unit in the last place at magnitude x."""
    x = abs(float(x))
    return 2.0 ** -149 if x == 0.0 else 2.0 ** (math.floor(math.log2(x)) - 23)


def bound(ref32, ref64):
    """Allowed absolute error of a kernel result: 4 x max |fp32 restatement - fp64 restatement| + 1 fp32 ulp of max |fp64|."""
    ref64 = ref64.double()
    diff = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    return 4.0 * diff + ulp32(float(ref64.abs().max()) if ref64.numel() else 0.0)


def batch_ref(X, idx, mean, rstd, ldo, dtype=torch.float64):
    """[B][ldo]: (X[idx] - mean) * rstd, column D = 1, the rest 0; a row whose index is outside [0, N) is all NaN."""
    n, d = X.shape
    out = torch.zeros(len(idx), ldo, dtype=dtype)
    for r, i in enumerate(idx.tolist()):
        if not 0 <= i < n:
            out[r] = float("nan")
            continue
        row = X[i].to(dtype)
        if mean is not None:
            row = (row - mean.to(dtype)) * rstd.to(dtype)
        out[r, :d] = row
        out[r, d] = 1.0
    return out


def ce_heads_ref(logits, label, H, C, Cp, gscale, dtype=torch.float64):
    """logits [B][ld >= H Cp] -> (loss_sum [H] dtype, correct [H] int64, dlogits [B][H Cp] dtype with zero pad columns).
    Labels must lie in [0, C).  The first arg-max is taken on the logits AS GIVEN (exact in any dtype that holds them)."""
    B = logits.shape[0]
    loss = torch.zeros(H, dtype=dtype)
    correct = torch.zeros(H, dtype=torch.int64)
    grad = torch.zeros(B, H * Cp, dtype=dtype)
    onehot = torch.zeros(B, C, dtype=dtype)
    onehot[torch.arange(B), label] = 1.0
    for h in range(H):
        z = logits[:, h * Cp:h * Cp + C].to(dtype)
        m = z.max(dim=1, keepdim=True).values
        e = (z - m).exp()
        s = e.sum(dim=1, keepdim=True)
        row = (m - z.gather(1, label[:, None])) + s.log()
        loss[h] = row.sum()
        first = (z == m).to(torch.int64).argmax(dim=1)               # the lowest index that holds the maximum
        correct[h] = int((first == label).sum())
        grad[:, h * Cp:h * Cp + C] = gscale * (e / s - onehot)
    return loss, correct, grad


def adamw_heads_ref(W, grads, lrs, wds, seg, lr_scales=None, dtype=torch.float64):
    """torch.optim.AdamW with one parameter group per head segment of the flat `W`, stepped once per entry of `grads` ->
    (W, exp_avg, exp_avg_sq) flat, after the last step."""
    H = len(lrs)
    params = [W.flatten()[h * seg:(h + 1) * seg].clone().to(dtype).requires_grad_(True) for h in range(H)]
    opt = torch.optim.AdamW([dict(params=[p], lr=float(lrs[h]), weight_decay=float(wds[h])) for h, p in enumerate(params)],
                            betas=BETAS, eps=EPS)
    for k, g in enumerate(grads):
        scale = 1.0 if lr_scales is None else float(lr_scales[k])
        for h, p in enumerate(params):
            p.grad = g.flatten()[h * seg:(h + 1) * seg].clone().to(dtype)
            opt.param_groups[h]["lr"] = float(lrs[h]) * scale
        opt.step()
    st = [opt.state[p] for p in params]
    return (torch.cat([p.detach() for p in params]), torch.cat([s["exp_avg"] for s in st]), torch.cat([s["exp_avg_sq"] for s in st]))


def cosine_scale(k, total):
    return 0.5 * (1.0 + math.cos(math.pi * k / total))


def fit_ref(X, y, C, hparams, perms, batch_size, stats=None, dtype=torch.float64):
    """The whole `LinearProbeGrid.fit` given the epoch permutations: zero-initialised heads, one AdamW group per head (bias
    decayed like the weight), the last short batch kept and averaged over its own size, cosine lr over all steps.
    -> list of (weight [C][D], bias [C]) acting on the STANDARDISED features."""
    n, d = X.shape
    Xs = X.to(dtype)
    if stats is not None:
        Xs = (Xs - stats[0].to(dtype)) * stats[1].to(dtype)
    H = len(hparams)
    ws = [torch.zeros(C, d, dtype=dtype, requires_grad=True) for _ in range(H)]
    bs = [torch.zeros(C, dtype=dtype, requires_grad=True) for _ in range(H)]
    opt = torch.optim.AdamW([dict(params=[ws[h], bs[h]], lr=float(hparams[h][0]), weight_decay=float(hparams[h][1])) for h in range(H)],
                            betas=BETAS, eps=EPS)
    per_epoch = (n + batch_size - 1) // batch_size
    total, k = len(perms) * per_epoch, 0
    for perm in perms:
        for i in range(0, n, batch_size):
            rows = perm[i:i + batch_size]
            xb, yb = Xs[rows], y[rows]
            for h in range(H):
                opt.param_groups[h]["lr"] = float(hparams[h][0]) * cosine_scale(k, total)
            opt.zero_grad(set_to_none=True)
            loss = sum(torch.nn.functional.cross_entropy(xb @ ws[h].T + bs[h], yb) for h in range(H))
            loss.backward()
            opt.step()
            k += 1
    return [(ws[h].detach(), bs[h].detach()) for h in range(H)]


def eval_ref(heads, X, y, stats=None, dtype=torch.float64):
    """-> (mean loss per head, logits per head [N][C]) of `fit_ref`'s heads on X."""
    Xs = X.to(dtype)
    if stats is not None:
        Xs = (Xs - stats[0].to(dtype)) * stats[1].to(dtype)
    logits = [Xs @ w.to(dtype).T + b.to(dtype) for w, b in heads]
    return [float(torch.nn.functional.cross_entropy(z, y)) for z in logits], logits


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())
