"""Linear evaluation on cached embeddings (the DINO / MSN / BYOL-A protocol): the encoder is frozen, so its embeddings are computed
once (`extract_embeddings`) and a whole grid of linear heads, one per (learning rate, weight decay) pair, is trained together on
the `[N, D]` matrix.  The head is picked on a validation split and its test accuracy is the number to report.

The heads are one fp32 matrix `W [H * Cp][Dp]` (csrc/probe.hip; `Cp` = C rounded up to 8, `Dp = D + 8`, column D is the bias).
A step is five launches whatever H is: `probe_batch` (gather + standardise + ones column), `gemm` (logits of every head),
`probe_ce` (segmented soft-max cross-entropy, loss / hit counters, dlogits), `gemm` (dW), `probe_adamw` (one lr / wd per head).
Logits exist per batch only, as `[B][H * Cp]`; nothing of size N x H C is allocated.  Everything allocates through torch.
Single GPU, single-label; there is no CPU path.
"""
import math

import torch

from src import _native as N

BETAS = (0.9, 0.999)       # torch.optim.AdamW defaults
EPS = 1e-8
SLAB = 8192                # rows per launch of evaluate / predict


def _need_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("audiossl HIP kernels need device tensors (no CPU fallback exists)")


def feature_stats(X):
    """[N, D] training matrix (device) -> (mean [D], rstd [D]) fp32 with rstd = 1 / (population std + 1e-6)."""
    _need_device(X)
    var, mean = torch.var_mean(X.float(), dim=0, unbiased=False)
    return mean.contiguous(), (1.0 / (var.sqrt() + 1e-6)).contiguous()


def stratified_holdout(labels, fraction, seed):
    """Split row numbers into (kept, held): per class, in ascending class order, max(1, round(fraction * n_c)) rows chosen by one
    seeded `torch.randperm` stream are held out; a class with a single row stays in training.  Both results are sorted."""
    y = torch.as_tensor(labels).cpu().to(torch.int64)
    if not 0.0 < fraction < 1.0:
        raise ValueError("holdout fraction must be in (0, 1)")
    g = torch.Generator().manual_seed(int(seed))
    held = []
    for c in torch.unique(y).tolist():
        rows = torch.nonzero(y == c).flatten()
        n = rows.numel()
        if n < 2:
            continue
        k = min(max(1, int(round(fraction * n))), n - 1)
        held.append(rows[torch.randperm(n, generator=g)[:k]])
    held = torch.sort(torch.cat(held)).values if held else torch.empty(0, dtype=torch.int64)
    mask = torch.ones(y.numel(), dtype=torch.bool)
    mask[held] = False
    return torch.nonzero(mask).flatten(), held


def head_index(i_lr, i_wd, n_wd):
    return i_lr * n_wd + i_wd


def epoch_permutations(n, epochs, generator=None):
    """The row orders `fit` walks: one CPU `torch.randperm(n, generator=generator)` per epoch."""
    return [torch.randperm(n, generator=generator) for _ in range(epochs)]


def cosine_scale(k, total):
    """lr multiplier of 0-based step k of `total`: 1 at the first step, towards 0 after the last."""
    return 0.5 * (1.0 + math.cos(math.pi * k / total))


def select_head(results):
    """Index of the best entry of `evaluate`'s list: highest top1, then lowest loss, then lowest index."""
    if not results:
        raise ValueError("no heads to select from")
    return min(range(len(results)), key=lambda h: (-results[h]["top1"], results[h]["loss"], h))


def fold_standardisation(weight, bias, mean, rstd):
    """(weight [C, D], bias [C]) acting on (x - mean) * rstd -> the pair acting on raw x, computed in fp64."""
    w = weight.double() * rstd.double()[None, :]
    return w, bias.double() - w @ mean.double()


class LinearProbeGrid:
    """`LinearProbeGrid(D, C, lrs, wds, stats).fit(X, y, epochs, batch_size)`: H = len(lrs) * len(wds) zero-initialised linear heads
    under AdamW, head `i_lr * len(wds) + i_wd` with (lrs[i_lr], wds[i_wd]); the bias is decayed like the weights
    (`AdamW(linear.parameters(), weight_decay=wd)`).  `stats` = `feature_stats(X_train)` or None for raw features."""

    def __init__(self, D, C, lrs, weight_decays, stats=None, device="cuda"):
        lrs, wds = [float(v) for v in lrs], [float(v) for v in weight_decays]
        if not lrs or not wds:
            raise ValueError("the grid needs at least one learning rate and one weight decay")
        if D % 8 != 0 or not 8 <= D <= 4096:
            raise ValueError(f"embedding width {D}: the probe kernels take 8 <= D <= 4096 with D % 8 == 0 (pad with zero columns)")
        if not 2 <= C <= 4096:
            raise ValueError(f"{C} classes: the probe kernels take 2 <= C <= 4096")
        self.D, self.C, self.Cp, self.Dp = int(D), int(C), (int(C) + 7) // 8 * 8, int(D) + 8
        self.lrs, self.wds = lrs, wds
        self.H = len(lrs) * len(wds)
        self.hparams = [(lr, wd) for lr in lrs for wd in wds]
        self.device = torch.device(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.W = torch.zeros(self.H * self.Cp, self.Dp, **f32)
        self.dW, self.m, self.v = torch.zeros_like(self.W), torch.zeros_like(self.W), torch.zeros_like(self.W)
        self.lr = torch.tensor([p[0] for p in self.hparams], **f32)
        self.wd = torch.tensor([p[1] for p in self.hparams], **f32)
        self.steps = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.loss_sum = torch.zeros(self.H, dtype=torch.float64, device=self.device)
        self.correct = torch.zeros(self.H, dtype=torch.int64, device=self.device)
        self.mean = self.rstd = None
        if stats is not None:
            mean, rstd = stats
            _need_device(mean, rstd)
            if mean.shape != (self.D,) or rstd.shape != (self.D,):
                raise ValueError("stats are (mean [D], rstd [D])")
            self.mean, self.rstd = mean.float().contiguous(), rstd.float().contiguous()
        self._rows = 0
        self._xb = self._logits = self._dlogits = None

    # ---- launches -----------------------------------------------------------------------------------------------------------
    def _buffers(self, B):
        if B > self._rows:
            f32 = dict(dtype=torch.float32, device=self.device)
            self._xb = torch.empty(B, self.Dp, **f32)
            self._logits = torch.empty(B, self.H * self.Cp, **f32)
            self._dlogits = torch.empty(B, self.H * self.Cp, **f32)
            self._rows = B
        return self._xb[:B], self._logits[:B], self._dlogits[:B]

    def _check(self, X, idx):
        _need_device(X, idx)
        if X.dim() != 2 or X.shape[1] != self.D or X.dtype != torch.float32:
            raise ValueError(f"X must be fp32 [N, {self.D}]")
        if idx.dtype != torch.int32 or idx.dim() != 1 or idx.numel() == 0:
            raise ValueError("idx must be a non-empty int32 vector")

    def _logits_of(self, X, idx):
        """probe_batch + the logits GEMM -> (xb [B, Dp], logits [B, H Cp], dlogits buffer)."""
        B, HCp = idx.numel(), self.H * self.Cp
        xb, logits, dlogits = self._buffers(B)
        N.call("probe_batch", X, X.shape[0], self.D, idx, B, self.mean, self.rstd, xb, self.Dp)
        N.call("gemm", N.F32, 0, 0, B, HCp, self.Dp, 1.0, xb, self.Dp, self.W, self.Dp, logits, HCp, None, 0, None, 0, 1.0, None, 0,
               0, 0, 1, None, 0)
        return xb, logits, dlogits

    def step(self, X, idx, y_batch, lr_scale=1.0):
        """One AdamW step of every head on rows `idx` (int32, device) of X with labels `y_batch` (int64, device): five launches.
        The batch's loss sums and hits are added to `loss_sum` / `correct`."""
        self._check(X, idx)
        _need_device(y_batch)
        B, HCp = idx.numel(), self.H * self.Cp
        if y_batch.dtype != torch.int64 or y_batch.shape != (B,):
            raise ValueError("y_batch must be int64, one label per batch row")
        xb, logits, dlogits = self._logits_of(X, idx)
        N.call("probe_ce", logits, HCp, y_batch, B, self.H, self.C, self.Cp, 1.0 / B, self.loss_sum, self.correct, dlogits)
        N.call("gemm", N.F32, 1, 1, HCp, self.Dp, B, 1.0, dlogits, HCp, xb, self.Dp, self.dW, self.Dp, None, 0, None, 0, 1.0, None, 0,
               0, 0, 1, None, 0)
        self.steps.add_(1)
        N.call("probe_adamw", self.W, self.dW, self.m, self.v, self.H, self.Cp * self.Dp, self.lr, self.wd, float(lr_scale),
               BETAS[0], BETAS[1], EPS, self.steps)

    # ---- protocol -----------------------------------------------------------------------------------------------------------
    def fit(self, X, y, epochs, batch_size, generator=None):
        """`epochs` passes over X [N, D] / y int64 [N] (device) in batches of `batch_size`; the last short batch of an epoch is kept
        and averaged over its own size.  The row order of an epoch is one CPU `torch.randperm(N, generator=generator)`; the lr of
        every head follows a cosine from its value to 0 over all steps."""
        _need_device(X, y)
        n = X.shape[0]
        if y.shape != (n,) or y.dtype != torch.int64:
            raise ValueError("y must be int64 [N]")
        per_epoch = (n + batch_size - 1) // batch_size
        total, k = epochs * per_epoch, 0
        for perm in epoch_permutations(n, epochs, generator):
            order = perm.to(torch.int32).to(self.device)
            y_perm = y[order.long()]
            for i in range(0, n, batch_size):
                self.step(X, order[i:i + batch_size], y_perm[i:i + batch_size].contiguous(), cosine_scale(k, total))
                k += 1
        return self

    def evaluate(self, X, y, slab=SLAB):
        """-> [{lr, wd, loss, top1}] per head on X [N, D] / y int64 [N] (device): mean cross-entropy and accuracy, forward only."""
        _need_device(X, y)
        n = X.shape[0]
        y = y.to(torch.int64).contiguous()
        loss = torch.zeros(self.H, dtype=torch.float64, device=self.device)
        hit = torch.zeros(self.H, dtype=torch.int64, device=self.device)
        rows = torch.arange(n, dtype=torch.int32, device=self.device)
        for i in range(0, n, slab):
            idx = rows[i:i + slab]
            self._check(X, idx)
            _, logits, _ = self._logits_of(X, idx)
            N.call("probe_ce", logits, self.H * self.Cp, y[i:i + slab], idx.numel(), self.H, self.C, self.Cp, 0.0, loss, hit, None)
        loss, hit = (loss / n).tolist(), hit.tolist()
        return [dict(lr=lr, wd=wd, loss=loss[h], top1=hit[h] / n) for h, (lr, wd) in enumerate(self.hparams)]

    def select(self, val_results):
        return select_head(val_results)

    def head(self, h):
        """-> (weight [C, D], bias [C]) fp32 of head h with the standardisation folded in: `x @ weight.T + bias` on RAW embeddings."""
        blk = self.W[h * self.Cp:h * self.Cp + self.C]
        w, b = blk[:, :self.D], blk[:, self.D]
        if self.mean is not None:
            w, b = fold_standardisation(w, b, self.mean, self.rstd)
        return w.float().contiguous(), b.float().contiguous()

    def predict(self, X, h, slab=SLAB):
        """-> int64 [N]: head h's first arg-max class per row of X."""
        _need_device(X)
        n = X.shape[0]
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        rows = torch.arange(n, dtype=torch.int32, device=self.device)
        for i in range(0, n, slab):
            idx = rows[i:i + slab]
            self._check(X, idx)
            _, logits, _ = self._logits_of(X, idx)
            out[i:i + slab] = logits[:, h * self.Cp:h * self.Cp + self.C].argmax(dim=1)
        return out
