"""Label spreading on the exact nearest-neighbour graph (csrc/spread.hip): what a user with a FEW labels does with a checkpoint.

Zhou et al. 2004 ("Learning with local and global consistency"; sklearn's `LabelSpreading`) on the matrix `pic_build` makes:
S = D^-1/2 W D^-1/2, F_0 = Y, F <- alpha S F + (1 - alpha) Y.  The columns of Y are independent, so every trial of a low-shot
evaluation (every shots value x every random draw x every class) is a column of ONE pass over ONE graph - `lowshot_evaluate`,
the 1 / 5 / 10 labels-per-class protocol of the MSN / DINO / SimCLR evaluations - and seeded pseudo-labels for the rest of a
collection are the one-trial case (`store_clusters --clustering spread`).  Y is passed as per-row seed lists and never stored.
Everything allocates through torch; single GPU.
"""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from src import _native as N
from src.evaluation.graph import knn_graph, pic_build

MAX_COLUMNS = 16384

SpreadResult = namedtuple("SpreadResult", "F labels confidence")

_NO_CPU = "audiossl HIP kernels need device tensors (no CPU fallback exists)"


def spread_workspace_bytes(n, m):
    return N.workspace_bytes("spread_workspace", n, m)


def default_iters(alpha):
    """Rounds after which alpha^T <= 1e-3: the distance to the fixed point is at most 2 alpha^T |Y_c| per column."""
    return int(math.ceil(math.log(1e-3) / math.log(alpha)))


def spread_normalize(W):
    """`Csr` of W -> (s fp32 [capacity], deg fp64 [n]): s_l = w_l / sqrt(deg_i deg_j) in fp64, rounded once; symmetric bit for bit;
    0 where a degree is 0.  Entries past the matrix's own are not written."""
    if not (W.col.is_cuda and W.w.is_cuda and W.rowptr.is_cuda):
        raise RuntimeError(_NO_CPU)
    deg = torch.empty(W.n, dtype=torch.float64, device=W.col.device)
    s = torch.empty(W.col.numel(), dtype=torch.float32, device=W.col.device)
    N.call("spread_normalize", W.rowptr, W.col, W.w, W.n, W.col.numel(), deg, s)
    return s, deg


def _seed_lists(seed_rows, seed_cols, n, m, device):
    """(node, column) pairs -> (seed_ptr int32 [n + 1], seed_col int32 [seeds]) on the device, columns ascending in every row."""
    rows = torch.as_tensor(seed_rows).reshape(-1)
    cols = torch.as_tensor(seed_cols).reshape(-1)
    if rows.numel() != cols.numel():
        raise ValueError(f"{rows.numel()} seed rows and {cols.numel()} seed columns")
    for name, t in (("seed_rows", rows), ("seed_cols", cols)):
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError(f"{name} are integers, got {t.dtype}")
    rows, cols = rows.to(device=device, dtype=torch.int64), cols.to(device=device, dtype=torch.int64)
    if rows.numel():
        bad = ((rows < 0) | (rows >= n) | (cols < 0) | (cols >= m)).nonzero().reshape(-1)
        if bad.numel():
            q = int(bad[0])
            raise ValueError(f"seed {q} = (node {int(rows[q])}, column {int(cols[q])}) is outside [0, {n}) x [0, {m})")
    key = torch.sort(rows * m + cols).values
    if key.numel() > 1:
        dup = (key[1:] == key[:-1]).nonzero().reshape(-1)
        if dup.numel():
            k = int(key[int(dup[0])])
            raise ValueError(f"seed (node {k // m}, column {k % m}) is given more than once")
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    ptr[1:] = torch.cumsum(torch.bincount(torch.div(key, m, rounding_mode="floor"), minlength=n), 0)
    return ptr.to(torch.int32), (key % m).to(torch.int32).contiguous()


@torch.no_grad()
def label_spread(W, seed_rows, seed_cols, m, classes, alpha=0.99, iters=None, s=None):
    """`Csr` of W, seeds as (node, column) pairs -> SpreadResult(F fp32 [n, m], labels int64 [n, trials], confidence fp32
    [n, trials]) with trials = m / classes: trial t owns columns t classes .. (t + 1) classes - 1.  labels are -1 where no seed of
    the trial lies within `iters` hops.  iters=None: `default_iters(alpha)`.  s: what `spread_normalize(W)` returned, to share it
    between calls.  Duplicate and out-of-range seeds are a ValueError (one read-back)."""
    if not (W.col.is_cuda and W.w.is_cuda and W.rowptr.is_cuda):
        raise RuntimeError(_NO_CPU)
    n, m, classes = W.n, int(m), int(classes)
    if classes < 1 or m < classes or m % classes:
        raise ValueError(f"m = {m} columns are not a positive multiple of classes = {classes}")
    if m > MAX_COLUMNS:
        raise ValueError(f"m must be at most {MAX_COLUMNS}, got {m}")
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must be in (0, 1), got {alpha}")
    iters = default_iters(alpha) if iters is None else int(iters)
    if iters < 1:
        raise ValueError(f"iters must be at least 1, got {iters}")
    mp = (m + 3) // 4 * 4
    if n * mp >= 2 ** 31:
        raise ValueError(f"n m = {n} x {mp} does not fit 2^31 elements; spread fewer columns per call")
    dev = W.col.device
    seed_ptr, seed_col = _seed_lists(seed_rows, seed_cols, n, m, dev)
    if seed_col.numel() == 0:
        raise ValueError("label spreading needs at least one seed")
    if s is None:
        s = spread_normalize(W)[0]
    trials = m // classes
    f = torch.empty(n, mp, dtype=torch.float32, device=dev)
    nbytes = spread_workspace_bytes(n, mp)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    N.call("spread_run", W.rowptr, W.col, s, n, W.col.numel(), seed_ptr, seed_col, seed_col.numel(), mp, float(alpha), iters, f, ws, nbytes)
    del ws
    labels, confidence = spread_assign(f, classes, trials)
    return SpreadResult(f[:, :m], labels, confidence)


def spread_assign(f, classes, trials):
    """F [n, >= classes trials] fp32 (device) -> (labels int64 [n, trials], confidence fp32 [n, trials])."""
    if not f.is_cuda:
        raise RuntimeError(_NO_CPU)
    f = f.float()
    if f.stride(1) != 1 or f.stride(0) < f.shape[1]:
        f = f.contiguous()
    n = f.shape[0]
    label = torch.empty(n, trials, dtype=torch.int32, device=f.device)
    confidence = torch.empty(n, trials, dtype=torch.float32, device=f.device)
    N.call("spread_assign", f.data_ptr(), n, f.stride(0), int(classes), int(trials), label, confidence)
    return label.long(), confidence


def lowshot_seeds(y_train, classes, shots, trials, seed):
    """Host.  For trial t and every class in ascending id: `shots` members of the class drawn without replacement by
    `numpy.random.default_rng([seed, shots, t])` from the class's members in ascending index order; a class with fewer members
    contributes all of them and is counted.  -> (rows int64, cols int64 = t classes + class, number of short classes)."""
    y = np.asarray(torch.as_tensor(y_train).cpu()).reshape(-1)
    members = [np.flatnonzero(y == c) for c in range(classes)]
    rows, cols = [], []
    for t in range(trials):
        rng = np.random.default_rng([seed, shots, t])
        for c, mem in enumerate(members):
            pick = mem if len(mem) <= shots else rng.choice(mem, size=shots, replace=False)
            rows.append(pick.astype(np.int64))
            cols.append(np.full(len(pick), t * classes + c, dtype=np.int64))
    short = sum(1 for mem in members if len(mem) < shots)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)      # noqa: E731
    return cat(rows), cat(cols), short


@torch.no_grad()
def lowshot_evaluate(train_emb, y_train, test_emb, y_test, shots=(1, 5, 10), trials=5, seed=0, k=10, sigma=None, alpha=0.99,
                     iters=None):
    """Transductive low-shot evaluation: one graph over train + test (L2-normalised rows, `knn_graph` -> `pic_build`), normalised
    once; every (shots value, trial) problem is a group of `classes` columns of one `label_spread` call, seeded from train rows
    only; accuracy on the test rows, an unreached row counting as wrong.  sigma=None: the square root of the median of the
    [n, k] squared neighbour distances.  -> dict (see evaluate_lowshot.py)."""
    if not (train_emb.is_cuda and test_emb.is_cuda):
        raise RuntimeError(_NO_CPU)
    shots = [int(v) for v in shots]
    if not shots or min(shots) < 1 or trials < 1:
        raise ValueError(f"shots {shots} and trials {trials} must be positive")
    y_train, y_test = torch.as_tensor(y_train).reshape(-1).cpu(), torch.as_tensor(y_test).reshape(-1).cpu()
    n_train, n_test = train_emb.shape[0], test_emb.shape[0]
    if y_train.numel() != n_train or y_test.numel() != n_test:
        raise ValueError(f"{n_train} + {n_test} embeddings, {y_train.numel()} + {y_test.numel()} labels")
    classes = int(max(int(y_train.max()), int(y_test.max()))) + 1
    x = F.normalize(torch.cat([train_emb.float(), test_emb.float()]), dim=1)
    k = min(int(k), x.shape[0] - 1)
    idx, d2 = knn_graph(x, k)
    if sigma is None:
        sigma = float(d2.median().sqrt())
        if not sigma > 0.0:
            raise ValueError("the median neighbour distance is 0 (duplicated embeddings): pass sigma")
    W = pic_build(idx, d2, sigma)
    rows, cols = [], []
    short = []
    for si, sh in enumerate(shots):
        r, c, sc = lowshot_seeds(y_train, classes, sh, trials, seed)
        rows.append(r)
        cols.append(c + si * trials * classes)
        short.append(sc)
    m = classes * len(shots) * trials
    alpha = float(alpha)
    iters = default_iters(alpha) if iters is None else int(iters)
    res = label_spread(W, torch.from_numpy(np.concatenate(rows)), torch.from_numpy(np.concatenate(cols)), m, classes, alpha, iters)
    pred = res.labels[n_train:].cpu().reshape(n_test, len(shots), trials)
    acc = (pred == y_test[:, None, None]).double().mean(0)                                   # [shots, trials]
    unreached = (pred < 0).double().mean(0)
    return dict(shots=shots, trials=int(trials), top1=[float(v) for v in acc.mean(1)],
                top1_std=[float(v) for v in acc.std(1, unbiased=False)], unreached=[float(v) for v in unreached.mean(1)],
                short_classes=short, k=k, sigma=float(sigma), alpha=alpha, iters=iters, N_train=int(n_train), N_test=int(n_test),
                d=int(train_emb.shape[1]), columns=int(m))
