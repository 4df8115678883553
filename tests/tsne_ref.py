"""t-SNE in float64 numpy, dense and slow: the rule `csrc/tsne.hip` is tested against (van der Maaten & Hinton 2008 with the parameters
and schedule of `sklearn.manifold.TSNE`, sparse affinities on given neighbour lists, exact repulsion).

`f32=True` evaluates the same formula with its exponentials / reciprocals and sums in float32: the distance between the two is
the yardstick the GPU tests scale their bars with."""
import numpy as np

STEPS, TOL = 100, 1e-5


def calibrate(d2, perplexity, f32=False):
    """d2 [n, k] squared distances -> (p_cond [n, k], beta [n], entropy [n]): `_binary_search_perplexity` of
    sklearn/manifold/_utils.pyx row by row, on distances shifted by the row's smallest (P is unchanged by the shift).  The row is
    stored in float32 (as sklearn's is), and the entropy the search steers is that of the STORED row, -sum p log p, so that what
    is returned meets the tolerance itself; sklearn's log(sum) + beta sum(d p) / sum is the same number before that rounding."""
    d2 = np.asarray(d2, dtype=np.float64)
    n, k = d2.shape
    target = np.log(perplexity)
    ft = np.float32 if f32 else np.float64
    P = np.empty((n, k))
    betas, ents = np.empty(n), np.empty(n)
    for i in range(n):
        d = d2[i] - d2[i].min()
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(STEPS):
            p = np.exp((-d * beta).astype(ft))
            row = (p / p.sum(dtype=ft)).astype(np.float32).astype(np.float64)
            h = -float((row * np.log(np.where(row > 0, row, 1.0))).sum())
            diff = h - target
            if abs(diff) <= TOL:
                break
            if diff > 0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        P[i] = row
        betas[i], ents[i] = beta, h
    return P, betas, ents


def joint(idx, p_cond):
    """-> dense P [n, n] float64 = (P_cond + P_cond^T) / (2 n)."""
    idx = np.asarray(idx)
    n, k = idx.shape
    C = np.zeros((n, n))
    C[np.repeat(np.arange(n), k), idx.reshape(-1)] = np.asarray(p_cond, dtype=np.float64).reshape(-1)
    return (C + C.T) / (2.0 * n)


def kl_and_gradient(P, y, exaggeration=1.0, f32=False):
    """Dense P [n, n] (the unexaggerated one), layout y [n, 2] -> (grad [n, 2], kl, Z, rep [n, 2]); self leaves by index.
    grad is the gradient of KL(exaggeration P || Q); kl is that of P itself and always float64."""
    ft = np.float32 if f32 else np.float64
    y = np.asarray(y).astype(ft)
    Pt = np.asarray(P).astype(ft)
    n = y.shape[0]
    diff = y[:, None, :] - y[None, :, :]
    w = (ft(1) / (ft(1) + (diff * diff).sum(-1, dtype=ft))).astype(ft)
    w[np.arange(n), np.arange(n)] = 0
    Z = w.sum(dtype=ft)
    rep = ((w * w)[:, :, None] * diff).sum(1, dtype=ft)
    att = ((Pt * w)[:, :, None] * diff).sum(1, dtype=ft)
    grad = ft(4) * (ft(exaggeration) * att - rep / Z)
    nz = np.asarray(P) > 0
    kl = float((np.asarray(P, dtype=np.float64)[nz] * np.log(np.asarray(P, dtype=np.float64)[nz] * float(Z) / w.astype(np.float64)[nz])).sum())
    return grad.astype(np.float64), kl, float(Z), rep.astype(np.float64)


def update(y, upd, gains, grad, momentum, lr):
    """`_gradient_descent` of sklearn/manifold/_t_sne.py, one step -> (y, update, gains)."""
    inc = upd * grad < 0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    upd = momentum * upd - lr * gains * grad
    return y + upd, upd, gains


def pca_init(x):
    """The two leading principal directions, each signed so that its largest-magnitude component is positive; the first
    coordinate's standard deviation scaled to 1e-4."""
    xc = np.asarray(x, dtype=np.float64)
    xc = xc - xc.mean(0, keepdims=True)
    lam, vec = np.linalg.eigh(xc.T @ xc / len(xc))
    v = vec[:, np.argsort(lam)[::-1][:2]]
    v = v * np.where(v[np.abs(v).argmax(0), np.arange(2)] < 0, -1.0, 1.0)
    y = xc @ v
    return y / y[:, 0].std() * 1e-4


def neighbours(x, k):
    """Exact k nearest other rows in float64, (d2 ascending, row ascending) -> (idx [n, k], d2 [n, k])."""
    x = np.asarray(x, dtype=np.float64)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    d[np.arange(len(x)), np.arange(len(x))] = np.inf
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(d, idx, 1)


def run(x, perplexity=20.0, n_iter=1000, early_exaggeration=12.0, exaggeration_iters=250, init=None):
    """The whole map -> (y [n, 2], kl of the initial layout, kl of the final one)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    k = min(n - 1, int(3.0 * perplexity) + 1)
    idx, d2 = neighbours(x, k)
    P = joint(idx, calibrate(d2, perplexity)[0])
    y = pca_init(x) if init is None else np.array(init, dtype=np.float64)
    lr = max(n / early_exaggeration / 4.0, 50.0)
    upd, gains = np.zeros_like(y), np.ones_like(y)
    kl0 = kl_and_gradient(P, y)[1]
    for it in range(n_iter):
        early = it < exaggeration_iters
        grad = kl_and_gradient(P, y, early_exaggeration if early else 1.0)[0]
        y, upd, gains = update(y, upd, gains, grad, 0.5 if early else 0.8, lr)
    return y, kl0, kl_and_gradient(P, y)[1]


def blobs(n_per, centres, d, spread, seed):
    """`centres` Gaussian blobs of `n_per` points, unit variance, centres drawn with standard deviation `spread` -> (x float32, labels)."""
    rng = np.random.RandomState(seed)
    c = rng.randn(centres, d) * spread
    labels = np.repeat(np.arange(centres), n_per)
    return (c[labels] + rng.randn(centres * n_per, d)).astype(np.float32), labels


def purity(y, labels, k=10):
    """Mean fraction of a point's k nearest neighbours in the plane that carry its label."""
    idx, _ = neighbours(y, k)
    return float((labels[idx] == labels[:, None]).mean())


def csr_to_dense(rowptr, col, val, n):
    rowptr, col, val = np.asarray(rowptr), np.asarray(col), np.asarray(val, dtype=np.float64)
    D = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    D[rows, col[:rowptr[n]]] = val[:rowptr[n]]
    return D


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))
