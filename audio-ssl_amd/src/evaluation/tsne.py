"""A 2-D t-SNE map of a feature matrix (csrc/tsne.hip): van der Maaten's t-SNE with the parameters and schedule of
`sklearn.manifold.TSNE`.  The affinities are sparse, on each point's nearest neighbours as in sklearn's `barnes_hut` path
(`knn_graph`, exact fp32, no n x n matrix); the repulsion is exact - all pairs on the GPU every iteration, which is what
`angle = 0` would give.  Nothing holds n x n numbers.

What differs from sklearn on purpose: the iteration count is fixed (its early stopping would need a host sync per check), and the
neighbour lists stop at `MAX_K` = 64 entries, which limits the perplexity to 21 (sklearn's count is 3 perplexity + 1 neighbours).
Everything allocates through torch; single GPU.

`src.evaluation` exports the function `tsne`, so after `import src.evaluation` the attribute `src.evaluation.tsne` is that function
and not this module: take this module's other names with `from src.evaluation.tsne import ...`.
"""
import numpy as np
import torch

from src import _native as N
from src.evaluation.graph import MAX_K, Csr, knn_graph

MAX_PERPLEXITY = (MAX_K - 1) // 3                # int(3 * perplexity) + 1 <= MAX_K
_NO_CPU = "audiossl HIP kernels need device tensors (no CPU fallback exists)"


def tsne_workspace_bytes(n, k=1):
    return N.workspace_bytes("tsne_workspace", n, k)


def neighbour_count(n, perplexity):
    """sklearn's `min(n - 1, int(3 * perplexity + 1))`, checked against the graph's limit."""
    perplexity = float(perplexity)
    if not 1.0 <= perplexity <= MAX_PERPLEXITY:
        raise ValueError(f"perplexity must be in [1, {MAX_PERPLEXITY}]: it needs int(3 * perplexity) + 1 neighbours and knn_graph "
                         f"stops at {MAX_K}; got {perplexity:g}")
    if n < 3:
        raise ValueError(f"t-SNE needs at least 3 points, got {n}")
    k = min(n - 1, int(3.0 * perplexity) + 1)
    if perplexity >= k:
        raise ValueError(f"perplexity {perplexity:g} must be below the {k} neighbours that {n} points give")
    return k


def tsne_calibrate(d2, perplexity):
    """d2 [n, k] fp32 squared distances, nearest first -> (p_cond [n, k] fp32, beta [n] fp32): every row's conditional
    distribution at the entropy log(perplexity), by sklearn's bisection in fp64."""
    if not d2.is_cuda:
        raise RuntimeError(_NO_CPU)
    n, k = d2.shape
    d2 = d2.float().contiguous()
    p_cond = torch.empty(n, k, dtype=torch.float32, device=d2.device)
    beta = torch.empty(n, dtype=torch.float32, device=d2.device)
    N.call("tsne_calibrate", d2, n, k, float(perplexity), p_cond, beta)
    return p_cond, beta


def tsne_symmetrize(idx, p_cond):
    """idx, p_cond [n, k] -> `Csr` of P = (P_cond + P_cond^T) / (2 n), fp32 values in `.w`; columns ascending in every row, a
    mutual pair is one entry."""
    if not (idx.is_cuda and p_cond.is_cuda):
        raise RuntimeError(_NO_CPU)
    n, k = idx.shape
    idx = idx.to(torch.int32).contiguous()
    p_cond = p_cond.float().contiguous()
    cap = 2 * n * k
    dev = idx.device
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(cap, dtype=torch.int32, device=dev)
    p = torch.empty(cap, dtype=torch.float32, device=dev)
    nnz = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = tsne_workspace_bytes(n, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    N.call("tsne_symmetrize", idx, p_cond, n, k, rowptr, col, p, nnz, ws, nbytes)
    return Csr(rowptr, col, p, nnz, n)


def tsne_affinities(x, perplexity=20.0, neighbours=None):
    """x [n, d] (device) -> `Csr` of the joint probabilities P (fp32 values, sum 1).  `neighbours=(idx, d2)` reuses a graph the
    caller already has (`knn_graph(x, k)` with k = `neighbour_count(n, perplexity)`)."""
    if x.dim() != 2:
        raise ValueError(f"points are [n, d], got {tuple(x.shape)}")
    n = x.shape[0]
    k = neighbour_count(n, perplexity)
    if not x.is_cuda:
        raise RuntimeError(_NO_CPU)
    if neighbours is None:
        idx, d2 = knn_graph(x, k)
    else:
        idx, d2 = neighbours
        if tuple(idx.shape) != (n, k) or tuple(d2.shape) != (n, k):
            raise ValueError(f"perplexity {float(perplexity):g} on {n} points needs neighbour lists [{n}, {k}], got "
                             f"{tuple(idx.shape)} and {tuple(d2.shape)}")
    p_cond, _ = tsne_calibrate(d2, perplexity)
    return tsne_symmetrize(idx, p_cond)


class _Stepper:
    """The buffers of one layout size: repulsion, gradient and update launches without an allocation per iteration."""

    def __init__(self, P, n, device):
        self.P, self.n = P, n
        self.cap = P.col.numel()
        self.nbytes = tsne_workspace_bytes(n)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        self.rep = torch.empty(n, 2, dtype=torch.float32, device=device)
        self.grad = torch.empty(n, 2, dtype=torch.float32, device=device)
        self.z = torch.empty(1, dtype=torch.float64, device=device)
        self.kl = torch.empty(1, dtype=torch.float64, device=device)

    def gradient(self, y, exaggeration, want_kl):
        P = self.P
        N.call("tsne_repulsion", y, self.n, self.rep, self.z, self.ws, self.nbytes)
        N.call("tsne_gradient", P.rowptr, P.col, P.w, self.cap, y, self.rep, self.z, self.n, float(exaggeration), self.grad,
               self.kl if want_kl else None, self.ws if want_kl else None, self.nbytes if want_kl else 0)
        return self.grad


def _layout(y, n):
    if not isinstance(y, torch.Tensor) or y.dim() != 2 or tuple(y.shape) != (n, 2):
        raise ValueError(f"a layout is a tensor [{n}, 2], got {tuple(y.shape) if hasattr(y, 'shape') else type(y).__name__}")
    if not y.is_cuda:
        raise RuntimeError(_NO_CPU)
    return y.float().contiguous()


def tsne_gradient(P, y, exaggeration=1.0):
    """-> (grad [n, 2] fp32, kl fp64 [1]) on the device: the gradient of KL(exaggeration P || Q) at the layout y and the KL
    divergence of the unexaggerated P from Q - exact repulsion over all pairs."""
    y = _layout(y, P.n)
    st = _Stepper(P, P.n, y.device)
    st.gradient(y, exaggeration, True)
    return st.grad, st.kl


def pca_init(x):
    """x [n, d] -> [n, 2] float32 (host): the projection on the two leading principal directions (float64 `eigh` of the covariance
    on the host), every direction's sign fixed so that its largest-magnitude component is positive, scaled so that the first
    coordinate's standard deviation is 1e-4 (sklearn's scaling of its PCA initialisation)."""
    xc = x.detach().double().cpu().numpy()
    xc = xc - xc.mean(0, keepdims=True)
    lam, vec = np.linalg.eigh(xc.T @ xc / xc.shape[0])
    v = vec[:, np.argsort(lam)[::-1][:2]]
    if v.shape[1] < 2:
        v = np.concatenate([v, np.zeros_like(v)], 1)                 # one feature: the second coordinate starts at 0
    top = np.abs(v).argmax(0)
    v = v * np.where(v[top, np.arange(2)] < 0, -1.0, 1.0)
    y = xc @ v
    sd = y[:, 0].std()
    return torch.from_numpy((y * (1e-4 / sd if sd > 0 else 0.0)).astype(np.float32))


@torch.no_grad()
def tsne(x, perplexity=20.0, n_iter=1000, early_exaggeration=12.0, exaggeration_iters=250, learning_rate="auto", init="pca", seed=0,
         return_kl=False):
    """x [n, d] (device) -> y [n, 2] float32 on the device (and the final KL divergence as a python float with `return_kl`).
    sklearn's schedule: `exaggeration_iters` iterations at `early_exaggeration` with momentum 0.5, the rest at 1 with momentum
    0.8; `learning_rate="auto"` is max(n / early_exaggeration / 4, 50); gains as in `_gradient_descent`.  `init`: "pca", "random"
    (a CPU generator seeded with `seed`, scale 1e-4) or a tensor [n, 2].  The iteration count is fixed: no early stopping."""
    if x.dim() != 2:
        raise ValueError(f"points are [n, d], got {tuple(x.shape)}")
    n = x.shape[0]
    n_iter, exaggeration_iters = int(n_iter), int(exaggeration_iters)
    if n_iter < 0 or exaggeration_iters < 0:
        raise ValueError(f"iteration counts are non-negative, got {n_iter} and {exaggeration_iters}")
    neighbour_count(n, perplexity)                                   # refuse bad arguments before any work
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise ValueError(f"init is 'pca', 'random' or a tensor [n, 2], got {init!r}")
    elif not isinstance(init, torch.Tensor) or tuple(init.shape) != (n, 2):
        raise ValueError(f"init is 'pca', 'random' or a tensor [{n}, 2], got {tuple(init.shape) if hasattr(init, 'shape') else init!r}")
    if learning_rate != "auto" and not float(learning_rate) > 0:
        raise ValueError(f"learning_rate must be positive or 'auto', got {learning_rate!r}")
    if not x.is_cuda:
        raise RuntimeError(_NO_CPU)
    lr = max(n / float(early_exaggeration) / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    if isinstance(init, str):
        if init == "pca":
            y = pca_init(x).to(x.device)
        else:
            y = (1e-4 * torch.randn(n, 2, generator=torch.Generator().manual_seed(int(seed)))).to(x.device)
    else:
        y = init.detach().to(device=x.device, dtype=torch.float32).contiguous().clone()
    P = tsne_affinities(x, perplexity)
    st = _Stepper(P, n, x.device)
    update = torch.zeros_like(y)
    gains = torch.ones_like(y)
    for it in range(n_iter):
        early = it < exaggeration_iters
        grad = st.gradient(y, early_exaggeration if early else 1.0, False)
        N.call("tsne_update", grad, n, 0.5 if early else 0.8, lr, y, update, gains)
    if return_kl:
        st.gradient(y, 1.0, True)
        return y, float(st.kl.item())
    return y
