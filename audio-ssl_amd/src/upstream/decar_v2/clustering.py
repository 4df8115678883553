"""Offline pseudo-labelling for DeepCluster / UnFuSeD-style label files on MI355X - `extras/decar-v2/clustering.py:9-115` and the
tail of `extras/decar-v2/store_clusters.py:64-160` of the reference: embeddings -> PCA-whitening to 128 dims -> L2 rows ->
k-means (20 Lloyd iterations) -> `images_lists` -> a `path,label` CSV.

The reference does all of it with faiss (`PCAMatrix(512, 128, eigen_power=-0.5)`, `Clustering` on a `GpuIndexFlatL2`); faiss is
a third-party dependency that is neither in the reference tree nor in this image, so this follows its documented algorithm
(parity unpinned): centre, eigendecompose the covariance, keep the `pca` leading directions scaled by eigenvalue^-0.5; Lloyd's
algorithm from `k` distinct random points (seed = np.random.randint(1234) as the reference sets it), nearest centroid in L2,
plain means, empty clusters keep their centroid (faiss re-splits large clusters instead).
GPU work: covariance, projection and the E step are MFMA GEMMs (fp32 path), argmin = `row_argmax` of x.c - |c|^2 / 2, M step =
`kmeans_accumulate` + `kmeans_update_mean`.  The 512 x 512 eigendecomposition runs once on the host (numpy, float64).

The second half of the reference file (`clustering.py:118-295`) is `PIC`: DeepCluster's power-iteration clustering on a graph of
nearest neighbours, which finds the number of clusters itself.  Here the graph is `audiossl_knn_graph_l2` (exact, fp32 end to
end, ties by ascending row) instead of a faiss index, and the adjacency matrix, the 200 power iterations and the walk to the
local maxima are `audiossl_pic_build` / `pic_power` / `pic_assign` (csrc/graph.hip) instead of scipy and Python loops.  Parity
decisions:
  * the graph excludes self by INDEX and `make_graph` puts the identity column back; faiss returns whatever sorts first, which
    for duplicated rows need not be the row itself;
  * all graph arithmetic is float64 (the kernel weights, v, the comparisons), which is what the reference computes under the
    numpy it pins; under numpy 2.x the same reference code stays in float32 end to end;
  * the reference numbers the final clusters in the iteration order of a Python `set`; here clusters are numbered in ascending
    order of their smallest member, and members are listed in ascending order."""
import time

import numpy as np
import torch

from src import _native as N
from src import engine as E


def rearrange_clusters(image_list):
    """cluster -> member ids lists -> pseudo-label per id, in id order (`clustering.py:9-17`)."""
    ids, labels = [], []
    for cluster, images in enumerate(image_list):
        ids.extend(images)
        labels.extend([cluster] * len(images))
    return np.asarray(labels)[np.argsort(ids)]


@torch.no_grad()
def preprocess_features(npdata, pca=128):
    """[N, ndim] features -> [N, pca] PCA-reduced, whitened, L2-normalised (float32, on the device)."""
    x = torch.as_tensor(npdata, dtype=torch.float32).cuda().contiguous()
    n, d = x.shape
    xc = (x - x.mean(0, keepdim=True)).contiguous()
    cov = torch.empty(d, d, dtype=torch.float32, device=x.device)
    E.gemm(N.F32, 1, 1, d, d, n, xc, d, xc, d, cov, d, alpha=1.0 / n, out_f32=1)                 # xc^T xc / n
    lam, vec = np.linalg.eigh(cov.double().cpu().numpy())
    order = np.argsort(lam)[::-1][:pca]
    proj = (vec[:, order] * np.power(np.maximum(lam[order], 1e-20), -0.5)).astype(np.float32)    # [d, pca], eigen_power -0.5
    pt = torch.from_numpy(np.ascontiguousarray(proj.T)).cuda()                                    # [pca, d]: Linear weight layout
    y = torch.empty(n, pca, dtype=torch.float32, device=x.device)
    E.gemm(N.F32, 0, 0, n, pca, d, xc, d, pt, d, y, pca, out_f32=1)
    out = torch.empty_like(y)
    inv = torch.empty(n, dtype=torch.float32, device=x.device)
    N.call("l2norm_fwd", N.F32, y, n, pca, out, out, inv)
    return out


@torch.no_grad()
def run_kmeans(x, nmb_clusters, verbose=False, niter=20, seed=None):
    """x [N, d] (device or numpy) -> (cluster id per row as a python list, final loss = sum of squared distances)."""
    x = torch.as_tensor(x, dtype=torch.float32).cuda().contiguous()
    n, d = x.shape
    seed = np.random.randint(1234) if seed is None else seed      # the reference changes faiss's seed at every call this way
    pick = np.random.RandomState(seed).permutation(n)[:nmb_clusters]
    assert len(pick) == nmb_clusters, "fewer points than clusters"
    cent = x[torch.from_numpy(pick).cuda()].clone()
    dot = torch.empty(n, nmb_clusters, dtype=torch.float32, device=x.device)
    assign = torch.empty(n, dtype=torch.int64, device=x.device)
    sums = torch.empty(nmb_clusters, d, dtype=torch.float32, device=x.device)
    counts = torch.empty(nmb_clusters, dtype=torch.int32, device=x.device)
    bias = torch.empty(nmb_clusters, dtype=torch.float32, device=x.device)
    losses = []
    for it in range(niter + 1):
        N.call("row_sqnorm", cent, nmb_clusters, d, -0.5, bias)
        E.gemm(N.F32, 0, 0, n, nmb_clusters, d, x, d, cent, d, dot, nmb_clusters, bias=bias, out_f32=1)   # x.c - |c|^2 / 2
        N.call("row_argmax", dot, n, nmb_clusters, assign)
        best = dot.gather(1, assign[:, None])[:, 0]
        losses.append(float(((x * x).sum(1) - 2.0 * best).clamp_min(0).sum()))          # sum_i |x_i - c_a(i)|^2
        if it == niter:
            break
        N.call("kmeans_accumulate", x, assign, n, nmb_clusters, d, sums, counts)
        N.call("kmeans_update_mean", sums, counts, nmb_clusters, d, cent)
    if verbose:
        print("k-means loss evolution: {0}".format(np.array(losses)))
    return [int(v) for v in assign.cpu().tolist()], losses[-1]


class Kmeans(object):
    def __init__(self, k):
        self.k = k

    def cluster(self, data, verbose=False, pca=128):
        end = time.time()
        xb = preprocess_features(data, pca=pca)
        self.features = xb                                          # what was clustered: `silhouette_score(self.features, labels)`
        I, loss = run_kmeans(xb, self.k, verbose)
        self.images_lists = [[] for _ in range(self.k)]
        for i in range(len(data)):
            self.images_lists[I[i]].append(i)
        if verbose:
            print("k-means time: {0:.0f} s".format(time.time() - end))
        return loss


def _device(a, dtype):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


@torch.no_grad()
def make_graph(xb, nnn):
    """xb [n, d] -> (I int64 [n, nnn + 1], D fp32 [n, nnn + 1]) on the device, the layout of faiss's `search(xb, nnn + 1)`
    (`clustering.py:118-138`): column 0 is the row itself at distance 0, then its nnn nearest other rows, nearest first, equal
    distances by ascending row."""
    from src.evaluation.graph import knn_graph
    xb = _device(xb, torch.float32)
    idx, d2 = knn_graph(xb, nnn)
    n = xb.shape[0]
    I = torch.cat([torch.arange(n, device=idx.device)[:, None], idx], 1)
    D = torch.cat([torch.zeros(n, 1, dtype=torch.float32, device=d2.device), d2], 1)
    return I, D


@torch.no_grad()
def make_adjacencyW(I, D, sigma):
    """I, D as `make_graph` returns them (numpy or tensors; column 0 is dropped) -> the affinity matrix W = A + A^T,
    A_ij = exp(-D_ij / sigma^2), as a device CSR (`src.evaluation.graph.Csr`).  The reference's function of this name returns A
    and `run_pic` symmetrises it (`clustering.py:141-170`); nothing uses A alone, so the sum is formed here."""
    from src.evaluation.graph import pic_build
    idx = _device(I, torch.int64)[:, 1:]
    d2 = _device(D, torch.float32)[:, 1:]
    return pic_build(idx, d2, sigma)


@torch.no_grad()
def find_maxima_cluster(W, v):
    """`clustering.py:200-230`: every node points at the neighbour j with the largest positive W_ij (v_j - v_i) (itself if there is
    none) and takes the cluster of the local maximum its pointers lead to; maxima are numbered in ascending node order.
    -> int64 numpy array [n]."""
    from src.evaluation.graph import pic_assign
    label, _ = pic_assign(W, _device(v, torch.float64))
    return label.cpu().numpy().astype(np.int64)


@torch.no_grad()
def run_pic(I, D, sigma, alpha, niter=200):
    """`clustering.py:167-197` -> the raw PIC cluster of every node as a python list."""
    from src.evaluation.graph import pic_power
    W = make_adjacencyW(I, D, sigma)
    v = pic_power(W, alpha, niter)
    return [int(c) for c in find_maxima_cluster(W, v)]


def distribute_singletons(clust, I):
    """`clustering.py:271-287`: a cluster of one member joins the cluster of that member's first listed neighbour (I[s, 1:]) whose
    cluster is not a singleton; with no such neighbour it stays.  Every decision looks at the ORIGINAL clustering only, so the
    outcome does not depend on the order in which singletons are visited.  -> new int64 label array (labels keep their values)."""
    clust = np.asarray(clust, dtype=np.int64)
    I = np.asarray(I.cpu() if isinstance(I, torch.Tensor) else I)
    _, inverse, counts = np.unique(clust, return_inverse=True, return_counts=True)
    single = counts[inverse] == 1                                   # per node
    nb = I[:, 1:]
    ok = ~single[nb]                                                # neighbour's original cluster is not a singleton
    first = ok.argmax(1)
    move = single & ok.any(1)
    out = clust.copy()
    rows = np.nonzero(move)[0]
    out[rows] = clust[nb[rows, first[rows]]]
    return out


def lists_from_labels(clust):
    """labels -> `images_lists`: clusters in ascending order of their smallest member, members ascending."""
    clust = np.asarray(clust, dtype=np.int64)
    _, first, inverse = np.unique(clust, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                        # cluster ranks by smallest member
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    lists = [[] for _ in range(len(order))]
    for i, c in enumerate(rank[inverse]):
        lists[int(c)].append(i)
    return lists


class PIC(object):
    """Power-iteration clustering on a graph of nearest neighbours (`clustering.py:232-295`).
        args: for consistency with k-means init (unused)
        sigma: bandwidth of the Gaussian kernel (default 0.2)
        nnn: number of nearest neighbours (default 5)
        alpha: the damping of the power iteration (default 0.001)
        distribute_singletons: reassign each singleton to the cluster of its closest non-singleton neighbour
    `cluster(data)` sets `images_lists` (one list of member ids per cluster; clusters numbered in ascending order of their
    smallest member - the reference's order is that of a Python `set`) and returns 0."""

    def __init__(self, args=None, sigma=0.2, nnn=5, alpha=0.001, distribute_singletons=True):
        self.sigma = sigma
        self.alpha = alpha
        self.nnn = nnn
        self.distribute_singletons = distribute_singletons

    def cluster(self, data, verbose=False, pca=128):
        end = time.time()
        xb = preprocess_features(data, pca=pca)
        self.features = xb
        I, D = make_graph(xb, self.nnn)
        clust = np.asarray(run_pic(I, D, self.sigma, self.alpha), dtype=np.int64)
        if self.distribute_singletons:
            clust = distribute_singletons(clust, I)
        self.images_lists = lists_from_labels(clust)
        if verbose:
            print("pic time: {0:.0f} s".format(time.time() - end))
        return 0


def write_pseudolabel_csv(paths, kmeans, out_csv, header=None):
    """`store_clusters.py:142-159`: one `path,pseudolabel` line per file, in file order.  header: a first line (the
    `files,label` that `train_upstream.py --upstream unfused` reads); the reference writes none."""
    labels = rearrange_clusters(kmeans.images_lists)
    with open(out_csv, "w") as f:
        if header:
            f.write(header + "\n")
        for p, l in zip(paths, labels):
            f.write(f"{p},{int(l)}\n")
    return labels
