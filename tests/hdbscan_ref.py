"""float64 restatement of HDBSCAN's stages (src/evaluation/hdbscan.py, csrc/mst.hip), the fixtures of tests/test_host_hdbscan.py
and tests/test_gpu_hdbscan.py, and sklearn's own answer.  Nothing here needs a GPU.

Dense mutual-reachability matrix; Kruskal under the strict order (w, lo, hi) (on fp64 values, or on the fp32 BITS a kernel
wrote); a straightforward condensed tree on explicit member lists and excess-of-mass selection with the root excluded."""
import functools

import numpy as np

# n_blobs, per, noise, d, seed, min_samples, min_cluster_size      -> n = 232, 545, 191, 280
CASES = [(4, 40, 30, 8, 0, 5, 10), (6, 60, 80, 16, 1, 5, 15), (3, 50, 20, 4, 2, 3, 8), (5, 30, 60, 32, 3, 8, 8)]
# sklearn's HDBSCAN(algorithm="brute") in fp64: (clusters, noise points)
CASE_FACTS = [(4, 30), (6, 80), (3, 13), (5, 60)]


def make(n_blobs, per, noise, d, seed, spread=0.15):
    r = np.random.default_rng(seed)
    c = r.normal(size=(n_blobs, d)) * 3
    x = np.concatenate([c[i] + spread * (1 + i % 3) * r.normal(size=(per + 7 * i, d)) for i in range(n_blobs)]
                       + [r.uniform(-8, 8, size=(noise, d))]).astype(np.float32)
    return x[r.permutation(len(x))]


@functools.lru_cache(maxsize=None)
def case_points(case):
    x = make(*CASES[case][:5])
    x.setflags(write=False)
    return x


def sq_dists(x):
    """float64 |x_i - x_j|^2 by differences (no cancellation)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((len(x), len(x)))
    for i in range(len(x)):
        out[i] = ((x - x[i]) ** 2).sum(1)
    return out


def mutual_reachability2(x, min_samples):
    """-> (w2 float64 [n, n], core2 [n]): core2_i = the min_samples-th smallest d2 of row i COUNTING d2_ii = 0 (sklearn's
    convention), w2_ij = max(d2_ij, core2_i, core2_j).  Squared throughout: max and the order commute with the square root."""
    d2 = sq_dists(x)
    core2 = np.sort(d2, axis=1)[:, min_samples - 1] if min_samples > 1 else np.zeros(len(d2))
    return np.maximum(d2, np.maximum(core2[:, None], core2[None, :])), core2


def kruskal(w):
    """w [n, n] symmetric (any dtype that orders as its values: float64, or the uint32 bits of non-negative fp32) -> (u, v, w_uv)
    of the unique minimum spanning tree under the strict order (w, lo, hi), in that order."""
    n = len(w)
    iu, iv = np.triu_indices(n, 1)
    ww = w[iu, iv]
    order = np.lexsort((iv, iu, ww))
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    u, v, out = [], [], []
    for e in order.tolist():
        a, b = find(int(iu[e])), find(int(iv[e]))
        if a != b:
            parent[a] = b
            u.append(int(iu[e])); v.append(int(iv[e])); out.append(ww[e])
            if len(u) == n - 1:
                break
    return np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64), np.asarray(out, dtype=w.dtype)


def scipy_mst(w):
    """w [n, n] float64, symmetric, no zero off the diagonal -> (u, v, w_uv) with u < v."""
    from scipy.sparse.csgraph import minimum_spanning_tree
    t = minimum_spanning_tree(np.triu(w, 1)).tocoo()
    assert len(t.data) == len(w) - 1
    return np.minimum(t.row, t.col).astype(np.int64), np.maximum(t.row, t.col).astype(np.int64), t.data.astype(np.float64)


def is_spanning_tree(u, v, n):
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    if len(u) != n - 1:
        return False
    for a, b in zip(u.tolist(), v.tolist()):
        a, b = find(a), find(b)
        if a == b:
            return False
        parent[a] = b
    return True


def hdbscan_plain(u, v, w, n, min_cluster_size):
    """Tree edges with distances w -> (labels by smallest member with -1 = noise, probabilities, clusters).  Member lists all the
    way: every dendrogram node knows its points; a cluster is a dict."""
    order = np.lexsort((v, u, w))
    node_of = list(range(n))                                                  # union-find over points -> current node
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    members = {i: [i] for i in range(n)}
    kids = {}
    for t, e in enumerate(order.tolist()):
        a, b = find(int(u[e])), find(int(v[e]))
        na, nb = node_of[a], node_of[b]
        parent[a] = b
        node_of[b] = n + t
        members[n + t] = members[na] + members[nb]
        kids[n + t] = (na, nb, float(w[e]))
    clusters = [dict(parent=None, birth=0.0, rows=[], sub=[])]               # rows: (lambda, point) that fell out of it
    todo = [(2 * n - 2, 0)]
    while todo:
        node, c = todo.pop()
        if node < n:
            continue
        a, b, dist = kids[node]
        lam = 1.0 / dist if dist > 0 else np.inf
        big = [s for s in (a, b) if len(members[s]) >= min_cluster_size]
        if len(big) == 2:
            for s in big:
                clusters.append(dict(parent=c, birth=lam, rows=[], sub=[], size=len(members[s])))
                clusters[c]["sub"].append(len(clusters) - 1)
                todo.append((s, len(clusters) - 1))
        else:
            for s in (a, b):
                if s in big:
                    todo.append((s, c))
                else:
                    clusters[c]["rows"] += [(lam, p) for p in members[s]]

    def stability(c):
        cl = clusters[c]
        own = sum(lam - cl["birth"] for lam, _ in cl["rows"])
        return own + sum(clusters[s]["size"] * (clusters[s]["birth"] - cl["birth"]) for s in cl["sub"])

    def best(c):                                                             # -> (stability of the best choice below c, that choice)
        below, chosen = 0.0, []
        for s in clusters[c]["sub"]:
            sv, sc = best(s)
            below += sv
            chosen += sc
        own = stability(c)
        return (below, chosen) if below > own else (own, [c])
    chosen = []
    for s in clusters[0]["sub"]:                                             # the root is excluded
        chosen += best(s)[1]

    def points_under(c):
        out = list(clusters[c]["rows"])
        for s in clusters[c]["sub"]:
            out += points_under(s)
        return out
    labels = np.full(n, -1, dtype=np.int64)
    prob = np.zeros(n)
    for c in chosen:
        death = max([lam for lam, _ in clusters[c]["rows"]] + [clusters[s]["birth"] for s in clusters[c]["sub"]])
        for lam, p in points_under(c):
            labels[p] = c
            prob[p] = 1.0 if death == 0.0 or np.isinf(lam) else min(lam, death) / death
    return renumber(labels), prob, len(chosen)


def renumber(label):
    """Ids >= 0 -> 0 .. C - 1 in the order of each group's smallest member; -1 stays."""
    label = np.asarray(label)
    out = np.full(len(label), -1, dtype=np.int64)
    seen = {}
    for i, l in enumerate(label.tolist()):
        if l >= 0:
            out[i] = seen.setdefault(l, len(seen))
    return out


@functools.lru_cache(maxsize=None)
def sklearn_answer(case):
    """-> (labels, probabilities) of sklearn's HDBSCAN on the fp64 copy of the case, brute force."""
    from sklearn.cluster import HDBSCAN
    ms, mcs = CASES[case][5:]
    h = HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute").fit(np.asarray(case_points(case), dtype=np.float64))
    return h.labels_.astype(np.int64), h.probabilities_.astype(np.float64)


def assert_same_clustering(labels, want):
    """ARI exactly 1.0, equal noise sets, equal cluster counts."""
    from sklearn.metrics import adjusted_rand_score
    labels, want = np.asarray(labels), np.asarray(want)
    assert np.array_equal(labels < 0, want < 0), "noise sets differ"
    assert labels.max(initial=-1) == want.max(initial=-1), "cluster counts differ"
    assert adjusted_rand_score(want, labels) == 1.0
