"""The norm kernel of csrc/gram_tile.h runs the Gram tile's own fmaf chain - on REAL-VALUED data, through the three users of the tile.

(n_i + n_j) - 2 g_ij is exactly 0 on a repeated row only if n_i carries the roundings g_ij does.  On integer inputs (every other
duplicate-row test) any summation order is exact and a norm kernel in the wrong chain order would pass; on randn entries it leaves a
rounding residue on every duplicate pair, of either sign, and the clamp at 0 hides only the negative ones.

x = randn(130, 36): d = 36 is a multiple of 4 but not of 8 and one full feature chunk plus a partial one (the `col + 4 < d` guard and
the zero-filled tail of the staging); n = 130 is two owned blocks and two walked tiles.  Rows 70 and 129 repeat row 0, row 64 repeats
row 63, row 128 repeats row 127: the duplicates straddle the owned-block edge, the walked-tile edge and the last partial tile.
d = 34 is the same through the Python layers' zero padding to a multiple of 4.

The seeds.  At d = 36 the two chain orders round a row's norm to the same float for about two rows in three, and the sign of the
residue where they differ is the row's own.  The seeds below were picked with a numpy emulation of both fmaf chains (fp64 product
and sum, rounded to fp32 per step; no kernel run): under the OTHER order rows 0 and 63 get a smaller norm and row 127 a larger one, at
d = 36 and at d = 34, and the silhouette's repeated vector a larger one.  So a norm in halves order under the index-order tile puts
row 128 at a positive distance from row 127 and makes the 70 equal rows score below 1, and a norm in index order under the
halves-order tile counts the pairs of rows 0 and 63 among CKA's non-zero distances.  A build with the two norm orders swapped did
exactly that on MI355X: d2 = 7.6e-6 between rows 127 and 128, a count of 8384 where 8380 is due, 0.99969 for the 70 equal rows - all
five cases failed."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, D, K = 130, 36, 6
TRIPLE = (0, 70, 129)
PAIRS = ((63, 64), (127, 128))


@functools.lru_cache(maxsize=None)
def _points():
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(20277))
    x[70] = x[0]
    x[129] = x[0]
    x[64] = x[63]
    x[128] = x[127]
    return x


@pytest.mark.parametrize("d", [36, 34])
def test_graph_lists_real_valued_duplicates_at_distance_zero(d):
    from src.evaluation.graph import knn_graph
    idx, d2 = knn_graph(_points()[:, :d].cuda(), K)
    idx, d2 = idx.cpu(), d2.cpu()
    for i in TRIPLE:
        others = sorted(j for j in TRIPLE if j != i)
        print(f"d {d} row {i}: idx {idx[i].tolist()} d2 {d2[i].tolist()}")
        assert idx[i, :2].tolist() == others and d2[i, 0].item() == 0.0 and d2[i, 1].item() == 0.0
        assert bool((d2[i, 2:] > 0).all())
    for a, b in PAIRS:
        print(f"d {d} rows {a}, {b}: idx {idx[a].tolist()} / {idx[b].tolist()} d2 {d2[a, :2].tolist()} / {d2[b, :2].tolist()}")
        assert idx[a, 0].item() == b and d2[a, 0].item() == 0.0 and d2[a, 1].item() > 0.0
        assert idx[b, 0].item() == a and d2[b, 0].item() == 0.0 and d2[b, 1].item() > 0.0
    assert not bool((idx == torch.arange(N)[:, None]).any()), "a row lists itself"


@pytest.mark.parametrize("d", [36, 34])
def test_cka_sigma2_counts_every_distance_but_the_duplicates(d):
    from src.evaluation.cka import median_sigma2
    s2, count = median_sigma2(_points()[:, :d].cuda(), center=False)         # uncentred: the kernels see the rows the seed was picked for
    zero_pairs = 3 + len(PAIRS)                                              # three equal rows are 3 pairs
    print(f"d {d}: sigma2 {float(s2):.6g} count {int(count)} (all pairs {N * (N - 1) // 2}, duplicate pairs {zero_pairs})")
    assert int(count) == N * (N - 1) // 2 - zero_pairs
    assert float(s2) > 0.0


def test_silhouette_of_a_cluster_of_equal_real_valued_rows_is_exactly_one():
    """Rows 0..69 are one random vector (cluster 0: a_i is a sum of exact zeros, so s_i = (b - 0) / b = 1), rows 70..129 distinct."""
    from src.evaluation.graph import silhouette_samples
    g = torch.Generator().manual_seed(20278)
    x = torch.randn(N, D, generator=g)
    x[:70] = torch.randn(D, generator=g)
    labels = torch.cat([torch.zeros(70, dtype=torch.int64), torch.ones(N - 70, dtype=torch.int64)])
    s = silhouette_samples(x.cuda(), labels).cpu()
    print(f"cluster 0: min {float(s[:70].min())!r} max {float(s[:70].max())!r}; cluster 1: min {float(s[70:].min()):.4f} max {float(s[70:].max()):.4f}")
    assert bool((s[:70] == 1.0).all())
    assert bool(torch.isfinite(s).all()) and bool((s[70:] < 1.0).all())
