"""The exact neighbour graph and the PIC stages on the GPU: `audiossl_knn_graph_l2`, `audiossl_pic_build`, `audiossl_pic_power`,
`audiossl_pic_assign` against the int64 / float64 restatements of tests/pic_ref.py and what the reference's own code recorded
(tests/golden/pic_reference.npz), the Python layer above them and the labeler command.

Bars.  Graph on real data: bar = 8 sqrt(d) 2^-24 max_i |x_i|^2 (the bound cka.hip's sigma^2 test uses for the same fp32 chain).
CSR: rowptr and col EQUAL, w within 2 ulp (float64).  v after 200 iterations: 16 (maxdeg + 4) 2^-53 relative per entry (one
iteration errs by a few ulp per row term; alpha * rowsum < 1 damps what is carried over).  Every case prints error / bar (the
table of DESIGN.md section 15)."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import pic_ref as R
from oracle import fill

pytestmark = pytest.mark.gpu

GUARD = 2
EPS24, EPS53 = 2.0 ** -24, 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pic_reference.npz")


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(GOLDEN, allow_pickle=False))


def _ws(nbytes):
    return torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")          # the kernels clear what they need


def _guarded(rows, cols, dtype, pattern):
    t = torch.empty(rows + GUARD, cols, dtype=dtype)
    t[:rows] = float("nan") if dtype.is_floating_point else -5
    t[rows:] = (torch.arange(GUARD * cols).view(GUARD, cols) + pattern).to(dtype)
    return t


def _launch_graph(x, k):
    """x [n, d] fp32 CPU (d % 4 == 0) -> (idx int32 [n, k], d2 fp32 [n, k]) on the CPU, guards and workspace checked."""
    from src import _native as N
    from src.evaluation.graph import graph_workspace_bytes
    n, d = x.shape
    idx, d2 = _guarded(n, k, torch.int32, 77), _guarded(n, k, torch.float32, 1000.5)
    idx_d, d2_d = idx.cuda(), d2.cuda()
    nbytes = graph_workspace_bytes(n, k)
    ws = _ws(nbytes)
    xd = x.cuda()
    N.call("knn_graph_l2", xd, n, d, k, idx_d, d2_d, ws, nbytes)
    torch.cuda.synchronize()
    assert torch.equal(idx_d[n:].cpu(), idx[n:]) and torch.equal(d2_d[n:].cpu(), d2[n:]), "guard rows overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "workspace overrun"
    assert torch.equal(xd.cpu(), x)
    return idx_d[:n].cpu(), d2_d[:n].cpu()


def _launch_build(idx, d2, sigma):
    """idx [n, k], d2 [n, k] numpy -> (rowptr, col, w) numpy, trimmed to nnz; plus the device tensors for the later stages."""
    from src import _native as N
    from src.evaluation.graph import pic_workspace_bytes
    n, k = idx.shape
    cap = 2 * n * k
    rowptr = torch.full((n + 1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    col = torch.full((cap + GUARD,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((cap + GUARD,), -7.5, dtype=torch.float64, device="cuda")
    nnz = torch.full((1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    nbytes = pic_workspace_bytes(n, k)
    ws = _ws(nbytes)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx)).to(torch.int32).cuda()
    d2_d = torch.from_numpy(np.ascontiguousarray(d2)).float().cuda()
    N.call("pic_build", idx_d, d2_d, n, k, float(sigma), rowptr, col, w, nnz, ws, nbytes)
    torch.cuda.synchronize()
    m = int(nnz[0])
    assert bool((rowptr[n + 1:] == -7).all()) and bool((nnz[1:] == -7).all()), "guard entries overwritten"
    assert bool((col[m:] == -7).all()) and bool((w[m:] == -7.5).all()), "entries past nnz written"
    assert bool((ws[nbytes:] == 0xA5).all()), "workspace overrun"
    return rowptr[:n + 1], col[:cap], w[:cap], m


def _launch_power(rowptr, col, w, n, alpha, iters=R.ITERS):
    from src import _native as N
    from src.evaluation.graph import pic_workspace_bytes
    v = torch.full((n + GUARD,), -7.5, dtype=torch.float64, device="cuda")
    nbytes = pic_workspace_bytes(n, 1)
    ws = _ws(nbytes)
    N.call("pic_power", rowptr, col, w, n, col.numel(), float(alpha), iters, v, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((v[n:] == -7.5).all()) and bool((ws[nbytes:] == 0xA5).all())
    return v[:n]


def _launch_assign(rowptr, col, w, v, n):
    from src import _native as N
    from src.evaluation.graph import pic_workspace_bytes
    label = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    nbytes = pic_workspace_bytes(n, 1)
    ws = _ws(nbytes)
    N.call("pic_assign", rowptr, col, w, v.contiguous(), n, col.numel(), label, count, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((label[n:] == -7).all()) and bool((count[1:] == -7).all()) and bool((ws[nbytes:] == 0xA5).all())
    return label[:n].cpu().numpy().astype(np.int64), int(count[0])


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g)


def _check_exact(x, k):
    want_i, want_d = R.knn_graph(x.numpy(), k)
    idx, d2 = _launch_graph(x.float(), k)
    np.testing.assert_array_equal(d2.numpy().astype(np.float64), want_d.astype(np.float64))
    np.testing.assert_array_equal(idx.numpy().astype(np.int64), want_i)
    return want_i, want_d


# ---- 1. exact cases, ties included -------------------------------------------------------------------------------------
# (1100, 32, 64): 18 row tiles and 9 walked tiles - the walked rows are split over blockIdx.y there, and k fills every lane
@pytest.mark.parametrize("n,d,k", [(2, 4, 1), (5, 4, 4), (127, 36, 5), (128, 64, 5), (129, 68, 6), (300, 512, 5), (1100, 32, 64)])
def test_graph_exact_on_integer_inputs_ties_by_ascending_row(n, d, k):
    """Entries in -2..2: every dot product, norm and distance is an integer below 2^24, exact in fp32 in any order.  Heavy ties
    (at most 16 d + 1 distinct distances per row): idx and d2 must be EQUAL to the int64 brute force under (d2, j)."""
    want_i, want_d = _check_exact(_ints((n, d), 31 + n), k)
    if n >= 127:
        assert int((want_d[:, 1:] == want_d[:, :-1]).sum()) > 0                     # the case does contain ties


def test_graph_duplicate_rows_are_neighbours_and_self_is_not():
    """Self leaves by index, not by value: a duplicate of row i is its neighbour at distance exactly 0, i itself never is."""
    x = _ints((130, 8), 5)
    x[70] = x[0]
    x[129] = x[0]
    x[64] = x[3]
    x[1] = 0                                                                        # the origin is a legitimate point
    want_i, want_d = _check_exact(x, 6)
    assert want_i[0, :2].tolist() == [70, 129] and want_d[0, :2].tolist() == [0, 0]
    assert want_i[70, :2].tolist() == [0, 129] and want_i[129, :2].tolist() == [0, 70] and want_i[3, 0] == 64
    _check_exact(torch.zeros(66, 4, dtype=torch.int64), 3)                          # all rows equal: neighbours 0, 1, 2, .. minus self


def test_graph_k_equal_n_minus_1():
    for n in (65, 7):
        want_i, _ = _check_exact(_ints((n, 12), 900 + n), n - 1)
        assert all(sorted(want_i[i].tolist()) == [j for j in range(n) if j != i] for i in range(n))


# ---- 2. real data ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real_case(n, d, seed):
    x = np.random.RandomState(seed).randn(n, d).astype(np.float32)
    dist = R.sq_dists(x)
    np.fill_diagonal(dist, np.inf)
    return x, dist, np.sort(dist, axis=1)


@pytest.mark.parametrize("n,d,k,seed,need_equal", [(300, 32, 5, 1, True), (1100, 64, 5, 2, True), (1100, 64, 64, 2, False),
                                                   (257, 512, 6, 3, False)])
def test_graph_on_real_data(n, d, k, seed, need_equal):
    x, dist, srt = _real_case(n, d, seed)
    bar = 8.0 * np.sqrt(d) * EPS24 * float((x.astype(np.float64) ** 2).sum(1).max())
    idx, d2 = _launch_graph(torch.from_numpy(x), k)
    idx, d2 = idx.numpy().astype(np.int64), d2.numpy().astype(np.float64)
    rows = np.arange(n)[:, None]
    assert (idx >= 0).all() and (idx < n).all() and (idx != rows).all(), "self or out-of-range index"
    assert all(len(set(r.tolist())) == k for r in idx), "repeated neighbour"
    assert (np.diff(d2, axis=1) >= 0).all(), "row not sorted"
    true_d = dist[rows, idx]
    err = float(np.abs(d2 - true_d).max())
    slack = float((true_d[:, k - 1] - srt[:, k - 1]).max())
    print(f"graph n {n} d {d} k {k}: |d2 - fp64| / bar = {err / bar:.3f}, (k-th returned - true k-th) / (2 bar) = {slack / (2 * bar):.3f}")
    assert err <= bar
    assert slack <= 2 * bar
    if need_equal:
        want = np.argsort(dist, axis=1, kind="stable")[:, :k]
        exempt = (np.diff(srt[:, :k + 1], axis=1) < 2 * bar).any(1)
        differ = (idx != want).any(1)
        print(f"graph n {n} d {d} k {k}: {int(exempt.sum())} exempt rows, {int(differ.sum())} rows differ from fp64")
        assert exempt.mean() <= 0.01
        assert not (differ & ~exempt).any()


# ---- 3. CSR: the hub and the fixture ---------------------------------------------------------------------------------------
def _check_csr(I, D, sigma):
    n = I.shape[0]
    want_ptr, want_col, want_w = R.adjacency(I, D, sigma)
    rowptr, col, w, nnz = _launch_build(I[:, 1:], D[:, 1:], sigma)
    assert nnz == len(want_col)
    np.testing.assert_array_equal(rowptr.cpu().numpy().astype(np.int64), want_ptr)
    np.testing.assert_array_equal(col[:nnz].cpu().numpy().astype(np.int64), want_col)
    ulp = float(R.ulp_diff(w[:nnz].cpu().numpy(), want_w).max())
    maxdeg = int(np.diff(want_ptr).max())
    print(f"csr n {n}: nnz {nnz}, max degree {maxdeg}, w error {ulp:.2f} ulp (bar 2)")
    assert ulp <= 2.0
    return (rowptr, col, w, nnz), (want_ptr, want_col, want_w), maxdeg


def test_csr_hub_row_of_full_in_degree():
    """The origin plus 1,099 random unit vectors: the origin is at distance 1 from every point, nearer than anything else in
    d = 64, so it is in every list and its row of W has 1,099 entries - far beyond the k + a few of an ordinary row."""
    g = np.random.RandomState(7)
    x = g.randn(1100, 64)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[0] = 0.0
    I, D = R.make_graph(x.astype(np.float32), 5)
    assert (I[1:, 1:] == 0).any(1).all()
    (rowptr, _, _, _), _, maxdeg = _check_csr(I, D, 0.7)
    assert maxdeg == 1099 and int(rowptr[1]) - int(rowptr[0]) == 1099
    # the kernel's own graph of the same points has the hub too
    idx, _ = _launch_graph(torch.from_numpy(x.astype(np.float32)), 5)
    assert bool((idx[1:] == 0).any(1).all())


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_pic_stages_on_the_reference_fixture(case):
    gold = _gold()
    I, D = gold[f"I_{case}"], gold[f"D_{case}"]
    n = I.shape[0]
    (rowptr, col, w, nnz), (want_ptr, want_col, want_w), maxdeg = _check_csr(I, D, R.SIGMA)
    v = _launch_power(rowptr, col, w, n, R.ALPHA)
    want_v = R.power(want_ptr, want_col, want_w, R.ALPHA)
    bar = 16.0 * (maxdeg + 4) * EPS53
    rel = float((np.abs(v.cpu().numpy() - want_v) / want_v).max())
    print(f"pic case {case}: v relative error / bar = {rel / bar:.4f} (bar {bar:.3g}, max degree {maxdeg})")
    assert rel <= bar
    assert abs(float(v.sum()) - 1.0) <= 1e-13
    label, count = _launch_assign(rowptr, col, w, v, n)
    want_raw = gold[f"raw_{case}"]
    assert count == len(set(want_raw.tolist())) and label.min() == 0 and label.max() == count - 1
    np.testing.assert_array_equal(label, want_raw)                     # roots in ascending node order: the reference's own ids
    # the Python layer: run_pic on the recorded graph, then the singleton rule and the numbering
    from src.upstream.decar_v2 import clustering as CL
    raw = np.asarray(CL.run_pic(I, D, R.SIGMA, R.ALPHA))
    np.testing.assert_array_equal(raw, want_raw)
    final = CL.rearrange_clusters(CL.lists_from_labels(CL.distribute_singletons(raw, I)))
    np.testing.assert_array_equal(final, R.renumber(gold[f"final_{case}"]))
    # and from the points themselves: the kernel's graph is the recorded one
    x = gold[f"x_{case}"]
    I2, D2 = CL.make_graph(x, R.NNN)
    I2, D2 = I2.cpu().numpy(), D2.cpu().numpy().astype(np.float64)
    gbar = 8.0 * np.sqrt(x.shape[1]) * EPS24 * float((x.astype(np.float64) ** 2).sum(1).max())
    dist = R.sq_dists(x)
    np.fill_diagonal(dist, np.inf)
    clear = (np.diff(np.sort(dist, axis=1)[:, :R.NNN + 1], axis=1) >= 2 * gbar).all(1)       # rows whose order fp32 can resolve
    np.testing.assert_array_equal(I2[clear], I[clear])
    assert (I2[:, 0] == np.arange(n)).all() and (D2[:, 0] == 0).all()
    assert float(np.abs(D2[clear] - D[clear]).max()) <= gbar + EPS24                           # D is the fp64 distance rounded to fp32


def test_ring_graph_every_node_is_a_root():
    n = 12
    i = np.arange(n)
    I = np.stack([i, (i + 1) % n, (i - 1) % n], 1)
    D = np.concatenate([np.zeros((n, 1)), np.full((n, 2), 0.3)], 1).astype(np.float32)
    from src.upstream.decar_v2 import clustering as CL
    assert CL.run_pic(I, D, 0.2, 0.001) == list(range(n))


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------
def test_two_launches_agree_bit_for_bit():
    x = torch.from_numpy(np.random.RandomState(4).randn(1100, 64).astype(np.float32))
    a, b = _launch_graph(x, 7), _launch_graph(x, 7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    idx, d2 = a[0].numpy(), a[1].numpy()
    outs = []
    for _ in range(2):
        rowptr, col, w, nnz = _launch_build(idx, d2, 3.0)
        v = _launch_power(rowptr, col, w, 1100, 0.001, iters=20)
        label, count = _launch_assign(rowptr, col, w, v, 1100)
        outs.append((rowptr.cpu(), col[:nnz].cpu(), w[:nnz].cpu().view(torch.int64), v.cpu().view(torch.int64), torch.from_numpy(label), count))
    for p, q in zip(*outs):
        assert (p == q) if isinstance(p, int) else torch.equal(p, q)


def test_two_points():
    x = torch.tensor([[1.0, 2.0, 0.0, -1.0], [0.5, 2.0, 1.0, -1.0]])
    idx, d2 = _launch_graph(x, 1)
    assert idx.tolist() == [[1], [0]] and d2.tolist() == [[1.25], [1.25]]
    rowptr, col, w, nnz = _launch_build(idx.numpy(), d2.numpy(), 1.0)
    assert nnz == 2 and rowptr.tolist() == [0, 1, 2] and col[:2].tolist() == [1, 0]
    assert float(R.ulp_diff(w[:2].cpu().numpy(), np.full(2, 2.0 * np.exp(-1.25))).max()) <= 2.0
    v = _launch_power(rowptr, col, w, 2, 0.001)
    assert v.tolist() == [0.5, 0.5]
    label, count = _launch_assign(rowptr, col, w, v, 2)
    assert label.tolist() == [0, 1] and count == 2
    v = _launch_power(rowptr, col, w, 2, 0.001, iters=0)
    assert v.tolist() == [0.5, 0.5]


def test_bad_arguments_are_refused_before_any_launch():
    from src import _native as N
    from src.evaluation.graph import graph_workspace_bytes, knn_graph, pic_workspace_bytes
    for what, got, want in R.bad_argument_codes(N.lib(), graph_workspace_bytes(100, 5), pic_workspace_bytes(100, 5)):
        assert got == want, what
    assert torch.cuda.is_available()
    torch.cuda.synchronize()                                            # nothing was launched: nothing can have faulted
    x = torch.zeros(10, 6, device="cuda")
    for k in (0, 10, 65):
        with pytest.raises(ValueError):
            knn_graph(x, k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn_graph(x.cpu(), 2)


def test_knn_graph_pads_the_width():
    x = torch.from_numpy(np.random.RandomState(9).randn(90, 30).astype(np.float32))
    from src.evaluation.graph import knn_graph
    idx, d2 = knn_graph(x.cuda(), 4)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and idx.shape == (90, 4)
    want_i, want_d = R.knn_graph(x.numpy(), 4)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_allclose(d2.cpu().numpy(), want_d, rtol=0, atol=8.0 * np.sqrt(32) * EPS24 * float((x ** 2).sum(1).max()))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
def _three_blobs():
    """Three well-separated blobs (centres 4 N(0, I)), each made of ten tight groups of ten points (group offsets N(0, I),
    jitter 0.1).  The groups matter: PCA-whitening gives every kept direction unit variance, so plain isotropic noise around
    three centres - two directions of signal - would be blown up to fourteen of the sixteen whitened dimensions and the
    blobs would dissolve (the restatement shows it: ~100 of 1,500 edges cross blobs).  Here the kept directions are the
    spread of the thirty groups and the jitter stays small."""
    g = np.random.RandomState(12)
    centres = g.randn(3, 32) * 4.0
    protos = g.randn(30, 32)
    which = np.arange(300) % 3
    group = (np.arange(300) // 3) % 10
    return (centres[which] + protos[which * 10 + group] + 0.1 * g.randn(300, 32)).astype(np.float32), which


def test_pic_does_not_mix_separated_blobs():
    from oracle import kmeans as OK
    from src.upstream.decar_v2.clustering import PIC, rearrange_clusters
    feats, which = _three_blobs()
    # the restatement first, on the CPU: whitened features -> graph -> PIC
    I, D = R.make_graph(OK.pca_whiten_l2(feats, 16).astype(np.float32), 5)
    _, final, _ = R.pic(I, D)
    for c in range(final.max() + 1):
        assert len(set(which[final == c].tolist())) == 1, "the restatement mixes blobs"
    model = PIC()
    assert model.cluster(feats, pca=16) == 0
    labels = rearrange_clusters(model.images_lists)
    assert sorted(i for l in model.images_lists for i in l) == list(range(300))
    assert [l[0] for l in model.images_lists] == sorted(l[0] for l in model.images_lists)      # numbered by smallest member
    assert all(l == sorted(l) for l in model.images_lists)
    for c in range(len(model.images_lists)):
        assert len(set(which[labels == c].tolist())) == 1, f"cluster {c} mixes blobs"
    assert 3 <= len(model.images_lists) <= 100


def _checkpoint(tmp_path, cfg_s):
    from src.encoder import AudioNTT2020Task6
    from src.upstream.delores_s.upstream_expert import Upstream_Expert
    expert = Upstream_Expert(copy.deepcopy(cfg_s), base_encoder=AudioNTT2020Task6)
    fill.fill_state_dict_(expert, seed=9)
    ck = expert.checkpoint()
    ck["hyper_parameters"]["config"] = expert.config                  # as HipTrainer.save_checkpoint writes it
    ck["hyper_parameters"]["base_encoder"] = expert.config["pretrain"]["base_encoder"]["type"]
    path = str(tmp_path / "delores_s.ckpt")
    torch.save(ck, path)
    return path


def _write_wavs(tmp_path, lengths, salt):
    from scipy.io import wavfile
    files = []
    for i, L in enumerate(lengths):
        w = fill.uniform((L,), salt + i, -0.3, 0.3) + 0.2 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(L) / 16000).astype(np.float32)
        p = str(tmp_path / f"clip{salt}_{i}.wav")
        wavfile.write(p, 16000, (w * 32767).astype(np.int16))
        files.append(p)
    return files


def test_store_clusters_pic_command(tmp_path, cfg_s, capsys):
    import types

    import pandas as pd
    from src.upstream.decar_v2 import store_clusters as sc
    ckpt = _checkpoint(tmp_path, cfg_s)
    files = _write_wavs(tmp_path, [16000 + 500 * (i % 3) for i in range(12)], salt=300)
    files_csv, out_csv, km_csv = str(tmp_path / "files.csv"), str(tmp_path / "pic.csv"), str(tmp_path / "km.csv")
    pd.DataFrame({"files": files}).to_csv(files_csv, index=False)
    base = ["--checkpoint", ckpt, "--upstream", "delores_s", "--input", files_csv, "--pca", "8", "--window", "center"]
    # the default command is what it was: the parent's pipeline (embed -> Kmeans(k).cluster -> CSV), restated from the same
    # library calls on the same seed, writes the same bytes as `--k 3` and as `--clustering kmeans --k 3`
    from src.evaluation.embed import extract_embeddings, load_embedder
    from src.upstream.decar_v2.clustering import Kmeans, write_pseudolabel_csv
    embedder = load_embedder(ckpt, "delores_s", config=None, layer="backbone")
    feats = extract_embeddings(embedder, files, batch_size=64, window="center", duration=1.0)
    np.random.seed(2)
    km = Kmeans(3)
    loss = km.cluster(feats, verbose=False, pca=8)
    write_pseudolabel_csv(files, km, str(tmp_path / "parent.csv"), header="files,label")
    want = open(tmp_path / "parent.csv", "rb").read()
    for name, extra in (("km.csv", []), ("km2.csv", ["--clustering", "kmeans"])):
        np.random.seed(2)
        sc.main(sc.get_args(base + extra + ["--k", "3", "--out", str(tmp_path / name)]))
        assert open(tmp_path / name, "rb").read() == want
        assert f"12 files, 3 clusters, k-means loss {loss:.6g} -> " in capsys.readouterr().out

    labels = sc.main(sc.get_args(base + ["--clustering", "pic", "--nnn", "3", "--out", out_csv, "--compare", km_csv]))
    text = capsys.readouterr().out
    lines = open(out_csv).read().split()
    assert lines[0] == "files,label" and len(lines) == 13
    assert [ln.rsplit(",", 1)[0] for ln in lines[1:]] == files                       # every file once, in order
    got = [int(ln.rsplit(",", 1)[1]) for ln in lines[1:]]
    count = max(got) + 1
    assert sorted(set(got)) == list(range(count)) and got == [int(l) for l in labels]         # labels 0..C-1 all used
    assert f"12 files, {count} clusters, pic" in text and "NMI against" in text
    nmi = float(text.split("NMI against")[1].split(":")[1])
    assert 0.0 <= nmi <= 1.0
    # what `train_upstream.py --upstream unfused` does with that file
    from src.dataset.upstream_dataset import BaseDataset
    ds = BaseDataset(copy.deepcopy(cfg_s), types.SimpleNamespace(upstream="unfused"), out_csv, tfms=None)
    assert len(ds) == 12 and ds.labelled
    wave, label = ds[5]
    assert 0 <= label < count and len(wave) == 16000 + 500 * (5 % 3)
