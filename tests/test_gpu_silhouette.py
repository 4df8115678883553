"""`audiossl_silhouette` on the GPU against the float64 restatement of tests/silhouette_ref.py (itself checked against sklearn on the
CPU), the Python layer above it and the labeler's `--score` / `--k_sweep`.

Tolerance, derived from the arithmetic: bar = 8 sqrt(d_pad) 2^-24 max_i |x_i|^2 bounds the error of the squared distance out of the
fp32 Gram tile (the bound tests/test_gpu_graph.py uses; DESIGN.md section 15 measured 0.11 - 0.16 of it).  With d_min / d_max the
smallest non-zero / the largest float64 distance of the case, a distance errs by at most delta = bar / (2 d_min) + 2^-23 d_max (the
square root's derivative at d_min, plus its own rounding and the conversion).  Every sum after the square root is fp64, so the means
a and b err by delta too, and s = (b - a) / max(a, b) by at most 3 delta / max(a, b) - plus 1e-12 for the restatement itself.  The
bound needs d_min^2 well above bar (asserted: >= 64 bar; a condition on the inputs).  Every case prints max error / tolerance before
it asserts (the table of DESIGN.md section 16)."""
import copy
import functools

import numpy as np
import pytest
import torch

import silhouette_ref as R
from oracle import fill

pytestmark = pytest.mark.gpu

GUARD = 2
EPS24 = 2.0 ** -24


def _launch(xs, seg):
    """xs [n, d] fp32 CPU tensor sorted by cluster (d % 4 == 0), seg [K + 1] int32 CPU tensor -> s fp64 [n] on the CPU, in the
    sorted order; guard entries, the workspace's end and the inputs checked."""
    from src import _native as N
    from src.evaluation.graph import silhouette_workspace_bytes
    n, d = xs.shape
    K = seg.numel() - 1
    s = torch.full((n + GUARD,), -7.5, dtype=torch.float64, device="cuda")
    nbytes = silhouette_workspace_bytes(n)
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")              # the kernels clear nothing and need nothing cleared
    xd, segd = xs.cuda(), seg.cuda()
    N.call("silhouette", xd, n, d, segd, seg.data_ptr(), K, s, ws, nbytes)
    torch.cuda.synchronize()
    assert bool((s[n:] == -7.5).all()), "guard entries overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "workspace overrun"
    assert torch.equal(xd.cpu(), xs) and torch.equal(segd.cpu(), seg)
    return s[:n].cpu()


def _tolerance(x, ref):
    d_pad = (x.shape[1] + 3) // 4 * 4
    bar = 8.0 * np.sqrt(d_pad) * EPS24 * float((x.astype(np.float64) ** 2).sum(1).max())
    assert ref.d_min ** 2 >= 64.0 * bar, "the case's closest pair is too close for the bound"
    delta = bar / (2.0 * ref.d_min) + 2.0 ** -23 * ref.d_max
    top = np.maximum(ref.a, ref.b)
    with np.errstate(divide="ignore"):
        return np.where(top > 0, 3.0 * delta / top, 0.0) + 1e-12                          # a = b = 0: the restatement's s is an exact 0


@pytest.mark.parametrize("name", list(R.CASES))
def test_silhouette_samples_against_the_restatement(name):
    """Case E additionally: the rows of u (copies of it fill another cluster too) score EXACTLY 0 and the rows of v exactly 1 - a
    repeated row is at distance exactly 0 and self leaves by index.
    Measured on MI355X, max error / tolerance: A 0.0021, B 0.0125, C 0.0050, D 0.0152, F 0.0102, G 0.0026, H 0.0146, E 0.0105
    (DESIGN.md section 16)."""
    from src.evaluation.graph import silhouette_samples, silhouette_score
    x, labels, ref = R.case(name)
    tol = _tolerance(x, ref)
    got = silhouette_samples(torch.from_numpy(x).cuda(), labels)
    assert got.dtype == torch.float64 and got.is_cuda and got.shape == (len(x),)
    s = got.cpu().numpy()
    err = np.abs(s - ref.s)
    print(f"silhouette case {name} n {x.shape[0]} d {x.shape[1]} K {len(set(labels.tolist()))}: max error / tolerance = {float((err / tol).max()):.4f}"
          f" (max error {float(err.max()):.3g})")
    assert np.isfinite(s).all() and (err <= tol).all()
    if name == "E":
        assert (s[(labels == 0) | (labels == 2)] == 0.0).all() and (s[labels == 1] == 1.0).all()
    size = np.unique(labels, return_counts=True)[1][np.unique(labels, return_inverse=True)[1]]
    assert (s[size == 1] == 0.0).all()                                                    # a one-member cluster scores 0
    assert abs(silhouette_score(torch.from_numpy(x).cuda(), labels) - float(s.mean())) <= 1e-15


def test_two_launches_agree_bit_for_bit_and_need_no_cleared_workspace():
    from src.evaluation.graph import silhouette_samples
    x, labels, ref = R.case("F")
    order = np.argsort(labels, kind="stable")
    counts = np.unique(labels, return_counts=True)[1]
    seg = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    xs = torch.from_numpy(np.ascontiguousarray(x[order]))
    s1, s2 = _launch(xs, seg), _launch(xs, seg)
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    assert float(np.abs(s1.numpy() - ref.s[order]).max()) <= float(_tolerance(x, ref).max())
    back = silhouette_samples(torch.from_numpy(x).cuda(), labels).cpu()                  # the Python layer sorts the same way
    assert torch.equal(back[torch.from_numpy(order)].view(torch.int64), s1.view(torch.int64))


def test_the_callers_order_and_label_types():
    """Permuting rows and labels permutes the result bit for bit: a pair's distance does not depend on where the two rows sit (g_ij
    is one fmaf chain over d whichever row is the owned one), and the fp64 sums of these fp32 distances are exact (333 terms within a
    factor 2^5 of each other need 24 + 5 + 9 bits), so their order does not matter either."""
    from src.evaluation.graph import silhouette_samples
    x, labels, _ = R.case("A")
    xd = torch.from_numpy(x).cuda()
    s = silhouette_samples(xd, labels)
    p = torch.from_numpy(np.random.RandomState(11).permutation(len(x)))
    sp = silhouette_samples(xd[p.cuda()], labels[p.numpy()])
    assert torch.equal(sp.view(torch.int64), s[p.cuda()].view(torch.int64))
    for other in (labels.tolist(), torch.from_numpy(labels), torch.from_numpy(labels).cuda().int(), labels.astype(np.int16)):
        assert torch.equal(silhouette_samples(xd, other).view(torch.int64), s.view(torch.int64))
    # label values are arbitrary: renaming the clusters changes nothing
    assert torch.equal(silhouette_samples(xd, -7 * labels + 3).view(torch.int64), s.view(torch.int64))


def test_bad_arguments_are_refused_before_any_launch():
    from src import _native as N
    from src.evaluation.graph import silhouette_samples, silhouette_workspace_bytes
    for what, got, want in R.bad_argument_codes(N.lib(), silhouette_workspace_bytes(100)):
        assert got == want, what
    assert torch.cuda.is_available()
    torch.cuda.synchronize()                                            # nothing was launched: nothing can have faulted
    x = torch.zeros(10, 6, device="cuda")
    for labels in ([0] * 10, list(range(10)), [0, 1] * 4, [0.5, 1.0] * 5):          # K = 1, K = n, 8 labels for 10 rows, not integers
        with pytest.raises(ValueError):
            silhouette_samples(x, labels)
    with pytest.raises(ValueError):
        silhouette_samples(torch.zeros(10, device="cuda"), [0, 1] * 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        silhouette_samples(x.cpu(), [0, 1] * 5)


# ---- the labeler -------------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def clips(tmp_path_factory, cfg_s):
    """The 12-clip checkpoint fixture of tests/test_gpu_graph.py::test_store_clusters_pic_command, embedded once."""
    import pandas as pd
    from src.evaluation.embed import extract_embeddings, load_embedder
    tmp = tmp_path_factory.mktemp("silhouette_labeler")
    ckpt = _checkpoint(tmp, cfg_s)
    files = _write_wavs(tmp, [16000 + 500 * (i % 3) for i in range(12)], salt=300)
    files_csv = str(tmp / "files.csv")
    pd.DataFrame({"files": files}).to_csv(files_csv, index=False)
    feats = extract_embeddings(load_embedder(ckpt, "delores_s", config=None, layer="backbone"), files, batch_size=64, window="center",
                               duration=1.0)
    base = ["--checkpoint", ckpt, "--upstream", "delores_s", "--input", files_csv, "--pca", "8", "--window", "center"]
    return tmp, files, feats, base


def _score_line(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("silhouette ")]
    assert len(lines) == 1, text
    return lines[0]


def test_labeler_score(clips, capsys):
    from src.evaluation.graph import silhouette_score
    from src.upstream.decar_v2 import store_clusters as sc
    from src.upstream.decar_v2.clustering import Kmeans, rearrange_clusters
    tmp, files, feats, base = clips
    np.random.seed(2)
    sc.main(sc.get_args(base + ["--k", "3", "--out", str(tmp / "plain.csv")]))
    plain = capsys.readouterr().out
    assert len(plain.splitlines()) == 1                                  # without --score the command prints what it printed
    np.random.seed(2)
    labels = sc.main(sc.get_args(base + ["--k", "3", "--score", "--out", str(tmp / "scored.csv")]))
    scored = capsys.readouterr().out
    assert open(tmp / "scored.csv", "rb").read() == open(tmp / "plain.csv", "rb").read()
    assert scored.splitlines()[0].replace("scored.csv", "plain.csv") == plain.splitlines()[0]           # the summary line is what it was
    np.random.seed(2)
    km = Kmeans(3)
    km.cluster(feats, verbose=False, pca=8)
    assert km.features.shape == (12, 8) and km.features.is_cuda
    want_labels = rearrange_clusters(km.images_lists)
    np.testing.assert_array_equal(labels, want_labels)
    sizes = np.unique(want_labels, return_counts=True)[1]
    want = silhouette_score(km.features, want_labels)
    assert _score_line(scored) == f"silhouette {want:.6f} ({len(sizes)} clusters, {int((sizes == 1).sum())} singletons)"
    assert -1.0 <= want <= 1.0
    # pic: the score of whatever it found
    labels = sc.main(sc.get_args(base + ["--clustering", "pic", "--nnn", "3", "--score", "--out", str(tmp / "pic.csv")]))
    text = capsys.readouterr().out
    count = int(max(labels)) + 1
    line = _score_line(text)
    assert text.splitlines()[0].startswith(f"12 files, {count} clusters, pic") and line.endswith(" singletons)")
    assert f"({count} clusters, " in line
    if 2 <= count <= 11:
        assert -1.0 <= float(line.split()[1]) <= 1.0
    else:
        assert line.split()[1] == "n/a"


def test_labeler_k_sweep(clips, capsys):
    from src.evaluation.graph import silhouette_score
    from src.upstream.decar_v2 import store_clusters as sc
    from src.upstream.decar_v2.clustering import preprocess_features, run_kmeans
    tmp, files, feats, base = clips
    out_csv = str(tmp / "sweep.csv")
    np.random.seed(5)
    labels = sc.main(sc.get_args(base + ["--k_sweep", "2,3,4", "--out", out_csv]))
    lines = capsys.readouterr().out.splitlines()
    table = [ln for ln in lines if ln.startswith("k ")]
    assert len(table) == 3 and [ln.split(":")[0] for ln in table] == ["k 2", "k 3", "k 4"]
    # restated: one preprocessing, run_kmeans per k on the same seed draws
    np.random.seed(5)
    xb = preprocess_features(feats, pca=8)
    runs = []
    for k, ln in zip((2, 3, 4), table):
        I, loss = run_kmeans(xb, k)
        used = len(set(I))
        score = silhouette_score(xb, I) if 2 <= used <= 11 else None
        runs.append((k, I, score))
        shown = "n/a" if score is None else f"{score:.6f}"
        assert ln == f"k {k}: {used} non-empty clusters, k-means loss {loss:.6g}, silhouette {shown}"
    best = max((r for r in runs if r[2] is not None), key=lambda r: (r[2], -r[0]))
    assert lines[-1].startswith(f"chosen k {best[0]} of 2,3,4 ")
    assert f"12 files, {best[0]} clusters, k-means loss " in "\n".join(lines)
    got = [int(ln.rsplit(",", 1)[1]) for ln in open(out_csv).read().split()[1:]]
    assert got == best[1] == [int(l) for l in labels]
    np.random.seed(5)
    with pytest.raises(ValueError, match="exceeds the 12 files"):
        sc.main(sc.get_args(base + ["--k_sweep", "3,13", "--out", out_csv]))
