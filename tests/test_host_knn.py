"""CPU: the k-NN entry points' C ABI (declared, exported, arguments refused before any launch, workspace size), the tests' own
references on a hand-written case, the window helper of the embedding pass, and the commands' argument parsers."""
import ctypes
import importlib.util
import os
import random
import subprocess

import pytest
import torch

import knn_ref as R
from src import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -3
ENTRIES = ("audiossl_knn_workspace", "audiossl_knn_topk", "audiossl_knn_vote")


def test_the_three_symbols_are_declared_and_exported():
    protos = N.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ENTRIES:
        assert name in protos, f"{name} is not declared in include/audiossl_hip.h"
        assert name in exported, f"{name} is not exported"
    assert [a for a, _ in protos["audiossl_knn_topk"]] == ["q", "bank", "Nq", "Nb", "D", "k", "top_sim", "top_idx", "workspace",
                                                          "workspace_bytes", "stream"]
    assert protos["audiossl_knn_workspace"][-1][0] == "bytes"          # a host entry point: no stream


def _ws(nq, nb, k):
    b = ctypes.c_long(-7)
    rc = N.lib().audiossl_knn_workspace(nq, nb, k, ctypes.addressof(b))
    return rc, b.value


def _topk(q=4096, bank=8192, nq=64, nb=4096, d=64, k=20, sim=256, idx=256, ws=16384, ws_bytes=None):
    """Fake (never dereferenced) device addresses: every case below must be refused before a launch."""
    if ws_bytes is None:
        rc, ws_bytes = _ws(nq, nb, k)
        ws_bytes = ws_bytes if rc == 0 else 1 << 40
    return N.lib().audiossl_knn_topk(q, bank, nq, nb, d, k, sim, idx, ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=129), dict(k=20, nb=19), dict(d=48), dict(d=4128), dict(nb=1 << 31),
                                dict(q=None), dict(d=0), dict(nq=0), dict(bank=None), dict(sim=None), dict(idx=None),
                                dict(ws=None)],
                         ids=lambda kw: "-".join(f"{a}={b}" for a, b in kw.items()))
def test_bad_arguments_are_einval_before_any_launch(kw):
    assert _topk(**kw) == EINVAL


def test_short_workspace_is_einval_and_misaligned_bank_is_ealign():
    rc, need = _ws(64, 70001, 20)
    assert rc == 0 and need > 0
    assert _topk(nb=70001, ws_bytes=need - 1) == EINVAL
    assert _topk(bank=8192 + 2) == EALIGN
    assert _topk(q=4096 + 8) == EALIGN


def test_workspace_query_rejects_what_topk_rejects():
    for nq, nb, k in ((64, 4096, 0), (64, 4096, 129), (64, 10, 11), (64, 1 << 31, 20), (0, 4096, 20)):
        assert _ws(nq, nb, k)[0] == EINVAL
    assert N.lib().audiossl_knn_workspace(64, 4096, 20, None) == EINVAL


def test_vote_rejects_bad_arguments():
    lib = N.lib()
    assert lib.audiossl_knn_vote(None, 256, 256, 4, 20, 100, 1.0, 256, 256, None) == EINVAL
    assert lib.audiossl_knn_vote(256, 256, 256, 4, 0, 100, 1.0, 256, 256, None) == EINVAL
    assert lib.audiossl_knn_vote(256, 256, 256, 4, 129, 100, 1.0, 256, 256, None) == EINVAL
    assert lib.audiossl_knn_vote(256, 256, 256, 0, 20, 100, 1.0, 256, 256, None) == EINVAL
    assert lib.audiossl_knn_vote(256, 256, 256, 4, 20, 100, -1.0, 256, 256, None) == EINVAL


def test_workspace_is_monotone_and_far_below_the_matrix():
    nb = 65536
    for k in (1, 20, 64, 65, 128):
        sizes = [_ws(nq, nb, k) for nq in (1, 2, 63, 64, 65, 127, 128, 129, 448, 449, 512, 1000, 4096, 4097, 50000)]
        assert all(rc == 0 for rc, _ in sizes)
        vals = [v for _, v in sizes]
        assert vals == sorted(vals), (k, vals)
    for nq in (1, 64, 130, 4096):
        vals = [_ws(nq, nb, k)[1] for k in range(1, 129)]
        assert vals == sorted(vals), (nq, vals)
    rc, big = _ws(4096, 65536, 128)
    assert rc == 0 and 0 < big < 4096 * 65536
    # a small bank does not pay for splits it cannot have
    assert _ws(1, 128, 128)[1] <= 64 * 128 * 8


# ---- the tests' own references, on a case written out by hand ------------------------------------------------------
Q3 = torch.tensor([[1, 0], [0, 1], [1, 1]])
B5 = torch.tensor([[2, 0], [0, 2], [2, 0], [1, 1], [-1, -1]])
# dots:      row0  row1  row2  row3  row4
#   q0 (1,0):  2     0     2     1    -1
#   q1 (0,1):  0     2     0     1    -1
#   q2 (1,1):  2     2     2     2    -2


def test_reference_topk_on_a_hand_written_case_resolves_ties_to_the_smaller_row():
    d, i = R.topk_exact_int(Q3, B5, 3)
    assert d.tolist() == [[2, 2, 1], [2, 1, 0], [2, 2, 2]]
    assert i.tolist() == [[0, 2, 3], [1, 3, 0], [0, 1, 2]]
    d, i = R.topk_exact_int(Q3, B5, 5)
    assert i.tolist() == [[0, 2, 3, 1, 4], [1, 3, 0, 2, 4], [0, 1, 2, 3, 4]]
    assert torch.equal(R.sims_f64(Q3, B5), (Q3 @ B5.T).double())


def test_reference_vote_on_the_same_case_resolves_ties_to_the_smaller_label():
    d, i = R.topk_exact_int(Q3, B5, 3)
    labels = torch.tensor([7, 3, 3, 7, 5])                   # rows 0..4
    # majority: q0 -> rows 0, 2, 3 = labels 7, 3, 7 -> 7 (2 of 3);  q1 -> rows 1, 3, 0 = 3, 7, 7 -> 7;  q2 -> rows 0, 1, 2 = 7, 3, 3 -> 3
    pred, conf, _ = R.vote(d, i, labels, 0.0)
    assert pred.tolist() == [7, 7, 3]
    assert conf.tolist() == pytest.approx([2 / 3, 2 / 3, 2 / 3])
    # a two-way tie: k = 2 for q0 -> rows 0, 2 = labels 7, 3, one vote each -> the smaller label
    pred, conf, _ = R.vote(d[:, :2], i[:, :2], labels, 0.0)
    assert pred[0].item() == 3 and conf[0].item() == pytest.approx(0.5)
    # weights: q1's neighbours have dots 2, 1, 0 and labels 3, 7, 7: exp(0) against exp(-1) + exp(-2) at inv_t = 1
    pred, conf, _ = R.vote(d, i, labels, 1.0)
    e1, e2 = torch.exp(torch.tensor(-1.0, dtype=torch.float64)).item(), torch.exp(torch.tensor(-2.0, dtype=torch.float64)).item()
    assert pred[1].item() == 3 and conf[1].item() == pytest.approx(1.0 / (1.0 + e1 + e2))
    # an index outside the bank
    bad = i.clone()
    bad[2, 1] = 5
    pred, conf, _ = R.vote(d, bad, labels, 0.0)
    assert pred[2].item() == -1 and torch.isnan(conf[2]) and pred[0].item() == 7


# ---- windows -----------------------------------------------------------------------------------------------------------
def test_center_window_equals_the_slices_written_out_and_draws_nothing():
    from src.evaluation.embed import take_window
    unit = 16000
    state = random.getstate()
    w = torch.arange(100, dtype=torch.float32) + 1
    got = take_window(w, unit, "center")
    want = torch.zeros(unit)
    want[7950:8050] = w                                      # (16000 - 100) // 2 zeros in front
    assert torch.equal(got, want)
    w = torch.arange(16000, dtype=torch.float32)
    assert torch.equal(take_window(w, unit, "center"), w)
    w = torch.arange(20000, dtype=torch.float32)
    assert torch.equal(take_window(w, unit, "center"), w[2000:18000])
    assert random.getstate() == state
    with pytest.raises(ValueError):
        take_window(w, unit, "middle")


def test_random_window_is_extract_window_under_the_same_seed():
    from src.evaluation.embed import take_window
    from src.utils import extract_window
    clips = [torch.arange(n, dtype=torch.float32) for n in (100, 16000, 20000, 48000)]
    random.seed(5)
    want = [extract_window(c, duration=16000) for c in clips]
    random.seed(5)
    got = [take_window(c, 16000, "random") for c in clips]
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- commands ----------------------------------------------------------------------------------------------------------
def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_command_help_parses(capsys):
    ev = _load(os.path.join(ROOT, "audio-ssl_amd", "evaluate_knn.py"), "evaluate_knn_hip")
    from src.upstream.decar_v2 import store_clusters as sc
    tu = _load(os.path.join(ROOT, "audio-ssl_amd", "train_upstream.py"), "train_upstream_hip_help")
    td = _load(os.path.join(ROOT, "audio-ssl_amd", "train_downstream.py"), "train_downstream_hip_help")
    for mod in (ev, sc, tu, td):
        with pytest.raises(SystemExit) as e:
            mod.get_args(["--help"])
        assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--checkpoint", "--upstream", "--train_csv", "--test_csv", "--temperature", "--layer", "--window", "--dump_embeddings",
                 "--input", "--out", "--pca"):
        assert flag in text, flag
    a = ev.get_args(["--checkpoint", "c", "--train_csv", "a", "--test_csv", "b"])
    assert (a.k, a.temperature, a.layer, a.window, a.upstream) == (20, 0.07, "backbone", "center", "delores_m")
    a = sc.get_args(["--checkpoint", "c", "--input", "f.csv", "--k", "585", "--out", "o.csv"])
    assert (a.k, a.pca, a.window) == (585, 128, "random")
