"""CPU: the tagging tests' own numpy reference against what the reference project's `calculate_stats` / `d_prime` recorded
(tests/golden/tagging_stats.npz), the label helpers, and the C ABI of `audiossl_bce_rows` / `audiossl_tagging_stats` (declared,
exported, arguments refused before any launch, workspace size)."""
import ctypes
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import tagging_ref as R
from src import _native as N
from src.evaluation import tagging as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -3
ENTRIES = ("audiossl_bce_rows", "audiossl_tagging_workspace", "audiossl_tagging_stats")


# ---- the reference of the GPU tests against the recorded sklearn / scipy results -----------------------------------------
def test_numpy_reference_equals_the_recorded_calculate_stats(golden):
    """AP and AUC within 1e-12: both sides are fp64 sums of at most N terms in [0, 1] (they differ by at most N 2^-52; observed
    2e-16).  d' within 1e-9 relative: two inverse-normal routines (scipy's ppf there, statistics.NormalDist here)."""
    g = golden("tagging_stats")
    worst = [0.0, 0.0, 0.0]
    for i, (n, c, _, _) in enumerate(R.GOLDEN_CASES):
        s, t = R.golden_matrix(i)
        assert np.array_equal(s, g[f"scores_{i}"]) and np.array_equal(t, g[f"targets_{i}"]), "the generator's matrices moved"
        assert s.shape == (n, c)
        st = R.stats(s, t)
        assert st["classes_scored"] == c
        worst[0] = max(worst[0], float(np.abs(st["AP"] - g[f"AP_{i}"]).max()))
        worst[1] = max(worst[1], float(np.abs(st["auc"] - g[f"auc_{i}"]).max()))
        dp = np.array([T.d_prime(a) for a in st["auc"]])
        worst[2] = max(worst[2], float(np.abs(dp / g[f"dprime_{i}"] - 1.0).max()))
    print(f"tagging_ref vs calculate_stats: AP {worst[0]:.2e}, AUC {worst[1]:.2e} (bar 1e-12), d' rel {worst[2]:.2e} (bar 1e-9)")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= 1e-9


def test_reference_on_a_hand_written_column():
    """scores 3 2 2 1 0, labels + - + + -.  Positives (in sample order) 3, 2, 1:
         3: ge_all 1, ge_pos 1 -> 1/1; negatives below 2, tied 0 -> 4
         2: ge_all 3, ge_pos 2 -> 2/3; negatives below 1 (the 0), tied 1 (the other 2) -> 3
         1: ge_all 4, ge_pos 3 -> 3/4; negatives below 1, tied 0 -> 2
       AP = (1 + 2/3 + 3/4) / 3, auc_num2 = 9, AUC = 9 / (2 * 3 * 2)."""
    npos, num2, ap, auc = R.class_stats(np.array([3, 2, 2, 1, 0], dtype=np.float32), np.array([1, 0, 1, 1, 0]))
    assert (npos, num2) == (3, 9)
    assert ap == pytest.approx((1 + 2 / 3 + 3 / 4) / 3, abs=1e-15) and auc == 0.75
    assert math.isnan(R.class_stats(np.zeros(4, dtype=np.float32), np.zeros(4))[2])
    assert math.isnan(R.class_stats(np.zeros(4, dtype=np.float32), np.ones(4))[3])


def test_d_prime_limits():
    assert T.d_prime(0.5) == 0.0 and T.d_prime(1.0) == math.inf and T.d_prime(0.0) == -math.inf and math.isnan(T.d_prime(float("nan")))
    assert T.d_prime(0.975) == pytest.approx(math.sqrt(2.0) * 1.959963984540054, rel=1e-12)


# ---- labels ------------------------------------------------------------------------------------------------------------------
def test_parse_labels_quoted_cells_and_separators(tmp_path):
    import pandas as pd
    assert T.parse_labels("dog") == ["dog"]
    assert T.parse_labels("dog, bark ,growl") == ["dog", "bark", "growl"]
    assert T.parse_labels('"/m/09x0r,/m/05zppz"') == ["/m/09x0r", "/m/05zppz"]
    assert T.parse_labels("a|b,c|d", sep="|") == ["a", "b,c", "d"]
    with pytest.raises(ValueError):
        T.parse_labels(" , ")
    # a quoted cell with commas, through the CSV reader the command uses
    p = tmp_path / "t.csv"
    p.write_text('wav,label\nx.wav,"dog,bark"\ny.wav,cat\n')
    cells = list(pd.read_csv(p)["label"])
    assert [T.parse_labels(c) for c in cells] == [["dog", "bark"], ["cat"]]


def test_class_index_both_forms_and_unknown_names(tmp_path):
    cells = ["dog,bark", "cat", "bark,Zebra", "10,9"]
    index = T.build_class_index(cells)
    assert index == {"10": 0, "9": 1, "Zebra": 2, "bark": 3, "cat": 4, "dog": 5}          # sorted as strings
    y = T.multi_hot([T.parse_labels(c) for c in cells], index)
    assert y.dtype == torch.float32 and y.tolist() == [[0, 0, 0, 1, 0, 1], [0, 0, 0, 0, 1, 0], [0, 0, 1, 1, 0, 0], [1, 1, 0, 0, 0, 0]]
    with pytest.raises(ValueError, match="emu"):
        T.multi_hot([["dog", "emu"]], index)
    p = tmp_path / "class_labels_indices.csv"
    p.write_text('index,mid,display_name\n0,/m/09x0r,"Speech"\n1,/m/05zppz,"Male speech, man speaking"\n2,/m/02zsn,"Female speech"\n')
    index = T.build_class_index(cells, label_csv=str(p))
    assert index == {"/m/09x0r": 0, "/m/05zppz": 1, "/m/02zsn": 2}
    assert T.multi_hot([T.parse_labels('"/m/02zsn,/m/09x0r"')], index).tolist() == [[1, 0, 1]]
    with pytest.raises(ValueError):
        T.multi_hot([["dog"]], index)
    p.write_text("index,mid,display_name\n0,a,A\n2,b,B\n")
    with pytest.raises(ValueError):
        T.build_class_index(cells, label_csv=str(p))


def test_mix_labels_equals_the_reference_loops():
    names = [["a"], ["b", "c"], ["a", "c"], ["d"], ["b"], ["a", "b", "c", "d"]]
    index = {"a": 0, "b": 1, "c": 2, "d": 3}
    partner = torch.tensor([3, -1, 1, 3, -1, 0], dtype=torch.int32)             # a self-partner and two unmixed clips
    lam = torch.tensor([0.37, 1.0, 0.5123, 0.81, 1.0, 0.4444], dtype=torch.float32)
    y = T.multi_hot(names, index)
    got = T.mix_labels(y, partner, lam)
    want = R.mix_rows(names, partner.tolist(), lam.tolist(), index)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert torch.equal(got[1], y[1]) and torch.equal(got[4], y[4])
    assert got[0].tolist() == [pytest.approx(0.37), 0.0, 0.0, pytest.approx(0.63)]
    assert torch.equal(got[3], y[3])                                             # mixed with itself: lam + (1 - lam)
    none = T.mix_labels(y, torch.full((6,), -1), torch.ones(6))
    assert torch.equal(none, y)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_declared_and_exported():
    protos = N.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ENTRIES:
        assert name in protos, f"{name} is not declared in include/audiossl_hip.h"
        assert name in exported, f"{name} is not exported"
    assert [a for a, _ in protos["audiossl_bce_rows"]] == ["dtype", "logits", "targets", "N", "C", "loss_out", "dlogits", "stream"]
    assert [a for a, _ in protos["audiossl_tagging_stats"]] == ["scores", "targets", "N", "C", "npos", "auc_num2", "ap", "auc",
                                                               "workspace", "workspace_bytes", "stream"]
    assert protos["audiossl_tagging_workspace"][-1][0] == "bytes"       # a host entry point: no stream


def _ws(n, c):
    b = ctypes.c_long(-7)
    rc = N.lib().audiossl_tagging_workspace(n, c, ctypes.addressof(b))
    return rc, b.value


def _stats(scores=4096, targets=8192, n=1000, c=7, npos=256, num2=512, ap=768, auc=1024, ws=16384, ws_bytes=None):
    """Fake (never dereferenced) device addresses: every case below must be refused before a launch."""
    if ws_bytes is None:
        rc, ws_bytes = _ws(n, c)
        ws_bytes = ws_bytes if rc == 0 else 1 << 50
    return N.lib().audiossl_tagging_stats(scores, targets, n, c, npos, num2, ap, auc, ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [dict(scores=None), dict(targets=None), dict(npos=None), dict(num2=None), dict(ap=None), dict(auc=None),
                                dict(ws=None), dict(n=0), dict(n=-3), dict(c=0), dict(c=-1), dict(n=1 << 31), dict(ws_bytes=0)],
                         ids=lambda kw: "-".join(f"{a}={b}" for a, b in kw.items()))
def test_stats_bad_arguments_are_einval_before_any_launch(kw):
    assert _stats(**kw) == EINVAL


def test_stats_short_workspace_is_einval_and_misaligned_pointers_are_ealign():
    rc, need = _ws(1000, 7)
    assert rc == 0 and need > 0
    assert _stats(ws_bytes=need - 1) == EINVAL
    assert _stats(scores=4096 + 4) == EALIGN
    assert _stats(ws=16384 + 8) == EALIGN


def test_workspace_query_rejects_what_stats_rejects_and_is_monotone():
    for n, c in ((0, 7), (1 << 31, 7), (1000, 0), (-1, 7)):
        assert _ws(n, c)[0] == EINVAL
    assert N.lib().audiossl_tagging_workspace(1000, 7, None) == EINVAL
    assert _ws((1 << 31) - 1, 1)[0] == 0
    for c in (1, 7, 527):
        vals = [_ws(n, c) for n in (1, 2, 3, 4, 5, 255, 256, 257, 1000, 20383, 100000)]
        assert all(rc == 0 for rc, _ in vals) and [v for _, v in vals] == sorted(v for _, v in vals)
    vals = [_ws(20383, c)[1] for c in range(1, 600)]
    assert vals == sorted(vals)
    # two class-major fp32 copies, one byte of flags and 16 bytes per 256 samples, a little padding: about 9 bytes per cell
    assert 9 * 20383 * 527 <= _ws(20383, 527)[1] <= 9.2 * 20383 * 527


def test_bce_rejects_bad_arguments():
    lib = N.lib()
    ok = dict(dtype=0, logits=256, targets=512, n=8, c=5, loss=768, dl=1024)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.audiossl_bce_rows(a["dtype"], a["logits"], a["targets"], a["n"], a["c"], a["loss"], a["dl"], None)
    for kw in (dict(logits=None), dict(targets=None), dict(loss=None), dict(n=0), dict(c=0), dict(n=-1), dict(dtype=2), dict(dtype=-1),
               dict(n=1 << 40, c=2)):
        assert call(**kw) == EINVAL, kw


def test_python_layer_refuses_host_tensors_and_bad_shapes():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.tagging_stats(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(ValueError):
        T.bce_with_logits(torch.zeros(4, 2), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.bce_with_logits(torch.zeros(4, 2), torch.zeros(4, 2))


def test_train_tagging_help_parses(capsys):
    spec = importlib.util.spec_from_file_location("train_tagging_hip_help", os.path.join(ROOT, "audio-ssl_amd", "train_tagging.py"))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)
    with pytest.raises(SystemExit) as e:
        tt.get_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--task", "--train_csv", "--valid_csv", "--test_csv", "--checkpoint", "--encoder", "--freeze", "--exp_dir", "--upstream",
                 "--config", "--verbose", "--label_csv", "--label_sep"):
        assert flag in text, flag
    a = tt.get_args(["--train_csv", "a", "--test_csv", "b"])
    assert (a.encoder, a.label_sep, a.label_csv, a.freeze) == ("AudioNTT2020Task6", ",", None, True)
    with pytest.raises(SystemExit):
        tt.get_args(["--train_csv", "a", "--test_csv", "b", "--encoder", "ResNet"])
