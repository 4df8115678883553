"""CPU: whole-clip embeddings - the rule that makes a padded batch exact (`tests/ragged_ref.py`) against each clip alone in the
oracle, the host plan of the ragged batches, argument validation of the new entry points before any launch, the commands' parsers
and the refusal of the transformer encoder."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import ragged_ref as RR
from helpers import rel_l2
from oracle import fill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (16000, 21917, 41600, 16037, 1280)
NEW = ("audiossl_logmel_ragged_fwd", "audiossl_tail_mask", "audiossl_tmean3_ragged_fwd", "audiossl_meanmax_ragged_fwd")


def _waves(lens, salt):
    return [torch.from_numpy(fill.uniform((n,), salt + i, -0.3, 0.3)
                             + 0.2 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(n) / 16000).astype(np.float32)) for i, n in enumerate(lens)]


def _oracle():
    from oracle import model as OM
    ref = OM.AudioNTT2020Task6(64, 2048, True)
    fill.fill_state_dict_(ref, seed=21)
    with torch.no_grad():
        for n, b in ref.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(torch.from_numpy(fill.uniform(tuple(b.shape), 500 + fill.salt_of(n) % 1000, -0.2, 0.2)))
            elif n.endswith("running_var"):
                b.copy_(torch.from_numpy(fill.uniform(tuple(b.shape), 501 + fill.salt_of(n) % 1000, 0.5, 1.5)))
    return ref.eval()


def test_the_rule_equals_each_clip_alone_in_the_oracle():
    """Pins the rule itself (it holds before any kernel exists): one padded batch of five lengths - a multiple of the hop, odd
    frame counts, the shortest clip the path takes - against five single-clip passes."""
    ref = _oracle()
    waves = _waves(LENS, 40)
    x = RR.ragged_logmel(waves)
    assert x.shape == (5, 1, 64, 264)
    got = RR.ragged_forward(ref, x, LENS)
    want = RR.alone_batch(ref, waves)
    for l in RR.LAYERS:
        for b in range(len(LENS)):
            e = rel_l2(got[l][b], want[l][b])
            assert e <= 1e-5, (l, b, e)


def _check_plan(plan, lengths, batch_size, max_frames):
    seen = sorted(i for idx, _ in plan for i in idx)
    assert seen == list(range(len(lengths)))                                   # every index exactly once
    for idx, tmax in plan:
        assert 1 <= len(idx) <= batch_size
        assert tmax % 8 == 0 and tmax >= max(1 + lengths[i] // 160 for i in idx)
        assert tmax - 8 < max(1 + lengths[i] // 160 for i in idx)              # and no more than the rounding asks for
        assert len(idx) * tmax <= max_frames or len(idx) == 1


@pytest.mark.parametrize("batch_size,max_frames", [(64, 65536), (3, 65536), (64, 700), (1, 65536), (64, 8)])
def test_plan_properties(batch_size, max_frames):
    from src.evaluation.embed import plan_ragged_batches
    lengths = [int(16000 * 30.0 ** u) for u in fill.uniform01((200,), 77)] + [16000] * 5 + [1120, 480000]
    plan = plan_ragged_batches(lengths, batch_size, max_frames)
    _check_plan(plan, lengths, batch_size, max_frames)
    assert plan == plan_ragged_batches(lengths, batch_size, max_frames)        # a pure function
    assert plan_ragged_batches([], 4, 100) == []
    with pytest.raises(ValueError):
        plan_ragged_batches([16000], 0, 100)


def test_plan_padding_stays_below_a_tenth():
    from src.evaluation.embed import MAX_FRAMES, plan_ragged_batches
    assert MAX_FRAMES == 65536 and MAX_FRAMES < 1048000
    lengths = [int(16000 * 30.0 ** u) for u in fill.uniform01((1000,), 1234)]
    assert min(lengths) >= 16000 and max(lengths) <= 480000
    plan = plan_ragged_batches(lengths, 64, 65536)
    _check_plan(plan, lengths, 64, 65536)
    total = sum(len(idx) * tmax for idx, tmax in plan)
    real = sum(1 + n // 160 for n in lengths)
    share = 1.0 - real / total
    print(f"ragged plan: {len(plan)} batches, padded share of frames {share:.4f}")
    assert share <= 0.10, share


def test_new_entry_points_are_declared_and_exported():
    from src import _native as N
    protos = N.parse_header()
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in NEW:
        assert name in protos, name
        assert hasattr(lib, name), name
    assert [a for a, _ in protos["audiossl_logmel_ragged_fwd"]][:4] == ["wave", "lens", "lens_host", "out"]


def test_ragged_arguments_are_refused_before_any_launch():
    from src import _native as N
    lib = N.lib()
    P = 256                                        # a non-null, 16-byte aligned address that is never dereferenced: every call returns first
    Lmax, hop = 41600, 160

    def logmel(lens, lens_dev=P, host=True, tmax=264, lmax=Lmax, wave=P):
        h = np.asarray(lens, np.int32)
        return lib.audiossl_logmel_ragged_fwd(wave, lens_dev, h.ctypes.data if host else None, P, len(h), lmax, tmax, 1024, hop, 64, 45,
                                              P, P, P, P, 0.0, 0.0, 1, None)
    ok = [16000, 21917, 41600, 16037, 1280]
    assert logmel(ok, lens_dev=None) == -1                                     # null lens
    assert logmel(ok, host=False) == -1                                        # null lens_host
    assert logmel(ok, wave=None) == -1
    assert logmel([16000, 1119]) == -1                                         # below 8 frames
    assert logmel([16000, Lmax + 1]) == -1                                     # longer than its row
    assert logmel(ok, tmax=1 + Lmax // hop - 1) == -1                          # one frame short
    assert logmel([16000, 1120], lmax=16000, tmax=100) == -1
    assert logmel(ok, wave=P + 4) == -3                                        # float2 reads of the interior frames
    # the mask: 16-byte stores
    assert lib.audiossl_tail_mask(1, None, P, hop, 1, 5, 132, 2048, None) == -1
    assert lib.audiossl_tail_mask(1, P, None, hop, 1, 5, 132, 2048, None) == -1
    assert lib.audiossl_tail_mask(2, P, P, hop, 1, 5, 132, 2048, None) == -1
    assert lib.audiossl_tail_mask(1, P + 8, P, hop, 1, 5, 132, 2048, None) == -3    # misaligned map
    assert lib.audiossl_tail_mask(1, P, P, hop, 1, 5, 132, 2044, None) == -3        # a row that is no multiple of 16 bytes
    assert lib.audiossl_tail_mask(0, P, P, hop, 1, 5, 132, 2046, None) == -3
    # the pools
    assert lib.audiossl_tmean3_ragged_fwd(1, P, P, 132, 32, P, P, 66, 16, P, P, 33, 8, None, hop, 5, None) == -1
    assert lib.audiossl_tmean3_ragged_fwd(1, P, P, 132, 32, P, P + 4, 66, 16, P, P, 33, 8, P, hop, 5, None) == -3
    assert lib.audiossl_meanmax_ragged_fwd(1, P, None, None, P, hop, 3, 5, 33, 2048, None) == -1   # no output at all
    assert lib.audiossl_meanmax_ragged_fwd(1, P, P, P, P, hop, 3, 5, 33, 2044, None) == -1         # D % 8
    assert lib.audiossl_meanmax_ragged_fwd(1, P, P, P, None, hop, 3, 5, 33, 2048, None) == -1


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_commands_take_the_whole_window_and_keep_their_defaults():
    from src.evaluation.embed import WINDOWS
    assert WINDOWS == ("center", "random", "whole")
    ev = _load(os.path.join(ROOT, "audio-ssl_amd", "evaluate_knn.py"), "evaluate_knn_whole")
    cl = _load(os.path.join(ROOT, "audio-ssl_amd", "compare_layers.py"), "compare_layers_whole")
    from src.upstream.decar_v2 import store_clusters as sc
    base_ev = ["--checkpoint", "c", "--train_csv", "a", "--test_csv", "b"]
    base_sc = ["--checkpoint", "c", "--input", "f.csv", "--k", "585", "--out", "o.csv"]
    base_cl = ["--checkpoint", "c", "--input", "f.csv"]
    for mod, base, default in ((ev, base_ev, "center"), (sc, base_sc, "random"), (cl, base_cl, "center")):
        a = mod.get_args(base)
        assert (a.window, a.max_duration) == (default, 30.0)
        a = mod.get_args(base + ["--window", "whole", "--max_duration", "12.5"])
        assert (a.window, a.max_duration) == ("whole", 12.5)
    with pytest.raises(SystemExit):
        cl.get_args(base_cl + ["--window", "random"])                          # CKA compares the same cut of every clip


def test_whole_window_argument_checks_need_no_gpu():
    from src.encoder import ASTModel
    from src.evaluation import Embedder, extract_embeddings
    m = ASTModel(label_dim=16, fstride=10, tstride=10, input_fdim=128, input_tdim=101, depth=1)
    emb = Embedder(m, layer="backbone")
    with pytest.raises(ValueError, match="input size"):
        emb.embed_ragged(torch.zeros(2, 16000), torch.tensor([16000, 16000], dtype=torch.int32))
    with pytest.raises(ValueError, match="input size"):
        extract_embeddings(emb, [], window="whole")
    with pytest.raises(ValueError):
        extract_embeddings(emb, [], window="middle")
