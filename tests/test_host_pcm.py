"""CPU: the host half of the packed PCM upload (`src/dataset/ingest.py`: decode_raw, PcmClip, PcmBatch) against the existing float32
host path on real WAV files, the collate's use of the random streams, and `audiossl_pcm_window`'s argument validation (no launch)."""
import random

import numpy as np
import pytest
import torch

import pcm_cases as P

EINVAL, EALIGN = -1, -3


# ------------------------------------------------------------------------------------------------ decode_raw
@pytest.mark.parametrize("C", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("fmt", ["u8", "s16", "s32", "s24", "f32"])
def test_decode_raw_to_float_is_decode(tmp_path, fmt, C):
    from src.dataset import ingest
    p = P.write_clip(tmp_path / "a.wav", fmt, 1001, C, C)
    clip = ingest.decode_raw(p)
    want, rate = ingest.decode(p)
    assert clip.rate == rate == P.RATE and len(clip) == 1001 and clip.channels == C
    assert clip.data.dtype == {"u8": np.uint8, "s16": np.int16, "s32": np.int32, "s24": np.int32, "f32": np.float32}[fmt]
    got = clip.to_float()
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_hand_written_24_bit_file_reads_left_justified(tmp_path):
    from src.dataset import ingest
    data = P.samples("s24", 9, 2, 3)
    clip = ingest.decode_raw(P.write_wav24(tmp_path / "a.wav", data))
    assert np.array_equal(clip.data, data) and not (clip.data & 0xff).any()


def test_decode_raw_npy(tmp_path):
    from src.dataset import ingest
    w = P.samples("f32", 500, 1, 0)
    np.save(tmp_path / "a.npy", w.astype(np.float64))
    clip = ingest.decode_raw(str(tmp_path / "a.npy"))
    want, rate = ingest.decode(str(tmp_path / "a.npy"))
    assert clip.rate == rate == 16000 and clip.data.dtype == np.float32 and np.array_equal(clip.to_float(), want)


def test_load_audio_raw(tmp_path):
    from src.dataset import ingest
    from src.dataset.upstream_dataset import load_audio
    p = P.write_clip(tmp_path / "a.wav", "s16", 300, 2, 1)
    clip = load_audio(p, 16000, raw=True)
    assert isinstance(clip, ingest.PcmClip) and clip.data.dtype == np.int16
    assert np.array_equal(clip.to_float(), load_audio(p, 16000))


# ------------------------------------------------------------------------------------------------ PcmBatch.pack
def test_pack_layout(tmp_path):
    from src.dataset import ingest
    unit = 1000
    batch, _ = P.make_batch(tmp_path, P.MIXED, unit, 0)
    B = len(P.MIXED)
    assert batch.shape == (B, unit) and batch.size(0) == B and not batch.is_cuda and batch.pin_memory() is batch
    raw = batch._host.numpy()
    tb = ingest.PcmBatch.table_bytes(B)
    assert tb == 512 and tb % 256 == 0 and raw.size % 16 == 0 and batch.nbytes == raw.size
    tab = batch.table.numpy()
    assert np.array_equal(tab, raw[:B * 32].view(np.int64).reshape(B, 4))
    size = {0: 1, 1: 2, 2: 4, 3: 4}
    code = {"u8": 0, "s16": 1, "s32": 2, "f32": 3}
    end = 0
    for b, (fmt, C, nf, start) in enumerate(P.MIXED):
        off, n, ch, f = (int(v) for v in tab[b])
        assert (n, ch, f) == (min(nf(unit), unit), C, code[fmt])
        assert off % size[f] == 0 and end <= off < end + size[f]            # natural alignment, no other gap
        # exactly the window's frames, in the file's own format
        data = P.samples(fmt, nf(unit), C, 10 * b + C)
        win = data[start:start + unit] if len(data) > unit else data
        assert np.array_equal(raw[tb + off:tb + off + win.nbytes].view(win.dtype).reshape(win.shape), win)
        end = off + win.nbytes
    assert raw.size == tb + -(-end // 16) * 16 and not raw[tb + end:].any()    # only window frames, then the 16-byte padding
    assert any(int(o) % 16 for o in tab[:, 0])                                  # offsets leave the 16-byte grid
    assert np.array_equal(batch.lens.numpy(), tab[:, 1]) and batch.lens.dtype == torch.int32


def test_mono_s16_batch_is_half_the_float_batch():
    from src.dataset import ingest
    B, unit = 16, 16000
    clips = [ingest.PcmClip(P.samples("s16", n, 1, n), 16000) for n in [unit + 100 * i for i in range(B)]]
    batch = ingest.PcmBatch.pack(clips, [i for i in range(B)], unit)
    assert batch.nbytes <= (4 * B * unit) // 2 + ingest.PcmBatch.table_bytes(B)
    for b in (0, 7):
        off = int(batch.table[b, 0])
        got = batch._host.numpy()[512 + off:512 + off + 2 * unit].view(np.int16)
        assert np.array_equal(got, clips[b].data[b:b + unit])


def test_pack_takes_float_arrays_and_tensors_for_resampled_clips():
    from src.dataset import ingest
    w = P.samples("f32", 50, 1, 5)
    batch = ingest.PcmBatch.pack([w, torch.from_numpy(w), ingest.PcmClip(P.samples("u8", 3, 1, 1), 16000)], [0, 0, 0], 64, align=1)
    assert batch.table.tolist() == [[0, 50, 1, 3], [200, 50, 1, 3], [400, 3, 1, 0]] and batch.align == 1


# ------------------------------------------------------------------------------------------------ collate
def test_window_collate_pcm_draws_like_the_float_collate(cfg_s, tmp_path):
    from src.augmentations import AugmentationModule
    from src.dataset import ingest
    from src.dataset.upstream_dataset import WindowCollate
    unit = 16000
    files = [P.write_clip(tmp_path / f"w{i}.wav", fmt, n, C, i)
             for i, (fmt, n, C) in enumerate([("s16", 100, 1), ("s16", 16000, 1), ("s16", 20000, 2), ("u8", 48000, 1), ("f32", 16001, 1)])]
    states, outs = [], []
    for pcm in (False, True):
        np.random.seed(4); random.seed(4)
        tf = AugmentationModule(cfg_s, 10, max_batch=8)
        items = [ingest.decode_raw(f) if pcm else torch.from_numpy(ingest.decode(f)[0]) for f in files]
        batch, plan = WindowCollate(tf, unit, 64, pcm=pcm)(items)
        states.append((random.getstate(), np.random.get_state()))
        outs.append((batch, plan, np.array(tf.last_starts), tf.n_entries))
    (s0, n0), (s1, n1) = states
    assert s0 == s1 and n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]
    (w, plan_f, starts_f, e_f), (batch, plan_p, starts_p, e_p) = outs
    assert isinstance(batch, ingest.PcmBatch) and batch.shape == tuple(w.shape) and batch.align == 0
    assert np.array_equal(starts_f, starts_p) and e_f == e_p and starts_p[2] > 0
    assert len(plan_f) == len(plan_p)
    for a, b in zip(plan_f, plan_p):
        assert (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b))
    # the packed frames are the float batch's samples before conversion
    tab = batch.table.numpy()
    raw = batch._host.numpy()[ingest.PcmBatch.table_bytes(5):]
    assert tab[:, 1].tolist() == [100, 16000, 16000, 16000, 16000]
    got = raw[int(tab[2, 0]):int(tab[2, 0]) + 4 * unit].view(np.int16).reshape(unit, 2)
    assert np.array_equal(ingest._to_float(got), w[2].numpy())


# ------------------------------------------------------------------------------------------------ validation
def _call(tab, pcm=4096, pcm_bytes=1 << 20, dev_tab=8192, host=True, out=1 << 16, B=None, unit=1000, align=0):
    """`audiossl_pcm_window` with fake device addresses and a real host table.  Every call here fails a check, so nothing is
    launched: the cases that must come back EINVAL also carry a misaligned `out`, which the alignment check that runs after the
    table rows would catch."""
    from src import _native as N
    tab = np.ascontiguousarray(tab, dtype=np.int64)
    return N.lib().audiossl_pcm_window(pcm, pcm_bytes, dev_tab, tab.ctypes.data if host else None, out, len(tab) if B is None else B,
                                       unit, align, None)


GOOD = [[0, 1000, 1, 1], [2000, 7, 3, 2], [2084, 0, 1, 0], [2084, 5, 8, 3], [2244, 1, 2, 0]]
BAD_OUT = (1 << 16) + 4


def test_valid_table_passes_the_row_checks():
    # the only thing wrong is the alignment of `out`, which is looked at after every row: EALIGN, not EINVAL
    assert _call(GOOD, out=BAD_OUT) == EALIGN
    assert _call(GOOD, out=BAD_OUT, align=1, unit=1603) == EALIGN
    assert _call([[1 << 20, 0, 1, 1]], out=BAD_OUT) == EALIGN                 # an empty clip at the very end of the buffer
    assert _call([[(1 << 20) - 2000, 1000, 1, 1]], out=BAD_OUT) == EALIGN     # a clip that ends with the buffer


@pytest.mark.parametrize("kw", [dict(pcm=None), dict(dev_tab=None), dict(host=False), dict(out=None),
                                dict(B=0), dict(B=-1), dict(B=65536), dict(unit=0), dict(unit=-4), dict(align=2), dict(align=-1)])
def test_bad_arguments_are_einval(kw):
    kw = dict(dict(out=BAD_OUT), **kw)
    tab = GOOD if kw.get("B", 0) <= len(GOOD) else np.tile(np.array([[0, 0, 1, 1]]), (kw["B"], 1))
    assert _call(tab, **kw) == EINVAL


@pytest.mark.parametrize("row", [[0, 10, 1, 4], [0, 10, 1, -1],                # format outside 0..3
                                 [0, 10, 0, 1], [0, 10, 9, 1],                # channels outside 1..8
                                 [0, -1, 1, 1], [0, 1001, 1, 1],              # frames outside 0..unit
                                 [1, 10, 1, 1], [2, 10, 1, 2], [6, 10, 1, 3], [-2, 10, 1, 1],      # offset against the sample size
                                 [(1 << 20) - 1998, 1000, 1, 1], [(1 << 20) - 4, 1, 2, 2], [1 << 21, 0, 1, 1]])   # past the buffer
def test_bad_rows_are_einval(row):
    for pos in (0, len(GOOD)):                                                 # every row is checked, the last one too
        tab = GOOD[:pos] + [row] + GOOD[pos:]
        assert _call(tab, out=BAD_OUT) == EINVAL


def test_misalignment_is_ealign():
    assert _call(GOOD, pcm=4096 + 8) == EALIGN
    assert _call(GOOD, out=(1 << 16) + 8) == EALIGN
    assert _call(GOOD, pcm_bytes=(1 << 20) + 8) == EALIGN


# ------------------------------------------------------------------------------------------------ datasets
def test_datasets_hand_out_pcm_clips(cfg_s, tmp_path):
    """`BaseDataset(pcm=True)` and `DownstreamDataset(pcm=True)` + `PcmCollate`: same draws as the float items, windows packed in
    the files' formats; with the switch off the items are what they were."""
    import pandas as pd
    from types import SimpleNamespace
    from src.dataset import BaseDataset, DownstreamDataset, ingest
    from src.dataset.downstream_dataset import PcmCollate
    files = [P.write_clip(tmp_path / f"d{i}.wav", "s16", n, C, 70 + i) for i, (n, C) in enumerate([(9000, 1), (16000, 2), (30000, 1)])]
    pd.DataFrame({"files": files}).to_csv(tmp_path / "up.csv", index=False)
    pd.DataFrame({"wav": files, "label": ["b", "a", "b"]}).to_csv(tmp_path / "down.csv", index=False)
    up = BaseDataset(cfg_s, SimpleNamespace(upstream="delores_s"), str(tmp_path / "up.csv"), None, pcm=True)
    up_f = BaseDataset(cfg_s, SimpleNamespace(upstream="delores_s"), str(tmp_path / "up.csv"), None)
    for i in range(3):
        clip = up[i]
        assert isinstance(clip, ingest.PcmClip) and clip.data.dtype == np.int16
        assert torch.equal(torch.from_numpy(clip.to_float()), up_f[i])
    args = SimpleNamespace(task="t", train_csv=str(tmp_path / "down.csv"), valid_csv=None, test_csv=str(tmp_path / "down.csv"))
    cfg = {"run": {"duration": 1}, "downstream": {"input": {"sampling_rate": 16000}}}
    random.seed(9)
    want = [DownstreamDataset(args, cfg, "train")[i] for i in range(3)]
    state = random.getstate()
    random.seed(9)
    ds = DownstreamDataset(args, cfg, "train", pcm=True)
    items = [ds[i] for i in range(3)]
    assert random.getstate() == state
    batch, labels = PcmCollate(16000)(items)
    assert labels.tolist() == [w[1] for w in want] == [1, 0, 1] and batch.shape == (3, 16000) and batch.align == 0
    assert batch.lens.tolist() == [9000, 16000, 16000]
    raw = batch._host.numpy()[ingest.PcmBatch.table_bytes(3):]
    for b, (w, _) in enumerate(want):
        off, n, C, fmt = batch.table[b].tolist()
        got = ingest._to_float(raw[off:off + 2 * n * C].view(np.int16).reshape((n, C) if C > 1 else (n,)))
        left = (16000 - n) // 2
        assert np.array_equal(got, w.numpy()[left:left + n]) and not w.numpy()[:left].any()
