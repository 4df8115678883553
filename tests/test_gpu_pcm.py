"""GPU: `audiossl_pcm_window` and the front ends fed a `PcmBatch`, against the existing float32 host path (`ingest.decode`, then
`extract_window` or right padding) on WAV files written into a temporary directory.  Every comparison is bit for bit."""
import copy
import random

import numpy as np
import pytest
import torch

import pcm_cases as P

pytestmark = pytest.mark.gpu

SENTINEL = -77.25


def _run(batch, extra_rows=2):
    """The kernel into the first B rows of a larger allocation -> (rows 0..B-1, the rows past B) on the host."""
    from src.dataset import ingest
    B, unit = batch.shape
    out = torch.full((B + extra_rows, unit), SENTINEL, dtype=torch.float32, device="cuda")
    assert ingest.pcm_window(batch, out=out) is out
    out = out.cpu()
    return out[:B], out[B:]


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("unit", [1000, 1603])
def test_kernel_is_the_host_path_bit_for_bit(tmp_path, unit, align):
    """All four formats, C in {1, 2, 3}, n in {0, 1, 7, unit - 1, unit} and a cut clip in one batch; 1603 is odd (scalar stores, the
    left padding changes parity), 1000 takes the 16-byte stores."""
    batch, want = P.make_batch(tmp_path, P.MIXED, unit, align)
    got, rest = _run(batch)
    for b in range(len(P.MIXED)):
        assert torch.equal(got[b], want[b]), (b, P.MIXED[b][:2])
    assert bool((rest == SENTINEL).all())


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("unit", [1000, 1004, 2056])
def test_mono_s16_stream_path(tmp_path, unit, align):
    """A batch of mono 16-bit clips only (8 samples per lane, aligned 16-byte loads): every even shift of the source against the
    store grid through odd frame counts and the centre padding, windows of 0 and 4 mod 8 samples, more than one block per row."""
    ns = [unit, 1, 7, unit - 1, 0, 3, unit - 2, 9, unit - 3, 5, 11, unit - 5, 13, unit + 21, 15, unit - 7] + [1] * 8     # the one-frame clips walk the offset through every even residue
    cases = [("s16", 1, (lambda u, n=n: n), 9 if n > unit else 0) for n in ns]
    batch, want = P.make_batch(tmp_path, cases, unit, align)
    shifts = {(int(o) - 2 * ((unit - int(n)) // 2 if align == 0 else 0)) % 16 for o, n in batch.table[:, :2].tolist()}
    assert shifts == set(range(0, 16, 2))
    got, rest = _run(batch)
    for b in range(len(ns)):
        assert torch.equal(got[b], want[b]), (b, ns[b])
    assert bool((rest == SENTINEL).all())


@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "f32"])
def test_six_and_eight_channels(tmp_path, fmt):
    """numpy's `mean(axis=1)` adds first to last up to 7 channels and pairwise at 8; the divisor 6 is no reciprocal multiply."""
    cases = [(fmt, 6, lambda u: 333, 0), (fmt, 8, lambda u: u, 0), (fmt, 8, lambda u: u + 3, 2), (fmt, 5, lambda u: 100, 0)]
    batch, want = P.make_batch(tmp_path, cases, 500, 0)
    got, _ = _run(batch)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ front ends
def _files(tmp_path, lengths):
    return [P.write_clip(tmp_path / f"f{i}.wav", "s16", n, 1 + (i == 2), 40 + i) for i, n in enumerate(lengths)]


def _both(files, unit, align, starts):
    """-> (float32 [B, unit] host batch of the existing path, PcmBatch of the same windows)."""
    from src.dataset import ingest
    want = torch.stack([P.host_row(f, unit, align, s) for f, s in zip(files, starts)])
    return want, ingest.PcmBatch.pack([ingest.decode_raw(f) for f in files], starts, unit, align)


@pytest.mark.parametrize("norm", ["l2", "mean_var"])
def test_upstream_log_mel_of_a_pcm_batch(tmp_path, cfg_s, norm):
    from src.augmentations import AugmentationModule
    from src.dataset import UpstreamFrontEnd
    cfg = copy.deepcopy(cfg_s)
    cfg["pretrain"]["normalization"] = norm
    front = UpstreamFrontEnd(cfg, AugmentationModule(cfg, 100, max_batch=4))
    waves, batch = _both(_files(tmp_path, [16000, 12001, 20000, 15999]), 16000, 0, [0, 0, 1234, 0])
    want = front.log_mel(waves.cuda())
    assert torch.equal(front.log_mel(batch), want)                    # still on the host: uploaded by the front end
    assert torch.equal(front.log_mel(batch.cuda()), want)
    assert want.shape == (4, 64, 101) and bool(torch.isfinite(want).all())


def test_downstream_front_end_of_a_pcm_batch(tmp_path):
    from src.dataset.downstream_dataset import DownstreamFrontEnd
    front = DownstreamFrontEnd()
    waves, batch = _both(_files(tmp_path, [16000, 12001, 20000, 15999]), 16000, 0, [0, 0, 77, 0])
    want = front(waves)
    assert want.shape == (4, 1, 64, 101) and torch.equal(front(batch), want)


@pytest.mark.parametrize("skip_norm", [True, False])
def test_mast_front_end_of_a_pcm_batch(tmp_path, skip_norm):
    from src.dataset import ingest
    from src.dataset.mast_dataset import MastFrontEnd
    files = _files(tmp_path, [4800, 19200, 11111, 8000])                  # 0.3 .. 1.2 s, ragged
    conf = dict(num_mel_bins=128, target_length=128, freqm=0, timem=0, mixup=0.0, mean=-4.27, std=4.57, skip_norm=skip_norm)
    front = MastFrontEnd(conf)
    want = front([torch.from_numpy(ingest.decode(f)[0]) for f in files])
    batch = ingest.PcmBatch.pack([ingest.decode_raw(f) for f in files], [0] * 4, 19200, align=1)
    got = front(batch)
    assert got.shape == (4, 1, 128, 128) and torch.equal(got, want)
    with pytest.raises(ValueError, match="align=1"):
        front(ingest.PcmBatch.pack([ingest.decode_raw(f) for f in files], [0] * 4, 19200, align=0))


def test_submit_collect_with_a_host_pcm_batch(tmp_path, cfg_s):
    """The pre-training path end to end: both collates from the same seeds, the front end one batch ahead on its own stream."""
    from src.augmentations import AugmentationModule
    from src.dataset import UpstreamFrontEnd, ingest
    from src.dataset.upstream_dataset import WindowCollate
    files = _files(tmp_path, [16000, 12001, 20000, 15999])
    views = []
    for pcm in (False, True):
        np.random.seed(11); random.seed(11)
        tf = AugmentationModule(cfg_s, 100, max_batch=4)
        front = UpstreamFrontEnd(cfg_s, tf)
        items = [ingest.decode_raw(f) if pcm else torch.from_numpy(ingest.decode(f)[0]) for f in files]
        waves, plan = WindowCollate(tf, 16000, 64, pcm=pcm)(items)
        assert isinstance(waves, ingest.PcmBatch) == pcm and not waves.is_cuda
        v1, v2 = front.collect(front.submit(waves.pin_memory(), plan))
        torch.cuda.synchronize()
        views.append((v1.cpu(), v2.cpu()))
    assert views[0][0].shape == (4, 1, 64, 101)
    assert torch.equal(views[0][0], views[1][0]) and torch.equal(views[0][1], views[1][1])
