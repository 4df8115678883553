"""CPU: the host side of the Kaldi fbank front end (`src/dataset/mast_dataset.py`) - the filterbank table against an fp64 closed
form, the mask / mix planners against literal transcriptions of the reference's draws, and the C entry's argument checks.

torchaudio is not available here, so nothing in this file is a parity pin against it: the references are restatements of its
documented algorithm (`torchaudio.compliance.kaldi.get_mel_banks`, `torchaudio.functional.mask_along_axis`)."""
import random

import numpy as np
import pytest
import torch

from src.dataset import mast_dataset as MD


# ------------------------------------------------------------------------------------------------ tables
def mel_banks_f64(num_bins, padded=512, sr=16000.0, low=20.0, high=0.0):
    """HTK mel triangles in float64 numpy: mel(f) = 1127 ln(1 + f/700), num_bins + 2 equally spaced edges between mel(low) and
    mel(Nyquist + high), weight = max(0, min(up, down)) at the mel of every FFT bin below Nyquist."""
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    if high <= 0.0:
        high += 0.5 * sr
    lo, hi = mel(low), mel(high)
    delta = (hi - lo) / (num_bins + 1)
    b = np.arange(num_bins, dtype=np.float64)[:, None]
    left, center, right = lo + b * delta, lo + (b + 1.0) * delta, lo + (b + 2.0) * delta
    m = mel(sr / padded * np.arange(padded // 2))[None, :]
    return np.maximum(0.0, np.minimum((m - left) / (center - left), (right - m) / (right - center)))


def test_kaldi_mel_banks_shape_sparsity_and_pattern():
    fb = MD.kaldi_mel_banks(128)
    assert fb.dtype == torch.float32 and tuple(fb.shape) == (128, 256)
    nnz = (fb != 0).sum(dim=1)
    assert int(nnz.max()) <= 10
    assert [i for i in range(128) if int(nnz[i]) == 0] == [3]          # Kaldi's empty bin: reproduced, not patched
    assert np.array_equal(fb.numpy() != 0, mel_banks_f64(128) != 0)    # the fp32 and the fp64 build agree on the pattern
    # every row is one contiguous run, which is what the packed form stores
    from src.utils.utils import pack_filterbank
    st, pk = pack_filterbank(fb.numpy())
    assert pk.shape == (128, 10) and int((pk != 0).sum()) == int(nnz.sum())


def test_kaldi_mel_banks_equal_the_fp64_closed_form():
    """The table against the fp64 closed form, 1e-5 relative on every non-zero weight.  The table is evaluated in float64 and
    rounded once for this reason: the same ops in float32 (torchaudio's own arithmetic, `dtype=torch.float32`) miss the bound -
    largest absolute difference 1.38e-5, largest relative difference 1.62e-3 at a weight of 0.0043, 162 of the 504 non-zero
    weights beyond 1e-5."""
    got, ref = MD.kaldi_mel_banks(128).double().numpy(), mel_banks_f64(128)
    nz = ref != 0
    rel = np.abs(got[nz] - ref[nz]) / ref[nz]
    print("mel bank: max abs diff", np.abs(got - ref).max(), "max rel diff on the non-zeros", rel.max())
    assert rel.max() <= 1e-5


def test_kaldi_mel_banks_float32_arithmetic_is_available():
    """`dtype=torch.float32` runs the ops as torchaudio runs them.  Float32 cancellation (mel values up to 2,840, spacing 2.4e-4,
    over a 21.8-mel band) bounds its distance from the default build by a few 1e-5 absolute; the pattern is the same."""
    a, b = MD.kaldi_mel_banks(128), MD.kaldi_mel_banks(128, dtype=torch.float32)
    assert b.dtype == torch.float32 and torch.equal(a != 0, b != 0) and not torch.equal(a, b)
    # |d weight| <= (ulp(2840) for the bin mel + ulp(2840) for the edge + their difference's rounding) / 21.8 mel ~ 3e-5
    assert float((a - b).abs().max()) <= 3e-5


def test_kaldi_window_is_the_symmetric_hann():
    w = MD.kaldi_window(400).double().numpy()
    ref = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400) / 399.0)
    assert w.shape == (400,) and np.abs(w - ref).max() < 1e-6
    assert np.allclose(w, w[::-1], atol=1e-7) and w[0] == 0.0


# ------------------------------------------------------------------------------------------------ planners
def draws_transcribed(B, F, T, freqm, timem):
    """torchaudio.functional.mask_along_axis, once per axis per clip, frequency first."""
    out = []
    for _ in range(B):
        row = []
        for param, size in ((freqm, F), (timem, T)):
            if param == 0:
                row += [0, 0]
                continue
            value = torch.rand(1) * param
            min_value = torch.rand(1) * (size - value)
            start = int(min_value)
            end = start + int(value)
            row += [start, end]
        out.append(row)
    return out


@pytest.mark.parametrize("seed", range(8))
def test_plan_masks_equals_the_transcribed_draws(seed):
    B, F, T = 5, 128, 1024
    torch.manual_seed(seed)
    ref = draws_transcribed(B, F, T, 24, 192)
    state_ref = torch.get_rng_state()
    torch.manual_seed(seed)
    got = MD.plan_masks(B, F, T, 24, 192)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, 4)
    assert got.tolist() == ref
    assert torch.equal(torch.get_rng_state(), state_ref)
    g = got.numpy()
    assert (g[:, 0] >= 0).all() and (g[:, 1] <= F).all() and (g[:, 1] - g[:, 0] < 24).all()
    assert (g[:, 2] >= 0).all() and (g[:, 3] <= T).all() and (g[:, 3] - g[:, 2] < 192).all()


def test_plan_masks_zero_parameter_draws_nothing():
    torch.manual_seed(3)
    s0 = torch.get_rng_state()
    got = MD.plan_masks(4, 128, 1024, 0, 0)
    assert torch.equal(torch.get_rng_state(), s0) and got.tolist() == [[0, 0, 0, 0]] * 4
    got = MD.plan_masks(2, 128, 1024, 0, 192)                 # only the time draws
    torch.manual_seed(3)
    assert got.tolist() == draws_transcribed(2, 128, 1024, 0, 192)


def test_plan_batch_interleaves_mix_and_mask_draws_like_getitem():
    """dataloader.py:157-195 per clip: random.random() < mixup, random.randint(0, n - 1), np.random.beta(10, 10), then the
    frequency and the time band."""
    B = 6

    def seed():
        random.seed(11)
        np.random.seed(12)
        torch.manual_seed(13)

    seed()
    ref_p, ref_l, ref_b = [], [], []
    for _ in range(B):
        if random.random() < 0.5:
            ref_p.append(random.randint(0, B - 1))
            ref_l.append(np.random.beta(10, 10))
        else:
            ref_p.append(-1)
            ref_l.append(1.0)
        ref_b += draws_transcribed(1, 128, 1024, 24, 192)
    after = (random.random(), np.random.rand(), torch.get_rng_state())
    seed()
    partner, lam, bands = MD.plan_batch(B, 128, 1024, 24, 192, 0.5)
    assert partner.tolist() == ref_p and bands.tolist() == ref_b
    assert torch.equal(lam, torch.tensor(ref_l, dtype=torch.float32))
    assert -1 in ref_p and any(p >= 0 for p in ref_p)
    assert (random.random(), np.random.rand()) == after[:2] and torch.equal(torch.get_rng_state(), after[2])


def test_front_end_refuses_what_it_cannot_reproduce():
    with pytest.raises(NotImplementedError):
        MD.MastFrontEnd({"num_mel_bins": 128, "target_length": 1024, "freqm": 0, "timem": 0, "mixup": 0, "skip_norm": True,
                         "noise": True})
    with pytest.raises(NotImplementedError):
        MD.MastFrontEnd({"num_mel_bins": 128, "target_length": 1024, "skip_norm": True}, sr=44100)   # window pads to 2048
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MD.KaldiFbank(128)(torch.zeros(1, 16000))


# ------------------------------------------------------------------------------------------------ C ABI
def test_fbank_entry_rejects_bad_arguments_before_any_launch():
    from src import _native as N
    lib = N.lib()
    assert "audiossl_fbank_fwd" in N.PROTOS
    P = 256                                                     # a non-null address that is never dereferenced

    def call(wave=P, bands=None, bands_host=None, out=P, B=2, Lmax=16000, win_len=400, shift=160, n_fft=512, n_mels=128,
             taps=10, T=98, win=P, partner=None, lam=None, clip_mean=None, std=1.0, skip_norm=1):
        return lib.audiossl_fbank_fwd(wave, None, partner, lam, clip_mean, bands, bands_host, out, B, Lmax, win_len, shift, n_fft, n_mels,
                                      taps, T, win, P, P, P, 0.97, 1.1920929e-07, 0.0, std, skip_norm, 0, None)

    assert call(wave=None) == -1 and call(out=None) == -1 and call(win=None) == -1
    assert call(n_fft=1024) == -1 and call(n_fft=256) == -1
    assert call(win_len=256) == -1 and call(win_len=513) == -1 and call(win_len=0) == -1
    assert call(T=0) == -1 and call(T=-5) == -1
    assert call(shift=0) == -1 and call(B=0) == -1
    assert call(n_mels=129) == -1 and call(taps=30) == -1 and call(taps=0) == -1      # more than a wave's registers / LDS tile hold
    assert call(partner=P) == -1 and call(lam=P) == -1                                  # both or neither
    assert call(clip_mean=P) == -1                                                      # scratch of the mix only
    assert call(skip_norm=0, std=0.0) == -1
    ok = np.array([[0, 24, 0, 98], [128, 128, 98, 98]], dtype=np.int32)
    for bad in ([[0, 129, 0, 0], [0, 0, 0, 0]], [[0, 0, 0, 0], [0, 0, 0, 99]], [[-1, 3, 0, 0], [0, 0, 0, 0]],
                [[5, 4, 0, 0], [0, 0, 0, 0]], [[0, 0, 9, 8], [0, 0, 0, 0]]):
        tab = np.array(bad, dtype=np.int32)
        assert call(bands=P, bands_host=tab.ctypes.data) == -1, bad
    assert call(bands=None, bands_host=ok.ctypes.data) == -1    # a host copy without the device table
