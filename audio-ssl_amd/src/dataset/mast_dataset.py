"""Host side of the MAST loader's front end (`extras/mast_new/mast/dataloader.py:98-214`, `run_mvit.py:107-125`,
`get_norm_stats.py`): Kaldi-compatible fbank, cut / zero-pad to `target_length`, frequency and time masks, (x - mean) / (2 std),
optional two-file mix - one `audiossl_fbank_fwd` call per batch (one kernel; with a mix a small clip-mean kernel runs first).

  kaldi_mel_banks / kaldi_window   the tables of torchaudio.compliance.kaldi (its operation order; the bank in float64, rounded once)
  plan_masks                       torchaudio's `mask_along_axis` draws from torch's global CPU generator, per clip
  plan_mix                         `__getitem__`'s mix draws (python `random`, numpy's global generator)
  MastFrontEnd(audio_conf)         waves (or a right-padded `ingest.PcmBatch`) -> [B, 1, F, T] network input on the device
  make_features                    `run_mvit.py`'s function with its built-in AudioSet statistics
  norm_stats                       `get_norm_stats.py`

torchaudio is not a dependency: the tables are restated from its published formulas and are parity-unpinned against it
(DESIGN.md), like the librosa tables of `src/utils/utils.py`.
"""
import math
import random

import numpy as np
import torch

from src import _native as N
from src.utils.utils import pack_filterbank

PADDED = 512                           # Kaldi rounds the 25 ms window (400 samples at 16 kHz) up to a power of two
PREEMPH = 0.97
EPS = float(torch.finfo(torch.float32).eps)
AUDIOSET_MEAN, AUDIOSET_STD = -4.2677393, 4.5689974        # run_mvit.py:124


# ------------------------------------------------------------------------------------- host tables
def kaldi_mel_banks(num_bins, padded=PADDED, sr=16000, low=20.0, high=0.0, dtype=torch.float64):
    """float32 [num_bins, padded/2]: HTK-scale, un-normalised triangles over the bins below Nyquist (the Nyquist bin has zero
    weight in Kaldi's bank), evaluated with torch ops in the order kaldi.get_mel_banks evaluates them (scalars in python floats).

    `dtype` is the precision of the tensor arithmetic; the result is rounded to float32 once.  The default float64 gives every
    weight to float32 rounding (5.5e-8 relative).  torchaudio itself runs these ops in float32: the slopes are then differences of
    mel values of up to 2,840 (float32 spacing 2.4e-4) over a band of 21.8 mel, which puts about 1e-5 of absolute error into
    every weight (128 bins: up to 1.4e-5 absolute, 1.6e-3 relative on the small weights at the feet of the triangles).
    `dtype=torch.float32` reproduces that arithmetic; both builds have the same non-zero pattern."""
    def mel_scalar(f):
        return 1127.0 * math.log(1.0 + f / 700.0)

    num_fft_bins = padded // 2
    nyquist = 0.5 * sr
    if high <= 0.0:
        high += nyquist
    fft_bin_width = sr / padded
    mel_lo, mel_hi = mel_scalar(low), mel_scalar(high)
    delta = (mel_hi - mel_lo) / (num_bins + 1)
    b = torch.arange(num_bins, dtype=dtype).unsqueeze(1)
    left = mel_lo + b * delta
    center = mel_lo + (b + 1.0) * delta
    right = mel_lo + (b + 2.0) * delta
    mel = (1127.0 * (1.0 + (fft_bin_width * torch.arange(num_fft_bins, dtype=dtype)) / 700.0).log()).unsqueeze(0)
    up = (mel - left) / (center - left)
    down = (right - mel) / (right - center)
    return torch.max(torch.zeros(1, dtype=dtype), torch.min(up, down)).float()


def kaldi_window(win_len=400):
    """The symmetric Hann window of window_type='hanning'."""
    return torch.hann_window(win_len, periodic=False)


# ------------------------------------------------------------------------------------- planners
def _axis_band(param, size):
    """One `mask_along_axis` call (torchaudio.functional): two float32 draws from torch's global CPU generator."""
    value = torch.rand(1) * param
    min_value = torch.rand(1) * (size - value)
    start = int(min_value)
    end = start + int(value)
    return start, end


def _clip_bands(F, T, freqm, timem):
    f0 = f1 = t0 = t1 = 0
    if freqm != 0:                                           # dataloader.py:192-195: a parameter of 0 skips the call
        f0, f1 = _axis_band(freqm, F)
    if timem != 0:
        t0, t1 = _axis_band(timem, T)
    return f0, f1, t0, t1


def plan_masks(B, F, T, freqm, timem):
    """int32 [B, 4] = {f0, f1, t0, t1} per clip: FrequencyMasking(freqm) then TimeMasking(timem) on a [1, F, T] image, T being
    the target length (padding comes first)."""
    return torch.tensor([_clip_bands(F, T, freqm, timem) for _ in range(B)], dtype=torch.int32).reshape(B, 4)


def _clip_mix(n, mixup):
    """dataloader.py:157-163, 124: (partner | -1, lambda)."""
    if random.random() < mixup:
        partner = random.randint(0, n - 1)
        return partner, float(np.random.beta(10, 10))
    return -1, 1.0


def plan_mix(B, mixup, n=None):
    """(partner int32 [B], lam float32 [B]); the partner is drawn among `n` clips (default: the batch)."""
    draws = [_clip_mix(n or B, mixup) for _ in range(B)]
    return torch.tensor([d[0] for d in draws], dtype=torch.int32), torch.tensor([d[1] for d in draws], dtype=torch.float32)


def plan_batch(B, F, T, freqm, timem, mixup):
    """The draws of B consecutive `__getitem__` calls in their order (dataloader.py:157-195): per clip the mix draws, then the
    frequency band, then the time band."""
    mix, bands = [], []
    for _ in range(B):
        mix.append(_clip_mix(B, mixup))
        bands.append(_clip_bands(F, T, freqm, timem))
    return (torch.tensor([m[0] for m in mix], dtype=torch.int32), torch.tensor([m[1] for m in mix], dtype=torch.float32),
            torch.tensor(bands, dtype=torch.int32).reshape(B, 4))


# ------------------------------------------------------------------------------------- front end
class KaldiFbank:
    """Tables of one fbank configuration and the launch."""

    def __init__(self, num_mel_bins=128, sr=16000, frame_length_ms=25.0, frame_shift_ms=10.0, bank_dtype=torch.float64):
        """bank_dtype: arithmetic of `kaldi_mel_banks` - float64 (default, every weight correctly rounded) or float32 (the table
        torchaudio's own float32 ops build, up to 1.4e-5 per weight away)."""
        self.win_len = int(sr * frame_length_ms * 0.001)
        self.shift = int(sr * frame_shift_ms * 0.001)
        padded = 1 << (self.win_len - 1).bit_length()
        if padded != PADDED:
            raise NotImplementedError(f"the HIP fbank is specialised for a 512-point padded window (16 kHz); sr={sr} pads to {padded}")
        self.n_mels = num_mel_bins
        self.banks = kaldi_mel_banks(num_mel_bins, padded, sr, dtype=bank_dtype)
        self._starts, self._packed = pack_filterbank(self.banks.numpy())
        taps = self._packed.shape[1]
        if num_mel_bins > 128 or taps > 29 or (taps > 21 and num_mel_bins > 64):
            raise NotImplementedError("the HIP fbank holds at most 128 mel rows of at most 21 taps, or 64 rows of at most 29")
        self._win = kaldi_window(self.win_len).numpy()
        ang = -2.0 * np.pi * np.arange(PADDED, dtype=np.float64) / PADDED
        self._tw = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
        self._dev = {}

    def _tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                                   for a in (self._win, self._tw, self._packed, self._starts))
        return self._dev[key]

    def n_frames(self, n_samples):
        return 1 + (n_samples - self.win_len) // self.shift if n_samples >= self.win_len else 0

    def __call__(self, wave, lens=None, target_length=None, bands=None, partner=None, lam=None, mean=0.0, std=1.0,
                 skip_norm=True, time_major=False):
        """wave [B, Lmax] f32 on the device; lens / partner / lam / bands host or device tensors.  -> [B, 1, F, T] (or [B, T, F])."""
        if not wave.is_cuda:
            raise RuntimeError("the fbank front end needs device tensors (no CPU fallback exists)")
        wave = wave.float().contiguous()
        B, Lmax = wave.shape
        dev = wave.device
        T = int(target_length) if target_length is not None else self.n_frames(Lmax)
        if T <= 0:
            raise ValueError("no frames: the clips are shorter than one window and no target_length was given")
        i32 = lambda x: None if x is None else torch.as_tensor(x).to(dtype=torch.int32).contiguous()
        lens_d = None if lens is None else i32(lens).to(dev)
        bands_h = None if bands is None else i32(bands).cpu().reshape(B, 4)
        bands_d = None if bands is None else bands_h.to(dev)
        partner_d = None if partner is None else i32(partner).to(dev)
        lam_d = None if partner is None else torch.as_tensor(lam).to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty((B, T, self.n_mels) if time_major else (B, 1, self.n_mels, T), dtype=torch.float32, device=dev)
        win, tw, packed, starts = self._tables(dev)
        clip_mean = None if partner is None else torch.empty(B, dtype=torch.float32, device=dev)
        N.call("fbank_fwd", wave, lens_d, partner_d, lam_d, clip_mean, bands_d, None if bands_h is None else bands_h.data_ptr(), out,
               B, Lmax, self.win_len, self.shift, PADDED, self.n_mels, packed.shape[1], T, win, tw, packed, starts,
               PREEMPH, EPS, float(mean), float(std), int(bool(skip_norm)), int(bool(time_major)))
        return out


def _batch(waves, lens):
    """[B, L] tensor or list of 1-D tensors -> ([B, Lmax] tensor, lens or None)."""
    if isinstance(waves, (list, tuple)):
        ws = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waves]
        lens = torch.tensor([len(w) for w in ws], dtype=torch.int32)
        out = torch.zeros(len(ws), int(lens.max()), dtype=torch.float32, device=ws[0].device)
        for i, w in enumerate(ws):
            out[i, :len(w)] = w
        return out, lens
    waves = torch.as_tensor(waves, dtype=torch.float32)
    return waves.reshape(-1, waves.shape[-1]), lens


class MastFrontEnd:
    """`AudiosetDataset.__getitem__`'s feature chain for a whole batch, configured by the reference's `audio_conf` dictionary
    (num_mel_bins, target_length, freqm, timem, mixup, mean, std, skip_norm, noise).  The random draws are the reference's, from
    the same generators in the same order; mix partners are drawn among the clips of the batch."""

    def __init__(self, audio_conf, sr=16000, bank_dtype=torch.float64):
        if audio_conf.get("noise"):
            # dataloader.py:207-209 adds a T x F torch.rand field per clip from the CPU generator: not reproducible on the device
            raise NotImplementedError("audio_conf['noise'] is not implemented on the HIP path")
        self.fbank = KaldiFbank(audio_conf.get("num_mel_bins", 128), sr, bank_dtype=bank_dtype)
        self.melbins = self.fbank.n_mels
        self.target_length = int(audio_conf["target_length"])
        self.freqm = audio_conf.get("freqm") or 0
        self.timem = audio_conf.get("timem") or 0
        self.mixup = audio_conf.get("mixup") or 0.0
        self.skip_norm = bool(audio_conf.get("skip_norm"))
        self.norm_mean, self.norm_std = audio_conf.get("mean"), audio_conf.get("std")
        if not self.skip_norm and (self.norm_mean is None or self.norm_std is None):
            raise ValueError("audio_conf needs 'mean' and 'std' unless 'skip_norm' is set")
        self.last_plan = None

    def __call__(self, waves, lens=None, time_major=False):
        """waves: [B, L] tensor, a list of 1-D clips, or a `PcmBatch` packed with align=1 (its windows are converted on the device,
        `lens` are the batch's frame counts and Lmax its unit)."""
        from src.dataset.ingest import PcmBatch, pcm_window
        if isinstance(waves, PcmBatch):
            if waves.align != 1:
                raise ValueError("the fbank front end takes right-padded clips: PcmBatch.pack(..., align=1)")
            waves, lens = pcm_window(waves), waves.lens
        else:
            waves, lens = _batch(waves, lens)
        B = waves.shape[0]
        partner, lam, bands = plan_batch(B, self.melbins, self.target_length, self.freqm, self.timem, self.mixup)
        self.last_plan = (partner, lam, bands)               # lam weighs the labels (dataloader.py:170-174)
        mixing = bool((partner >= 0).any())
        return self.fbank(waves.cuda(), lens, self.target_length, bands if (self.freqm or self.timem) else None,
                          partner if mixing else None, lam if mixing else None,
                          0.0 if self.skip_norm else self.norm_mean, 1.0 if self.skip_norm else self.norm_std,
                          self.skip_norm, time_major)


_FEATURES = {}


def make_features(wave, mel_bins=128, target_length=1000, bank_dtype=torch.float64):
    """`run_mvit.py:107-125` on a decoded waveform ([L], [1, L] or a batch [B, L]): fbank, cut / pad, AudioSet statistics.
    -> [target_length, mel_bins] (the reference's layout; [B, target_length, mel_bins] for a batch) on the device."""
    wave = torch.as_tensor(wave, dtype=torch.float32)
    single = wave.dim() == 1 or wave.shape[0] == 1
    fb = _FEATURES.get((mel_bins, bank_dtype))
    if fb is None:
        fb = _FEATURES[(mel_bins, bank_dtype)] = KaldiFbank(mel_bins, bank_dtype=bank_dtype)
    out = fb(wave.reshape(-1, wave.shape[-1]).cuda(), None, target_length, mean=AUDIOSET_MEAN, std=AUDIOSET_STD, skip_norm=False,
             time_major=True)
    return out[0] if single else out


def norm_stats(batches):
    """`get_norm_stats.py`: (mean of the per-batch torch.mean, mean of the per-batch torch.std) over `skip_norm` outputs."""
    means, stds = [], []
    for x in batches:
        x = x.double()                                       # fp64 accumulation: the figure does not depend on the reduction order
        means.append(float(torch.mean(x)))
        stds.append(float(torch.std(x)))
    if not means:
        raise ValueError("norm_stats needs at least one batch")
    return float(np.mean(means)), float(np.mean(stds))
