"""Audio ingest for the MI355X path: decode on the host, resample to the training rate on the GPU.

The reference reads every file with `librosa.core.load(path, sr=16000)` (`src/dataset/upstream_dataset.py:55`): soundfile /
audioread decode to float32, channel mean, then `resampy.resample(y, sr_orig, 16000, filter='kaiser_best')` and
`librosa.util.fix_length` to ceil(n * ratio) samples.  librosa 0.8.1 and resampy 0.2.2 are not in the reference tree nor in
this image: the resampler is restated from resampy's published algorithm and filter parameters (parity unpinned) -
`kaiser_best` = 64 zero crossings x 512 table entries, Kaiser beta 14.769656459379492, roll-off 0.9475937167399596.
Host part: the filter table (float64, built once) and, per (input length, rate pair), the positions of every output sample from
resampy's sequentially accumulated float64 time register; device part: `audiossl_resample_sinc`, one thread per output sample.
Decoding stays `scipy.io.wavfile` (PCM WAV) / `.npy`.

Packed upload (opt-in, `run.pcm_upload`): `decode_raw` keeps a clip in its file's sample format (`PcmClip`), `PcmBatch.pack` copies the
training window of every clip of a batch into ONE pinned buffer (table + samples, one host-to-device copy, half the bytes of the
float32 batch for 16-bit audio) and `pcm_window` (`audiossl_pcm_window`) converts, mixes down and pads on the GPU - bit for bit what
`decode` + `extract_window` (or the fbank batch's right padding) produce on the host."""
import math

import numpy as np
import torch

from src import _native as N

KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)
_FILTERS, _PLANS = {}, {}


def sinc_window(num_zeros, precision, beta, rolloff):
    """resampy.filters.sinc_window with a Kaiser taper: right half of the interpolation filter, (table, entries per zero)."""
    num_bits = 2 ** precision
    n = num_bits * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc_win, num_bits


def positions(n_orig, sample_ratio, nwin, num_table):
    """Per output sample: n, (offset, eta) of the left and right wing - `resampy.interpn.resample_f`, time register included."""
    n_out = int(n_orig * sample_ratio)
    scale = min(1.0, sample_ratio)
    inc = np.full(n_out, 1.0 / sample_ratio)
    inc[0] = 0.0
    time_register = np.add.accumulate(inc)                  # 0, inc, inc + inc, ... (sequential float64 additions)
    n = time_register.astype(np.int64)
    frac = scale * (time_register - n)
    index_frac = frac * num_table
    off_l = index_frac.astype(np.int64)
    eta_l = index_frac - off_l
    frac = scale - frac
    index_frac = frac * num_table
    off_r = index_frac.astype(np.int64)
    eta_r = index_frac - off_r
    return n_out, n.astype(np.int32), off_l.astype(np.int32), off_r.astype(np.int32), eta_l, eta_r, int(scale * num_table)


def _filter(name, sample_ratio, device):
    key = (name, round(sample_ratio, 12) if sample_ratio < 1 else 1.0, str(device))
    if key not in _FILTERS:
        if name != "kaiser_best":
            raise NotImplementedError("only librosa's default res_type 'kaiser_best' is built")
        win, num_table = sinc_window(**KAISER_BEST)
        if sample_ratio < 1:
            win = win * sample_ratio
        delta = np.zeros_like(win)
        delta[:-1] = np.diff(win)
        _FILTERS[key] = (torch.from_numpy(win).to(device), torch.from_numpy(delta).to(device), num_table)
    return _FILTERS[key]


@torch.no_grad()
def resample(wave, sr_orig, sr_new, res_type="kaiser_best", fix=True):
    """wave [n] or [clips, n] float32 -> resampled on the GPU, [..., ceil(n * sr_new / sr_orig)] like librosa.resample (fix=True
    pads / trims resampy's int(n * ratio) samples to that length)."""
    wave = torch.as_tensor(wave, dtype=torch.float32)
    squeeze = wave.dim() == 1
    x = (wave if wave.is_cuda else wave.cuda()).reshape(-1, wave.shape[-1]).contiguous()
    if sr_orig == sr_new:
        return x[0] if squeeze else x
    ratio = float(sr_new) / sr_orig
    clips, n_orig = x.shape
    win, delta, num_table = _filter(res_type, ratio, x.device)
    key = (n_orig, sr_orig, sr_new, res_type, str(x.device))
    if key not in _PLANS:
        n_out, n, ol, orr, el, er, step = positions(n_orig, ratio, win.numel(), num_table)
        _PLANS.clear() if len(_PLANS) > 64 else None
        _PLANS[key] = (n_out, step) + tuple(torch.from_numpy(a).to(x.device) for a in (n, ol, orr, el, er))
    n_out, step, n_d, ol_d, or_d, el_d, er_d = _PLANS[key]
    if n_out < 1:
        raise ValueError("Input signal length is too small to resample")
    y = torch.empty(clips, n_out, dtype=torch.float32, device=x.device)
    N.call("resample_sinc", x, y, clips, n_orig, n_out, n_d, ol_d, or_d, el_d, er_d, win, delta, win.numel(), step)
    if fix:
        want = int(math.ceil(n_orig * ratio))
        if want != n_out:
            y = torch.nn.functional.pad(y, (0, want - n_out)) if want > n_out else y[:, :want]
    return y[0] if squeeze else y


def decode(path):
    """-> (float32 mono numpy array, native sample rate); PCM WAV through scipy, `.npy` arrays are taken as 16 kHz."""
    if str(path).endswith(".npy"):
        return np.load(path, allow_pickle=False).astype(np.float32), 16000
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    return _to_float(data), int(rate)


# ------------------------------------------------------------------------------------- packed PCM batches
PCM_FORMATS = {np.dtype(np.uint8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2, np.dtype(np.float32): 3}
PCM_MAX_CHANNELS = 8
TABLE_ALIGN = 256                      # the table leads the packed buffer, padded so that the sample area keeps the buffer's alignment


def _to_float(data):
    """`decode`'s arithmetic on an array in the file's dtype, [n] or [n, C] -> float32 mono."""
    if data.dtype.kind == "i":
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1)
    elif data.dtype.kind == "u":
        data = (data.astype(np.float32) - 128.0) / 128.0
    data = data.astype(np.float32)
    if data.ndim > 1:
        data = data.mean(axis=1)                           # librosa.to_mono
    return data


class PcmClip:
    """A decoded clip still in its file's sample format: `data` [n] or [n, C] (uint8 / int16 / int32 / float32), `rate`."""

    def __init__(self, data, rate):
        data = np.asarray(data)
        if data.dtype not in PCM_FORMATS:                  # float64 WAV: `decode` rounds it to float32 before the channel mean
            data = data.astype(np.float32)
        if data.ndim not in (1, 2) or (data.ndim == 2 and not 1 <= data.shape[1] <= PCM_MAX_CHANNELS):
            raise ValueError(f"a clip is [n] or [n, C <= {PCM_MAX_CHANNELS}], got {data.shape}")
        self.data, self.rate = data, int(rate)

    def __len__(self):
        return self.data.shape[0]

    @property
    def channels(self):
        return 1 if self.data.ndim == 1 else self.data.shape[1]

    def window(self, start, unit):
        """The frames `start : start + unit` (the whole clip when it is not longer than `unit`) - what a batch ships."""
        return self if len(self) <= unit else PcmClip(self.data[start:start + unit], self.rate)

    def to_float(self):
        """Exactly `decode(path)[0]`."""
        return _to_float(self.data)


def decode_raw(path):
    """-> PcmClip: the file's samples in their own dtype (`.npy`: float32 at 16 kHz); `.to_float()` gives `decode(path)[0]`."""
    if str(path).endswith(".npy"):
        return PcmClip(np.load(path, allow_pickle=False).astype(np.float32), 16000)
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    return PcmClip(data, rate)


def _in_worker():
    import torch.utils.data as tud
    return tud.get_worker_info() is not None


class PcmBatch:
    """The windows of B clips in their own sample formats in one buffer: int64 table [B, 4] = (byte offset into the sample area,
    frames, channels, format) padded to 256 bytes, then the interleaved frames of every clip (each at a multiple of its sample
    size), the whole padded to 16 bytes.  Stands in for the [B, unit] float32 waveform tensor between the collate and the front
    end: `.to` / `.cuda` move it with one copy, `pcm_window` turns it into that tensor on the device."""

    def __init__(self, host, dev, B, unit, align, lens):
        self._host, self._dev, self.B, self.unit, self.align, self.lens = host, dev, B, unit, align, lens

    @staticmethod
    def table_bytes(B):
        return -(-B * 32 // TABLE_ALIGN) * TABLE_ALIGN

    @classmethod
    def pack(cls, clips, starts, unit, align=0):
        """clips: PcmClip, or float32 arrays / tensors (resampled clips); starts[b]: first frame of the window of a clip longer
        than `unit`.  Only the window's frames are copied.  align 0: centre padding (`extract_window`), 1: right padding (fbank)."""
        B, unit = len(clips), int(unit)
        wins, rows, pos = [], [], 0
        for b, c in enumerate(clips):
            a = c.data if isinstance(c, PcmClip) else (c.numpy() if isinstance(c, torch.Tensor) else np.asarray(c))
            if a.dtype not in PCM_FORMATS:
                a = a.astype(np.float32)
            if a.shape[0] > unit:
                s = int(starts[b])
                a = a[s:s + unit]
            ch = 1 if a.ndim == 1 else a.shape[1]
            if a.ndim > 2 or ch > PCM_MAX_CHANNELS:
                raise ValueError(f"clip {b}: [n] or [n, C <= {PCM_MAX_CHANNELS}] expected, got {a.shape}")
            pos = -(-pos // a.itemsize) * a.itemsize
            rows.append((pos, a.shape[0], ch, PCM_FORMATS[a.dtype]))
            wins.append(a)
            pos += a.size * a.itemsize
        tb = cls.table_bytes(B)
        total = tb + -(-pos // 16) * 16
        host = torch.empty(total, dtype=torch.uint8, pin_memory=torch.cuda.is_available() and not _in_worker())
        buf = host.numpy()
        buf[:tb].view(np.int64)[:4 * B] = np.asarray(rows, np.int64).reshape(-1)
        buf[B * 32:tb] = 0
        buf[tb + pos:] = 0
        for (off, n, ch, _), a in zip(rows, wins):
            buf[tb + off:tb + off + a.size * a.itemsize].view(a.dtype).reshape(a.shape)[...] = a
        return cls(host, None, B, unit, int(align), torch.tensor([r[1] for r in rows], dtype=torch.int32))

    # ---- what the call sites use on a waveform tensor
    @property
    def shape(self):
        return (self.B, self.unit)

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    @property
    def nbytes(self):
        return self._host.numel()

    @property
    def is_cuda(self):
        return self._dev is not None

    @property
    def device(self):
        return self._host.device if self._dev is None else self._dev.device

    @property
    def table(self):
        """The host copy of the table, int64 [B, 4] (a view of the packed buffer)."""
        return self._host[:self.B * 32].view(torch.int64).view(self.B, 4)

    def pin_memory(self):
        if not self._host.is_pinned() and torch.cuda.is_available() and not _in_worker():
            self._host = self._host.pin_memory()           # packed in a loader worker: page-locked here, in the main process
        return self

    def to(self, device, non_blocking=False):
        device = torch.device(device)
        if device.type != "cuda":
            return PcmBatch(self._host, None, self.B, self.unit, self.align, self.lens)
        if self._dev is not None and device.index in (None, self._dev.device.index):
            return self
        return PcmBatch(self._host, self._host.to(device, non_blocking=non_blocking), self.B, self.unit, self.align, self.lens)

    def cuda(self, non_blocking=False):
        return self.to(torch.device("cuda", torch.cuda.current_device()), non_blocking=non_blocking)

    def record_stream(self, stream):
        if self._dev is not None:
            self._dev.record_stream(stream)


@torch.no_grad()
def pcm_window(batch, out=None):
    """PcmBatch -> [B, unit] float32 on the device (uploaded first when it is still on the host): one `audiossl_pcm_window` launch
    on the current stream.  out: a contiguous float32 device tensor of at least B rows of `unit` to write into (rows past B are
    left alone)."""
    if not batch.is_cuda:
        batch = batch.cuda(non_blocking=True)
    dev = batch._dev
    dev.record_stream(torch.cuda.current_stream(dev.device))
    tb = PcmBatch.table_bytes(batch.B)
    if out is None:
        out = torch.empty(batch.B, batch.unit, dtype=torch.float32, device=dev.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] < batch.B or out.shape[1] != batch.unit:
        raise ValueError(f"out must be float32 [>= {batch.B}, {batch.unit}], got {out.dtype} {tuple(out.shape)}")
    N.call("pcm_window", dev.data_ptr() + tb, dev.numel() - tb, dev.data_ptr(), batch._host.data_ptr(), out, batch.B, batch.unit,
           batch.align)
    return out
