"""Shared by tests/test_host_pcm.py and tests/test_gpu_pcm.py: WAV files in every sample format written into a temporary directory,
and the EXISTING host path on them (`ingest.decode`, then `extract_window` or the fbank batch's right padding) as the expectation."""
import struct

import numpy as np
import torch
from scipy.io import wavfile

RATE = 16000


def samples(fmt, n, C, salt):
    """[n] or [n, C] in the file dtype of `fmt`, seeded; the extremes and the int32 values that round in float32 come first."""
    rng = np.random.default_rng(1000 + salt)
    shape = (n,) if C == 1 else (n, C)
    if fmt == "u8":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        edge = [0, 255, 128, 127]
    elif fmt == "s16":
        a = rng.integers(-32768, 32768, shape, dtype=np.int16)
        edge = [-32768, 32767, 0, -1]
    elif fmt == "s32":
        a = rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int32)
        edge = [2 ** 24 + 1, 2 ** 31 - 1, -2 ** 31, 2 ** 25 + 3, -(2 ** 24) - 1, 0]
    elif fmt == "s24":                                       # as scipy hands a 24-bit file out: left-justified int32
        a = rng.integers(-2 ** 23, 2 ** 23, shape, dtype=np.int32) << 8
        edge = [(2 ** 23 - 1) << 8, -2 ** 31, 0]
    else:
        a = (rng.standard_normal(shape) * rng.choice([1e-3, 0.3, 1.0], shape)).astype(np.float32)
        edge = [1.0, -1.0, 0.0]
    flat = a.reshape(-1)
    k = min(len(edge), flat.size)
    flat[:k] = np.asarray(edge[:k]).astype(a.dtype)
    return a


def write_wav(path, data, rate=RATE):
    wavfile.write(str(path), rate, data)
    return str(path)


def write_wav24(path, data, rate=RATE):
    """A 24-bit PCM WAV written by hand (scipy writes none); `data` is left-justified int32, [n] or [n, C]."""
    data = np.asarray(data, np.int32)
    C = 1 if data.ndim == 1 else data.shape[1]
    raw = (data.reshape(-1, 1) >> np.array([8, 16, 24])).astype(np.uint8).tobytes()      # three little-endian bytes per sample
    head = b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, C, rate, rate * 3 * C, 3 * C, 24)
    with open(path, "wb") as f:
        f.write(head + b"data" + struct.pack("<I", len(raw)) + raw)
        if len(raw) % 2:
            f.write(b"\0")
    return str(path)


def write_clip(path, fmt, n, C, salt):
    data = samples(fmt, n, C, salt)
    return write_wav24(path, data) if fmt == "s24" else write_wav(path, data)


def host_row(path, unit, align, start=0):
    """What the float32 host path puts into the batch row of this file."""
    from src.dataset import ingest
    from src.utils import extract_window
    w = torch.from_numpy(ingest.decode(path)[0])
    if len(w) > unit:
        return w[start:start + unit]
    if align == 0:
        return extract_window(w, duration=unit)              # no draw: the clip is not longer than the window
    return torch.nn.functional.pad(w, (0, unit - len(w)))


# (format, channels, frames as a function of unit, window start): all four formats, C in {1, 2, 3}, n in {0, 1, 7, unit - 1, unit} and
# one clip longer than the window; odd frame counts of 16-bit mono clips in a row put the following offsets off the 16-byte grid
MIXED = [("s16", 1, lambda u: u, 0), ("s16", 1, lambda u: 7, 0), ("s16", 1, lambda u: u - 1, 0), ("u8", 2, lambda u: 1, 0),
         ("s16", 2, lambda u: u + 37, 5), ("s32", 3, lambda u: 7, 0), ("f32", 1, lambda u: 0, 0), ("f32", 3, lambda u: u - 1, 0),
         ("s32", 1, lambda u: u, 0)]


def make_batch(tmp_path, cases, unit, align):
    """-> (PcmBatch, expected [B, unit] float32 from the host path)."""
    from src.dataset import ingest
    clips, starts, want = [], [], []
    for i, (fmt, C, nf, start) in enumerate(cases):
        p = write_clip(tmp_path / f"c{i}_{unit}.wav", fmt, nf(unit), C, 10 * i + C)
        clips.append(ingest.decode_raw(p))
        starts.append(start)
        want.append(host_row(p, unit, align, start))
    return ingest.PcmBatch.pack(clips, starts, unit, align), torch.stack(want)
