"""Downstream (labelled) data path - API mirror of `src/dataset/downstream_dataset.py:64-107` of the reference
(`DownstreamDataset(args, config, split, tfms=None, labels_dict=None)`, a CSV with `wav` and `label` columns).

The reference decodes, crops and log-mels ONE clip per `__getitem__` on the CPU; here the dataset hands out the cropped
waveform and `DownstreamFrontEnd` turns a whole [B, L] batch into [B, 1, n_mels, T] log-mels on the GPU (`logmel_fwd`).
`per_sample=True` keeps the reference's item shape (log-mel computed through the same kernel, one clip per call).
`pcm=True` (config key `run.pcm_upload`) hands out the window in the file's own sample format (`PcmClip`); `PcmCollate` packs a
batch of them into one `PcmBatch` and `DownstreamFrontEnd` converts it on the GPU into the same float32 windows, bit for bit.
The HuggingFace variant (`DownstreamDatasetHF`) downloads its data and is not available offline: it raises.
Label ids: the reference enumerates a python `set` of strings (order changes from run to run); here the labels are sorted."""
import pandas as pd
import torch
from torch.utils.data import Dataset

from src.dataset.upstream_dataset import _waveforms, load_audio
from src.utils import MelSpectrogramLibrosa, extract_log_mel_spectrogram, extract_window
from src.utils.utils import window_start


class DownstreamDataset(Dataset):
    def __init__(self, args, config, split, tfms=None, labels_dict=None, per_sample=False, pcm=False):
        self.pcm = pcm
        self.config, self.task, self.split = config, getattr(args, "task", None), split
        path = {"train": getattr(args, "train_csv", None), "valid": getattr(args, "valid_csv", None),
                "validation": getattr(args, "valid_csv", None), "test": getattr(args, "test_csv", None)}[split]
        self.dataset = pd.read_csv(path)
        self.sample_rate = config["downstream"]["input"]["sampling_rate"]
        self.duration = config["run"]["duration"]
        self.labels_dict = self.get_label2id() if labels_dict is None else labels_dict
        self.no_of_classes = len(self.labels_dict)
        self.per_sample = per_sample
        self.to_mel_spec = MelSpectrogramLibrosa() if per_sample else None
        self.tfms = tfms

    def get_label2id(self):
        return {k: i for i, k in enumerate(sorted(set(self.dataset["label"]), key=str))}

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        row = self.dataset.iloc[idx, :]
        wave = load_audio(row["wav"], self.sample_rate, raw=self.pcm and not self.per_sample)
        label = self.labels_dict[row["label"]]
        if self.pcm and not self.per_sample:
            unit = int(self.duration * 16000)
            start, _ = window_start(len(wave), unit)         # `extract_window`'s draw; the padding is left to the kernel
            return (wave.window(start, unit) if hasattr(wave, "window") else wave[start:start + unit]), label
        wave = extract_window(torch.from_numpy(wave), data_size=self.duration)
        if not self.per_sample:
            return wave, label
        mel = extract_log_mel_spectrogram(wave.cuda(), self.to_mel_spec).unsqueeze(0)
        if self.tfms:
            mel = self.tfms(mel)
        return mel, label


class DownstreamDatasetHF(Dataset):
    def __init__(self, *a, **k):
        raise NotImplementedError("DownstreamDatasetHF downloads its dataset from the HuggingFace hub; provide CSVs "
                                  "(--train_csv / --test_csv) and use DownstreamDataset instead")


class PcmCollate:
    """`collate_fn` of a `DownstreamDataset(pcm=True)` loader: [(window, label), ...] -> (PcmBatch, int64 labels)."""

    def __init__(self, unit_length):
        self.unit = int(unit_length)

    def __call__(self, items):
        from src.dataset.ingest import PcmBatch
        clips = [w for w, _ in items]
        return PcmBatch.pack(clips, [0] * len(clips), self.unit), torch.tensor([l for _, l in items], dtype=torch.int64)


class DownstreamFrontEnd:
    """[B, L] waveforms or a `PcmBatch` -> [B, 1, n_mels, T] log-mel on the GPU (one launch per batch, two for a `PcmBatch`)."""

    def __init__(self):
        self.to_mel_spec = MelSpectrogramLibrosa()

    @torch.no_grad()
    def __call__(self, waves):
        waves = _waveforms(waves.cuda(non_blocking=True))
        return extract_log_mel_spectrogram(waves.float().contiguous(), self.to_mel_spec).unsqueeze(1)

    @torch.no_grad()
    def ragged(self, waves, lens=None):
        """Clips of different lengths: [B, Lmax] float32 with lens[b] samples at the head of row b, or a `PcmBatch` packed with
        align=1 (its own `.lens`) -> ([B, 1, n_mels, Tmax] log-mel with zeros after each clip's frames, lens int32 on the device)."""
        from src.dataset.ingest import PcmBatch, pcm_window
        if isinstance(waves, PcmBatch):
            if waves.align != 1:
                raise ValueError("a ragged batch takes left-aligned rows: PcmBatch.pack(..., align=1)")
            lens = waves.lens if lens is None else lens
            waves = pcm_window(waves)
        elif lens is None:
            raise ValueError("lens is required with a waveform tensor")
        x, lens_dev = self.to_mel_spec.logmel_ragged(waves.cuda(non_blocking=True), lens)
        return x.unsqueeze(1), lens_dev
