"""Embeddings out of a checkpoint - the head of the reference's offline labeler, `compute_features`
(`extras/decar-v2/utils.py:75-112`) and the `main` of `extras/decar-v2/store_clusters.py:64-160`: load a checkpoint, run the
encoder in `model.eval()` (running BatchNorm statistics, no dropout) under `no_grad` over a file list without augmentation,
final short batch included, and collect [N, d] features in file order.

What an embedding is:
  AudioNTT2020Task6  backbone = mean over time of the [N, T', d] encoder output (what the reference's probe feeds its Linear,
                                `src/downstream/downstream_encoder.py:38-44`);
                     head     = the expert's `encoder_q` / `encoder` output: max + mean over time, and `fc` where the wrapper has one;
                     x1 x2 x3 = the time means of the three conv blocks' pooled outputs ([N, 2048 / 1024 / 512] at 64 mels), the
                                tensors DeLoRes-M puts its Barlow heads on and UnFuSeD distils into - whatever the config's
                                `return_all_layers` says.
  ASTModel           backbone = the mean over the patch tokens before `fc` (`ast_work.py:229`), base224 and mvit alike;
                     head     = the `fc` output, i.e. the module's own forward.
The token mean is `ctx.pooled` of the engines' forward: nothing an existing call returns changes.
Windows: `random` is the reference's `extract_window` draw; `center` (default) takes the centre crop / centre zero-pad, so two
runs agree; `whole` (conv encoder) embeds every clip at its own length - the encoder is convolutional in time and its embeddings
are time pools - in ragged batches whose rows equal what each clip gives alone (`Embedder.embed_ragged`).
Single GPU.
"""
import importlib

import torch
import torch.nn.functional as F

from src.utils import extract_window

WINDOWS = ("center", "random", "whole")
MIN_RAGGED = 1120                      # samples: 8 frames at hop 160 = one row after three pools (`audiossl_logmel_ragged_fwd`)
# Frames (clips x padded frames) one ragged batch may hold.  Must stay below 1,048,000: the block-2 convolution addresses its input
# through a 32-bit offset (rows * Fi * 128 < 0x7FFFFF00 with rows = N * Tmax / 2, Fi = 32).
MAX_FRAMES = 65536
LAYERS = ("backbone", "head", "x1", "x2", "x3")
CONV_LAYERS = ("x1", "x2", "x3")
_BASES = ("AudioNTT2020Task6", "ASTModel")


# ------------------------------------------------------------------------------------- windows
def center_start(n_samples, unit_length):
    """(start, left_pad) of the centre window: the crop's first sample for a long clip, the zeros in front of a short one."""
    if n_samples >= unit_length:
        return (n_samples - unit_length) // 2, 0
    return 0, (unit_length - n_samples) // 2


def take_window(wav, unit_length, window="center"):
    """1-D tensor -> [unit_length] tensor.  `random`: `extract_window` (draws from python `random` iff the clip is longer)."""
    if window == "random":
        return extract_window(wav, duration=unit_length)
    if window != "center":
        raise ValueError("take_window cuts one window: 'center' or 'random'")
    start, left = center_start(len(wav), unit_length)
    if len(wav) < unit_length:
        wav = F.pad(wav, (left, unit_length - len(wav) - left))
    return wav[start:start + unit_length]


def plan_ragged_batches(lengths, batch_size, max_frames=MAX_FRAMES, hop=160):
    """Host plan of the `whole` window.  lengths: samples per clip -> [(indices, Tmax), ...]: clips sorted by length (ties by
    index), a batch closed when it holds `batch_size` clips or when one more clip would push N * Tmax over `max_frames`; a single
    clip always fits.  Tmax: the batch's longest clip in frames (1 + n // hop), rounded up to a multiple of 8."""
    if batch_size < 1 or max_frames < 1:
        raise ValueError("batch_size and max_frames must be positive")
    order = sorted(range(len(lengths)), key=lambda i: (int(lengths[i]), i))
    plan, cur = [], []
    for i in order:
        tmax = -(-(1 + int(lengths[i]) // hop) // 8) * 8        # ascending lengths: the newcomer is the longest
        if cur and (len(cur) == batch_size or (len(cur) + 1) * tmax > max_frames):
            plan.append((cur, -(-(1 + int(lengths[cur[-1]]) // hop) // 8) * 8))
            cur = []
        cur.append(i)
    if cur:
        plan.append((cur, -(-(1 + int(lengths[cur[-1]]) // hop) // 8) * 8))
    return plan


# ------------------------------------------------------------------------------------- the model side
def _resolve(model):
    """expert | encoder wrapper | base encoder -> (wrapper, base encoder)."""
    if repr(model) in _BASES:
        return model, model
    wrapper = getattr(model, "encoder_q", None)
    if wrapper is None:
        wrapper = getattr(model, "encoder", None)
        if wrapper is None:
            raise TypeError(f"{type(model).__name__} has no encoder_q / encoder to take embeddings from")
        if repr(wrapper) in _BASES and not hasattr(model, "hparams"):
            wrapper = model                                   # `model` is itself a wrapper around a base encoder
    base = wrapper if repr(wrapper) in _BASES else getattr(wrapper, "encoder", None)
    if repr(base) not in _BASES:
        raise NotImplementedError(f"no embedding rule for a {type(base).__name__} base encoder")
    return wrapper, base


class Embedder:
    """`Embedder(expert_or_encoder, layer="backbone"|"head"|"x1"|"x2"|"x3", precision=None)`; `embedder(x)` maps a front-end
    batch [B, 1, F, T] to float32 [B, d].  layer may be a tuple / list of names: `embedder(x)` is then a dict name -> [B, d]
    from one pass.  precision: "fp32" / "bf16" for the conv encoder (None = the module's own)."""

    def __init__(self, model, layer="backbone", precision=None, input_shape=None):
        self.multi = not isinstance(layer, str)
        self.layers = tuple(layer) if self.multi else (layer,)
        if not self.layers or any(l not in LAYERS for l in self.layers) or len(set(self.layers)) != len(self.layers):
            raise ValueError(f"layer must be one of {LAYERS}, or a tuple of distinct ones")
        self.model, self.layer = model, layer
        self.wrapper, self.base = _resolve(model)
        self.kind = repr(self.base)
        if self.kind != "AudioNTT2020Task6" and any(l in CONV_LAYERS for l in self.layers):
            raise ValueError(f"layers {CONV_LAYERS} are the conv blocks of AudioNTT2020Task6; {self.kind} has none")
        self.precision = precision
        self.input_shape = input_shape
        self._front = None

    # ---- front ends (no augmentation, no masking, no mixing)
    def front_end(self):
        if self._front is None:
            if self.kind == "AudioNTT2020Task6":
                from src.dataset.downstream_dataset import DownstreamFrontEnd
                self._front = DownstreamFrontEnd()
            else:
                from src.dataset.mast_dataset import AUDIOSET_MEAN, AUDIOSET_STD, MastFrontEnd
                b = self.base
                fdim, tdim = self.input_shape or ((b.f_dim - 1) * b.cfg["fstride"] + 16, (b.t_dim - 1) * b.cfg["tstride"] + 16)
                fb = MastFrontEnd(dict(num_mel_bins=fdim, target_length=tdim, freqm=0, timem=0, mixup=0.0, mean=AUDIOSET_MEAN,
                                       std=AUDIOSET_STD, skip_norm=False)).fbank
                # the feature chain of `make_features` (run_mvit.py:107-125); called below the planner, so nothing is drawn
                self._front = lambda waves: fb(waves.cuda().float(), None, tdim, mean=AUDIOSET_MEAN, std=AUDIOSET_STD, skip_norm=False)
        return self._front

    def _base_all(self, x):
        """(x1, x2, x3, h) of the conv encoder, whatever its `return_all_layers`; the flag is put back."""
        own = self.base.return_all_layers
        self.base.return_all_layers = True
        try:
            return self.base(x)
        finally:
            self.base.return_all_layers = own

    def _forward(self, x):
        """-> {name: tensor} for self.layers.  One encoder forward serves every layer taken from the base encoder; `head` of a
        wrapper with layers of its own is the wrapper's forward."""
        out = {}
        if self.kind == "ASTModel":
            b = self.base
            y, c = b.engine_forward(b.param_dict(), b.weight_shadow(), x.float().contiguous(), b.cfg, need_ctx=True)
            for l in self.layers:
                out[l] = y if l == "head" else c.pooled
            return out
        head_is_wrapper = self.wrapper is not self.base
        if any(l != "head" or not head_is_wrapper for l in self.layers):
            if any(l in CONV_LAYERS for l in self.layers):
                x1, x2, x3, h = self._base_all(x)
                out.update({l: t for l, t in (("x1", x1), ("x2", x2), ("x3", x3)) if l in self.layers})
            else:
                h = self.base(x)
                h = h[-1] if isinstance(h, tuple) else h
            if "backbone" in self.layers:
                from src.downstream.downstream_encoder import MeanTFn
                out["backbone"] = MeanTFn.apply(h)
            if "head" in self.layers and not head_is_wrapper:
                from src.functional import MaxMeanFn
                out["head"] = MaxMeanFn.apply(h)
        if "head" in self.layers and head_is_wrapper:
            y = self.wrapper(x)
            out["head"] = y[0] if isinstance(y, tuple) else y
        return out

    def _forward_ragged(self, x, lens):
        """`_forward` for a ragged batch: x [B, 1, F, Tmax] with zeros after each clip's frames, lens int32 [B] on the device."""
        from src import engine as E
        b = self.base
        conv = any(l in CONV_LAYERS for l in self.layers)
        x1, x2, x3, h, _ = E.encoder_forward(b.param_dict(), x.float().contiguous(), b.precision, keep=None, p_drop=b.fc[2].p,
                                             train=False, update_running=False, want_layers=conv, need_bwd=False, lens=lens)
        out = {l: t for l, t in (("x1", x1), ("x2", x2), ("x3", x3)) if l in self.layers}
        mean, mm = E.ragged_pool(b.precision, h, lens, want_mean="backbone" in self.layers, want_maxmean="head" in self.layers)
        if "backbone" in self.layers:
            out["backbone"] = mean
        if "head" in self.layers:
            # what the wrapper puts after its max + mean: DELORES_M's `fc`, SLICER's instance projector, nothing elsewhere
            proj = None if self.wrapper is b else getattr(self.wrapper, "fc", None) or getattr(self.wrapper, "instance_projector", None)
            if proj is not None:
                from src.functional import LinearFn
                from src import _native as N
                mm = LinearFn.apply(mm.to(N.torch_dtype(b.precision)), proj.weight, proj.bias, False)
            out["head"] = mm
        return out

    def _in_eval(self, fn):
        """Run fn() with the model in eval mode and the embedder's precision; train flags and precision are put back."""
        mods = list(self.model.modules())
        flags = [m.training for m in mods]
        own = getattr(self.base, "precision", None)
        self.model.eval()
        if self.precision is not None and self.kind == "AudioNTT2020Task6":
            from src import _native as N
            self.base.precision = {"fp32": N.F32, "bf16": N.BF16}.get(self.precision, self.precision)
        try:
            out = {l: t.float() for l, t in fn().items()}
            return {l: out[l] for l in self.layers} if self.multi else out[self.layer]
        finally:
            if own is not None:
                self.base.precision = own
            for m, f in zip(mods, flags):
                m.training = f

    @torch.no_grad()
    def __call__(self, x):
        return self._in_eval(lambda: self._forward(x))

    @torch.no_grad()
    def embed_ragged(self, waves, lens=None):
        """Clips of different lengths in one batch, each embedded at its own length: waves [B, Lmax] float32 on the device with
        lens[b] >= 1120 samples at the head of row b (lens: int32 on the host), or a `PcmBatch` packed with align=1 (lens = its
        own).  -> float32 [B, d] (the dict for several layers); row b is what clip b gives alone.  Conv encoder, eval mode."""
        if self.kind != "AudioNTT2020Task6":
            raise ValueError(f"ragged batches need an encoder that is convolutional in time; the positional embeddings of {self.kind} "
                             "fix its input size")
        x, lens_dev = self.front_end().ragged(waves, lens)
        return self._in_eval(lambda: self._forward_ragged(x, lens_dev))


def _whole_clip(c, unit, longest):
    """A decoded clip (array / tensor / PcmClip) as the `whole` window ships it: centre-cropped to `longest` samples, centre-padded
    to `unit` when shorter (as `center` pads it; float32 then), else untouched in its own sample format."""
    n = len(c)
    if n > longest:
        start = (n - longest) // 2
        return c.window(start, longest) if hasattr(c, "window") else c[start:start + longest]
    if n < unit:
        w = torch.from_numpy(c.to_float()) if hasattr(c, "to_float") else torch.as_tensor(c)
        return take_window(w, unit, "center").numpy()
    return c


def _extract_whole(embedder, files, batch_size, unit, longest, max_frames, pcm):
    """The `whole` window: every file is read once, sorted into ragged batches by `plan_ragged_batches` and embedded at its own
    length; rows come back in file order."""
    from src.dataset.ingest import PcmBatch
    from src.dataset.upstream_dataset import load_audio
    if embedder.kind != "AudioNTT2020Task6":
        raise ValueError(f"window 'whole' needs the conv encoder; {embedder.kind} has a fixed input size")
    if unit < MIN_RAGGED or longest < unit:
        raise ValueError(f"duration must be at least {MIN_RAGGED} samples and max_duration not below it")
    if not 0 < max_frames < 1048000:
        raise ValueError("max_frames must be below 1,048,000 (32-bit offsets of the block-2 convolution)")
    clips = [_whole_clip(load_audio(f, 16000, raw=pcm), unit, longest) for f in files]
    lengths = [len(c) for c in clips]
    rows = {l: [None] * len(files) for l in embedder.layers}
    for idx, _ in plan_ragged_batches(lengths, batch_size, max_frames):
        lens = torch.tensor([lengths[i] for i in idx], dtype=torch.int32)
        lmax = lengths[idx[-1]] + lengths[idx[-1]] % 2
        if pcm:
            batch, lens_arg = PcmBatch.pack([clips[i] for i in idx], [0] * len(idx), lmax, align=1), None
        else:
            batch = torch.zeros(len(idx), lmax, dtype=torch.float32)
            for r, i in enumerate(idx):
                batch[r, :lengths[i]] = torch.as_tensor(clips[i])
            batch, lens_arg = batch.cuda(non_blocking=True), lens
        e = embedder.embed_ragged(batch, lens_arg)
        for l in embedder.layers:
            t = e[l] if embedder.multi else e
            for r, i in enumerate(idx):
                rows[l][i] = t[r]
    out = {l: torch.stack(rows[l]) for l in embedder.layers}
    return out if embedder.multi else out[embedder.layer]


@torch.no_grad()
def extract_embeddings(embedder, files, batch_size=64, window="center", duration=1.0, pcm=False, max_duration=30.0,
                       max_frames=MAX_FRAMES):
    """files: paths (WAV / .npy, any rate) -> float32 [N, d] on the device, in file order (a dict name -> [N, d] when the
    embedder takes several layers: one pass over the files).  duration in seconds.
    pcm: ship the windows in the files' own sample formats and convert on the GPU (conv encoders; `PcmBatch`).
    window="whole" (conv encoder): every clip at its own length - shorter than `duration`: centre-padded to it as `center` does,
    longer than `max_duration` seconds: centre-cropped to that - in ragged batches of at most `batch_size` clips and `max_frames`
    padded frames (`plan_ragged_batches`); only real samples are uploaded."""
    from src.dataset.upstream_dataset import load_audio
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}")
    unit = int(duration * 16000)
    front = embedder.front_end()
    pcm = bool(pcm) and embedder.kind == "AudioNTT2020Task6"
    files = list(files)
    if window == "whole":
        return _extract_whole(embedder, files, batch_size, unit, int(max_duration * 16000), max_frames, pcm)
    out = []
    for i in range(0, len(files), batch_size):
        clips = [load_audio(f, 16000, raw=pcm) for f in files[i:i + batch_size]]
        if pcm:
            from src.dataset.ingest import PcmBatch
            from src.utils.utils import window_start
            wins = []
            for c in clips:
                start = window_start(len(c), unit)[0] if window == "random" else center_start(len(c), unit)[0]
                wins.append(c.window(start, unit) if hasattr(c, "window") else c[start:start + unit])
            batch = PcmBatch.pack(wins, [0] * len(wins), unit)
        else:
            batch = torch.stack([take_window(torch.from_numpy(c) if not torch.is_tensor(c) else c, unit, window) for c in clips])
        n = len(clips)
        if embedder.kind == "ASTModel" and n % 2:            # the transformer engines take batch * tokens in multiples of 8
            batch = torch.cat([batch, batch[-1:]])
        e = embedder(front(batch))
        out.append({l: t[:n] for l, t in e.items()} if embedder.multi else e[:n])
    if embedder.multi:
        return {l: torch.cat([o[l] for o in out]) for l in embedder.layers}
    return torch.cat(out)


def load_embedder(checkpoint, upstream, config=None, layer="backbone", precision=None):
    """Checkpoint -> Embedder through `Upstream_Expert.load_from_checkpoint`, the way `load_pretrained_encoder` does it.
    config: overrides the checkpoint's (a dict, as `train_upstream.load_config` returns)."""
    try:
        mod = importlib.import_module(f"src.upstream.{upstream}.upstream_expert")
    except ModuleNotFoundError as e:
        raise ValueError(f"src/upstream/{upstream} has no Upstream_Expert to load a checkpoint with") from e
    over = {} if config is None else {"config": config}
    expert = mod.Upstream_Expert.load_from_checkpoint(checkpoint, strict=False, **over).cuda()
    shape = None
    inp = expert.config["pretrain"]["input"]
    if repr(_resolve(expert)[1]) == "ASTModel":
        shape = (inp["n_mels"], 1 + int(inp["length_wave"] * inp["sampling_rate"]) // 160)
    return Embedder(expert, layer=layer, precision=precision, input_shape=shape)
