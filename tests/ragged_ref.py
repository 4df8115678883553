"""The rule that makes a padded batch of clips exact, in torch on the oracle.

Clip b has len_b samples and T_b = 1 + len_b // 160 frames; the batch is padded to Tmax frames.
  1. log-mel: frames t < T_b from clip b alone (reflection at the clip's own end), frames t >= T_b exact zeros;
  2. after the pooled outputs of block 1 and block 2: rows t >= T_b >> 1 / T_b >> 2 set to zero;
  3. x1, x2, x3 = means over the first T_b >> 1, >> 2, >> 3 rows; backbone = mean of h over its first T_b >> 3 rows,
     head = max + mean over those rows.
`model` is `oracle.model.AudioNTT2020Task6` in eval mode (BatchNorm on running statistics)."""
import torch

from oracle import frontend as FE

LAYERS = ("x1", "x2", "x3", "backbone", "head")
HOP = 160


def n_frames(n_samples):
    return 1 + int(n_samples) // HOP


def padded_frames(lens):
    return -(-max(n_frames(n) for n in lens) // 8) * 8


def ragged_logmel(waves, tmax=None):
    """waves: list of 1-D float32 tensors -> [B, 1, 64, Tmax]: each clip's own log-mel, zeros after its frames."""
    tmax = tmax or padded_frames([len(w) for w in waves])
    out = torch.zeros(len(waves), 1, 64, tmax)
    for b, w in enumerate(waves):
        m = FE.log_mel(w)
        out[b, 0, :, :m.shape[1]] = m
    return out


def _mask_tail(x, frames, shift):
    """x [B, C, F, To]: columns t >= frames[b] >> shift -> 0 (where, not a product: the tail may hold anything)."""
    keep = torch.arange(x.shape[-1])[None, :] < (frames >> shift)[:, None]
    return torch.where(keep[:, None, None, :], x, torch.zeros((), dtype=x.dtype))


def _rows(x):
    """[B, C, F, T] -> [B, T, F * C] (`AudioNTT2020Task6._tmean`)."""
    x = x.permute(0, 3, 2, 1)
    B, T, D, C = x.shape
    return x.reshape(B, T, C * D)


def _mean_rows(y, rows):
    return torch.stack([y[b, :int(rows[b])].mean(0) for b in range(y.shape[0])])


@torch.no_grad()
def ragged_forward(model, x, lens):
    """x [B, 1, 64, Tmax] from `ragged_logmel`, lens: samples per clip -> {layer: [B, d]} by the rule above."""
    frames = torch.tensor([n_frames(n) for n in lens])
    assert x.shape[-1] % 8 == 0 and not model.training
    p1 = _mask_tail(model.features_1(x), frames, 1)
    p2 = _mask_tail(model.features_2(p1), frames, 2)
    p3 = model.features_3(p2)
    h = _rows(p3)
    h = torch.relu(model.fc[3](torch.relu(model.fc[0](h))))          # row by row: the tail rows are computed and ignored
    r3 = frames >> 3
    mean = _mean_rows(h, r3)
    mx = torch.stack([h[b, :int(r3[b])].max(0).values for b in range(h.shape[0])])
    return {"x1": _mean_rows(_rows(p1), frames >> 1), "x2": _mean_rows(_rows(p2), frames >> 2), "x3": _mean_rows(_rows(p3), r3),
            "backbone": mean, "head": mx + mean}


@torch.no_grad()
def alone(model, wave):
    """One clip at its own length through the oracle, nothing padded -> {layer: [d]}."""
    own = model.return_all_layers
    model.return_all_layers = True
    try:
        x1, x2, x3, h = model(FE.log_mel(wave)[None, None])
    finally:
        model.return_all_layers = own
    return {"x1": x1[0], "x2": x2[0], "x3": x3[0], "backbone": h[0].mean(0), "head": h[0].max(0).values + h[0].mean(0)}


def alone_batch(model, waves):
    each = [alone(model, w) for w in waves]
    return {l: torch.stack([e[l] for e in each]) for l in LAYERS}
