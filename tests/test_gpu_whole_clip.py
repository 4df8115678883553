"""Whole-clip embeddings on the GPU: ragged batches through the log-mel front end and the conv encoder in eval mode.  Every row
of a padded batch must equal what that clip gives alone at its own length - against the oracle on each clip alone, at the bars the
rectangular path is held to (`test_logmel_matches_oracle`, `test_embeddings_of_the_conv_encoder_vs_oracle_in_eval_mode`)."""
import copy

import numpy as np
import pytest
import torch

import ragged_ref as RR
from helpers import rel_l2
from oracle import fill
from oracle import frontend as FE

pytestmark = pytest.mark.gpu

LENS = (16000, 21917, 41600, 16037, 1280)          # a multiple of the hop, odd frame counts (137, 261), the shortest clip taken
FRAMES = tuple(1 + n // 160 for n in LENS)         # (101, 137, 261, 101, 9)
TMAX = 264
HOP = 160
BARS = (("fp32", 1e-4), ("bf16", 2e-2))
FILE_LENS = (23001, 9000, 60000, 16000, 41600, 12345, 30011)      # not sorted; two shorter than the 1 s window


def _waves(lens, salt):
    return [torch.from_numpy(fill.uniform((n,), salt + i, -0.3, 0.3)
                             + 0.2 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(n) / 16000).astype(np.float32)) for i, n in enumerate(lens)]


def _padded(waves, lmax, tail=0.0):
    x = torch.full((len(waves), lmax), tail, dtype=torch.float32)
    for b, w in enumerate(waves):
        x[b, :len(w)] = w
    return x


@pytest.fixture(scope="module")
def oracle_model():
    from oracle import model as OM
    ref = OM.AudioNTT2020Task6(64, 2048, False)
    fill.fill_state_dict_(ref, seed=21)
    with torch.no_grad():                          # the non-trivial running statistics of the eval-mode embedding test
        for n, b in ref.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(torch.from_numpy(fill.uniform(tuple(b.shape), 500 + fill.salt_of(n) % 1000, -0.2, 0.2)))
            elif n.endswith("running_var"):
                b.copy_(torch.from_numpy(fill.uniform(tuple(b.shape), 501 + fill.salt_of(n) % 1000, 0.5, 1.5)))
    return ref.eval()


@pytest.fixture(scope="module")
def five(oracle_model):
    """The five clips and what the oracle gives for each alone; computed once, never written to."""
    waves = _waves(LENS, 40)
    return waves, RR.alone_batch(oracle_model, waves)


def _expert(oracle_model, cfg_s):
    from src.encoder import AudioNTT2020Task6
    from src.upstream.delores_s.upstream_expert import Upstream_Expert
    expert = Upstream_Expert(copy.deepcopy(cfg_s), base_encoder=AudioNTT2020Task6)
    expert.encoder.encoder.load_state_dict(oracle_model.state_dict())
    return expert.cuda().train()


# ---- 1. ragged log-mel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,lens,lmax,tmax", [(64, LENS, 41600, TMAX), (128, (16000, 21917, 1280), 21918, 144)])
def test_ragged_logmel_is_each_clip_alone_and_zeros_after_it(n_mels, lens, lmax, tmax):
    from src import _native as N
    from src.utils import MelSpectrogramLibrosa
    from src.utils.utils import F32_EPS, F64_EPS
    B = len(lens)
    waves = _waves(lens, 60)
    mel = MelSpectrogramLibrosa(n_mels=n_mels)
    wave = _padded(waves, lmax, tail=float("nan")).cuda()                      # nothing behind a clip may be read
    out = torch.full((B + 1, n_mels, tmax), float("nan"), device="cuda")       # one guard clip behind the output
    lens_host = np.asarray(lens, np.int32)
    lens_dev = torch.from_numpy(lens_host).cuda()
    win, tw, packed, starts = mel._tables(wave.device)
    N.call("logmel_ragged_fwd", wave, lens_dev, lens_host.ctypes.data, out, B, lmax, tmax, 1024, HOP, n_mels, packed.shape[1], win, tw,
           packed, starts, np.float32(F64_EPS).item(), F32_EPS, 1)
    got = out.cpu()
    assert bool(torch.isnan(got[B]).all()), "guard clip overwritten"
    to_mel = FE.MelSpectrogram(n_mels=n_mels)
    for b, w in enumerate(waves):
        T_b = 1 + lens[b] // HOP
        ref = FE.log_mel(w, to_mel)
        assert ref.shape == (n_mels, T_b)
        e_got, e_ref = torch.exp(got[b, :, :T_b].double()), torch.exp(ref.double())
        tol = 1e-5 * float(e_ref.max()) + 1e-7
        err = float((e_got - e_ref).abs().max())
        print(f"ragged logmel n_mels {n_mels} clip {b} ({lens[b]} samples): max |d exp| {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (b, err, tol)
        assert bool((got[b, :, T_b:] == 0.0).all()), f"clip {b}: frames after the clip are not exact zeros"
    # the wrapper: same numbers, lens shipped once
    x, ld = mel.logmel_ragged(wave, torch.tensor(lens, dtype=torch.int32), n_frames=tmax)
    assert torch.equal(x.cpu(), got[:B]) and torch.equal(ld.cpu(), torch.from_numpy(lens_host))


# ---- 2. tail mask and pools --------------------------------------------------------------------------------------------------
def _map(shape, salt, td):
    """post-ReLU-like values in `td`, exactly representable there"""
    return torch.from_numpy(fill.uniform(shape, salt, -0.5, 1.5)).clamp_min(0.0).to(td)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("td", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_tail_mask_and_ragged_pools_against_torch(td):
    from src import _native as N
    from src import engine as E
    dt = N.BF16 if td == torch.bfloat16 else N.F32
    lens = torch.tensor(LENS, dtype=torch.int32).cuda()
    nan = float("nan")
    maps = []
    for l, (To, Fo) in enumerate(((132, 32), (66, 16), (33, 8))):
        P = _map((5, To, Fo * 64), 300 + l, td)
        for b in range(5):
            P[b, FRAMES[b] >> (l + 1):] = nan
        maps.append(P)
    # the mask: zeros behind each clip's rows, the rows themselves bit for bit (blocks 1 and 2 of the encoder)
    for l in (0, 1):
        P = maps[l]
        buf = torch.full((P.numel() + 64,), nan, dtype=td, device="cuda")      # guard behind the map
        dev = buf[:P.numel()].view(P.shape)
        dev.copy_(P)
        N.call("tail_mask", dt, dev, lens, HOP, l + 1, 5, P.shape[1], P.shape[2])
        got = dev.cpu()
        assert bool(torch.isnan(buf[P.numel():]).all()), "guard overwritten"
        for b in range(5):
            r = FRAMES[b] >> (l + 1)
            assert torch.equal(_bits(got[b, :r]), _bits(P[b, :r])), (l, b)
            assert bool((got[b, r:] == 0).all()) and not bool(torch.isnan(got[b]).any()), (l, b)
    # the layer means over each clip's own rows, from maps that still hold NaN behind them
    outs = [torch.full((5, P.shape[2]), nan, device="cuda") for P in maps]
    d = [P.cuda() for P in maps]
    N.call("tmean3_ragged_fwd", dt, d[0], outs[0], 132, 32, d[1], outs[1], 66, 16, d[2], outs[2], 33, 8, lens, HOP, 5)
    for l, P in enumerate(maps):
        for b in range(5):
            want = P[b, :FRAMES[b] >> (l + 1)].double().mean(0)
            e = rel_l2(outs[l][b].cpu().double(), want)
            assert e <= 1e-6, (l, b, e)
    # mean and max + mean of h in one launch; one clip with 300 valid rows (past a uint8 arg-max), D that ends inside a strip
    hl = (16000, 21917, 383840, 16037, 1280)
    rows = [(1 + n // HOP) >> 3 for n in hl]
    assert rows == [12, 17, 300, 12, 1]
    D = 520
    H = _map((5, 300, D), 310, td)
    for b in range(5):
        H[b, rows[b]:] = nan
    mean, mm = E.ragged_pool(dt, H.cuda(), torch.tensor(hl, dtype=torch.int32).cuda())
    assert mean.dtype == mm.dtype == torch.float32 and mean.shape == mm.shape == (5, D)
    for b in range(5):
        v = H[b, :rows[b]].double()
        e_mean, e_mm = rel_l2(mean[b].cpu().double(), v.mean(0)), rel_l2(mm[b].cpu().double(), v.max(0).values + v.mean(0))
        print(f"ragged pools {td} clip {b} ({rows[b]} rows): mean {e_mean:.2e} max+mean {e_mm:.2e}")
        assert e_mean <= 1e-6 and e_mm <= 1e-6, (b, e_mean, e_mm)
    only_mean, none = E.ragged_pool(dt, H.cuda(), torch.tensor(hl, dtype=torch.int32).cuda(), want_maxmean=False)
    assert none is None and torch.equal(only_mean, mean)


# ---- 3. encoder end to end ---------------------------------------------------------------------------------------------------
def test_embed_ragged_rows_equal_each_clip_alone(five, oracle_model, cfg_s):
    from src.evaluation import Embedder
    waves, want = five
    expert = _expert(oracle_model, cfg_s)
    flags = [m.training for m in expert.modules()]
    before = {k: v.clone() for k, v in expert.state_dict().items()}
    lens = torch.tensor(LENS, dtype=torch.int32)
    clean, dirty = _padded(waves, 41600).cuda(), _padded(waves, 41600, tail=float("nan")).cuda()
    for prec, bar in BARS:
        emb = Embedder(expert, layer=RR.LAYERS, precision=prec)
        got = emb.embed_ragged(clean, lens)
        assert list(got) == list(RR.LAYERS)
        for l in RR.LAYERS:
            assert got[l].shape == want[l].shape and got[l].dtype == torch.float32 and got[l].is_cuda
            for b in range(5):
                e = rel_l2(got[l][b].cpu(), want[l][b])
                print(f"embed_ragged {prec} {l} clip {b}: rel-L2 {e:.3e} (bar {bar})")
                assert e <= bar, (prec, l, b, e)
        again = emb.embed_ragged(dirty, lens)                                  # nothing past len_b may reach a result
        for l in RR.LAYERS:
            assert torch.equal(again[l], got[l]), (prec, l)
        one = Embedder(expert, layer="head", precision=prec).embed_ragged(clean, lens)
        assert torch.equal(one, got["head"])
    assert [m.training for m in expert.modules()] == flags
    after = expert.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    with pytest.raises(RuntimeError, match="EINVAL"):                          # a clip below 8 frames is refused, not padded
        Embedder(expert, layer="backbone").embed_ragged(clean, torch.tensor((16000, 21917, 41600, 16037, 1119), dtype=torch.int32))


# ---- 4. extract_embeddings(window="whole") -----------------------------------------------------------------------------------
def _write_wavs(tmp_path, lengths, salt):
    from scipy.io import wavfile
    files, waves = [], []
    for i, L in enumerate(lengths):
        w = fill.uniform((L,), salt + i, -0.3, 0.3) + 0.2 * np.sin(2 * np.pi * (200 + 40 * i) * np.arange(L) / 16000).astype(np.float32)
        pcm = (w * 32767).astype(np.int16)
        p = str(tmp_path / f"whole{salt}_{i}.wav")
        wavfile.write(p, 16000, pcm)
        files.append(p)
        waves.append(torch.from_numpy(pcm.astype(np.float32) / 32768.0))
    return files, waves


def _center_pad(w, unit=16000):
    if len(w) >= unit:
        return w
    out = torch.zeros(unit)
    left = (unit - len(w)) // 2
    out[left:left + len(w)] = w
    return out


def test_extract_embeddings_whole_window(tmp_path, oracle_model, cfg_s):
    from src.evaluation import Embedder, extract_embeddings
    files, waves = _write_wavs(tmp_path, FILE_LENS, 700)
    want = RR.alone_batch(oracle_model, [_center_pad(w) for w in waves])       # shorter than the window: padded as `center` pads
    cut = RR.alone(oracle_model, waves[2][14000:46000])                        # the centre 2 s of the 60000-sample file
    expert = _expert(oracle_model, cfg_s)
    for prec, bar in BARS:
        emb = Embedder(expert, layer=("backbone", "head", "x2"), precision=prec)
        got = extract_embeddings(emb, files, batch_size=3, window="whole", duration=1.0)
        for l in ("backbone", "head", "x2"):
            assert got[l].shape == want[l].shape and got[l].is_cuda
            for i in range(len(files)):                                        # file order, whatever the plan sorted
                e = rel_l2(got[l][i].cpu(), want[l][i])
                assert e <= bar, (prec, l, i, e)
        again = extract_embeddings(emb, files, batch_size=3, window="whole", duration=1.0)
        assert all(torch.equal(again[l], got[l]) for l in got)
        pcm = extract_embeddings(emb, files, batch_size=3, window="whole", duration=1.0, pcm=True)
        assert all(torch.equal(pcm[l], got[l]) for l in got)
        short = extract_embeddings(emb, files, batch_size=3, window="whole", duration=1.0, max_duration=2.0)
        center = extract_embeddings(emb, files, batch_size=3, window="center", duration=1.0)
        for l in ("backbone", "head", "x2"):
            assert rel_l2(short[l][2].cpu(), cut[l]) <= bar, (prec, l)
            assert rel_l2(got[l][1].cpu(), center[l][1].cpu()) <= bar, (prec, l)       # the 9000-sample file: one padded window
    single = extract_embeddings(Embedder(expert, layer="backbone", precision="fp32"), files, batch_size=3, window="whole", max_frames=300)
    assert single.shape == (7, 2048) and rel_l2(single.cpu(), want["backbone"]) <= 1e-4


# ---- 5. the labeler ----------------------------------------------------------------------------------------------------------
def test_store_clusters_whole_window_command(tmp_path, cfg_s, capsys):
    import pandas as pd
    from src.encoder import AudioNTT2020Task6
    from src.upstream.decar_v2 import store_clusters as sc
    from src.upstream.delores_s.upstream_expert import Upstream_Expert
    expert = Upstream_Expert(copy.deepcopy(cfg_s), base_encoder=AudioNTT2020Task6)
    fill.fill_state_dict_(expert, seed=9)
    ck = expert.checkpoint()
    ck["hyper_parameters"]["config"] = expert.config
    ck["hyper_parameters"]["base_encoder"] = expert.config["pretrain"]["base_encoder"]["type"]
    ckpt = str(tmp_path / "delores_s.ckpt")
    torch.save(ck, ckpt)
    # twelve files: the labeler's k-means takes a PCA width that is a multiple of 8, and n - 1 caps the width
    files, _ = _write_wavs(tmp_path, FILE_LENS + (17000, 25000, 9500, 33000, 48000), 720)
    files_csv, out_csv = str(tmp_path / "files.csv"), str(tmp_path / "whole.csv")
    pd.DataFrame({"files": files}).to_csv(files_csv, index=False)
    np.random.seed(2)
    labels = sc.main(sc.get_args(["--checkpoint", ckpt, "--upstream", "delores_s", "--input", files_csv, "--pca", "8", "--window", "whole",
                                  "--batch_size", "5", "--k", "3", "--out", out_csv]))
    assert f"{len(files)} files, 3 clusters" in capsys.readouterr().out
    lines = open(out_csv).read().split()
    assert lines[0] == "files,label" and len(lines) == 1 + len(files)
    assert [ln.rsplit(",", 1)[0] for ln in lines[1:]] == files                 # one label per file, in order
    got = [int(ln.rsplit(",", 1)[1]) for ln in lines[1:]]
    assert got == [int(l) for l in labels] and set(got) <= {0, 1, 2}
