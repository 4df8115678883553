"""GPU: `audiossl_fbank_fwd` and the MAST front end on top of it against an fp64 restatement of the documented Kaldi fbank
algorithm (torchaudio.compliance.kaldi.fbank with htk_compat, window_type='hanning', dither 0, 25 ms / 10 ms, snip_edges) fed the
same float32 filterbank table, on the inputs the log-mel tests use.

torchaudio is not available, so this is not a parity pin against it.  The bar on the raw log values is the project's log-mel bar
(tests/test_gpu_kernels.py): per clip |d exp(v)| <= 1e-5 * max(exp ref) + 1e-7."""
import random

import numpy as np
import pytest
import torch

from oracle import fill

pytestmark = pytest.mark.gpu

EPS = 1.1920929e-07
LOG_EPS = float(np.log(np.float32(EPS)))


# ------------------------------------------------------------------------------------------------ fp64 restatement
def fbank_f64(wave, banks, win_len=400, shift=160, padded=512, preemph=0.97):
    """wave [L] -> [n_frames, n_mels] float64 log mel energies; `banks` [n_mels, padded/2] is the product's float32 table."""
    wave = np.asarray(wave, dtype=np.float64)
    n = 1 + (len(wave) - win_len) // shift if len(wave) >= win_len else 0
    if n == 0:
        return np.zeros((0, banks.shape[0]))
    fr = np.stack([wave[t * shift:t * shift + win_len] for t in range(n)])
    fr = fr - fr.mean(axis=1, keepdims=True)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)                 # replicate padding
    fr = fr - preemph * prev
    fr = fr * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_len) / (win_len - 1)))
    spec = np.fft.rfft(fr, n=padded, axis=1)
    power = (spec.real ** 2 + spec.imag ** 2)[:, :padded // 2]             # the Nyquist bin has zero weight
    return np.log(np.maximum(power @ np.asarray(banks, dtype=np.float64).T, EPS))


def image_f64(wave, banks, T):
    """cut / zero-pad to T frames -> [n_mels, T] and the number of real frames."""
    fb = fbank_f64(wave, banks)
    out = np.zeros((T, banks.shape[0]))
    n = min(len(fb), T)
    out[:n] = fb[:n]
    return out.T, n


def _waves(B, L, salt):
    w = fill.uniform((B, L), salt, -0.1, 0.1)
    t = np.arange(L) / 16000.0
    w += (0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3000 * t)).astype(np.float32)
    return w


def _batch(L, salt=31):
    w = _waves(6, L, salt)
    w[4] = 0.0                 # silence
    w[5] = 1.0                 # full-scale DC
    return w


@pytest.fixture(scope="module")
def fb():
    from src import _native
    from src.dataset.mast_dataset import KaldiFbank
    _native.lib()
    assert torch.cuda.is_available()
    return KaldiFbank(128)


def check_raw(got, ref, n, what):
    """the log-mel bar on the real frames, exact zeros on the padding."""
    e_got, e_ref = np.exp(got[:, :n].astype(np.float64)), np.exp(ref[:, :n])
    if n:
        tol = 1e-5 * float(e_ref.max()) + 1e-7
        err = float(np.abs(e_got - e_ref).max())
        print(f"{what}: frames {n}  max|d exp| {err:.3e}  bar {tol:.3e}  ({err / float(e_ref.max()):.2e} of max)")
        assert err <= tol, what
    assert np.all(got[:, n:] == 0.0), what


# ------------------------------------------------------------------------------------------------ raw log values
@pytest.mark.parametrize("L,T,frames", [(16000, None, 98), (15200, None, 93), (160000, 1024, 998), (170000, 1024, 1024), (300, 16, 0)])
def test_fbank_raw_matches_fp64(fb, L, T, frames):
    w = _batch(L)
    got = fb(torch.from_numpy(w).cuda(), target_length=T).cpu().numpy()
    T = T or frames
    assert got.shape == (6, 1, 128, T)
    banks = fb.banks.numpy()
    for b in range(6):
        ref, n = image_f64(w[b], banks, T)
        assert n == frames
        check_raw(got[b, 0], ref, n, f"L={L} clip {b}")
    if frames:
        # silence and full-scale DC are log(eps) everywhere (the per-frame mean removal is exact on a constant)
        assert np.abs(got[4:, 0, :, :frames] - LOG_EPS).max() <= 1e-5
        # Kaldi's empty bin
        assert np.abs(got[:, 0, 3, :frames] - LOG_EPS).max() <= 1e-5


def test_fbank_mixed_lengths_through_lens(fb):
    lens = [160000, 16000, 300, 15200, 170000, 399, 400, 52345]
    Lmax = max(lens)
    w = _waves(len(lens), Lmax, 77)
    w[:, ::7] *= 0.1
    got = fb(torch.from_numpy(w).cuda(), lens=torch.tensor(lens), target_length=1024).cpu().numpy()
    banks = fb.banks.numpy()
    expect = [998, 98, 0, 93, 1024, 0, 1, 325]
    for b, Lb in enumerate(lens):
        ref, n = image_f64(w[b, :Lb], banks, 1024)
        assert n == expect[b]
        check_raw(got[b, 0], ref, n, f"len {Lb}")
    # many clips: more frame pairs than waves, odd target length
    B = 40
    w = _waves(B, 16000, 78)
    got = fb(torch.from_numpy(w).cuda(), target_length=97).cpu().numpy()
    assert got.shape == (B, 1, 128, 97)
    for b in (0, 1, B // 2, B - 1):
        ref, n = image_f64(w[b], banks, 97)
        check_raw(got[b, 0], ref, n, f"B=40 clip {b}")


@pytest.mark.parametrize("bins,taps", [(64, 20), (80, 16)])
def test_fbank_wider_rows_of_smaller_banks(bins, taps):
    """64 bins (20 taps: one mel row per lane, eight chunks) and 80 bins (16 taps: two rows per lane, six chunks), with and without
    the mix: the instantiations the 128-bin bank never launches."""
    from src.dataset.mast_dataset import KaldiFbank
    fbk = KaldiFbank(bins)
    assert fbk._packed.shape[1] == taps
    w = _batch(16000, 35)
    banks = fbk.banks.numpy()
    got = fbk(torch.from_numpy(w).cuda(), target_length=100).cpu().numpy()
    assert got.shape == (6, 1, bins, 100)
    for b in range(6):
        ref, n = image_f64(w[b], banks, 100)
        check_raw(got[b, 0], ref, n, f"{bins} bins clip {b}")
    got = fbk(torch.from_numpy(w).cuda(), target_length=100, partner=torch.tensor([-1] * 6), lam=torch.ones(6), time_major=True).cpu().numpy()
    for b in range(6):
        ref, n = image_f64(w[b], banks, 100)
        check_raw(got[b].T, ref, n, f"{bins} bins, mix kernel, clip {b}")
    with pytest.raises(NotImplementedError):
        KaldiFbank(40)                                            # 31 taps


# ------------------------------------------------------------------------------------------------ padding, masks, normalisation
BANDS = [[10, 30, 100, 250], [0, 0, 0, 0], [0, 128, 5, 5], [3, 3, 0, 1024], [127, 128, 1023, 1024], [0, 1, 0, 1]]


def _masked(T):
    m = np.zeros((6, 128, T), dtype=bool)
    for b, (f0, f1, t0, t1) in enumerate(BANDS):
        m[b, f0:f1, :] = True
        m[b, :, t0:t1] = True
    return m


def test_fbank_masks_are_exact_zeros_and_touch_nothing_else(fb):
    w = torch.from_numpy(_batch(160000)).cuda()
    plain = fb(w, target_length=1024).cpu().numpy()[:, 0]
    got = fb(w, target_length=1024, bands=torch.tensor(BANDS)).cpu().numpy()[:, 0]
    m = _masked(1024)
    assert np.all(got[m] == 0.0)
    assert np.array_equal(got[~m].view(np.uint32), plain[~m].view(np.uint32))
    assert np.all(plain[:, :, 998:] == 0.0)
    with pytest.raises(RuntimeError, match="EINVAL"):
        fb(w, target_length=1024, bands=torch.tensor([[0, 129, 0, 0]] * 6))
    with pytest.raises(RuntimeError, match="EINVAL"):
        fb(w, target_length=1024, bands=torch.tensor([[0, 0, 3, 1025]] * 6))


@pytest.mark.parametrize("mean,std", [(-4.2677393, 4.5689974), (0.37, 0.021)])
def test_fbank_normalisation_within_2_ulp(fb, mean, std):
    w = torch.from_numpy(_batch(160000)).cuda()
    bands = torch.tensor(BANDS)
    raw = fb(w, target_length=1024, bands=bands).cpu()
    got = fb(w, target_length=1024, bands=bands, mean=mean, std=std, skip_norm=False).cpu()
    ref = (raw - mean) / (std * 2)                              # dataloader.py:202, float32
    ulp = torch.from_numpy(np.spacing(np.maximum(np.abs(got.numpy()), np.abs(ref.numpy()))))
    worst = float(((got - ref).abs() / ulp).max())
    print("normalisation: worst difference in ulp", worst)
    assert worst <= 2.0
    m = torch.from_numpy(_masked(1024))
    cell = torch.tensor(0.0 - mean, dtype=torch.float32) / torch.tensor(std * 2, dtype=torch.float32)
    assert float((got[:, 0][m] - cell).abs().max()) <= 2.0 * float(np.spacing(np.float32(abs(float(cell)))))
    assert float((got[:, 0, :, 998:] - cell).abs().max()) <= 2.0 * float(np.spacing(np.float32(abs(float(cell)))))


def test_fbank_layouts_are_transposes(fb):
    w = torch.from_numpy(_batch(52345, 33)).cuda()
    bands = torch.tensor([[10, 30, 100, 250]] * 6)
    for T in (1024, 301):
        a = fb(w, target_length=T, bands=bands, mean=-4.2677393, std=4.5689974, skip_norm=False)
        b = fb(w, target_length=T, bands=bands, mean=-4.2677393, std=4.5689974, skip_norm=False, time_major=True)
        assert a.shape == (6, 1, 128, T) and b.shape == (6, T, 128)
        assert torch.equal(a[:, 0].transpose(1, 2).contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ two-file mix
def test_fbank_two_file_mix(fb):
    lens = [16000, 16000, 12000, 20000, 16000, 16000]
    w = _waves(6, 20000, 41)
    w[5] = 0.0
    for b, Lb in enumerate(lens):
        w[b, Lb:] = 0.25                                        # must never be read
    partner = [1, -1, 3, 2, 5, 4]                               # longer and shorter partners, silence on either side
    lam = [0.37, 1.0, 0.5, 0.61, 0.45, 0.45]
    got = fb(torch.from_numpy(w).cuda(), lens=torch.tensor(lens), target_length=128, partner=torch.tensor(partner),
             lam=torch.tensor(lam)).cpu().numpy()
    banks = fb.banks.numpy()
    for b, Lb in enumerate(lens):
        a = w[b, :Lb].astype(np.float64)
        a = a - a.mean()
        if partner[b] >= 0:
            p = w[partner[b], :lens[partner[b]]].astype(np.float64)
            p = p - p.mean()
            q = np.zeros(Lb)
            q[:min(Lb, len(p))] = p[:Lb]                        # zero-padded or cut (dataloader.py:111-119)
            l = float(np.float32(lam[b]))
            a = l * a + (1.0 - l) * q
            a = a - a.mean()
        ref, n = image_f64(a, banks, 128)
        assert n == 1 + (Lb - 400) // 160
        check_raw(got[b, 0], ref, n, f"mix clip {b}")


# ------------------------------------------------------------------------------------------------ public interface
def test_mast_front_end_feeds_the_mvit_encoder():
    from src.dataset import MastFrontEnd
    from src.encoder import ASTModel
    conf = {"num_mel_bins": 128, "target_length": 1024, "freqm": 24, "timem": 192, "mixup": 0.5, "mean": -4.2677393,
            "std": 4.5689974, "skip_norm": False, "noise": False}
    front = MastFrontEnd(conf)
    waves = [torch.from_numpy(_waves(1, L, 50 + i)[0]) for i, L in enumerate((160000, 170000, 96000))]

    def run():
        random.seed(5)
        np.random.seed(6)
        torch.manual_seed(7)
        return front(waves), front.last_plan

    x1, plan1 = run()
    x2, plan2 = run()
    assert x1.is_cuda and x1.shape == (3, 1, 128, 1024) and bool(torch.isfinite(x1).all())
    assert torch.equal(x1, x2) and all(torch.equal(a, b) for a, b in zip(plan1, plan2))
    partner, lam, bands = plan1
    cell = (0.0 - conf["mean"]) / (conf["std"] * 2)
    for b, (f0, f1, t0, t1) in enumerate(bands.tolist()):
        assert 0 <= f0 <= f1 <= 128 and 0 <= t0 <= t1 <= 1024
        if f1 > f0:
            assert float((x1[b, 0, f0:f1] - cell).abs().max()) < 1e-6
        if t1 > t0:
            assert float((x1[b, 0, :, t0:t1] - cell).abs().max()) < 1e-6
    assert float((x1[2, 0, :, 598:] - cell).abs().max()) < 1e-6            # 96,000 samples: 598 frames, then padding
    y = front(waves, time_major=True)
    assert y.shape == (3, 1024, 128)
    torch.manual_seed(60)
    m = ASTModel(label_dim=256, input_fdim=128, input_tdim=1024, model_size="mvit").cuda().eval()
    with torch.no_grad():
        out = m(x1)
    torch.cuda.synchronize()
    assert out.shape == (3, 256) and bool(torch.isfinite(out).all())


def test_make_features_and_norm_stats(fb):
    from src.dataset import MastFrontEnd, make_features, norm_stats
    w = _waves(4, 160000, 90)
    f = make_features(torch.from_numpy(w[0]))
    assert f.is_cuda and f.shape == (1000, 128)
    raw = fb(torch.from_numpy(w[:1]).cuda(), target_length=1000, time_major=True)[0].cpu()
    ref = (raw - (-4.2677393)) / (4.5689974 * 2)                           # run_mvit.py:124
    ulp = np.spacing(np.maximum(np.abs(f.cpu().numpy()), np.abs(ref.numpy())))
    assert float((np.abs(f.cpu().numpy() - ref.numpy()) / ulp).max()) <= 2.0
    assert make_features(torch.from_numpy(w)).shape == (4, 1000, 128)
    front = MastFrontEnd({"num_mel_bins": 128, "target_length": 1024, "freqm": 0, "timem": 0, "mixup": 0, "skip_norm": True})
    batches = [front(torch.from_numpy(w[:2]), time_major=True), front(torch.from_numpy(w[2:]), time_major=True)]
    mean, std = norm_stats(batches)
    ref_mean = float(np.mean([float(torch.mean(x.cpu())) for x in batches]))
    ref_std = float(np.mean([float(torch.std(x.cpu())) for x in batches]))
    assert abs(mean - ref_mean) <= 1e-6 * abs(ref_mean) and abs(std - ref_std) <= 1e-6 * abs(ref_std)
