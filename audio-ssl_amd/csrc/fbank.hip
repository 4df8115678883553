// K1b: waveform -> Kaldi fbank -> finished MAST network input, gfx950.
//
// Replaces the per-clip CPU chain of the reference's MAST loader (`extras/mast_new/mast/dataloader.py:129-130`:
// torchaudio.compliance.kaldi.fbank(htk_compat, hanning, dither 0, 25 ms / 10 ms); `:132-142` cut or zero-pad to target_length;
// `:187-202` FrequencyMasking / TimeMasking, (x - mean) / (2 std); `:105-127` the optional two-file mix) with one launch over
// the whole batch.  Kaldi's front end is not a parameter of logmel.hip: frames are win_len samples every `shift` with no centre
// padding, each frame loses its own mean, is pre-emphasised (replicate padding), windowed by a symmetric Hann, zero-padded to
// 512, and the 256 power bins below Nyquist go through an un-normalised HTK-scale bank into log(max(e, eps)).
//
// One 64-lane wave owns TWO consecutive frames of a clip at a time: both are real, so they travel as the real and the imaginary
// part of one 512-point complex transform (the wave-level radix-8 Stockham FFT of wave_fft.h, 8 points per lane) and are separated
// by the conjugate-mirror identity  Xa[k] = (Z[k] + conj Z[512-k]) / 2,  Xb[k] = (Z[k] - conj Z[512-k]) / 2i  - no twiddle in
// the split, half a 512-point transform per frame.  Cross-talk between the two frames is one rounding of the larger one
// (~1e-7 relative in amplitude), far inside the per-clip power tolerance the log-mel tests use; frames of different clips never
// share a transform.  Transform, mirror fetch (ds_bpermute), register mel rows (a lane is a mel row, two rows per lane at 128 bins)
// and the tile flush are those of wave_fft.h, shared with the persistent log-mel kernel: window, twiddles and mel rows stay in
// registers for the whole launch, the waves of a block never synchronise, and the next pair's samples are in flight while the
// current pair is transformed.
// The tail (padding, masks, normalisation) is applied to the value in the register; the default [B][1][n_mels][T] layout is
// staged through an LDS tile and leaves as 64-byte row segments, the reference's [B][T][n_mels] leaves as 256-byte rows.
// HBM roofline: 4*L bytes read + 4*n_mels*T_target bytes written per clip.
#include "wave_fft.h"

namespace {

constexpr int NFFT = 512;               // real FFT length; the complex transform of a frame pair has as many points
constexpr int PWW = 288;                // floats: 256 power bins + zero tail up to the last aligned mel chunk (252 + 4 * 8)
constexpr int OTF = 16, OTP = OTF + 1;  // frames per output tile; odd row pitch: the per-frame column writes are conflict-free
constexpr int MROWS = 128;              // mel rows a wave can own (two per lane)
constexpr int WAVE_LDS = 2 * EXW + 2 * PWW + MROWS * OTP;    // floats

struct FbankArgs {
    const float* wave; const int* lens; const int* partner; const float* lam; const float* clip_mean; const int* bands; float* out;
    int B, Lmax, win_len, shift, n_mels, taps, T;
    const float* win;        // [win_len] symmetric Hann
    const float* tw;         // [512][2] exp(-2 pi i k / 512)
    const float* melw;       // [n_mels][taps] packed non-zero run of each filterbank row
    const int* mel_start;    // [n_mels] first bin of the run
    float preemph, eps, mean, two_std, inv2std;
    int skip_norm, time_major;
};

__device__ __forceinline__ int clip_len(const FbankArgs& a, int b) { return a.lens ? min(max(a.lens[b], 0), a.Lmax) : a.Lmax; }
__device__ __forceinline__ int clip_frames(const FbankArgs& a, int len) {
    return len >= a.win_len ? min(1 + (len - a.win_len) / a.shift, a.T) : 0;       // frames that survive the cut to T
}

// Whole-clip means for the two-file mix (dataloader.py:108-109): a partner shorter than the clip is zero-padded AFTER its mean was
// removed, which leaves a step the per-frame DC removal does not cancel.
__global__ __launch_bounds__(256) void fbank_clip_mean_kernel(FbankArgs a, float* mean) {
    __shared__ double sh[16];
    const int b = blockIdx.x, len = clip_len(a, b);
    const float* x = a.wave + (long)b * a.Lmax;
    float s = 0.f;
    for (int i = threadIdx.x; i < len; i += 256) s += x[i];
    const double t = block_sum((double)s, sh);
    if (threadIdx.x == 0) mean[b] = len > 0 ? (float)(t / len) : 0.f;
}

// NCH: 16-byte chunks of a mel row (taps + 3 <= 4 NCH); MPL: mel rows per lane (1 when n_mels <= 64: the widest rows then fit in registers)
template <int NCH, int MPL, bool MIX>
__global__ __launch_bounds__(256, 2) void fbank_kernel(FbankArgs a, int P, int total_pairs) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v2* ex = reinterpret_cast<v2*>(s_dyn + wave * WAVE_LDS);
    float* pw0 = reinterpret_cast<float*>(ex + EXW);
    float* pw1 = pw0 + PWW;
    float* ot = pw1 + PWW;                                   // [128][OTP] output tile of this wave
    for (int i = 256 + lane; i < PWW; i += 64) { pw0[i] = 0.f; pw1[i] = 0.f; }

    // ---- per-lane constants
    float win[8];
    v2 tw1[8], tw2[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int i = lane + 64 * r;
        win[r] = i < a.win_len ? a.win[i] : 0.f;
    }
    wave_fft_twiddles<1>(a.tw, lane, tw1, tw2);
    MelRows<MPL, NCH> mel;
    mel.load(a.melw, a.mel_start, a.n_mels, a.taps, NFFT / 2 - 1, lane);
    const float fn = (float)a.win_len;

    // pair range of this wave (wave-uniform, scalar registers)
    const int gw = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), nw = gridDim.x * 4;
    const int p0 = (int)((long)gw * total_pairs / nw), p1 = (int)((long)(gw + 1) * total_pairs / nw);

    // raw samples of the pair's two frames: x[i] and x[i-1] (replicated at i = 0), i = lane + 64 r; zeros past the window and
    // for frames that do not exist
    auto load_pair = [&](int p, float (&xa)[8], float (&xpa)[8], float (&xb)[8], float (&xpb)[8]) {
        const int b = p / P, t = 2 * (p - b * P);
        const int len = clip_len(a, b), nv = clip_frames(a, len);
        const float* x = a.wave + (long)b * a.Lmax;
        const float* y = x;
        float lam = 1.f, oml = 0.f, mx = 0.f, my = 0.f;
        int len2 = 0;
        bool mix = false;
        if (MIX) {
            const int pb = a.partner[b];
            if (pb >= 0 && pb < a.B) { y = a.wave + (long)pb * a.Lmax; lam = a.lam[b]; oml = 1.f - lam; len2 = clip_len(a, pb); mix = true;
                if (a.clip_mean) { mx = a.clip_mean[b]; my = a.clip_mean[pb]; } }
        }
        auto sample = [&](int j) -> float {
            float s = x[j];
            if (MIX && mix) s = lam * (s - mx) + oml * (j < len2 ? y[j] - my : 0.f);
            return s;
        };
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int i = lane + 64 * r;
            xa[r] = xpa[r] = xb[r] = xpb[r] = 0.f;
            if (64 * r < a.win_len) {
                if (t < nv && i < a.win_len) { const int j = t * a.shift + i; xa[r] = sample(j); xpa[r] = sample(j - (i > 0)); }
                if (t + 1 < nv && i < a.win_len) { const int j = (t + 1) * a.shift + i; xb[r] = sample(j); xpb[r] = sample(j - (i > 0)); }
            }
        }
    };

    float nxa[8], nxpa[8], nxb[8], nxpb[8];
    if (p0 < p1) load_pair(p0, nxa, nxpa, nxb, nxpb);
    int tl = 0;                                              // column of the output tile the pair's first frame goes to
    for (int p = p0; p < p1; ++p) {
        const int b = p / P, pp = p - b * P, t = 2 * pp;
        const int nv = clip_frames(a, clip_len(a, b));
        float val[MPL][2] = {};                                       // [mel row of the lane][frame of the pair]
        if (t < nv) {
            // ---- frame means: lanes 0..31 reduce frame a, lanes 32..63 frame b
            float sa = 0.f, sb = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) { sa += nxa[r]; sb += nxb[r]; }
            float s = (lane < 32 ? sa : sb) + __shfl_xor(lane < 32 ? sb : sa, 32, 64);
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const float mua = __shfl(s, 0, 64) / fn, mub = __shfl(s, 32, 64) / fn;
            // ---- DC removal, pre-emphasis, window; frame a -> real part, frame b -> imaginary part
            v2 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float da = nxa[r] - mua, dpa = nxpa[r] - mua, db = nxb[r] - mub, dpb = nxpb[r] - mub;
                v[r] = v2{(da - a.preemph * dpa) * win[r], (db - a.preemph * dpb) * win[r]};
            }
            if (p + 1 < p1) load_pair(p + 1, nxa, nxpa, nxb, nxpb);      // the next pair's samples travel while this one is transformed
            wave_fft512(v, ex, lane, tw1, tw2);
            // ---- separate the two real spectra, bins 0..255
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const v2 zm = wave_fft_mirror(v, r, lane);
                const v2 A = v[r], Bc = v2{zm.x, -zm.y};
                const v2 S = A + Bc, D = A - Bc;
                pw0[lane + 64 * r] = 0.25f * (S.x * S.x + S.y * S.y);
                pw1[lane + 64 * r] = 0.25f * (D.x * D.x + D.y * D.y);
            }
            wave_fence();
            // ---- mel rows: aligned 16-byte chunks of the power spectra against register weights, then log(max(., eps))
#pragma unroll
            for (int q = 0; q < MPL; ++q) {
                float acc[2];
                mel.dot(q, {pw0, pw1}, acc);
                val[q][0] = logf(fmaxf(acc[0], a.eps));
                val[q][1] = t + 1 < nv ? logf(fmaxf(acc[1], a.eps)) : 0.f;
            }
            wave_fence();
        } else if (p + 1 < p1) {
            load_pair(p + 1, nxa, nxpa, nxb, nxpb);          // a pair of padding frames: nothing to transform
        }
        // ---- tail: masks, normalisation (padding and masked cells included)
        int f0 = 0, f1 = 0, m0 = 0, m1 = 0;
        if (a.bands) { f0 = a.bands[4 * b]; f1 = a.bands[4 * b + 1]; m0 = a.bands[4 * b + 2]; m1 = a.bands[4 * b + 3]; }
#pragma unroll
        for (int q = 0; q < MPL; ++q) {
            const int m = lane + 64 * q;
#pragma unroll
            for (int fr = 0; fr < 2; ++fr) {
                float x = val[q][fr];
                if ((m >= f0 && m < f1) || (t + fr >= m0 && t + fr < m1)) x = 0.f;
                if (!a.skip_norm) {                           // (x - mean) / (2 std): reciprocal multiply plus one Newton correction of the quotient
                    const float d = x - a.mean, quo = d * a.inv2std;
                    x = __builtin_fmaf(__builtin_fmaf(-quo, a.two_std, d), a.inv2std, quo);
                }
                if (a.time_major) {
                    if (t + fr < a.T && m < a.n_mels) a.out[((long)b * a.T + t + fr) * a.n_mels + m] = x;
                } else {
                    ot[m * OTP + tl + fr] = x;
                }
            }
        }
        if (a.time_major) continue;
        wave_fence();
        // ---- flush the tile when it is full, at the end of a clip and at the end of the run: frames t - tl .. t + 1 of clip b
        //      (an odd T ends on a half pair: columns past T stay behind)
        if (tl + 2 == OTF || pp == P - 1 || p == p1 - 1) {
            const int t0 = t - tl;
            wave_tile_flush<OTF, MROWS>(ot, a.out + (long)b * a.n_mels * a.T + t0, min(tl + 2, a.T - t0), a.n_mels, a.T, lane);
            wave_fence();
            tl = 0;
        } else {
            tl += 2;
        }
    }
}

}  // namespace

extern "C" int audiossl_fbank_fwd(const float* wave, const int* lens, const int* partner, const float* lam, float* clip_mean,
                                  const int* bands, const int* bands_host, float* out, int B, int Lmax, int win_len, int shift, int n_fft,
                                  int n_mels, int taps, int T_target, const float* win, const float* tw, const float* melw,
                                  const int* mel_start, float preemph, float eps_log, float mean, float std, int skip_norm,
                                  int time_major, void* stream) {
    ASSL_REQUIRE(wave && out && win && tw && melw && mel_start);
    ASSL_REQUIRE(n_fft == NFFT);                               // the transform is specialised for Kaldi's padded 25 ms window at 16 kHz
    ASSL_REQUIRE(win_len > NFFT / 2 && win_len <= NFFT);
    ASSL_REQUIRE(B > 0 && Lmax > 0 && shift > 0 && T_target > 0);
    ASSL_REQUIRE(n_mels > 0 && n_mels <= MROWS && taps > 0 && taps <= 29);
    ASSL_REQUIRE(taps <= 21 || n_mels <= 64);                  // a row and its alignment slack: 4 or 6 chunks of 4 bins at two rows per lane, 8 at one
    ASSL_REQUIRE((partner == nullptr) == (lam == nullptr));
    ASSL_REQUIRE(!clip_mean || partner);
    ASSL_REQUIRE(skip_norm || (std > 0.f && mean == mean));
    ASSL_REQUIRE(!bands_host || bands);
    if (bands_host)
        for (int b = 0; b < B; ++b) {
            const int* q = bands_host + 4 * b;
            ASSL_REQUIRE(0 <= q[0] && q[0] <= q[1] && q[1] <= n_mels && 0 <= q[2] && q[2] <= q[3] && q[3] <= T_target);
        }
    const int P = (T_target + 1) / 2;
    const long total = (long)B * P;
    ASSL_REQUIRE(total < (1l << 30));
    FbankArgs a{wave, lens, partner, lam, clip_mean, bands, out, B, Lmax, win_len, shift, n_mels, taps, T_target, win, tw, melw, mel_start,
                preemph, eps_log, mean, 2.f * std, skip_norm ? 1.f : 1.f / (2.f * std), skip_norm, time_major};
    const int blocks = (int)min((long)512, (total + 3) / 4);  // two workgroups per CU
    const size_t lds = sizeof(float) * 4 * WAVE_LDS;
    const dim3 g(blocks), t(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (clip_mean) hipLaunchKernelGGL(fbank_clip_mean_kernel, dim3(B), dim3(256), 0, s, a, clip_mean);
#define FBANK_LAUNCH(NCH, MPL) \
    do { if (partner) hipLaunchKernelGGL((fbank_kernel<NCH, MPL, true>), g, t, lds, s, a, P, (int)total); \
         else         hipLaunchKernelGGL((fbank_kernel<NCH, MPL, false>), g, t, lds, s, a, P, (int)total); } while (0)
    if (taps + 3 <= 16) FBANK_LAUNCH(4, 2);
    else if (taps + 3 <= 24) FBANK_LAUNCH(6, 2);
    else FBANK_LAUNCH(8, 1);
#undef FBANK_LAUNCH
    ASSL_LAUNCH_CHECK();
}
