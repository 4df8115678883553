// K1: waveform -> log-mel spectrogram, gfx950.
//
// Replaces the per-clip CPU chain of the reference (`src/utils/utils.py:26-28, 43-49`:
// librosa.stft(n_fft=1024, hop) -> |X|^2 -> mel filterbank matmul -> log(. + eps)) with one launch over
// the whole batch.  One 64-lane wave owns one frame: the 1024 real samples (reflect-padded, periodic
// Hann) are packed as 512 complex points, 8 per lane, and transformed by a Stockham radix-8 FFT
// (3 passes; pass 0 straight from registers, two exchanges through padded LDS), then split into the
// 513-bin real spectrum, squared, reduced by the sparse mel rows (<=45 taps each for the default
// filterbank) held in LDS, and logged.  A 256-thread block handles 8 frames of one clip and writes an
// [n_mels][8] tile so the global stores are 32-byte runs.  That is logmel_kernel, the block kernel: it takes every shape.  Banks
// that fit its register budget go to logmel2_kernel further down, one persistent wave per run of frames on the wave-level FFT of
// wave_fft.h (shared with fbank.hip); the complex arithmetic and the 8-point DFT of both kernels come from that header.
// HBM roofline: 4*L bytes read + 4*n_mels*T bytes written per clip (89,856 B at L=16000, T=101).
#include <cstdlib>
#include "wave_fft.h"

namespace {

constexpr int NFFT = 1024;
constexpr int FPB = 8;                 // frames per block
constexpr int CPAD = 512 + 64;         // padded complex-buffer length: idx + (idx >> 3)

struct LogmelArgs {
    const float* wave; float* out;
    int B, L, T, hop, n_mels, taps;
    const float* win;        // [1024] periodic Hann
    const float* tw;         // [1024][2] exp(-2 pi i k / 1024)
    const float* melw;       // [n_mels][taps] packed non-zero run of each filterbank row
    const int* mel_start;    // [n_mels] first bin of the run
    float eps_pow, eps_log;
    int apply_log;           // 0: return the mel power (MelSpectrogramLibrosa.__call__), 1: log(mel + eps_log)
    const int* lens;         // ragged form only: [B] samples of each clip (rows are L apart, out rows T apart); else nullptr
};

__global__ __launch_bounds__(256) void logmel_kernel(LogmelArgs a) {
    __shared__ float s_tw[2 * NFFT];
    __shared__ float s_re[4][CPAD];
    __shared__ float s_im[4][CPAD];
    __shared__ float s_pw[4][516];
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];   // melw [n_mels][taps], tile [n_mels][FPB+1]
    float* s_melw = s_dyn;
    float* s_tile = s_dyn + a.n_mels * a.taps;

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * FPB;
    for (int i = threadIdx.x; i < 2 * NFFT; i += 256) s_tw[i] = a.tw[i];
    for (int i = threadIdx.x; i < a.n_mels * a.taps; i += 256) s_melw[i] = a.melw[i];
    __syncthreads();

    const float* x = a.wave + (long)b * a.L;
    float* re = s_re[w];
    float* im = s_im[w];
    float* pw = s_pw[w];

    for (int s = 0; s < FPB / 4; ++s) {
        const int f = w + 4 * s;
        const int t = min(t0 + f, a.T - 1);          // clamped duplicate keeps barriers uniform
        v2 v[8];
        // ---- pass 0 (Ns = 1): inputs z[m] = x[2m] + i x[2m+1], m = lane + 64 r
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n = 2 * (lane + 64 * r);
            int p0 = t * a.hop + n - NFFT / 2, p1 = p0 + 1;
            p0 = p0 < 0 ? -p0 : (p0 >= a.L ? 2 * (a.L - 1) - p0 : p0);
            p1 = p1 < 0 ? -p1 : (p1 >= a.L ? 2 * (a.L - 1) - p1 : p1);
            v[r].x = x[p0] * a.win[n];
            v[r].y = x[p1] * a.win[n + 1];
        }
        dft8v(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) { const int o = pidx(8 * lane + r); re[o] = v[r].x; im[o] = v[r].y; }
        __syncthreads();
        // ---- pass 1 (Ns = 8): twiddle W_64^{r k} = W_1024^{16 r k}
        {
            const int k = lane & 7;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int o = pidx(lane + 64 * r);
                const v2 z = v2{re[o], im[o]};
                const int ti = 16 * r * k;
                v[r] = cmulv(z, v2{s_tw[2 * ti], s_tw[2 * ti + 1]});
            }
            dft8v(v);
            __syncthreads();
            const int j0 = (lane >> 3) * 64 + (lane & 7);
#pragma unroll
            for (int r = 0; r < 8; ++r) { const int o = pidx(j0 + 8 * r); re[o] = v[r].x; im[o] = v[r].y; }
        }
        __syncthreads();
        // ---- pass 2 (Ns = 64): twiddle W_512^{r k} = W_1024^{2 r k}; output Z[lane + 64 r] in natural order
        {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int o = pidx(lane + 64 * r);
                const v2 z = v2{re[o], im[o]};
                const int ti = 2 * r * lane;
                v[r] = cmulv(z, v2{s_tw[2 * ti], s_tw[2 * ti + 1]});
            }
            dft8v(v);
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 8; ++r) { const int o = pidx(lane + 64 * r); re[o] = v[r].x; im[o] = v[r].y; }
        }
        __syncthreads();
        // ---- real-FFT split: X[k] = E - i W_1024^k O,  E = (Z[k] + conj Z[512-k])/2, O = (Z[k] - conj Z[512-k])/2
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k = lane + 64 * r;
            const int o2 = pidx((512 - k) & 511);
            const v2 A = v[r], Bc = v2{re[o2], -im[o2]};
            const v2 E = (A + Bc) * 0.5f, O = (A - Bc) * 0.5f;
            const v2 WO = cmulv(v2{s_tw[2 * k], s_tw[2 * k + 1]}, O);
            const v2 X = v2{E.x + WO.y, E.y - WO.x};                // E - i*WO
            pw[k] = X.x * X.x + X.y * X.y + a.eps_pow;
            if (k == 0) { const float ny = A.x - A.y; pw[512] = ny * ny + a.eps_pow; }
        }
        __syncthreads();
        // ---- sparse mel rows + log
        for (int m = lane; m < a.n_mels; m += 64) {
            const float* wrow = s_melw + m * a.taps;
            const int st = a.mel_start[m];
            float acc = 0.f;
            for (int i = 0; i < a.taps; ++i) acc += wrow[i] * pw[min(st + i, 512)];
            s_tile[m * (FPB + 1) + f] = a.apply_log ? logf(acc + a.eps_log) : acc;
        }
        __syncthreads();
    }
    // ---- [n_mels][FPB] tile -> out[b][m][t0 + f]
    for (int i = threadIdx.x; i < a.n_mels * FPB; i += 256) {
        const int m = i / FPB, f = i % FPB;
        if (t0 + f < a.T) a.out[((long)b * a.n_mels + m) * a.T + t0 + f] = s_tile[m * (FPB + 1) + f];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Second form: one PERSISTENT wave per run of frames, nothing but the samples and the results crosses HBM more than once.
// The kernel above is bound by its LDS traffic and scalar fp32 issue, not by memory (3 % of the HBM roof): every frame fetched
// 12 KB of twiddles and up to 23 KB of padded mel rows from LDS, its window from global memory, and used one fp32 lane-op per
// real multiply-add.  Here, on the wave-level FFT of wave_fft.h,
//   * window, the three twiddle sets and the wave's mel rows live in registers for the whole launch (a lane is a mel row);
//   * the conjugate-mirror operand of the real-FFT split comes from ds_bpermute instead of a third LDS exchange; no workgroup
//     barrier anywhere (waves are independent);
//   * the mel row is read as 16-byte aligned LDS chunks against register weights (13 ds_read_b128 instead of 90 ds_read_b32);
//   * interior frames load their 1,024 samples as eight coalesced float2 per lane (no reflect arithmetic).
constexpr int PWW = 576;                // floats: 513 power bins + zero tail up to the last aligned mel chunk
// Output staging (wave_tile_flush): up to OTF consecutive frames of a wave's run leave as row segments of up to OTF * 4 = 128
// contiguous bytes.  Storing each frame on its own made every store instruction 64 partial-line writes: 140 MB left the L2 per
// launch for 13.2 MB of output (PMC WRITE_SIZE, round 2).
constexpr int OTF = 32, OTP = OTF + 1;  // frames per tile; row pitch in floats
// (OTF = 16: 64-byte segments at the 404-byte row pitch of T = 101 straddle three 32-byte sectors - 23.1 MB left the L2 for 13.2 MB
// of output; at B = 512 a wave's run is 25-26 frames of one clip, so 32 columns give ONE flush of ~100-byte segments per run)

// RAGGED: clip b has lens[b] samples in a row of L and T_b = 1 + lens[b] / hop frames of its own (reflected at ITS end); the frames
// of all clips are numbered one after the other (total_frames = sum T_b), so no wave transforms a padded frame.  The wave that
// finishes a clip writes zeros over out[b][.][T_b .. T): a tail frame costs a store, not an FFT.
struct FrameCur { int b, t, Tb, Lb; };                       // clip, frame in the clip, frames and samples of that clip (wave-uniform)

template <int MPL, int NCH, bool RAGGED>
__global__ __launch_bounds__(256) void logmel2_kernel(LogmelArgs a, int total_frames) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v2* ex = reinterpret_cast<v2*>(s_dyn + wave * (2 * EXW + PWW + 64 * MPL * OTP));
    float* pw = reinterpret_cast<float*>(ex + EXW);
    float* ot = pw + PWW;                                    // [64 * MPL][OTP] output tile of this wave
    for (int i = 513 + lane; i < PWW; i += 64) pw[i] = 0.f;

    // ---- per-lane constants
    v2 win[8], tw1[8], tw2[8], tws[8];                       // tws: W_1024^k of the real-FFT split
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = 2 * (lane + 64 * r);
        win[r] = v2{a.win[n], a.win[n + 1]};
        tws[r] = reinterpret_cast<const v2*>(a.tw)[lane + 64 * r];
    }
    wave_fft_twiddles<2>(a.tw, lane, tw1, tw2);
    MelRows<MPL, NCH> mel;
    mel.load(a.melw, a.mel_start, a.n_mels, a.taps, NFFT / 2, lane);

    // frame range of this wave - wave-uniform values kept in scalar registers (readfirstlane), so the frame loop, the
    // clip / frame split and the interior-or-border choice are scalar code
    const int gw = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), nw = gridDim.x * 4;
    const int f0 = (int)((long)gw * total_frames / nw), f1 = (int)((long)(gw + 1) * total_frames / nw);
    // length and frames of clip c.b (ragged form).  The host checked its copy of lens before the launch; the clamps keep a stale
    // device copy inside the row and the output all the same
    auto enter = [&](FrameCur& c) {
        c.Lb = min(max(a.lens[c.b], NFFT), a.L);
        c.Tb = min(1 + c.Lb / a.hop, a.T);
    };
    // where frame f lies: a division for the rectangle; the ragged form walks the clips once to its first frame and steps after that
    auto locate = [&](int f) {
        if constexpr (RAGGED) {
            FrameCur c{0, f, 0, 0};
            for (;; ++c.b) {
                enter(c);
                if (c.t < c.Tb) return c;
                if (c.b == a.B - 1) { c.t = c.Tb - 1; return c; }
                c.t -= c.Tb;
            }
        } else {
            const int b = f / a.T;
            return FrameCur{b, f - b * a.T, a.T, a.L};
        }
    };
    auto step = [&](FrameCur c, int f) {                     // c is frame f - 1 -> frame f (f < total_frames)
        if constexpr (RAGGED) {
            if (++c.t == c.Tb) {
                if (c.b == a.B - 1) { --c.t; return c; }
                ++c.b; c.t = 0;
                enter(c);
            }
            return c;
        } else {
            return locate(f);
        }
    };
    // raw samples of a frame: z[m] = x[2m] + i x[2m+1], m = lane + 64 r (reflected at the clip borders)
    auto load_frame = [&](const FrameCur& c, v2 (&z)[8]) {
        const float* x = a.wave + (long)c.b * a.L;
        const int base = c.t * a.hop - NFFT / 2;
        if (base >= 0 && base + NFFT <= c.Lb) {              // interior frame: eight coalesced float2 per lane
            const v2* src = reinterpret_cast<const v2*>(x + base);
#pragma unroll
            for (int r = 0; r < 8; ++r) z[r] = src[lane + 64 * r];
        } else {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                int p0 = base + 2 * (lane + 64 * r), p1 = p0 + 1;
                p0 = p0 < 0 ? -p0 : (p0 >= c.Lb ? 2 * (c.Lb - 1) - p0 : p0);
                p1 = p1 < 0 ? -p1 : (p1 >= c.Lb ? 2 * (c.Lb - 1) - p1 : p1);
                z[r] = v2{x[p0], x[p1]};
            }
        }
    };
    v2 nxt[8];
    FrameCur cn{0, 0, 0, 0};
    if (f0 < f1) { cn = locate(f0); load_frame(cn, nxt); }
    int tl = 0;                                              // column of the output tile the current frame goes to (wave-uniform)
    for (int f = f0; f < f1; ++f) {
        const FrameCur cur = cn;
        const int b = cur.b, t = cur.t;
        v2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = nxt[r] * win[r];
        if (f + 1 < f1) { cn = step(cur, f + 1); load_frame(cn, nxt); }   // the next frame's samples travel while this frame is transformed
        wave_fft512(v, ex, lane, tw1, tw2);
        // ---- real-FFT split: X[k] = E - i W_1024^k O,  E = (Z[k] + conj Z[512-k])/2, O = (Z[k] - conj Z[512-k])/2
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const v2 zm = wave_fft_mirror(v, r, lane);
            const v2 A = v[r], Bc = v2{zm.x, -zm.y};
            const v2 E = (A + Bc) * 0.5f, O = (A - Bc) * 0.5f;
            const v2 WO = cmulv(tws[r], O);
            const v2 X = v2{E.x + WO.y, E.y - WO.x};
            pw[lane + 64 * r] = X.x * X.x + X.y * X.y + a.eps_pow;
            if (r == 0 && lane == 0) { const float ny = A.x - A.y; pw[512] = ny * ny + a.eps_pow; }
        }
        wave_fence();
        // ---- mel rows: aligned 16-byte chunks of the power spectrum against register weights, then log
#pragma unroll
        for (int q = 0; q < MPL; ++q) {
            float acc[1];
            mel.dot(q, {pw}, acc);
            ot[(lane + 64 * q) * OTP + tl] = a.apply_log ? logf(acc[0] + a.eps_log) : acc[0];
        }
        wave_fence();
        // ---- flush the tile when it is full, at the end of a clip (the next frame belongs to another clip's rows) and at the
        //      end of the run: frames t - tl .. t of clip b
        if (tl == OTF - 1 || t == cur.Tb - 1 || f == f1 - 1) {
            wave_tile_flush<OTF, 64 * MPL>(ot, a.out + (long)b * a.n_mels * a.T + t - tl, tl + 1, a.n_mels, a.T, lane);
            if constexpr (RAGGED) {
                if (t == cur.Tb - 1) {                       // the clip is done: zeros over its tail frames, row by row
                    float* const z0 = a.out + (long)b * a.n_mels * a.T;
                    for (int row = 0; row < a.n_mels; ++row)
                        for (int c = cur.Tb + lane; c < a.T; c += 64) z0[(long)row * a.T + c] = 0.f;
                }
            }
            wave_fence();
            tl = 0;
        } else {
            ++tl;
        }
    }
}

// Does the packed bank fit the persistent kernel's registers: a row and its alignment slack in 13 chunks of 4 bins at one mel
// row per lane, in 7 at two.
bool persistent_fits(int n_mels, int taps) { return n_mels <= 64 ? taps + 3 <= 4 * 13 : taps + 3 <= 4 * 7; }

// The persistent kernel over `total` frames, in the form persistent_fits chose.
template <bool RAGGED>
int launch_persistent(const LogmelArgs& a, long total, hipStream_t s) {
    const int blocks = (int)min((long)512, (total + 3) / 4);              // two workgroups per CU, ~25 frames per wave at B = 512
    const size_t lds = sizeof(float) * 4 * (2 * EXW + PWW + 64 * (a.n_mels <= 64 ? 1 : 2) * OTP);
    if (a.n_mels <= 64) {
        g_assl_last_kernel = RAGGED ? "logmel2_kernel<1, 13, true>" : "logmel2_kernel<1, 13, false>";
        hipLaunchKernelGGL((logmel2_kernel<1, 13, RAGGED>), dim3(blocks), dim3(256), lds, s, a, (int)total);
    } else {
        g_assl_last_kernel = RAGGED ? "logmel2_kernel<2, 7, true>" : "logmel2_kernel<2, 7, false>";
        hipLaunchKernelGGL((logmel2_kernel<2, 7, RAGGED>), dim3(blocks), dim3(256), lds, s, a, (int)total);
    }
    ASSL_LAUNCH_CHECK();
}

}  // namespace

extern "C" int audiossl_logmel_fwd(const float* wave, float* out, int B, int L, int T, int n_fft, int hop, int n_mels,
                                   int taps, const float* win, const float* tw, const float* melw,
                                   const int* mel_start, float eps_pow, float eps_log, int apply_log, void* stream) {
    ASSL_REQUIRE(wave && out && win && tw && melw && mel_start);
    ASSL_REQUIRE(n_fft == NFFT);                       // the FFT is specialised for the reference's n_fft=1024
    ASSL_REQUIRE(B > 0 && hop > 0 && L > NFFT / 2 && n_mels > 0 && n_mels <= 128 && taps > 0 && taps <= 513);
    ASSL_REQUIRE(T == 1 + L / hop);
    const size_t dyn = sizeof(float) * ((size_t)n_mels * taps + (size_t)n_mels * (FPB + 1));
    ASSL_REQUIRE(dyn <= 28 * 1024);
    LogmelArgs a{wave, out, B, L, T, hop, n_mels, taps, win, tw, melw, mel_start, eps_pow, eps_log, apply_log, nullptr};
    // the persistent form needs 8-byte aligned frame starts and mel rows that fit its register budget
    static const int v1_only = getenv("AUDIOSSL_LOGMEL_V1") ? atoi(getenv("AUDIOSSL_LOGMEL_V1")) : 0;
    const bool v2_ok = !v1_only && hop % 2 == 0 && L % 2 == 0 && (((uintptr_t)wave) & 7) == 0 && L >= NFFT;
    if (v2_ok && persistent_fits(n_mels, taps)) return launch_persistent<false>(a, (long)B * T, static_cast<hipStream_t>(stream));
    g_assl_last_kernel = "logmel_kernel";
    hipLaunchKernelGGL(logmel_kernel, dim3(ceil_div(T, FPB), B), dim3(256), dyn, static_cast<hipStream_t>(stream), a);
    ASSL_LAUNCH_CHECK();
}

// Ragged batch: wave [B][Lmax] with lens[b] real samples at the head of row b (what follows them is never read), out [B][n_mels][Tmax]
// with frames t < 1 + lens[b] / hop computed from clip b alone and exact zeros after them.  lens_host is the caller's host copy of
// lens: every length is checked before the launch.  Runs on the persistent kernel only.
extern "C" int audiossl_logmel_ragged_fwd(const float* wave, const int* lens, const int* lens_host, float* out, int B, int Lmax, int Tmax,
                                          int n_fft, int hop, int n_mels, int taps, const float* win, const float* tw, const float* melw,
                                          const int* mel_start, float eps_pow, float eps_log, int apply_log, void* stream) {
    ASSL_REQUIRE(wave && lens && lens_host && out && win && tw && melw && mel_start);
    ASSL_REQUIRE(n_fft == NFFT);
    ASSL_REQUIRE(B > 0 && hop > 0 && hop % 2 == 0 && Lmax > 0 && Lmax % 2 == 0 && Tmax > 0 && n_mels > 0 && n_mels <= 128 && taps > 0);
    ASSL_REQUIRE(persistent_fits(n_mels, taps));
    constexpr int MIN_LEN = 1120;      // 8 frames at hop 160: one row after three pools; > n_fft / 2, so a reflection stays inside the clip
    long total = 0;
    int longest = 0;
    for (int b = 0; b < B; ++b) {
        const int n = lens_host[b];
        ASSL_REQUIRE(n >= MIN_LEN && n <= Lmax);
        longest = max(longest, n);
        total += 1 + n / hop;
    }
    ASSL_REQUIRE(Tmax >= 1 + longest / hop && total < (1l << 31) && (long)B * Tmax < (1l << 31));
    if ((((uintptr_t)wave) & 7) != 0) return ASSL_EALIGN;                  // interior frames are read as float2
    LogmelArgs a{wave, out, B, Lmax, Tmax, hop, n_mels, taps, win, tw, melw, mel_start, eps_pow, eps_log, apply_log, lens};
    return launch_persistent<true>(a, total, static_cast<hipStream_t>(stream));
}
