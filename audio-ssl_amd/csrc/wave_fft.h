// The wave-level 512-point FFT front end shared by logmel.hip (logmel2_kernel) and fbank.hip (fbank_kernel), gfx950.
//
// One 64-lane wave owns one 512-point complex transform, 8 points per lane, as a Stockham radix-8 FFT: pass 0 straight from
// registers, two exchanges through the wave's own padded float2 LDS buffer.  Waves are independent: no workgroup barrier, only
// compiler fences (LDS is in-order per wave).  Complex values travel as float2 (packed fp32 math, 8-byte LDS accesses).  What a
// real-input user needs next is here too: the conjugate-mirror bin Z[512 - k] from ds_bpermute instead of a third exchange, the
// mel rows of a lane as register weights against aligned 16-byte chunks of a power spectrum in LDS (a lane is a mel row), and
// the flush of the odd-pitch LDS tile that collects a wave's results as row segments.  The block kernel of logmel.hip
// (logmel_kernel) uses only the complex helpers and dft8v.
#pragma once
#include "common.h"

namespace {

typedef float v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2 cmulv(v2 a, v2 b) { return v2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ v2 mulmi(v2 a) { return v2{a.y, -a.x}; }     // * (-i)
// 8-point forward DFT, natural order in / out.
__device__ __forceinline__ void dft8v(v2* v) {
    const float s = 0.70710678118654752440f;
    v2 a0 = v[0] + v[4], a1 = v[0] - v[4];
    v2 a2 = v[2] + v[6], a3 = mulmi(v[2] - v[6]);
    v2 a4 = v[1] + v[5], a5 = v[1] - v[5];
    v2 a6 = v[3] + v[7], a7 = mulmi(v[3] - v[7]);
    v2 b0 = a0 + a2, b2 = a0 - a2, b1 = a1 + a3, b3 = a1 - a3;
    v2 b4 = a4 + a6, b6 = mulmi(a4 - a6);
    v2 t5 = a5 + a7, t7 = a5 - a7;
    v2 b5 = v2{(t5.x + t5.y) * s, (t5.y - t5.x) * s};          // * e^{-i pi/4}
    v2 b7 = v2{(t7.y - t7.x) * s, (-t7.x - t7.y) * s};         // * e^{-3i pi/4}
    v[0] = b0 + b4; v[4] = b0 - b4;
    v[1] = b1 + b5; v[5] = b1 - b5;
    v[2] = b2 + b6; v[6] = b2 - b6;
    v[3] = b3 + b7; v[7] = b3 - b7;
}
__device__ __forceinline__ int pidx(int a) { return a + (a >> 3); }                 // padded exchange index: 8-byte accesses stay conflict-free
__device__ __forceinline__ void wave_fence() { asm volatile("" ::: "memory"); }     // LDS is in-order per wave: only the compiler must not reorder

constexpr int EXW = 576;                // float2 exchange buffer of a wave (512 + 512 / 8 padding)

// Per-lane twiddles of passes 1 and 2 from a table tw[512 * S] = exp(-2 pi i k / (512 S)): tw1 = W_64^{r (lane & 7)}, tw2 = W_512^{r lane}.
template <int S>
__device__ __forceinline__ void wave_fft_twiddles(const float* tw, int lane, v2 (&tw1)[8], v2 (&tw2)[8]) {
    const v2* twt = reinterpret_cast<const v2*>(tw);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        tw1[r] = twt[8 * S * r * (lane & 7)];
        tw2[r] = twt[S * r * lane];
    }
}

// z[lane + 64 r] in v[r] -> Z[lane + 64 r] in v[r], through the wave's exchange buffer ex[EXW].
__device__ __forceinline__ void wave_fft512(v2 (&v)[8], v2* ex, int lane, const v2 (&tw1)[8], const v2 (&tw2)[8]) {
    const int j0 = (lane >> 3) * 64 + (lane & 7);
    // ---- pass 0 (Ns = 1)
    dft8v(v);
    wave_fence();
#pragma unroll
    for (int r = 0; r < 8; ++r) ex[pidx(8 * lane + r)] = v[r];
    wave_fence();
    // ---- pass 1 (Ns = 8)
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = ex[pidx(lane + 64 * r)];
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmulv(v[r], tw1[r]);
    dft8v(v);
    wave_fence();
#pragma unroll
    for (int r = 0; r < 8; ++r) ex[pidx(j0 + 8 * r)] = v[r];
    wave_fence();
    // ---- pass 2 (Ns = 64)
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = ex[pidx(lane + 64 * r)];
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmulv(v[r], tw2[r]);
    dft8v(v);
}

// Z[(512 - k) & 511] for k = lane + 64 r: it sits in lane 64 - lane, register 7 - r (lane 0: its own register (8 - r) & 7).
__device__ __forceinline__ v2 wave_fft_mirror(const v2 (&v)[8], int r, int lane) {
    const int mirror = ((64 - lane) & 63) * 4;               // ds_bpermute source lane (bytes)
    const v2 own = v[(8 - r) & 7], oth = v[7 - r];
    v2 zm;
    zm.x = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(oth.x)));
    zm.y = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(oth.y)));
    return lane == 0 ? own : zm;
}

// The mel rows lane + 64 q of a lane: NCH aligned 16-byte chunks of register weights per row (taps + 3 <= 4 NCH) and the bin
// the first chunk starts at.  The spectrum buffer is zero from its last bin up to the end of the last chunk a row can reach.
template <int MPL, int NCH>
struct MelRows {
    float w[MPL][4 * NCH];
    int at[MPL];
    // melw [n_mels][taps] packed non-zero runs, mel_start [n_mels] their first bins, clamped to [0, last_bin]
    __device__ __forceinline__ void load(const float* melw, const int* mel_start, int n_mels, int taps, int last_bin, int lane) {
#pragma unroll
        for (int q = 0; q < MPL; ++q) {
            const int m = lane + 64 * q;
            const int st = m < n_mels ? min(max(mel_start[m], 0), last_bin) : 0;
            at[q] = st & ~3;
#pragma unroll
            for (int j = 0; j < 4 * NCH; ++j) {
                const int i = at[q] + j - st;
                w[q][j] = (m < n_mels && i >= 0 && i < taps) ? melw[m * taps + i] : 0.f;
            }
        }
    }
    // acc[s] = row q against the spectrum pw[s]: four products summed per chunk, chunks accumulated in order; the NS spectra
    // advance chunk by chunk together, so a chunk's weights serve all of them while they are at hand
    template <int NS>
    __device__ __forceinline__ void dot(int q, const float* const (&pw)[NS], float (&acc)[NS]) const {
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            f32x4 p[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) p[s] = *reinterpret_cast<const f32x4*>(pw[s] + at[q] + 4 * c);
#pragma unroll
            for (int s = 0; s < NS; ++s)
                acc[s] += w[q][4 * c] * p[s][0] + w[q][4 * c + 1] * p[s][1] + w[q][4 * c + 2] * p[s][2] + w[q][4 * c + 3] * p[s][3];
        }
    }
};

// Output staging: a wave collects up to OTF consecutive frames in an LDS tile ot[ROWS][OTF + 1] (odd pitch: the per-frame column
// writes are conflict-free) and writes the first ncols of them out as row segments, OTF lanes per mel row and 64 / OTF rows per
// store instruction: dst[row * T + col] for row < nrows.  One float per lane with lane = mel row, 4 * T bytes apart, would make
// every store instruction 64 partial-line writes.  The caller fences before it refills the tile.
template <int OTF, int ROWS>
__device__ __forceinline__ void wave_tile_flush(const float* ot, float* dst, int ncols, int nrows, int T, int lane) {
    constexpr int RPI = 64 / OTF;
    const int col = lane & (OTF - 1);
#pragma unroll 4
    for (int i = 0; i < ROWS / RPI; ++i) {
        const int row = RPI * i + lane / OTF;
        const float x = ot[row * (OTF + 1) + col];
        if (col < ncols && row < nrows) dst[(long)row * T + col] = x;
    }
}

}  // namespace
