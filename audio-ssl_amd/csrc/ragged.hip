// Ragged batches through the conv encoder in eval mode: clips of different lengths share one padded [N][Tmax] batch and every
// row of the result equals what the clip gives alone.  The log-mel kernel writes exact zeros after a
// clip's frames (csrc/logmel.hip); here are the two pieces the encoder needs after that:
//   tail_mask            rows t >= T_n >> shift of a pooled map [N][To][row] become zeros, in place (BatchNorm + ReLU made them
//                        non-zero; the next 3x3 convolution must see its own zero padding there)
//   tmean3_ragged_fwd    x_1, x_2, x_3: means over the first T_n >> 1, >> 2, >> 3 rows of the three pooled maps
//   meanmax_ragged_fwd   mean_t h and max_t h + mean_t h over the first T_n >> shift rows of h [N][Tt][D], one pass, no arg-max
// T_n = 1 + lens[n] / hop is taken on the device from the batch's one int32 `lens` (samples), so the host ships lengths once.
// Eval only: nothing here has a backward.
#include "common.h"

namespace {

__device__ __forceinline__ int ragged_rows(const int* __restrict__ lens, int n, int hop, int shift, int To) {
    return min(max((1 + lens[n] / hop) >> shift, 0), To);
}

// One workgroup column (blockIdx.y) per clip; the tail of a clip is ONE contiguous run of 16-byte vectors.  Rows below the bound
// are neither read nor written.
__global__ __launch_bounds__(256) void tail_mask_kernel(uint4* __restrict__ P, const int* __restrict__ lens, int hop, int shift, int To,
                                                        long rowvec) {
    const int n = blockIdx.y;
    const int valid = ragged_rows(lens, n, hop, shift, To);
    const long cnt = (long)(To - valid) * rowvec;
    uint4* const p = P + ((long)n * To + valid) * rowvec;
    const uint4 z = {0u, 0u, 0u, 0u};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (long)gridDim.x * 256) p[i] = z;
}

// Column sums (and maxima) over the first `rows` rows of a [rows][nv] matrix of 8-element vectors: a workgroup owns a strip of 64
// vectors, its four waves take the rows w, w + 4, ... (1 KB contiguous per wave and row for bf16) and fold through LDS in a fixed
// order.  Returns true in the lanes of wave 0 that hold a result.
template <typename T_, bool MAX>
__device__ __forceinline__ bool ragged_fold(const T_* __restrict__ P, int rows, int nv, int v, float (&s)[8], float (&m)[8]) {
    __shared__ float red[MAX ? 2 : 1][4][64][9];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool live = v < nv;
#pragma unroll
    for (int i = 0; i < 8; ++i) { s[i] = 0.f; m[i] = -INFINITY; }
    if (live) {
        const T_* p = P + (long)v * 8;
#pragma unroll 4
        for (int t = w; t < rows; t += 4) {
            const Vec8<T_> x = Vec8<T_>::load(p + (long)t * nv * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float f = x.get(i);
                s[i] += f;
                if (MAX) m[i] = fmaxf(m[i], f);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        red[0][w][lane][i] = s[i];
        if (MAX) red[MAX ? 1 : 0][w][lane][i] = m[i];
    }
    __syncthreads();
    if (w != 0 || !live) return false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s[i] = (red[0][0][lane][i] + red[0][1][lane][i]) + (red[0][2][lane][i] + red[0][3][lane][i]);
        if (MAX) m[i] = fmaxf(fmaxf(red[MAX ? 1 : 0][0][lane][i], red[MAX ? 1 : 0][1][lane][i]),
                              fmaxf(red[MAX ? 1 : 0][2][lane][i], red[MAX ? 1 : 0][3][lane][i]));
    }
    return true;
}

__device__ __forceinline__ void store8(float* __restrict__ dst, const float (&o)[8]) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
}

// blockIdx = (strip of 64 vectors, clip, layer); layer l is shifted by l + 1
struct Tmean3Ragged { const void* P[3]; float* xl[3]; int To[3], Fo[3]; };
template <typename T_>
__global__ __launch_bounds__(256) void tmean3_ragged_kernel(Tmean3Ragged a, const int* __restrict__ lens, int hop) {
    const int l = blockIdx.z, n = blockIdx.y;
    const int nv = a.Fo[l] * 8;
    if ((int)blockIdx.x * 64 >= nv) return;
    const int rows = ragged_rows(lens, n, hop, l + 1, a.To[l]);
    const int v = blockIdx.x * 64 + (threadIdx.x & 63);
    float s[8], m[8];
    if (!ragged_fold<T_, false>(static_cast<const T_*>(a.P[l]) + (long)n * a.To[l] * nv * 8, rows, nv, v, s, m)) return;
    const float inv = rows > 0 ? 1.f / (float)rows : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] *= inv;
    store8(a.xl[l] + ((long)n * nv + v) * 8, s);
}

template <typename T_>
__global__ __launch_bounds__(256) void meanmax_ragged_kernel(const T_* __restrict__ H, float* __restrict__ mean, float* __restrict__ maxmean,
                                                             const int* __restrict__ lens, int hop, int shift, int Tt, int D) {
    const int n = blockIdx.y, nv = D / 8;
    const int rows = ragged_rows(lens, n, hop, shift, Tt);
    const int v = blockIdx.x * 64 + (threadIdx.x & 63);
    float s[8], m[8];
    if (!ragged_fold<T_, true>(H + (long)n * Tt * D, rows, nv, v, s, m)) return;
    const float inv = rows > 0 ? 1.f / (float)rows : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { s[i] *= inv; m[i] = rows > 0 ? m[i] + s[i] : 0.f; }
    if (mean) store8(mean + ((long)n * nv + v) * 8, s);
    if (maxmean) store8(maxmean + ((long)n * nv + v) * 8, m);
}

}  // namespace

// P [N][To][row_elems] of `dtype`, in place: rows t >= (1 + lens[n] / hop) >> shift become zeros.  16-byte stores: P and a row are
// multiples of 16 bytes (EALIGN).
extern "C" int audiossl_tail_mask(int dtype, void* P, const int* lens, int hop, int shift, int N, int To, long row_elems, void* stream) {
    ASSL_REQUIRE(P && lens && (dtype == 0 || dtype == 1));
    ASSL_REQUIRE(N > 0 && N <= 65535 && To > 0 && row_elems > 0 && hop > 0 && shift >= 0 && shift < 31);
    const long row_bytes = row_elems * (dtype == 0 ? 4 : 2);
    if (!ASSL_ALIGNED16(P) || (row_bytes & 15)) return ASSL_EALIGN;
    const long rowvec = row_bytes / 16;
    const int gx = (int)min((long)64, max((long)1, ((long)To * rowvec + 2047) / 2048));
    hipLaunchKernelGGL(tail_mask_kernel, dim3(gx, N), dim3(256), 0, S_(stream), static_cast<uint4*>(P), lens, hop, shift, To, rowvec);
    ASSL_LAUNCH_CHECK();
}

// x_l [N][Fo_l * 64] fp32 = mean over the first (1 + lens[n] / hop) >> l rows of P_l [N][To_l][Fo_l][64] of `dtype`, l = 1, 2, 3.
extern "C" int audiossl_tmean3_ragged_fwd(int dtype, const void* P1, float* x1, int To1, int Fo1, const void* P2, float* x2, int To2,
                                          int Fo2, const void* P3, float* x3, int To3, int Fo3, const int* lens, int hop, int N,
                                          void* stream) {
    ASSL_REQUIRE(P1 && x1 && P2 && x2 && P3 && x3 && lens && (dtype == 0 || dtype == 1));
    ASSL_REQUIRE(N > 0 && N <= 65535 && hop > 0 && To1 > 0 && To2 > 0 && To3 > 0 && Fo1 > 0 && Fo2 > 0 && Fo3 > 0);
    if (!ASSL_ALIGNED16(P1) || !ASSL_ALIGNED16(P2) || !ASSL_ALIGNED16(P3) || !ASSL_ALIGNED16(x1) || !ASSL_ALIGNED16(x2) ||
        !ASSL_ALIGNED16(x3))
        return ASSL_EALIGN;
    Tmean3Ragged a{{P1, P2, P3}, {x1, x2, x3}, {To1, To2, To3}, {Fo1, Fo2, Fo3}};
    const int gx = ceil_div(max(Fo1, max(Fo2, Fo3)) * 8, 64);
    assl_dispatch(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((tmean3_ragged_kernel<T>), dim3(gx, N, 3), dim3(256), 0, S_(stream), a, lens, hop);
    });
    ASSL_LAUNCH_CHECK();
}

// H [N][Tt][D] of `dtype` -> mean [N][D] and maxmean [N][D] (max + mean), fp32, over the first (1 + lens[n] / hop) >> shift rows of
// each clip; either output may be NULL.  Any Tt (no arg-max is kept).  D % 8 == 0.
extern "C" int audiossl_meanmax_ragged_fwd(int dtype, const void* H, float* mean, float* maxmean, const int* lens, int hop, int shift,
                                           int N, int Tt, int D, void* stream) {
    ASSL_REQUIRE(H && (mean || maxmean) && lens && (dtype == 0 || dtype == 1));
    ASSL_REQUIRE(N > 0 && N <= 65535 && Tt > 0 && D > 0 && D % 8 == 0 && hop > 0 && shift >= 0 && shift < 31);
    if (!ASSL_ALIGNED16(H) || !ASSL_ALIGNED16(mean) || !ASSL_ALIGNED16(maxmean)) return ASSL_EALIGN;
    assl_dispatch(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((meanmax_ragged_kernel<T>), dim3(ceil_div(D / 8, 64), N), dim3(256), 0, S_(stream), static_cast<const T*>(H),
                           mean, maxmean, lens, hop, shift, Tt, D);
    });
    ASSL_LAUNCH_CHECK();
}
