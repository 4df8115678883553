// K6: the 1->64 channel stem of AudioNTT2020Task6 (`src/encoder/audiontt.py:46-50, 74`):
// Conv2d(1,64,3,pad 1) + BatchNorm2d(train) + ReLU + MaxPool2d(2), forward and backward, without ever
// materialising the full-resolution 64-channel tensor (1.65 MB per view in fp32).
//
// A 3x3 convolution of a single-channel image is linear in 9 shifted copies x_tap of that image, so the
// batch statistics of every output channel follow from the 9 first and 45 second moments of the taps:
//   mean_c = w_c . S1 / n + b_c,   var_c = w_c^T Cov w_c            (moments kernel + finalize, fp64)
// and the forward is ONE pass that recomputes the conv per pooled pixel and writes only the pooled map.  In bf16 training the
// finalize is the prologue of that pass (conv1_fwd_train): two launches per view, moments and forward.
// The backward never needs dX (the input is data), and BN's correction terms are again linear in the
// same moments:
//   dW_c,tap = gamma rstd [ G_c,tap - dbeta_c/n S1_tap - dgamma_c/n * rstd (w_c . S2[:,tap] + (b_c-mean_c) S1_tap) ]
// with G = sum over pooled pixels of (routed, ReLU-gated) gradient x tap value, so it is ONE more pass.
// Layouts: image [N][F][T] fp32 (NCHW, C=1); pooled output [N][T/2][F/2][64] (time, mel, channel) in T_.
#include <cstdlib>
#include "common.h"

namespace {

constexpr int NMOM = 9 + 45;
constexpr int MOM_REPL = 16;  // replicas of the moment accumulator (`mom` scratch = MOM_REPL * 54 doubles)

__device__ __forceinline__ int tri(int a, int b) {   // index of pair (a<=b) in the packed upper triangle
    return a * 9 - a * (a - 1) / 2 + (b - a);
}

// Moment slot of one view (AUDIOSSL_CONV1_MOM_SLOT doubles): [0..53] the 54 totals, then MOM_REPL replica sets of 54.  The moments
// kernel adds into the replicas; whoever finalizes folds them in replica order and leaves the totals in [0..53] (the backward
// reads those).  The totals sit in front of the replicas, not on top of replica 0, because in the fused stem forward every
// workgroup folds the replicas while workgroup 0 writes the totals.
constexpr int MOM_SLOT = (1 + MOM_REPL) * NMOM;

// Tap moments of up to two views in one launch.  Items are (image, band of MOM_BAND rows, chunk of MOM_TC time columns); a
// workgroup belongs to one view (blockIdx.y) and walks items blockIdx.x, + gridDim.x, ...: the item (+ halo, zero outside the
// image) is staged in LDS, the NEXT item's elements are already on their way into registers while the products of this one are
// accumulated (lanes along time: conflict-free LDS reads), and the cross-lane reduction and the 54 fp64 atomics happen once per
// workgroup, not once per image.  (One workgroup per image that staged, computed, reduced and added strictly in that order was
// bound by that serial chain: 44 us per view in the step for 13 MB and 54 FMAs per pixel; a flat grid-stride loop with 9 global
// loads per pixel: 52 us.)  fp32 accumulation stays inside one lane's run, which the launcher bounds at 256 pixels.
constexpr int MOM_BAND = 16, MOM_TC = 128;
constexpr int MOM_TILE = (MOM_BAND + 2) * (MOM_TC + 2);
constexpr int MOM_PRE = (MOM_TILE + 255) / 256;                   // staged elements per thread and item
constexpr int MOM_RUN = 32;                                       // items per workgroup at most: 32 * (16 * 128 / 256) = 256 pixels per lane

typedef __attribute__((ext_vector_type(2))) float f32x2;
// index of tap pair j (taps 2j, 2j + 1; tap 9 is the constant 1) in row a of the packed accumulators: rows hold 5,5,4,4,3,3,2,2,1 pairs
constexpr int MOM_NPK = 29;
__device__ __forceinline__ constexpr int mom_pk(int a, int j) {
    int base = 0;
    for (int r = 0; r < a; ++r) base += 5 - r / 2;
    return base + (j - a / 2);
}

struct MomItem { const float* im; int f0, rows, t0, tc; };
__device__ __forceinline__ MomItem mom_item(const float* __restrict__ img, int item, int F, int T, int nband, int nchunk) {
    const int per = nband * nchunk, n = item / per, rem = item - n * per, b = rem / nchunk, ch = rem - b * nchunk;
    MomItem it;
    it.im = img + (long)n * F * T;
    it.f0 = b * MOM_BAND; it.rows = min(MOM_BAND, F - it.f0);
    it.t0 = ch * MOM_TC;  it.tc = min(MOM_TC, T - it.t0);
    return it;
}
// element i of the staged tile [(rows + 2)][tc + 2] is image element (f0 - 1 + i / ld, t0 - 1 + i % ld).  The quotient comes from
// one multiplication: i < 2,560 and ld <= 130, so (i + 0.5) / ld is at least 0.5 / 130 away from an integer - a thousand times
// the rounding error of the product.
struct MomRegs {
    float v[MOM_PRE];
    __device__ __forceinline__ void fetch(const MomItem& it, int F, int T) {
        const int ld = it.tc + 2, total = (it.rows + 2) * ld;
        const float inv = 1.f / (float)ld;
#pragma unroll
        for (int k = 0; k < MOM_PRE; ++k) {
            const int i = threadIdx.x + k * 256;
            const int r = (int)(((float)i + 0.5f) * inv), f = it.f0 - 1 + r, t = it.t0 - 1 + (i - r * ld);
            v[k] = (i < total && f >= 0 && f < F && t >= 0 && t < T) ? it.im[f * T + t] : 0.f;
        }
    }
    __device__ __forceinline__ void put(float* tile, const MomItem& it) const {
        const int total = (it.rows + 2) * (it.tc + 2);
#pragma unroll
        for (int k = 0; k < MOM_PRE; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i < total) tile[i] = v[k];
        }
    }
};

// Sums over the wave of 64 values per lane: lane l ends with the sum of v[l] in v[0].  Each step halves the values a lane
// holds - it keeps one half and hands the other to the lane `h` away - so the whole transposition is 63 exchanges, not the
// 54 x 6 of one butterfly per value.
template <int H>
__device__ __forceinline__ void wave_transpose_sum(float (&v)[64], int lane) {
    const bool up = (lane & H) != 0;
#pragma unroll
    for (int k = 0; k < H; ++k) {                                 // (constant indices: a loop over H left the array in scratch memory)
        const float send = up ? v[k] : v[k + H], keep = up ? v[k + H] : v[k];
        v[k] = keep + __shfl_xor(send, H, 64);
    }
    if constexpr (H > 1) wave_transpose_sum<H / 2>(v, lane);
}

__global__ __launch_bounds__(256, 4) void conv1_moments_kernel(const float* __restrict__ img_a, const float* __restrict__ img_b,
                                                               double* __restrict__ rep_a, double* __restrict__ rep_b,
                                                               int N, int F, int T, int nband, int nchunk) {
    __shared__ float tile[MOM_TILE];
    __shared__ float sh[4][64];
    const float* __restrict__ img = blockIdx.y ? img_b : img_a;
    double* __restrict__ rep = blockIdx.y ? rep_b : rep_a;
    const int items = N * nband * nchunk;
    // The taps are held as five aligned pairs (x0,x1) ... (x8, 1): row a of the moment matrix is x_a times the pairs from a / 2 on,
    // one packed FMA per pair - 29 per pixel for the 45 second moments and, through the constant 1, the 9 first moments (54 + 9
    // scalar operations otherwise; this kernel is bound by VALU issue and shares the CUs with the front end's log-mel).  Rows with
    // odd a carry one redundant element (a, a - 1).
    f32x2 acc2[MOM_NPK];
#pragma unroll
    for (int i = 0; i < MOM_NPK; ++i) acc2[i] = f32x2{0.f, 0.f};
    MomRegs pre;
    MomItem cur = {}, nx = {};
    int item = blockIdx.x;
    if (item < items) { cur = mom_item(img, item, F, T, nband, nchunk); pre.fetch(cur, F, T); }
    while (item < items) {
        pre.put(tile, cur);
        __syncthreads();
        const int nxt = item + gridDim.x;
        if (nxt < items) { nx = mom_item(img, nxt, F, T, nband, nchunk); pre.fetch(nx, F, T); }
        const int ld = cur.tc + 2, npix = cur.rows * cur.tc;
        const float inv = 1.f / (float)cur.tc;
        for (int p = threadIdx.x; p < npix; p += 256) {
            const int f = (int)(((float)p + 0.5f) * inv), t = p - f * cur.tc;
            const float* c = tile + f * ld + t;                   // top-left tap of pixel (f0 + f, t0 + t)
            float x[10];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) x[kh * 3 + kw] = c[kh * ld + kw];
            x[9] = 1.f;
#pragma unroll
            for (int a = 0; a < 9; ++a) {
                const f32x2 xa = {x[a], x[a]};
#pragma unroll
                for (int j = a / 2; j < 5; ++j)                   // (constant indices after unrolling: the array stays in registers)
                    acc2[mom_pk(a, j)] = __builtin_elementwise_fma(xa, f32x2{x[2 * j], x[2 * j + 1]}, acc2[mom_pk(a, j)]);
            }
        }
        __syncthreads();
        item = nxt; cur = nx;
    }
    float acc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = 0.f;
#pragma unroll
    for (int a = 0; a < 9; ++a) {
        acc[a] = acc2[mom_pk(a, 4)][1];                           // x_a * 1
#pragma unroll
        for (int b = a; b < 9; ++b) acc[9 + tri(a, b)] = acc2[mom_pk(a, b / 2)][b & 1];
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    wave_transpose_sum<32>(acc, lane);
    sh[w][lane] = acc[0];
    __syncthreads();
    if (threadIdx.x < NMOM) {
        const double v = (double)sh[0][threadIdx.x] + (double)sh[1][threadIdx.x] + (double)sh[2][threadIdx.x] +
                         (double)sh[3][threadIdx.x];
        atomicAdd(&rep[(blockIdx.x & (MOM_REPL - 1)) * NMOM + threadIdx.x], v);       // replicated: same-address atomics serialise
    }
}

// BatchNorm scale / shift / mean / rstd of the 64 stem channels from the tap moments, by the NT threads of one workgroup: fold
// the `repl` replica sets at `rep` in replica order (totals also to tot_out[0..53] when it is given), the 81 covariances, per
// (channel, tap a) the row sum_b w_b cov(a, b), then the 9 rows of a channel folded in tap order.  ONE definition for the
// stand-alone finalize kernel and the prologue of the fused stem forward: the two give the same bits from the same totals.
// Results: L.sc / L.sh always; the global vectors and the running buffers only where `publish`.
struct StemBnLds {
    double tot[NMOM], cov[81], rowv[64 * 9];
    float sc[64], sh[64];
};
struct StemBn {
    double* slot;                                                 // fused forward only: the view's moment slot
    const float *gamma, *beta;
    float *running_mean, *running_var;
    float momentum, eps;
    double count;
    float *scale, *shift, *save_mean, *save_rstd;
};
template <int NT>
__device__ __forceinline__ void stem_bn_finalize(StemBnLds& L, const double* rep, int repl, double* tot_out,
                                                 const float* __restrict__ w, const float* __restrict__ bias, const StemBn& bn,
                                                 bool publish) {
    const double count = bn.count;
    for (int i = threadIdx.x; i < NMOM; i += NT) {
        double t = 0.0;
        for (int r = 0; r < repl; ++r) t += rep[r * NMOM + i];
        L.tot[i] = t;
    }
    __syncthreads();
    if (tot_out)
        for (int i = threadIdx.x; i < NMOM; i += NT) tot_out[i] = L.tot[i];
    for (int i = threadIdx.x; i < 81; i += NT) {
        const int a = i / 9, bb = i - a * 9;
        const double s2 = L.tot[9 + (a <= bb ? tri(a, bb) : tri(bb, a))] / count;
        L.cov[i] = s2 - (L.tot[a] / count) * (L.tot[bb] / count);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 576; i += NT) {
        const int c = i / 9, a = i - c * 9;
        double r = 0.0;
        for (int bb = 0; bb < 9; ++bb) r += (double)w[c * 9 + bb] * L.cov[a * 9 + bb];
        L.rowv[i] = (double)w[c * 9 + a] * r;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 64; c += NT) {
        double mean = 0.0, var = 0.0;
        {
#pragma clang fp contract(off)                                    // w_k * S1_k is rounded before it is added (it used to pass through LDS)
            for (int k = 0; k < 9; ++k) { mean += (double)w[c * 9 + k] * L.tot[k]; var += L.rowv[c * 9 + k]; }
        }
        mean = mean / count;
        var = var < 0.0 ? 0.0 : var;
        mean += (double)bias[c];
        const double rstd = 1.0 / sqrt(var + (double)bn.eps);
        const float sc = (float)((double)bn.gamma[c] * rstd);
        const float sh = (float)((double)bn.beta[c] - mean * (double)bn.gamma[c] * rstd);
        L.sc[c] = sc;
        L.sh[c] = sh;
        if (publish) {
            bn.scale[c] = sc;
            bn.shift[c] = sh;
            bn.save_mean[c] = (float)mean;
            bn.save_rstd[c] = (float)rstd;
            if (bn.running_mean) {
                bn.running_mean[c] = (1.f - bn.momentum) * bn.running_mean[c] + bn.momentum * (float)mean;
                bn.running_var[c] = (1.f - bn.momentum) * bn.running_var[c] + bn.momentum * (float)(var * count / (count - 1.0));
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(576) void conv1_finalize_kernel(double* __restrict__ momr, const float* __restrict__ w,
                                                             const float* __restrict__ bias, StemBn bn, int repl) {
    __shared__ StemBnLds L;
    stem_bn_finalize<576>(L, momr, repl, momr, w, bias, bn, true);
}

// Stage the 4 time columns x (F+2) mel rows an (n, tp) item needs: patch[f+1][k] = img[n][f][2tp-1+k].
__device__ __forceinline__ void load_patch(float* patch, const float* __restrict__ img, int n, int tp, int F, int T) {
    const float* im = img + (long)n * F * T;
    for (int i = threadIdx.x; i < (F + 2) * 4; i += 256) {
        const int f = (i >> 2) - 1, t = 2 * tp - 1 + (i & 3);
        patch[i] = (f >= 0 && f < F && t >= 0 && t < T) ? im[f * T + t] : 0.f;
    }
}

// Register-staged variant: fetch the NEXT item's patch while the current one is being consumed.
struct PatchRegs {
    float v[2];
    __device__ __forceinline__ void fetch(const float* __restrict__ img, int n, int tp, int F, int T) {
        const float* im = img + (long)n * F * T;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = threadIdx.x + j * 256;
            const int f = (i >> 2) - 1, t = 2 * tp - 1 + (i & 3);
            v[j] = (i < (F + 2) * 4 && f >= 0 && f < F && t >= 0 && t < T) ? im[f * T + t] : 0.f;
        }
    }
    __device__ __forceinline__ void put(float* patch, int F) const {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = threadIdx.x + j * 256;
            if (i < (F + 2) * 4) patch[i] = v[j];
        }
    }
};

// conv outputs of the 2x2 pooling window at pooled mel row fp: y[p], p = 2*df + dt (torch's scan order)
__device__ __forceinline__ void conv4(const float* patch, int fp, const float* w, float bias, float* y, float (*x)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                              // rows f = 2fp-1 .. 2fp+2, one 16-byte read each
        const f32x4 row = *reinterpret_cast<const f32x4*>(patch + (2 * fp + r) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[r][k] = row[k];
    }
#pragma unroll
    for (int df = 0; df < 2; ++df)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            float s = bias;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) s += w[kh * 3 + kw] * x[df + kh][dt + kw];
            y[2 * df + dt] = s;
        }
}

template <typename T_>
__global__ __launch_bounds__(256) void conv1_fwd_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, T_* __restrict__ out,
                                                        int N, int F, int T) {
    extern __shared__ __attribute__((aligned(16))) float patch[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int To = T / 2, Fo = F / 2;
    float wr[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wr[i] = w[lane * 9 + i];
    const float b = bias[lane], sc = scale[lane], sh = shift[lane];
    PatchRegs pre;
    int item = blockIdx.x;
    if (item < N * To) { pre.fetch(img, item / To, item % To, F, T); pre.put(patch, F); }
    __syncthreads();
    for (; item < N * To; item += gridDim.x) {
        const int n = item / To, tp = item - n * To;
        const int nxt = item + gridDim.x;
        if (nxt < N * To) pre.fetch(img, nxt / To, nxt % To, F, T);
        for (int fp = wv; fp < Fo; fp += 4) {
            float y[4], x[4][4];
            conv4(patch, fp, wr, b, y, x);
            float m = fmaxf(sc * y[0] + sh, 0.f);
#pragma unroll
            for (int p = 1; p < 4; ++p) m = fmaxf(m, fmaxf(sc * y[p] + sh, 0.f));
            out[(((long)n * To + tp) * Fo + fp) * 64 + lane] = from_f32<T_>(m);
        }
        __syncthreads();
        if (nxt < N * To) pre.put(patch, F);
        __syncthreads();
    }
}

// acc[c][0..8] = G, acc[c][9] = dbeta, acc[c][10] = dgamma   (fp32 atomics, one set per block)
template <typename T_>
__global__ __launch_bounds__(256) void conv1_bwd_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const T_* __restrict__ dP,
                                                        const T_* __restrict__ dxl, float inv_To, float* __restrict__ acc,
                                                        int N, int F, int T) {
    extern __shared__ __attribute__((aligned(16))) float patch[];
    __shared__ float red[4][64][11];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int To = T / 2, Fo = F / 2;
    float wr[9], G[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { wr[i] = w[lane * 9 + i]; G[i] = 0.f; }
    const float b = bias[lane], sc = scale[lane], sh = shift[lane], mu = mean[lane], rs = rstd[lane];
    float dbeta = 0.f, dgamma = 0.f;
    PatchRegs pre;
    int item = blockIdx.x;
    if (item < N * To) { pre.fetch(img, item / To, item % To, F, T); pre.put(patch, F); }
    __syncthreads();
    for (; item < N * To; item += gridDim.x) {
        const int n = item / To, tp = item - n * To;
        const int nxt = item + gridDim.x;
        if (nxt < N * To) pre.fetch(img, nxt / To, nxt % To, F, T);
        // all of this wave's pooled gradients of the item are fetched up front (<= 8 independent loads in flight): the
        // per-pixel dependent load was the kernel's critical path (latency-bound at 0.5 TB/s)
        float gin[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int fp = wv + 4 * i;
            gin[i] = 0.f;
            if (fp < Fo) {
                gin[i] = to_f32(dP[(((long)n * To + tp) * Fo + fp) * 64 + lane]);
                if (dxl) gin[i] += to_f32(dxl[(long)n * Fo * 64 + fp * 64 + lane]) * inv_To;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int fp = wv + 4 * i;
            if (fp >= Fo) break;
            float y[4], x[4][4];
            conv4(patch, fp, wr, b, y, x);
            int best = 0;
            float m = sc * y[0] + sh;
#pragma unroll
            for (int p = 1; p < 4; ++p) { const float a = sc * y[p] + sh; if (a > m) { m = a; best = p; } }
            const float g = gin[i];
            const float da = m > 0.f ? g : 0.f;
            const float ybest = best == 0 ? y[0] : best == 1 ? y[1] : best == 2 ? y[2] : y[3];
            dbeta += da;
            dgamma += da * (ybest - mu) * rs;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float dm = (best == p) ? da : 0.f;
                const int df = p >> 1, dt = p & 1;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) G[kh * 3 + kw] += dm * x[df + kh][dt + kw];      // registers, not LDS
            }
        }
        __syncthreads();
        if (nxt < N * To) pre.put(patch, F);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) red[wv][lane][i] = G[i];
    red[wv][lane][9] = dbeta;
    red[wv][lane][10] = dgamma;
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 11; i += 256) {
        const int c = i / 11, k = i - c * 11;
        // 32 replicas of the accumulator (same-address float atomics from every workgroup serialise at the memory side)
        atomicAdd(&acc[(blockIdx.x & 31) * 704 + i], red[0][c][k] + red[1][c][k] + red[2][c][k] + red[3][c][k]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// bf16 MFMA formulation of the stem (the fp32 VALU kernels above are the validation path; they are VALU-bound: 7.5 GFLOP of
// fp32 FMAs per 512-clip step forward).  One wave owns 8 pooled mel rows of an (image, pooled time column) item = 32 conv
// pixels = one 32-row MFMA tile, ordered row = 4 * pooled_pixel + window_position, so that in the C/D map
// (row = (r & 3) + 8 * (r >> 2) + 4 * half) register r of a lane is window position r & 3 of pooled pixel 2 * (r >> 2) + half:
// BatchNorm + ReLU + the 2x2 max are in-register per lane (= channel).  K = 9 taps padded to 16: lanes of the lower half
// carry taps 0..7, the upper half tap 8 and zeros.
__device__ __forceinline__ Vec8<bf16> stem_taps(const float* patch, int f, int dt, int half) {
    Vec8<bf16> a;
    if (half == 0) {
        a.v[0] = (bf16)patch[(f + 0) * 4 + dt + 0]; a.v[1] = (bf16)patch[(f + 0) * 4 + dt + 1]; a.v[2] = (bf16)patch[(f + 0) * 4 + dt + 2];
        a.v[3] = (bf16)patch[(f + 1) * 4 + dt + 0]; a.v[4] = (bf16)patch[(f + 1) * 4 + dt + 1]; a.v[5] = (bf16)patch[(f + 1) * 4 + dt + 2];
        a.v[6] = (bf16)patch[(f + 2) * 4 + dt + 0]; a.v[7] = (bf16)patch[(f + 2) * 4 + dt + 1];
    } else {
        a = Vec8<bf16>::zero();
        a.v[0] = (bf16)patch[(f + 2) * 4 + dt + 2];
    }
    return a;
}
// weights as the B operand: B[k = tap][n = channel], lane = channel 32 j + (lane & 31), k = 8 half + jj
__device__ __forceinline__ Vec8<bf16> stem_weights(const float* w, int c, int half) {
    Vec8<bf16> b = Vec8<bf16>::zero();
    if (half == 0) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) b.v[jj] = (bf16)w[c * 9 + jj];
    } else {
        b.v[0] = (bf16)w[c * 9 + 8];
    }
    return b;
}

// TRAIN: scale / shift are not read but derived in the prologue, by every workgroup, from the view's moment slot (stem_bn_finalize
// on the LDS that the patch and the staging tile use afterwards); workgroup 0 publishes them with mean / rstd, the running
// buffers and the folded totals - the 576-thread finalize launch between the moments and this kernel is gone.
template <bool TRAIN>
__global__ __launch_bounds__(256) void conv1_fwd_mfma_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, bf16* __restrict__ out,
                                                             float* __restrict__ xl, int XS, int N, int F, int T, StemBn bn) {
    extern __shared__ __attribute__((aligned(16))) float patch[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int To = T / 2, Fo = F / 2;
    // the item's pooled output [Fo][64] is collected in LDS and written as whole 16-byte pieces (it is one contiguous run of
    // Fo * 128 bytes): straight from the accumulator layout it was 2 bytes per lane - ~820 k store instructions per launch
    bf16* const stage = reinterpret_cast<bf16*>(patch + (((F + 2) * 4 + 3) & ~3));
    Vec8<bf16> wb[2];
    float b[2], sc[2], sh[2];
    if (TRAIN) {
        StemBnLds& L = *reinterpret_cast<StemBnLds*>(patch);
        stem_bn_finalize<256>(L, bn.slot + NMOM, MOM_REPL, blockIdx.x == 0 ? bn.slot : nullptr, w, bias, bn, blockIdx.x == 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) { sc[j] = L.sc[32 * j + l31]; sh[j] = L.sh[32 * j + l31]; }
        __syncthreads();                                          // the patch goes where L was
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = 32 * j + l31;
        wb[j] = stem_weights(w, c, half);
        b[j] = bias[c];
        if (!TRAIN) { sc[j] = scale[c]; sh[j] = shift[c]; }
    }
    const int pp = l31 >> 2, df = (l31 >> 1) & 1, dt = l31 & 1;          // this lane's A row: pooled pixel pp, window (df, dt)
    PatchRegs pre;
    // items (image, pooled time column): strided over the grid - or, when the layer output x_l = mean over time of the pooled
    // map is wanted too (`audiontt.py:76-78`), XS workgroups per image walking a share of its columns each, so the column sums
    // stay in registers; each leaves its part in xl[share][N][Fo*64] and tmean3_fwd adds the parts in a fixed order (a separate
    // pass re-read the whole 105 MB map; one workgroup per image was no faster than that pass; atomics are not reproducible)
    int item, step, end;
    if (xl) {
        const int n = blockIdx.x / XS, s4 = blockIdx.x - n * XS, per = (To + XS - 1) / XS;
        item = n * To + s4 * per; step = 1; end = n * To + min(To, (s4 + 1) * per);
    } else {
        item = blockIdx.x; step = gridDim.x; end = N * To;
    }
    float xs[2][2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) xs[u][j][q] = 0.f;
    if (item < end) { pre.fetch(img, item / To, item % To, F, T); pre.put(patch, F); }
    __syncthreads();
    for (; item < end; item += step) {
        const int n = item / To, tp = item - n * To;
        const int nxt = item + step;
        if (nxt < end) pre.fetch(img, nxt / To, nxt % To, F, T);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tile = wv + 4 * u;                          // Fo <= 63: at most two 8-row tiles per wave
            if (tile * 8 >= Fo) break;
            const int fp = min(tile * 8 + pp, Fo - 1);
            const Vec8<bf16> a = stem_taps(patch, 2 * fp + df, dt, half);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, wb[j].v, acc, 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float m = 0.f;
#pragma unroll
                    for (int r3 = 0; r3 < 4; ++r3) m = fmaxf(m, sc[j] * (acc[4 * q + r3] + b[j]) + sh[j]);
                    const int fpo = tile * 8 + 2 * q + half;
                    if (fpo < Fo) {
                        const bf16 mb = (bf16)m;
                        stage[fpo * 64 + 32 * j + l31] = mb;
                        xs[u][j][q] += (float)mb;
                    }
                }
            }
        }
        __syncthreads();
        if (nxt < end) pre.put(patch, F);
        bf16* o = out + (((long)n * To + tp) * Fo) * 64;
        for (int v = threadIdx.x; v < Fo * 8; v += 256) Vec8<bf16>::load(stage + v * 8).store(o + v * 8);
        __syncthreads();
    }
    if (xl) {
        const int n = blockIdx.x / XS, s4 = blockIdx.x - n * XS;
        const float inv = 1.f / (float)To;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int fpo = (wv + 4 * u) * 8 + 2 * q + half;
                    if (fpo < Fo) {
                        xl[((long)s4 * N + n) * Fo * 64 + fpo * 64 + 32 * j + l31] = xs[u][j][q] * inv;   // this quarter's part
                    }
                }
    }
}

// Backward with the same MFMA recompute (so the arg-max of the pooling window is the forward's) and the 9 tap sums
// G[c][tap] = sum_pixels dz[pixel][c] * x_tap[pixel] as a second MFMA: A = x taps (row = tap, k = pixel), B = the routed
// gradient straight out of the accumulator registers (lane = channel, k = pixel in the register order - the A operand reads
// its pixels from the LDS patch in that same order).
// TP: type of the pooled gradient dP (fp32, or bf16 - half the bytes of the largest tensor this kernel reads); dxl is fp32
template <bool SLAB, typename TP>
__global__ __launch_bounds__(256, 3) void conv1_bwd_mfma_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const TP* __restrict__ dP,
                                                             const float* __restrict__ dxl, float inv_To, float* __restrict__ accg,
                                                             int N, int F, int T) {
    // SLAB (n_mels = 64): the item's 8 KB slab of pooled gradients [32 rows][64 ch] fp32 is DMA'd straight into LDS
    // (global_load_lds, no registers) one item ahead - with three workgroups per CU the per-lane loads it replaces left
    // ~0.6 TB/s of reads in flight.  Dynamic LDS: two slabs, then the input patch.
    extern __shared__ __attribute__((aligned(1024))) float dyn[];
    float* const patch = dyn + (SLAB ? 2 * 2048 : 0);
    __shared__ float red[4][64][11];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int To = T / 2, Fo = F / 2;
    Vec8<bf16> wb[2];
    float b[2], sc[2], sh[2], mu[2], rs[2], dbeta[2] = {0.f, 0.f}, dgamma[2] = {0.f, 0.f};
    f32x16 G[2];
    auto slab_dma = [&](int it, int slot) {
        typedef __attribute__((address_space(1))) const void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        const char* src = reinterpret_cast<const char*>(dP + (long)it * Fo * 64);   // (n, tp) items are contiguous [Fo][64] slabs
        char* dst = reinterpret_cast<char*>(dyn + slot * 2048);
#pragma unroll
        for (int k = 0; k < (int)sizeof(TP) / 2; ++k)                      // 4 KB (bf16) or 8 KB (fp32) per item: 1 KB per wave and trip
            __builtin_amdgcn_global_load_lds((gptr_t)(src + ((k * 4 + wv) * 64 + lane) * 16),
                                             (lptr_t)(dst + (k * 4 + wv) * 1024), 16, 0, 0);
    };
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = 32 * j + l31;
        wb[j] = stem_weights(w, c, half);
        b[j] = bias[c]; sc[j] = scale[c]; sh[j] = shift[c]; mu[j] = mean[c]; rs[j] = rstd[c];
#pragma unroll
        for (int r = 0; r < 16; ++r) G[j][r] = 0.f;
    }
    const int pp = l31 >> 2, df = (l31 >> 1) & 1, dt = l31 & 1;
    const int tap = l31, kh = tap / 3, kw = tap - 3 * kh;               // A2 row of this lane (taps >= 9: zero rows)
    // pooled gradients of this lane's 2 channels x 4 pooled pixels of one (item, tile)
    // dxl term (gradient of the layer-mean output, [N][Fo*64], shared by all time columns) of one (item, tile)
    const float dxs = dxl ? inv_To : 0.f;
    auto fetch_dxl = [&](int it, int tile, float (&gx)[2][4]) {
        const int n = it / To;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int fpo = min(tile * 8 + 2 * q + half, Fo - 1);
#pragma unroll
            for (int j = 0; j < 2; ++j) gx[j][q] = dxl ? dxl[(long)n * Fo * 64 + fpo * 64 + 32 * j + l31] : 0.f;   // raw: scaled at use
        }
    };
    // pooled gradients of this lane's 2 channels x 4 pooled pixels of one (item, tile)
    auto fetch_gp = [&](int it, int tile, int slot, const float (&gx)[2][4], float (&gp)[2][4]) {
        const int n = it / To, tp = it - n * To;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int fpo = tile * 8 + 2 * q + half;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float g = 0.f;
                if (fpo < Fo)
                    g = (float)(SLAB ? reinterpret_cast<const TP*>(dyn + slot * 2048)[fpo * 64 + 32 * j + l31]
                                     : dP[(((long)n * To + tp) * Fo + fpo) * 64 + 32 * j + l31]) + gx[j][q] * dxs;
                gp[j][q] = g;
            }
        }
    };
    PatchRegs pre;
    int item = blockIdx.x;
    float gp[2][4], gx[2][4], gxn[2][4];
    if (item < N * To) {
        pre.fetch(img, item / To, item % To, F, T);
        pre.put(patch, F);
        if (SLAB) { fetch_dxl(item, wv, gx); slab_dma(item, 0); }
    }
    __syncthreads();                                                    // (drains the first slab's DMA as well)
    int slot = 0;
    for (; item < N * To; item += gridDim.x, slot ^= 1) {
        const int nxt = item + gridDim.x;
        if (nxt < N * To) {
            // everything for the NEXT item is requested here and consumed after the barrier that ends this one: no
            // register-destination load is waited for in between (hipcc drains vmcnt to 0 for those, DMA included)
            pre.fetch(img, nxt / To, nxt % To, F, T);
            if (SLAB) { fetch_dxl(nxt, wv, gxn); slab_dma(nxt, slot ^ 1); }
        }
        for (int tile = wv; tile * 8 < Fo; tile += 4) {
            if (!SLAB) fetch_dxl(item, tile, gx);
            fetch_gp(item, tile, slot, gx, gp);
            const int fp = min(tile * 8 + pp, Fo - 1);
            const Vec8<bf16> a = stem_taps(patch, 2 * fp + df, dt, half);
            // x taps as the A operand of the G product: element jj of k-step st is pixel 16 st + (jj & 3) + 8 (jj >> 2) + 4 half
            // (hi + lo splitting of both operands was tried: the weight-gradient error of this flavour comes from pooling
            // windows whose arg-max differs from the fp32 convolution's, not from the rounding of the tap sums)
            Vec8<bf16> xh[2];
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                xh[st] = Vec8<bf16>::zero();
                if (tap < 9) {
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) {
                        const int pix = 16 * st + (jj & 3) + 8 * (jj >> 2) + 4 * half;
                        const int fpx = min(tile * 8 + (pix >> 2), Fo - 1), wp = pix & 3;
                        xh[st].v[jj] = (bf16)patch[(2 * fpx + (wp >> 1) + kh) * 4 + (wp & 1) + kw];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, wb[j].v, acc, 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int best = 0;
                    float ybest = acc[4 * q] + b[j];
                    float m = sc[j] * ybest + sh[j];
#pragma unroll
                    for (int r3 = 1; r3 < 4; ++r3) {
                        const float y = acc[4 * q + r3] + b[j], z = sc[j] * y + sh[j];
                        if (z > m) { m = z; best = r3; ybest = y; }
                    }
                    const float da = m > 0.f ? gp[j][q] : 0.f;
                    dbeta[j] += da;
                    dgamma[j] += da * (ybest - mu[j]) * rs[j];
#pragma unroll
                    for (int r3 = 0; r3 < 4; ++r3) acc[4 * q + r3] = (r3 == best) ? da : 0.f;          // routed gradient dz
                }
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    Vec8<bf16> gh;
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) gh.v[jj] = (bf16)acc[8 * st + jj];
                    G[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[st].v, gh.v, G[j], 0, 0, 0);
                }
            }
        }
        __syncthreads();
        if (nxt < N * To) pre.put(patch, F);
        if (SLAB) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) gx[j][q] = gxn[j][q];
        }
        __syncthreads();
    }
    // G[j][r]: row (tap) = (r & 3) + 8 (r >> 2) + 4 half, column = channel 32 j + l31
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = 32 * j + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = (r & 3) + 8 * (r >> 2) + 4 * half;
            if (t < 9) red[wv][c][t] = G[j][r];
        }
        const float db = dbeta[j] + __shfl_xor(dbeta[j], 32, 64), dg = dgamma[j] + __shfl_xor(dgamma[j], 32, 64);
        if (half == 0) { red[wv][c][9] = db; red[wv][c][10] = dg; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 11; i += 256) {
        const int c = i / 11, k = i - c * 11;
        atomicAdd(&accg[(blockIdx.x & 31) * 704 + i], red[0][c][k] + red[1][c][k] + red[2][c][k] + red[3][c][k]);
    }
}

// 704 threads: thread i folds entry i of the 32 replicas (fp64, replica order - coalesced across the workgroup; one thread per channel
// walking 11 x 32 strided loads took 12 us at the serial end of the step), then one thread per (channel, tap) finishes dW
__global__ __launch_bounds__(704) void conv1_bwd_finalize_kernel(const float* __restrict__ acc, const double* __restrict__ mom,
                                          const float* __restrict__ w, const float* __restrict__ bias,
                                          const float* __restrict__ gamma, const float* __restrict__ mean,
                                          const float* __restrict__ rstd, double count, float* dW, float* dbias,
                                          float* dgamma, float* dbeta, const float* __restrict__ gstat, float* lstat) {
    __shared__ double s11[704];                                   // [channel][9 tap sums, dbeta, dgamma]
    const int i = threadIdx.x;
    if (i < 704) {
        double t = 0.0;
        for (int r = 0; r < 32; ++r) t += (double)acc[r * 704 + i];
        s11[i] = t;
    }
    __syncthreads();
    if (lstat) {                                                  // sums only: this rank's (dbeta, dgamma)
        if (i < 64) { lstat[i] = (float)s11[i * 11 + 9]; lstat[64 + i] = (float)s11[i * 11 + 10]; }
        return;
    }
    if (i < 576) {
        const int c = i / 9, t = i - c * 9;
        // SyncBatchNorm: the two means of the BatchNorm backward are over the GLOBAL batch (gstat = all-reduced sums, count global);
        // the parameter gradients and the tap sums stay this rank's own
        const double db = gstat ? (double)gstat[c] : s11[c * 11 + 9], dg = gstat ? (double)gstat[64 + c] : s11[c * 11 + 10];
        const double rs = rstd[c], mu = mean[c], gm = gamma[c];
        double wS2 = 0.0;
        for (int a = 0; a < 9; ++a) wS2 += (double)w[c * 9 + a] * mom[9 + (a <= t ? tri(a, t) : tri(t, a))];
        const double yhat_x = rs * (wS2 + ((double)bias[c] - mu) * mom[t]);           // sum_pos yhat_c * x_tap
        const double v = gm * rs * (s11[c * 11 + t] - db / count * mom[t] - dg / count * yhat_x);
        dW[c * 9 + t] += (float)v;
    }
    if (i < 64) {
        dgamma[i] += (float)s11[i * 11 + 10];
        dbeta[i] += (float)s11[i * 11 + 9];
    }
    (void)dbias;            // d(conv bias) is identically zero under train-mode BN
}

int launch_moments(const float* img_a, const float* img_b, double* rep_a, double* rep_b, int N, int F, int T, hipStream_t s) {
    const int nband = ceil_div(F, MOM_BAND), nchunk = ceil_div(T, MOM_TC), items = N * nband * nchunk, views = img_b ? 2 : 1;
    // as many workgroups as the chip holds at four per CU, shared between the views - more only where a lane's fp32 run would
    // otherwise pass MOM_RUN items
    static const int resident = getenv("AUDIOSSL_MOM_GRID") ? atoi(getenv("AUDIOSSL_MOM_GRID")) : 1024;
    const int grid = min(items, max(max(resident / views, 1), ceil_div(items, MOM_RUN)));
    hipLaunchKernelGGL(conv1_moments_kernel, dim3(grid, views), dim3(256), 0, s, img_a, img_b, rep_a, rep_b, N, F, T, nband, nchunk);
    return hipGetLastError() == hipSuccess ? ASSL_OK : ASSL_ELAUNCH;
}

bool moments_shape_ok(int N, int F, int T) {
    return N > 0 && F >= 2 && F <= 120 && T >= 2 && (long)N * F * T < 0x7FFFFFFFL - 0x1000000L;
}

}  // namespace

extern "C" int audiossl_conv1_stats(const float* img, int N, int F, int T, const float* w, const float* bias,
                                    const float* gamma, const float* beta, float* running_mean, float* running_var,
                                    float momentum, float eps, double* mom, float* scale, float* shift,
                                    float* save_mean, float* save_rstd, void* stream) {
    ASSL_REQUIRE(img && w && bias && gamma && beta && mom && scale && shift && save_mean && save_rstd);
    ASSL_REQUIRE(moments_shape_ok(N, F, T));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ASSL_ZERO(mom, sizeof(double) * NMOM * MOM_REPL, s);
    // every workgroup ends with 54 fp64 atomics; on ONE set of 54 addresses they serialise at the memory side -
    // MOM_REPL replicas of the accumulator, folded by the finalize kernel
    if (launch_moments(img, nullptr, mom, nullptr, N, F, T, s) != ASSL_OK) return ASSL_ELAUNCH;
    const StemBn bn = {nullptr, gamma, beta, running_mean, running_var, momentum, eps, (double)((long)N * F * T),
                       scale, shift, save_mean, save_rstd};
    hipLaunchKernelGGL(conv1_finalize_kernel, dim3(1), dim3(576), 0, s, mom, w, bias, bn, MOM_REPL);
    ASSL_LAUNCH_CHECK();
}

// The same for up to two views in one launch, into moment slots the consumer finalizes (conv1_fwd_train): `mom` holds one slot of
// AUDIOSSL_CONV1_MOM_SLOT doubles per view, img_b == NULL leaves the second slot alone.
extern "C" int audiossl_conv1_moments_pair(const float* img_a, const float* img_b, int N, int F, int T, double* mom, void* stream) {
    ASSL_REQUIRE(img_a && mom && moments_shape_ok(N, F, T));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ASSL_ZERO(mom, sizeof(double) * MOM_SLOT * (img_b ? 2 : 1), s);
    return launch_moments(img_a, img_b, mom + NMOM, mom + MOM_SLOT + NMOM, N, F, T, s);
}

// ---- the same in two halves, for statistics that are exchanged between ranks in between (SyncBatchNorm of the
// DeepCluster-v2 trainer, extras/decar-v2/main.py:82): conv1_moments leaves this rank's 54 tap-moment totals in mom[0..53];
// conv1_finalize turns (all-reduced) totals and the GLOBAL element count into scale / shift / mean / rstd + running buffers.
__global__ void conv1_fold_kernel(double* __restrict__ momr) {
    __shared__ double tot[NMOM];
    const int c = threadIdx.x;
    if (c < NMOM) {
        double t = 0.0;
        for (int r = 0; r < MOM_REPL; ++r) t += momr[r * NMOM + c];
        tot[c] = t;
    }
    __syncthreads();
    if (c < NMOM) momr[c] = tot[c];
}
extern "C" int audiossl_conv1_moments(const float* img, int N, int F, int T, double* mom, void* stream) {
    ASSL_REQUIRE(img && mom && moments_shape_ok(N, F, T));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ASSL_ZERO(mom, sizeof(double) * NMOM * MOM_REPL, s);
    if (launch_moments(img, nullptr, mom, nullptr, N, F, T, s) != ASSL_OK) return ASSL_ELAUNCH;
    hipLaunchKernelGGL(conv1_fold_kernel, dim3(1), dim3(64), 0, s, mom);
    ASSL_LAUNCH_CHECK();
}
extern "C" int audiossl_conv1_finalize(double* mom_totals, const float* w, const float* bias, const float* gamma, const float* beta,
                                       float* running_mean, float* running_var, float momentum, float eps, double count,
                                       float* scale, float* shift, float* save_mean, float* save_rstd, void* stream) {
    ASSL_REQUIRE(mom_totals && w && bias && gamma && beta && scale && shift && save_mean && save_rstd && count > 1.0);
    const StemBn bn = {nullptr, gamma, beta, running_mean, running_var, momentum, eps, count, scale, shift, save_mean, save_rstd};
    hipLaunchKernelGGL(conv1_finalize_kernel, dim3(1), dim3(576), 0, static_cast<hipStream_t>(stream), mom_totals, w, bias, bn, 1);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_conv1_fwd(int dtype, const float* img, int N, int F, int T, const float* w, const float* bias,
                                  const float* scale, const float* shift, void* out, float* xl, void* stream) {
    ASSL_REQUIRE(img && w && bias && scale && shift && out && N > 0 && F >= 2 && F <= 126 && T >= 2 && (F % 2) == 0);
    ASSL_REQUIRE(dtype == 0 || dtype == 1 || dtype == 2);
    ASSL_REQUIRE(!xl || dtype == 1);                              // the fused layer mean exists for the MFMA kernel only
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int xs_split = 4;                                       // AUDIOSSL_CONV1_XL_PARTS in include/audiossl_hip.h
    const int grid = xl ? N * xs_split : min(N * (T / 2), 2048);
    size_t lds = sizeof(float) * (F + 2) * 4;
    if (dtype == 1) lds = sizeof(float) * (((F + 2) * 4 + 3) & ~3) + sizeof(bf16) * (F / 2) * 64;     // + the output staging tile
    if (dtype == 0)
        hipLaunchKernelGGL(conv1_fwd_kernel<float>, dim3(grid), dim3(256), lds, s, img, w, bias, scale, shift,
                           static_cast<float*>(out), N, F, T);
    else if (dtype == 2)
        hipLaunchKernelGGL(conv1_fwd_kernel<bf16>, dim3(grid), dim3(256), lds, s, img, w, bias, scale, shift,
                           static_cast<bf16*>(out), N, F, T);
    else
        hipLaunchKernelGGL(conv1_fwd_mfma_kernel<false>, dim3(grid), dim3(256), lds, s, img, w, bias, scale, shift,
                           static_cast<bf16*>(out), xl, xs_split, N, F, T, StemBn{});
    ASSL_LAUNCH_CHECK();
}

// conv1_finalize + conv1_fwd(dtype 1) in one launch: `mom` is the view's moment slot as conv1_moments_pair left it; the totals end
// up in mom[0..53], scale / shift / mean / rstd and the running buffers are written as conv1_finalize writes them (same bits).
extern "C" int audiossl_conv1_fwd_train(const float* img, int N, int F, int T, double* mom, double count, const float* w,
                                        const float* bias, const float* gamma, const float* beta, float* running_mean,
                                        float* running_var, float momentum, float eps, float* scale, float* shift,
                                        float* save_mean, float* save_rstd, void* out, float* xl, void* stream) {
    ASSL_REQUIRE(img && mom && w && bias && gamma && beta && scale && shift && save_mean && save_rstd && out && count > 1.0);
    ASSL_REQUIRE(N > 0 && F >= 2 && F <= 126 && T >= 2 && (F % 2) == 0 && (!running_mean == !running_var));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int xs_split = 4;                                       // AUDIOSSL_CONV1_XL_PARTS in include/audiossl_hip.h
    const int grid = xl ? N * xs_split : min(N * (T / 2), 2048);
    const size_t lds = max(sizeof(float) * (((F + 2) * 4 + 3) & ~3) + sizeof(bf16) * (F / 2) * 64, sizeof(StemBnLds));
    const StemBn bn = {mom, gamma, beta, running_mean, running_var, momentum, eps, count, scale, shift, save_mean, save_rstd};
    hipLaunchKernelGGL(conv1_fwd_mfma_kernel<true>, dim3(grid), dim3(256), lds, s, img, w, bias, (const float*)nullptr,
                       (const float*)nullptr, static_cast<bf16*>(out), xl, xs_split, N, F, T, bn);
    ASSL_LAUNCH_CHECK();
}

// acc: 32*64*11 floats of scratch (zeroed here).  dxl may be null.  Grad outputs are accumulated (+=).
static int conv1_bwd_main(int dtype, int conv_dtype, const float* img, int N, int F, int T, const float* w, const float* bias,
                                  const float* gamma, const float* scale, const float* shift, const float* mean,
                                  const float* rstd, const double* mom, const void* dP, const void* dxl, float* acc,
                                  void* stream) {
    ASSL_REQUIRE(img && w && bias && gamma && scale && shift && mean && rstd && mom && dP && acc);
    ASSL_REQUIRE(N > 0 && F >= 2 && F <= 64 && T >= 2 && (F % 2) == 0 && (dtype == 0 || dtype == 1));
    // conv_dtype 1 (MFMA recompute): dtype is the type of dP alone (fp32 or bf16), dxl is fp32 either way
    hipStream_t s = static_cast<hipStream_t>(stream);
    ASSL_ZERO(acc, sizeof(float) * 32 * 64 * 11, s);
    static const int bwd_grid = getenv("AUDIOSSL_CONV1_BWD_GRID") ? atoi(getenv("AUDIOSSL_CONV1_BWD_GRID")) : 2048;
    const int grid = min(N * (T / 2), bwd_grid);
    const size_t lds = sizeof(float) * (F + 2) * 4;
    const float inv_To = 1.f / (float)(T / 2);
    auto mfma = [&](auto slab, size_t shmem) {                    // the slab kernel (F == 64) takes 16 KB more LDS
        assl_dispatch(dtype, [&](auto tg) { using TG = typename decltype(tg)::type;
            hipLaunchKernelGGL((conv1_bwd_mfma_kernel<slab(), TG>), dim3(grid), dim3(256), shmem, s, img, w, bias, scale, shift, mean, rstd,
                               static_cast<const TG*>(dP), static_cast<const float*>(dxl), inv_To, acc, N, F, T);
        });
    };
    if (conv_dtype == 1 && F == 64) mfma(std::true_type{}, lds + 2 * 2048 * sizeof(float));
    else if (conv_dtype == 1) mfma(std::false_type{}, lds);
    else assl_dispatch(dtype, [&](auto tg) { using TG = typename decltype(tg)::type;
        hipLaunchKernelGGL(conv1_bwd_kernel<TG>, dim3(grid), dim3(256), lds, s, img, w, bias, scale, shift, mean, rstd,
                           static_cast<const TG*>(dP), static_cast<const TG*>(dxl), inv_To, acc, N, F, T);
    });
    return ASSL_OK;
}

extern "C" int audiossl_conv1_bwd(int dtype, int conv_dtype, const float* img, int N, int F, int T, const float* w, const float* bias,
                                  const float* gamma, const float* scale, const float* shift, const float* mean,
                                  const float* rstd, const double* mom, const void* dP, const void* dxl, float* acc,
                                  float* dW, float* dbias, float* dgamma, float* dbeta, void* stream) {
    ASSL_REQUIRE(dW && dgamma && dbeta);
    const int rc = conv1_bwd_main(dtype, conv_dtype, img, N, F, T, w, bias, gamma, scale, shift, mean, rstd, mom, dP, dxl, acc, stream);
    if (rc != ASSL_OK) return rc;
    hipLaunchKernelGGL(conv1_bwd_finalize_kernel, dim3(1), dim3(704), 0, static_cast<hipStream_t>(stream), acc, mom, w, bias, gamma, mean,
                       rstd, (double)N * F * T, dW, dbias, dgamma, dbeta, (const float*)nullptr, (float*)nullptr);
    ASSL_LAUNCH_CHECK();
}

// SyncBatchNorm halves: conv1_bwd_sums = the gradient kernel + this rank's (sum g, sum g xhat) per channel in lstat [2][64];
// conv1_bwd_finalize = weight / BatchNorm gradients from the rank's own sums with the GLOBAL means (gstat = all-reduced lstat).
extern "C" int audiossl_conv1_bwd_sums(int dtype, int conv_dtype, const float* img, int N, int F, int T, const float* w,
                                       const float* bias, const float* gamma, const float* scale, const float* shift,
                                       const float* mean, const float* rstd, const double* mom, const void* dP, const void* dxl,
                                       float* acc, float* lstat, void* stream) {
    ASSL_REQUIRE(lstat);
    const int rc = conv1_bwd_main(dtype, conv_dtype, img, N, F, T, w, bias, gamma, scale, shift, mean, rstd, mom, dP, dxl, acc, stream);
    if (rc != ASSL_OK) return rc;
    hipLaunchKernelGGL(conv1_bwd_finalize_kernel, dim3(1), dim3(704), 0, static_cast<hipStream_t>(stream), acc, mom, w, bias, gamma, mean,
                       rstd, 1.0, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, (const float*)nullptr, lstat);
    ASSL_LAUNCH_CHECK();
}
extern "C" int audiossl_conv1_bwd_finalize(const float* acc, const double* mom, const float* w, const float* bias, const float* gamma,
                                           const float* mean, const float* rstd, double count_global, const float* gstat, float* dW,
                                           float* dbias, float* dgamma, float* dbeta, void* stream) {
    ASSL_REQUIRE(acc && mom && w && bias && gamma && mean && rstd && gstat && dW && dgamma && dbeta && count_global > 1.0);
    hipLaunchKernelGGL(conv1_bwd_finalize_kernel, dim3(1), dim3(704), 0, static_cast<hipStream_t>(stream), acc, mom, w, bias, gamma, mean,
                       rstd, count_global, dW, dbias, dgamma, dbeta, gstat, (float*)nullptr);
    ASSL_LAUNCH_CHECK();
}
