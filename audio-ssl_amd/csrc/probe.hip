// Linear evaluation on cached embeddings: a grid of H linear heads (one per (lr, weight decay) pair) trained together on the
// [N][D] matrix `extract_embeddings` returns (src/evaluation/probe.py, evaluate_linear.py).  The heads live in one fp32 matrix
// W [H * Cp][Dp]: head h owns rows [h Cp, h Cp + C), its pad rows stay zero, column D is the bias (the batch carries 1.0 there).
// A step is five launches: probe_batch, audiossl_gemm (logits = Xb W^T), probe_ce, audiossl_gemm (dW = G^T Xb), probe_adamw.
//   probe_batch : gather the batch rows, standardise them, append the ones column and the zero pad
//   probe_ce    : per (row, head) stable soft-max cross-entropy over the head's C columns: loss sums (fp64), first-arg-max hits
//                 (int64) and dlogits, pad columns written as zeros
//   probe_adamw : torch.optim.AdamW with one (lr, wd) per head segment of the flat buffers (adamw.h: the arithmetic of adamw_kernel)
// Nothing here uses an atomic: every loss slot and hit counter has exactly one writer, which sums in a fixed order.
#include "adamw.h"

#define PROBE_MAX_C 4096
#define PROBE_MAX_D 4096

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4_;

// One thread per float4 of the [B][ldo] output.  (x - mean) * rstd: subtract, then multiply, each rounded once (no fused
// multiply-add can form from a difference times a factor; the intrinsics say so explicitly).
__global__ __launch_bounds__(256) void probe_batch_kernel(const float* __restrict__ X, long N, int D, const int* __restrict__ idx,
                                                          int B, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          float* __restrict__ out, long ldo) {
    const long q4 = ldo / 4;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * q4) return;
    const long r = e / q4;
    const int c0 = (int)(e % q4) * 4;
    const long src = (long)idx[r];
    f32x4_ o;
    if (src < 0 || src >= N) {                                   // never dereferenced: the whole row says so
        const float nan = __builtin_nanf("");
        o = f32x4_{nan, nan, nan, nan};
    } else if (c0 < D) {                                         // D % 4 == 0: a float4 is all data or all tail
        o = *reinterpret_cast<const f32x4_*>(X + src * D + c0);
        if (mean != nullptr) {
            const f32x4_ mu = *reinterpret_cast<const f32x4_*>(mean + c0), rs = *reinterpret_cast<const f32x4_*>(rstd + c0);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = __fmul_rn(__fsub_rn(o[j], mu[j]), rs[j]);
        }
    } else {
        o = f32x4_{c0 == D ? 1.f : 0.f, 0.f, 0.f, 0.f};
    }
    *reinterpret_cast<f32x4_*>(out + r * ldo + c0) = o;
}

// Lane exchange inside a row of 16 lanes on the DPP path (no LDS round trip): 0xB1 / 0x4E swap neighbours / pairs inside a quad,
// 0x141 mirrors the 8 lanes of a half row and 0x140 the 16 of a row.  After the two quad steps a quad is uniform, after the half
// mirror a half row, after the mirror the row: a 16-lane all-reduce for any commutative op.
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_take(T v) {
    static_assert(sizeof(T) == 4, "one dword");
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false));
}

// Reductions over the W threads that share a row (W = 16: a DPP row, four rows per wave; 64: a wave; 256 / 1024: 4 / 16 waves
// through `sh`, W / 64 slots per row group).  `op` is commutative; every thread of the workgroup takes part with all 64 lanes
// active (the barriers are workgroup-wide); result valid in all W threads.
template <int W, typename T, typename Op>
__device__ __forceinline__ T row_all(T v, T* sh, Op op) {
    v = op(v, dpp_take<0xB1>(v));
    v = op(v, dpp_take<0x4E>(v));
    v = op(v, dpp_take<0x141>(v));
    v = op(v, dpp_take<0x140>(v));
    if (W >= 64) {
        v = op(v, __shfl_xor(v, 16, 64));
        v = op(v, __shfl_xor(v, 32, 64));
    }
    if (W > 64) {
        constexpr int NW = W / 64;
        const int w = threadIdx.x >> 6, base = (w / NW) * NW;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sh[w] = v;
        __syncthreads();
        v = sh[base];
#pragma unroll
        for (int i = 1; i < NW; ++i) v = op(v, sh[base + i]);
    }
    return v;
}

// One workgroup of 1024 threads per head; W threads per row (16 up to 64 classes, 64 up to 256, 256 up to 1024, else 1024), one
// float4 of the head's columns per thread (4 W >= C), so 1024 / W rows are in flight and row group `sub` walks rows sub,
// sub + RPB, ... in order.  The soft-max is fp32 (max, sum of expf(x - max)); the row's loss (max - x[y]) + log(sum) and the sums
// over rows are fp64, per row group in row order and then over the groups in group order by thread 0, which is the only writer
// of loss_sum[h] and correct[h].
template <int W>
__global__ __launch_bounds__(1024) void probe_ce_kernel(const float* __restrict__ logits, long ld, const long long* __restrict__ label,
                                                        int B, int C, int Cp, float gscale, double* __restrict__ loss_sum,
                                                        long long* __restrict__ correct, float* __restrict__ dlogits) {
    constexpr int RPB = 1024 / W;
    __shared__ float shf[16];
    __shared__ int shi[16];
    __shared__ double sh_loss[RPB];
    __shared__ long long sh_hit[RPB];
    const int h = blockIdx.x;
    const int lir = threadIdx.x % W, sub = threadIdx.x / W;
    const int c0 = lir * 4;
    const long col = (long)h * Cp;
    double acc = 0.0;
    long long hits = 0;
    const int passes = (B + RPB - 1) / RPB;                     // the same trip count for every thread: the barriers stay uniform
#pragma unroll 2
    for (int it = 0; it < passes; ++it) {
        const long r = (long)it * RPB + sub;
        const bool live = r < B;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (live && c0 < C) {                                    // c0 + 3 < Cp: Cp % 4 == 0 and Cp >= C
            const f32x4_ v = *reinterpret_cast<const f32x4_*>(logits + r * ld + col + c0);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = v[j];
        }
        const long long y = live ? label[r] : 0;
        const bool valid = y >= 0 && y < (long long)C;           // the label is only ever compared, never used as an index
        const int yi = valid ? (int)y : -1;

        float m = -3.0e38f;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (c0 + j < C) m = fmaxf(m, x[j]);
        m = row_all<W>(m, shf, [](float a, float b) { return fmaxf(a, b); });
        int am = 0x7fffffff;                                     // first arg-max: the lowest column that holds the maximum
        float se = 0.f, xy = 0.f;
#pragma unroll
        for (int j = 3; j >= 0; --j)
            if (c0 + j < C) {
                if (x[j] == m) am = c0 + j;
                if (c0 + j == yi) xy = x[j];
                se += expf(x[j] - m);
            }
        am = row_all<W>(am, shi, [](int a, int b) { return a < b ? a : b; });
        se = row_all<W>(se, shf, [](float a, float b) { return a + b; });
        xy = row_all<W>(xy, shf, [](float a, float b) { return a + b; });       // one thread holds x[y], the others 0
        if (live && lir == 0) {
            const double row_loss = ((double)m - (double)xy) + log((double)se);       // one lane per row: the fp64 log is free
            acc += valid ? row_loss : (double)__builtin_nanf("");
            hits += (am == yi) ? 1 : 0;
        }
        if (dlogits != nullptr && live) {
            const float inv = 1.f / se;
            float* const dst = dlogits + r * ld + col;
            if (c0 < Cp) {
                f32x4_ g;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + j;
                    const float p = expf(x[j] - m) * inv;
                    float gj = gscale * (p - (c == yi ? 1.f : 0.f));
                    if (!valid) gj = __builtin_nanf("");
                    g[j] = c < C ? gj : 0.f;
                }
                *reinterpret_cast<f32x4_*>(dst + c0) = g;
            }
            for (int c = c0 + 4 * W; c < Cp; c += 4 * W)          // pad columns beyond the register tile (Cp > 4 W only)
                *reinterpret_cast<f32x4_*>(dst + c) = f32x4_{0.f, 0.f, 0.f, 0.f};
        }
    }
    if (lir == 0) { sh_loss[sub] = acc; sh_hit[sub] = hits; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        long long n = 0;
        for (int i = 0; i < RPB; ++i) { t += sh_loss[i]; n += sh_hit[i]; }
        loss_sum[h] += t;
        correct[h] += n;
    }
}

// blockIdx.y = head; the head's segment [h seg, (h + 1) seg) of the flat buffers with its own lr and weight decay.
__global__ __launch_bounds__(256) void probe_adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long seg, const float* __restrict__ lr,
                                                          const float* __restrict__ wd, float lr_scale, double beta1,
                                                          double beta2, float eps, const long long* __restrict__ step) {
    const int h = blockIdx.y;
    const float lr_h = lr[h] * lr_scale, wd_h = wd[h];
    // The betas arrive in fp64 and 1 - beta and the bias corrections are formed there, as torch.optim.AdamW forms them on the
    // host: 1 - 0.999f is 1.3e-5 off 0.001 in fp32, and 1 - b2^t rounded in fp32 up to 3e-5 / t (b2^t sits next to 1).
    const float b1 = (float)beta1, omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
    const double t = (double)step[0];
    const float step_size = (float)((double)lr_h / (1.0 - pow(beta1, t)));
    const float bc2s = (float)sqrt(1.0 - pow(beta2, t));
    const long base = (long)h * seg;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < seg; i += (long)gridDim.x * 1024) {       // seg % 4 == 0
        f32x4_ pv = *reinterpret_cast<f32x4_*>(p + base + i), mv = *reinterpret_cast<f32x4_*>(m + base + i);
        f32x4_ vv = *reinterpret_cast<f32x4_*>(v + base + i);
        const f32x4_ gv = *reinterpret_cast<const f32x4_*>(g + base + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pv[k], mk = mv[k], vk = vv[k];
            adamw_elem(pk, gv[k], mk, vk, lr_h, wd_h, b1, omb1, b2, omb2, eps, 1.f, step_size, bc2s);
            pv[k] = pk; mv[k] = mk; vv[k] = vk;
        }
        *reinterpret_cast<f32x4_*>(p + base + i) = pv;
        *reinterpret_cast<f32x4_*>(m + base + i) = mv;
        *reinterpret_cast<f32x4_*>(v + base + i) = vv;
    }
}

}  // namespace

extern "C" int audiossl_probe_batch(const float* X, long N, int D, const int* idx, int B, const float* mean, const float* rstd,
                                    float* out, long ldo, void* stream) {
    ASSL_REQUIRE(X && idx && out && N > 0 && B > 0);
    ASSL_REQUIRE((mean == nullptr) == (rstd == nullptr));
    ASSL_REQUIRE(D >= 8 && D <= PROBE_MAX_D && D % 8 == 0 && ldo >= (long)D + 8 && ldo % 4 == 0);
    if (!ASSL_ALIGNED16(X) || !ASSL_ALIGNED16(out) || !ASSL_ALIGNED16(mean) || !ASSL_ALIGNED16(rstd)) return ASSL_EALIGN;
    const long total = (long)B * (ldo / 4);
    ASSL_REQUIRE((total + 255) / 256 < 0x7fffffffL);
    hipLaunchKernelGGL(probe_batch_kernel, GRID1(total), dim3(256), 0, S_(stream), X, N, D, idx, B, mean, rstd, out, ldo);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_probe_ce(const float* logits, long ld, const long long* label, int B, int H, int C, int Cp, float gscale,
                                 double* loss_sum, long long* correct, float* dlogits, void* stream) {
    ASSL_REQUIRE(logits && label && loss_sum && correct && B > 0 && H >= 1);
    ASSL_REQUIRE(C >= 2 && C <= PROBE_MAX_C && Cp >= C && Cp % 4 == 0 && ld >= (long)H * Cp && ld % 4 == 0);
    if (!ASSL_ALIGNED16(logits) || !ASSL_ALIGNED16(dlogits)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
#define PROBE_CE(W_) hipLaunchKernelGGL(probe_ce_kernel<W_>, dim3(H), dim3(1024), 0, s, logits, ld, label, B, C, Cp, gscale, loss_sum, \
                                        correct, dlogits)
    if (C <= 64) PROBE_CE(16); else if (C <= 256) PROBE_CE(64); else if (C <= 1024) PROBE_CE(256); else PROBE_CE(1024);
#undef PROBE_CE
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_probe_adamw(float* W, const float* dW, float* m, float* v, int H, long seg, const float* lr, const float* wd,
                                    float lr_scale, double beta1, double beta2, float eps, const long long* step, void* stream) {
    ASSL_REQUIRE(W && dW && m && v && lr && wd && step && H >= 1 && H <= 65535 && seg > 0 && seg % 4 == 0);
    ASSL_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    if (!ASSL_ALIGNED16(W) || !ASSL_ALIGNED16(dW) || !ASSL_ALIGNED16(m) || !ASSL_ALIGNED16(v)) return ASSL_EALIGN;
    const int gx = (int)min((long)256, (seg + 1023) / 1024);
    hipLaunchKernelGGL(probe_adamw_kernel, dim3(gx, H), dim3(256), 0, S_(stream), W, dW, m, v, seg, lr, wd, lr_scale, beta1, beta2,
                       eps, step);
    ASSL_LAUNCH_CHECK();
}
