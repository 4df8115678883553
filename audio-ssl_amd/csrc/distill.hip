// UnFuSeD pseudo-label self-distillation loss (`src/upstream/unfused/upstream_expert.py:141-168`, `src/utils/utils.py:191-197`;
// original `extras/unfused/moco_model.py:286-342`): 4 cross-entropies, 3 KL terms whose target soft-max is differentiable and
// 3 normalised-MSE terms over the student logits z1..z3 and the teacher logits t, forward AND all four gradients in ONE launch.
//
// A row's four logit vectors are read once with 16-byte loads and stay in registers: one wave per row up to 256 classes
// (4 rows per workgroup), one workgroup per row up to 1024 (one float4 per thread and tensor) and up to UNFUSED_MAX_C = 4096
// (four float4: 64 data registers).  Everything is fp32; every exp takes `x - rowmax`; `log pt` is `t - lse(t)`, so a target
// probability that underflows contributes its limit 0 where fp32 autograd of `0 * log 0` gives NaN.
#include "common.h"

#define UNFUSED_MAX_C 4096

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4_;

// sum / max of NR values over the W threads that share a row; result valid in every one of them.  W == 256: the four waves
// exchange through `sh` (4 * NR floats), all threads of the workgroup take part.
template <int W, int NR, bool MAX>
__device__ __forceinline__ void row_reduce(float (&v)[NR], float* sh) {
#pragma unroll
    for (int i = 0; i < NR; ++i) v[i] = MAX ? wave_max(v[i]) : wave_sum(v[i]);
    if (W == 256) {
        const int w = threadIdx.x >> 6;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) sh[w * NR + i] = v[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const float a = sh[i], b = sh[NR + i], c = sh[2 * NR + i], d = sh[3 * NR + i];
            v[i] = MAX ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : (a + b) + (c + d);
        }
    }
}

template <typename T_> __device__ __forceinline__ void store4(T_* p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void store4<float>(float* p, float a, float b, float c, float d) {
    *reinterpret_cast<f32x4_*>(p) = f32x4_{a, b, c, d};
}
template <> __device__ __forceinline__ void store4<bf16>(bf16* p, float a, float b, float c, float d) {
    bf16x4 v;
    v[0] = (bf16)a; v[1] = (bf16)b; v[2] = (bf16)c; v[3] = (bf16)d;
    *reinterpret_cast<bf16x4*>(p) = v;
}

// W threads per row (64: a wave, 256: the workgroup), NV float4 per thread and tensor: columns [0, 4 * W * NV).
// q = 0..2 students, q = 3 teacher.  loss4 += {total, CE, KL, MSE}: one atomic per slot and workgroup.
template <typename T_, int W, int NV>
__global__ __launch_bounds__(256) void unfused_loss_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                           const float* __restrict__ z3, const float* __restrict__ tt,
                                                           const long long* __restrict__ label, int B, int C, long ld, float alpha,
                                                           float beta, float gamma, float* __restrict__ loss4, T_* __restrict__ dz1,
                                                           T_* __restrict__ dz2, T_* __restrict__ dz3, T_* __restrict__ dt) {
    constexpr int RPB = 256 / W;                 // rows per workgroup and pass
    __shared__ float sh[4 * 16];
    const int lir = threadIdx.x % W, sub = threadIdx.x / W;
    const float invB = 1.f / (float)B;
    const float eps = 1e-12f;
    float acc_ce = 0.f, acc_kl = 0.f, acc_mse = 0.f;
    const float* const src[4] = {z1, z2, z3, tt};
    T_* const dst[4] = {dz1, dz2, dz3, dt};

    for (long r = (long)blockIdx.x * RPB + sub; r < B; r += (long)gridDim.x * RPB) {
        // ---- the row's four vectors; columns >= C become 0 (whatever the padding holds, NaN included)
        float x[4][NV][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int c0 = (k * W + lir) * 4;
                f32x4_ v = f32x4_{0.f, 0.f, 0.f, 0.f};
                if (c0 < C) v = *reinterpret_cast<const f32x4_*>(src[q] + r * ld + c0);        // c0 + 3 < ld: ld % 4 == 0, ld >= C
#pragma unroll
                for (int j = 0; j < 4; ++j) x[q][k][j] = (c0 + j < C) ? v[j] : 0.f;
            }
        const long long y = label[r];
        const bool valid = y >= 0 && y < (long long)C;          // the label is only ever compared, never used as an index
        const int yi = valid ? (int)y : -1;

        // ---- pass 1: row maxima; squared norms, student . teacher, the label's logits
        float mx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float m = -3.0e38f;
#pragma unroll
            for (int k = 0; k < NV; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) if ((k * W + lir) * 4 + j < C) m = fmaxf(m, x[q][k][j]);
            mx[q] = m;
        }
        row_reduce<W, 4, true>(mx, sh);
        float s1[11];                 // [0:4) |x_q|^2, [4:7) <z_h, t>, [7:11) x_q[y]
#pragma unroll
        for (int i = 0; i < 11; ++i) s1[i] = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (k * W + lir) * 4 + j;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    s1[q] = __builtin_fmaf(x[q][k][j], x[q][k][j], s1[q]);
                    if (c == yi) s1[7 + q] = x[q][k][j];
                }
#pragma unroll
                for (int h = 0; h < 3; ++h) s1[4 + h] = __builtin_fmaf(x[h][k][j], x[3][k][j], s1[4 + h]);
            }
        row_reduce<W, 11, false>(s1, sh);

        // ---- pass 2: soft-max denominators
        float se[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((k * W + lir) * 4 + j < C) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) se[q] += expf(x[q][k][j] - mx[q]);
                }
        row_reduce<W, 4, false>(se, sh);
        float lg[4], inv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { lg[q] = logf(se[q]); inv[q] = 1.f / se[q]; }

        // ---- pass 3: KL rows  sum_c pt (log pt - log ps_h),  log pt - log ps_h = (t - mt) - (z - mh) - (log st - log sh)
        float kl[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((k * W + lir) * 4 + j < C) {
                    const float tc = x[3][k][j] - mx[3];
                    const float pt = expf(tc) * inv[3];
#pragma unroll
                    for (int h = 0; h < 3; ++h) kl[h] = __builtin_fmaf(pt, (tc - (x[h][k][j] - mx[h])) - (lg[3] - lg[h]), kl[h]);
                }
        row_reduce<W, 3, false>(kl, sh);

        // ---- the row's loss terms
        float nrm[4], nc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { nrm[q] = sqrtf(s1[q]); nc[q] = fmaxf(nrm[q], eps); }
        float cosv[3];
#pragma unroll
        for (int h = 0; h < 3; ++h) cosv[h] = s1[4 + h] / (nc[h] * nc[3]);
        if (lir == 0) {
            float ce = 0.f, k3 = 0.f, ms = 0.f;
#pragma unroll
            for (int h = 0; h < 3; ++h) {
                ce += (mx[h] - s1[7 + h]) + lg[h];
                k3 += kl[h];
                ms += 2.f - 2.f * cosv[h];
            }
            ce = alpha * ce + ((mx[3] - s1[10]) + lg[3]);
            const float bad = valid ? 0.f : __builtin_nanf("");          // a label outside [0, C) poisons all four slots
            acc_ce += ce * invB + bad;
            acc_kl += beta * k3 * invB + bad;
            acc_mse += gamma * ms * invB + bad;
        }

        // ---- gradients
        if (dz1 != nullptr) {
            const float g2 = 2.f * gamma * invB;
            // clamp(min = eps) backward: below eps the norm is a constant, the projection term vanishes
            float pz[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) pz[q] = nrm[q] >= eps ? 1.f : 0.f;
            const float it = 1.f / nc[3];
            float iz[3];
#pragma unroll
            for (int h = 0; h < 3; ++h) iz[h] = 1.f / nc[h];
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int c0 = (k * W + lir) * 4;
                if (c0 >= ld) continue;
                float g[4][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + j;
                    const float tc = x[3][k][j] - mx[3];
                    const float pt = expf(tc) * inv[3];
                    const float oh = c == yi ? 1.f : 0.f;
                    const float th = x[3][k][j] * it;
                    float gt = (pt - oh) * invB;
#pragma unroll
                    for (int h = 0; h < 3; ++h) {
                        const float zc = x[h][k][j] - mx[h];
                        const float ps = expf(zc) * inv[h];
                        const float zh = x[h][k][j] * iz[h];
                        g[h][j] = (alpha * (ps - oh) + beta * (ps - pt)) * invB - g2 * (th - pz[h] * cosv[h] * zh) * iz[h];
                        gt += beta * invB * pt * (((tc - zc) - (lg[3] - lg[h])) - kl[h]) - g2 * (zh - pz[3] * cosv[h] * th) * it;
                    }
                    g[3][j] = gt;
                    if (c >= C) { g[0][j] = 0.f; g[1][j] = 0.f; g[2][j] = 0.f; g[3][j] = 0.f; }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) store4<T_>(dst[q] + r * ld + c0, g[q][0], g[q][1], g[q][2], g[q][3]);
            }
            // padding columns beyond this variant's register tile: exact zeros (the engine runs GEMMs at the padded width)
            for (long c0 = ((long)NV * W + lir) * 4; c0 < ld; c0 += W * 4)
#pragma unroll
                for (int q = 0; q < 4; ++q) store4<T_>(dst[q] + r * ld + c0, 0.f, 0.f, 0.f, 0.f);
        }
    }

    // ---- one atomic per term and workgroup
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        sh[w * 3 + 0] = acc_ce; sh[w * 3 + 1] = acc_kl; sh[w * 3 + 2] = acc_mse;
    }
    __syncthreads();
    if (threadIdx.x == 0 && (long)blockIdx.x * RPB < B) {
        const float ce = (sh[0] + sh[3]) + (sh[6] + sh[9]);
        const float kl = (sh[1] + sh[4]) + (sh[7] + sh[10]);
        const float ms = (sh[2] + sh[5]) + (sh[8] + sh[11]);
        atomicAdd(&loss4[0], ce + kl + ms);
        atomicAdd(&loss4[1], ce);
        atomicAdd(&loss4[2], kl);
        atomicAdd(&loss4[3], ms);
    }
}

}  // namespace

// Class limit: C <= UNFUSED_MAX_C = 4096 (a row's four vectors in the registers of one workgroup).  The grid is capped at 64
// workgroups of four rows (wave per row) / 256 workgroups (workgroup per row): 256 rows per pass, longer batches walk a grid-stride
// loop, and a loss slot takes at most 256 atomics.
extern "C" int audiossl_unfused_loss(int gdtype, const float* z1, const float* z2, const float* z3, const float* t,
                                     const long long* label, int B, int C, long ld, float alpha, float beta, float gamma,
                                     float* loss4, void* dz1, void* dz2, void* dz3, void* dt, void* stream) {
    ASSL_REQUIRE(z1 && z2 && z3 && t && label && loss4 && (gdtype == 0 || gdtype == 1));
    ASSL_REQUIRE(B > 0 && C >= 2 && C <= UNFUSED_MAX_C && ld >= C);
    const int ng = (dz1 != nullptr) + (dz2 != nullptr) + (dz3 != nullptr) + (dt != nullptr);
    ASSL_REQUIRE(ng == 0 || ng == 4);
    if (ld % 4 != 0) return ASSL_EALIGN;
    if (!ASSL_ALIGNED16(z1) || !ASSL_ALIGNED16(z2) || !ASSL_ALIGNED16(z3) || !ASSL_ALIGNED16(t) || !ASSL_ALIGNED16(dz1) ||
        !ASSL_ALIGNED16(dz2) || !ASSL_ALIGNED16(dz3) || !ASSL_ALIGNED16(dt))
        return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    assl_dispatch(gdtype, [&](auto tag) { using T = typename decltype(tag)::type;
        T *g1 = static_cast<T*>(dz1), *g2 = static_cast<T*>(dz2), *g3 = static_cast<T*>(dz3), *g4 = static_cast<T*>(dt);
        if (C <= 256)
            hipLaunchKernelGGL((unfused_loss_kernel<T, 64, 1>), dim3(B < 256 ? (B + 3) / 4 : 64), dim3(256), 0, s, z1, z2, z3, t, label,
                               B, C, ld, alpha, beta, gamma, loss4, g1, g2, g3, g4);
        else if (C <= 1024)
            hipLaunchKernelGGL((unfused_loss_kernel<T, 256, 1>), dim3(B < 256 ? B : 256), dim3(256), 0, s, z1, z2, z3, t, label, B, C, ld,
                               alpha, beta, gamma, loss4, g1, g2, g3, g4);
        else
            hipLaunchKernelGGL((unfused_loss_kernel<T, 256, 4>), dim3(B < 256 ? B : 256), dim3(256), 0, s, z1, z2, z3, t, label, B, C, ld,
                               alpha, beta, gamma, loss4, g1, g2, g3, g4);
    });
    ASSL_LAUNCH_CHECK();
}
