// Audio tagging (multi-label) downstream: BCE-with-logits on soft targets and the per-class ranking metrics of
// `extras/mast_new/mast/utilities/stats.py:11-57` (sklearn's average_precision_score / roc_auc_score), on the device.
//
// bce_rows: nn.BCEWithLogitsLoss(), mean over N*C, stable form max(x,0) - x t + log1p(exp(-|x|)); dlogits = (sigmoid(x) - t) /
//   (N*C).  The entry point takes no scratch, so the loss is summed by ONE workgroup of 1024 threads: fp32 terms (the product
//   folded in by one fma), fp64 accumulation per thread in element order, wave butterfly, 16 wave partials in LDS added in
//   order by the last stage.  No atomics anywhere: two runs agree bit for bit.  The gradient is a plain grid-wide map.
//
// tagging_stats: AP and ROC-AUC need, for every positive i of a class, four counts over the class column:
//     ge_all = #{j: s_j >= s_i}   gt_all = #{j: s_j > s_i}   ge_pos, gt_pos = the same over the positives
//   AP  = (1/npos) sum_i ge_pos_i / ge_all_i              (precision after the whole tie group of s_i, one recall step per
//                                                          positive: sklearn's step-wise sum over the distinct thresholds)
//   AUC = sum_i (2 lt_neg_i + eq_neg_i) / (2 npos nneg)   (Mann-Whitney with half credit = the ROC trapezoid over tie groups)
//   with lt_neg = nneg - (ge_all - ge_pos), eq_neg = (ge_all - ge_pos) - (gt_all - gt_pos).  Integer counts, no sort; the work
//   is sum_c npos_c * (N + npos_c) comparisons, and tagging targets are sparse.
//
//   1. tag_transpose_kernel  [N][C] scores / targets -> class-major copies in the workspace, 256 x 16 tiles through LDS.
//   2. tag_compact_kernel    one workgroup per class: the positives' scores in sample order (ballot prefix per wave, running base
//                            over the sample tiles), npos[c].
//   3. tag_count_kernel      one workgroup per (class, 256 positives); workgroups past npos[c] leave at once.  A thread holds one
//                            positive; the class column and then the positive list stream through LDS in chunks of 1024 (the
//                            next chunk's global loads in flight during the scan) and every lane reads the same LDS address: a
//                            broadcast.  int32 counts -> fp64 AP term, int64 AUC term -> fixed-order block sum -> one partial.
//   4. tag_fold_kernel       one wave per class folds the partials (lane-strided, then the butterfly) and divides.
//   Every workspace cell that is read has been written by an earlier kernel of the same call: no clearing.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- BCE
__device__ __forceinline__ float bce_term(float x, float t) {
    return __builtin_fmaf(-x, t, fmaxf(x, 0.f)) + log1pf(expf(-fabsf(x)));
}

// e = exp(-|x|) <= 1: sigmoid = 1 / (1 + e) for x >= 0, e / (1 + e) below: no overflow, absolute error <= 2^-23
__device__ __forceinline__ float sigmoid_stable(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.f : e) / (1.f + e);
}

template <typename T_>
__global__ __launch_bounds__(256) void bce_grad_kernel(const float* __restrict__ logits, const float* __restrict__ targets, long n,
                                                       double inv, T_* __restrict__ dlogits) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        dlogits[i] = from_f32<T_>((float)((double)(sigmoid_stable(logits[i]) - targets[i]) * inv));
}

__global__ __launch_bounds__(1024) void bce_loss_kernel(const float* __restrict__ logits, const float* __restrict__ targets, long n,
                                                        float* __restrict__ loss_out) {
    __shared__ double sh[16];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) acc += (double)bce_term(logits[i], targets[i]);
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += sh[w];
        loss_out[0] = (float)(t / (double)n);
    }
}

// ------------------------------------------------------------------------------------------------------------ metrics
constexpr int TS = 256;             // samples per transpose tile = positives per counting workgroup
constexpr int TC = 16;              // classes per transpose tile: 64-byte runs of a score row
constexpr int CH = 1024;            // floats per LDS chunk of the counting kernel

struct TagPlan {
    long Np;                        // class-major row pitch (elements): N rounded up to 4
    long tiles;                     // ceil(N / 256)
    long off_pos, off_flag, off_ap, off_auc, bytes;     // scoresT sits at offset 0
};

inline long up16(long b) { return (b + 15) & ~15L; }

// Limits beyond the documented ones: the class-major copies hold C * Np elements (<= 2^40), and the counting kernel's flat grid
// C * tiles fits 31 bits.
bool tag_plan(long N, int C, TagPlan& p) {
    if (!(N >= 1 && N < (1L << 31) && C >= 1)) return false;
    p.Np = (N + 3) & ~3L;
    p.tiles = (N + TS - 1) / TS;
    if (p.Np > (1L << 40) / C || p.tiles > ((1L << 31) - 1) / C) return false;
    const long cells = (long)C * p.Np;
    p.off_pos = up16(cells * 4);
    p.off_flag = p.off_pos + up16(cells * 4);
    p.off_ap = p.off_flag + up16(cells);
    p.off_auc = p.off_ap + up16((long)C * p.tiles * 8);
    p.bytes = p.off_auc + up16((long)C * p.tiles * 8);
    return true;
}

__global__ __launch_bounds__(256) void tag_transpose_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ targets,
                                                            long N, int C, long Np, int ctiles, float* __restrict__ scoresT,
                                                            unsigned char* __restrict__ flagsT) {
    __shared__ float tile[TC][TS + 1];
    __shared__ unsigned char fl[TC][TS + 4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long n0 = (long)(blockIdx.x / ctiles) * TS;
    const int c0 = (int)(blockIdx.x % ctiles) * TC;
    const int cc = tid & (TC - 1);
#pragma unroll
    for (int k = 0; k < TS / (256 / TC); ++k) {
        const int s = k * (256 / TC) + (tid >> 4);
        const long n = n0 + s;
        const int c = c0 + cc;
        const bool in = n < N && c < C;
        tile[cc][s] = in ? scores[n * C + c] : 0.f;
        fl[cc][s] = in ? (unsigned char)(targets[n * C + c] != 0) : (unsigned char)0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TC / 4; ++q) {
        const int r = w * (TC / 4) + q;
        const int c = c0 + r;
        if (c >= C) break;                                           // wave-uniform
#pragma unroll
        for (int j = 0; j < TS / 64; ++j) {
            const int s = j * 64 + lane;
            const long n = n0 + s;
            if (n < N) {
                scoresT[(long)c * Np + n] = tile[r][s];
                flagsT[(long)c * Np + n] = fl[r][s];
            }
        }
    }
}

__global__ __launch_bounds__(256) void tag_compact_kernel(const float* __restrict__ scoresT, const unsigned char* __restrict__ flagsT,
                                                          long N, long Np, float* __restrict__ posT, int* __restrict__ npos) {
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long row = (long)blockIdx.x * Np;
    long base = 0;
    for (long n0 = 0; n0 < N; n0 += 256) {
        const long n = n0 + tid;
        const bool f = n < N && flagsT[row + n] != 0;
        const unsigned long long m = __ballot(f);
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int v = wcnt[i]; before += i < w ? v : 0; total += v; }
        if (f) posT[row + base + before + __popcll(m & ((1ull << lane) - 1ull))] = scoresT[row + n];      // base + ... <= n
        base += total;
        __syncthreads();
    }
    if (tid == 0) npos[blockIdx.x] = (int)base;
}

// Counts of one stream (n values at src) against the thread's score s; every lane walks the same LDS addresses.
__device__ __forceinline__ void tag_stream(const float* __restrict__ src, long n, float s, float* __restrict__ buf, int tid, int& ge,
                                           int& gt) {
    const float pad = __builtin_nanf("");                            // compares false both ways: the tail of a chunk counts nothing
    float r[CH / 256];
    auto load = [&](long b) {
#pragma unroll
        for (int k = 0; k < CH / 256; ++k) {
            const long j = b + k * 256 + tid;
            r[k] = j < n ? src[j] : pad;
        }
    };
    load(0);
    for (long b = 0; b < n; b += CH) {
        __syncthreads();                                             // the previous chunk's scan is done
#pragma unroll
        for (int k = 0; k < CH / 256; ++k) buf[k * 256 + tid] = r[k];
        __syncthreads();
        if (b + CH < n) load(b + CH);
        const long left = n - b;
        const int lim = left >= CH ? CH / 4 : (int)((left + 3) >> 2);
        const f32x4* b4 = reinterpret_cast<const f32x4*>(buf);
#pragma unroll 4
        for (int j = 0; j < lim; ++j) {
            const f32x4 v = b4[j];
            ge += (v[0] >= s) + (v[1] >= s) + (v[2] >= s) + (v[3] >= s);
            gt += (v[0] > s) + (v[1] > s) + (v[2] > s) + (v[3] > s);
        }
    }
}

__global__ __launch_bounds__(256) void tag_count_kernel(const float* __restrict__ scoresT, const float* __restrict__ posT,
                                                        const int* __restrict__ npos, long N, int C, long Np, long tiles,
                                                        double* __restrict__ part_ap, long long* __restrict__ part_auc) {
    __shared__ __attribute__((aligned(16))) float buf[CH];
    __shared__ double sh_ap[4];
    __shared__ long long sh_auc[4];
    const int c = (int)(blockIdx.x % (unsigned)C);
    const long tile = blockIdx.x / (unsigned)C;
    const int np = npos[c];
    if (tile * TS >= np) return;                                     // the whole workgroup leaves: no barrier is split
    const int tid = threadIdx.x;
    const long row = (long)c * Np;
    const long i = tile * TS + tid;
    const bool live = i < np;
    const float s = live ? posT[row + i] : 0.f;
    int ge_all = 0, gt_all = 0, ge_pos = 0, gt_pos = 0;
    tag_stream(scoresT + row, N, s, buf, tid, ge_all, gt_all);
    tag_stream(posT + row, np, s, buf, tid, ge_pos, gt_pos);
    double ap = 0.0;
    long long auc = 0;
    if (live) {                                                      // ge_all >= ge_pos >= 1: the positive counts itself
        const long long nneg = N - np;
        const long long ge_neg = ge_all - ge_pos, gt_neg = gt_all - gt_pos;
        ap = (double)ge_pos / (double)ge_all;
        auc = 2 * (nneg - ge_neg) + (ge_neg - gt_neg);
    }
    ap = wave_sum(ap);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) auc += __shfl_xor(auc, o, 64);
    if ((tid & 63) == 0) { sh_ap[tid >> 6] = ap; sh_auc[tid >> 6] = auc; }
    __syncthreads();
    if (tid == 0) {
        part_ap[(long)c * tiles + tile] = ((sh_ap[0] + sh_ap[1]) + sh_ap[2]) + sh_ap[3];
        part_auc[(long)c * tiles + tile] = sh_auc[0] + sh_auc[1] + sh_auc[2] + sh_auc[3];
    }
}

__global__ __launch_bounds__(256) void tag_fold_kernel(const double* __restrict__ part_ap, const long long* __restrict__ part_auc,
                                                       const int* __restrict__ npos, long N, int C, long tiles,
                                                       long long* __restrict__ auc_num2, double* __restrict__ ap_out,
                                                       double* __restrict__ auc_out) {
    const int lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;                                              // whole waves leave; no barrier below
    const long np = npos[c], nneg = N - np;
    const long used = (np + TS - 1) / TS;                            // the partials the counting kernel wrote
    double ap = 0.0;
    long long num = 0;
    for (long t = lane; t < used; t += 64) { ap += part_ap[c * tiles + t]; num += part_auc[c * tiles + t]; }
    ap = wave_sum(ap);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) num += __shfl_xor(num, o, 64);
    if (lane == 0) {
        const bool scored = np > 0 && nneg > 0;
        const double nan = __builtin_nan("");
        auc_num2[c] = num;
        ap_out[c] = scored ? ap / (double)np : nan;
        auc_out[c] = scored ? (double)num / (2.0 * (double)np * (double)nneg) : nan;
    }
}

}  // namespace

extern "C" int audiossl_bce_rows(int dtype, const float* logits, const float* targets, long N, int C, float* loss_out, void* dlogits,
                                 void* stream) {
    ASSL_REQUIRE(logits && targets && loss_out && N >= 1 && C >= 1 && (dtype == 0 || dtype == 1));
    ASSL_REQUIRE(N <= (1L << 40) / C);
    hipStream_t s = S_(stream);
    const long n = N * C;
    if (dlogits) {
        const long blocks = (n + 255) / 256;
        const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
        assl_dispatch(dtype, [&](auto t) { using T = typename decltype(t)::type;
            hipLaunchKernelGGL(bce_grad_kernel<T>, grid, dim3(256), 0, s, logits, targets, n, 1.0 / (double)n, static_cast<T*>(dlogits));
        });
    }
    hipLaunchKernelGGL(bce_loss_kernel, dim3(1), dim3(1024), 0, s, logits, targets, n, loss_out);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_tagging_workspace(long N, int C, long* bytes) {
    TagPlan p;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(tag_plan(N, C, p));
    *bytes = p.bytes;
    return ASSL_OK;
}

extern "C" int audiossl_tagging_stats(const float* scores, const unsigned char* targets, long N, int C, int* npos, long long* auc_num2,
                                      double* ap, double* auc, void* workspace, long workspace_bytes, void* stream) {
    TagPlan p;
    ASSL_REQUIRE(scores && targets && npos && auc_num2 && ap && auc && workspace);
    ASSL_REQUIRE(tag_plan(N, C, p));
    ASSL_REQUIRE(workspace_bytes >= p.bytes);
    if (!ASSL_ALIGNED16(scores) || !ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float* scoresT = reinterpret_cast<float*>(ws);
    float* posT = reinterpret_cast<float*>(ws + p.off_pos);
    unsigned char* flagsT = ws + p.off_flag;
    double* part_ap = reinterpret_cast<double*>(ws + p.off_ap);
    long long* part_auc = reinterpret_cast<long long*>(ws + p.off_auc);
    const int ctiles = (C + TC - 1) / TC;
    hipLaunchKernelGGL(tag_transpose_kernel, dim3((unsigned)(p.tiles * ctiles)), dim3(256), 0, s, scores, targets, N, C, p.Np, ctiles,
                       scoresT, flagsT);
    hipLaunchKernelGGL(tag_compact_kernel, dim3((unsigned)C), dim3(256), 0, s, scoresT, flagsT, N, p.Np, posT, npos);
    hipLaunchKernelGGL(tag_count_kernel, dim3((unsigned)(p.tiles * C)), dim3(256), 0, s, scoresT, posT, npos, N, C, p.Np, p.tiles,
                       part_ap, part_auc);
    hipLaunchKernelGGL(tag_fold_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, s, part_ap, part_auc, npos, N, C, p.tiles, auc_num2,
                       ap, auc);
    ASSL_LAUNCH_CHECK();
}
