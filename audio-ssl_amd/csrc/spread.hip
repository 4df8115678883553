// Label spreading on the nearest-neighbour graph (Zhou et al. 2004, "Learning with local and global consistency"; sklearn's
// `LabelSpreading`): the few-label counterpart of PIC on the matrix pic_build makes (W = A + A^T, canonical CSR, fp64 weights).
//
// spread_normalize: deg_i = row sum of W (fp64, column order), s_l = (float)(w_l / sqrt(deg_i deg_j)) for entry l = (i, j).  The
//   product under the root commutes, so S = D^-1/2 W D^-1/2 is symmetric bit for bit; a zero product gives 0 (an outlier whose
//   Gaussian weights all underflowed), never inf or NaN.
// spread_run: F_0 = Y, iters x { F <- alpha S F + (1 - alpha) Y } on an [n][m] fp32 block whose m columns are independent
//   problems.  Y is the 0/1 matrix of the per-row seed lists (seed_ptr / seed_col) and is never stored.  One launch per
//   iteration (spread_iter_kernel): a CSR x dense product that gathers rows of F, with the scale and the seed add in its
//   epilogue; F ping-pongs between the caller's buffer and the workspace so that the last round lands in the caller's.
//     Layout: the m columns are cut into `chunks` equal slices of at most 256 columns (a multiple of 4), so that no slice is a
//     mostly idle tail.  Slices wider than 64 columns: one wave per (row, slice) - the row's (col, s) pairs are wave-uniform
//     (the row index goes through readfirstlane, the pairs come by scalar loads), every lane owns 4 columns and reads one
//     16-byte piece of each neighbour's row: one coalesced read of up to 1 KiB per neighbour, four neighbours in flight.
//     Narrower slices: 16 lanes per row, four rows per wave, the same loop with per-lane pairs.
//     Every (row, column) value is ONE fmaf chain over the row's entries in column order, whatever the slice width, the
//     unrolling or the other columns of the launch are: two calls agree bit for bit and a column's result does not depend on
//     which columns share the launch.  No atomics, no barriers, nothing read from the workspace before it is written.
//     A hub row (csr_sym.h allows any in-degree) is walked by one wave per slice; it is correct at any length and is not split.
//   Workgroup id -> (row block, slice): AUDIOSSL_SPREAD_MAP=0 puts a row block's slices on consecutive ids, 1 (the default)
//   walks all row blocks of one slice before the next, so that the workgroups in flight gather from one slice-wide slab of F.
//   The results are the same bits either way (tools/spread_bench.py times both).
// spread_assign: per (row, trial) the arg-max over the trial's `classes` columns (ties to the lowest class, -1 when the largest
//   value is <= 0: no seed of the trial within `iters` hops) and the certainty 1 - H(p) / log(classes) of Iscen et al. 2019,
//   eq. 11, in fp64 from the fp32 row.
#include <stdlib.h>
#include "common.h"

namespace {

constexpr int SPREAD_MAX_M = 16384;       // columns of one spread_run call
constexpr int SLICE = 256;                // widest column slice: 64 lanes x 4 columns

inline long align16(long b) { return (b + 15) & ~15L; }

struct SpreadPlan {
    int chunks, cw;      // slices and their width in columns (a multiple of 4)
    int lpr;             // lanes per row: 64 or 16
    long row_blocks, blocks;
    long bytes;          // the second F buffer
};

bool spread_plan(int n, int m, SpreadPlan& p) {
    if (!(n >= 2 && m >= 4 && m % 4 == 0 && m <= SPREAD_MAX_M && (long)n * m < (1L << 31))) return false;
    p.chunks = (m + SLICE - 1) / SLICE;
    p.cw = ((m / 4 + p.chunks - 1) / p.chunks) * 4;
    p.lpr = p.cw > 64 ? 64 : 16;
    const int rows_per_wg = 256 / p.lpr;
    p.row_blocks = ((long)n + rows_per_wg - 1) / rows_per_wg;
    p.blocks = p.row_blocks * p.chunks;
    p.bytes = align16((long)n * m * 4);
    return true;
}

// Y's four columns c .. c + 3 of row `row`, scaled by `one`.
__device__ __forceinline__ f32x4 seed_piece(const int* __restrict__ seed_ptr, const int* __restrict__ seed_col, int seeds, int row, int c,
                                            float one) {
    f32x4 y = {0.f, 0.f, 0.f, 0.f};
    const int q0 = min(max(seed_ptr[row], 0), seeds), q1 = min(max(seed_ptr[row + 1], 0), seeds);
    for (int q = q0; q < q1; ++q) {
        const int d = seed_col[q] - c;               // a column outside [0, m) matches no lane
        y.x = d == 0 ? one : y.x;
        y.y = d == 1 ? one : y.y;
        y.z = d == 2 ? one : y.z;
        y.w = d == 3 ? one : y.w;
    }
    return y;
}

__global__ __launch_bounds__(256) void spread_seed_kernel(const int* __restrict__ seed_ptr, const int* __restrict__ seed_col, int seeds,
                                                          int n, int m, float* __restrict__ f) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int m4 = m >> 2;
    if (t >= (long)n * m4) return;
    const int row = (int)(t / m4), c = (int)(t % m4) * 4;
    *reinterpret_cast<f32x4*>(f + (long)row * m + c) = seed_piece(seed_ptr, seed_col, seeds, row, c, 1.f);
}

template <int LPR>
__global__ __launch_bounds__(256) void spread_iter_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                          const float* __restrict__ s, const int* __restrict__ seed_ptr,
                                                          const int* __restrict__ seed_col, const float* __restrict__ fin,
                                                          float* __restrict__ fout, int n, int m, long cap, int seeds, float alpha,
                                                          float beta, unsigned chunks, int cw, unsigned row_blocks, int map) {
    constexpr int ROWS = 256 / LPR;
    const unsigned id = blockIdx.x;
    const long rb = map == 0 ? id / chunks : id % row_blocks;
    const int ch = (int)(map == 0 ? id % chunks : id / row_blocks);
    const int lane = threadIdx.x % LPR;
    long r = rb * ROWS + threadIdx.x / LPR;
    if (LPR == 64) r = rb * ROWS + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform: scalar loads of the row
    if (r >= n) return;
    const int row = (int)r;
    const int c = ch * cw + lane * 4;
    if (lane * 4 >= cw || c >= m) return;
    const long l0 = max((long)rowptr[row], 0L), l1 = min((long)rowptr[row + 1], cap);
    const float* __restrict__ base = fin + c;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    long l = l0;
    for (; l + 4 <= l1; l += 4) {                    // four neighbours in flight; the chain stays in entry order
        int j[4];
        float sv[4];
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            j[u] = col[l + u];
            sv[u] = s[l + u];
            const bool ok = (unsigned)j[u] < (unsigned)n;      // a column outside [0, n) is skipped: weight 0, a valid address
            sv[u] = ok ? sv[u] : 0.f;
            j[u] = ok ? j[u] : row;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(base + (long)j[u] * m);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc.x = __builtin_fmaf(sv[u], v[u].x, acc.x);
            acc.y = __builtin_fmaf(sv[u], v[u].y, acc.y);
            acc.z = __builtin_fmaf(sv[u], v[u].z, acc.z);
            acc.w = __builtin_fmaf(sv[u], v[u].w, acc.w);
        }
    }
    for (; l < l1; ++l) {
        int j = col[l];
        float sv = s[l];
        const bool ok = (unsigned)j < (unsigned)n;
        sv = ok ? sv : 0.f;
        j = ok ? j : row;
        const f32x4 v = *reinterpret_cast<const f32x4*>(base + (long)j * m);
        acc.x = __builtin_fmaf(sv, v.x, acc.x);
        acc.y = __builtin_fmaf(sv, v.y, acc.y);
        acc.z = __builtin_fmaf(sv, v.z, acc.z);
        acc.w = __builtin_fmaf(sv, v.w, acc.w);
    }
    const f32x4 y = seed_piece(seed_ptr, seed_col, seeds, row, c, beta);
    f32x4 o;
    o.x = __builtin_fmaf(alpha, acc.x, y.x);
    o.y = __builtin_fmaf(alpha, acc.y, y.y);
    o.z = __builtin_fmaf(alpha, acc.z, y.z);
    o.w = __builtin_fmaf(alpha, acc.w, y.w);
    *reinterpret_cast<f32x4*>(fout + (long)row * m + c) = o;
}

// deg_i: one thread per row, terms in column order.
__global__ __launch_bounds__(256) void spread_degree_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                            const double* __restrict__ w, int n, long cap, double* __restrict__ deg) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long l0 = max((long)rowptr[i], 0L), l1 = min((long)rowptr[i + 1], cap);
    double d = 0.;
    for (long l = l0; l < l1; ++l) {
        const int j = col[l];
        if (j >= 0 && j < n) d += w[l];
    }
    deg[i] = d;
}

__global__ __launch_bounds__(256) void spread_scale_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const double* __restrict__ w, const double* __restrict__ deg, int n, long cap,
                                                           float* __restrict__ s) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long l0 = max((long)rowptr[i], 0L), l1 = min((long)rowptr[i + 1], cap);
    const double di = deg[i];
    for (long l = l0; l < l1; ++l) {
        const int j = col[l];
        float v = 0.f;
        if (j >= 0 && j < n) {
            const double p = di * deg[j];                        // commutes: s_ij == s_ji bit for bit
            if (p > 0.) v = (float)(w[l] / sqrt(p));
        }
        s[l] = v;
    }
}

__global__ __launch_bounds__(256) void spread_assign_kernel(const float* __restrict__ f, int n, int ldf, int classes, int trials,
                                                            int* __restrict__ label, float* __restrict__ confidence) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)n * trials) return;
    const float* __restrict__ row = f + (t / trials) * ldf + (t % trials) * (long)classes;
    float best = 0.f;
    int arg = -1;
    double sum = 0.;
    for (int c = 0; c < classes; ++c) {
        const float v = row[c];
        if (v > best) { best = v; arg = c; }                     // strictly greater: a tie stays with the lowest class
        if (v > 0.f) sum += (double)v;
    }
    double conf = 0.;
    if (arg >= 0) {
        conf = 1.;
        if (classes > 1) {
            double h = 0.;
            for (int c = 0; c < classes; ++c) {
                const float v = row[c];
                if (v > 0.f) { const double p = (double)v / sum; h -= p * log(p); }
            }
            conf = 1. - h / log((double)classes);
        }
    }
    label[t] = arg;
    confidence[t] = (float)conf;
}

}  // namespace

extern "C" int audiossl_spread_workspace(int n, int m, long* bytes) {
    SpreadPlan p;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(spread_plan(n, m, p));
    *bytes = p.bytes;
    return ASSL_OK;
}

extern "C" int audiossl_spread_normalize(const int* rowptr, const int* col, const double* w, int n, long cap, double* deg, float* s,
                                         void* stream) {
    ASSL_REQUIRE(rowptr && col && w && deg && s);
    ASSL_REQUIRE(n >= 2 && cap >= 0);
    hipStream_t st = S_(stream);
    hipLaunchKernelGGL(spread_degree_kernel, GRID1(n), dim3(256), 0, st, rowptr, col, w, n, cap, deg);
    hipLaunchKernelGGL(spread_scale_kernel, GRID1(n), dim3(256), 0, st, rowptr, col, w, deg, n, cap, s);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_spread_run(const int* rowptr, const int* col, const float* s, int n, long cap, const int* seed_ptr,
                                   const int* seed_col, int seeds, int m, double alpha, int iters, float* f, void* workspace,
                                   long workspace_bytes, void* stream) {
    SpreadPlan p;
    ASSL_REQUIRE(rowptr && col && s && seed_ptr && seed_col && f && workspace);
    ASSL_REQUIRE(spread_plan(n, m, p));
    ASSL_REQUIRE(cap >= 0 && seeds >= 0 && iters >= 1 && iters <= 1000000);
    ASSL_REQUIRE(alpha > 0. && alpha < 1.);                      // NaN fails both
    ASSL_REQUIRE(workspace_bytes >= p.bytes);
    if (!ASSL_ALIGNED16(f) || !ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t st = S_(stream);
    const char* e = getenv("AUDIOSSL_SPREAD_MAP");               // diagnostics: the same bits either way
    const int map = e ? atoi(e) : 1;
    float* other = static_cast<float*>(workspace);
    float* cur = (iters & 1) ? other : f;                        // round `iters` writes the caller's buffer
    float* nxt = (iters & 1) ? f : other;
    const float a = (float)alpha, b = (float)(1.0 - alpha);
    hipLaunchKernelGGL(spread_seed_kernel, GRID1((long)n * (m / 4)), dim3(256), 0, st, seed_ptr, seed_col, seeds, n, m, cur);
    for (int it = 0; it < iters; ++it) {
        if (p.lpr == 64)
            hipLaunchKernelGGL(spread_iter_kernel<64>, dim3((unsigned)p.blocks), dim3(256), 0, st, rowptr, col, s, seed_ptr, seed_col, cur,
                               nxt, n, m, cap, seeds, a, b, (unsigned)p.chunks, p.cw, (unsigned)p.row_blocks, map);
        else
            hipLaunchKernelGGL(spread_iter_kernel<16>, dim3((unsigned)p.blocks), dim3(256), 0, st, rowptr, col, s, seed_ptr, seed_col, cur,
                               nxt, n, m, cap, seeds, a, b, (unsigned)p.chunks, p.cw, (unsigned)p.row_blocks, map);
        float* t = cur; cur = nxt; nxt = t;
    }
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_spread_assign(const float* f, int n, int ldf, int classes, int trials, int* label, float* confidence,
                                      void* stream) {
    ASSL_REQUIRE(f && label && confidence);
    ASSL_REQUIRE(n >= 1 && classes >= 1 && trials >= 1);
    ASSL_REQUIRE((long)classes * trials <= ldf && (long)n * ldf < (1L << 31));
    hipStream_t st = S_(stream);
    hipLaunchKernelGGL(spread_assign_kernel, GRID1((long)n * trials), dim3(256), 0, st, f, n, ldf, classes, trials, label, confidence);
    ASSL_LAUNCH_CHECK();
}
