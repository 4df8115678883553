// M + M^T in CSR from fixed-length neighbour lists, on the device: the builder under pic_build (graph.hip: M_ij = exp(-d2_ij /
// sigma^2), fp64 out) and tsne_symmetrize (tsne.hip: M_ij = the conditional p_j|i, scaled, fp32 out).
//
// Row i of M holds k entries, columns idx[i][0..k-1] (distinct, no self; an index outside [0, n) is dropped).  Count in-degrees
// (integer atomics), scan, scatter (out-edges at fixed slots, in-edges through an integer cursor), then each row is sorted by
// column (rank sort: any in-degree up to n - 1 works) and a mutual pair merged into one entry m_ij + m_ji - two terms, so the
// order in which the cursor handed out slots does not reach the result.  Values travel in fp64 and are converted once, at the
// final write: out = (W)(sum * scale), scale = 1 leaves an fp64 sum as it is.
//
// No float atomics; the builder clears the two counters it accumulates into with a kernel; the rest of the workspace needs no
// clearing.
#pragma once
#include "common.h"
#include <limits.h>

namespace {

// out[i] = sum over t < i of (in[t] + add), out[n] = the total (also to *total when given).  One workgroup: every thread
// sums a contiguous run, the 1024 run sums are scanned in LDS.
__global__ __launch_bounds__(1024) void csr_scan_kernel(const int* __restrict__ in, int add, int n, int* __restrict__ out,
                                                        int* __restrict__ total) {
    __shared__ int sh[1024];
    const int tid = threadIdx.x;
    const long chunk = ((long)n + 1023) / 1024;
    const long lo = min(tid * chunk, (long)n), hi = min(lo + chunk, (long)n);
    int s = 0;
    for (long i = lo; i < hi; ++i) s += in[i] + add;
    sh[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    int base = sh[tid] - s;
    for (long i = lo; i < hi; ++i) { out[i] = base; base += in[i] + add; }
    if (tid == 1023) {
        out[n] = sh[1023];
        if (total) total[0] = sh[1023];
    }
}

__global__ __launch_bounds__(256) void csr_count_kernel(const int* __restrict__ idx, long edges, int n, int* __restrict__ cnt) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= edges) return;
    const int j = idx[e];
    if (j >= 0 && j < n) atomicAdd(&cnt[j], 1);
}

// Row i of the unsorted graph: slots 0..k-1 its own list (an index outside [0, n) leaves an INT_MAX column that the merge
// drops), then one slot per in-edge in cursor order.  value(e) = M's entry for edge e = i k + t, in fp64.
template <typename Value>
__global__ __launch_bounds__(256) void csr_scatter_kernel(const int* __restrict__ idx, long edges, int n, int k, Value value,
                                                          const int* __restrict__ ptr, int* __restrict__ fill,
                                                          int* __restrict__ raw_col, double* __restrict__ raw_w) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= edges) return;
    const int i = (int)(e / k), t = (int)(e % k);
    const int j = idx[e];
    const bool ok = j >= 0 && j < n;
    const double aij = value(e);
    const long o = (long)ptr[i] + t;
    raw_col[o] = ok ? j : INT_MAX;
    raw_w[o] = ok ? aij : 0.;
    if (ok) {
        const long pos = (long)ptr[j] + k + atomicAdd(&fill[j], 1);
        raw_col[pos] = i;
        raw_w[pos] = aij;
    }
}

// One wave per row: rank sort by (column, slot) - a row may be as long as k + n - 1 (a hub that is in every list).
__global__ __launch_bounds__(256) void csr_sort_kernel(const int* __restrict__ ptr, int n, const int* __restrict__ raw_col,
                                                       const double* __restrict__ raw_w, int* __restrict__ srt_col,
                                                       double* __restrict__ srt_w) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const long base = ptr[i];
    const int len = ptr[i + 1] - ptr[i];
    for (int e = lane; e < len; e += 64) {
        const int c = raw_col[base + e];
        int rank = 0;
        for (int f = 0; f < len; ++f) {
            const int cf = raw_col[base + f];
            rank += (cf < c || (cf == c && f < e)) ? 1 : 0;
        }
        srt_col[base + rank] = c;
        srt_w[base + rank] = raw_w[base + e];
    }
}

// One wave per sorted row: the first entry of every run of equal columns is a head.  WRITE = false counts the heads,
// WRITE = true writes head columns and the run's sum (a mutual pair: two terms) times `scale` at rowptr[i].
template <bool WRITE, typename W>
__global__ __launch_bounds__(256) void csr_merge_kernel(const int* __restrict__ ptr, int n, const int* __restrict__ srt_col,
                                                        const double* __restrict__ srt_w, int* __restrict__ ucnt,
                                                        const int* __restrict__ rowptr, int* __restrict__ col,
                                                        W* __restrict__ w, double scale) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const long base = ptr[i];
    const int len = ptr[i + 1] - ptr[i];
    int run = 0;
    for (int p0 = 0; p0 < len; p0 += 64) {
        const int p = p0 + lane;
        const bool in = p < len;
        const int c = in ? srt_col[base + p] : INT_MAX;
        const int prev = (in && p > 0) ? srt_col[base + p - 1] : -1;
        const bool head = in && c != INT_MAX && c != prev;
        const unsigned long long m = __ballot(head);
        if (WRITE && head) {
            double s = srt_w[base + p];
            for (int f = p + 1; f < len && srt_col[base + f] == c; ++f) s += srt_w[base + f];
            const long o = (long)rowptr[i] + run + __popcll(m & ((1ull << lane) - 1ull));
            col[o] = c;
            w[o] = (W)(s * scale);
        }
        run += __popcll(m);
    }
    if (!WRITE && lane == 0) ucnt[i] = run;
}

inline long csr_align16(long b) { return (b + 15) / 16 * 16; }

struct CsrSymPlan {
    long edges, cap;
    long off_raw_w, off_srt_w, off_raw_col, off_srt_col, off_cnt, off_fill, off_ptr, off_ucnt, bytes;
};

inline bool csr_sym_plan(int n, int k, CsrSymPlan& p) {
    if (!(n >= 2 && k >= 1 && k <= n - 1 && (long)n * k < (1L << 30))) return false;
    p.edges = (long)n * k;
    p.cap = 2 * p.edges;
    long o = 0;
    p.off_raw_w = o;   o += p.cap * 8;
    p.off_srt_w = o;   o += p.cap * 8;
    p.off_raw_col = o; o += csr_align16(p.cap * 4);
    p.off_srt_col = o; o += csr_align16(p.cap * 4);
    p.off_cnt = o;     o += csr_align16((long)n * 4);
    p.off_fill = o;    o += csr_align16((long)n * 4);            // directly behind cnt: one clear serves both
    p.off_ptr = o;     o += csr_align16(((long)n + 1) * 4);
    p.off_ucnt = o;    o += csr_align16((long)n * 4);
    p.bytes = o;
    return true;
}

// rowptr [n + 1], col / w [2 n k] (capacity; nnz[0] entries are written).  The caller has validated the plan, the pointers
// and the workspace size (p.bytes, 16-byte aligned).
template <typename W, typename Value>
int csr_sym_build(const CsrSymPlan& p, const int* idx, int n, int k, Value value, double scale, int* rowptr, int* col, W* w,
                  int* nnz, void* workspace, hipStream_t s) {
    char* ws = static_cast<char*>(workspace);
    double* raw_w = reinterpret_cast<double*>(ws + p.off_raw_w);
    double* srt_w = reinterpret_cast<double*>(ws + p.off_srt_w);
    int* raw_col = reinterpret_cast<int*>(ws + p.off_raw_col);
    int* srt_col = reinterpret_cast<int*>(ws + p.off_srt_col);
    int* cnt = reinterpret_cast<int*>(ws + p.off_cnt);
    int* fill = reinterpret_cast<int*>(ws + p.off_fill);
    int* ptr = reinterpret_cast<int*>(ws + p.off_ptr);
    int* ucnt = reinterpret_cast<int*>(ws + p.off_ucnt);
    const dim3 rows4((unsigned)(((long)n + 3) / 4));
    ASSL_ZERO_ALWAYS(cnt, (size_t)(p.off_ptr - p.off_cnt), s);                   // cnt and fill are adjacent
    hipLaunchKernelGGL(csr_count_kernel, GRID1(p.edges), dim3(256), 0, s, idx, p.edges, n, cnt);
    hipLaunchKernelGGL(csr_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, k, n, ptr, static_cast<int*>(nullptr));
    hipLaunchKernelGGL(csr_scatter_kernel<Value>, GRID1(p.edges), dim3(256), 0, s, idx, p.edges, n, k, value, ptr, fill, raw_col, raw_w);
    hipLaunchKernelGGL(csr_sort_kernel, rows4, dim3(256), 0, s, ptr, n, raw_col, raw_w, srt_col, srt_w);
    hipLaunchKernelGGL((csr_merge_kernel<false, W>), rows4, dim3(256), 0, s, ptr, n, srt_col, srt_w, ucnt, static_cast<const int*>(nullptr),
                       static_cast<int*>(nullptr), static_cast<W*>(nullptr), scale);
    hipLaunchKernelGGL(csr_scan_kernel, dim3(1), dim3(1024), 0, s, ucnt, 0, n, rowptr, nnz);
    hipLaunchKernelGGL((csr_merge_kernel<true, W>), rows4, dim3(256), 0, s, ptr, n, srt_col, srt_w, static_cast<int*>(nullptr), rowptr, col, w,
                       scale);
    ASSL_LAUNCH_CHECK();
}

}  // namespace
