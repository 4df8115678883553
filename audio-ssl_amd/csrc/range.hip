// Exact range search on the fp32 Gram tile and connected components of the resulting graph: every pair of rows closer than a
// radius (near-duplicate search in one file list, leakage between two), the faiss `range_search` of the reference's stack.  A
// top-k list cannot answer it: a group larger than k is cut off, and a row without a match still gets k neighbours.
//
// range_count / range_fill: the output length is not known before the launch, so the walk runs twice - count, scan, fill.  Owned
//   rows [own_lo, own_hi) against walked rows [walk_lo, walk_hi) of one [n][d] fp32 matrix; d2_ij = max(0, (n_i + n_j) - 2 g_ij)
//   with g_ij from gram_tile<ChainOrder::Index> and n_i from gram_norm_kernel<ChainOrder::Index>: knn_graph_l2's arithmetic
//   (graph.hip), so a repeated row is at distance exactly 0 and d2_ij == d2_ji bit for bit.  i == j leaves by index.  One
//   workgroup per 64 owned rows and split of the walked tiles (blockIdx.y).
//   Count: the compare runs straight on the accumulators (lane column = owned row, registers = walked rows, the map of
//   gram_tile_to_lds); a lane's integer sum goes to LDS once, one store per (row, split) at the end.
//   Scan: one workgroup forms rowptr (exclusive, int32) and the true total (64-bit) from the per-(row, split) counts.
//   Fill: the tile is dumped to LDS; wave w scans owned rows 16 w .. 16 w + 15, 64 walked columns at a time in ascending j, the
//   hits' slots from a ballot prefix; a row's cursor starts at rowptr + the counts of the splits before this one and lives in
//   LDS.  Ascending j is a strict order: the result does not depend on `splits` or on how tiles are walked.
//
// graph_components: weakly connected components of a CSR graph.  Hook: every stored entry (i, j) unites the trees of i and j,
//   the larger root under the smaller by integer compare-and-swap, so a parent is never larger than its child and a tree's root
//   is its smallest member (finds shorten paths with atomicMin: a parent only ever moves rootward).  After that ONE kernel every
//   component is one tree; ceil(log2 n) rounds of pointer doubling (ping-pong) flatten it, roots are numbered in ascending node
//   order.  The forest's shape depends on timing, its roots do not: the result is deterministic.  A bounded number of launches,
//   nothing read back.
//
// No float atomics, no grid-wide barriers, plain launches only; the kernels initialise whatever they read of the workspace.
#include "topk.h"          // plan_splits, TARGET_WG
#include "gram_tile.h"
#include "csr_sym.h"       // csr_scan_kernel, csr_align16

namespace {

constexpr int MAX_SPLITS = 64;
constexpr int COUNT_LDS_BYTES = STAGE_BYTES + 2 * BT * 4 + QT * 4;   // staging + the walked tile's norms (two buffers) + row sums
constexpr int FILL_LDS_BYTES = TILE_BYTES + QT * 4;                  // the Gram tile (over the staging buffers) + row cursors

struct RangeArgs {
    const float* x;          // [n][d]
    const float* gn;         // [n] squared norms in the tile's own chain
    int* cnt;                // [q_tiles * QT][splits]
    const int* rowptr;       // fill: [rows + 1]
    int* col;                // fill
    float* d2;               // fill
    long limit;              // fill: entries that may be written = min(cap, total)
    float r2;
    int n, d;
    int own_lo, own_hi, walk_lo, walk_hi;
    int tiles, tiles_per_split, splits;
};

__global__ __launch_bounds__(256) void range_count_kernel(RangeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Os = reinterpret_cast<float*>(smem);                      // [QT][RP] owned rows
    float* Ws = Os + QT * RP;                                        // [BT][RP] walked rows
    float* Nj = reinterpret_cast<float*>(smem + STAGE_BYTES);        // [2][BT]
    int* Rs = reinterpret_cast<int*>(Nj + 2 * BT);                   // [QT]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const long q0 = (long)a.own_lo + (long)blockIdx.x * QT;
    const int q = (w & 1) * 32 + l31;                                // this lane's owned row (the C/D column)
    const long gq = q0 + q;
    const bool qok = gq < a.own_hi;
    const float ni = qok ? a.gn[gq] : 0.f;
    if (tid < QT) Rs[tid] = 0;

    const int t0 = blockIdx.y * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.tiles);
    int hits = 0;
    for (int t = t0; t < t1; ++t) {
        const long b0 = (long)a.walk_lo + (long)t * BT;
        float* nj = Nj + (t & 1) * BT;                               // the other buffer may still be read by a slower wave
        if (tid < BT) nj[tid] = b0 + tid < a.walk_hi ? a.gn[b0 + tid] : 0.f;
        f32x16 acc[2];
        gram_tile<ChainOrder::Index>(a.x, a.n, a.d, q0, b0, Os, Ws, acc);    // (its barriers publish nj)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 64 * (w >> 1) + 32 * tt + (r & 3) + 8 * (r >> 2) + 4 * half;
                const long j = b0 + c;
                const float dd = fmaxf((ni + nj[c]) - 2.f * acc[tt][r], 0.f);
                hits += (qok && j < a.walk_hi && j != gq && dd <= a.r2) ? 1 : 0;    // self leaves by index, not by value
            }
    }
    __syncthreads();                                                 // Rs is cleared (also when the split walked nothing)
    if (hits) atomicAdd(&Rs[q], hits);                               // integer: four lanes per owned row
    __syncthreads();
    if (tid < QT) a.cnt[((long)blockIdx.x * QT + tid) * a.splits + blockIdx.y] = Rs[tid];
}

// rowptr[i] = matches of the owned rows before i (int32: unspecified once the total passes 2^31), rowptr[rows] and total[0]
// (64-bit) = all of them.  One workgroup: every thread sums a contiguous run of rows, the 1024 run sums are scanned in LDS.
__global__ __launch_bounds__(1024) void range_scan_kernel(const int* __restrict__ cnt, int splits, int rows, int* __restrict__ rowptr,
                                                          long long* __restrict__ total) {
    __shared__ long long sh[1024];
    const int tid = threadIdx.x;
    const long chunk = ((long)rows + 1023) / 1024;
    const long lo = min(tid * chunk, (long)rows), hi = min(lo + chunk, (long)rows);
    long long s = 0;
    for (long i = lo; i < hi; ++i)
        for (int p = 0; p < splits; ++p) s += cnt[i * splits + p];
    sh[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long long t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    long long base = sh[tid] - s;
    for (long i = lo; i < hi; ++i) {
        rowptr[i] = (int)base;
        for (int p = 0; p < splits; ++p) base += cnt[i * splits + p];
    }
    if (tid == 1023) {
        rowptr[rows] = (int)sh[1023];
        total[0] = sh[1023];
    }
}

__global__ __launch_bounds__(256) void range_fill_kernel(RangeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Os = reinterpret_cast<float*>(smem);
    float* Ws = Os + QT * RP;
    float* St = reinterpret_cast<float*>(smem);                      // [QT][SP], over Os / Ws once the feature loop is done
    int* Cur = reinterpret_cast<int*>(smem + TILE_BYTES);            // [QT] next free slot of the row, relative to rowptr
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long q0 = (long)a.own_lo + (long)blockIdx.x * QT;
    const int rows = a.own_hi - a.own_lo;

    if (tid < QT) {                                                  // the splits before this one come first in the row
        const long lr = (long)blockIdx.x * QT + tid;
        int c = 0;
        for (int p = 0; p < (int)blockIdx.y; ++p) c += a.cnt[lr * a.splits + p];
        Cur[tid] = c;
    }

    const int t0 = blockIdx.y * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.tiles);
    for (int t = t0; t < t1; ++t) {
        const long b0 = (long)a.walk_lo + (long)t * BT;
        f32x16 acc[2];
        gram_tile<ChainOrder::Index>(a.x, a.n, a.d, q0, b0, Os, Ws, acc);    // (its first barrier: Cur is set, the previous scan is done)
        gram_tile_to_lds(acc, St);

        const long r0 = b0 + lane, r1 = b0 + 64 + lane;
        const bool ok0 = r0 < a.walk_hi, ok1 = r1 < a.walk_hi;
        const float nj0 = ok0 ? a.gn[r0] : 0.f, nj1 = ok1 ? a.gn[r1] : 0.f;
        for (int qq = 0; qq < 16; ++qq) {
            const int q = 16 * w + qq;
            const long lr = (long)blockIdx.x * QT + q;
            if (lr >= rows) break;                                   // uniform over the wave
            const long gq = q0 + q;
            const float ni = a.gn[gq];
            const long base = (long)a.rowptr[lr];
            int cur = Cur[q];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const long j = h ? r1 : r0;
                const float dd = fmaxf((ni + (h ? nj1 : nj0)) - 2.f * St[q * SP + 64 * h + lane], 0.f);
                const bool hit = (h ? ok1 : ok0) && j != gq && dd <= a.r2;
                const unsigned long long m = __ballot(hit);
                const long o = base + cur + __popcll(m & ((1ull << lane) - 1ull));
                if (hit && o >= 0 && o < a.limit) {
                    a.col[o] = (int)j;
                    a.d2[o] = dd;
                }
                cur += __popcll(m);
            }
            if (lane == 0) Cur[q] = cur;                             // rows 16 w .. belong to this wave alone
        }
    }
}

struct RangePlan {
    long q_tiles, rows_pad;
    int rows, tiles, splits, tiles_per_split;
    long off_cnt, bytes;
};

inline long range_cnt_slots(long q_tiles, int splits) {
    // the library's own choice never exceeds ceil(TARGET_WG / q_tiles) and MAX_SPLITS; a forced value is taken as it is
    const long a = q_tiles + TARGET_WG - 1, b = q_tiles * MAX_SPLITS;
    const long own = a < b ? a : b, forced = q_tiles * (long)(splits > 0 ? splits : 1);
    return own > forced ? own : forced;
}

bool range_plan(int n, int own_lo, int own_hi, int walk_lo, int walk_hi, int splits, RangePlan& p) {
    if (!(n >= 1 && 0 <= own_lo && own_lo < own_hi && own_hi <= n && 0 <= walk_lo && walk_lo < walk_hi && walk_hi <= n)) return false;
    if (!(splits >= 0 && splits <= MAX_SPLITS)) return false;
    p.rows = own_hi - own_lo;
    p.q_tiles = ((long)p.rows + QT - 1) / QT;
    p.rows_pad = p.q_tiles * QT;
    p.tiles = (int)(((long)(walk_hi - walk_lo) + BT - 1) / BT);
    if (splits == 0) {
        const SplitPlan sp = plan_splits(p.q_tiles, p.tiles, 4);
        p.splits = sp.splits < MAX_SPLITS ? sp.splits : MAX_SPLITS;
    } else {
        p.splits = splits < p.tiles ? splits : p.tiles;
    }
    p.tiles_per_split = (p.tiles + p.splits - 1) / p.splits;
    p.splits = (p.tiles + p.tiles_per_split - 1) / p.tiles_per_split;              // no empty split
    p.off_cnt = csr_align16((long)n * 4);
    p.bytes = p.off_cnt + range_cnt_slots(p.q_tiles, splits) * QT * 4;
    return true;
}

bool finite_nonnegative(float x) { return x >= 0.f && x < __builtin_inff(); }       // NaN fails both comparisons

void range_args(RangeArgs& a, const RangePlan& p, const float* x, int n, int d, int own_lo, int own_hi, int walk_lo, int walk_hi,
                float r2, void* workspace) {
    a.x = x;
    a.gn = static_cast<const float*>(workspace);
    a.cnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + p.off_cnt);
    a.rowptr = nullptr; a.col = nullptr; a.d2 = nullptr; a.limit = 0;
    a.r2 = r2;
    a.n = n; a.d = d;
    a.own_lo = own_lo; a.own_hi = own_hi; a.walk_lo = walk_lo; a.walk_hi = walk_hi;
    a.tiles = p.tiles; a.tiles_per_split = p.tiles_per_split; a.splits = p.splits;
}

// ---- components -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void cc_init_kernel(int* __restrict__ parent, int n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}

// Root of v's tree.  A parent is an ancestor that only ever moves rootward, so a stale read is still an ancestor; every step
// hands v its grandparent (atomicMin: ancestors are ordered by index along a root path).
__device__ __forceinline__ int cc_find(int* parent, int v) {
    int p = __atomic_load_n(&parent[v], __ATOMIC_RELAXED);
    while (p != v) {
        const int g = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
        if (g != p) atomicMin(&parent[v], g);
        v = p;
        p = g;
    }
    return v;
}

// One wave per row; every stored entry (i, j) unites i and j.  A failed compare-and-swap means another hook moved that root:
// follow it and try again - each success removes a root, so the loop ends.
__global__ __launch_bounds__(256) void cc_hook_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, int n, long cap,
                                                      int* __restrict__ parent) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const long l0 = max((long)rowptr[i], 0L), l1 = min((long)rowptr[i + 1], cap);
    for (long l = l0 + lane; l < l1; l += 64) {
        const int j = col[l];
        if (j < 0 || j >= n || j == (int)i) continue;
        int a = cc_find(parent, (int)i), b = cc_find(parent, j);
        while (a != b) {
            const int hi = a > b ? a : b, lo = a > b ? b : a;
            const int old = atomicCAS(&parent[hi], hi, lo);
            if (old == hi) break;
            a = cc_find(parent, old);
            b = cc_find(parent, lo);
        }
    }
}

__global__ __launch_bounds__(256) void cc_jump_kernel(const int* __restrict__ in, int n, int* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[in[i]];
}

__global__ __launch_bounds__(256) void cc_root_flag_kernel(const int* __restrict__ root, int n, int* __restrict__ flag) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = root[i] == (int)i ? 1 : 0;
}

__global__ __launch_bounds__(256) void cc_label_kernel(const int* __restrict__ root, const int* __restrict__ cid, int n,
                                                       int* __restrict__ label) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) label[i] = cid[root[i]];
}

struct CcPlan {
    long off_pa, off_pb, off_flag, off_cid, bytes;
};

bool cc_plan(int n, CcPlan& p) {
    if (n < 1) return false;
    long o = 0;
    p.off_pa = o;      o += csr_align16((long)n * 4);
    p.off_pb = o;      o += csr_align16((long)n * 4);
    p.off_flag = o;    o += csr_align16((long)n * 4);
    p.off_cid = o;     o += csr_align16(((long)n + 1) * 4);
    p.bytes = o;
    return true;
}

}  // namespace

extern "C" int audiossl_range_workspace(int n, int rows, int splits, long* bytes) {
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(n >= 1 && rows >= 1 && rows <= n && splits >= 0 && splits <= MAX_SPLITS);
    const long q_tiles = ((long)rows + QT - 1) / QT;
    *bytes = csr_align16((long)n * 4) + range_cnt_slots(q_tiles, splits) * QT * 4;
    return ASSL_OK;
}

extern "C" int audiossl_range_count(const float* x, int n, int d, int own_lo, int own_hi, int walk_lo, int walk_hi, float r2,
                                    int splits, int* rowptr, long long* total, void* workspace, long workspace_bytes, void* stream) {
    RangePlan p;
    ASSL_REQUIRE(x && rowptr && total && workspace);
    ASSL_REQUIRE(gram_width_ok(d));
    ASSL_REQUIRE(range_plan(n, own_lo, own_hi, walk_lo, walk_hi, splits, p));
    ASSL_REQUIRE(finite_nonnegative(r2));
    ASSL_REQUIRE(workspace_bytes >= p.bytes);
    if (!ASSL_ALIGNED16(x) || !ASSL_ALIGNED16(workspace) || (((uintptr_t)total) & 7) != 0) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    RangeArgs a;
    range_args(a, p, x, n, d, own_lo, own_hi, walk_lo, walk_hi, r2, workspace);
    hipLaunchKernelGGL(gram_norm_kernel<ChainOrder::Index>, GRID1(n), dim3(256), 0, s, x, n, d, (long)n, static_cast<float*>(workspace));
    hipLaunchKernelGGL(range_count_kernel, dim3((unsigned)p.q_tiles, (unsigned)p.splits), dim3(256), COUNT_LDS_BYTES, s, a);
    hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(1024), 0, s, a.cnt, p.splits, p.rows, rowptr, total);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_range_fill(const float* x, int n, int d, int own_lo, int own_hi, int walk_lo, int walk_hi, float r2,
                                   int splits, const int* rowptr, long long total, int* col, float* d2, long cap, void* workspace,
                                   long workspace_bytes, void* stream) {
    RangePlan p;
    ASSL_REQUIRE(x && rowptr && col && d2 && workspace);
    ASSL_REQUIRE(gram_width_ok(d));
    ASSL_REQUIRE(range_plan(n, own_lo, own_hi, walk_lo, walk_hi, splits, p));
    ASSL_REQUIRE(finite_nonnegative(r2));
    ASSL_REQUIRE(total >= 0 && total < (1LL << 31) && cap >= total);
    ASSL_REQUIRE(workspace_bytes >= p.bytes);
    if (!ASSL_ALIGNED16(x) || !ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    RangeArgs a;
    range_args(a, p, x, n, d, own_lo, own_hi, walk_lo, walk_hi, r2, workspace);
    a.rowptr = rowptr; a.col = col; a.d2 = d2; a.limit = (long)total;
    hipLaunchKernelGGL(range_fill_kernel, dim3((unsigned)p.q_tiles, (unsigned)p.splits), dim3(256), FILL_LDS_BYTES, s, a);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_graph_components_workspace(int n, long* bytes) {
    CcPlan p;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(cc_plan(n, p));
    *bytes = p.bytes;
    return ASSL_OK;
}

extern "C" int audiossl_graph_components(const int* rowptr, const int* col, int n, long cap, int* label, int* count, void* workspace,
                                         long workspace_bytes, void* stream) {
    CcPlan p;
    ASSL_REQUIRE(rowptr && label && count && workspace);
    ASSL_REQUIRE(cc_plan(n, p));
    ASSL_REQUIRE(cap >= 0 && (col != nullptr || cap == 0));
    ASSL_REQUIRE(workspace_bytes >= p.bytes);
    if (!ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    char* ws = static_cast<char*>(workspace);
    int* pa = reinterpret_cast<int*>(ws + p.off_pa);
    int* pb = reinterpret_cast<int*>(ws + p.off_pb);
    int* flag = reinterpret_cast<int*>(ws + p.off_flag);
    int* cid = reinterpret_cast<int*>(ws + p.off_cid);
    hipLaunchKernelGGL(cc_init_kernel, GRID1(n), dim3(256), 0, s, pa, n);
    if (cap > 0) hipLaunchKernelGGL(cc_hook_kernel, dim3((unsigned)(((long)n + 3) / 4)), dim3(256), 0, s, rowptr, col, n, cap, pa);
    int rounds = 0;
    while ((1L << rounds) < n) ++rounds;                             // ceil(log2 n): a tree is at most n - 1 deep
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(cc_jump_kernel, GRID1(n), dim3(256), 0, s, pa, n, pb);
        int* t = pa; pa = pb; pb = t;
    }
    hipLaunchKernelGGL(cc_root_flag_kernel, GRID1(n), dim3(256), 0, s, pa, n, flag);
    hipLaunchKernelGGL(csr_scan_kernel, dim3(1), dim3(1024), 0, s, flag, 0, n, cid, count);
    hipLaunchKernelGGL(cc_label_kernel, GRID1(n), dim3(256), 0, s, pa, cid, n, label);
    ASSL_LAUNCH_CHECK();
}
