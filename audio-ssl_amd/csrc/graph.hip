// Power-iteration clustering (PIC) on a nearest-neighbour graph: the second algorithm of the reference's
// `extras/decar-v2/clustering.py:118-295` (DeepCluster's PIC), the one that finds the number of clusters itself.  The reference
// builds the graph with faiss and walks it with scipy / Python loops; here every stage is a kernel.
//
// knn_graph_l2: exact k nearest neighbours of n points among themselves, squared L2, fp32 END TO END.  The graph is a discrete
//   input to everything after it and on whitened, normalised features the gaps between neighbours are ~1e-4 of the squared
//   norm: far below bf16 resolution, so knn.hip's bf16 similarity does not serve.  g_ij = <x_i, x_j> is the fp32 Gram tile of
//   gram_tile.h in index chain order, n_i = g_ii its norm kernel, so d2_ij = max(0, (n_i + n_j) - 2 g_ij) is exactly 0
//   wherever row j repeats row i.  What this file adds on top of the tile: the 64 x 128 tile is dumped to LDS and wave w
//   scans rows 16w..16w+15 with the streaming selector of topk.h (k <= 64: the one-slot list), order (d2 ascending,
//   j ascending).  Self is excluded by INDEX, so a duplicate row is a legitimate neighbour at distance 0.  Few rows: the
//   walked rows are split over blockIdx.y, every split writes its k best to the workspace, topk_merge_kernel folds them.
//
// pic_build: CSR of W = A + A^T, A_ij = exp(-d2_ij / sigma^2) for j in row i's list (fp64 from the fp32 distance): count
//   in-degrees (integer atomics), scan, scatter (out-edges at fixed slots, in-edges through an integer cursor), then each
//   row is sorted by column (rank sort: any in-degree up to n - 1 works) and a mutual pair merged into one entry
//   a_ij + a_ji - two terms, so the order in which the cursor handed out slots does not reach the result.
// pic_power: v = 1/n; iters x { u = alpha W v + (1 - alpha) / n; v = u / sum(u) }: a row's sum in column order by one
//   thread, the global sum in a fixed tree (per-workgroup partials, folded the same way by every workgroup).
// pic_assign: parent(i) = argmax_j W_ij (v_j - v_i) over strictly positive values, ties to the smaller j, else i
//   (`find_maxima_cluster`); roots by pointer doubling (ping-pong, a fixed ceil(log2 n) rounds, nothing read back);
//   roots numbered in ascending node order (the reference's `cluster_ids`).
//
// No float atomics, no grid-wide barriers, plain launches only; the kernels initialise whatever they read of the workspace.
#include "topk.h"
#include "gram_tile.h"

namespace {

constexpr int KP = 64;               // list slots per row: one per lane
constexpr int LDS_BYTES = TILE_BYTES + QT * KP * 8;      // the Gram tile (over the staging buffers) + the rows' lists

struct GraphArgs {
    const float* x;      // [n][d]
    const float* gn;     // [n] squared norms in the tile's own chain
    float* out_v;        // [splits][n][k]  (the caller's d2 when splits == 1)
    int* out_i;
    long split_stride;   // n * k
    int n, d, k;
    int tiles, tiles_per_split;
};

__global__ __launch_bounds__(256) void graph_topk_kernel(GraphArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Os = reinterpret_cast<float*>(smem);                      // [QT][RP] owned rows
    float* Ws = Os + QT * RP;                                        // [BT][RP] walked rows
    float* St = reinterpret_cast<float*>(smem);                      // [QT][SP], over Os / Ws once the feature loop is done
    float* Lv = reinterpret_cast<float*>(smem + TILE_BYTES);         // [QT][KP]
    int* Li = reinterpret_cast<int*>(Lv + QT * KP);                  // [QT][KP]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long q0 = (long)blockIdx.x * QT;
    const int n = a.n, k = a.k;

    topk_lds_init<QT, KP, DistAscending>(Lv, Li);

    const int t0 = blockIdx.y * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.tiles);

    for (int t = t0; t < t1; ++t) {
        const long b0 = (long)t * BT;
        f32x16 acc[2];
        gram_tile<ChainOrder::Index>(a.x, n, a.d, q0, b0, Os, Ws, acc);      // (its first barrier: the previous tile's scan is done)
        gram_tile_to_lds(acc, St);

        const long r0 = b0 + lane, r1 = b0 + 64 + lane;
        const bool ok0 = r0 < n, ok1 = r1 < n;
        const int i0 = (int)r0, i1 = (int)r1;
        const float nj0 = ok0 ? a.gn[r0] : 0.f, nj1 = ok1 ? a.gn[r1] : 0.f;
        topk_lds_scan<QT, KP, DistAscending>(Lv, Li, k, q0, n, lane, w, [&](int q, int h) {
            const long gq = q0 + q;
            const float ni = a.gn[gq];
            const float dd = fmaxf((ni + (h ? nj1 : nj0)) - 2.f * St[q * SP + 64 * h + lane], 0.f);
            return TopCand{dd, h ? i1 : i0, h ? ok1 && r1 != gq : ok0 && r0 != gq};   // self leaves by index, not by value
        });
    }

    topk_lds_write<QT, KP>(Lv, Li, k, q0, n, lane, w, a.out_v + (long)blockIdx.y * a.split_stride,
                           a.out_i + (long)blockIdx.y * a.split_stride);
}

struct GraphPlan {
    long q_tiles;
    int tiles, splits, tiles_per_split;
    long n_pad, ws_bytes;
};

// Splits (plan_splits): at least four walked tiles each.  The workspace figure is a bound on splits * n * k * 8 that grows
// with n and with k.
bool graph_plan(int n, int k, GraphPlan& p) {
    if (!(n >= 2 && k >= 1 && k <= KP && k <= n - 1 && (long)n * k < (1L << 31))) return false;
    p.q_tiles = ((long)n + QT - 1) / QT;
    p.tiles = (int)(((long)n + BT - 1) / BT);
    const SplitPlan sp = plan_splits(p.q_tiles, p.tiles, 4);
    p.splits = sp.splits;
    p.tiles_per_split = sp.tiles_per_split;
    p.n_pad = p.q_tiles * QT;
    const long a = p.q_tiles + TARGET_WG - 1, b = p.q_tiles * sp.max_splits;
    p.ws_bytes = p.n_pad * 4 + (a < b ? a : b) * QT * (long)k * 8;
    return true;
}

// ---- PIC ------------------------------------------------------------------------------------------------------------------

// out[i] = sum over t < i of (in[t] + add), out[n] = the total (also to *total when given).  One workgroup: every thread
// sums a contiguous run, the 1024 run sums are scanned in LDS.
__global__ __launch_bounds__(1024) void pic_scan_kernel(const int* __restrict__ in, int add, int n, int* __restrict__ out,
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

__global__ __launch_bounds__(256) void pic_count_kernel(const int* __restrict__ idx, long edges, int n, int* __restrict__ cnt) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= edges) return;
    const int j = idx[e];
    if (j >= 0 && j < n) atomicAdd(&cnt[j], 1);
}

// Row i of the unsorted graph: slots 0..k-1 its own list (an index outside [0, n) leaves an INT_MAX column that the merge
// drops), then one slot per in-edge in cursor order.
__global__ __launch_bounds__(256) void pic_scatter_kernel(const int* __restrict__ idx, const float* __restrict__ d2, long edges, int n,
                                                          int k, double sigma2, const int* __restrict__ ptr, int* __restrict__ fill,
                                                          int* __restrict__ raw_col, double* __restrict__ raw_w) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= edges) return;
    const int i = (int)(e / k), t = (int)(e % k);
    const int j = idx[e];
    const bool ok = j >= 0 && j < n;
    const double aij = exp(-(double)d2[e] / sigma2);
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
__global__ __launch_bounds__(256) void pic_sort_kernel(const int* __restrict__ ptr, int n, const int* __restrict__ raw_col,
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
// WRITE = true writes head columns and the run's sum (a mutual pair: two terms) at rowptr[i].
template <bool WRITE>
__global__ __launch_bounds__(256) void pic_merge_kernel(const int* __restrict__ ptr, int n, const int* __restrict__ srt_col,
                                                        const double* __restrict__ srt_w, int* __restrict__ ucnt,
                                                        const int* __restrict__ rowptr, int* __restrict__ col,
                                                        double* __restrict__ w) {
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
            w[o] = s;
        }
        run += __popcll(m);
    }
    if (!WRITE && lane == 0) ucnt[i] = run;
}

__global__ __launch_bounds__(256) void pic_fill_kernel(double* __restrict__ v, int n, double value) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = value;
}

// u_i = alpha sum_j W_ij v_j + (1 - alpha) / n: one thread per row, terms in column order; the workgroup's sum of u to part.
__global__ __launch_bounds__(256) void pic_spmv_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       const double* __restrict__ w, const double* __restrict__ v, int n, long cap,
                                                       double alpha, double shift, double* __restrict__ u, double* __restrict__ part) {
    __shared__ double sh[16];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    double ui = 0.;
    if (i < n) {
        const long l0 = max((long)rowptr[i], 0L), l1 = min((long)rowptr[i + 1], cap);
        double s = 0.;
        for (long l = l0; l < l1; ++l) {
            const int j = col[l];
            if (j >= 0 && j < n) s += w[l] * v[j];
        }
        ui = alpha * s + shift;
        u[i] = ui;
    }
    const double t = block_sum(ui, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// v = u / sum(u): every workgroup folds the partials in the same fixed order.
__global__ __launch_bounds__(256) void pic_scale_kernel(const double* __restrict__ u, const double* __restrict__ part, int nparts, int n,
                                                        double* __restrict__ v) {
    __shared__ double sh[16];
    double s = 0.;
    for (int b = threadIdx.x; b < nparts; b += 256) s += part[b];
    const double total = block_sum(s, sh);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = u[i] / total;
}

__global__ __launch_bounds__(256) void pic_parent_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const double* __restrict__ w, const double* __restrict__ v, int n, long cap,
                                                         int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long l0 = max((long)rowptr[i], 0L), l1 = min((long)rowptr[i + 1], cap);
    const double vi = v[i];
    double best = 0.;
    int p = (int)i;
    for (long l = l0; l < l1; ++l) {
        const int j = col[l];
        if (j < 0 || j >= n) continue;
        const double val = w[l] * (v[j] - vi);
        if (val > best) { best = val; p = j; }                      // columns ascend: a tie stays with the smaller j
    }
    parent[i] = p;
}

__global__ __launch_bounds__(256) void pic_jump_kernel(const int* __restrict__ in, int n, int* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[in[i]];
}

__global__ __launch_bounds__(256) void pic_root_flag_kernel(const int* __restrict__ root, int n, int* __restrict__ flag) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = root[i] == (int)i ? 1 : 0;
}

__global__ __launch_bounds__(256) void pic_label_kernel(const int* __restrict__ root, const int* __restrict__ cid, int n,
                                                        int* __restrict__ label) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) label[i] = cid[root[i]];
}

long align16(long b) { return (b + 15) / 16 * 16; }

struct PicPlan {
    long edges, cap;
    long off_raw_w, off_srt_w, off_raw_col, off_srt_col, off_cnt, off_fill, off_ptr, off_ucnt, build_bytes;
    long off_u, off_part, power_bytes;
    long off_pa, off_pb, off_flag, off_cid, assign_bytes;
    long bytes;
    int nparts;
};

bool pic_plan(int n, int k, PicPlan& p) {
    if (!(n >= 2 && k >= 1 && k <= n - 1 && (long)n * k < (1L << 30))) return false;
    p.edges = (long)n * k;
    p.cap = 2 * p.edges;
    long o = 0;
    p.off_raw_w = o;   o += p.cap * 8;
    p.off_srt_w = o;   o += p.cap * 8;
    p.off_raw_col = o; o += align16(p.cap * 4);
    p.off_srt_col = o; o += align16(p.cap * 4);
    p.off_cnt = o;     o += align16((long)n * 4);
    p.off_fill = o;    o += align16((long)n * 4);            // directly behind cnt: one clear serves both
    p.off_ptr = o;     o += align16(((long)n + 1) * 4);
    p.off_ucnt = o;    o += align16((long)n * 4);
    p.build_bytes = o;
    p.nparts = (int)(((long)n + 255) / 256);
    o = 0;
    p.off_u = o;       o += (long)n * 8;
    p.off_part = o;    o += (long)p.nparts * 8;
    p.power_bytes = align16(o);
    o = 0;
    p.off_pa = o;      o += align16((long)n * 4);
    p.off_pb = o;      o += align16((long)n * 4);
    p.off_flag = o;    o += align16((long)n * 4);
    p.off_cid = o;     o += align16(((long)n + 1) * 4);
    p.assign_bytes = o;
    p.bytes = p.build_bytes > p.power_bytes ? p.build_bytes : p.power_bytes;
    if (p.assign_bytes > p.bytes) p.bytes = p.assign_bytes;
    return true;
}

bool finite_positive(double x) { return x > 0. && x < __builtin_inf(); }      // NaN fails both comparisons

}  // namespace

extern "C" int audiossl_knn_graph_workspace(int n, int k, long* bytes) {
    GraphPlan p;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(graph_plan(n, k, p));
    *bytes = p.ws_bytes;
    return ASSL_OK;
}

extern "C" int audiossl_knn_graph_l2(const float* x, int n, int d, int k, int* idx, float* d2, void* workspace, long workspace_bytes,
                                     void* stream) {
    GraphPlan p;
    ASSL_REQUIRE(x && idx && d2 && workspace);
    ASSL_REQUIRE(gram_width_ok(d));
    ASSL_REQUIRE(graph_plan(n, k, p));
    ASSL_REQUIRE(workspace_bytes >= p.ws_bytes);
    if (!ASSL_ALIGNED16(x) || !ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    if (!allow_dynamic_lds<graph_topk_kernel>(LDS_BYTES)) return ASSL_ELAUNCH;
    float* gn = static_cast<float*>(workspace);
    GraphArgs a;
    a.x = x; a.gn = gn;
    a.n = n; a.d = d; a.k = k;
    a.tiles = p.tiles; a.tiles_per_split = p.tiles_per_split;
    a.split_stride = (long)n * k;
    float* wv = gn + p.n_pad;
    int* wi = reinterpret_cast<int*>(wv + (long)p.splits * a.split_stride);
    a.out_v = p.splits == 1 ? d2 : wv;
    a.out_i = p.splits == 1 ? idx : wi;
    hipLaunchKernelGGL(gram_norm_kernel<ChainOrder::Index>, GRID1(p.n_pad), dim3(256), 0, s, x, n, d, p.n_pad, gn);
    hipLaunchKernelGGL(graph_topk_kernel, dim3((unsigned)p.q_tiles, (unsigned)p.splits), dim3(256), LDS_BYTES, s, a);
    if (p.splits > 1)
        hipLaunchKernelGGL((topk_merge_kernel<KP, DistAscending>), dim3((unsigned)(((long)n + 3) / 4)), dim3(256), 0, s, wv, wi, p.splits,
                           a.split_stride, n, k, d2, idx);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_pic_workspace(int n, int k, long* bytes) {
    PicPlan p;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(pic_plan(n, k, p));
    *bytes = p.bytes;
    return ASSL_OK;
}

extern "C" int audiossl_pic_build(const int* idx, const float* d2, int n, int k, double sigma, int* rowptr, int* col, double* w,
                                  int* nnz, void* workspace, long workspace_bytes, void* stream) {
    PicPlan p;
    ASSL_REQUIRE(idx && d2 && rowptr && col && w && nnz && workspace);
    ASSL_REQUIRE(pic_plan(n, k, p));
    ASSL_REQUIRE(finite_positive(sigma));
    ASSL_REQUIRE(workspace_bytes >= p.build_bytes);
    if (!ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
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
    hipLaunchKernelGGL(pic_count_kernel, GRID1(p.edges), dim3(256), 0, s, idx, p.edges, n, cnt);
    hipLaunchKernelGGL(pic_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, k, n, ptr, static_cast<int*>(nullptr));
    hipLaunchKernelGGL(pic_scatter_kernel, GRID1(p.edges), dim3(256), 0, s, idx, d2, p.edges, n, k, sigma * sigma, ptr, fill, raw_col,
                       raw_w);
    hipLaunchKernelGGL(pic_sort_kernel, rows4, dim3(256), 0, s, ptr, n, raw_col, raw_w, srt_col, srt_w);
    hipLaunchKernelGGL(pic_merge_kernel<false>, rows4, dim3(256), 0, s, ptr, n, srt_col, srt_w, ucnt, static_cast<const int*>(nullptr),
                       static_cast<int*>(nullptr), static_cast<double*>(nullptr));
    hipLaunchKernelGGL(pic_scan_kernel, dim3(1), dim3(1024), 0, s, ucnt, 0, n, rowptr, nnz);
    hipLaunchKernelGGL(pic_merge_kernel<true>, rows4, dim3(256), 0, s, ptr, n, srt_col, srt_w, static_cast<int*>(nullptr), rowptr, col, w);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_pic_power(const int* rowptr, const int* col, const double* w, int n, long cap, double alpha, int iters,
                                  double* v, void* workspace, long workspace_bytes, void* stream) {
    PicPlan p;
    ASSL_REQUIRE(rowptr && col && w && v && workspace);
    ASSL_REQUIRE(pic_plan(n, 1, p));
    ASSL_REQUIRE(cap >= 0 && iters >= 0 && iters <= 100000 && alpha >= 0. && alpha < __builtin_inf());
    ASSL_REQUIRE(workspace_bytes >= p.power_bytes);
    if (!ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    char* ws = static_cast<char*>(workspace);
    double* u = reinterpret_cast<double*>(ws + p.off_u);
    double* part = reinterpret_cast<double*>(ws + p.off_part);
    hipLaunchKernelGGL(pic_fill_kernel, GRID1(n), dim3(256), 0, s, v, n, 1.0 / (double)n);
    const double shift = (1.0 - alpha) / (double)n;
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(pic_spmv_kernel, dim3((unsigned)p.nparts), dim3(256), 0, s, rowptr, col, w, v, n, cap, alpha, shift, u, part);
        hipLaunchKernelGGL(pic_scale_kernel, dim3((unsigned)p.nparts), dim3(256), 0, s, u, part, p.nparts, n, v);
    }
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_pic_assign(const int* rowptr, const int* col, const double* w, const double* v, int n, long cap, int* label,
                                   int* count, void* workspace, long workspace_bytes, void* stream) {
    PicPlan p;
    ASSL_REQUIRE(rowptr && col && w && v && label && count && workspace);
    ASSL_REQUIRE(pic_plan(n, 1, p));
    ASSL_REQUIRE(cap >= 0);
    ASSL_REQUIRE(workspace_bytes >= p.assign_bytes);
    if (!ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    char* ws = static_cast<char*>(workspace);
    int* pa = reinterpret_cast<int*>(ws + p.off_pa);
    int* pb = reinterpret_cast<int*>(ws + p.off_pb);
    int* flag = reinterpret_cast<int*>(ws + p.off_flag);
    int* cid = reinterpret_cast<int*>(ws + p.off_cid);
    hipLaunchKernelGGL(pic_parent_kernel, GRID1(n), dim3(256), 0, s, rowptr, col, w, v, n, cap, pa);
    int rounds = 0;
    while ((1L << rounds) < n) ++rounds;                             // ceil(log2 n): a path has at most n - 1 pointers
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(pic_jump_kernel, GRID1(n), dim3(256), 0, s, pa, n, pb);
        int* t = pa; pa = pb; pb = t;
    }
    hipLaunchKernelGGL(pic_root_flag_kernel, GRID1(n), dim3(256), 0, s, pa, n, flag);
    hipLaunchKernelGGL(pic_scan_kernel, dim3(1), dim3(1024), 0, s, flag, 0, n, cid, count);
    hipLaunchKernelGGL(pic_label_kernel, GRID1(n), dim3(256), 0, s, pa, cid, n, label);
    ASSL_LAUNCH_CHECK();
}
