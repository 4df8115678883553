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
// pic_build: CSR of W = A + A^T, A_ij = exp(-d2_ij / sigma^2) for j in row i's list (fp64 from the fp32 distance), by the
//   builder of csr_sym.h (shared with tsne.hip): columns ascending in every row, a mutual pair merged into one entry
//   a_ij + a_ji.
// pic_power: v = 1/n; iters x { u = alpha W v + (1 - alpha) / n; v = u / sum(u) }: a row's sum in column order by one
//   thread, the global sum in a fixed tree (per-workgroup partials, folded the same way by every workgroup).
// pic_assign: parent(i) = argmax_j W_ij (v_j - v_i) over strictly positive values, ties to the smaller j, else i
//   (`find_maxima_cluster`); roots by pointer doubling (ping-pong, a fixed ceil(log2 n) rounds, nothing read back);
//   roots numbered in ascending node order (the reference's `cluster_ids`).
//
// No float atomics, no grid-wide barriers, plain launches only; the kernels initialise whatever they read of the workspace.
#include "topk.h"
#include "gram_tile.h"
#include "csr_sym.h"

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

// A_ij of edge e = i k + t, in fp64 from the fp32 distance.
struct PicWeight {
    const float* d2;
    double sigma2;
    __device__ double operator()(long e) const { return exp(-(double)d2[e] / sigma2); }
};

struct PicPlan {
    CsrSymPlan build;
    long build_bytes;
    long off_u, off_part, power_bytes;
    long off_pa, off_pb, off_flag, off_cid, assign_bytes;
    long bytes;
    int nparts;
};

bool pic_plan(int n, int k, PicPlan& p) {
    if (!csr_sym_plan(n, k, p.build)) return false;
    p.build_bytes = p.build.bytes;
    p.nparts = (int)(((long)n + 255) / 256);
    long o = 0;
    p.off_u = o;       o += (long)n * 8;
    p.off_part = o;    o += (long)p.nparts * 8;
    p.power_bytes = csr_align16(o);
    o = 0;
    p.off_pa = o;      o += csr_align16((long)n * 4);
    p.off_pb = o;      o += csr_align16((long)n * 4);
    p.off_flag = o;    o += csr_align16((long)n * 4);
    p.off_cid = o;     o += csr_align16(((long)n + 1) * 4);
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
    return csr_sym_build<double>(p.build, idx, n, k, PicWeight{d2, sigma * sigma}, 1.0, rowptr, col, w, nnz, workspace, s);
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
    hipLaunchKernelGGL(csr_scan_kernel, dim3(1), dim3(1024), 0, s, flag, 0, n, cid, count);
    hipLaunchKernelGGL(pic_label_kernel, GRID1(n), dim3(256), 0, s, pa, cid, n, label);
    ASSL_LAUNCH_CHECK();
}
