// t-SNE (van der Maaten & Hinton 2008) of a feature matrix into the plane, with sklearn's parameters and schedule
// (`sklearn.manifold.TSNE`): sparse affinities on each point's nearest neighbours as in its `barnes_hut` path, EXACT repulsion
// (what `angle = 0` would give).  The neighbour lists come from knn_graph_l2 (graph.hip); nothing here holds n x n numbers.
//
// tsne_calibrate: one wave per row, lane t holds d2[i][t] minus the row's smallest distance (P is unchanged by the shift and
//   no row underflows to 0 / 0).  The bisection of `_binary_search_perplexity`: beta = 1, doubled / halved while a bound is
//   infinite, the midpoint after that, at most 100 steps, stop at |H - log(perplexity)| <= 1e-5; search and sums in fp64.  H
//   is the entropy -sum p log p of the row AS STORED (rounded to fp32), so the row that is written meets the tolerance itself;
//   sklearn's log(sum) + beta sum(d p) / sum is the same number before that rounding, 1e-8 away.  A row of equal distances
//   (duplicates of one point) ends after its 100 steps as the uniform row 1 / k.
// tsne_symmetrize: P = (P_cond + P_cond^T) / (2 n) in CSR by the builder of csr_sym.h (shared with pic_build).
// tsne_repulsion: rep_i = sum_{j != i} w_ij^2 (y_i - y_j), Z = sum_{i != j} w_ij, w_ij = 1 / (1 + |y_i - y_j|^2): all pairs, VALU
//   work.  A workgroup owns 256 points (one per lane, in registers) and walks a range of 256-point tiles staged in LDS; every
//   lane of a wave reads the same y_j (a broadcast).  The walked range is split over blockIdx.y so that several waves share a
//   SIMD.  Sums are fp32 inside one tile and fp64 across tiles.  The one tile that holds the owned points themselves drops
//   (i, i) by index; a coincident other point contributes w = 1 and force 0.  1 / x is the hardware reciprocal plus one Newton
//   step (x >= 1: no denormals), which is within an ulp of the correctly rounded quotient at 3 instructions.  The S partial
//   forces and the per-workgroup Z parts go to the workspace and are folded in a fixed order by tsne_fold_kernel.
// tsne_gradient: one wave per CSR row: att_i = sum_j p_ij w_ij (y_i - y_j), grad_i = 4 (exaggeration att_i - rep_i / Z); the
//   optional KL = sum_ij p_ij log(p_ij Z / w_ij) with log and sum in fp64 (per-workgroup parts, one fixed-order fold).
// tsne_update: sklearn's `_gradient_descent` rule on y, update and gains, elementwise in fp32.
//
// No float atomics, no grid-wide barriers, plain launches only; the kernels initialise whatever they read of the workspace;
// two calls on the same input give the same bits.
#include "csr_sym.h"

namespace {

constexpr int MAX_K = 64;            // knn_graph_l2's list length: one lane per neighbour
constexpr int TP = 256;              // points a workgroup owns = points per staged tile
constexpr int TARGET_WG = 2048;      // 256 CUs x 8 workgroups of 4 waves: two waves per SIMD and a second round to even the tail
constexpr int MAX_SPLITS = 32;

// ---- calibration ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_calibrate_kernel(const float* __restrict__ d2, int n, int k, double target,
                                                             float* __restrict__ p_cond, float* __restrict__ beta_out) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                              // whole waves leave: the shuffles below see full waves
    const bool in = lane < k;
    const float raw = in ? d2[i * k + lane] : __builtin_inff();
    float lo = raw;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o, 64));
    const double d = in ? (double)raw - (double)lo : 0.;
    double beta = 1., bmin = -__builtin_inf(), bmax = __builtin_inf();
    float row = 0.f;
    for (int step = 0; step < 100; ++step) {
        const double p = in ? exp(-d * beta) : 0.;
        row = (float)(p / wave_sum(p));                              // the sum is >= 1: the nearest neighbour's term is exp(0)
        const double r = (double)row;
        const double diff = -wave_sum(row > 0.f ? r * log(r) : 0.) - target;
        if (fabs(diff) <= 1e-5) break;
        if (diff > 0.) {
            bmin = beta;
            beta = bmax == __builtin_inf() ? beta * 2. : (beta + bmax) / 2.;
        } else {
            bmax = beta;
            beta = bmin == -__builtin_inf() ? beta / 2. : (beta + bmin) / 2.;
        }
    }
    if (in) p_cond[i * k + lane] = row;
    if (lane == 0) beta_out[i] = (float)beta;
}

// M_ij of edge e for csr_sym.h: the conditional probability itself.
struct CondValue {
    const float* p_cond;
    __device__ double operator()(long e) const { return (double)p_cond[e]; }
};

// ---- repulsion ------------------------------------------------------------------------------------------------------------
struct RepPlan {
    int row_blocks, tiles, splits, tiles_per_split;
    long off_z, bytes;               // [splits][n][2] fp64 partial forces, then [row_blocks * splits] fp64 Z parts
};

bool rep_plan(int n, RepPlan& p) {
    if (n < 2) return false;
    p.row_blocks = p.tiles = (int)(((long)n + TP - 1) / TP);
    int s = (TARGET_WG + p.row_blocks - 1) / p.row_blocks;
    s = s < 1 ? 1 : (s > MAX_SPLITS ? MAX_SPLITS : s);
    s = s > p.tiles ? p.tiles : s;
    p.tiles_per_split = (p.tiles + s - 1) / s;
    p.splits = (p.tiles + p.tiles_per_split - 1) / p.tiles_per_split;        // no empty split
    p.off_z = (long)p.splits * n * 2 * 8;
    p.bytes = csr_align16(p.off_z + (long)p.row_blocks * p.splits * 8);
    return true;
}

__device__ __forceinline__ float rcp_newton(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, r, 1.f), r, r);
}

// The owned point against `cnt` staged points; SELF: staged slot `self` is the owned point itself and leaves.
template <bool SELF>
__device__ __forceinline__ void rep_tile(const float2* __restrict__ T, int cnt, int self, float xi, float yi, float& fx, float& fy,
                                         float& z) {
#pragma unroll 8
    for (int j = 0; j < cnt; ++j) {
        const float2 q = T[j];
        const float dx = xi - q.x, dy = yi - q.y;
        float w = rcp_newton(__builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, 1.f)));
        if (SELF) w = j == self ? 0.f : w;
        const float w2 = w * w;
        z += w;
        fx = __builtin_fmaf(w2, dx, fx);
        fy = __builtin_fmaf(w2, dy, fy);
    }
}

__global__ __launch_bounds__(TP) void tsne_repulsion_kernel(const float2* __restrict__ y, int n, int tiles, int tiles_per_split,
                                                            double* __restrict__ part, double* __restrict__ zpart) {
    __shared__ float2 T[TP];
    __shared__ double sh[16];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * TP + tid;
    const bool own = i < n;
    const float2 yi = own ? y[i] : make_float2(0.f, 0.f);
    const int t0 = blockIdx.y * tiles_per_split, t1 = min(t0 + tiles_per_split, tiles);
    double Fx = 0., Fy = 0., Z = 0.;
    for (int t = t0; t < t1; ++t) {
        const long j0 = (long)t * TP;
        const int cnt = (int)min((long)TP, n - j0);
        __syncthreads();                                             // the previous tile has been read
        if (tid < cnt) T[tid] = y[j0 + tid];
        __syncthreads();
        float fx = 0.f, fy = 0.f, z = 0.f;
        if (t == (int)blockIdx.x) rep_tile<true>(T, cnt, tid, yi.x, yi.y, fx, fy, z);
        else rep_tile<false>(T, cnt, 0, yi.x, yi.y, fx, fy, z);
        Fx += (double)fx; Fy += (double)fy; Z += (double)z;
    }
    if (own) {
        double* o = part + ((long)blockIdx.y * n + i) * 2;
        o[0] = Fx; o[1] = Fy;
    }
    const double zt = block_sum(own ? Z : 0., sh);
    if (tid == 0) zpart[(long)blockIdx.y * gridDim.x + blockIdx.x] = zt;
}

// rep[e] = the S partial forces of element e in split order; workgroup 0 also folds `nparts` scalar parts into total[0].  Also
// the KL fold of tsne_gradient (n2 = 0).
__global__ __launch_bounds__(256) void tsne_fold_kernel(const double* __restrict__ part, long n2, int splits, float* __restrict__ rep,
                                                        const double* __restrict__ sparts, long nparts, double* __restrict__ total) {
    __shared__ double sh[16];
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < n2) {
        double s = 0.;
        for (int k = 0; k < splits; ++k) s += part[(long)k * n2 + e];
        rep[e] = (float)s;
    }
    if (blockIdx.x == 0) {
        double s = 0.;
        for (long b = threadIdx.x; b < nparts; b += 256) s += sparts[b];
        const double t = block_sum(s, sh);
        if (threadIdx.x == 0) total[0] = t;
    }
}

// ---- gradient -------------------------------------------------------------------------------------------------------------
template <bool KL>
__global__ __launch_bounds__(256) void tsne_gradient_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                            const float* __restrict__ p, long cap, const float2* __restrict__ y,
                                                            const float2* __restrict__ rep, const double* __restrict__ Zp, int n,
                                                            double exaggeration, float2* __restrict__ grad, double* __restrict__ klpart) {
    __shared__ double sh[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 4 + wv;
    const double Z = Zp[0];
    double kl = 0.;
    if (i < n) {
        const long l0 = max((long)rowptr[i], 0L), l1 = min((long)rowptr[i + 1], cap);
        const float2 yi = y[i];
        float ax = 0.f, ay = 0.f;
        for (long l = l0 + lane; l < l1; l += 64) {
            const int j = col[l];
            if (j < 0 || j >= n) continue;                           // a malformed matrix cannot make the kernel read out of bounds
            const float2 yj = y[j];
            const float pij = p[l];
            const float dx = yi.x - yj.x, dy = yi.y - yj.y;
            const float den = __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, 1.f));
            const float pw = pij / den;
            ax = __builtin_fmaf(pw, dx, ax);
            ay = __builtin_fmaf(pw, dy, ay);
            if (KL && pij > 0.f) kl += (double)pij * log((double)pij * Z * (double)den);
        }
        const double sx = wave_sum((double)ax), sy = wave_sum((double)ay);
        if (lane == 0) {
            const float2 r = rep[i];
            grad[i] = make_float2((float)(4. * (exaggeration * sx - (double)r.x / Z)), (float)(4. * (exaggeration * sy - (double)r.y / Z)));
        }
    }
    if (KL) {
        kl = wave_sum(kl);
        if (lane == 0) sh[wv] = kl;
        __syncthreads();
        if (threadIdx.x == 0) klpart[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    }
}

// ---- update ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_update_kernel(const float* __restrict__ grad, long n2, float momentum, float lr,
                                                          float* __restrict__ y, float* __restrict__ update, float* __restrict__ gains) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n2) return;
    const float g = grad[e], u = update[e];
    const bool inc = u * g < 0.f;
    const float gain = fmaxf(inc ? gains[e] + 0.2f : gains[e] * 0.8f, 0.01f);
    const float un = momentum * u - lr * gain * g;
    gains[e] = gain;
    update[e] = un;
    y[e] += un;
}

long grad_bytes(int n) { return csr_align16(((long)n + 3) / 4 * 8); }

bool finite_nonneg(double x) { return x >= 0. && x < __builtin_inf(); }          // NaN fails both comparisons

}  // namespace

extern "C" int audiossl_tsne_workspace(int n, int k, long* bytes) {
    CsrSymPlan c;
    RepPlan r;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(k >= 1 && k <= MAX_K);
    ASSL_REQUIRE(csr_sym_plan(n, k, c) && rep_plan(n, r));
    long b = c.bytes > r.bytes ? c.bytes : r.bytes;
    if (grad_bytes(n) > b) b = grad_bytes(n);
    *bytes = b;
    return ASSL_OK;
}

extern "C" int audiossl_tsne_calibrate(const float* d2, int n, int k, double perplexity, float* p_cond, float* beta, void* stream) {
    ASSL_REQUIRE(d2 && p_cond && beta);
    ASSL_REQUIRE(n >= 2 && k >= 1 && k <= MAX_K && k <= n - 1 && (long)n * k < (1L << 30));
    ASSL_REQUIRE(perplexity > 0. && perplexity <= (double)k);       // (a NaN fails the first comparison)
    hipLaunchKernelGGL(tsne_calibrate_kernel, dim3((unsigned)(((long)n + 3) / 4)), dim3(256), 0, S_(stream), d2, n, k, log(perplexity),
                       p_cond, beta);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_tsne_symmetrize(const int* idx, const float* p_cond, int n, int k, int* rowptr, int* col, float* p, int* nnz,
                                        void* workspace, long workspace_bytes, void* stream) {
    CsrSymPlan c;
    ASSL_REQUIRE(idx && p_cond && rowptr && col && p && nnz && workspace);
    ASSL_REQUIRE(k >= 1 && k <= MAX_K);
    ASSL_REQUIRE(csr_sym_plan(n, k, c));
    ASSL_REQUIRE(workspace_bytes >= c.bytes);
    if (!ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    return csr_sym_build<float>(c, idx, n, k, CondValue{p_cond}, 0.5 / (double)n, rowptr, col, p, nnz, workspace, S_(stream));
}

extern "C" int audiossl_tsne_repulsion(const float* y, int n, float* rep, double* Z, void* workspace, long workspace_bytes, void* stream) {
    RepPlan r;
    ASSL_REQUIRE(y && rep && Z && workspace);
    ASSL_REQUIRE(rep_plan(n, r));
    ASSL_REQUIRE(workspace_bytes >= r.bytes);
    if (!ASSL_ALIGNED16(workspace) || (((uintptr_t)y) & 7) != 0) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    double* part = static_cast<double*>(workspace);
    double* zpart = reinterpret_cast<double*>(static_cast<char*>(workspace) + r.off_z);
    hipLaunchKernelGGL(tsne_repulsion_kernel, dim3((unsigned)r.row_blocks, (unsigned)r.splits), dim3(TP), 0, s,
                       reinterpret_cast<const float2*>(y), n, r.tiles, r.tiles_per_split, part, zpart);
    hipLaunchKernelGGL(tsne_fold_kernel, GRID1(2L * n), dim3(256), 0, s, part, 2L * n, r.splits, rep, zpart, (long)r.row_blocks * r.splits, Z);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_tsne_gradient(const int* rowptr, const int* col, const float* p, long cap, const float* y, const float* rep,
                                      const double* Z, int n, double exaggeration, float* grad, double* kl, void* workspace,
                                      long workspace_bytes, void* stream) {
    ASSL_REQUIRE(rowptr && col && p && y && rep && Z && grad);
    ASSL_REQUIRE(n >= 2 && cap >= 0 && finite_nonneg(exaggeration));
    ASSL_REQUIRE(kl == nullptr || (workspace && workspace_bytes >= grad_bytes(n)));
    if (((((uintptr_t)y) | ((uintptr_t)rep) | ((uintptr_t)grad)) & 7) != 0) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    const dim3 rows4((unsigned)(((long)n + 3) / 4));
    const float2* y2 = reinterpret_cast<const float2*>(y);
    const float2* r2 = reinterpret_cast<const float2*>(rep);
    float2* g2 = reinterpret_cast<float2*>(grad);
    if (kl) {
        double* klpart = static_cast<double*>(workspace);
        hipLaunchKernelGGL(tsne_gradient_kernel<true>, rows4, dim3(256), 0, s, rowptr, col, p, cap, y2, r2, Z, n, exaggeration, g2, klpart);
        hipLaunchKernelGGL(tsne_fold_kernel, dim3(1), dim3(256), 0, s, static_cast<const double*>(nullptr), 0L, 0, static_cast<float*>(nullptr),
                           klpart, (long)rows4.x, kl);
    } else {
        hipLaunchKernelGGL(tsne_gradient_kernel<false>, rows4, dim3(256), 0, s, rowptr, col, p, cap, y2, r2, Z, n, exaggeration, g2,
                           static_cast<double*>(nullptr));
    }
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_tsne_update(const float* grad, int n, double momentum, double learning_rate, float* y, float* update,
                                    float* gains, void* stream) {
    ASSL_REQUIRE(grad && y && update && gains);
    ASSL_REQUIRE(n >= 2 && finite_nonneg(momentum) && finite_nonneg(learning_rate));
    hipLaunchKernelGGL(tsne_update_kernel, GRID1(2L * n), dim3(256), 0, S_(stream), grad, 2L * n, (float)momentum, (float)learning_rate, y,
                       update, gains);
    ASSL_LAUNCH_CHECK();
}
