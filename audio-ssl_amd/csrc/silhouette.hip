// Silhouette coefficient of a labeling on the features it was computed on (sklearn's `silhouette_samples`, Euclidean): the score
// the labeler prints (`store_clusters --score`) and sweeps k by (`--k_sweep`).
//
//   a_i = mean distance from row i to the OTHER members of its cluster, b_i = min over the other clusters of the mean distance
//   to that cluster's members, s_i = (b_i - a_i) / max(a_i, b_i); 0 for a one-member cluster and for 0 / 0.
//
// It needs every pairwise distance and stores none of them.  The rows arrive SORTED BY CLUSTER (seg [K + 1] = offsets).
// g_ij = <x_i, x_j> is the fp32 Gram tile of gram_tile.h in index chain order and n_i = g_ii its norm kernel, so
// dist_ij = sqrt(max(0, (n_i + n_j) - 2 g_ij)) is exactly 0 wherever row j repeats row i.  Self leaves by INDEX.  sqrt is the
// correctly rounded fp32 one (hipcc's default for sqrtf); everything after it is fp64.  What this file adds on top of the
// tile is the per-cluster walk:
//
// Reduction.  The 64 x 128 tile is dumped to LDS over the dead staging buffers and wave w takes rows 16w..16w+15: each lane
// turns its two columns (lane, 64 + lane) of every row into distances, in place, and adds them to one fp64 accumulator per
// row, which lives across tiles for as long as the walk stays inside one cluster.  Columns are in cluster order, so the runs of a tile
// are wave-uniform: a tile is cut at every seg[c + 1] that falls inside it, and when cluster c ends the wave folds its 16
// accumulators over the lanes in a fixed tree (four halving exchanges that leave row r in lanes 4r..4r+3, then two butterfly
// steps: 17 fp64 shuffles, not 16 x 6), divides by |c| (|c| - 1 for the row's own cluster), updates b (a) and clears the
// accumulators.  Neither the n x n matrix nor an n x K table exists.  One workgroup walks ALL columns of its 64 rows: a
// column split would need per-cluster partial sums across splits.
//
// No atomics, no memset, plain launches; the workspace (the norms) needs no clearing; two launches agree bit for bit.
#include "gram_tile.h"

namespace {

constexpr int RW = QT / 4;           // rows per wave
constexpr int LDS_BYTES = TILE_BYTES + QT * 4;           // the Gram tile (over the staging buffers) + the owned rows' norms

struct SilArgs {
    const float* x;      // [n][d], rows sorted by cluster
    const float* gn;     // [n] squared norms in the tile's own chain
    const int* seg;      // [K + 1]
    double* s;           // [n]
    int n, d, K;
    int tiles;
};

// The wave's RW per-lane partial sums -> every row's total: row r in lanes 4r..4r+3 (returned value).  A fixed tree.
__device__ __forceinline__ double fold_rows(double (&v)[RW], int lane) {
#pragma unroll
    for (int m = RW / 2, o = 32; m >= 1; m >>= 1, o >>= 1) {        // lanes with bit o set keep rows i + m, the others rows i
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int i = 0; i < m; ++i) {
            const double keep = up ? v[i + m] : v[i], send = up ? v[i] : v[i + m];
            v[i] = keep + __shfl_xor(send, o, 64);
        }
    }
    double t = v[0];                                                // row 8 b5 + 4 b4 + 2 b3 + b2 = lane >> 2
    t += __shfl_xor(t, 2, 64);
    t += __shfl_xor(t, 1, 64);
    return t;
}

__global__ __launch_bounds__(256) void silhouette_kernel(SilArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Os = reinterpret_cast<float*>(smem);                      // [QT][RP] owned rows
    float* Ws = Os + QT * RP;                                        // [BT][RP] walked rows
    float* St = reinterpret_cast<float*>(smem);                      // [QT][SP], over Os / Ws once the feature loop is done
    float* Ns = reinterpret_cast<float*>(smem + TILE_BYTES);         // [QT] owned norms
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long q0 = (long)blockIdx.x * QT;
    const int n = a.n, K = a.K;

    if (tid < QT) Ns[tid] = q0 + tid < n ? a.gn[q0 + tid] : 0.f;     // (the first barrier of the tile loop orders this)

    // the walk's state: cluster c (wave-uniform; its columns are seg[c] .. seg[c + 1] - 1), the rows' sums over the part of c
    // walked so far, and for the lane's row (lane >> 2 of this wave's 16) a, b and whether its cluster has one member
    const int row0 = __builtin_amdgcn_readfirstlane(w) * RW;
    const long my = q0 + row0 + (lane >> 2);
    int c = 0;
    double sum[RW];
#pragma unroll
    for (int q = 0; q < RW; ++q) sum[q] = 0.;
    double aa = 0., bb = __builtin_inf();
    bool single = false;

    for (int t = 0; t < a.tiles; ++t) {
        const long b0 = (long)t * BT;
        f32x16 acc[2];
        gram_tile<ChainOrder::Index>(a.x, n, a.d, q0, b0, Os, Ws, acc);      // (its first barrier: the previous tile's walk is done)
        gram_tile_to_lds(acc, St);

        // this wave's 16 rows x the lane's two columns -> distances; a column past n or the row itself contributes 0
        const long r0 = b0 + lane, r1 = b0 + 64 + lane;
        const bool ok0 = r0 < n, ok1 = r1 < n;
        const float nj0 = ok0 ? a.gn[r0] : 0.f, nj1 = ok1 ? a.gn[r1] : 0.f;
        // (written back over the lane's own two Gram entries: no other lane reads them, so no barrier; a rolled loop - sixteen
        // interleaved sqrt expansions would cost the kernel its occupancy)
        float* mine = St + row0 * SP + lane;
#pragma unroll 2
        for (int q = 0; q < RW; ++q) {
            const long gq = q0 + row0 + q;
            const float ni = Ns[row0 + q];
            float* g = mine + q * SP;
            const float d0 = sqrtf(fmaxf((ni + nj0) - 2.f * g[0], 0.f));
            const float d1 = sqrtf(fmaxf((ni + nj1) - 2.f * g[64], 0.f));
            g[0] = ok0 && r0 != gq ? d0 : 0.f;                       // self leaves by index, not by value
            g[64] = ok1 && r1 != gq ? d1 : 0.f;
        }
        // the tile's runs: [col, end) lies in cluster c.  c < K also ends the walk if the device's seg is not the host's.
        const long tile_end = b0 + BT < n ? b0 + BT : (long)n;
        long col = b0;
        while (col < tile_end && c < K) {
            const int lo = a.seg[c], hi = a.seg[c + 1];
            long end = hi < tile_end ? (long)hi : tile_end;
            if (end < col) end = col;
            const bool m0 = r0 >= col && r0 < end, m1 = r1 >= col && r1 < end;
#pragma unroll
            for (int q = 0; q < RW; ++q) {
                sum[q] += (double)(m0 ? mine[q * SP] : 0.f);
                sum[q] += (double)(m1 ? mine[q * SP + 64] : 0.f);
            }
            col = end;
            if (hi > tile_end) break;                                // cluster c goes on in the next tile
            const double total = fold_rows(sum, lane);
#pragma unroll
            for (int q = 0; q < RW; ++q) sum[q] = 0.;
            const int size = hi - lo;
            const bool own = my >= lo && my < hi;
            const double mean = total / (double)(own ? size - 1 : size);     // own and alone: 0 / 0, replaced below
            if (own) { aa = mean; single = size <= 1; }
            else bb = fmin(bb, mean);
            ++c;
        }
    }

    if ((lane & 3) == 0 && my < n) {
        double s = (bb - aa) / fmax(aa, bb);
        if (single || s != s) s = 0.;                                // sklearn: a one-member cluster scores 0, and so does 0 / 0
        a.s[my] = s;
    }
}

bool sil_plan(int n, long& q_tiles, int& tiles, long& ws_bytes) {
    if (n < 3) return false;
    q_tiles = ((long)n + QT - 1) / QT;
    tiles = (int)(((long)n + BT - 1) / BT);
    ws_bytes = q_tiles * QT * 4;
    return true;
}

}  // namespace

extern "C" int audiossl_silhouette_workspace(int n, long* bytes) {
    long q_tiles, ws;
    int tiles;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(sil_plan(n, q_tiles, tiles, ws));
    *bytes = ws;
    return ASSL_OK;
}

extern "C" int audiossl_silhouette(const float* xs, int n, int d, const int* seg, const int* seg_host, int K, double* s,
                                   void* workspace, long workspace_bytes, void* stream) {
    long q_tiles, ws;
    int tiles;
    ASSL_REQUIRE(xs && seg && seg_host && s && workspace);
    ASSL_REQUIRE(sil_plan(n, q_tiles, tiles, ws));
    ASSL_REQUIRE(gram_width_ok(d));
    ASSL_REQUIRE(K >= 2 && K <= n - 1);
    ASSL_REQUIRE(workspace_bytes >= ws);
    ASSL_REQUIRE(seg_host[0] == 0 && seg_host[K] == n);
    for (int c = 0; c < K; ++c) ASSL_REQUIRE(seg_host[c + 1] > seg_host[c]);      // no empty, no decreasing segment
    if (!ASSL_ALIGNED16(xs) || !ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t st = S_(stream);
    float* gn = static_cast<float*>(workspace);
    SilArgs a;
    a.x = xs; a.gn = gn; a.seg = seg; a.s = s;
    a.n = n; a.d = d; a.K = K;
    a.tiles = tiles;
    hipLaunchKernelGGL(gram_norm_kernel<ChainOrder::Index>, GRID1(q_tiles * QT), dim3(256), 0, st, xs, n, d, q_tiles * QT, gn);
    hipLaunchKernelGGL(silhouette_kernel, dim3((unsigned)q_tiles), dim3(256), LDS_BYTES, st, a);
    ASSL_LAUNCH_CHECK();
}
