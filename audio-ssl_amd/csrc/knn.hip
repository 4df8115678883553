// k-nearest-neighbour evaluation on frozen embeddings: the weighted k-NN classifier of InstDisc / MoCo / DINO
// (`knn_classifier` in DINO's eval_knn.py; the reference's `validation_step`s reach for `precision_at_k` and never got there).
//
// knn_topk: sim = bank q^T on the bf16 MFMA pipe, fp32 accumulation, reduced to each query's k best bank rows in the kernel
// that forms it - the [Nq][Nb] matrix never exists in memory (audiossl_moco_logits does the same with a soft-max reduction).
//
//   * A workgroup (4 waves) owns 64 queries and walks a run of 128-row bank tiles.  Per tile: a plain LDS-staged GEMM over D
//     in chunks of 64 (next chunk's global loads in flight during the MFMAs), similarities TRANSPOSED as in attention.hip
//     (A = bank rows, B = queries: a lane's column is a query, its 16 registers are bank rows).
//   * The 64 x 128 fp32 tile is dumped to LDS over the dead staging buffers; wave w then scans queries 16w..16w+15 with the
//     streaming selector of topk.h (k <= 128: a one- or two-slot list per query), order (sim descending, bank row ascending).
//   * Few queries: the bank is split over blockIdx.y; every split writes its k best per query to the workspace and
//     topk_merge_kernel folds them.  With one split the lists go straight to the output.
//
// knn_vote: one wave per query, k x k label comparison (labels are compared, never used as an index).
#include "topk.h"

namespace {

constexpr int QT = 64;              // queries per workgroup
constexpr int BT = 128;             // bank rows per tile
constexpr int KC = 64;              // D chunk per staging step
constexpr int RP = KC + 8;          // staging pitch (elements): 144-byte rows, 16-byte aligned fragments
constexpr int SP = BT + 4;          // similarity tile pitch (floats): 528-byte rows, 16-byte aligned float4 stores
constexpr int TILE_BYTES = QT * SP * 4;                 // 33,792 >= the staging buffers' (QT + BT) * RP * 2 = 27,648
static_assert(TILE_BYTES >= (QT + BT) * RP * 2, "the similarity tile lies over the staging buffers");

constexpr size_t knn_lds_bytes(int KP) { return (size_t)TILE_BYTES + (size_t)QT * KP * 8; }

struct KnnArgs {
    const bf16* q;       // [Nq][D]
    const bf16* bank;    // [Nb][D]
    float* out_v;        // [splits][Nq][k]  (the caller's top_sim when splits == 1)
    int* out_i;
    long Nb;
    long split_stride;   // Nq * k
    int Nq, D, k;
    int bank_tiles, tiles_per_split;
};

template <int KP>
__global__ __launch_bounds__(256) void knn_topk_kernel(KnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16* Qs = reinterpret_cast<bf16*>(smem);
    bf16* Bs = Qs + QT * RP;
    float* St = reinterpret_cast<float*>(smem);                      // [QT][SP], over Qs / Bs once the K loop is done
    float* Lv = reinterpret_cast<float*>(smem + TILE_BYTES);         // [QT][KP]
    int* Li = reinterpret_cast<int*>(Lv + QT * KP);                  // [QT][KP]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const long q0 = (long)blockIdx.x * QT;
    const int D = a.D, k = a.k;

    topk_lds_init<QT, KP, SimDescending>(Lv, Li);

    const int t0 = blockIdx.y * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.bank_tiles);
    const int nchunk = (D + KC - 1) / KC;
    // staging: 8 threads per row (16 bytes each), rows tid / 8 + 32 v
    const int srow = tid >> 3, scol = (tid & 7) * 8;

    for (int t = t0; t < t1; ++t) {
        const long b0 = (long)t * BT;
        f32x16 acc[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[qt][r] = 0.f;

        Vec8<bf16> rq[2], rb[4];
        auto load_chunk = [&](int c) {
            const int col = c * KC + scol;
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const long gq = q0 + srow + 32 * v;
                rq[v] = (gq < a.Nq && col < D) ? Vec8<bf16>::load(a.q + gq * D + col) : Vec8<bf16>::zero();
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const long gb = b0 + srow + 32 * v;
                rb[v] = (gb < a.Nb && col < D) ? Vec8<bf16>::load(a.bank + gb * D + col) : Vec8<bf16>::zero();
            }
        };
        load_chunk(0);
        for (int c = 0; c < nchunk; ++c) {
            __syncthreads();                                         // previous chunk's fragments / previous tile's scan are done
#pragma unroll
            for (int v = 0; v < 2; ++v) rq[v].store(Qs + (srow + 32 * v) * RP + scol);
#pragma unroll
            for (int v = 0; v < 4; ++v) rb[v].store(Bs + (srow + 32 * v) * RP + scol);
            __syncthreads();
            if (c + 1 < nchunk) load_chunk(c + 1);
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                const Vec8<bf16> fb = Vec8<bf16>::load(Bs + (w * 32 + l31) * RP + ks * 16 + 8 * half);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) {
                    const Vec8<bf16> fq = Vec8<bf16>::load(Qs + (qt * 32 + l31) * RP + ks * 16 + 8 * half);
                    acc[qt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb.v, fq.v, acc[qt], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                             // all fragment reads done: the staging buffers are dead
        // C/D map: column = lane & 31 = query, row (bank) of register r = (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 x = {acc[qt][4 * g], acc[qt][4 * g + 1], acc[qt][4 * g + 2], acc[qt][4 * g + 3]};
                *reinterpret_cast<f32x4*>(St + (qt * 32 + l31) * SP + w * 32 + 8 * g + 4 * half) = x;
            }
        __syncthreads();

        const long r0 = b0 + lane, r1 = b0 + 64 + lane;
        const bool ok0 = r0 < a.Nb, ok1 = r1 < a.Nb;
        const int i0 = (int)r0, i1 = (int)r1;
        topk_lds_scan<QT, KP, SimDescending>(Lv, Li, k, q0, a.Nq, lane, w, [&](int q, int h) {
            return TopCand{St[q * SP + 64 * h + lane], h ? i1 : i0, h ? ok1 : ok0};
        });
    }

    topk_lds_write<QT, KP>(Lv, Li, k, q0, a.Nq, lane, w, a.out_v + (long)blockIdx.y * a.split_stride,
                           a.out_i + (long)blockIdx.y * a.split_stride);
}

// Weighted vote, one wave per query.  Neighbour j (lanes hold j = lane and lane + 64) weighs exp((s_j - max_j s) inv_t); a
// lane sums the weights of all neighbours that share its label, in neighbour order, so equal labels see bit-equal sums.
__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ top_sim, const int* __restrict__ top_idx,
                                                       const long long* __restrict__ bank_label, int Nq, int k, long Nb,
                                                       float inv_t, long long* __restrict__ pred, float* __restrict__ conf) {
    __shared__ long long sl[4][128];
    __shared__ float sw[4][128];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long q = (long)blockIdx.x * 4 + w;
    const bool active = q < Nq;
    float s[2] = {-INFINITY, -INFINITY};
    long long lab[2] = {0, 0};
    bool bad = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = h * 64 + lane;
        if (active && j < k) {
            s[h] = top_sim[q * k + j];
            const int id = top_idx[q * k + j];
            if (id < 0 || (long)id >= Nb) bad = true;              // never dereferenced
            else lab[h] = bank_label[id];
        }
    }
    const float mx = wave_max(fmaxf(s[0], s[1]));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = h * 64 + lane;
        sl[w][j] = lab[h];
        sw[w][j] = (active && j < k) ? expf((s[h] - mx) * inv_t) : 0.f;
    }
    __syncthreads();
    float best = -1.f;
    long long best_lab = 0;
    float total = 0.f;
    if (active) {
        float sum[2] = {0.f, 0.f};
        for (int i = 0; i < k; ++i) {
            const long long li = sl[w][i];
            const float wi = sw[w][i];
            total += wi;
            sum[0] += (li == lab[0]) ? wi : 0.f;
            sum[1] += (li == lab[1]) ? wi : 0.f;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (h * 64 + lane < k && (sum[h] > best || (sum[h] == best && lab[h] < best_lab))) { best = sum[h]; best_lab = lab[h]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const long long ol = __shfl_xor(best_lab, o, 64);
        if (ob > best || (ob == best && ol < best_lab)) { best = ob; best_lab = ol; }
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (active && lane == 0) {
        pred[q] = any_bad ? -1ll : best_lab;
        conf[q] = any_bad ? __builtin_nanf("") : best / total;
    }
}

struct KnnPlan {
    long q_tiles;
    int bank_tiles, splits, tiles_per_split;
    long ws_bytes;
};

// Splits (plan_splits): at least four bank tiles each.  The workspace figure is a bound on splits * Nq * k * 8 that grows with
// Nq and with k: q_tiles * splits <= min(q_tiles + TARGET_WG - 1, q_tiles * max_splits) because splits <= ceil(TARGET_WG /
// q_tiles).
bool knn_plan(int Nq, long Nb, int k, KnnPlan& p) {
    if (!(k >= 1 && k <= 128 && (long)k <= Nb && Nb < (1L << 31) && Nq >= 1)) return false;
    p.q_tiles = ((long)Nq + QT - 1) / QT;
    p.bank_tiles = (int)((Nb + BT - 1) / BT);
    const SplitPlan sp = plan_splits(p.q_tiles, p.bank_tiles, 4);
    p.splits = sp.splits;
    p.tiles_per_split = sp.tiles_per_split;
    const long a = p.q_tiles + TARGET_WG - 1, b = p.q_tiles * sp.max_splits;
    p.ws_bytes = (a < b ? a : b) * QT * (long)k * 8;
    return true;
}

template <int KP>
int knn_launch(const KnnArgs& a, const KnnPlan& p, float* wv, int* wi, float* top_sim, int* top_idx, hipStream_t s) {
    if (!allow_dynamic_lds<knn_topk_kernel<KP>>(knn_lds_bytes(KP))) return ASSL_ELAUNCH;
    hipLaunchKernelGGL(knn_topk_kernel<KP>, dim3((unsigned)p.q_tiles, (unsigned)p.splits), dim3(256), knn_lds_bytes(KP), s, a);
    if (p.splits > 1)
        hipLaunchKernelGGL((topk_merge_kernel<KP, SimDescending>), dim3((unsigned)(((long)a.Nq + 3) / 4)), dim3(256), 0, s, wv, wi,
                           p.splits, a.split_stride, a.Nq, a.k, top_sim, top_idx);
    ASSL_LAUNCH_CHECK();
}

}  // namespace

extern "C" int audiossl_knn_workspace(int Nq, long Nb, int k, long* bytes) {
    KnnPlan p;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(knn_plan(Nq, Nb, k, p));
    *bytes = p.ws_bytes;
    return ASSL_OK;
}

extern "C" int audiossl_knn_topk(const void* q, const void* bank, int Nq, long Nb, int D, int k, float* top_sim, int* top_idx,
                                 void* workspace, long workspace_bytes, void* stream) {
    KnnPlan p;
    ASSL_REQUIRE(q && bank && top_sim && top_idx && workspace);
    ASSL_REQUIRE(D >= 32 && D <= 4096 && D % 32 == 0);
    ASSL_REQUIRE(knn_plan(Nq, Nb, k, p));
    ASSL_REQUIRE(workspace_bytes >= p.ws_bytes);
    if (!ASSL_ALIGNED16(q) || !ASSL_ALIGNED16(bank) || !ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    KnnArgs a;
    a.q = static_cast<const bf16*>(q);
    a.bank = static_cast<const bf16*>(bank);
    a.Nb = Nb; a.Nq = Nq; a.D = D; a.k = k;
    a.bank_tiles = p.bank_tiles; a.tiles_per_split = p.tiles_per_split;
    a.split_stride = (long)Nq * k;
    float* wv = static_cast<float*>(workspace);
    int* wi = reinterpret_cast<int*>(wv + (long)p.splits * a.split_stride);
    a.out_v = p.splits == 1 ? top_sim : wv;
    a.out_i = p.splits == 1 ? top_idx : wi;
    return k <= 64 ? knn_launch<64>(a, p, wv, wi, top_sim, top_idx, s) : knn_launch<128>(a, p, wv, wi, top_sim, top_idx, s);
}

extern "C" int audiossl_knn_vote(const float* top_sim, const int* top_idx, const long long* bank_label, int Nq, int k, long Nb,
                                 float inv_t, long long* pred, float* conf, void* stream) {
    ASSL_REQUIRE(top_sim && top_idx && bank_label && pred && conf);
    ASSL_REQUIRE(Nq >= 1 && k >= 1 && k <= 128 && Nb >= 1 && Nb < (1L << 31) && inv_t >= 0.f);
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)(((long)Nq + 3) / 4)), dim3(256), 0, S_(stream), top_sim, top_idx, bank_label, Nq,
                       k, Nb, inv_t, pred, conf);
    ASSL_LAUNCH_CHECK();
}
