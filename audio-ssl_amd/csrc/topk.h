// Streaming top-k selector shared by knn.hip (similarity, descending) and graph.hip (squared distance, ascending), the
// split planner of every kernel that walks tiles per owned row block (knn.hip, graph.hip, cka.hip), and the dynamic-LDS
// opt-in.
//
// A workgroup of 4 waves owns ROWS list rows and walks 128-candidate tiles.  Each row keeps its k best candidates as a
// sorted list in LDS ([ROWS][KP] values, [ROWS][KP] indices).  Per tile, wave w scans rows ROWS/4 w .. ROWS/4 (w + 1) - 1:
// one ballot of "beats the row's current k-th entry" over the lanes' two candidates.  Almost always the ballot is empty
// once the lists have warmed up (a row sees about k ln(N / k) insertions in all).  Otherwise the row's list (slot
// s * 64 + lane: one or two entries per lane) is pulled into registers and the candidates are inserted one at a time:
// position = popcount of a ballot, shift = one lane rotation, with the last lane of a slot carried into lane 0 of the next.
// Order: the policy's `before` is a strict total order on (value, index) and every comparison uses it, so the result does
// not depend on the order in which tiles, waves or splits deliver candidates, ties included.
// Few rows: the walked tiles are split over blockIdx.y (plan_splits); every split writes its k best per row to a workspace
// and topk_merge_kernel (one wave per row, the same register list) folds them.
#pragma once
#include "common.h"
#include <limits.h>

namespace {

constexpr int TARGET_WG = 512;      // two workgroups per CU on 256 CUs

// ---- order policies: strict total orders on (value, row), smaller row first among equal values ------------------------------
struct SimDescending {              // larger similarity first
    __device__ __forceinline__ static bool before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }
    __device__ __forceinline__ static float empty() { return -INFINITY; }
};
struct DistAscending {              // smaller distance first
    __device__ __forceinline__ static bool before(float a, int ia, float b, int ib) { return a < b || (a == b && ia < ib); }
    __device__ __forceinline__ static float empty() { return INFINITY; }
};

struct TopCand {                    // one lane's candidate
    float v;
    int i;
    bool ok;
};

// A row's sorted list spread over one wave: slot s * 64 + lane.  Empty slots hold (Ord::empty(), INT_MAX).
template <int KP, class Ord> struct TopList {
    float v[KP / 64];
    int i[KP / 64];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int s = 0; s < KP / 64; ++s) { v[s] = Ord::empty(); i[s] = INT_MAX; }
    }
    __device__ __forceinline__ void kth(int k, float& tv, int& ti) const {
        if (KP == 64 || k <= 64) { tv = __shfl(v[0], k - 1, 64); ti = __shfl(i[0], k - 1, 64); }
        else                     { tv = __shfl(v[KP / 64 - 1], k - 65, 64); ti = __shfl(i[KP / 64 - 1], k - 65, 64); }
    }
};

// One candidate per lane (cv, ci, valid) folded into the list; k is wave-uniform.  Everything after the first ballot is
// wave-uniform control flow.
template <int KP, class Ord>
__device__ __forceinline__ void fold(TopList<KP, Ord>& L, float cv, int ci, bool valid, int k, int lane) {
    constexpr int NS = KP / 64;
    float tv; int ti;
    L.kth(k, tv, ti);
    unsigned long long m = __ballot(valid && Ord::before(cv, ci, tv, ti));
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float c = __shfl(cv, src, 64);
        const int cidx = __shfl(ci, src, 64);
        if (!Ord::before(c, cidx, tv, ti)) continue;               // an earlier insertion raised the bar
        int pos = 0;                                               // entries ahead of the candidate = its slot (< k)
#pragma unroll
        for (int s = 0; s < NS; ++s) pos += __popcll(__ballot(Ord::before(L.v[s], L.i[s], c, cidx)));
        float carry_v = 0.f; int carry_i = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float pv = __shfl_up(L.v[s], 1, 64);
            int pi = __shfl_up(L.i[s], 1, 64);
            if (s > 0 && lane == 0) { pv = carry_v; pi = carry_i; }   // slot 0 is never > pos: no carry into s == 0
            if (s + 1 < NS) { carry_v = __shfl(L.v[s], 63, 64); carry_i = __shfl(L.i[s], 63, 64); }
            const int slot = s * 64 + lane;
            if (slot == pos) { L.v[s] = c; L.i[s] = cidx; }
            else if (slot > pos) { L.v[s] = pv; L.i[s] = pi; }
        }
        L.kth(k, tv, ti);
    }
}

// ---- the lists of a workgroup's ROWS rows in LDS: Lv, Li = [ROWS][KP]; 256 threads, wave w owns rows ROWS / 4 * w .. ------------
// (lane and w are the caller's threadIdx.x & 63 and threadIdx.x >> 6)
template <int ROWS, int KP, class Ord>
__device__ __forceinline__ void topk_lds_init(float* Lv, int* Li) {
    for (int e = threadIdx.x; e < ROWS * KP; e += 256) { Lv[e] = Ord::empty(); Li[e] = INT_MAX; }
    // (the first barrier of the caller's tile loop orders this against the scans; every split owns at least one tile)
}

// Wave w's list rows [q_first, q_end) below nrows, in scalar registers: the loops over them are wave-uniform (a bound
// derived from threadIdx in vector registers would make them exec-masked loops).
template <int ROWS>
__device__ __forceinline__ void wave_rows(int w, long row0, long nrows, int& q_first, int& q_end) {
    q_first = __builtin_amdgcn_readfirstlane(w) * (ROWS / 4);
    const long left = nrows - row0;
    q_end = left < q_first + ROWS / 4 ? (int)left : q_first + ROWS / 4;
}

// One 128-candidate tile against this wave's rows: cand(q, h) is the lane's candidate of list row q in column half h
// (tile column 64 h + lane).  Rows at and past nrows are left alone; no barrier in here.
template <int ROWS, int KP, class Ord, class Cand>
__device__ __forceinline__ void topk_lds_scan(float* Lv, int* Li, int k, long row0, long nrows, int lane, int w, Cand cand) {
    int q_first, q_end;
    wave_rows<ROWS>(w, row0, nrows, q_first, q_end);
    for (int q = q_first; q < q_end; ++q) {
        const TopCand c0 = cand(q, 0), c1 = cand(q, 1);
        const float tv = Lv[q * KP + k - 1];
        const int ti = Li[q * KP + k - 1];
        if (__ballot((c0.ok && Ord::before(c0.v, c0.i, tv, ti)) || (c1.ok && Ord::before(c1.v, c1.i, tv, ti))) == 0ull) continue;
        TopList<KP, Ord> L;
#pragma unroll
        for (int s = 0; s < KP / 64; ++s) { L.v[s] = Lv[q * KP + s * 64 + lane]; L.i[s] = Li[q * KP + s * 64 + lane]; }
        fold(L, c0.v, c0.i, c0.ok, k, lane);
        fold(L, c1.v, c1.i, c1.ok, k, lane);
#pragma unroll
        for (int s = 0; s < KP / 64; ++s) { Lv[q * KP + s * 64 + lane] = L.v[s]; Li[q * KP + s * 64 + lane] = L.i[s]; }
    }
}

// This wave's lists to ov / oi = [nrows][k].  A wave's lists are its own: no barrier between its last scan and this.
template <int ROWS, int KP>
__device__ __forceinline__ void topk_lds_write(const float* Lv, const int* Li, int k, long row0, long nrows, int lane, int w,
                                               float* ov, int* oi) {
    int q_first, q_end;
    wave_rows<ROWS>(w, row0, nrows, q_first, q_end);
    for (int q = q_first; q < q_end; ++q) {
        const long gq = row0 + q;
        for (int j = lane; j < k; j += 64) { ov[gq * k + j] = Lv[q * KP + j]; oi[gq * k + j] = Li[q * KP + j]; }
    }
}

// One wave per row: the splits' lists [splits][nrows][k] -> the k best.  Slots a split could not fill carry INT_MAX.
template <int KP, class Ord>
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ wv, const int* __restrict__ wi, int splits,
                                                         long split_stride, int nrows, int k, float* __restrict__ out_v,
                                                         int* __restrict__ out_i) {
    const int lane = threadIdx.x & 63;
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nrows) return;                                          // whole waves leave; no barrier below
    TopList<KP, Ord> L;
    L.clear();
    for (int s = 0; s < splits; ++s) {
        const long base = (long)s * split_stride + q * k;
        for (int j0 = 0; j0 < (KP > 64 ? k : 64); j0 += 64) {              // k <= KP: one pass for the one-slot list
            const int j = j0 + lane;
            const bool in = j < k;
            const float cv = in ? wv[base + j] : 0.f;
            const int ci = in ? wi[base + j] : INT_MAX;
            fold(L, cv, ci, in && ci != INT_MAX, k, lane);
        }
    }
#pragma unroll
    for (int s = 0; s < KP / 64; ++s) {
        const int j = s * 64 + lane;
        if (j < k) { out_v[q * k + j] = L.v[s]; out_i[q * k + j] = L.i[s]; }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct SplitPlan {
    int splits, tiles_per_split;
    long max_splits;                // walked_tiles / min_tiles, at least 1: the callers' workspace bounds use it
};

// Enough workgroups (row_tiles x splits) to fill the chip when there are few row tiles, at least min_tiles walked tiles per
// split, no empty split.
inline SplitPlan plan_splits(long row_tiles, int walked_tiles, int min_tiles) {
    SplitPlan p;
    p.max_splits = walked_tiles / min_tiles > 0 ? walked_tiles / min_tiles : 1;
    long splits = (TARGET_WG + row_tiles - 1) / row_tiles;
    if (splits > p.max_splits) splits = p.max_splits;
    p.tiles_per_split = (int)((walked_tiles + splits - 1) / splits);
    p.splits = (walked_tiles + p.tiles_per_split - 1) / p.tiles_per_split;          // no empty split
    return p;
}

// Kernels that need more than 64 KB of dynamic LDS opt in once per kernel.
template <auto Kernel>
bool allow_dynamic_lds(size_t bytes) {
    static bool done = false;
    if (!done) done = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
    return done;
}

}  // namespace
