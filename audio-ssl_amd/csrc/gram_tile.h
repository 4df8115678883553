// The fp32 Gram tile shared by graph.hip (k-NN graph), silhouette.hip and cka.hip: every pairwise inner product
// g_ij = <x_i, x_j> of the rows of an [n][d] fp32 matrix, in tiles, without an n x n matrix anywhere.
//
// Layout.  g_ij comes off the fp32-input MFMA (mfma_f32_32x32x2f32: exact f32, a k-ordered fmaf chain).  A workgroup of
// 256 threads (4 waves) owns QT = 64 rows i and walks BT = 128-row tiles j.  The tile is formed TRANSPOSED, as in knn.hip:
// A = the walked rows, B = the owned rows, so a lane's C/D column is one owned row and its registers are walked rows.  Wave
// w holds owned rows 32 (w & 1) .. x walked rows 64 (w >> 1) .. in two independent accumulators (the instruction's dependent
// latency is its issue interval: two chains per wave keep the pipe busy).
//
// Staging.  Features go through LDS in chunks of KC = 32 at a pitch of RP = 36 floats (144-byte rows: 16-byte aligned float4
// fragments); 4 threads per row load 8 features each as two float4s, and the next chunk's global loads are in flight during
// the MFMAs.  Rows past n and features past d are staged as zeros.  Lane half h reads the float4 at 8 g + 4 h of its row - one
// ds_read_b128 per operand per four MFMAs - and feeds element s to step s, so one MFMA sums the s-th element of the first
// stored float4, then of the second.
//
// Chain order.  gram_stage8 decides what the two stored float4s of a group of 8 features are, and with that the order of
// the fmaf chain over d, the same for every entry of the tile:
//   ChainOrder::Index   stores 0 2 4 6 | 1 3 5 7: the chain runs 0 1 2 3 4 5 6 7 (graph.hip, silhouette.hip);
//   ChainOrder::Halves  stores the float4s as loaded, 0 1 2 3 | 4 5 6 7: the chain runs 0 4 1 5 2 6 3 7 (cka.hip).
//
// The norm invariant.  gram_norm_kernel runs gram_stage8 and then the chain of the MFMA on a row against itself, so its
// g_ii carries the tile's own roundings and (g_ii + g_jj) - 2 g_ij is EXACTLY 0 wherever row j repeats row i.  The graph's
// "a duplicate row is a neighbour at distance 0", the silhouette's a_i and CKA's "median of the non-zero distances" rest on it.
//
// LDS overlay.  Once the feature loop is done the staging buffers are dead: gram_tile_to_lds dumps the 64 x 128 tile over them
// at a pitch of SP = 132 floats, for users that reduce along rows across waves.
#pragma once
#include "common.h"

namespace {

constexpr int QT = 64;               // owned rows per workgroup
constexpr int BT = 128;              // walked rows per tile
constexpr int KC = 32;               // feature chunk per staging step
constexpr int RP = KC + 4;           // staging pitch (floats): 144-byte rows, 16-byte aligned float4 fragments
constexpr int SP = BT + 4;           // Gram tile pitch (floats): 528-byte rows, 16-byte aligned float4 stores
constexpr int STAGE_BYTES = (QT + BT) * RP * 4;          // 27,648: owned rows [QT][RP], then walked rows [BT][RP]
constexpr int TILE_BYTES = QT * SP * 4;                  // 33,792
constexpr int MAX_D = 4096;
static_assert(TILE_BYTES >= STAGE_BYTES, "the Gram tile lies over the staging buffers");

inline bool gram_width_ok(int d) { return d >= 4 && d <= MAX_D && d % 4 == 0; }

enum class ChainOrder { Index, Halves };

// Features 8 g .. 8 g + 7 of a row (lo, hi) -> the two float4s as staged: MFMA step s sums s0[s], then s1[s].
template <ChainOrder ORDER>
__device__ __forceinline__ void gram_stage8(const f32x4& lo, const f32x4& hi, f32x4& s0, f32x4& s1) {
    if (ORDER == ChainOrder::Index) {
        s0 = f32x4{lo[0], lo[2], hi[0], hi[2]};
        s1 = f32x4{lo[1], lo[3], hi[1], hi[3]};
    } else {
        s0 = lo;
        s1 = hi;
    }
}

// g[i] = g_ii in the tile's own fmaf chain for i < n, 0 for n <= i < n_pad.  d % 4 == 0: a last group of 4 is a group of 8
// whose second half is zero (fmaf(0, 0, acc) == acc).
template <ChainOrder ORDER>
__global__ __launch_bounds__(256) void gram_norm_kernel(const float* __restrict__ x, int n, int d, long n_pad, float* __restrict__ g) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    float acc = 0.f;
    if (i < n) {
        const float* r = x + i * d;
        for (int k0 = 0; k0 < d; k0 += 8) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(r + k0);
            const f32x4 hi = (k0 + 4 < d) ? *reinterpret_cast<const f32x4*>(r + k0 + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 s0, s1;
            gram_stage8<ORDER>(lo, hi, s0, s1);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc = __builtin_fmaf(s0[s], s0[s], acc);
                acc = __builtin_fmaf(s1[s], s1[s], acc);
            }
        }
    }
    g[i] = acc;
}

// One Gram tile of the [n][d] matrix m: owned rows q0 .. q0 + 63 against walked rows b0 .. b0 + 127; this wave's 32 owned x
// 64 walked part is left in acc[0..1].  Os [QT][RP] and Ws [BT][RP] are the staging buffers.  Every thread of the workgroup
// calls it (barriers inside; the first one also orders the caller's previous use of the buffers).
template <ChainOrder ORDER>
__device__ __forceinline__ void gram_tile(const float* __restrict__ m, int n, int d, long q0, long b0, float* Os, float* Ws,
                                          f32x16 (&acc)[2]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int nchunk = (d + KC - 1) / KC;
    // staging: 4 threads per row (8 features each), rows tid / 4 + 64 v; v = 0 owned, v = 1, 2 walked
    const int srow = tid >> 2, scol = (tid & 3) * 8;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tt][r] = 0.f;
    f32x4 rg[3][2];
    auto load_chunk = [&](int c) {
        const int col = c * KC + scol;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const long gr = v == 0 ? q0 + srow : b0 + srow + 64 * (v - 1);
            const float* p = m + gr * d + col;
            rg[v][0] = (gr < n && col < d) ? *reinterpret_cast<const f32x4*>(p) : zero4;
            rg[v][1] = (gr < n && col + 4 < d) ? *reinterpret_cast<const f32x4*>(p + 4) : zero4;
        }
    };
    load_chunk(0);
    for (int c = 0; c < nchunk; ++c) {
        __syncthreads();                                             // previous chunk's fragments / the caller's last use are done
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            float* dst = (v == 0 ? Os + srow * RP : Ws + (srow + 64 * (v - 1)) * RP) + scol;
            f32x4 s0, s1;
            gram_stage8<ORDER>(rg[v][0], rg[v][1], s0, s1);
            *reinterpret_cast<f32x4*>(dst) = s0;
            *reinterpret_cast<f32x4*>(dst + 4) = s1;
        }
        __syncthreads();
        if (c + 1 < nchunk) load_chunk(c + 1);
#pragma unroll
        for (int g = 0; g < KC / 8; ++g) {
            const f32x4 fo = *reinterpret_cast<const f32x4*>(Os + ((w & 1) * 32 + l31) * RP + g * 8 + 4 * half);
            const f32x4 f0 = *reinterpret_cast<const f32x4*>(Ws + ((w >> 1) * 64 + l31) * RP + g * 8 + 4 * half);
            const f32x4 f1 = *reinterpret_cast<const f32x4*>(Ws + ((w >> 1) * 64 + 32 + l31) * RP + g * 8 + 4 * half);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f0[s], fo[s], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f1[s], fo[s], acc[1], 0, 0, 0);
            }
        }
    }
}

// The workgroup's 64 x 128 tile -> St [QT][SP], which may lie over the staging buffers (barriers before and after).
// C/D map: column = lane & 31 = owned row 32 (w & 1) + .., register r of acc[tt] = walked row
// 64 (w >> 1) + 32 tt + (r & 3) + 8 (r >> 2) + 4 half.
__device__ __forceinline__ void gram_tile_to_lds(const f32x16 (&acc)[2], float* St) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    __syncthreads();                                                 // all fragment reads done: the staging buffers are dead
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v4 = {acc[tt][4 * g], acc[tt][4 * g + 1], acc[tt][4 * g + 2], acc[tt][4 * g + 3]};
            *reinterpret_cast<f32x4*>(St + ((w & 1) * 32 + l31) * SP + (w >> 1) * 64 + tt * 32 + 8 * g + 4 * half) = v4;
        }
    __syncthreads();
}

}  // namespace
