// MFMA GEMM for gfx950 (CDNA4): C[M,N] (+)= alpha * op(A)[M,K] * op(B)[K,N] with fused epilogue.
//
// One 256-thread workgroup (4 waves, 2x2) owns a 128x128 output tile; each wave a 64x64 sub-tile =
// 2x2 MFMA 32x32 accumulators.  K is walked in steps of 32 through double-buffered LDS with register
// prefetch (global loads of step k+1 are issued before the MFMAs of step k; their LDS write lands after).
//   T = bf16 : v_mfma_f32_32x32x16_bf16  (fp32 accumulate)
//   T = float: v_mfma_f32_32x32x2_f32    (exact fp32 fma chain) - the validation / high-precision path
// Operand storage ("row" = the M index of A or the N index of B):
//   TRANS=false : [row][K]  K contiguous  -> LDS image [row][K], fragments by one 16/32-byte read
//   TRANS=true  : [K][row]  row contiguous -> LDS image [K][row], fragments by 8 strided reads
// so  NT (Linear fwd: X*W^T) = <false,false>, NN (dX = dY*W) = <false,true>, TN (dW = dY^T*X) = <true,true>.
// Fragment K-order: lane half h owns k in [8h, 8h+8) of every 16-wide k-step for both operands; for
// bf16 that is the hardware map of 32x32x16, for f32 the 8 k's are fed to 8 successive 32x32x2 MFMAs
// (any bijection k->(step,half) is valid as long as A and B agree).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "common.h"

namespace {

constexpr int BM = 128, BN = 128;
// K-step per launch: bf16 64 when the grid fills the chip several times over (73 KB of LDS -> 2 workgroups / CU), 128 when
// there is at most one workgroup per CU anyway (the loop is then latency-bound per step: fewer, fatter steps win;
// measured 40 -> 26 us on 1024x2048x2048).  fp32 (validation path): 32.

struct GemmArgs {
    const void* A; const void* B; void* C;
    int M, N, K;
    long lda, ldb, ldc;
    float alpha;
    const float* bias;        // [N] fp32 or null
    int relu;
    const uint8_t* keep;      // [M][ldk] keep-mask (1 = keep) or null
    long ldk;
    float keep_scale;
    const void* gate;         // T [M][ldg]: out = gate > 0 ? out : 0
    long ldg;
    int out_f32;              // C is float even when T is bf16
    int atomic;               // 1: C (float) += via atomicAdd (split-K / concurrent accumulation); 2: C += by plain
                              // load-add-store (one launch at a time owns C: no split-K, no concurrent writers)
    int ksplit;               // gridDim.z
    const float* resid;       // fp32 [M][ldr] added to the result (out-of-place residual connection) or null
    long ldr;
    unsigned a_bytes, b_bytes; // extents of A and B for the buffer descriptors (hardware bounds check)
    int vec_epi;              // every epilogue operand allows 8-column vectors (set by epi_vectorisable)
    int xcd_remap;            // grid is a multiple of 8 workgroups: contiguous tile runs per XCD (set by the launchers)
    // row-softmax epilogues of the MoCo InfoNCE head (audiossl_moco_logits): the [B][K] logits never reach memory
    int lse_mode;             // 1: part[row][col0/64] = (max, sum exp) of alpha*acc over the wave's 64 columns
                              // 2: C (bf16) = exp(alpha*acc - lse[row]) * gscale
    float* part;              // mode 1: [M][nslot][2] fp32
    const float* lse;         // mode 2: [M]
    float gscale;
    int nslot;                // ceil(N / 64)
    // Barlow-twins epilogue (audiossl_gemm_multi_barlow): c = alpha*acc is the cross-correlation; the launch stores
    // dc = bl_dscale * (c - I) (bf16) and adds bl_coef * sum (c - I)^2 into one of 32 replicas of the loss - c itself never reaches memory
    int bl_mode;
    float* bl_loss;           // [32] fp32 replicas (workgroup i adds into replica i & 31; the caller sums them)
    float bl_coef, bl_dscale;
    // SGD epilogue (audiossl_gemm_multi_sgd): the fp32 result is a weight gradient that is consumed on the spot - parameter sgd_p and
    // momentum sgd_m ([M][ldc] fp32, indexed like C) are updated in place, the bf16 copy of the new parameter goes to sgd_s (nullable);
    // nothing is written to C
    float* sgd_p; float* sgd_m; bf16* sgd_s;
    const float* sgd_gs_dev;  // optional device scalar multiplied into the gradient scale
    float sgd_lr, sgd_mu, sgd_wd, sgd_gs;
    // dropout drawn in the epilogue (audiossl_gemm_dropout): element (row, col) is kept iff dropout_keep(seed', row * N + col) - the very
    // mask audiossl_dropout_mask would have written for an [M][N] tensor - and scaled by keep_scale; no mask tensor exists
    int drop_on;
    unsigned int drop_thr;
    unsigned long long drop_seed;
    const long long* drop_counter;
};


template <typename T> struct Mma;
template <> struct Mma<bf16> {
    __device__ __forceinline__ static void run(f32x16& acc, const Vec8<bf16>& a, const Vec8<bf16>& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    __device__ __forceinline__ static void run(f32x16& acc, const Vec8<float>& a, const Vec8<float>& b) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.lo[s], b.lo[s], acc, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.hi[s], b.hi[s], acc, 0, 0, 0);
    }
};

// Epilogue through LDS.  The accumulators of a wave (64 x 64, C/D map of the 32x32 MFMA: col = lane & 31,
// row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) are parked in a wave-private fp32 tile, then written out row by row with
// lane = column: every optional term (bias, ReLU, dropout mask, gate, residual) is a coalesced load in a short runtime loop.
// The fully unrolled per-element version this replaces was ~35 KB of straight-line code executed once per workgroup - the
// instruction fetch alone cost ~14 us per launch (a one-tile, one-k-step GEMM took 16.7 us; tools/gemm_floor.py).
constexpr int EPI_PITCH = 65;                                    // floats; odd pitch: conflict-free row reads
constexpr size_t EPI_LDS = sizeof(float) * 4 * 64 * EPI_PITCH;   // 66,560 B for four waves (8-wave workgroups: twice that)

// Accumulators -> the wave's fp32 tile [32 * MI][64] in LDS.  32x32 MFMA: C/D map col = lane & 31, row = (r & 3) + 8 * (r >> 2) +
// 4 * (lane >> 5); 16x16 MFMA: col = lane & 15, row = 4 * (lane >> 4) + r.
template <int MI>
__device__ __forceinline__ void park(const f32x16 (&acc)[MI][2], float* ct, int lane) {
    const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                ct[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * 65 + j * 32 + l31] = acc[i][j][r];
}
template <int MB>
__device__ __forceinline__ void park(const f32x4 (&acc)[MB][4], float* ct, int lane) {
    const int q = lane >> 4, c = lane & 15;
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) ct[(i * 16 + 4 * q + r) * 65 + j * 16 + c] = acc[i][j][r];
}

// MI = 32-row MFMA blocks per wave in M (wave tile = 32*MI x 64)
template <typename T, int MI, typename ACC>
__device__ __forceinline__ void epilogue_lds(const GemmArgs& g, ACC& acc, char* smem, int row0, int col0, int lane,
                                             int wave) {
    __syncthreads();                                             // every wave is done with the staging buffers
    float* ct = reinterpret_cast<float*>(smem) + wave * (32 * MI) * EPI_PITCH;
    park(acc, ct, lane);
    const int col = col0 + lane;
    if (col >= g.N) return;
    const float bias = (g.bias && blockIdx.z == 0) ? g.bias[col] : 0.f;      // split-K: the first split adds the bias
    const float floor_ = g.relu ? 0.f : -3.4e38f;
    const T* gate = static_cast<const T*>(g.gate);
    const int rows = min(32 * MI, g.M - row0);
    // 8 rows per trip: the LDS reads and the optional global loads of a trip are independent, so their latencies overlap
    // (one row per trip serialised ~150 cycles of LDS + store issue per row: 4 us of a 14 us single-tile launch)
    for (int r0 = 0; r0 < rows; r0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = ct[min(r0 + u, 32 * MI - 1) * EPI_PITCH + lane];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long row = row0 + min(r0 + u, rows - 1);
            float x = fmaxf(g.alpha * v[u] + bias, floor_);
            if (g.keep) x = g.keep[row * g.ldk + col] ? x * g.keep_scale : 0.f;
            if (g.drop_on) x = dropout_keep(dropout_seed(g.drop_seed, g.drop_counter), row * g.N + col, g.drop_thr) ? x * g.keep_scale : 0.f;
            if (gate) x = to_f32(gate[row * g.ldg + col]) > 0.f ? x : 0.f;
            if (g.resid) x += g.resid[row * g.ldr + col];
            v[u] = x;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (r0 + u >= rows) break;
            const long o = (long)(row0 + r0 + u) * g.ldc + col;
            if (g.sgd_p) {
                float pj = g.sgd_p[o], b = g.sgd_m[o];
                sgd_step(pj, v[u], b, g.sgd_lr, g.sgd_mu, g.sgd_wd, g.sgd_gs_dev ? g.sgd_gs * g.sgd_gs_dev[0] : g.sgd_gs, false);
                g.sgd_p[o] = pj; g.sgd_m[o] = b;
                if (g.sgd_s) g.sgd_s[o] = (bf16)pj;
                continue;
            }
            if (g.atomic == 1)  atomicAdd(static_cast<float*>(g.C) + o, v[u]);
            else if (g.atomic)  static_cast<float*>(g.C)[o] += v[u];
            else if (g.out_f32) static_cast<float*>(g.C)[o] = v[u];
            else                static_cast<T*>(g.C)[o] = from_f32<T>(v[u]);
        }
    }
}

// The same with 8 consecutive columns per lane (8 rows x 64 columns per wave trip): 16-byte stores of bf16 results (two for
// fp32), 8-byte keep-mask loads, 16-byte gate / residual loads.  The one-column-per-lane form above issues a 128-byte
// store per row and wave - on the 6144 x 2048 Linear layers of the encoder the epilogue then took longer than the k-loop
// (70 us at K = 512 against 113 us at K = 2048).  bf16 operands, non-atomic results, N % 8 == 0 and aligned operands only.
template <int MI, typename ACC>
__device__ __forceinline__ void epilogue_vec(const GemmArgs& g, ACC& acc, char* smem, int row0, int col0, int lane,
                                             int wave) {
    __syncthreads();
    float* ct = reinterpret_cast<float*>(smem) + wave * (32 * MI) * EPI_PITCH;
    park(acc, ct, lane);
    const int c8 = (lane & 7) * 8, rr = lane >> 3;
    const int col = col0 + c8;
    if (col >= g.N) return;
    float bias[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) bias[u] = 0.f;
    if (g.bias && blockIdx.z == 0) {
        const Vec8<float> b = Vec8<float>::load(g.bias + col);
#pragma unroll
        for (int u = 0; u < 8; ++u) bias[u] = b.get(u);
    }
    const float floor_ = g.relu ? 0.f : -3.4e38f;
    const bf16* gate = static_cast<const bf16*>(g.gate);
    float bl_acc = 0.f;
#pragma unroll 2
    for (int r0 = 0; r0 < 32 * MI; r0 += 8) {
        const int rl = r0 + rr;
        const long row = row0 + rl;
        if (row >= g.M) continue;
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = fmaxf(g.alpha * ct[rl * EPI_PITCH + c8 + u] + bias[u], floor_);
        if (g.bl_mode) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float d = v[u] - (row == col + u ? 1.f : 0.f);
                bl_acc += d * d;
                v[u] = g.bl_dscale * d;
            }
        }
        if (g.keep) {
            const unsigned long long k8 = *reinterpret_cast<const unsigned long long*>(g.keep + row * g.ldk + col);
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ((k8 >> (8 * u)) & 0xFFull) ? v[u] * g.keep_scale : 0.f;
        }
        if (g.drop_on) {
            const unsigned long long sd = dropout_seed(g.drop_seed, g.drop_counter);
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = dropout_keep(sd, row * g.N + col + u, g.drop_thr) ? v[u] * g.keep_scale : 0.f;
        }
        if (gate) {
            const Vec8<bf16> gt = Vec8<bf16>::load(gate + row * g.ldg + col);
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = gt.get(u) > 0.f ? v[u] : 0.f;
        }
        if (g.resid) {
            const Vec8<float> rs = Vec8<float>::load(g.resid + row * g.ldr + col);
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] += rs.get(u);
        }
        const long o = row * g.ldc + col;
        if (g.sgd_p) {
            const float gs = g.sgd_gs_dev ? g.sgd_gs * g.sgd_gs_dev[0] : g.sgd_gs;
            Vec8<float> pv = Vec8<float>::load(g.sgd_p + o), mv = Vec8<float>::load(g.sgd_m + o);
            Vec8<bf16> sv;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float pj = pv.get(u), b = mv.get(u);
                sgd_step(pj, v[u], b, g.sgd_lr, g.sgd_mu, g.sgd_wd, gs, false);
                pv.set(u, pj); mv.set(u, b); sv.set(u, pj);
            }
            pv.store(g.sgd_p + o);
            mv.store(g.sgd_m + o);
            if (g.sgd_s) sv.store(g.sgd_s + o);
            continue;
        }
        if (g.out_f32) {
            Vec8<float> out;
            if (g.atomic) {                                   // exclusive accumulation (atomic == 2)
                const Vec8<float> c0 = Vec8<float>::load(static_cast<const float*>(g.C) + o);
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] += c0.get(u);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) out.set(u, v[u]);
            out.store(static_cast<float*>(g.C) + o);
        } else {
            Vec8<bf16> out;
#pragma unroll
            for (int u = 0; u < 8; ++u) out.set(u, v[u]);
            out.store(static_cast<bf16*>(g.C) + o);
        }
    }
    if (g.bl_mode) {                                          // N % 64 == 0 here: no lane left the function early
        bl_acc = wave_sum(bl_acc);
        if (lane == 0) atomicAdd(g.bl_loss + (blockIdx.x & 31), g.bl_coef * bl_acc);
    }
}

// Row-softmax epilogues (MoCo InfoNCE, `delores_m/upstream_expert.py:250-264`): logits = alpha * acc are reduced / transformed
// in the tile and never stored.  Same parking of the accumulators as above; a lane owns 8 consecutive columns of one of 8 rows.
template <int MI, typename ACC>
__device__ __forceinline__ void epilogue_softmax(const GemmArgs& g, ACC& acc, char* smem, int row0, int col0, int lane,
                                                 int wave) {
    __syncthreads();
    float* ct = reinterpret_cast<float*>(smem) + wave * (32 * MI) * EPI_PITCH;
    park(acc, ct, lane);
    const int c8 = (lane & 7) * 8, rr = lane >> 3;
    const int col = col0 + c8;
    if (col0 >= g.N) return;                                   // the whole wave tile is outside (wave-uniform)
#pragma unroll 2
    for (int r0 = 0; r0 < 32 * MI; r0 += 8) {
        const int rl = r0 + rr;
        const long row = row0 + rl;
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (col + u < g.N) ? g.alpha * ct[rl * EPI_PITCH + c8 + u] : -3.0e38f;
        if (g.lse_mode == 1) {
            float m = v[0];
#pragma unroll
            for (int u = 1; u < 8; ++u) m = fmaxf(m, v[u]);
            float sm = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) sm += __expf(v[u] - m);
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {                   // the 8 lanes of a row are consecutive
                const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(sm, o, 64);
                const float mm = fmaxf(m, m2);
                sm = sm * __expf(m - mm) + s2 * __expf(m2 - mm);
                m = mm;
            }
            if ((lane & 7) == 0 && row < g.M) {
                float* o = g.part + (row * g.nslot + (col0 >> 6)) * 2;
                o[0] = m; o[1] = sm;
            }
        } else if (row < g.M && col < g.N) {
            const float l = g.lse[row];
            Vec8<bf16> out;
#pragma unroll
            for (int u = 0; u < 8; ++u) out.set(u, __expf(v[u] - l) * g.gscale);
            out.store(static_cast<bf16*>(g.C) + row * g.ldc + col);
        }
    }
}

// MI = 32-row blocks of the wave tile; ACC = f32x16 [MI][2] (32x32 MFMA) or f32x4 [2 * MI][4] (16x16 MFMA)
template <typename T, int MI, typename ACC>
__device__ __forceinline__ void epilogue(const GemmArgs& g, ACC& acc, char* smem, int row0, int col0, int lane, int wave) {
    if constexpr (sizeof(T) == 2) {
        if (g.lse_mode) { epilogue_softmax<MI>(g, acc, smem, row0, col0, lane, wave); return; }
        if (g.vec_epi) { epilogue_vec<MI>(g, acc, smem, row0, col0, lane, wave); return; }
    }
    epilogue_lds<T, MI>(g, acc, smem, row0, col0, lane, wave);
}

// One operand's staging: 128 rows x 32 k per step, two Vec8 per thread.
template <typename T, bool TRANS, int BK_, int ROWS = 128, int NTH = 256>
struct Stage {
    static constexpr int BK = BK_;
    static constexpr int NT_PITCH = BK + 8;          // elements; [row][k] image, conflict-free 16-byte row reads
    static constexpr int TR_PITCH = ROWS + 32;       // elements; [k][row] image: 4 consecutive k-rows fall on distinct 32-byte bank groups
    static constexpr int VR = ROWS / 8;              // vectors per k-row of the [k][row] image
    static constexpr int NV = ROWS * BK / 8 / NTH;   // 8-element vectors per thread and step
    static constexpr int VPR = BK / 8;               // vectors per row of the [row][k] image
    Vec8<T> r[NV];
    // Branch-free staging loads: a raw buffer load per 16 bytes, out-of-range vectors get an offset past the
    // descriptor's extent and come back as zeros (no exec-masked branches -> the compiler keeps counted vmcnt waits).
    // rows = extent of the row dimension (M or N); kend = exclusive K bound of this split
    __device__ __forceinline__ static Vec8<bf16> bload16(__amdgpu_buffer_rsrc_t rs, unsigned off) {
        Vec8<bf16> r;
        r.v = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        return r;
    }
    __device__ __forceinline__ static Vec8<float> bload32(__amdgpu_buffer_rsrc_t rs, unsigned off) {
        Vec8<float> r;
        r.lo = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        r.hi = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16u, 0, 0));
        return r;
    }
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, long ld, int row0, int rows, int k0, int kend) {
        const int t = threadIdx.x;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = t + i * NTH;
            int row, k;
            long idx;
            if (!TRANS) { row = row0 + v / VPR; k = k0 + (v % VPR) * 8; idx = (long)row * ld + k; }
            else        { k = k0 + v / VR; row = row0 + (v % VR) * 8; idx = (long)k * ld + row; }
            const unsigned off = (row < rows && k < kend) ? (unsigned)(idx * (long)sizeof(T)) : 0xFFFFFFE0u;
            r[i] = select_load(rs, off, (T*)nullptr);
        }
    }
    __device__ __forceinline__ static Vec8<bf16> select_load(__amdgpu_buffer_rsrc_t rs, unsigned off, bf16*) { return bload16(rs, off); }
    __device__ __forceinline__ static Vec8<float> select_load(__amdgpu_buffer_rsrc_t rs, unsigned off, float*) { return bload32(rs, off); }
    __device__ __forceinline__ void put(T* lds) const {
        const int t = threadIdx.x;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = t + i * NTH;
            if (!TRANS) r[i].store(lds + (v / VPR) * NT_PITCH + (v % VPR) * 8);
            else        r[i].store(lds + (v / VR) * TR_PITCH + (v % VR) * 8);
        }
    }
    // fragment of 32 rows starting at `row`, k-step `kk` (0 or 16) for this lane
    __device__ __forceinline__ static Vec8<T> frag(const T* lds, int row, int kk, int lane) {
        const int r_ = row + (lane & 31), kb = kk + 8 * (lane >> 5);
        if (!TRANS) return Vec8<T>::load(lds + r_ * NT_PITCH + kb);
        return frag_trans(lds, row, kb, r_, lane);
    }
    // [k][row] image -> 8 consecutive k of one row.  bf16: two ds_read_b64_tr_b16 (each 16-lane group transposes a
    // 4 (k) x 16 (row) block: lane 4q+p supplies the address of k-row q, columns 4p..4p+3, and receives column i);
    // fp32: 8 scalar reads (validation path).
    __device__ __forceinline__ static Vec8<float> frag_trans(const float* lds, int, int kb, int r_, int) {
        Vec8<float> f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f.set(j, lds[(kb + j) * TR_PITCH + r_]);
        return f;
    }
    __device__ __forceinline__ static Vec8<bf16> frag_trans(const bf16* lds, int row, int kb, int, int lane) {
        typedef __attribute__((address_space(3))) bf16x4* lds4_t;
        const int i = lane & 15, q = i >> 2, p = i & 3;
        const bf16* a = lds + (kb + q) * TR_PITCH + row + 16 * ((lane >> 4) & 1) + 4 * p;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4_t)a);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4_t)(a + 4 * TR_PITCH));
        Vec8<bf16> f;
        f.v = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return f;
    }
    static constexpr int LDS_ELEMS = TRANS ? BK * TR_PITCH : ROWS * NT_PITCH;
};

// NW = 4 waves (2 x 2): 128 x 128 tile (MI = 2) or 64 x 128 (MI = 1: twice the workgroups for grids that would leave CUs idle).
// NW = 8 waves (4 x 2): 256 x 128 tile - twice the MFMA work per byte staged (the 128 x 128 tile needs as many L1->LDS cycles
// per k-step as MFMA cycles) and two waves per SIMD, so one wave's MFMAs cover the other's LDS reads and staging stores.
template <typename T, bool TA, bool TB, int BK, int MI, int NW = 4, bool SPLIT_EPI = false>
__device__ __forceinline__ void gemm_body(const GemmArgs& g, char* smem, int wg) {
    constexpr int BMv = 16 * MI * NW;
    using SA = Stage<T, TA, BK, BMv, 64 * NW>;
    using SB = Stage<T, TB, BK, BN, 64 * NW>;
    T* const ldsA0 = reinterpret_cast<T*>(smem);                 // two A buffers, then two B buffers
    T* const ldsB0 = ldsA0 + 2 * SA::LDS_ELEMS;

    const int tiles_n = (g.N + BN - 1) / BN;
    const int bm = (wg / tiles_n) * BMv, bn = (wg % tiles_n) * BN;
    // split-K range, in whole BK steps
    const int ksteps = (g.K + BK - 1) / BK;
    const int per = (ksteps + g.ksplit - 1) / g.ksplit;
    const int ks0 = blockIdx.z * per, ks1 = min(ksteps, ks0 + per);
    if (ks0 >= ks1) return;
    const int kend = min(g.K, ks1 * BK);

    const __amdgpu_buffer_rsrc_t A = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.A), 0, g.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t B = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.B), 0, g.b_bytes, 0x00020000);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = (wave >> 1) * 32 * MI, wn = (wave & 1) * 64;

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // Double-buffered LDS + one register stage: the loads of step k+1 are issued before the MFMAs of step k and land in
    // LDS after them (counted vmcnt, no branches).  A second register stage (prefetch distance 2) was measured slower:
    // hipcc aliases the staging and fragment registers and drains vmcnt at the loop back-edge (gpurun_out/gemm_d2.log).
    SA sa; SB sb;
    sa.load(A, g.lda, bm, g.M, ks0 * BK, kend);
    sb.load(B, g.ldb, bn, g.N, ks0 * BK, kend);
    sa.put(ldsA0); sb.put(ldsB0);
    __syncthreads();

    int cur = 0;
    for (int ks = ks0; ks < ks1; ++ks) {
        const bool more = ks + 1 < ks1;
        if (more) {
            sa.load(A, g.lda, bm, g.M, (ks + 1) * BK, kend);
            sb.load(B, g.ldb, bn, g.N, (ks + 1) * BK, kend);
        }
        const T* la = ldsA0 + cur * SA::LDS_ELEMS;
        const T* lb = ldsB0 + cur * SB::LDS_ELEMS;
#pragma unroll
        for (int kk = 0; kk < BK; kk += 16) {
            Vec8<T> fa[MI], fb[2];
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[i] = SA::frag(la, wm + i * 32, kk, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = SB::frag(lb, wn + j * 32, kk, lane);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) Mma<T>::run(acc[i][j], fa[i], fb[j]);
        }
        if (more) { sa.put(ldsA0 + (cur ^ 1) * SA::LDS_ELEMS); sb.put(ldsB0 + (cur ^ 1) * SB::LDS_ELEMS); }
        __syncthreads();
        cur ^= 1;
    }

    if constexpr (SPLIT_EPI && MI == 2) {                    // half-height epilogue tile: 33 KB of LDS instead of 66.5 KB
        epilogue<T, 1>(g, *reinterpret_cast<f32x16 (*)[1][2]>(&acc[0]), smem, bm + wm, bn + wn, lane, wave);
        epilogue<T, 1>(g, *reinterpret_cast<f32x16 (*)[1][2]>(&acc[1]), smem, bm + wm + 32, bn + wn, lane, wave);
    } else {
        epilogue<T, MI>(g, acc, smem, bm + wm, bn + wn, lane, wave);
    }
}

template <typename T, bool TA, bool TB, int BK, int MI, int NW = 4>
__global__ __launch_bounds__(64 * NW) void gemm_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // Workgroups are dealt to the 8 XCDs round-robin (id mod 8), each with its own 4 MB L2.  Give every XCD a CONTIGUOUS run
    // of tiles (whole tile rows: one A row panel is then fetched into one L2 instead of all eight) - operand re-reads
    // that miss L2 are served by the Infinity Cache at about half the L2 rate, which bounded the 6144-row GEMMs.
    gemm_body<T, TA, TB, BK, MI, NW>(g, smem, g.xcd_remap ? (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) : (int)blockIdx.x);
}

// Several independent problems of one kind in ONE launch (blockIdx.y = problem): the three Barlow heads of delores_m run
// the same chain of GEMMs on different operands; issued as separate launches on separate streams they were serialised by
// the hardware-queue mapping of the graph executor (1.6 ms of a 3.3 ms step), and each launch filled half the chip at best.
constexpr int MAX_MULTI = 4;
// tile_end: running totals of the problems' tile counts for the tile shape of the kernel that is launched (set by multi_grid)
struct GemmMulti { GemmArgs p[MAX_MULTI]; int tile_end[MAX_MULTI]; int total; };

// One-dimensional grid over the tiles of ALL problems, padded to a multiple of 8 workgroups.  Workgroup ids go to the XCDs round-
// robin, so id -> (id & 7) * (grid / 8) + (id >> 3) hands every XCD a CONTIGUOUS run of the concatenated tile list: whole tile
// rows of ONE problem (its A panels and its B operand meet in one L2) instead of a slice of every tile row of every problem -
// the multi-problem launches of round 2 re-fetched their operands 4.2 x (86.6 MB per launch against 21 MB, PMC), and the grid was
// sized for the widest problem (idle workgroups for the narrower ones).  -> problem index (-1: padding), tile index in `wg`.
__device__ __forceinline__ int multi_locate(const GemmMulti& gm, int& wg) {
    const int v = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (v >= gm.total) return -1;
    int p = 0;
    while (v >= gm.tile_end[p]) ++p;
    wg = v - (p ? gm.tile_end[p - 1] : 0);
    return p;
}
// host side: fills tile_end / total for BMt x BNt tiles, returns the grid size
static int multi_grid(GemmMulti& gm, int count, int BMt, int BNt) {
    int tot = 0;
    for (int i = 0; i < MAX_MULTI; ++i) {
        if (i < count) tot += ceil_div(gm.p[i].M, BMt) * ceil_div(gm.p[i].N, BNt);
        gm.tile_end[i] = tot;
    }
    gm.total = tot;
    return (tot + 7) / 8 * 8;
}

template <typename T, bool TA, bool TB, int BK, int MI, int NW = 4>
__global__ __launch_bounds__(64 * NW) void gemm_multi_kernel(GemmMulti gm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int wg;
    const int p = multi_locate(gm, wg);
    if (p < 0) return;
    gemm_body<T, TA, TB, BK, MI, NW>(gm.p[p], smem, wg);
}

template <typename T, bool TA, bool TB, int BK, int MI, int NW>
constexpr size_t gemm_lds() {
    constexpr size_t stage = sizeof(T) * 2 * (Stage<T, TA, BK, 16 * MI * NW, 64 * NW>::LDS_ELEMS + Stage<T, TB, BK, BN, 64 * NW>::LDS_ELEMS);
    constexpr size_t epi = EPI_LDS * (NW / 4);
    return stage > epi ? stage : epi;
}


// ---------------------------------------------------------------------------------------------------------------------
// bf16 with direct-to-LDS staging (`global_load_lds_dwordx4`) and an NST-deep ring: the pipelined variant.  The
// register-staged kernel above keeps ONE 64-deep k-step in flight per workgroup, so a k-step costs a full global-load
// latency (~1 us against 0.1-0.2 us of MFMA work on the projector shapes of the step); here up to NST-1 stages are in
// flight across a single raw barrier per step, waited for with counted s_waitcnt vmcnt(N) (never 0 in steady state).
//   * an LDS-DMA instruction writes wave-uniform base + lane * 16 B, so a stage image is the plain tile with no padding;
//     bank conflicts of the fragment reads are removed by XOR swizzles applied to the SOURCE address of the DMA and to
//     the ds_read address:
//       [row][64 k] image (K-contiguous operand, 128-byte rows): 16-byte chunk ^= (row >> 1) & 7
//       [64 k][R rows] image (row-contiguous operand, read with ds_read_b64_tr_b16): 64-byte group ^= k & 3 (R = 128)
//         or ^= (k >> 1) & 1 (R = 64), so the four k-rows one transposing read touches fall on four distinct bank groups;
//   * rows past M / N are clamped to the last row / last 8-row chunk (their results are never stored); K % 64 == 0.
constexpr int GBK = 64;

__device__ __forceinline__ void glds16(const bf16* src, char* dst) {
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
}

template <int N_> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory"); }

// One operand of the ring: R rows x 64 k per stage.
template <bool TRANS, int R>
struct RingOp {
    static constexpr int BYTES = R * GBK * 2;
    static constexpr int NI = BYTES / 4096;                  // DMA instructions per wave and stage (1 KiB each, 4 waves)
    static constexpr int NB = R / 64;                        // 32-row fragment blocks per wave
    const bf16* p[NI];
    long kstride;
    int foff[NB], fsw[NB];
    __device__ __forceinline__ void init(const void* base_, long ld, int r0, int ext, int k0, int wave, int lane, int wr) {
        const bf16* base = static_cast<const bf16*>(base_);
        if (!TRANS) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int rl = wave * (R / 4) + i * 8 + (lane >> 3);
                const int sc = (lane & 7) ^ ((rl >> 1) & 7);
                p[i] = base + (long)min(r0 + rl, ext - 1) * ld + sc * 8 + k0;
            }
            kstride = GBK;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int r = wr + b * 32 + (lane & 31);
                foff[b] = r * 128; fsw[b] = (r >> 1) & 7;
            }
        } else {
            constexpr int CPR = R / 8;                       // 16-byte chunks per k-row
            constexpr int KPI = 64 / CPR;                    // k-rows per DMA instruction
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int kl = wave * 16 + i * KPI + lane / CPR, pc = lane % CPR;
                const int sw = R == 128 ? (kl & 3) : ((kl >> 1) & 1);
                const int roff = ((((pc >> 2) ^ sw) << 2) + (pc & 3)) * 8;
                p[i] = base + (long)(k0 + kl) * ld + min(r0 + roff, ext - 8);
            }
            kstride = (long)GBK * ld;
            const int q = (lane & 15) >> 2, pp = lane & 3, h4 = (lane >> 4) & 1, half = lane >> 5;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int grp = ((wr + b * 32) >> 5) ^ (R == 128 ? q : (q >> 1));
                foff[b] = (8 * half + q) * (R * 2) + grp * 64 + 32 * h4 + 8 * pp; fsw[b] = 0;
            }
        }
    }
    __device__ __forceinline__ void issue(long st, char* dst) const {
#pragma unroll
        for (int i = 0; i < NI; ++i) glds16(p[i] + st * kstride, dst + i * 1024);
    }
    // fragment of block b, 16-wide k-step kk (0..3) of the stage image at `img`
    __device__ __forceinline__ Vec8<bf16> frag(const char* img, int b, int kk, int half) const {
        if (!TRANS) return Vec8<bf16>::load(reinterpret_cast<const bf16*>(img + foff[b] + (((kk * 2 + half) ^ fsw[b]) << 4)));
        typedef __attribute__((address_space(3))) bf16x4* lds4_t;
        const char* a = img + foff[b] + kk * 16 * (R * 2);
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4_t)a);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4_t)(a + 4 * (R * 2)));
        Vec8<bf16> f;
        f.v = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return f;
    }
};

template <bool TA, bool TB, int MI, int NST>
__global__ __launch_bounds__(256) void gemm_ring_kernel(GemmArgs g) {
    constexpr int RA = 64 * MI;
    using OA = RingOp<TA, RA>;
    using OB = RingOp<TB, 128>;
    constexpr int STAGE = OA::BYTES + OB::BYTES;
    constexpr int NPS = OA::NI + OB::NI;                     // DMA instructions per wave and stage
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tiles_n = (g.N + BN - 1) / BN;
    // blocks that share an XCD (ids congruent mod 8) get consecutive tiles: they share A row panels / B column panels in L2
    const int nwg = gridDim.x, xcd = blockIdx.x & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
    const int bm = (wg / tiles_n) * RA, bn = (wg % tiles_n) * BN;
    const int ksteps = g.K / GBK;
    const int per = (ksteps + g.ksplit - 1) / g.ksplit;
    const int ks0 = blockIdx.z * per, ks1 = min(ksteps, ks0 + per);
    if (ks0 >= ks1) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const int wm = (wave >> 1) * 32 * MI, wn = (wave & 1) * 64;

    OA oa; OB ob;
    oa.init(g.A, g.lda, bm, g.M, ks0 * GBK, wave, lane, wm);
    ob.init(g.B, g.ldb, bn, g.N, ks0 * GBK, wave, lane, wn);
    char* const wa = smem + wave * (OA::BYTES / 4);          // this wave's slice of the A image / the B image of slot 0
    char* const wb = smem + OA::BYTES + wave * (OB::BYTES / 4);

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = ks1 - ks0;
    int islot = 0;                                           // ring slot the next issued stage goes to
    auto issue = [&](int st) {
        oa.issue(st, wa + islot * STAGE);
        ob.issue(st, wb + islot * STAGE);
        islot = islot + 1 == NST ? 0 : islot + 1;
    };
    for (int st = 0; st < NST - 1 && st < nk; ++st) issue(st);

    int cslot = 0;
    for (int it = 0; it < nk; ++it) {
        const int ahead = min(nk - 1 - it, NST - 2);
        if (ahead == 0) wait_vm<0>();                        // all but the `ahead` youngest stages have landed
        else if (ahead == 1) wait_vm<NPS>();
        else if (ahead == 2) wait_vm<2 * NPS>();
        else if (ahead == 3) wait_vm<3 * NPS>();
        else wait_vm<4 * NPS>();
        __builtin_amdgcn_s_barrier();                        // stage `it` visible to every wave; slot of stage it-1 free again
        if (it + NST - 1 < nk) issue(it + NST - 1);
        const char* sa = smem + cslot * STAGE;
        const char* sb = sa + OA::BYTES;
        cslot = cslot + 1 == NST ? 0 : cslot + 1;
        // fragment reads run one k-step ahead of the MFMAs that consume them
        Vec8<bf16> fa[2][MI], fb[2][2];
#pragma unroll
        for (int i = 0; i < MI; ++i) fa[0][i] = oa.frag(sa, i, 0, half);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[0][j] = ob.frag(sb, j, 0, half);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            if (kk < 3) {
#pragma unroll
                for (int i = 0; i < MI; ++i) fa[nxt][i] = oa.frag(sa, i, kk + 1, half);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[nxt][j] = ob.frag(sb, j, kk + 1, half);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) Mma<bf16>::run(acc[i][j], fa[cur][i], fb[cur][j]);
        }
    }

    epilogue<bf16, MI>(g, acc, smem, bm + wm, bn + wn, lane, wave);
}


// ---------------------------------------------------------------------------------------------------------------------
// 256 x 256 output tile, 8 waves (2 x 4, wave tile 128 x 64), K-tile 64, eight phases per pair of K-tiles: the
// hand-scheduled main loop.  What bounded the kernels above was the loop SHAPE (one fat k-step: issue loads, read fragments,
// MFMA, wait for everything, barrier): 31 % MFMA-busy on 6144 x 2048 x 2048, waves parked at s_waitcnt / the barrier.
// Here
//   * a K-tile is staged as FOUR 16 KB parts - A(r0), B(c0), B(c1), A(r1): the 64-row halves of every wave's 128 rows and
//     the 32-column halves of every wave's 64 columns - by direct-to-LDS DMA, two 1 KB instructions per wave and part;
//   * a phase = one quadrant (64 x 32 x K 64 = 8 MFMA 32x32x16) of every wave's tile; it issues ONE part of a later K-tile,
//     reads only the fragments that are new for its quadrant (A(r0) + B(c0), then B(c1), then A(r1), then nothing), runs
//     its MFMAs under s_setprio, waits with a COUNTED vmcnt that leaves five parts (80 KB) in flight, and meets the other
//     waves at ONE raw s_barrier;
//   * a part is re-staged no earlier than the phase after the barrier that followed its last fragment read (WAR), and is read
//     no earlier than the phase after the barrier that followed the wait that retired it (RAW): with the issue order
//     A(r0) B(c0) B(c1) A(r1) per K-tile and the consumption order the same, "everything but the five youngest parts has
//     landed" is exactly what each phase needs, so the wait is the same vmcnt(10) in every steady-state phase.
// Two buffers x four parts = 128 KB of LDS; accumulators 128 VGPRs + 64 of fragments.  Operand layouts as the ring kernel
// (K-contiguous: [row][64 k] image, 16-byte chunk ^= (row >> 1) & 7; row-contiguous: [64 k][128 rows] image read with
// ds_read_b64_tr_b16, 64-byte group ^= k & 3), the swizzle applied to the DMA's source address.  K % 64 == 0.
// GROUP = rows of ONE wave row (column) inside a part, STRIDE = tile rows between consecutive wave rows: part-row p of part X is
// tile row (p / GROUP) * STRIDE + X * GROUP + p % GROUP.  256 x 256 kernel: A <64, 128>, B <32, 64>; 256 x 128 kernel: A <32, 64>, B <64, 64>.
template <bool TRANS, int GROUP, int STRIDE>
struct PartOp {
    static constexpr int NBLK = GROUP / 32;                  // 32-row fragment blocks of this wave inside a part
    // DMA = buffer_load_dwordx4 ... lds: 32-bit per-lane byte offsets (two instructions per part), everything that is uniform -
    // tile origin, K-tile, part - in the scalar offset; rows / columns past the matrix read zeros or other valid elements of the
    // buffer (the descriptor bounds the access), their results are never stored
    __amdgpu_buffer_rsrc_t rsrc;
    int voff[2];
    int kstride, part_delta, base_off;                       // bytes; wave-uniform
    int foff[NBLK], fsw[NBLK];
    __device__ __forceinline__ void init(const void* base_, unsigned bytes, long ld, int r0, int k0, int wave, int lane, int wsel) {
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base_), 0, bytes, 0x00020000);
        const int w0 = wsel * GROUP;                         // this wave's first part-row
        if (!TRANS) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int p = wave * 16 + i * 8 + (lane >> 3);
                const int sc = (lane & 7) ^ ((p >> 1) & 7);
                const int row = (p / GROUP) * STRIDE + (p % GROUP);
                voff[i] = (int)(((long)row * ld + sc * 8) * 2);
            }
            kstride = GBK * 2;
            part_delta = (int)(GROUP * ld * 2);
            base_off = (int)(((long)r0 * ld + k0) * 2);
#pragma unroll
            for (int b = 0; b < NBLK; ++b) {
                const int p = w0 + b * 32 + (lane & 31);
                foff[b] = p * 128; fsw[b] = (p >> 1) & 7;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int kl = wave * 8 + i * 4 + (lane >> 4), pc = lane & 15;
                const int roff = ((((pc >> 2) ^ (kl & 3)) << 2) + (pc & 3)) * 8;
                const int row = (roff / GROUP) * STRIDE + (roff % GROUP);
                voff[i] = (int)(((long)kl * ld + row) * 2);
            }
            kstride = (int)(GBK * ld * 2);
            part_delta = GROUP * 2;
            base_off = (int)(((long)k0 * ld + r0) * 2);
            const int q = (lane & 15) >> 2, pp = lane & 3, h4 = (lane >> 4) & 1, half = lane >> 5;
#pragma unroll
            for (int b = 0; b < NBLK; ++b) {
                const int grp = ((w0 + b * 32) >> 5) ^ q;
                foff[b] = (8 * half + q) * 256 + grp * 64 + 32 * h4 + 8 * pp; fsw[b] = 0;
            }
        }
    }
    __device__ __forceinline__ void issue(int part, int st, char* dst, bool live) const {
        typedef __attribute__((address_space(3))) void* lptr_t;
        const int so = live ? base_off + st * kstride + part * part_delta : 0x7FFFFF00;        // past the buffer: zeros, no traffic
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)dst, 16, voff[0], so, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)(dst + 1024), 16, voff[1], so, 0, 0);
    }
    __device__ __forceinline__ Vec8<bf16> frag(const char* img, int b, int kk, int half) const {
        if (!TRANS) return Vec8<bf16>::load(reinterpret_cast<const bf16*>(img + foff[b] + (((kk * 2 + half) ^ fsw[b]) << 4)));
        // The transposing reads go through inline asm: behind an LDS-DMA in flight hipcc waits vmcnt(0) before a
        // ds_read_b64_tr_b16 BUILTIN (it treats the DMA as a store the read may alias), which drained the pipeline in every
        // phase.  The caller's s_waitcnt lgkmcnt(0) + sched_barrier after the section's barrier covers these reads.
        typedef __attribute__((address_space(3))) const char* lds_t;
        const unsigned a = (unsigned)(size_t)(lds_t)(img + foff[b] + kk * 16 * 256);
        bf16x4 lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a) : "memory");
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(hi) : "v"(a) : "memory");
        Vec8<bf16> f;
        f.v = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return f;
    }
};

constexpr int P8_PART = 16384, P8_BUF = 4 * P8_PART;         // slot order inside a buffer: A(r0) B(c0) B(c1) A(r1)

// Workgroup ids are dealt to the 8 XCDs round-robin (id mod 8): give every XCD a CONTIGUOUS run of tiles, so that the tiles of a
// row (one A panel) and neighbouring rows meet in one L2.  Bijective for any grid size.
__device__ __forceinline__ int xcd_contiguous(int id, int nwg) {
    const int xcd = id & 7, q8 = nwg >> 3, r8 = nwg & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (id >> 3);
}

template <bool TA, bool TB, int DBG = 0>
__device__ __forceinline__ void p8_body(const GemmArgs& g, char* smem, int wg) {
    const int tiles_n = (g.N + 255) / 256;
    const int bm = (wg / tiles_n) * 256, bn = (wg % tiles_n) * 256;
    const int ksteps = g.K / GBK;
    const int per = (ksteps + g.ksplit - 1) / g.ksplit;
    const int ks0 = blockIdx.z * per, ks1 = min(ksteps, ks0 + per);
    if (ks0 >= ks1) return;
    const int nk = ks1 - ks0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const int wr = wave >> 2, wc = wave & 3;

    PartOp<TA, 64, 128> oa; PartOp<TB, 32, 64> ob;
    oa.init(g.A, g.a_bytes, g.lda, bm, ks0 * GBK, wave, lane, wr);
    ob.init(g.B, g.b_bytes, g.ldb, bn, ks0 * GBK, wave, lane, wc);
    char* const wdst = smem + wave * 2048;                   // this wave's 2 KB slice of every part image

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // slot: 0 A(r0), 1 B(c0), 2 B(c1), 3 A(r1).  A part of a K-tile past the end is still "issued" (branch-free, the counted
    // waits stay uniform) but with a scalar offset past the buffer: the descriptor turns it into a no-traffic load of zeros
    auto issue = [&](int slot, int t, int buf) {
        char* d = wdst + buf * P8_BUF + slot * P8_PART;
        const bool live = t < nk && !((DBG & 2) && t >= 2);
        if (slot == 0) oa.issue(0, t, d, live); else if (slot == 3) oa.issue(1, t, d, live);
        else ob.issue(slot - 1, t, d, live);
    };
    // A phase has two sections, each closed by a raw s_barrier: LOAD (issue one part, read this quadrant's new fragments, wait
    // until everything but the five youngest parts has landed and the fragment reads have returned) and MFMA.  The two waves
    // of a SIMD (wave rows wr = 0 / 1) run ONE SECTION APART - wr = 1 passes an extra barrier up front, wr = 0 one at the end -
    // so while one of them issues MFMAs the other issues its DMA and LDS reads instead of both doing the same thing at once
    // (in lockstep the MFMA pipe idled during every load section: 67.7 us on 6144 x 2048 x 2048 against 45 us of MFMA sections alone).
    // RAW / WAR as above: a part read in phase p + 1 was retired by every wave's wait in its LOAD section of phase p, and the
    // later of those sections is followed by a barrier before the earlier reader starts; a part is re-staged at least one phase
    // after its last read, i.e. after a barrier that follows the later group's (completed: lgkmcnt(0)) reads.
    auto load_end = [&]() {
        wait_vm<8>();                                        // all but the four youngest parts have landed
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this section's fragment reads (they returned while waiting at the barrier)
        __builtin_amdgcn_sched_barrier(0);
    };
    auto sync = [&]() {                                      // end of the MFMA section
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    Vec8<bf16> fa[2][4], fb0[4], fb1[4];
    if (DBG & 4) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) { fa[0][kk] = Vec8<bf16>::zero(); fa[1][kk] = Vec8<bf16>::zero(); fb0[kk] = Vec8<bf16>::zero(); fb1[kk] = Vec8<bf16>::zero(); }
    }
    auto loadA = [&](const char* img) {
        if ((DBG & 4) && nk > 0) return;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) fa[b][kk] = oa.frag(img, b, kk, half);
    };
    auto loadB = [&](const char* img, Vec8<bf16> (&fb)[4]) {
        if ((DBG & 4) && nk > 0) return;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) fb[kk] = ob.frag(img, 0, kk, half);
    };
    auto quad = [&](int X, int Y, const Vec8<bf16> (&fb)[4]) {
        if (DBG & 1) return;
        if (!(DBG & 8)) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int b = 0; b < 2; ++b) Mma<bf16>::run(acc[2 * X + b][Y], fa[b][kk], fb[kk]);
        if (!(DBG & 8)) __builtin_amdgcn_s_setprio(0);
    };

    // Issue order = consumption order (per K-tile A(r0) B(c0) B(c1) A(r1)), one part per phase, each part re-staged TWO phases
    // after its last fragment read (those reads are only known complete after the barrier that closes their LOAD section) and five
    // to six phases before its first: "all but the four youngest parts landed" (vmcnt(8)) is what every phase needs.
    // prologue: the first K-tile whole, two parts of the second
    issue(0, 0, 0); issue(1, 0, 0); issue(2, 0, 0); issue(3, 0, 0);
    issue(0, 1, 1); issue(1, 1, 1);
    wait_vm<8>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (wr == 1) { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }      // the second wave of every SIMD: one section behind
    const char* const E = smem;
    const char* const O = smem + P8_BUF;
    for (int t = 0; t < nk; t += 2) {
        // ---- K-tile t (buffer E)
        loadA(E); loadB(E + P8_PART, fb0);
        issue(2, t + 1, 1);                                  // B(c1) of the odd tile of this pair
        load_end();
        quad(0, 0, fb0);
        sync();
        loadB(E + 2 * P8_PART, fb1);
        issue(3, t + 1, 1);                                  // A(r1) of the odd tile
        load_end();
        quad(0, 1, fb1);
        sync();
        loadA(E + 3 * P8_PART);
        issue(0, t + 2, 0);
        load_end();
        quad(1, 1, fb1);
        sync();
        issue(1, t + 2, 0);
        load_end();
        quad(1, 0, fb0);
        sync();
        // ---- K-tile t + 1 (buffer O); past the end its parts are zeros: the MFMAs add nothing
        loadA(O); loadB(O + P8_PART, fb0);
        issue(2, t + 2, 0);
        load_end();
        quad(0, 0, fb0);
        sync();
        loadB(O + 2 * P8_PART, fb1);
        issue(3, t + 2, 0);
        load_end();
        quad(0, 1, fb1);
        sync();
        loadA(O + 3 * P8_PART);
        issue(0, t + 3, 1);
        load_end();
        quad(1, 1, fb1);
        sync();
        issue(1, t + 3, 1);
        load_end();
        quad(1, 0, fb0);
        sync();
    }
    if (wr == 0) { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }
    wait_vm<0>();
    epilogue<bf16, 2>(g, *reinterpret_cast<f32x16 (*)[2][2]>(&acc[0]), smem, bm + wr * 128, bn + wc * 64, lane, wave);
    epilogue<bf16, 2>(g, *reinterpret_cast<f32x16 (*)[2][2]>(&acc[2]), smem, bm + wr * 128 + 64, bn + wc * 64, lane, wave);
}

template <bool TA, bool TB, int DBG = 0>
__global__ __launch_bounds__(512) void gemm_p8_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    p8_body<TA, TB, DBG>(g, smem, xcd_contiguous(blockIdx.x, gridDim.x));
}

template <bool TA, bool TB>
__global__ __launch_bounds__(512) void gemm_p8_multi_kernel(GemmMulti gm) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    int wg;
    const int p = multi_locate(gm, wg);
    if (p < 0) return;
    p8_body<TA, TB, 0>(gm.p[p], smem, wg);
}
// the same kernel under its own name when the epilogue applies the optimiser's update (audiossl_gemm_multi_sgd): a launch that moves
// 16 + 2 bytes per result element on top of the GEMM shows up as what it is in a profile
template <bool TA, bool TB>
__global__ __launch_bounds__(512) void gemm_p8_multi_sgd_kernel(GemmMulti gm) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    int wg;
    const int p = multi_locate(gm, wg);
    if (p < 0) return;
    p8_body<TA, TB, 0>(gm.p[p], smem, wg);
}

// ---------------------------------------------------------------------------------------------------------------------
// 128 x 128 output tile, 8 waves (4 x 2, wave tile 32 x 64): the same loop for the M = 512 problems (the heads' dzn / last data
// gradient launches: 96 tiles of 256 x 128, 192 of 128 x 128) and single problems with a narrow output.  A K-tile is TWO 16 KB parts
// (A: every wave's 32 rows, B: every wave's 64 columns) and ONE phase (8 MFMA 32x32x16 per wave); K-tile t + 3 is staged in
// phase t into a ring of five buffers (160 KB: the buffer it replaces was last read in phase t - 2, two phases back as the WAR rule
// asks), and the wait at the end of phase t's LOAD section retires K-tile t + 1 (issued two phases earlier): all but the two
// youngest K-tiles = vmcnt(8).  More LDS read bytes per MFMA than the 256-row kernels (12 fragment reads per 8 MFMAs).
constexpr int P5_PART = 16384, P5_BUF = 2 * P5_PART, P5_NBUF = 5, P5_AHEAD = 3;

template <bool TA, bool TB, int SCHED>
__device__ __forceinline__ void p5_body(const GemmArgs& g, char* smem, int wg) {
    const int tiles_n = (g.N + 127) / 128;
    const int bm = (wg / tiles_n) * 128, bn = (wg % tiles_n) * 128;
    const int ksteps = g.K / GBK;
    const int per = (ksteps + g.ksplit - 1) / g.ksplit;
    const int ks0 = blockIdx.z * per, ks1 = min(ksteps, ks0 + per);
    if (ks0 >= ks1) return;
    const int nk = ks1 - ks0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;

    PartOp<TA, 32, 32> oa; PartOp<TB, 64, 64> ob;
    oa.init(g.A, g.a_bytes, g.lda, bm, ks0 * GBK, wave, lane, wr);
    ob.init(g.B, g.b_bytes, g.ldb, bn, ks0 * GBK, wave, lane, wc);
    char* const wdst = smem + wave * 2048;

    f32x16 acc[1][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][j][r] = 0.f;

    auto issue = [&](int t, int boff) {
        const bool live = t < nk;
        oa.issue(0, t, wdst + boff, live);
        ob.issue(0, t, wdst + boff + P5_PART, live);
    };
    Vec8<bf16> fa[4], fb[2][4];
    issue(0, 0); issue(1, P5_BUF); issue(2, 2 * P5_BUF);
    wait_vm<8>();                                            // K-tile 0 has landed
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (wave >= 4) { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }
    int cb = 0, ib = P5_AHEAD * P5_BUF;
    for (int t = 0; t < nk; ++t) {
        const char* const img = smem + cb;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) fa[kk] = oa.frag(img, 0, kk, half);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) fb[j][kk] = ob.frag(img + P5_PART, j, kk, half);
        if (SCHED == 0) { issue(t + P5_AHEAD, ib); wait_vm<8>(); }
        else wait_vm<4>();                                   // K-tile t + 3 is issued inside the MFMA section below
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
            for (int j = 0; j < 2; ++j) Mma<bf16>::run(acc[0][j], fa[kk], fb[j][kk]);
            if (SCHED == 1 && kk == 0) oa.issue(0, t + P5_AHEAD, wdst + ib, t + P5_AHEAD < nk);
            if (SCHED == 1 && kk == 2) ob.issue(0, t + P5_AHEAD, wdst + ib + P5_PART, t + P5_AHEAD < nk);
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        cb = cb + P5_BUF == P5_NBUF * P5_BUF ? 0 : cb + P5_BUF;
        ib = ib + P5_BUF == P5_NBUF * P5_BUF ? 0 : ib + P5_BUF;
    }
    if (wave < 4) { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }
    wait_vm<0>();
    epilogue<bf16, 1>(g, acc, smem, bm + wr * 32, bn + wc * 64, lane, wave);
}

// KIND 5 = the 128 x 128 tiles of p5_body (DMA issued inside the MFMA section: 25.1 -> 22.4 us on the M = 512 launches).  The
// 256 x 128 tiles that used to be KIND 6 run in the software-pipelined form below (SpBody, shape 6).
template <bool TA, bool TB, int KIND>
__device__ __forceinline__ void pk_body(const GemmArgs& g, char* smem, int wg) {
    static_assert(KIND == 5, "the sectioned loop remains for the 128 x 128 tiles only");
    p5_body<TA, TB, 1>(g, smem, wg);
}

template <bool TA, bool TB, int KIND>
__global__ __launch_bounds__(512) void gemm_pk_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    pk_body<TA, TB, KIND>(g, smem, xcd_contiguous(blockIdx.x, gridDim.x));
}
template <bool TA, bool TB, int KIND>
__global__ __launch_bounds__(512) void gemm_pk_multi_kernel(GemmMulti gm) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    int wg;
    const int p = multi_locate(gm, wg);
    if (p < 0) return;
    pk_body<TA, TB, KIND>(gm.p[p], smem, wg);
}

// ---------------------------------------------------------------------------------------------------------------------
// The SOFTWARE-PIPELINED family: the hand-scheduled tiles above without LOAD / MFMA sections and without the wave-group stagger.
// A step = one 16-deep slice of the contraction: the wave's 2 MI MFMAs (MI x 2 blocks of 32 x 32) on one register set of MI + 2
// fragments, while the fragments of the NEXT step are read into the other set - two reads in each gap between MFMAs, where the LDS
// array serves them at no cost to the MFMA pipe - and the DMA instructions that stage a later slice follow in the remaining gaps.
// A stage = BK / 16 steps = one [rows][BK] slice of both operands, kept as 128-row sub-images in a ring of NB stages.  ONE
// s_barrier per stage, at the top of its last step, behind the wait that retired that step's own fragments (the wave's last reads
// of the stage):
//   * after it every wave is done reading stage h -> its ring slot takes stage h + NB (WAR), issued in this step and the following
//     BK / 16 - 1 steps;
//   * before it every wave waited for all of its DMA but the NB - 2 youngest stages -> stage h + 1, which the reads issued from
//     here on address, has landed in every wave's slice of the sub-images (RAW).
// Measured on the three-head launches (M = 1,024, K = 2,048, 256 x 128 tiles): 35.1 -> 31.8 us against the sectioned loop.
// Sub-image layouts: K-contiguous operand: [128 rows][BK] with the 16-byte chunk c of row r stored at c ^ swz(r), swz = (r >> 2) & 3
// for BK = 32 (64-byte rows) and (r >> 1) & 7 for BK = 64: the 16 lanes the LDS serves together (ds_read_b128) hit all 64 banks
// once; row-contiguous operand: [BK k][128 rows], 64-byte group ^= k & 3, read with ds_read_b64_tr_b16 (as PartOp above).
template <bool TRANS, int BK>
struct SliceOp {
    static constexpr int NI = BK / 32;                       // DMA instructions per wave and sub-image (1 KB each)
    static constexpr int SUBB = 128 * BK * 2;                // bytes of a sub-image
    static constexpr int CH = BK / 8;                        // 16-byte chunks per row (K-contiguous form)
    __amdgpu_buffer_rsrc_t rsrc;
    int voff[NI];
    int kstride, sub_delta, base_off;                        // bytes; wave-uniform
    __device__ __forceinline__ static int swz(int r) { return BK == 32 ? (r >> 2) & 3 : (r >> 1) & 7; }
    __device__ __forceinline__ void init(const void* base_, unsigned bytes, long ld, int r0, int k0, int wave, int lane) {
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base_), 0, bytes, 0x00020000);
        if (!TRANS) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int p = wave * 16 + i * (64 / CH) + lane / CH;          // row of the sub-image this lane fills
                const int sc = (lane % CH) ^ swz(p);                          // the logical chunk stored at position lane % CH
                voff[i] = (int)(((long)p * ld + sc * 8) * 2);
            }
            kstride = BK * 2;
            sub_delta = (int)(128 * ld * 2);
            base_off = (int)(((long)r0 * ld + k0) * 2);
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int kl = wave * (BK / 8) + i * 4 + (lane >> 4), pc = lane & 15;
                const int roff = ((((pc >> 2) ^ (kl & 3)) << 2) + (pc & 3)) * 8;
                voff[i] = (int)(((long)kl * ld + roff) * 2);
            }
            kstride = (int)(BK * ld * 2);
            sub_delta = 256;
            base_off = (int)(((long)k0 * ld + r0) * 2);
        }
    }
    // DMA instruction i of sub-image `sub` of stage st; dst = this wave's slice (wave * 1024 * NI) of that sub-image
    __device__ __forceinline__ void issue(int sub, int i, int st, char* dst, bool live) const {
        typedef __attribute__((address_space(3))) void* lptr_t;
        const int so = live ? base_off + st * kstride + sub * sub_delta : 0x7FFFFF00;          // past the buffer: zeros, no traffic
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)(dst + i * 1024), 16, voff[i], so, 0, 0);
    }
    // byte offset (inside a stage's run of this operand's sub-images) of the step-0 fragment of the 32-row block at tile row row0
    __device__ __forceinline__ static int frag_off(int row0, int lane) {
        if (!TRANS) {
            const int local = (row0 & 127) + (lane & 31), half = lane >> 5;
            return (row0 >> 7) * SUBB + local * (BK * 2) + ((half ^ swz(local)) << 4);
        }
        const int gb = row0 >> 5, q = (lane & 15) >> 2, pp = lane & 3, h4 = (lane >> 4) & 1, half = lane >> 5;
        return (gb >> 2) * SUBB + (8 * half + q) * 256 + (((gb & 3) ^ q) << 6) + 32 * h4 + 8 * pp;
    }
    __device__ __forceinline__ static Vec8<bf16> frag(const char* stage, int off, int kk) {
        if (!TRANS) return Vec8<bf16>::load(reinterpret_cast<const bf16*>(stage + (off ^ (kk << 5))));
        typedef __attribute__((address_space(3))) const char* lds_t;                            // inline asm: see PartOp::frag
        const unsigned a = (unsigned)(size_t)(lds_t)(stage + off + kk * 4096);
        bf16x4 lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a) : "memory");
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(hi) : "v"(a) : "memory");
        Vec8<bf16> f;
        f.v = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return f;
    }
};

// SHAPE 8: 256 x 256 (waves 2 x 4, wave tile 128 x 64), BK 32, ring of 5 x 32 KB; SHAPE 6: 256 x 128 (4 x 2, 64 x 64), BK 64, ring of
// 3 x 48 KB; SHAPE 5: 128 x 128 (4 x 2, 32 x 64), BK 64, ring of 5 x 32 KB
template <int SHAPE> struct SpCfg;
template <> struct SpCfg<8> { static constexpr int WR = 2, WC = 4, MI = 4, BK = 32, NB = 5; };
template <> struct SpCfg<6> { static constexpr int WR = 4, WC = 2, MI = 2, BK = 64, NB = 3; };
template <> struct SpCfg<5> { static constexpr int WR = 4, WC = 2, MI = 1, BK = 64, NB = 5; };
template <int SHAPE> struct SpDim {
    using C = SpCfg<SHAPE>;
    static constexpr int RA = C::WR * C::MI * 32, RB = C::WC * 64;
    static constexpr int SA = RA / 128, SBN = RB / 128, NSUB = SA + SBN;
    static constexpr int SUBB = 128 * C::BK * 2, STG = NSUB * SUBB;
    static constexpr int PER = NSUB * (C::BK / 32);          // DMA instructions per wave and stage
    static constexpr int KS = C::BK / 16;                    // steps per stage
    static constexpr int DPS = (PER + KS - 1) / KS;          // DMA instructions per step
    static constexpr size_t LDS = (size_t)C::NB * STG > EPI_LDS * 2 ? (size_t)C::NB * STG : EPI_LDS * 2;
};

// (a class with a static member: as a function template the host pass of hipcc rejected every instantiation after the first)
template <bool TA, bool TB, int SHAPE>
struct SpBody {
__device__ __forceinline__ static void run(const GemmArgs& g, char* smem, int wg) {
    using C = SpCfg<SHAPE>; using D = SpDim<SHAPE>;
    constexpr int MI = C::MI, BK = C::BK, NB = C::NB, KS = D::KS, NI = BK / 32, NM = 2 * MI, NR = MI + 2;
    static_assert(C::WR * C::WC == 8 && D::RA % 128 == 0 && D::RB % 128 == 0 && KS % 2 == 0, "shape");
    constexpr int first_dma_gap = NM - 1 > (NR + 1) / 2 ? (NR + 1) / 2 : NM - 2;     // the gap after the last pair of fragment reads
    const int tiles_n = (g.N + D::RB - 1) / D::RB;
    const int bm = (wg / tiles_n) * D::RA, bn = (wg % tiles_n) * D::RB;
    const int k64 = g.K / GBK;
    const int per = (k64 + g.ksplit - 1) / g.ksplit;
    const int ks0 = blockIdx.z * per, ks1 = min(k64, ks0 + per);
    if (ks0 >= ks1) return;
    const int nk = (ks1 - ks0) * (GBK / BK);                 // stages
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave / C::WC, wc = wave % C::WC;

    SliceOp<TA, BK> oa; SliceOp<TB, BK> ob;
    oa.init(g.A, g.a_bytes, g.lda, bm, ks0 * GBK, wave, lane);
    ob.init(g.B, g.b_bytes, g.ldb, bn, ks0 * GBK, wave, lane);
    char* const wdst = smem + wave * (1024 * NI);            // this wave's slice of every sub-image

    int foff[NR];                                            // step-0 fragment offsets inside a stage: MI row blocks, 2 column blocks
#pragma unroll
    for (int i = 0; i < MI; ++i) foff[i] = oa.frag_off(wr * MI * 32 + i * 32, lane);
#pragma unroll
    for (int j = 0; j < 2; ++j) foff[MI + j] = D::SA * D::SUBB + ob.frag_off(wc * 64 + j * 32, lane);

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // DMA instruction n (0 .. PER - 1) of stage st into the ring slot at byte offset sbase
    auto dma = [&](int n, int st, int sbase) {
        const int sub = n / NI, i = n % NI;
        const bool live = st < nk;
        if (sub < D::SA) oa.issue(sub, i, st, wdst + sbase + sub * D::SUBB, live);
        else ob.issue(sub - D::SA, i, st, wdst + sbase + sub * D::SUBB, live);
    };
    Vec8<bf16> fr[2][NR];                                    // [register set][fragment]
    auto read = [&](int set, int n, const char* stage, int kk) {
        if (n < MI) fr[set][n] = oa.frag(stage, foff[n], kk);
        else fr[set][n] = ob.frag(stage, foff[n], kk);
    };

    // prologue: stages 0 .. NB - 2 whole and the first step's share of stage NB - 1
#pragma unroll
    for (int h = 0; h < NB - 1; ++h)
#pragma unroll
        for (int n = 0; n < D::PER; ++n) dma(n, h, h * D::STG);
#pragma unroll
    for (int n = 0; n < D::DPS && n < D::PER; ++n) dma(n, NB - 1, (NB - 1) * D::STG);
    wait_vm<(NB - 2) * D::PER + (D::DPS < D::PER ? D::DPS : D::PER)>();       // stage 0
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int n = 0; n < NR; ++n) read(0, n, smem, 0);

    int cb = 0, pb = (NB - 1) * D::STG;                      // ring slots of stage h and of stage h - 1
    for (int h = 0; h < nk; ++h) {
        const int nb = cb + D::STG == NB * D::STG ? 0 : cb + D::STG;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            const bool last = kk == KS - 1;
            const char* const src = smem + (last ? nb : cb);
            const int kn = last ? 0 : kk + 1;
            // DMA share of this step: the slot freed by the most recent barrier takes stage (that stage) + NB
            const int c = last ? 0 : kk + 1, dst_stage = last ? h + NB : h - 1 + NB, dst_slot = last ? cb : pb;
            // the transposing reads are inline asm the compiler does not track; the K-contiguous ones get its own counted waits
            if (TA || TB || last) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (last) {
                wait_vm<(NB - 2) * D::PER>();
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                Mma<bf16>::run(acc[m >> 1][m & 1], fr[cur][m >> 1], fr[cur][MI + (m & 1)]);
                __builtin_amdgcn_sched_barrier(0);
                if (m < NM - 1) {
                    // gap m: two fragment reads, then (behind the reads) the step's DMA instructions, all of them by the last gap
#pragma unroll
                    for (int n = 2 * m; n < 2 * m + 2 && n < NR; ++n) read(nxt, n, src, kn);
#pragma unroll
                    for (int d = 0; d < D::DPS; ++d) {
                        constexpr int gaps = NM - 1 - first_dma_gap, per_gap = (D::DPS + gaps - 1) / gaps;
                        const int gap = first_dma_gap + d / per_gap;
                        if (gap == m && c * D::DPS + d < D::PER) dma(c * D::DPS + d, dst_stage, dst_slot);
                    }
                    if (NM == 2) {                           // one gap only: the third fragment too
#pragma unroll
                        for (int n = 2; n < NR; ++n) read(nxt, n, src, kn);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        pb = cb; cb = nb;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (MI == 4) {
        epilogue<bf16, 2>(g, *reinterpret_cast<f32x16 (*)[2][2]>(&acc[0]), smem, bm + wr * 128, bn + wc * 64, lane, wave);
        epilogue<bf16, 2>(g, *reinterpret_cast<f32x16 (*)[2][2]>(&acc[2]), smem, bm + wr * 128 + 64, bn + wc * 64, lane, wave);
    } else epilogue<bf16, MI>(g, acc, smem, bm + wr * MI * 32, bn + wc * 64, lane, wave);
}
};

template <bool TA, bool TB, int SHAPE>
__global__ __launch_bounds__(512) void gemm_sp_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    SpBody<TA, TB, SHAPE>::run(g, smem, xcd_contiguous(blockIdx.x, gridDim.x));
}
template <bool TA, bool TB, int SHAPE>
__global__ __launch_bounds__(512) void gemm_sp_multi_kernel(GemmMulti gm) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    int wg;
    const int p = multi_locate(gm, wg);
    if (p < 0) return;
    SpBody<TA, TB, SHAPE>::run(gm.p[p], smem, wg);
}
template <bool TA, bool TB, int SHAPE>
__global__ __launch_bounds__(512) void gemm_sp_multi_sgd_kernel(GemmMulti gm) {      // see gemm_p8_multi_sgd_kernel
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    int wg;
    const int p = multi_locate(gm, wg);
    if (p < 0) return;
    SpBody<TA, TB, SHAPE>::run(gm.p[p], smem, wg);
}
// Shape 6 always runs in this form; the 256 x 256 and 128 x 128 tiles have it as the non-default variants sp8 / sp5.
// Measured (tools/heads_gemm_bench.py, tools/gemm_shapes.py; us, sectioned -> pipelined):
//   256 x 128: three-head M = 1,024 launches NT 35.1 -> 31.3 (822 TF/s), first layer 33.4 -> 30.0, NN 36.5 -> 35.3; single TN
//              2048 x 2048 x 1024 26.2 -> 23.6, x 512 19.4 -> 17.7                                              -> default
//   256 x 256: 6144 x 2048 x 2048 NT 63.0 -> 65.2, NN 64.2 -> 64.4, three-head TN 39.1 -> 38.4 (BK 32, ring of five; BK 64 with two
//              buffers and the whole stage issued in the last step: 64.7 / 65.1 / 41.2): the same within the box-to-box spread - the
//              sectioned kernel stays, these tiles are MFMA-paced either way
//   128 x 128: M = 512 launches 21.9 -> 22.6, 23.3 -> 24.2, 20.4 -> 21.4: two MFMAs per step leave one gap for three reads and a DMA
//              instruction - the sectioned kernel stays
//   BK 32 stages for the 256 x 128 / 128 x 128 tiles (rings of 6 / 10): 38.3 vs 31.5 and 25.4 vs 22.5 - twice the barriers

// BK = 32 with a register budget for THREE workgroups per CU (41 KB of LDS each; the epilogue runs on half-height tiles so
// that it fits the same 41 KB).
template <bool TA, bool TB>
__global__ __launch_bounds__(256, 3) void gemm_bk32_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    gemm_body<bf16, TA, TB, 32, 2, 4, true>(g, smem, g.xcd_remap ? (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) : (int)blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------------
// The kernel set: these instantiations and no others are compiled into the library (a -DAUDIOSSL_ABLATE build adds the ablation variants
// of gemm_p8_kernel, see launch_variant).  Keep the order.  It is the order in which the kernels have been emitted since they were
// written, and the machine code the compiler produces for a kernel is not independent of what the module holds before it (emitting the
// single-problem kernels first changed the register allocation of two multi-problem ones): with the order pinned, a change to the host
// side below leaves every kernel byte for byte as it was.
#define FOR_LAYOUTS(X, ...) X(false, false, __VA_ARGS__) X(false, true, __VA_ARGS__) X(true, true, __VA_ARGS__) X(true, false, __VA_ARGS__)
#define KERNEL(TA, TB, NAME, ARGS, ...) template __global__ void NAME<TA, TB, ##__VA_ARGS__>(ARGS);
#define KERNEL_AND_SGD(TA, TB, STEM, ...) KERNEL(TA, TB, STEM##_kernel, GemmMulti, ##__VA_ARGS__) KERNEL(TA, TB, STEM##_sgd_kernel, GemmMulti, ##__VA_ARGS__)
#define REG_KERNEL(TA, TB, NAME, ARGS, T, BK, MI) template __global__ void NAME<T, TA, TB, BK, MI, 4>(ARGS);
FOR_LAYOUTS(KERNEL_AND_SGD, gemm_p8_multi)
FOR_LAYOUTS(KERNEL, gemm_p8_kernel, GemmArgs, 0)
FOR_LAYOUTS(KERNEL, gemm_bk32_kernel, GemmArgs)
FOR_LAYOUTS(KERNEL_AND_SGD, gemm_sp_multi, 6)
FOR_LAYOUTS(KERNEL_AND_SGD, gemm_sp_multi, 5)
FOR_LAYOUTS(KERNEL, gemm_pk_multi_kernel, GemmMulti, 5)
FOR_LAYOUTS(KERNEL_AND_SGD, gemm_sp_multi, 8)
FOR_LAYOUTS(REG_KERNEL, gemm_multi_kernel, GemmMulti, bf16, 64, 1)
FOR_LAYOUTS(REG_KERNEL, gemm_multi_kernel, GemmMulti, bf16, 128, 2)
FOR_LAYOUTS(REG_KERNEL, gemm_multi_kernel, GemmMulti, bf16, 64, 2)
FOR_LAYOUTS(KERNEL, gemm_sp_kernel, GemmArgs, 6)
FOR_LAYOUTS(KERNEL, gemm_sp_kernel, GemmArgs, 8)
FOR_LAYOUTS(KERNEL, gemm_sp_kernel, GemmArgs, 5)
FOR_LAYOUTS(KERNEL, gemm_pk_kernel, GemmArgs, 5)
FOR_LAYOUTS(KERNEL, gemm_ring_kernel, GemmArgs, 1, 4)
FOR_LAYOUTS(KERNEL, gemm_ring_kernel, GemmArgs, 2, 4)
FOR_LAYOUTS(REG_KERNEL, gemm_kernel, GemmArgs, bf16, 64, 1)
FOR_LAYOUTS(REG_KERNEL, gemm_kernel, GemmArgs, bf16, 128, 2)
FOR_LAYOUTS(REG_KERNEL, gemm_kernel, GemmArgs, bf16, 64, 2)
FOR_LAYOUTS(REG_KERNEL, gemm_kernel, GemmArgs, float, 32, 2)
#undef FOR_LAYOUTS
#undef KERNEL
#undef KERNEL_AND_SGD
#undef REG_KERNEL

// ---------------------------------------------------------------------------------------------------------------------
// Host side.  A VARIANT is one kernel family at one tile shape.  Every entry point runs
//   validate the operands -> describe the problem -> choose a variant (pure functions) -> one switch that launches it.
enum Variant { V_NONE = -1, V_REG64, V_REG128_K64, V_REG128_K128, V_RING64, V_RING128, V_BK32, V_P8, V_PK5, V_SP5, V_SP6, V_SP8, V_COUNT };
// the names DESIGN.md section 4 uses; AUDIOSSL_GEMM_FORCE / AUDIOSSL_GEMM_OFF take them
const char* const VARIANT_NAME[V_COUNT] = {"reg64x128", "reg128_k64", "reg128_k128", "ring64", "ring128", "bk32", "p8", "pk5", "sp5", "sp6", "sp8"};

// What the choice looks at: one problem (multi = false), or `count` problems with common M, transposes and epilogue in one launch.
struct Problem {
    bool multi;
    int count, ta, tb, M, ksplit, atomic, lse_mode;
    const int* Nv; const int* K;                             // one entry per problem
    int N, kmin;                                             // widest problem, shortest contraction
};
Problem describe(bool multi, int count, int ta, int tb, int M, const int* Nv, const int* K, int ksplit, int atomic, int lse_mode) {
    Problem p{multi, count, ta, tb, M, ksplit, atomic, lse_mode, Nv, K, 0, 1 << 30};
    for (int i = 0; i < count; ++i) { p.N = max(p.N, Nv[i]); p.kmin = min(p.kmin, K[i]); }
    return p;
}
// tiles of 128 x 128 / 256 x 128 / 256 x 256 over all problems and K splits; blocks: the register-staged grid of 128 x 128 tiles, which is
// sized for the widest problem
struct Tiles { long t5, t6, t8, blocks; };
Tiles count_tiles(const Problem& p) {
    Tiles t{0, 0, 0, (long)ceil_div(p.M, BM) * ceil_div(p.N, BN) * p.ksplit * p.count};
    for (int i = 0; i < p.count; ++i) {
        t.t5 += (long)ceil_div(p.M, 128) * ceil_div(p.Nv[i], 128);
        t.t6 += (long)ceil_div(p.M, 256) * ceil_div(p.Nv[i], 128);
        t.t8 += (long)ceil_div(p.M, 256) * ceil_div(p.Nv[i], 256);
    }
    t.t5 *= p.ksplit; t.t6 *= p.ksplit; t.t8 *= p.ksplit;
    return t;
}

// Where a variant may run at all, bf16 operands (the choice functions add where it is measured to win; AUDIOSSL_GEMM_FORCE needs only this).
// tests/gemm_cases.py restates this function (legal()) to generate only cases the forced variant takes: change both together, or the
// kernel-name assertions of tests/test_gpu_gemm_matrix.py turn red.
bool legal(Variant v, const Problem& p, const Tiles& t) {
    // the hand-scheduled kernels: K % 64, whole 16-byte rows, at least one full tile of the smallest shape
    bool hs_ok = p.M >= 128 && p.N >= 128 && (!p.ta || p.M % 8 == 0);
    for (int i = 0; i < p.count; ++i) hs_ok = hs_ok && p.K[i] % GBK == 0 && (!p.tb || p.Nv[i] % 8 == 0);
    switch (v) {
        case V_REG64:       return t.blocks <= 128 && p.M > 64;
        case V_REG128_K64:  return true;
        case V_REG128_K128: return t.blocks <= 256 && p.kmin >= 512;
        case V_RING64:
        case V_RING128:     return !p.multi && p.kmin % GBK == 0 && p.M >= 8 && p.N >= 8;      // no multi-problem kernel
        case V_BK32:        return !p.multi && t.blocks >= 512;                                // no multi-problem kernel
        case V_P8:
        case V_SP8:         return hs_ok && p.M >= 256 && p.N >= 256;
        case V_SP6:         return hs_ok && !p.lse_mode && p.M >= 256;
        case V_PK5:
        case V_SP5:         return hs_ok && !p.lse_mode;
        default:            return false;
    }
}

struct Choice { Variant v; int ksplit; };                    // ksplit: the caller's, or raised (256 x 256 tiles with an accumulating output)

// the 256 x 256 kernels on accumulating outputs: split K until the chip is full
int p8_ksplit(const Problem& p, const Tiles& t) {
    const long t256 = t.t8 / p.ksplit;
    int ks = p.ksplit;
    if (!p.multi && p.atomic == 1 && t256 * ks < 192)
        while (t256 * ks * 2 <= 256 && p.kmin / (ks * 2) >= 1024) ks *= 2;
    return ks;
}

// kernel choice for one bf16 problem (measured rules, see the comments inside); off: bit v set = skip variant v
Choice choose_single(const Problem& p, const Tiles& t, unsigned off) {
    const int M = p.M, K = p.kmin, ksplit = p.ksplit;
    const auto on = [&](Variant v) { return !(off >> v & 1) && legal(v, p, t); };
    // transposed-A problems whose split-K launch fills the chip with 256 x 128 tiles: the software-pipelined kernel with the caller's
    // split beats the 256 x 256 kernel with the split raised to fill the chip (the encoder's fc.3 weight gradient, 2048 x 2048 x 6144
    // split in two: 97.4 -> 77.6 us, 664 TFLOP/s)
    if (on(V_SP6) && p.ta && p.atomic == 1 && t.t6 >= 192 && t.t6 <= 288 && K / ksplit >= 2048) return {V_SP6, ksplit};
    if (on(V_P8)) {
        // measured (tools/gemm_shapes.py, gemm_one.py): it wins once the 256 x 256 tiles occupy at least half of the CUs and every
        // workgroup walks >= 16 K-tiles (6144 x 2048 x 2048 NT 83.9 -> 63.0 us with the bias / ReLU / dropout epilogue, NN 71.0 ->
        // 60.4; 4096^3 214 -> 127 us, 8192^3 1.30 PFLOP/s); with few K-tiles its one-workgroup-per-CU epilogue is exposed
        // (6144 x 2048 x 512: 30.8 vs 27.2 us) and on small grids the 128-row kernels spread over more CUs.
        const long t256 = t.t8 / ksplit;
        const int ks = p8_ksplit(p, t);
        // ... and with 12 K-tiles once the grid is several rounds deep (the transformer blocks' K = 768 layers at 27,648 rows:
        // 27648 x 2304 x 768 NT 188.6 -> 140.5 us, x 3072 235.3 -> 181.2, x 768 63.9 -> 53.2 against the K-step-32 kernel)
        const bool deep = t256 * ks >= 512 && K / ks >= 768;
        if (t256 * ks >= 128 && (K / ks >= 1024 || deep)) return {V_P8, ks};
    }
    // the 256 x 128 kernel (written for the multi-problem launches of the projector heads, see choose_multi):
    // single problems whose 256 x 128 tiles fill the chip once while the 256 x 256 tiles would leave half of it idle
    if (on(V_SP6) && t.t6 >= 128 && t.t6 <= 288 && t.t8 < 128 && K / ksplit >= 512) return {V_SP6, ksplit};
    // measured (tools/gemm_shapes.py): NN 6144 x 512 x 2048 34.1 -> 25.8 us, TN 2048 x 512 x 6144 / 3 41.9 -> 32.2 us; with short K
    // loops (2048 x 2048 x 512 TN: 19.3 vs 17.9 us) and for K-contiguous operands on <= 128 tiles (the ring kernel: 20.2 vs 21.7 us)
    // the older kernels stay
    if (on(V_PK5) && t.t5 >= 96 && t.t5 <= 288 && t.t6 < 128 && K / ksplit >= 1024 && (p.ta || p.tb || t.t5 > 128)) return {V_PK5, ksplit};
    // grids of >= 2 workgroups per CU with a K-contiguous A operand: K-step 32 and THREE co-resident workgroups per CU (41 KB
    // of LDS each, 126 VGPRs) - 12 waves per CU hide the staged-load and barrier waits better than two workgroups at K-step
    // 64 (6144x2048x2048 NT 80.9 -> 71.5 us, NN 90.2 -> 76.8 us; with a transposed A operand it measured slower)
    if (on(V_BK32) && !p.ta) return {V_BK32, ksplit};
    // measured (tools/gemm_shapes.py): the ring wins for K-contiguous operands (NT) on grids of at most two waves of
    // workgroups - 64-row tiles up to 128 full tiles, 128-row tiles up to 512; with a transposed operand or on larger grids
    // two co-resident workgroups of the register-staged kernel overlap each other better
    if (on(V_RING64) && !p.ta && !p.tb && t.blocks <= 128 && M > 64) return {V_RING64, ksplit};
    if (on(V_RING128) && !p.ta && !p.tb && t.blocks > 128 && t.blocks <= 512) return {V_RING128, ksplit};
    // these shapes are latency-bound per workgroup (~0.5 us per 64-deep k-step whatever the tile): when 128 x 128 tiles
    // would occupy at most half of the 256 CUs, halve the tile in M and run twice as many workgroups
    if (on(V_REG64)) return {V_REG64, ksplit};
    return {on(V_REG128_K128) ? V_REG128_K128 : V_REG128_K64, ksplit};
}

// kernel choice for a multi-problem launch
Choice choose_multi(const Problem& p, const Tiles& t, unsigned off) {
    const int ksplit = p.ksplit;
    const auto on = [&](Variant v) { return !(off >> v & 1) && legal(v, p, t); };
    // the 256 x 128 kernel: problems whose 256 x 256 tiles would leave more than half of the CUs idle while the 256 x 128 tiles
    // fit the chip in one round (the M = 1,024 layers and data gradients of the three heads: 192 workgroups); the 128 x 128 kernel
    // where even those are too few (M = 512: 96 -> 192 workgroups)
    if (on(V_SP6) && t.t6 >= 128 && t.t6 <= 288 && t.t8 < 128 && p.kmin >= 512) return {V_SP6, ksplit};
    if (on(V_PK5) && t.t5 >= 96 && t.t5 <= 288 && t.t6 < 128 && p.kmin >= 512) return {V_PK5, ksplit};
    // multi-problem launches: measured wins for the transposed-A weight gradients of the three heads (2048 x 2048 x 1024:
    // 50.9 -> 43.9 us, x 512: 31.3 -> 29.0 us)
    if (on(V_P8) && p.ta && t.t8 >= 128 && p.kmin >= 512) return {V_P8, ksplit};
    if (on(V_REG64)) return {V_REG64, ksplit};
    return {on(V_REG128_K128) ? V_REG128_K128 : V_REG128_K64, ksplit};
}

// The two diagnostic switches, read once per process (tests force variants in a child process):
//   AUDIOSSL_GEMM_FORCE=<variant>            every bf16 problem for which the variant is legal runs it; the rest take the default choice
//   AUDIOSSL_GEMM_OFF=<variant>[,<variant>]  the default choice skips these (reg128_k64 is the last resort and cannot be skipped)
// An unknown name makes every GEMM entry point return ASSL_EINVAL: a misspelt switch must not silently run the default.
struct Switches { Variant force; unsigned off; bool bad; };
const Switches& switches() {
    static const Switches sw = [] {
        Switches r{V_NONE, 0, false};
        for (int w = 0; w < 2; ++w) {
            const bool is_force = w == 0;
            const char* s = getenv(is_force ? "AUDIOSSL_GEMM_FORCE" : "AUDIOSSL_GEMM_OFF");
            while (s && *s) {
                const char* e = strchr(s, ',');
                const size_t n = e ? (size_t)(e - s) : strlen(s);
                Variant v = V_NONE;
                for (int i = 0; i < V_COUNT; ++i)
                    if (strlen(VARIANT_NAME[i]) == n && !strncmp(VARIANT_NAME[i], s, n)) v = (Variant)i;
                if (v == V_NONE || (is_force && (e || r.force != V_NONE))) r.bad = true;
                else if (is_force) r.force = v;
                else r.off |= 1u << v;
                s = e ? e + 1 : s + n;
            }
        }
        return r;
    }();
    return sw;
}

Choice choose(const Problem& p) {
    const Switches& sw = switches();
    const Tiles t = count_tiles(p);
    if (sw.force != V_NONE && legal(sw.force, p, t))
        return {sw.force, sw.force == V_P8 || sw.force == V_SP8 ? p8_ksplit(p, t) : p.ksplit};
    return p.multi ? choose_multi(p, t, sw.off) : choose_single(p, t, sw.off);
}

// One kernel instantiation: entry, the name rocprofv3 prints for it (demangled, except for instantiations on __bf16, which its
// demangler leaves mangled), output tile, workgroup size, dynamic LDS.  Built once, on first use, which is also when the LDS limit
// of the kernel is raised; immutable afterwards (g_assl_last_kernel only ever points at these names).
template <typename Args>
struct Kernel { void (*fn)(Args); char name[96]; int rows, cols, block; size_t lds; hipError_t attr; };
template <typename Args>
Kernel<Args> make_kernel(void (*fn)(Args), int rows, int cols, int block, size_t lds, const char* fmt, ...) {
    Kernel<Args> k{fn, {0}, rows, cols, block, lds, hipSuccess};
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(k.name, sizeof(k.name), fmt, ap);
    va_end(ap);
    k.attr = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return k;
}
#define TF(b) ((b) ? "true" : "false")
template <typename T> const char* type_code();
template <> const char* type_code<bf16>() { return "DF16b"; }
template <> const char* type_code<float>() { return "f"; }

// the one launcher
template <typename Args>
int launch_kernel(const Kernel<Args>& k, int grid, int ksplit, hipStream_t s, const Args& a) {
    if (k.attr != hipSuccess) return ASSL_ELAUNCH;
    g_assl_last_kernel = k.name;
    void* args[] = {const_cast<Args*>(&a)};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(k.fn), dim3(grid, 1, ksplit), dim3(k.block), args, k.lds, s);
    ASSL_LAUNCH_CHECK();
}
// one problem: a grid of the kernel's tiles.  remap: the kernels that take their XCD-contiguous tile order from g.xcd_remap
int launch_single(const Kernel<GemmArgs>& k, const GemmArgs& g, bool remap, hipStream_t s) {
    const int tiles = ceil_div(g.M, k.rows) * ceil_div(g.N, k.cols);
    GemmArgs ga = g;
    ga.xcd_remap = remap && tiles % 8 == 0 && tiles >= 64;
    return launch_kernel(k, tiles, g.ksplit, s, ga);
}
int launch_multi(const Kernel<GemmMulti>& k, const GemmMulti& gm_, int count, int ksplit, hipStream_t s) {
    GemmMulti gm = gm_;
    return launch_kernel(k, multi_grid(gm, count, k.rows, k.cols), ksplit, s, gm);
}

// (ta, tb) -> the <TA, TB> instantiation of a templated callable: f(std::bool_constant<TA>, std::bool_constant<TB>)
template <typename F>
int by_layout(int ta, int tb, F&& f) {
    if (!ta && !tb) return f(std::false_type{}, std::false_type{});
    if (!ta && tb) return f(std::false_type{}, std::true_type{});
    if (ta && tb) return f(std::true_type{}, std::true_type{});
    return f(std::true_type{}, std::false_type{});
}

// The kernel table: per family, what a launch needs beyond the kernel itself - tile shape, workgroup size, LDS bytes, name.
template <typename T, bool TA, bool TB, int BK, int MI>
const Kernel<GemmArgs>& reg_kernel() {
    static const auto k = make_kernel(&gemm_kernel<T, TA, TB, BK, MI, 4>, 64 * MI, BN, 256, gemm_lds<T, TA, TB, BK, MI, 4>(),
                                      "gemm_kernelI%sLb%dELb%dELi%dELi%dELi%dE", type_code<T>(), (int)TA, (int)TB, BK, MI, 4);
    return k;
}
template <bool TA, bool TB, int BK, int MI>
const Kernel<GemmMulti>& reg_multi_kernel() {
    static const auto k = make_kernel(&gemm_multi_kernel<bf16, TA, TB, BK, MI, 4>, 64 * MI, BN, 256, gemm_lds<bf16, TA, TB, BK, MI, 4>(),
                                      "gemm_multi_kernelI%sLb%dELb%dELi%dELi%dELi%dE", type_code<bf16>(), (int)TA, (int)TB, BK, MI, 4);
    return k;
}
template <bool TA, bool TB, int MI>
const Kernel<GemmArgs>& ring_kernel() {
    constexpr int NST = 4;                                   // ring depth (2, 3 and 6 were swept and dropped)
    constexpr size_t stage = RingOp<TA, 64 * MI>::BYTES + RingOp<TB, 128>::BYTES;
    static const auto k = make_kernel(&gemm_ring_kernel<TA, TB, MI, NST>, 64 * MI, BN, 256, max((size_t)NST * stage, EPI_LDS),
                                      "gemm_ring_kernel<%s, %s, %d, %d>", TF(TA), TF(TB), MI, NST);
    return k;
}
template <bool TA, bool TB>
const Kernel<GemmArgs>& bk32_kernel() {
    constexpr size_t stage = sizeof(bf16) * 2 * (Stage<bf16, TA, 32, 128, 256>::LDS_ELEMS + Stage<bf16, TB, 32, BN, 256>::LDS_ELEMS);
    static const auto k = make_kernel(&gemm_bk32_kernel<TA, TB>, 128, BN, 256, stage > EPI_LDS / 2 ? stage : EPI_LDS / 2,
                                      "gemm_bk32_kernel<%s, %s>", TF(TA), TF(TB));
    return k;
}
constexpr size_t P8_LDS = (size_t)2 * P8_BUF > EPI_LDS * 2 ? (size_t)2 * P8_BUF : EPI_LDS * 2;
template <bool TA, bool TB, int DBG>
const Kernel<GemmArgs>& p8_kernel() {
    static const auto k = make_kernel(&gemm_p8_kernel<TA, TB, DBG>, 256, 256, 512, P8_LDS, "gemm_p8_kernel<%s, %s, %d>", TF(TA), TF(TB), DBG);
    return k;
}
template <bool TA, bool TB>
const Kernel<GemmMulti>& p8_multi_kernel(bool sgd) {         // sgd: the same kernel under the name it carries when the epilogue applies the update
    static const auto k = make_kernel(&gemm_p8_multi_kernel<TA, TB>, 256, 256, 512, P8_LDS, "gemm_p8_multi_kernel<%s, %s>", TF(TA), TF(TB));
    static const auto ks = make_kernel(&gemm_p8_multi_sgd_kernel<TA, TB>, 256, 256, 512, P8_LDS, "gemm_p8_multi_sgd_kernel<%s, %s>", TF(TA), TF(TB));
    return sgd ? ks : k;
}
constexpr size_t PK5_LDS = (size_t)P5_NBUF * P5_BUF;
template <bool TA, bool TB>
const Kernel<GemmArgs>& pk5_kernel() {
    static const auto k = make_kernel(&gemm_pk_kernel<TA, TB, 5>, 128, 128, 512, PK5_LDS, "gemm_pk_kernel<%s, %s, %d>", TF(TA), TF(TB), 5);
    return k;
}
template <bool TA, bool TB>
const Kernel<GemmMulti>& pk5_multi_kernel() {
    static const auto k = make_kernel(&gemm_pk_multi_kernel<TA, TB, 5>, 128, 128, 512, PK5_LDS, "gemm_pk_multi_kernel<%s, %s, %d>", TF(TA), TF(TB), 5);
    return k;
}
template <bool TA, bool TB, int SHAPE>
const Kernel<GemmArgs>& sp_kernel() {
    using D = SpDim<SHAPE>;
    static const auto k = make_kernel(&gemm_sp_kernel<TA, TB, SHAPE>, D::RA, D::RB, 512, D::LDS, "gemm_sp_kernel<%s, %s, %d>", TF(TA), TF(TB), SHAPE);
    return k;
}
template <bool TA, bool TB, int SHAPE>
const Kernel<GemmMulti>& sp_multi_kernel(bool sgd) {
    using D = SpDim<SHAPE>;
    static const auto k = make_kernel(&gemm_sp_multi_kernel<TA, TB, SHAPE>, D::RA, D::RB, 512, D::LDS, "gemm_sp_multi_kernel<%s, %s, %d>", TF(TA), TF(TB), SHAPE);
    static const auto ks = make_kernel(&gemm_sp_multi_sgd_kernel<TA, TB, SHAPE>, D::RA, D::RB, 512, D::LDS, "gemm_sp_multi_sgd_kernel<%s, %s, %d>", TF(TA), TF(TB), SHAPE);
    return sgd ? ks : k;
}

int launch_variant(Variant v, const GemmArgs& g, int ta, int tb, hipStream_t s) {
    return by_layout(ta, tb, [&](auto a, auto b) {
        constexpr bool TA = decltype(a)::value, TB = decltype(b)::value;
        switch (v) {
            case V_REG64:       return launch_single(reg_kernel<bf16, TA, TB, 64, 1>(), g, true, s);
            case V_REG128_K64:  return launch_single(reg_kernel<bf16, TA, TB, 64, 2>(), g, true, s);
            case V_REG128_K128: return launch_single(reg_kernel<bf16, TA, TB, 128, 2>(), g, true, s);
            case V_RING64:      return launch_single(ring_kernel<TA, TB, 1>(), g, false, s);
            case V_RING128:     return launch_single(ring_kernel<TA, TB, 2>(), g, false, s);
            case V_BK32:        return launch_single(bk32_kernel<TA, TB>(), g, true, s);
            case V_P8:
#ifdef AUDIOSSL_ABLATE
                // ablation variants of the main loop (WRONG results by design); they exist only in -DAUDIOSSL_ABLATE builds
                // (python audio-ssl_amd/build.py --ablate)
                if (!TA && !TB) {
                    static const char* const e = getenv("AUDIOSSL_GEMM_P8_DBG");
                    static const int dbg = e ? atoi(e) : 0;
                    switch (dbg) {
                        case 1: return launch_single(p8_kernel<false, false, 1>(), g, false, s);      // no MFMA
                        case 2: return launch_single(p8_kernel<false, false, 2>(), g, false, s);      // no DMA after the first two K-tiles
                        case 4: return launch_single(p8_kernel<false, false, 4>(), g, false, s);      // no fragment reads
                        case 6: return launch_single(p8_kernel<false, false, 6>(), g, false, s);      // MFMA + barriers only
                        case 8: return launch_single(p8_kernel<false, false, 8>(), g, false, s);      // no s_setprio
                        default: break;
                    }
                }
#endif
                                return launch_single(p8_kernel<TA, TB, 0>(), g, false, s);
            case V_PK5:         return launch_single(pk5_kernel<TA, TB>(), g, false, s);
            case V_SP5:         return launch_single(sp_kernel<TA, TB, 5>(), g, false, s);
            case V_SP6:         return launch_single(sp_kernel<TA, TB, 6>(), g, false, s);
            case V_SP8:         return launch_single(sp_kernel<TA, TB, 8>(), g, false, s);
            default:            return ASSL_EINVAL;
        }
    });
}

int launch_variant_multi(Variant v, const GemmMulti& gm, int count, int ksplit, int ta, int tb, hipStream_t s) {
    const bool sgd = gm.p[0].sgd_p != nullptr;
    return by_layout(ta, tb, [&](auto a, auto b) {
        constexpr bool TA = decltype(a)::value, TB = decltype(b)::value;
        switch (v) {
            case V_REG64:       return launch_multi(reg_multi_kernel<TA, TB, 64, 1>(), gm, count, ksplit, s);
            case V_REG128_K64:  return launch_multi(reg_multi_kernel<TA, TB, 64, 2>(), gm, count, ksplit, s);
            case V_REG128_K128: return launch_multi(reg_multi_kernel<TA, TB, 128, 2>(), gm, count, ksplit, s);
            case V_P8:          return launch_multi(p8_multi_kernel<TA, TB>(sgd), gm, count, ksplit, s);
            case V_PK5:         return launch_multi(pk5_multi_kernel<TA, TB>(), gm, count, ksplit, s);
            case V_SP5:         return launch_multi(sp_multi_kernel<TA, TB, 5>(sgd), gm, count, ksplit, s);
            case V_SP6:         return launch_multi(sp_multi_kernel<TA, TB, 6>(sgd), gm, count, ksplit, s);
            case V_SP8:         return launch_multi(sp_multi_kernel<TA, TB, 8>(sgd), gm, count, ksplit, s);
            default:            return ASSL_EINVAL;                  // ring, bk32: never legal here
        }
    });
}

// one bf16 problem, validated: choose and launch
int run_bf16(const GemmArgs& g, int ta, int tb, hipStream_t s) {
    if (switches().bad) return ASSL_EINVAL;
    const Choice c = choose(describe(false, 1, ta, tb, g.M, &g.N, &g.K, g.ksplit, g.atomic, g.lse_mode));
    GemmArgs ga = g;
    ga.ksplit = c.ksplit;
    return launch_variant(c.v, ga, ta, tb, s);
}
// count bf16 problems, validated (every gm.p[i] describes one): choose and launch
int run_multi(const GemmMulti& gm, int count, int ta, int tb, const int* Nv, const int* K, hipStream_t s) {
    if (switches().bad) return ASSL_EINVAL;
    const Choice c = choose(describe(true, count, ta, tb, gm.p[0].M, Nv, K, gm.p[0].ksplit, gm.p[0].atomic, 0));
    return launch_variant_multi(c.v, gm, count, c.ksplit, ta, tb, s);
}

// the 8-columns-per-lane epilogue needs whole, aligned vectors of every operand it touches
int epi_vectorisable(const GemmArgs& g, int dtype) {
    if (dtype != 1 || g.atomic == 1 || g.N % 8) return 0;
    const size_t csz = g.out_f32 ? 4 : 2;
    if (((size_t)g.C * 1) % 16 || (g.ldc * csz) % 16) return 0;
    if (g.bias && (size_t)g.bias % 16) return 0;
    if (g.keep && ((size_t)g.keep % 8 || g.ldk % 8)) return 0;
    if (g.gate && ((size_t)g.gate % 16 || g.ldg % 8)) return 0;
    if (g.resid && ((size_t)g.resid % 16 || g.ldr % 4)) return 0;
    return 1;
}

// The operand rules of every entry point, and the start of its GemmArgs (zero-initialised: no epilogue term, keep_scale 1, one K split):
// the vector (8-element) dimension of each operand is a multiple of 8 (ASSL_EINVAL), base pointers and rows are 16-byte aligned -
// the entry point's other pointers too, passed as extra_aligned - (ASSL_EALIGN), and the extents fit 32-bit buffer offsets (ASSL_EINVAL).
int operands(GemmArgs& g, int ta, int tb, int M, int N, int K, const void* A, long lda, const void* B, long ldb, long esz,
             bool extra_aligned = true) {
    ASSL_REQUIRE((ta ? M : K) % 8 == 0 && (tb ? N : K) % 8 == 0);
    if (!ASSL_ALIGNED16(A) || !ASSL_ALIGNED16(B) || lda % 8 || ldb % 8 || !extra_aligned) return ASSL_EALIGN;
    const long a_ext = (ta ? ((long)(K - 1) * lda + M) : ((long)(M - 1) * lda + K)) * esz;
    const long b_ext = (tb ? ((long)(K - 1) * ldb + N) : ((long)(N - 1) * ldb + K)) * esz;
    ASSL_REQUIRE(a_ext < 0xFFFFFF00L && b_ext < 0xFFFFFF00L);
    g = GemmArgs{};
    g.A = A; g.B = B; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb;
    g.a_bytes = (unsigned)a_ext; g.b_bytes = (unsigned)b_ext;
    g.keep_scale = 1.f; g.ksplit = 1;
    return ASSL_OK;
}

}  // namespace

extern "C" int audiossl_gemm_multi(int count, int trans_a, int trans_b, int M, const int* Nv, const int* K, float alpha,
                                   const void* const* A, const long* lda, const void* const* B, const long* ldb,
                                   void* const* C, const long* ldcv, int out_f32, int atomic, int ksplit, void* stream) {
    ASSL_REQUIRE(count >= 1 && count <= MAX_MULTI && Nv && K && A && B && C && lda && ldb && ldcv && M > 0 && ksplit >= 1);
    for (int i = 0; i < count; ++i) ASSL_REQUIRE(Nv[i] > 0);
    ASSL_REQUIRE(atomic >= 0 && atomic <= 2);
    ASSL_REQUIRE(!atomic || out_f32);
    ASSL_REQUIRE(ksplit == 1 || atomic == 1);
    GemmMulti gm;
    for (int i = 0; i < count; ++i) {
        GemmArgs& g = gm.p[i];
        ASSL_REQUIRE(A[i] && B[i] && C[i] && K[i] > 0);
        if (const int rc = operands(g, trans_a, trans_b, M, Nv[i], K[i], A[i], lda[i], B[i], ldb[i], 2)) return rc;
        g.C = C[i]; g.ldc = ldcv[i]; g.alpha = alpha;
        g.out_f32 = out_f32; g.atomic = atomic; g.ksplit = ksplit;
        g.vec_epi = epi_vectorisable(g, 1);
    }
    return run_multi(gm, count, trans_a, trans_b, Nv, K, static_cast<hipStream_t>(stream));
}

// Weight gradients that are applied where they are produced: G_i = alpha * op(A_i) op(B_i) is the gradient of parameter P_i ([M][N_i]
// fp32, leading dimension ldp[i]); the epilogue runs torch.optim.SGD's update on P_i and its momentum buffer Mom_i in place (sgd_step,
// common.h - the same arithmetic as audiossl_sgd_momentum, bit for bit) and writes the bf16 copy of the new parameter to Shadow_i
// (array or entries nullable).  G is never stored: per step that saves the 4-byte write and the optimiser's 4-byte read of every element
// of the projector weights (264 MB at DeLoRes-M's three heads).  One K split only; the momentum buffers must exist (not the first step).
extern "C" int audiossl_gemm_multi_sgd(int count, int trans_a, int trans_b, int M, const int* Nv, const int* K, float alpha,
                                       const void* const* A, const long* lda, const void* const* B, const long* ldb,
                                       float* const* P, float* const* Mom, void* const* Shadow, const long* ldp, float lr, float momentum,
                                       float weight_decay, float grad_scale, const float* grad_scale_dev, void* stream) {
    ASSL_REQUIRE(count >= 1 && count <= MAX_MULTI && Nv && K && A && B && P && Mom && lda && ldb && ldp && M > 0);
    for (int i = 0; i < count; ++i) ASSL_REQUIRE(Nv[i] > 0);
    GemmMulti gm;
    for (int i = 0; i < count; ++i) {
        GemmArgs& g = gm.p[i];
        ASSL_REQUIRE(A[i] && B[i] && P[i] && Mom[i] && K[i] > 0);
        void* sh = Shadow ? Shadow[i] : nullptr;
        if (const int rc = operands(g, trans_a, trans_b, M, Nv[i], K[i], A[i], lda[i], B[i], ldb[i], 2,
                      ASSL_ALIGNED16(P[i]) && ASSL_ALIGNED16(Mom[i]) && ldp[i] % 8 == 0 && Nv[i] % 8 == 0 && ASSL_ALIGNED16(sh))) return rc;
        g.C = P[i]; g.ldc = ldp[i]; g.alpha = alpha;
        g.out_f32 = 1;
        g.vec_epi = epi_vectorisable(g, 1);
        g.sgd_p = P[i]; g.sgd_m = Mom[i]; g.sgd_s = static_cast<bf16*>(sh); g.sgd_gs_dev = grad_scale_dev;
        g.sgd_lr = lr; g.sgd_mu = momentum; g.sgd_wd = weight_decay; g.sgd_gs = grad_scale;
    }
    return run_multi(gm, count, trans_a, trans_b, Nv, K, static_cast<hipStream_t>(stream));
}

// The Barlow-twins cross-correlation of several heads, c_h = alpha * A_h^T B_h (A_h, B_h: [K_h][M] / [K_h][N] row-major, i.e. the
// two normalised views), with the loss and its gradient folded into the epilogue (`delores_s/upstream_expert.py:118-131`):
// dc_h = dscale_h * (c_h - I) in bf16, loss_rep_h[0..31] += coef_h * sum (c_h - I)^2 (32 replicas, the caller sums them; zeroed by
// the caller).  c_h is never stored (50 MB written + read per launch at D = 2048, three heads).
extern "C" int audiossl_gemm_multi_barlow(int count, int D, const int* K, float alpha, const void* const* A, const long* lda,
                                          const void* const* B, const long* ldb, void* const* dc, const float* coef, const float* dscale,
                                          float* const* loss_rep, void* stream) {
    ASSL_REQUIRE(count >= 1 && count <= MAX_MULTI && K && A && B && dc && lda && ldb && coef && dscale && loss_rep && D > 0 && D % 64 == 0);
    GemmMulti gm;
    int Nv[MAX_MULTI];
    for (int i = 0; i < count; ++i) {
        GemmArgs& g = gm.p[i];
        ASSL_REQUIRE(A[i] && B[i] && dc[i] && loss_rep[i] && K[i] > 0 && K[i] % 8 == 0);
        if (const int rc = operands(g, 1, 1, D, D, K[i], A[i], lda[i], B[i], ldb[i], 2, ASSL_ALIGNED16(dc[i]))) return rc;
        g.C = dc[i]; g.ldc = D; g.alpha = alpha;
        g.vec_epi = epi_vectorisable(g, 1);
        ASSL_REQUIRE(g.vec_epi);
        g.bl_mode = 1; g.bl_loss = loss_rep[i]; g.bl_coef = coef[i]; g.bl_dscale = dscale[i];
        Nv[i] = D;
    }
    return run_multi(gm, count, 1, 1, Nv, K, static_cast<hipStream_t>(stream));
}

// dtype: 0 = fp32 operands (exact f32 MFMA), 1 = bf16 operands.  See include/audiossl_hip.h.
extern "C" int audiossl_gemm(int dtype, int trans_a, int trans_b, int M, int N, int K, float alpha,
                             const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                             const float* bias, int relu, const uint8_t* keep, long ldk, float keep_scale,
                             const void* gate, long ldg, int out_f32, int atomic, int ksplit, const float* resid, long ldr,
                             void* stream) {
    ASSL_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0 && ksplit >= 1);
    ASSL_REQUIRE(dtype == 0 || dtype == 1);
    ASSL_REQUIRE(atomic >= 0 && atomic <= 2);
    ASSL_REQUIRE(!atomic || out_f32 || dtype == 0);
    ASSL_REQUIRE(ksplit == 1 || atomic == 1);
    ASSL_REQUIRE(ksplit == 1 || (!relu && !keep && !gate));             // non-linear epilogue terms need the whole sum (the bias is added by split 0)
    ASSL_REQUIRE(!resid || (ksplit == 1 && !atomic));
    GemmArgs g;
    if (const int rc = operands(g, trans_a, trans_b, M, N, K, A, lda, B, ldb, dtype == 0 ? 4 : 2)) return rc;
    g.C = C; g.ldc = ldc; g.alpha = alpha;
    g.bias = bias; g.relu = relu; g.keep = keep; g.ldk = ldk; g.keep_scale = keep_scale; g.gate = gate; g.ldg = ldg;
    g.out_f32 = (dtype == 0) ? 1 : out_f32; g.atomic = atomic; g.ksplit = ksplit; g.resid = resid; g.ldr = ldr;
    g.vec_epi = epi_vectorisable(g, dtype);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == 1) return run_bf16(g, trans_a, trans_b, s);
    if (switches().bad) return ASSL_EINVAL;
    // fp32 operands (the validation / high-precision path): one kernel
    return by_layout(trans_a, trans_b, [&](auto a, auto b) {
        return launch_single(reg_kernel<float, decltype(a)::value, decltype(b)::value, 32, 2>(), g, true, s);
    });
}

// Linear -> ReLU -> Dropout of the encoder's first fully connected layer (`src/encoder/audiontt.py:62-66`) with the keep mask drawn in
// the epilogue: C = dropout(relu(alpha * op(A) op(B) + bias)), element (row, col) kept iff dropout_keep(seed', row * N + col) with
// seed' = (seed + *counter) mod 2^48 - bit for bit the mask audiossl_dropout_mask(keep [M][N], seed, p, counter) writes, which this
// launch neither needs written (12.6 MB at B = 512) nor read back.  The backward needs no mask: it gates on the stored output.
extern "C" int audiossl_gemm_dropout(int trans_a, int trans_b, int M, int N, int K, float alpha, const void* A, long lda,
                                     const void* B, long ldb, void* C, long ldc, const float* bias, int relu,
                                     unsigned long long seed, float p, const long long* counter, float keep_scale, void* stream) {
    ASSL_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0 && p >= 0.f && p < 1.f);
    GemmArgs g;
    if (const int rc = operands(g, trans_a, trans_b, M, N, K, A, lda, B, ldb, 2)) return rc;
    g.C = C; g.ldc = ldc; g.alpha = alpha;
    g.bias = bias; g.relu = relu; g.keep_scale = keep_scale;
    g.vec_epi = epi_vectorisable(g, 1);
    g.drop_on = 1;
    g.drop_thr = (unsigned int)fminf(p * 4294967296.f, 4294967295.f);
    g.drop_seed = seed;
    g.drop_counter = counter;
    return run_bf16(g, trans_a, trans_b, static_cast<hipStream_t>(stream));
}

// MoCo InfoNCE logits  qn [B][dim] * queue [dim][K] / T  with the row soft-max folded into the GEMM epilogue
// (`src/upstream/delores_m/upstream_expert.py:250-264`): mode 1 writes per-row (max, sum exp) partials of every 64-column
// slab (merged by audiossl_moco_lse_merge), mode 2 recomputes the logits and stores P = exp(l - lse) * gscale in bf16, the
// operand of the dq GEMM.  The [B][K] fp32 logits (134 MB at B = 512, K = 65,536) are never written.
extern "C" int audiossl_moco_logits(int mode, const void* qn, const void* queue, int B, int K, int dim, float inv_t, float* part,
                                    const float* lse, float gscale, void* P, void* stream) {
    ASSL_REQUIRE(qn && queue && B > 0 && K > 0 && dim > 0 && (mode == 1 || mode == 2));
    ASSL_REQUIRE(mode == 1 ? part != nullptr : (lse != nullptr && P != nullptr));
    GemmArgs g;
    if (const int rc = operands(g, 0, 1, B, K, dim, qn, dim, queue, K, 2, ASSL_ALIGNED16(P))) return rc;
    g.C = P; g.ldc = K; g.alpha = inv_t;
    g.lse_mode = mode; g.part = part; g.lse = lse; g.gscale = gscale; g.nslot = ceil_div(K, 64);
    return run_bf16(g, 0, 1, static_cast<hipStream_t>(stream));
}
