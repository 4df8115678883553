// Exact minimum spanning tree of the COMPLETE mutual-reachability graph of an [n][d] fp32 matrix, without the n x n matrix: the
// one stage HDBSCAN (Campello et al. 2013) needs that a nearest-neighbour list cannot give.  w2_ij = max(d2_ij, core2_i, core2_j),
// d2_ij = max(0, (n_i + n_j) - 2 g_ij) with g_ij from gram_tile<ChainOrder::Index> and n_i from gram_norm_kernel<ChainOrder::Index>:
// knn_graph_l2's and range_fill's arithmetic, so a core2 taken from knn_graph_l2 ties bit for bit with the matching d2_ij here.
//
// Boruvka.  Edges are compared by the strict total order (w2 bits, min(i, j), max(i, j)); w2 >= 0, so the bits order as the
// values do.  Every round each component picks its smallest outgoing edge and the components an edge joins are merged.  Under a
// strict total order the picks cannot close a cycle longer than two: along a cycle c_1 -> c_2 -> ... -> c_1 every pick would have
// to be strictly smaller than the one before it; a cycle of two is a pair that picked the SAME edge, which is written once.  The
// smallest outgoing edge of a component is in the unique MST, so the tree is the one Kruskal finds under the same order, whatever
// `splits` is and however the tiles are walked.  A round at least halves the number of components: ceil(log2 n) rounds.
//
// One round (state[r] = components and edges before round r; a kernel of a round whose count is 1 returns at once):
//   row pass    one workgroup per 64 owned rows and split of the walked tiles, as range_count_kernel: the compare runs on the
//               accumulators, a lane keeps the smallest key (w2 bits << 32 | j) among walked rows of ANOTHER component (for a fixed i
//               the order of the edges is the order of j); four lanes per row meet in LDS (64-bit integer min), one candidate per
//               (row, split).  Norms, core distances and component ids of the walked tile are staged in LDS.
//   merge       per row: the smallest candidate over the splits; per component a 64-bit atomicMin of (w2 bits << 32 | lo).
//   hi          per row whose (w2, lo) is its component's: a 32-bit atomicMin of hi.  Integer minima do not depend on order.
//   choose      per component: partner = the component of the far end; the pair is mutual when the partner chose the same edge.
//               A component owns its edge unless it is the larger id of a mutual pair; parent = partner (the smaller id of a
//               mutual pair is a root).
//   scan        exclusive scan of the owner flags over component ids -> output slots; state[r + 1].
//   write       owners store their edge at edges_before + slot: rounds in order, inside a round by component id.
//   jump        pointer doubling, ceil(log2 n) - r launches: round r starts with at most n / 2^r components.
//   relabel     comp[i] = root of comp[i]; the per-component minima are reset for the next round.
//
// Every loop has a trip count fixed by n, d and splits: a mistake in the handling of ties can give a wrong tree, never a kernel
// that does not end.  No float atomics, no grid-wide barriers, plain launches only; the kernels initialise whatever they read of
// the workspace, and nothing synchronises with the host.
#include "topk.h"          // plan_splits, TARGET_WG
#include "gram_tile.h"
#include "csr_sym.h"       // csr_align16

namespace {

constexpr int MAX_SPLITS = 64;
constexpr unsigned long long NO_EDGE = ~0ull;
// staging + the walked tile's norms, core distances and component ids (two buffers each) + the owned rows' keys
constexpr int ROW_LDS_BYTES = STAGE_BYTES + 3 * 2 * BT * 4 + QT * 8;

struct MstArgs {
    const float* x;          // [n][d]
    const float* core2;      // [n] or null (all zeros)
    const float* gn;         // [n] squared norms in the tile's own chain
    const int* comp;         // [n] the row's component, named by one of its rows (the root of the merges so far)
    const int* state;        // [2 (rounds + 1)]: components, edges before round r
    unsigned long long* cand;    // [q_tiles * QT][splits]
    int n, d, round;
    int tiles, tiles_per_split, splits;
};

__global__ __launch_bounds__(256) void mst_row_kernel(MstArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (a.state[2 * a.round] <= 1) return;                           // uniform over the grid: the tree is complete
    float* Os = reinterpret_cast<float*>(smem);                      // [QT][RP] owned rows
    float* Ws = Os + QT * RP;                                        // [BT][RP] walked rows
    float* Nj = reinterpret_cast<float*>(smem + STAGE_BYTES);        // [2][BT]
    float* Kj = Nj + 2 * BT;                                         // [2][BT]
    int* Cj = reinterpret_cast<int*>(Kj + 2 * BT);                   // [2][BT]
    unsigned long long* Rs = reinterpret_cast<unsigned long long*>(Cj + 2 * BT);     // [QT]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const long q0 = (long)blockIdx.x * QT;
    const int q = (w & 1) * 32 + l31;                                // this lane's owned row (the C/D column)
    const long gq = q0 + q;
    const bool qok = gq < a.n;
    const float ni = qok ? a.gn[gq] : 0.f;
    const float ki = (qok && a.core2) ? a.core2[gq] : 0.f;
    const int ci = qok ? a.comp[gq] : -1;
    if (tid < QT) Rs[tid] = NO_EDGE;

    const int t0 = blockIdx.y * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.tiles);
    unsigned long long best = NO_EDGE;
    for (int t = t0; t < t1; ++t) {
        const long b0 = (long)t * BT;
        const int buf = (t & 1) * BT;                                // the other buffer may still be read by a slower wave
        if (tid < BT) {
            const long j = b0 + tid;
            const bool ok = j < a.n;
            Nj[buf + tid] = ok ? a.gn[j] : 0.f;
            Kj[buf + tid] = (ok && a.core2) ? a.core2[j] : 0.f;
            Cj[buf + tid] = ok ? a.comp[j] : -1;                     // a row past n is in no component: never a candidate
        }
        f32x16 acc[2];
        gram_tile<ChainOrder::Index>(a.x, a.n, a.d, q0, b0, Os, Ws, acc);    // (its barriers publish the three buffers)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 64 * (w >> 1) + 32 * tt + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int cj = Cj[buf + c];
                const float dd = fmaxf((ni + Nj[buf + c]) - 2.f * acc[tt][r], 0.f);
                const float w2 = fmaxf(fmaxf(dd, ki), Kj[buf + c]);
                const unsigned long long key = ((unsigned long long)__float_as_uint(w2) << 32) | (unsigned)(b0 + c);
                const bool ok = qok && cj >= 0 && cj != ci;          // another component: i == j leaves with its own
                best = (ok && key < best) ? key : best;
            }
    }
    __syncthreads();                                                 // Rs is set (also when the split walked nothing)
    if (best != NO_EDGE) atomicMin(&Rs[q], best);                    // integer: four lanes per owned row
    __syncthreads();
    if (tid < QT) a.cand[((long)blockIdx.x * QT + tid) * a.splits + blockIdx.y] = Rs[tid];
}

// comp[i] = i, the per-component minima empty, state[0] = (n components, 0 edges).
__global__ __launch_bounds__(256) void mst_init_kernel(int n, int* __restrict__ comp, unsigned long long* __restrict__ ckey,
                                                       unsigned* __restrict__ chi, int* __restrict__ state) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        comp[i] = (int)i;
        ckey[i] = NO_EDGE;
        chi[i] = ~0u;
    }
    if (i == 0) {
        state[0] = n;
        state[1] = 0;
    }
}

// rowbest[i] = the row's smallest candidate over the splits; its (w2, lo) goes into the component's 64-bit minimum.
__global__ __launch_bounds__(256) void mst_merge_kernel(const unsigned long long* __restrict__ cand, int splits, int n, int round,
                                                        const int* __restrict__ state, const int* __restrict__ comp,
                                                        unsigned long long* __restrict__ rowbest, unsigned long long* __restrict__ ckey) {
    if (state[2 * round] <= 1) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long best = NO_EDGE;
    for (int p = 0; p < splits; ++p) {
        const unsigned long long c = cand[i * splits + p];
        best = c < best ? c : best;
    }
    rowbest[i] = best;
    if (best == NO_EDGE) return;
    const unsigned j = (unsigned)best, lo = j < (unsigned)i ? j : (unsigned)i;
    atomicMin(&ckey[comp[i]], (best & 0xFFFFFFFF00000000ull) | lo);
}

__global__ __launch_bounds__(256) void mst_hi_kernel(const unsigned long long* __restrict__ rowbest, int n, int round,
                                                     const int* __restrict__ state, const int* __restrict__ comp,
                                                     const unsigned long long* __restrict__ ckey, unsigned* __restrict__ chi) {
    if (state[2 * round] <= 1) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long best = rowbest[i];
    if (best == NO_EDGE) return;
    const unsigned j = (unsigned)best, lo = j < (unsigned)i ? j : (unsigned)i, hi = j < (unsigned)i ? (unsigned)i : j;
    const int c = comp[i];
    if (((best & 0xFFFFFFFF00000000ull) | lo) == ckey[c]) atomicMin(&chi[c], hi);
}

// Per component (a row that is its own component id).  With more than one component every component has an outgoing edge; an
// empty minimum or an end outside [0, n) can only come from a damaged workspace and leaves the component alone.
__global__ __launch_bounds__(256) void mst_choose_kernel(int n, int round, const int* __restrict__ state, const int* __restrict__ comp,
                                                         const unsigned long long* __restrict__ ckey, const unsigned* __restrict__ chi,
                                                         int* __restrict__ parent, int* __restrict__ flag) {
    if (state[2 * round] <= 1) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int p = (int)i, own = 0;
    if (comp[i] == (int)i) {
        const unsigned long long key = ckey[i];
        const unsigned lo = (unsigned)key, hi = chi[i];
        if (key != NO_EDGE && lo < (unsigned)n && hi < (unsigned)n) {
            const int clo = comp[lo], chh = comp[hi];
            const int pc = clo == (int)i ? chh : clo;                // the component of the far end
            if (pc >= 0 && pc < n && pc != (int)i) {
                const bool mutual = ckey[pc] == key && chi[pc] == hi;
                own = (mutual && pc < (int)i) ? 0 : 1;
                p = (mutual && (int)i < pc) ? (int)i : pc;
            }
        }
    }
    parent[i] = p;
    flag[i] = own;
}

// slot[i] = owners before i; state[r + 1] = (components - owners, edges + owners).  One workgroup, as range_scan_kernel.
__global__ __launch_bounds__(1024) void mst_scan_kernel(const int* __restrict__ flag, int n, int round, int* __restrict__ state,
                                                        int* __restrict__ slot) {
    __shared__ int sh[1024];
    const int tid = threadIdx.x;
    const int comps = state[2 * round], edges = state[2 * round + 1];
    if (comps <= 1) {
        if (tid == 0) {
            state[2 * round + 2] = comps;
            state[2 * round + 3] = edges;
        }
        return;
    }
    const long chunk = ((long)n + 1023) / 1024;
    const long lo = min(tid * chunk, (long)n), hi = min(lo + chunk, (long)n);
    int s = 0;
    for (long i = lo; i < hi; ++i) s += flag[i];
    sh[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    int base = sh[tid] - s;
    for (long i = lo; i < hi; ++i) {
        slot[i] = base;
        base += flag[i];
    }
    if (tid == 1023) {
        state[2 * round + 2] = comps - sh[1023];
        state[2 * round + 3] = edges + sh[1023];
    }
}

__global__ __launch_bounds__(256) void mst_write_kernel(int n, int round, const int* __restrict__ state, const int* __restrict__ flag,
                                                        const int* __restrict__ slot, const unsigned long long* __restrict__ ckey,
                                                        const unsigned* __restrict__ chi, int* __restrict__ eu, int* __restrict__ ev,
                                                        float* __restrict__ ew2) {
    if (state[2 * round] <= 1) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const long o = (long)state[2 * round + 1] + slot[i];
    if (o < 0 || o >= n - 1) return;                                 // a tree has n - 1 edges: nothing is written past them
    const unsigned long long key = ckey[i];
    eu[o] = (int)(unsigned)key;
    ev[o] = (int)chi[i];
    ew2[o] = __uint_as_float((unsigned)(key >> 32));
}

__global__ __launch_bounds__(256) void mst_jump_kernel(const int* __restrict__ in, int n, int round, const int* __restrict__ state,
                                                       int* __restrict__ out) {
    if (state[2 * round] <= 1) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[in[i]];
}

__global__ __launch_bounds__(256) void mst_relabel_kernel(const int* __restrict__ root, int n, int round, const int* __restrict__ state,
                                                          int* __restrict__ comp, unsigned long long* __restrict__ ckey,
                                                          unsigned* __restrict__ chi) {
    if (state[2 * round] <= 1) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    comp[i] = root[comp[i]];                                         // comp[i] is a component id; the roots were flattened
    ckey[i] = NO_EDGE;
    chi[i] = ~0u;
}

__global__ void mst_rounds_kernel(const int* __restrict__ state, int total, int* __restrict__ rounds) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int used = 0;
    for (int r = 0; r < total; ++r) used += state[2 * r] > 1 ? 1 : 0;
    rounds[0] = used;
}

struct MstPlan {
    long q_tiles;
    int tiles, splits, tiles_per_split, rounds;
    long off_comp, off_pa, off_pb, off_flag, off_slot, off_chi, off_state, off_ckey, off_rowbest, off_cand, bytes;
};

inline long mst_cand_slots(long q_tiles, int splits) {
    // the library's own choice never exceeds ceil(TARGET_WG / q_tiles) and MAX_SPLITS; a forced value is taken as it is
    const long a = q_tiles + TARGET_WG - 1, b = q_tiles * MAX_SPLITS;
    const long own = a < b ? a : b, forced = q_tiles * (long)(splits > 0 ? splits : 1);
    return own > forced ? own : forced;
}

bool mst_plan(int n, int splits, MstPlan& p) {
    if (!(n >= 2 && splits >= 0 && splits <= MAX_SPLITS)) return false;
    p.q_tiles = ((long)n + QT - 1) / QT;
    p.tiles = (int)(((long)n + BT - 1) / BT);
    if (splits == 0) {
        const SplitPlan sp = plan_splits(p.q_tiles, p.tiles, 4);
        p.splits = sp.splits < MAX_SPLITS ? sp.splits : MAX_SPLITS;
    } else {
        p.splits = splits < p.tiles ? splits : p.tiles;
    }
    p.tiles_per_split = (p.tiles + p.splits - 1) / p.splits;
    p.splits = (p.tiles + p.tiles_per_split - 1) / p.tiles_per_split;              // no empty split
    p.rounds = 0;
    while ((1L << p.rounds) < n) ++p.rounds;                                       // ceil(log2 n)
    const long words = csr_align16((long)n * 4);
    long o = words;                                                                // the norms come first
    p.off_comp = o;      o += words;
    p.off_pa = o;        o += words;
    p.off_pb = o;        o += words;
    p.off_flag = o;      o += words;
    p.off_slot = o;      o += words;
    p.off_chi = o;       o += words;
    p.off_state = o;     o += csr_align16(2L * (p.rounds + 1) * 4);
    p.off_ckey = o;      o += csr_align16((long)n * 8);
    p.off_rowbest = o;   o += csr_align16((long)n * 8);
    p.off_cand = o;      o += mst_cand_slots(p.q_tiles, splits) * QT * 8;
    p.bytes = o;
    return true;
}

}  // namespace

extern "C" int audiossl_mreach_mst_workspace(int n, int splits, long* bytes) {
    MstPlan p;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(mst_plan(n, splits, p));
    *bytes = p.bytes;
    return ASSL_OK;
}

extern "C" int audiossl_mreach_mst(const float* x, int n, int d, const float* core2, int splits, int* eu, int* ev, float* ew2,
                                   int* rounds, void* workspace, long workspace_bytes, void* stream) {
    MstPlan p;
    ASSL_REQUIRE(x && eu && ev && ew2 && workspace);
    ASSL_REQUIRE(gram_width_ok(d));
    ASSL_REQUIRE(mst_plan(n, splits, p));
    ASSL_REQUIRE(workspace_bytes >= p.bytes);
    if (!ASSL_ALIGNED16(x) || !ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    char* ws = static_cast<char*>(workspace);
    float* gn = reinterpret_cast<float*>(ws);
    int* comp = reinterpret_cast<int*>(ws + p.off_comp);
    int* pa = reinterpret_cast<int*>(ws + p.off_pa);
    int* pb = reinterpret_cast<int*>(ws + p.off_pb);
    int* flag = reinterpret_cast<int*>(ws + p.off_flag);
    int* slot = reinterpret_cast<int*>(ws + p.off_slot);
    unsigned* chi = reinterpret_cast<unsigned*>(ws + p.off_chi);
    int* state = reinterpret_cast<int*>(ws + p.off_state);
    unsigned long long* ckey = reinterpret_cast<unsigned long long*>(ws + p.off_ckey);
    unsigned long long* rowbest = reinterpret_cast<unsigned long long*>(ws + p.off_rowbest);
    MstArgs a;
    a.x = x; a.core2 = core2; a.gn = gn; a.comp = comp; a.state = state;
    a.cand = reinterpret_cast<unsigned long long*>(ws + p.off_cand);
    a.n = n; a.d = d; a.round = 0;
    a.tiles = p.tiles; a.tiles_per_split = p.tiles_per_split; a.splits = p.splits;

    hipLaunchKernelGGL(gram_norm_kernel<ChainOrder::Index>, GRID1(n), dim3(256), 0, s, x, n, d, (long)n, gn);
    hipLaunchKernelGGL(mst_init_kernel, GRID1(n), dim3(256), 0, s, n, comp, ckey, chi, state);
    for (int r = 0; r < p.rounds; ++r) {
        a.round = r;
        hipLaunchKernelGGL(mst_row_kernel, dim3((unsigned)p.q_tiles, (unsigned)p.splits), dim3(256), ROW_LDS_BYTES, s, a);
        hipLaunchKernelGGL(mst_merge_kernel, GRID1(n), dim3(256), 0, s, a.cand, p.splits, n, r, state, comp, rowbest, ckey);
        hipLaunchKernelGGL(mst_hi_kernel, GRID1(n), dim3(256), 0, s, rowbest, n, r, state, comp, ckey, chi);
        hipLaunchKernelGGL(mst_choose_kernel, GRID1(n), dim3(256), 0, s, n, r, state, comp, ckey, chi, pa, flag);
        hipLaunchKernelGGL(mst_scan_kernel, dim3(1), dim3(1024), 0, s, flag, n, r, state, slot);
        hipLaunchKernelGGL(mst_write_kernel, GRID1(n), dim3(256), 0, s, n, r, state, flag, slot, ckey, chi, eu, ev, ew2);
        int* in = pa;
        int* out = pb;
        for (int jmp = 0; jmp < p.rounds - r; ++jmp) {               // at most n / 2^r components: a path is shorter than 2^(rounds - r)
            hipLaunchKernelGGL(mst_jump_kernel, GRID1(n), dim3(256), 0, s, in, n, r, state, out);
            int* t = in; in = out; out = t;
        }
        hipLaunchKernelGGL(mst_relabel_kernel, GRID1(n), dim3(256), 0, s, in, n, r, state, comp, ckey, chi);
    }
    if (rounds) hipLaunchKernelGGL(mst_rounds_kernel, dim3(1), dim3(64), 0, s, state, p.rounds, rounds);
    ASSL_LAUNCH_CHECK();
}
