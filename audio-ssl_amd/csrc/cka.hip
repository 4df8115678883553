// Centred kernel alignment (CKA) between two sets of features of the same n clips: linear and RBF, the analysis of the
// reference's `extras/CKA.py` (numpy: n x n Gram matrices, centred by n x n x n products).  Here no n x n matrix is stored.
//
// Centring identity.  For symmetric K, L and H = I - 11^T / n:
//     sum(HKH * HLH) = S_KL - (2 / n) sum_i k_i l_i + k l / n^2,    S_KL = sum_ij K_ij L_ij,  k_i, l_i row sums,  k, l totals.
// One sweep over the tiles of K and L TOGETHER gives S_KL, S_KK, S_LL and both row-sum vectors; all three HSIC values and
// CKA = HSIC_xy / sqrt(HSIC_xx HSIC_yy) follow.  Subtracting the column means of X and Y first (cka_center; the Python layer
// does it by default) changes neither the centred linear Gram nor any distance and removes the cancellation in both.
//
// Tile.  g_ij = <x_i, x_j> is the fp32 Gram tile of gram_tile.h in halves chain order (0 4 1 5 2 6 3 7 inside every group
// of 8), g_ii its norm kernel, so (g_ii + g_jj) - 2 g_ij is 0 wherever row j repeats row i, and i == j is set to 0
// outright.  The tile stays in registers here: a lane's MFMA column is one owned row and its 2 x 16 registers are 32 + 32
// columns j, so row sums never leave the lane; the sweep calls the tile twice per column tile (x, then y) and two
// workgroups per CU keep the pipe busy.  Rows and columns past n are masked out of every sum and histogram.  What this
// file adds on top of the tile: the HSIC sums, the histogram passes of the median rule, the select and the finalise.
//
// RBF.  d_ij = max((g_ii + g_jj) - 2 g_ij, 0), K_ij = exp(d_ij c), c = (float)(-0.5 / sigma^2) formed in fp64 and rounded once.
// sigma^2 = median of the non-zero d_ij (the reference's np.median(KX[KX != 0]); the matrix is symmetric, so the median over
// j > i alone is the same number): the mean of the order statistics (M - 1) / 2 and M / 2 of the M non-zero entries above
// the diagonal, found EXACTLY by a radix select over the bit patterns of the kernel's own fp32 distances (positive floats
// order like their bits): three digit passes (11 + 11 + 10 bits), each recomputing the Gram tiles (tiles wholly on or
// below the diagonal are skipped), an LDS histogram per workgroup flushed with 64-bit integer atomics, and a one-block
// select kernel that picks the bin, derives M and both ranks on the device and clears the histogram for the next pass.
// The two ranks may part ways at any digit, so two prefixes are followed, each with its own histogram.
//
// Accumulation.  Tile values are fp32; S_*, the row sums and the fold are fp64 (exact on integer data).  No floating-point
// atomics: every workgroup writes its partials to the workspace, cka_finalize_kernel folds them in a fixed order, so two
// runs agree bit for bit.  The kernels initialise whatever they read; the workspace needs no clearing by the caller.
// The full square is swept (K and L are symmetric; the triangle would halve a cost of milliseconds).
#include "topk.h"          // plan_splits, TARGET_WG
#include "gram_tile.h"

namespace {

constexpr int MIN_TILES = 2;         // column tiles per split at least
constexpr int NBIN = 2048;           // radix-select bins per pass (11 + 11 + 10 bits)
constexpr int MAX_N = 65536;

enum { MODE_LINEAR = 0, MODE_RBF = 1, MODE_HIST = 2 };

// radix-select state in the workspace (unsigned long long each): two followed order statistics
enum { ST_PREFIX_LO = 0, ST_PREFIX_HI = 1, ST_RANK_LO = 2, ST_RANK_HI = 3, ST_COUNT = 4, ST_WORDS = 8 };

struct CkaPlan {
    int row_blocks, col_tiles, splits, tiles_per_split;
    long n_pad;
    // workspace offsets (bytes)
    long off_gx, off_gy, off_rk, off_rl, off_s, off_hist, off_state, bytes;
};

// Splits (plan_splits in topk.h): MIN_TILES column tiles each at least.  The workspace figure uses row_blocks + TARGET_WG >=
// row_blocks * splits, so it grows with n.
bool cka_plan(long n, CkaPlan& p) {
    if (!(n >= 2 && n <= MAX_N)) return false;
    p.row_blocks = (int)((n + QT - 1) / QT);
    p.col_tiles = (int)((n + BT - 1) / BT);
    p.n_pad = (long)p.row_blocks * QT;
    const SplitPlan sp = plan_splits(p.row_blocks, p.col_tiles, MIN_TILES);
    p.splits = sp.splits;
    p.tiles_per_split = sp.tiles_per_split;
    const long wg_bound = (long)p.row_blocks + TARGET_WG;
    long o = 0;
    p.off_gx = o;    o += p.n_pad * 4;
    p.off_gy = o;    o += p.n_pad * 4;
    p.off_rk = o;    o += wg_bound * QT * 8;
    p.off_rl = o;    o += wg_bound * QT * 8;
    p.off_s = o;     o += wg_bound * 4 * 8;
    p.off_hist = o;  o += 2L * NBIN * 8;
    p.off_state = o; o += ST_WORDS * 8;
    p.bytes = o;
    return true;
}

struct CkaArgs {
    const float* x;       // [n][p]
    const float* y;       // [n][q]  (unused in MODE_HIST)
    const float* gx;      // [n_pad] squared norms in the tile's own chain order (RBF, HIST)
    const float* gy;
    const double* s2x;    // device sigma^2 per matrix, or null: s2_given serves both
    const double* s2y;
    double s2_given;
    double* part_rk;      // [splits][n_pad]
    double* part_rl;
    double* part_s;       // [row_blocks * splits][4]
    unsigned long long* hist;     // [2][NBIN]
    const unsigned long long* state;
    int n, p, q;
    int col_tiles, tiles_per_split;
    long n_pad;
    int dshift, dmask, pshift;    // HIST: digit = (bits >> dshift) & dmask, followed iff (bits >> pshift) == prefix
};

template <int MODE>
__global__ __launch_bounds__(256, 2) void cka_sweep_kernel(CkaArgs a) {
    __shared__ __attribute__((aligned(16))) float Os[QT * RP];
    __shared__ __attribute__((aligned(16))) float Ws[BT * RP];
    __shared__ unsigned int hist_s[MODE == MODE_HIST ? 2 * NBIN : 1];
    __shared__ double red[MODE == MODE_HIST ? 1 : 4 * 64 * 2 + 16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const long r0 = (long)blockIdx.x * QT;
    const int n = a.n;
    const long gi = r0 + (w & 1) * 32 + l31;                         // this lane's owned row
    const bool row_ok = gi < n;

    const int t0 = blockIdx.y * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.col_tiles);

    float cx = 0.f, cy = 0.f, gxi = 0.f, gyi = 0.f;
    unsigned long long pre_lo = 0, pre_hi = 0;
    if (MODE == MODE_RBF) {
        cx = (float)(-0.5 / (a.s2x ? a.s2x[0] : a.s2_given));
        cy = (float)(-0.5 / (a.s2y ? a.s2y[0] : a.s2_given));
        gxi = a.gx[gi];
        gyi = a.gy[gi];
    }
    if (MODE == MODE_HIST) {
        gxi = a.gx[gi];
        pre_lo = a.state[ST_PREFIX_LO];
        pre_hi = a.state[ST_PREFIX_HI];
        for (int e = tid; e < 2 * NBIN; e += 256) hist_s[e] = 0u;
        __syncthreads();
    }

    double s_kl = 0., s_kk = 0., s_ll = 0., rk = 0., rl = 0.;
    for (int t = t0; t < t1; ++t) {
        const long c0 = (long)t * BT;
        if (MODE == MODE_HIST && c0 + BT - 1 <= r0) continue;        // no j > i in this tile (workgroup-uniform)
        f32x16 ak[2], al[2];
        gram_tile<ChainOrder::Halves>(a.x, n, a.p, r0, c0, Os, Ws, ak);
        if (MODE != MODE_HIST) gram_tile<ChainOrder::Halves>(a.y, n, a.q, r0, c0, Os, Ws, al);
        // gj: the walked column of register r (the C/D map of gram_tile.h)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long gj = c0 + (w >> 1) * 64 + tt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (MODE == MODE_HIST) {
                    if (!(row_ok && gj < n && gj > gi)) continue;
                    const float d = fmaxf((gxi + a.gx[gj]) - 2.f * ak[tt][r], 0.f);
                    const unsigned int bits = __float_as_uint(d);
                    if (bits == 0u) continue;
                    const unsigned long long top = (unsigned long long)bits >> a.pshift;
                    const unsigned int digit = (bits >> a.dshift) & (unsigned int)a.dmask;
                    if (top == pre_lo) atomicAdd(&hist_s[digit], 1u);
                    if (top == pre_hi) atomicAdd(&hist_s[NBIN + digit], 1u);
                } else {
                    if (!(row_ok && gj < n)) continue;
                    float kv = ak[tt][r], lv = al[tt][r];
                    if (MODE == MODE_RBF) {
                        const float dk = gj == gi ? 0.f : fmaxf((gxi + a.gx[gj]) - 2.f * kv, 0.f);
                        const float dl = gj == gi ? 0.f : fmaxf((gyi + a.gy[gj]) - 2.f * lv, 0.f);
                        kv = expf(dk * cx);
                        lv = expf(dl * cy);
                    }
                    const double kd = (double)kv, ld = (double)lv;
                    s_kl += kd * ld;
                    s_kk += kd * kd;
                    s_ll += ld * ld;
                    rk += kd;
                    rl += ld;
                }
            }
    }

    if (MODE == MODE_HIST) {
        __syncthreads();
        for (int e = tid; e < 2 * NBIN; e += 256) {
            const unsigned int c = hist_s[e];
            if (c) atomicAdd(&a.hist[e], (unsigned long long)c);
        }
        return;
    }

    // fold: a row's four partials (2 lane halves x 2 column waves) in a fixed order; S over the workgroup in a fixed order
    double* rrk = red;                 // [4 waves][64 lanes]
    double* rrl = red + 256;
    rrk[w * 64 + lane] = rk;
    rrl[w * 64 + lane] = rl;
    __syncthreads();
    if (tid < QT) {
        const int wl = tid >> 5, l = tid & 31;                       // owned row tid: waves wl and wl + 2, lanes l and l + 32
        const double k4 = ((rrk[wl * 64 + l] + rrk[wl * 64 + 32 + l]) + rrk[(wl + 2) * 64 + l]) + rrk[(wl + 2) * 64 + 32 + l];
        const double l4 = ((rrl[wl * 64 + l] + rrl[wl * 64 + 32 + l]) + rrl[(wl + 2) * 64 + l]) + rrl[(wl + 2) * 64 + 32 + l];
        a.part_rk[(long)blockIdx.y * a.n_pad + r0 + tid] = k4;
        a.part_rl[(long)blockIdx.y * a.n_pad + r0 + tid] = l4;
    }
    double* sh = red + 512;
    const double t_kl = block_sum(s_kl, sh);
    const double t_kk = block_sum(s_kk, sh);
    const double t_ll = block_sum(s_ll, sh);
    if (tid == 0) {
        double* o = a.part_s + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 4;
        o[0] = t_kl; o[1] = t_kk; o[2] = t_ll; o[3] = 0.;
    }
}

// One workgroup.  Pass 0 derives M and both ranks from the (identical) histograms; every pass picks each rank's bin, extends
// its prefix, clears the histograms; the last pass writes sigma^2 = (v_lo + v_hi) / 2 in fp64 and M.  M = 0: NaN.
__global__ __launch_bounds__(256) void cka_select_kernel(unsigned long long* __restrict__ hist, unsigned long long* __restrict__ state,
                                                         int pass, int bits, double* __restrict__ sigma2, long long* __restrict__ count) {
    __shared__ unsigned long long res[4];
    const int tid = threadIdx.x;
    if (tid < 2) {
        const unsigned long long* h = hist + tid * NBIN;
        unsigned long long rank;
        if (pass == 0) {
            unsigned long long m = 0;
            for (int b = 0; b < NBIN; ++b) m += h[b];
            if (tid == 0) state[ST_COUNT] = m;
            rank = m == 0 ? 0 : (tid == 0 ? (m - 1) / 2 : m / 2);
        } else {
            rank = state[ST_RANK_LO + tid];
        }
        unsigned long long cum = 0;
        int bin = 0;
        for (int b = 0; b < (1 << bits); ++b) {
            const unsigned long long c = h[b];
            if (rank < cum + c) { bin = b; break; }
            cum += c;
        }
        res[tid] = ((pass == 0 ? 0ull : state[ST_PREFIX_LO + tid]) << bits) | (unsigned long long)bin;
        res[2 + tid] = rank - cum;
    }
    __syncthreads();
    for (int e = tid; e < 2 * NBIN; e += 256) hist[e] = 0ull;
    if (tid < 2) {
        state[ST_PREFIX_LO + tid] = res[tid];
        state[ST_RANK_LO + tid] = res[2 + tid];
    }
    if (pass == 2 && tid == 0) {
        const unsigned long long m = state[ST_COUNT];
        const double lo = (double)__uint_as_float((unsigned int)res[0]), hi = (double)__uint_as_float((unsigned int)res[1]);
        sigma2[0] = m == 0 ? __builtin_nan("") : (lo + hi) * 0.5;
        if (count) count[0] = (long long)m;
    }
}

// Fixed-order fp64 fold of the workgroups' partials.  out = {cka, hsic_xy, hsic_xx, hsic_yy, S_kl, S_kk, S_ll, 0}.
__global__ __launch_bounds__(256) void cka_finalize_kernel(const double* __restrict__ part_rk, const double* __restrict__ part_rl,
                                                           const double* __restrict__ part_s, int n, long n_pad, int splits,
                                                           int nwg, double* __restrict__ out, double* __restrict__ rowsum_k,
                                                           double* __restrict__ rowsum_l) {
    __shared__ double sh[16];
    const int tid = threadIdx.x;
    double kl = 0., kk = 0., ll = 0., k = 0., l = 0.;
    for (long i = tid; i < n; i += 256) {
        double ki = 0., li = 0.;
        for (int s = 0; s < splits; ++s) { ki += part_rk[s * n_pad + i]; li += part_rl[s * n_pad + i]; }
        if (rowsum_k) rowsum_k[i] = ki;
        if (rowsum_l) rowsum_l[i] = li;
        kl += ki * li; kk += ki * ki; ll += li * li; k += ki; l += li;
    }
    double s_kl = 0., s_kk = 0., s_ll = 0.;
    for (int g = tid; g < nwg; g += 256) { s_kl += part_s[4L * g]; s_kk += part_s[4L * g + 1]; s_ll += part_s[4L * g + 2]; }
    kl = block_sum(kl, sh); kk = block_sum(kk, sh); ll = block_sum(ll, sh); k = block_sum(k, sh); l = block_sum(l, sh);
    s_kl = block_sum(s_kl, sh); s_kk = block_sum(s_kk, sh); s_ll = block_sum(s_ll, sh);
    if (tid == 0) {
        const double dn = (double)n, n2 = dn * dn;
        const double hxy = s_kl - 2. / dn * kl + k * l / n2;
        const double hxx = s_kk - 2. / dn * kk + k * k / n2;
        const double hyy = s_ll - 2. / dn * ll + l * l / n2;
        out[0] = hxy / sqrt(hxx * hyy);
        out[1] = hxy; out[2] = hxx; out[3] = hyy;
        out[4] = s_kl; out[5] = s_kk; out[6] = s_ll; out[7] = 0.;
    }
}

// out = x - column mean: fp64 means (32 columns x 8 row phases per workgroup, phases folded in a fixed order), one rounding.
__global__ __launch_bounds__(256) void cka_center_kernel(const float* __restrict__ x, int n, int p, float* __restrict__ out) {
    __shared__ double part[8][32];
    const int c = threadIdx.x & 31, ph = threadIdx.x >> 5;
    const long col = (long)blockIdx.x * 32 + c;
    double s = 0.;
    if (col < p)
        for (long i = ph; i < n; i += 8) s += (double)x[i * p + col];
    part[ph][c] = s;
    __syncthreads();
    double mean = 0.;
#pragma unroll
    for (int j = 0; j < 8; ++j) mean += part[j][c];
    mean /= (double)n;
    if (col < p)
        for (long i = ph; i < n; i += 8) out[i * p + col] = (float)((double)x[i * p + col] - mean);
}

}  // namespace

extern "C" int audiossl_cka_workspace(int n, int p, int q, long* bytes) {
    CkaPlan pl;
    ASSL_REQUIRE(bytes != nullptr);
    ASSL_REQUIRE(gram_width_ok(p) && gram_width_ok(q));
    ASSL_REQUIRE(cka_plan(n, pl));
    *bytes = pl.bytes;
    return ASSL_OK;
}

extern "C" int audiossl_cka_center(const float* x, int n, int p, float* out, void* stream) {
    ASSL_REQUIRE(x && out);
    ASSL_REQUIRE(n >= 2 && n <= MAX_N && gram_width_ok(p));
    if (!ASSL_ALIGNED16(x) || !ASSL_ALIGNED16(out)) return ASSL_EALIGN;
    hipLaunchKernelGGL(cka_center_kernel, dim3((unsigned)((p + 31) / 32)), dim3(256), 0, S_(stream), x, n, p, out);
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_cka_sigma2(const float* x, int n, int p, double* sigma2, long long* count, void* workspace,
                                   long workspace_bytes, void* stream) {
    CkaPlan pl;
    ASSL_REQUIRE(x && sigma2 && workspace);
    ASSL_REQUIRE(gram_width_ok(p));
    ASSL_REQUIRE(cka_plan(n, pl));
    ASSL_REQUIRE(workspace_bytes >= pl.bytes);
    if (!ASSL_ALIGNED16(x) || !ASSL_ALIGNED16(workspace)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    char* ws = static_cast<char*>(workspace);
    CkaArgs a = {};
    a.x = x;
    a.gx = reinterpret_cast<float*>(ws + pl.off_gx);
    a.hist = reinterpret_cast<unsigned long long*>(ws + pl.off_hist);
    unsigned long long* state = reinterpret_cast<unsigned long long*>(ws + pl.off_state);
    a.state = state;
    a.n = n; a.p = p; a.q = p;
    a.col_tiles = pl.col_tiles; a.tiles_per_split = pl.tiles_per_split; a.n_pad = pl.n_pad;
    ASSL_ZERO_ALWAYS(ws + pl.off_hist, (size_t)(2L * NBIN + ST_WORDS) * 8, s);      // histograms and state are adjacent
    hipLaunchKernelGGL(gram_norm_kernel<ChainOrder::Halves>, GRID1(pl.n_pad), dim3(256), 0, s, x, n, p, pl.n_pad, reinterpret_cast<float*>(ws + pl.off_gx));
    const dim3 grid((unsigned)pl.row_blocks, (unsigned)pl.splits);
    static const int dshift[3] = {21, 10, 0}, dbits[3] = {11, 11, 10}, pshift[3] = {32, 21, 10};
    for (int pass = 0; pass < 3; ++pass) {
        a.dshift = dshift[pass]; a.dmask = (1 << dbits[pass]) - 1; a.pshift = pshift[pass];
        hipLaunchKernelGGL(cka_sweep_kernel<MODE_HIST>, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(cka_select_kernel, dim3(1), dim3(256), 0, s, a.hist, state, pass, dbits[pass], sigma2, count);
    }
    ASSL_LAUNCH_CHECK();
}

extern "C" int audiossl_cka_hsic(const float* x, const float* y, int n, int p, int q, int kernel, double sigma,
                                 const double* sigma2_x, const double* sigma2_y, double* out, double* rowsum_k,
                                 double* rowsum_l, void* workspace, long workspace_bytes, void* stream) {
    CkaPlan pl;
    ASSL_REQUIRE(x && y && out && workspace);
    ASSL_REQUIRE(kernel == MODE_LINEAR || kernel == MODE_RBF);
    ASSL_REQUIRE(gram_width_ok(p) && gram_width_ok(q));
    ASSL_REQUIRE(cka_plan(n, pl));
    ASSL_REQUIRE(workspace_bytes >= pl.bytes);
    if (kernel == MODE_RBF) {
        if (sigma2_x || sigma2_y) ASSL_REQUIRE(sigma2_x && sigma2_y && sigma == 0.);
        else ASSL_REQUIRE(sigma > 0. && sigma < __builtin_inf());              // NaN fails both comparisons
    }
    if (!ASSL_ALIGNED16(x) || !ASSL_ALIGNED16(y) || !ASSL_ALIGNED16(workspace) || !ASSL_ALIGNED16(out)) return ASSL_EALIGN;
    hipStream_t s = S_(stream);
    char* ws = static_cast<char*>(workspace);
    CkaArgs a = {};
    a.x = x; a.y = y;
    a.gx = reinterpret_cast<float*>(ws + pl.off_gx);
    a.gy = reinterpret_cast<float*>(ws + pl.off_gy);
    a.s2x = sigma2_x; a.s2y = sigma2_y; a.s2_given = sigma * sigma;
    a.part_rk = reinterpret_cast<double*>(ws + pl.off_rk);
    a.part_rl = reinterpret_cast<double*>(ws + pl.off_rl);
    a.part_s = reinterpret_cast<double*>(ws + pl.off_s);
    a.n = n; a.p = p; a.q = q;
    a.col_tiles = pl.col_tiles; a.tiles_per_split = pl.tiles_per_split; a.n_pad = pl.n_pad;
    const dim3 grid((unsigned)pl.row_blocks, (unsigned)pl.splits);
    if (kernel == MODE_RBF) {
        hipLaunchKernelGGL(gram_norm_kernel<ChainOrder::Halves>, GRID1(pl.n_pad), dim3(256), 0, s, x, n, p, pl.n_pad, reinterpret_cast<float*>(ws + pl.off_gx));
        hipLaunchKernelGGL(gram_norm_kernel<ChainOrder::Halves>, GRID1(pl.n_pad), dim3(256), 0, s, y, n, q, pl.n_pad, reinterpret_cast<float*>(ws + pl.off_gy));
        hipLaunchKernelGGL(cka_sweep_kernel<MODE_RBF>, grid, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(cka_sweep_kernel<MODE_LINEAR>, grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(cka_finalize_kernel, dim3(1), dim3(256), 0, s, a.part_rk, a.part_rl, a.part_s, n, pl.n_pad, pl.splits,
                       pl.row_blocks * pl.splits, out, rowsum_k, rowsum_l);
    ASSL_LAUNCH_CHECK();
}
