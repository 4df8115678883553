// f3: packed integer PCM -> the float32 [B][unit] window batch the front ends consume, gfx950.
//
// Replaces the host half of the reference's clip loading: the sample conversion and channel mean inside
// `librosa.core.load` (`src/dataset/upstream_dataset.py:55`) / `torchaudio.load` (`extras/mast_new/mast/dataloader.py:101`), and the
// placement of the clip in its training window (`src/utils/utils.py:166-182`: random crop, or centre zero padding; the fbank batch
// pads on the right).  The host only cuts each clip at its drawn start and ships the frames in the file's own sample format, so a
// 16-bit batch crosses PCIe at half the bytes of the float32 one; this kernel writes the float32 rows.
//
// Arithmetic is the host decoder's, bit for bit: u8 (x - 128) / 128, s16 x / 2^15, s32 float(x) (nearest even) / 2^31 - all exact
// scalings by a power of two - and f32 untouched; several channels are added in float32 in numpy's `mean(axis=1)` order and the sum
// is DIVIDED by C (a reciprocal multiply differs for C = 3, 5, 6, 7).  numpy's order is first to last for C <= 7; at C = 8 its
// unrolled pairwise sum applies, ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)), and so does it here.
//
// One workgroup row per clip (grid.y = B), no LDS, no atomics.  The hot rows - mono s16 with unit % 4 == 0 - stream: a lane
// owns 8 output samples = 16 source bytes.  The clip's offset and its left padding shift those bytes against the 16-byte grid
// by an even amount that is the same for the whole row, so a lane reads the two ALIGNED 16-byte chunks its bytes straddle (one
// when the row happens to be aligned; the neighbour's copy of the shared chunk comes from L1) and funnel-shifts them into place
// with a wave-uniform dword rotation plus a 0- or 2-byte v_alignbit.  Chunks are read only where they intersect the clip, and
// the packed buffer is 16-byte aligned with a multiple of 16 bytes, so no read leaves it.  Two 16-byte stores per lane.
// Every other row (other formats, several channels, unit % 4 != 0) takes one natural-width load per channel sample and
// stores 4 (unit % 4 == 0) or 1 float per lane.
// HBM roofline of a mono s16 batch: 2 n bytes read + 4 unit bytes written per clip.
#include "common.h"

namespace {

enum { PCM_U8 = 0, PCM_S16 = 1, PCM_S32 = 2, PCM_F32 = 3 };
constexpr int PCM_THREADS = 256;
constexpr int PCM_MAX_CH = 8;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

__host__ __device__ __forceinline__ int pcm_sample_bytes(int fmt) { return fmt == PCM_U8 ? 1 : fmt == PCM_S16 ? 2 : 4; }

template <int FMT> struct PcmType;
template <> struct PcmType<PCM_U8> { typedef unsigned char T; };
template <> struct PcmType<PCM_S16> { typedef short T; };
template <> struct PcmType<PCM_S32> { typedef int T; };
template <> struct PcmType<PCM_F32> { typedef float T; };

template <int FMT>
__device__ __forceinline__ float pcm_sample(typename PcmType<FMT>::T x) {
    if (FMT == PCM_U8) return ((float)x - 128.f) * 0.0078125f;
    if (FMT == PCM_S16) return (float)x * 0x1p-15f;
    if (FMT == PCM_S32) return (float)x * 0x1p-31f;            // v_cvt_f32_i32 rounds to nearest even
    return (float)x;
}

// frame j of a clip: the channel mean in numpy's order
template <int FMT>
__device__ __forceinline__ float pcm_frame(const unsigned char* clip, long j, int C) {
    const typename PcmType<FMT>::T* p = reinterpret_cast<const typename PcmType<FMT>::T*>(clip) + j * C;
    float s = pcm_sample<FMT>(p[0]);
    if (C == 1) return s;
    if (C == PCM_MAX_CH) {
        const float s1 = pcm_sample<FMT>(p[1]), s2 = pcm_sample<FMT>(p[2]), s3 = pcm_sample<FMT>(p[3]), s4 = pcm_sample<FMT>(p[4]),
                    s5 = pcm_sample<FMT>(p[5]), s6 = pcm_sample<FMT>(p[6]), s7 = pcm_sample<FMT>(p[7]);
        s = ((s + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
    } else {
        for (int c = 1; c < C; ++c) s += pcm_sample<FMT>(p[c]);
    }
    return __fdiv_rn(s, (float)C);
}

// V consecutive output samples of a row, one natural-width load per channel sample
template <int FMT, int V>
__device__ __forceinline__ void pcm_general(const unsigned char* clip, float* row, long o, int left, int n, int C) {
    float y[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const long j = o + k - left;
        y[k] = (j >= 0 && j < n) ? pcm_frame<FMT>(clip, j, C) : 0.f;
    }
    if (V == 4) *reinterpret_cast<f32x4*>(row + o) = f32x4{y[0], y[V > 1 ? 1 : 0], y[V > 2 ? 2 : 0], y[V > 3 ? 3 : 0]};
    else row[o] = y[0];
}

// 16 bytes at buffer offset c (a multiple of 16), zeros when the chunk does not touch the clip's bytes [lo, hi)
__device__ __forceinline__ u32x4 pcm_chunk(const unsigned char* pcm, long long c, long long lo, long long hi) {
    if (c + 16 > lo && c < hi) return *reinterpret_cast<const u32x4*>(pcm + c);
    return u32x4{0u, 0u, 0u, 0u};
}

// WIDE: unit % 4 == 0, every row of `out` starts on a 16-byte boundary
template <bool WIDE>
__global__ __launch_bounds__(PCM_THREADS) void pcm_window_kernel(const unsigned char* __restrict__ pcm, const long long* __restrict__ tab,
                                                                 float* __restrict__ out, int unit, int align) {
    const int b = blockIdx.y;
    const long long off = tab[4 * b];
    const int n = (int)tab[4 * b + 1], C = (int)tab[4 * b + 2], fmt = (int)tab[4 * b + 3];
    const int left = align == 0 ? (unit - n) >> 1 : 0;        // n <= unit was checked on the host
    float* const row = out + (long)b * unit;
    const int g = blockIdx.x * PCM_THREADS + threadIdx.x;

    if (WIDE && fmt == PCM_S16 && C == 1) {
        const int o = 8 * g;
        if (o >= unit) return;
        f32x4 y0 = {0.f, 0.f, 0.f, 0.f}, y1 = y0;
        if (o + 8 > left && o < left + n) {
            const long long a = off + 2ll * (o - left);       // first source byte of this lane; may lie before the clip
            const long long a0 = a & ~15ll;
            const int sh = (int)(a & 15);                     // the same for every lane of the row
            const long long hi = off + 2ll * n;
            const u32x4 c0 = pcm_chunk(pcm, a0, off, hi);
            u32x4 c1 = {0u, 0u, 0u, 0u};
            if (sh) c1 = pcm_chunk(pcm, a0 + 16, off, hi);
            // bytes sh .. sh + 15 of the 32-byte pair: a dword rotation in two conditional steps (static register indices), then
            // a 0- or 2-byte funnel shift
            unsigned int w[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
            if (sh & 8) {
#pragma unroll
                for (int i = 0; i < 6; ++i) w[i] = w[i + 2];
            }
            if (sh & 4) {
#pragma unroll
                for (int i = 0; i < 5; ++i) w[i] = w[i + 1];
            }
            unsigned int r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = (sh & 2) ? __builtin_amdgcn_alignbyte(w[k + 1], w[k], 2) : w[k];
            float y[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                y[2 * k] = (float)(short)(r[k] & 0xffffu) * 0x1p-15f;
                y[2 * k + 1] = (float)((int)r[k] >> 16) * 0x1p-15f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (o + k < left || o + k >= left + n) y[k] = 0.f;
            y0 = f32x4{y[0], y[1], y[2], y[3]};
            y1 = f32x4{y[4], y[5], y[6], y[7]};
        }
        *reinterpret_cast<f32x4*>(row + o) = y0;
        if (o + 4 < unit) *reinterpret_cast<f32x4*>(row + o + 4) = y1;
        return;
    }

    constexpr int V = WIDE ? 4 : 1;
    const long o = (long)V * g;
    if (o >= unit) return;
    const unsigned char* clip = pcm + off;
    switch (fmt) {                                            // uniform over the row
        case PCM_U8: pcm_general<PCM_U8, V>(clip, row, o, left, n, C); break;
        case PCM_S16: pcm_general<PCM_S16, V>(clip, row, o, left, n, C); break;
        case PCM_S32: pcm_general<PCM_S32, V>(clip, row, o, left, n, C); break;
        default: pcm_general<PCM_F32, V>(clip, row, o, left, n, C); break;
    }
}

}  // namespace

extern "C" int audiossl_pcm_window(const void* pcm, long pcm_bytes, const long long* tab, const long long* tab_host, float* out,
                                   int B, int unit, int align, void* stream) {
    ASSL_REQUIRE(pcm && tab && tab_host && out);
    ASSL_REQUIRE(B > 0 && B <= 65535 && unit > 0 && unit <= (1 << 30) && pcm_bytes >= 0);
    ASSL_REQUIRE(align == 0 || align == 1);
    bool hot = true;                                          // every row is mono s16
    for (int b = 0; b < B; ++b) {
        const long long* q = tab_host + 4 * b;
        const long long off = q[0], n = q[1], C = q[2], fmt = q[3];
        ASSL_REQUIRE(fmt >= PCM_U8 && fmt <= PCM_F32);
        ASSL_REQUIRE(C >= 1 && C <= PCM_MAX_CH);
        ASSL_REQUIRE(n >= 0 && n <= unit);
        const int sz = pcm_sample_bytes((int)fmt);
        ASSL_REQUIRE(off >= 0 && off % sz == 0 && off <= (long long)pcm_bytes);
        ASSL_REQUIRE(n * C * sz <= (long long)pcm_bytes - off);
        hot &= fmt == PCM_S16 && C == 1;
    }
    if (!ASSL_ALIGNED16(pcm) || !ASSL_ALIGNED16(out) || (pcm_bytes & 15)) return ASSL_EALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned char* p = static_cast<const unsigned char*>(pcm);
    if (unit % 4 == 0) {
        // 8 samples per lane when every row streams; a mixed batch is launched at the general rows' 4 per lane (its mono s16
        // rows then leave the upper half of their lanes idle)
        const dim3 g(ceil_div(unit, (hot ? 8 : 4) * PCM_THREADS), B);
        hipLaunchKernelGGL(pcm_window_kernel<true>, g, dim3(PCM_THREADS), 0, s, p, tab, out, unit, align);
    } else {
        const dim3 g(ceil_div(unit, PCM_THREADS), B);
        hipLaunchKernelGGL(pcm_window_kernel<false>, g, dim3(PCM_THREADS), 0, s, p, tab, out, unit, align);
    }
    ASSL_LAUNCH_CHECK();
}
