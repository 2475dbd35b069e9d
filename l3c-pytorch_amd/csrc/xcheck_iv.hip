// xcheck_iv.hip -- TEST-ONLY (libl3c_hip_xcheck.so, include/l3c_xcheck_small.h): the encoder's interval head as it stood before its tile fill
// learnt 16-byte loads of the 150-channel tiles and its two production shapes became compile-time ones (csrc/dmll_kernels.hip): fill_tile
// and encode_intervals_kernel with their text unchanged, C, K and rgb run-time values, behind l3c_xcheck_dmll_encode_intervals (arguments
// and output layout: l3c_dmll_encode_intervals of include/l3c_hip.h).  tests/test_gpu_interval_head_bits.py asks the product for the same
// words.  Built with the product's flags (-ffp-contract=off) and the product's csrc/dmll_core.h.  The product never loads this.
#include "../../include/l3c_xcheck_small.h"
#include "ac_core.h"
#include "dmll_core.h"
#include "l3c_common.h"

namespace {

using l3c::sigmoid_f;
using l3c::sigmoid_sat;
using l3c::MixStats;
using l3c::MixComponent;
using l3c::mix_component_e;
using l3c::cdf_term;
using l3c::cdf_quantise;

constexpr int kMaxK = 16;

// ---- P tile -> LDS ------------------------------------------------------------------------------------------------------
// npix pixel rows of Kp floats (contiguous in memory) into tile[pixel][ld = Kp + 1] (the odd stride keeps the per-pixel column reads of
// the compute phases conflict-free).  Kp % 4 == 0 (the RGB scale: 120) and a 16-byte aligned source: one 16-byte load per four values and
// one division per load -- by multiplication with a host-made reciprocal (exact for the < 2^16 indices of a tile) -- instead of a
// 4-byte load and an integer division per value (round 5: the divisions were a quarter of the interval kernel's VALU work).
struct TileDiv {
    unsigned q4, magic;   // q4 = Kp / 4 (0: scalar fill); i / q4 == (i * magic) >> 20 for i < 65536 / ... (checked by the host)
};
static TileDiv tile_div(int Kp, int max_pix) {
    TileDiv d{0u, 0u};
#ifdef L3C_IV_SCALAR_FILL
    return d;       // (A/B builds: the scalar fill of rounds 1-4)
#endif
    if (Kp % 4 != 0) return d;
    const unsigned q = (unsigned)(Kp / 4);
    const unsigned magic = ((1u << 20) + q - 1u) / q;
    for (unsigned i = 0; i < (unsigned)max_pix * q; ++i)
        if (i / q != (unsigned)(((unsigned long long)i * magic) >> 20)) return d;   // (never for the shapes of this path; falls back to scalar)
    d.q4 = q;
    d.magic = magic;
    return d;
}
// NT threads (a compile-time constant) fill; the loads of a batch of U turns are all issued before the first value is stored, so that the
// batch pays one memory round trip (with a run-time stride the compiler keeps one load in flight per turn: the 150-channel tiles of
// the bottleneck scales then took 30 round trips, twice the time of the whole kernel before).
template <int NT>
__device__ __forceinline__ void fill_tile(float *__restrict__ tile, const float *__restrict__ src, int npix, int Kp, int ld, TileDiv dv, int tid) {
    if (dv.q4 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        constexpr int U = 4;
        const float4 *src4 = reinterpret_cast<const float4 *>(src);
        const int n4 = npix * (int)dv.q4;
        for (int i0 = tid; i0 < n4; i0 += NT * U) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * NT;
                v[u] = src4[i < n4 ? i : i0];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * NT;
                if (i < n4) {
                    const int p = (int)(((unsigned)i * dv.magic) >> 20);
                    float *dst = tile + p * ld + (i - p * (int)dv.q4) * 4;
                    dst[0] = v[u].x;
                    dst[1] = v[u].y;
                    dst[2] = v[u].z;
                    dst[3] = v[u].w;
                }
            }
        }
    } else {
        constexpr int U = 8;
        const int n = npix * Kp;
        for (int i0 = tid; i0 < n; i0 += NT * U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * NT;
                v[u] = src[i < n ? i : i0];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * NT;
                if (i < n) tile[(i / Kp) * ld + (i % Kp)] = v[u];
            }
        }
    }
}

constexpr int kHeadPix = 64;  // == interval block length, so one block writes whole 256-byte interval runs

// (Tried: kHeadPix * C threads per block -- one (pixel, channel) item per thread, no idle lanes in the compute phase: 4.4 ->
// 6.8 ms per launch at batch 128 [PMC]: fewer wavefronts per CU for the LDS-bound tile fill outweigh the busier lanes.)
template <int NT>
__global__ __launch_bounds__(NT) void encode_intervals_kernel(const float *__restrict__ P, const int16_t *__restrict__ sym,
                                                               const float *__restrict__ targets, int64_t HW, int C, int K,
                                                               int rgb, int Lp, uint32_t *__restrict__ iv, TileDiv dv) {
    extern __shared__ __attribute__((aligned(16))) float tile[];   // [kHeadPix][Kp + 1]
    const int Kp = (rgb ? 4 : 3) * C * K;
    const int ld = Kp + 1;
    const int64_t b = blockIdx.y;
    const int64_t chunk = blockIdx.x;
    const int64_t pix0 = chunk * kHeadPix;
    const int npix = (int)((HW - pix0) < kHeadPix ? (HW - pix0) : kHeadPix);
    const int tid = threadIdx.x;
    const float *src = P + (b * HW + pix0) * Kp;
    constexpr int nthreads = NT;
    fill_tile<NT>(tile, src, npix, Kp, ld, dv, tid);   // (a wavefront per pixel row instead: 4.4 -> 6.8 ms)
    __syncthreads();
    const float scale = (float)(65536 - (Lp - 1));
    const int64_t n_streams = (int64_t)gridDim.y * C;
    for (int w = tid; w < kHeadPix * C; w += nthreads) {
        const int p = w % kHeadPix, c = w / kHeadPix;
        uint32_t word0 = 0, word1 = 0;   // the stream's lane pair reads one word per role (csrc/ac_core.h: role_word)
        if (p < npix) {
            const float *px = tile + p * ld;
            auto get = [&](int ch) { return px[ch]; };
            const int64_t n = pix0 + p;
            const int x = sym[(b * C + c) * HW + n];
            float x0 = 0.f, x1 = 0.f;
            if (rgb && c > 0) {
                x0 = (float)sym[(b * C + 0) * HW + n];
                if (c > 1) x1 = (float)sym[(b * C + 1) * HW + n];
            }
            const float t_lo = targets[x];
            const float t_hi = targets[x + 1];
            // softmax statistics with the numerators kept (mix_stats' two loops, same operations in the same order)
            MixStats st;
            st.max_logit = get(c * K);
            for (int k = 1; k < K; ++k) st.max_logit = fmaxf(st.max_logit, get(c * K + k));
            float e[kMaxK];
            st.denom = 0.0f;
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) {
                e[k] = k < K ? expf(get(c * K + k) - st.max_logit) : 0.0f;
                if (k < K) st.denom = st.denom + e[k];
            }
            float acc_lo = 0.0f, acc_hi = 0.0f;
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) {
                if (k >= K) break;
                const MixComponent m = mix_component_e(get, st, e[k], C, K, rgb, c, k, x0, x1);
                const float inv = expf(-m.log_sigma);
                acc_lo = acc_lo + cdf_term(m.pi, m.mu, inv, t_lo);
                acc_hi = acc_hi + cdf_term(m.pi, m.mu, inv, t_hi);
            }
            const uint32_t c_lo = cdf_quantise(acc_lo, scale, x);
            const uint32_t c_hi = (x == Lp - 2) ? 0x10000u : cdf_quantise(acc_hi, scale, x + 1);
            word0 = l3c::role_word(c_lo, c_hi, 0);
            word1 = l3c::role_word(c_lo, c_hi, 1);
        }
        uint32_t *dst = iv + (chunk * n_streams + b * C + c) * (2 * kHeadPix) + p;
        dst[0] = word0;
        dst[kHeadPix] = word1;
    }
}

}  // namespace

extern "C" {

int l3c_xcheck_dmll_encode_intervals(const float *P, const int16_t *sym, const float *targets, int64_t B, int64_t HW, int C,
                                     int K, int rgb, int Lp, uint32_t *intervals, l3c_stream_t stream) {
    L3C_REQUIRE(P && sym && targets && intervals, "null pointer");
    L3C_REQUIRE(B > 0 && B < 65536 && HW > 0 && C > 0 && K > 0, "bad shape");
    L3C_REQUIRE(K <= kMaxK, "K out of range");
    L3C_REQUIRE(!rgb || C == 3, "lambda coupling is only defined for C == 3");
    L3C_REQUIRE(Lp >= 2 && Lp <= 65536, "Lp out of range");
    const int Kp = (rgb ? 4 : 3) * C * K;
    const size_t lds = (size_t)kHeadPix * (Kp + 1) * sizeof(float);
    L3C_REQUIRE(lds <= 64 * 1024, "Kp too large for the LDS tile");
    const dim3 grid((unsigned)((HW + kHeadPix - 1) / kHeadPix), (unsigned)B);
    // Threads per block [measured, round 5, profiles/r05_interval_kernel_threads.log, batch 32]: the bottleneck scales' 320 (pixel, channel)
    // items on 320 threads -- one each -- 1.28 ms against 1.40 ms on 256 (where a second, quarter-full turn of the compute loop follows the
    // first); the RGB scale's 192 items stay on 256 threads: 2.16 ms against 2.30 ms on 192 (the fourth wavefront idles through the compute
    // phase but helps fill the tile).
#ifdef L3C_IV_THREADS_256
    const int nthreads = 256;
#else
    const int nthreads = kHeadPix * C == 320 ? 320 : 256;
#endif
    if (nthreads == 320)
        hipLaunchKernelGGL(encode_intervals_kernel<320>, grid, dim3(320), lds, l3c::as_stream(stream), P, sym, targets, HW, C, K, rgb, Lp,
                           intervals, tile_div(Kp, kHeadPix));
    else
        hipLaunchKernelGGL(encode_intervals_kernel<256>, grid, dim3(256), lds, l3c::as_stream(stream), P, sym, targets, HW, C, K, rgb, Lp,
                           intervals, tile_div(Kp, kHeadPix));
    return l3c::check_launch("encode_intervals_kernel");
}
}
