// codec.hip -- the whole codec behind the C ABI: l3c_encode_batch / l3c_decode_batch (include/l3c_hip.h).
//
// Two host loops over entry points the library already has, in the order the Python schedule calls them:
//     encode   Bitcoding.prepare_batch + code + EncodedBatch._write_container (bitcoding/bitcoding.py): image -> l3c_net_forward -> per scale
//              the interval head -> ONE grouped coder launch -> file sizes -> l3c_container_write
//     decode   Bitcoding._walk_records: l3c_container_read -> the coarsest record on the uniform row -> per finer record
//              l3c_sym_to_bn, l3c_net_get_p, tables + range decoders (the RGB scale: the chunk pipeline) -> pixels
// so the files equal the Python path's byte for byte and either side decodes the other's.  Every buffer lives in ONE caller-owned workspace
// whose contents are garbage on entry; nothing is allocated, nothing synchronises with the host.  The framing of an untrusted file is
// parsed by the HIP-free codec_plan.h (legacy files) and codec_plan_banded.h (BANDED files).
//
// BANDED files (l3c_encode_batch_banded / l3c_decode_batch_banded: Bitcoding.code with enc.bands) go through the same two loops:
//     encode   one plan (a legacy channel is one band), one descriptor check, one front half (enc_forward) and one interval head per scale
//              (enc_intervals); enc_run and enc_banded_run keep what differs: how a scale's intervals become coder groups -- l3c_ac_band_intervals
//              cuts them into band groups -- which layout kernel sizes the files and which writer writes them
//     decode   dec_check and the walk dec_run are templates over the plan header; the three steps that differ are overloaded on it: in a banded
//              file every band of a record decodes as a stream of its own -- l3c_ac_decode_bands, the ragged launches, l3c_decode_rgb_banded
//
// Pictures that are not planar, padded or equally sized (l3c_encode_images / l3c_decode_images): the same loops -- each encode entry is
// split into its checks and its schedule for that -- behind l3c_u8_gather and in front of l3c_u8_scatter (csrc/images.hip), the planar
// frames in front of the wrapped entry's workspace.
//
// A BOX of the pictures (l3c_decode_region_plan / l3c_decode_region: Bitcoding.decode_region): the walk of dec_run ended one record early --
// the same steps, shared -- then the finest step on a row window: the picked band streams (codec_plan_region.h), l3c_net_get_p_rows, one
// l3c_decode_rgb_entries call, l3c_u8_scatter with the blob's crop table.
//
// Three small kernels of its own: the file sizes and offsets of a batch (what EncodedBatch.file_sizes sums with torch ops) for either
// format -- a thread per legacy file, a block with a wave reduction per banded file -- and int16 symbols -> uint8 pixels.
#include <string.h>

#include <exception>
#include <vector>

#include "codec_plan.h"
#include "codec_plan_banded.h"
#include "codec_plan_region.h"
#include "l3c_common.h"
#include "repair_plan.h"
#include "seal_parity_plan.h"

#define CODEC_FAIL(code, ...) (snprintf(l3c::error_buffer(), 512, __VA_ARGS__), (code))
#define CODEC_TRY(x)                        \
    do {                                    \
        const int rc_ = (int)(x);           \
        if (rc_ != L3C_OK) return rc_;      \
    } while (0)

namespace {

constexpr int64_t ALIGN = 256;
constexpr int MAX_REC = l3c_plan::MAX_RECORDS;
inline int64_t up(int64_t n) { return (n + ALIGN - 1) / ALIGN * ALIGN; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline char *base256(void *ws) { return reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(ws) + ALIGN - 1) / ALIGN * ALIGN); }

// ---- kernels -----------------------------------------------------------------------------------------------------------------

struct LayoutArgs {
    static constexpr int MAX_SCALES = 8;
    const uint32_t *nbytes[MAX_SCALES];   // [B * C] per scale, as the coder wrote them
    uint32_t *clean[MAX_SCALES];          // optional copies with L3C_AC_OVERRUN replaced by 0 (what the file writer may safely copy)
    int C[MAX_SCALES];
    int n_scales;
    int64_t B, file_stride;
    int64_t *file_offset, *file_bytes;
};

// one thread per file: 8 + sum over scales (5 + 4 C + 4) + the payload bytes; -1 when a stream of the file overran
__global__ __launch_bounds__(256) void container_layout_kernel(const LayoutArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    int64_t total = 8;
    bool overrun = false;
#pragma unroll
    for (int k = 0; k < LayoutArgs::MAX_SCALES; ++k) {
        if (k < a.n_scales) {
            const int C = a.C[k];
            total += 9 + 4 * C;
            for (int c = 0; c < C; ++c) {
                const uint32_t n = a.nbytes[k][b * C + c];
                const bool bad = n == L3C_AC_OVERRUN;
                overrun = overrun || bad;
                total += bad ? 0 : (int64_t)n;
                if (a.clean[k]) a.clean[k][b * C + c] = bad ? 0u : n;
            }
        }
    }
    a.file_offset[b] = b * a.file_stride;
    a.file_bytes[b] = overrun ? -1 : total;
}

struct BandedLayoutArgs {
    static constexpr int MAX_SCALES = 8;
    const uint32_t *nb_full[MAX_SCALES], *nb_last[MAX_SCALES];   // [B * C * (n - 1)] (null when n == 1), [B * C] per scale, as the coder wrote them
    uint32_t *clean_full[MAX_SCALES], *clean_last[MAX_SCALES];   // optional copies with L3C_AC_OVERRUN replaced by 0
    int C[MAX_SCALES];
    int64_t n[MAX_SCALES];
    int n_scales;
    int64_t framing;                                             // 14 + sum over scales (9 + 4 C n + 4)
    int64_t B, file_stride;
    int64_t *file_offset, *file_bytes;
};

// one block per file: its C (n - 1) full-band and C last-band length fields of every scale are two contiguous runs; the four wavefronts
// stride over them, then a wave reduction and one LDS step.  -1 when a band of the file overran.
__global__ __launch_bounds__(256) void container_layout_banded_kernel(const BandedLayoutArgs a) {
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    int64_t total = 0;
    int overrun = 0;
    for (int k = 0; k < a.n_scales; ++k) {
        const int64_t nf = a.C[k] * (a.n[k] - 1), nl = a.C[k];
        for (int64_t i = tid; i < nf; i += 256) {
            const uint32_t v = a.nb_full[k][b * nf + i];
            const bool bad = v == L3C_AC_OVERRUN;
            overrun |= bad ? 1 : 0;
            total += bad ? 0 : (int64_t)v;
            if (a.clean_full[k]) a.clean_full[k][b * nf + i] = bad ? 0u : v;
        }
        for (int64_t i = tid; i < nl; i += 256) {
            const uint32_t v = a.nb_last[k][b * nl + i];
            const bool bad = v == L3C_AC_OVERRUN;
            overrun |= bad ? 1 : 0;
            total += bad ? 0 : (int64_t)v;
            if (a.clean_last[k]) a.clean_last[k][b * nl + i] = bad ? 0u : v;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        total += __shfl_xor(total, d, 64);
        overrun |= __shfl_xor(overrun, d, 64);
    }
    __shared__ int64_t part[4];
    __shared__ int part_bad[4];
    if ((tid & 63) == 0) {
        part[tid >> 6] = total;
        part_bad[tid >> 6] = overrun;
    }
    __syncthreads();
    if (tid == 0) {
        a.file_offset[b] = b * a.file_stride;
        a.file_bytes[b] = (part_bad[0] | part_bad[1] | part_bad[2] | part_bad[3]) ? -1 : a.framing + part[0] + part[1] + part[2] + part[3];
    }
}

// 16 symbols per thread and step: two 16-byte loads, one 16-byte store; the last n % 16 symbols one by one
__device__ __forceinline__ uint32_t pack4(uint32_t lo, uint32_t hi) {
    return (lo & 0xffu) | ((lo >> 8) & 0xff00u) | ((hi & 0xffu) << 16) | ((hi << 8) & 0xff000000u);
}

__global__ __launch_bounds__(256) void sym_to_u8_kernel(const int16_t *__restrict__ sym, int64_t n, uint8_t *__restrict__ out) {
    const int64_t n_vec = n >> 4;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const uint4 *in4 = reinterpret_cast<const uint4 *>(sym);
    uint4 *out4 = reinterpret_cast<uint4 *>(out);
    for (int64_t i = tid; i < n_vec; i += stride) {
        const uint4 a = in4[2 * i], b = in4[2 * i + 1];
        out4[i] = make_uint4(pack4(a.x, a.y), pack4(a.z, a.w), pack4(b.x, b.y), pack4(b.z, b.w));
    }
    for (int64_t i = (n_vec << 4) + tid; i < n; i += stride) out[i] = (uint8_t)sym[i];
}

// l3c_decode_repair_round: the symbols of entry e = blockIdx.x of the table pixbase | hw | pix0 | len in the three planes of its image, two
// per store (pix0 and len are multiples of 64 but for a frame's last band, whose end is the even H W)
__global__ __launch_bounds__(256) void zero_entries_kernel(const int64_t *__restrict__ entries, int64_t S, int16_t *__restrict__ sym) {
    const int64_t e = blockIdx.x, pixbase = entries[e], hw = entries[S + e], pix0 = entries[2 * S + e], len = entries[3 * S + e];
    for (int c = 0; c < 3; ++c) {
        uint32_t *p = reinterpret_cast<uint32_t *>(sym + 3 * pixbase + c * hw + pix0);
        for (int64_t i = threadIdx.x; i < len / 2; i += 256) p[i] = 0u;
    }
}

int launch_layout(const LayoutArgs &a, l3c_stream_t stream) {
    hipLaunchKernelGGL(container_layout_kernel, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, l3c::as_stream(stream), a);
    return l3c::check_launch("container_layout_kernel");
}

int launch_layout_banded(const BandedLayoutArgs &a, l3c_stream_t stream) {
    hipLaunchKernelGGL(container_layout_banded_kernel, dim3((unsigned)a.B), dim3(256), 0, l3c::as_stream(stream), a);
    return l3c::check_launch("container_layout_banded_kernel");
}

// what l3c_container_layout and l3c_container_layout_banded ask of their arguments alike
int check_layout_args(const void *scales, int n_scales, int64_t B, int64_t file_stride, const int64_t *file_offset, const int64_t *file_bytes) {
    L3C_REQUIRE(scales && file_offset && file_bytes, "null pointer");
    L3C_REQUIRE(n_scales > 0 && n_scales <= LayoutArgs::MAX_SCALES, "1..8 scales");
    L3C_REQUIRE(B > 0 && B < 65536, "bad batch size (1 .. 65535)");
    const bool stride_ok = file_stride > 0 && file_stride % 16 == 0;
    L3C_REQUIRE(stride_ok, "file_stride must be a positive multiple of 16");
    L3C_REQUIRE(aligned16(file_offset) && aligned16(file_bytes), "every pointer must be 16-byte aligned");
    return L3C_OK;
}

// the batch of either kernel's arguments
template <class Args>
void layout_batch(Args &a, int n_scales, int64_t B, int64_t file_stride, int64_t *file_offset, int64_t *file_bytes) {
    a.n_scales = n_scales;
    a.B = B;
    a.file_stride = file_stride;
    a.file_offset = file_offset;
    a.file_bytes = file_bytes;
}

// ---- the model ---------------------------------------------------------------------------------------------------------------

int kp_of(const l3c_net_config &c, int s) {
    const int Cp = s == 0 ? 3 : c.C;
    return (Cp == 3 ? 4 : 3) * Cp * c.K;
}

// the L3C family within what the network schedule supports; the message names what is outside
int codec_config(const l3c_net_config *cfg) {
    CODEC_TRY(l3c_plan::check_config(cfg, l3c::error_buffer(), 512));
    const int64_t n = l3c_net_packed_bytes(cfg);
    return n < 0 ? (int)n : L3C_OK;
}

int check_model(const l3c_codec_model *m) {
    L3C_REQUIRE(m, "null pointer: model_host");
    CODEC_TRY(codec_config(m->cfg_host));
    L3C_REQUIRE(m->packed && m->targets_rgb && m->targets_z && m->uniform_row, "null pointer in the model");
    L3C_REQUIRE(aligned16(m->packed) && aligned16(m->targets_rgb) && aligned16(m->targets_z) && aligned16(m->uniform_row),
                "every pointer must be 16-byte aligned (model)");
    const int64_t n = l3c_net_packed_bytes(m->cfg_host);
    if (m->packed_bytes != n)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "packed_bytes %lld != l3c_net_packed_bytes %lld (packed for another config?)",
                          (long long)m->packed_bytes, (long long)n);
    return L3C_OK;
}

int check_sides(const l3c_net_config &c, int H, int W) {
    if (H <= 0 || W <= 0 || H >= 65536 || W >= 65536)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "bad shape: %d x %d, H and W must be 1 .. 65535 (u16 fields of the file)", H, W);
    if (H % (1 << c.num_scales) || W % (1 << c.num_scales))
        return CODEC_FAIL(L3C_ERR_UNSUPPORTED, "unsupported shape: %d x %d, H and W must be multiples of 2^num_scales = %d (pad first)", H, W,
                          1 << c.num_scales);
    return L3C_OK;
}

// ---- encode plans --------------------------------------------------------------------------------------------------------------

inline int64_t take(int64_t &at, int64_t n) { const int64_t o = at; at += up(n); return o; }

// The workspace of either encode.  bands == 0 is the legacy format: every channel of a scale is ONE band, the last (L = hw, n = 1), and
// the scale's intervals go to the coder from a buffer of their own (iv_l).  A banded scale's intervals go through the one buffer iv,
// from which l3c_ac_band_intervals re-lays them into the full bands' group (absent when n == 1) and the last bands' group.
struct EncPlan {
    int S;
    int Cs[MAX_REC];
    int64_t hw[MAX_REC], L[MAX_REC], n[MAX_REC], last[MAX_REC];         // per scale: band length, bands per channel, symbols of the last band
    int64_t img, sym[MAX_REC], bn_q[MAX_REC], P[MAX_REC], file_offset, zero_pad;
    int64_t nb_f[MAX_REC], nb_l[MAX_REC], clean_f[MAX_REC], clean_l[MAX_REC];
    int64_t scratch;                                                     // the forward's workspace, then the coder's buffers
    int64_t net_ws, iv, iv_f[MAX_REC], iv_l[MAX_REC], out_f[MAX_REC], out_l[MAX_REC], stride_f[MAX_REC], stride_l[MAX_REC], ac_ws, pos;
    int64_t streams_per_image, framing;                                  // (banded files)
    int64_t bytes;
};

inline int64_t band_len_of(int64_t hw, int bands) { return bands ? 64 * ((hw + 64 * (int64_t)bands - 1) / (64 * (int64_t)bands)) : hw; }

int check_bands(int bands) {
    if (bands < 1 || bands > l3c_plan::MAX_BANDS) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "bands = %d: must be 1 .. 1024", bands);
    return L3C_OK;
}

// framing (legacy: 8 + 5 + 4 C + 4 per scale, banded: 14 + 9 + 4 C n + 4 per scale) and the longest payloads, up to a multiple of 16
int64_t file_stride_of(const l3c_net_config &c, int H, int W, int bands) {
    int64_t total = bands ? 14 : 8;
    for (int s = 0; s <= c.num_scales; ++s) {
        const int64_t Cs = s == 0 ? 3 : c.C, hw = (int64_t)(H >> s) * (W >> s), L = band_len_of(hw, bands), n = (hw + L - 1) / L;
        total += (bands ? 9 : 5) + 4 * Cs * n + 4 + Cs * ((n - 1) * l3c_ac_max_bytes(L) + l3c_ac_max_bytes(hw - (n - 1) * L));
    }
    return (total + 15) / 16 * 16;
}

int enc_plan(const l3c_net_config &c, int64_t B, int H, int W, int bands, EncPlan *out) {
    EncPlan p{};
    p.S = c.num_scales;
    p.net_ws = l3c_net_forward_workspace_bytes(&c, B, H, W);     // (checks the image against the schedule's limits)
    if (p.net_ws < 0) return (int)p.net_ws;
    int64_t at = 0, coder = 0, total_streams = 0, iv_words = 0;
    int n_groups = 0;
    p.img = take(at, B * 3 * (int64_t)H * W * 4);
    p.framing = 14;
    for (int s = 0; s <= p.S; ++s) {
        p.Cs[s] = s == 0 ? 3 : c.C;
        p.hw[s] = (int64_t)(H >> s) * (W >> s);
        p.L[s] = band_len_of(p.hw[s], bands);
        p.n[s] = (p.hw[s] + p.L[s] - 1) / p.L[s];
        p.last[s] = p.hw[s] - (p.n[s] - 1) * p.L[s];
        const int64_t streams = B * p.Cs[s], n = streams * p.hw[s];
        if (bands && B * p.n[s] > l3c_plan::MAX_BAND_STREAMS)
            return CODEC_FAIL(L3C_ERR_UNSUPPORTED, "unsupported batch: %lld images x %lld bands at scale %d, more than 65535 band streams per channel "
                              "in one call: slice the batch", (long long)B, (long long)p.n[s], s);
        p.sym[s] = take(at, n * 2);
        if (s) p.bn_q[s] = take(at, n * 4);
        if (s < p.S) p.P[s] = take(at, B * p.hw[s] * kp_of(c, s) * 4);
        p.nb_f[s] = take(at, streams * (p.n[s] - 1) * 4);
        p.clean_f[s] = take(at, streams * (p.n[s] - 1) * 4);
        p.nb_l[s] = take(at, streams * 4);
        p.clean_l[s] = take(at, streams * 4);
        total_streams += streams * p.n[s];
        n_groups += p.n[s] > 1 ? 2 : 1;
        p.streams_per_image += p.Cs[s] * p.n[s];
        p.framing += 9 + 4 * p.Cs[s] * p.n[s] + 4;
        const int64_t w = l3c_interval_words(streams, p.hw[s]);
        iv_words = w > iv_words ? w : iv_words;
    }
    p.file_offset = take(at, B * 8);
    p.zero_pad = take(at, B * 8);
    p.scratch = at;
    if (bands) p.iv = take(coder, iv_words * 4);                  // one scale's intervals at a time: l3c_ac_band_intervals copies them out
    for (int s = 0; s <= p.S; ++s) {
        const int64_t streams = B * p.Cs[s];
        if (p.n[s] > 1) {
            p.iv_f[s] = take(coder, l3c_interval_words(streams * (p.n[s] - 1), p.L[s]) * 4);
            p.stride_f[s] = l3c_ac_max_bytes(p.L[s]);
            p.out_f[s] = take(coder, streams * (p.n[s] - 1) * p.stride_f[s]);
        }
        p.iv_l[s] = take(coder, l3c_interval_words(streams, p.last[s]) * 4);
        p.stride_l[s] = l3c_ac_max_bytes(p.last[s]);
        p.out_l[s] = take(coder, streams * p.stride_l[s]);
    }
    p.ac_ws = take(coder, l3c_ac_encode_groups_workspace_bytes(n_groups, total_streams));
    if (bands) p.pos = take(coder, B * p.streams_per_image * 8);
    p.bytes = p.scratch + (coder > up(p.net_ws) ? coder : up(p.net_ws)) + ALIGN;   // + ALIGN: the caller's pointer is 16-byte aligned
    *out = p;
    return L3C_OK;
}

// ---- encode: every check, then the schedule (two halves, shared with l3c_encode_images) ------------------------------------------

// the descriptor of either entry; bands is 0 for the legacy format
int enc_check_desc(const l3c_encode_batch_desc *d, bool banded, int bands, EncPlan *plan) {
    L3C_REQUIRE(d, "null descriptor");
    CODEC_TRY(check_model(d->model_host));
    const l3c_codec_model &m = *d->model_host;
    const l3c_net_config &c = *m.cfg_host;
    L3C_REQUIRE(d->img && d->files && d->file_bytes && d->workspace, "null pointer");
    L3C_REQUIRE(aligned16(d->img) && aligned16(d->padding) && aligned16(d->files) && aligned16(d->file_bytes) && aligned16(d->workspace),
                "every pointer must be 16-byte aligned");
    L3C_REQUIRE(d->B > 0 && d->B < 65536, "bad batch size (1 .. 65535)");
    CODEC_TRY(check_sides(c, d->H, d->W));
    if (banded) CODEC_TRY(check_bands(bands));
    CODEC_TRY(enc_plan(c, d->B, d->H, d->W, bands, plan));
    const int64_t stride = file_stride_of(c, d->H, d->W, bands);
    if (d->file_stride < stride || d->file_stride % 16)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "file_stride %lld: must be a multiple of 16 and at least %s = %lld", (long long)d->file_stride,
                          banded ? "l3c_encode_banded_file_stride" : "l3c_encode_file_stride", (long long)stride);
    if (d->workspace_bytes < plan->bytes)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)d->workspace_bytes, (long long)plan->bytes);
    return L3C_OK;
}

// the front half of either schedule: a padding of zeros when the caller has none, the image's symbols and floats, the whole network
int enc_forward(const l3c_encode_batch_desc *d, const EncPlan &p, char *ws, l3c_stream_t stream, l3c_net_forward_desc *out) {
    const l3c_codec_model &m = *d->model_host;
    if (!d->padding)
        CODEC_TRY(l3c::check_hip(hipMemsetAsync(ws + p.zero_pad, 0, (size_t)d->B * 8, l3c::as_stream(stream)), "hipMemsetAsync"));
    const float zero_mean[3] = {0.f, 0.f, 0.f};
    float *img = reinterpret_cast<float *>(ws + p.img);
    CODEC_TRY(l3c_u8_to_sym_bn(d->img, zero_mean, d->B, p.hw[0], reinterpret_cast<int16_t *>(ws + p.sym[0]), img, stream));
    l3c_net_forward_desc &f = *out;
    memset(&f, 0, sizeof(f));
    f.cfg_host = m.cfg_host;
    f.packed = m.packed;
    f.packed_bytes = m.packed_bytes;
    f.img = img;
    f.B = d->B;
    f.H = d->H;
    f.W = d->W;
    for (int s = 0; s <= p.S; ++s) {
        f.sym[s] = reinterpret_cast<int16_t *>(ws + p.sym[s]);
        if (s) f.bn_q[s] = reinterpret_cast<float *>(ws + p.bn_q[s]);
        if (s < p.S) f.P[s] = reinterpret_cast<float *>(ws + p.P[s]);
    }
    f.workspace = ws + p.scratch;
    f.workspace_bytes = p.net_ws;
    return l3c_net_forward(&f, stream);
}

// the intervals of scale s: the coarsest on the uniform row, every other through the mixture head
int enc_intervals(const l3c_codec_model &m, const l3c_net_forward_desc &f, const EncPlan &p, int s, uint32_t *iv, l3c_stream_t stream) {
    const l3c_net_config &c = *m.cfg_host;
    if (s == p.S) return l3c_ac_intervals_from_table(m.uniform_row, 0, c.L + 1, f.sym[s], f.B * p.Cs[s], p.hw[s], iv, stream);
    return l3c_dmll_encode_intervals(f.P[s], f.sym[s], s == 0 ? m.targets_rgb : m.targets_z, f.B, p.hw[s], p.Cs[s], c.K, s == 0,
                                     s == 0 ? 257 : c.L + 1, iv, stream);
}

int enc_run(const l3c_encode_batch_desc *d, const EncPlan &p, l3c_stream_t stream) {
    const int64_t B = d->B;
    const int S = p.S;
    char *ws = base256(d->workspace);
    l3c_net_forward_desc f;
    CODEC_TRY(enc_forward(d, p, ws, stream, &f));

    // the forward's workspace is dead: the coder's intervals and output rows take its place.  Scales coarsest first: file order.
    char *cs = ws + p.scratch;
    l3c_ac_group groups[MAX_REC];
    l3c_container_scale scales[MAX_REC];
    LayoutArgs la{};
    for (int k = 0; k <= S; ++k) {
        const int s = S - k;
        uint32_t *iv = reinterpret_cast<uint32_t *>(cs + p.iv_l[s]);
        CODEC_TRY(enc_intervals(*d->model_host, f, p, s, iv, stream));
        uint8_t *out = reinterpret_cast<uint8_t *>(cs + p.out_l[s]);
        uint32_t *nb = reinterpret_cast<uint32_t *>(ws + p.nb_l[s]), *clean = reinterpret_cast<uint32_t *>(ws + p.clean_l[s]);
        groups[k] = l3c_ac_group{iv, out, nb, B * p.Cs[s], p.hw[s], p.stride_l[s]};
        scales[k] = l3c_container_scale{out, clean, p.stride_l[s], p.Cs[s], d->H >> s, d->W >> s};
        la.nbytes[k] = nb;
        la.clean[k] = clean;
        la.C[k] = p.Cs[s];
    }
    CODEC_TRY(l3c_ac_encode_groups(groups, S + 1, cs + p.ac_ws, stream));
    // file sizes and offsets; a stream that overran (L3C_AC_OVERRUN) marks its file -1 and is written as an empty payload, so that
    // the writer below stays inside the file's slot whatever the coder reported
    layout_batch(la, S + 1, B, d->file_stride, reinterpret_cast<int64_t *>(ws + p.file_offset), d->file_bytes);
    CODEC_TRY(launch_layout(la, stream));
    const uint16_t *padding = d->padding ? d->padding : reinterpret_cast<const uint16_t *>(ws + p.zero_pad);
    return l3c_container_write(scales, S + 1, B, padding, la.file_offset, d->files, stream);
}

// scales_out (the parity entry): receives the S + 1 records the files were written from, coarsest first
int enc_banded_run(const l3c_encode_batch_desc *d, const EncPlan &p, l3c_stream_t stream, l3c_banded_scale *scales_out = nullptr) {
    const int64_t B = d->B;
    const int S = p.S;
    char *ws = base256(d->workspace);
    l3c_net_forward_desc f;
    CODEC_TRY(enc_forward(d, p, ws, stream, &f));

    // the forward's workspace is dead.  Scales coarsest first (file order): the interval head into the one interval buffer, then its bands
    // re-laid into the scale's two coder groups -- the full bands (absent when n == 1) and the last bands
    char *cs = ws + p.scratch;
    l3c_ac_group groups[2 * MAX_REC];
    l3c_banded_scale scales[MAX_REC];
    BandedLayoutArgs la{};
    int n_groups = 0;
    uint32_t *iv = reinterpret_cast<uint32_t *>(cs + p.iv);
    for (int k = 0; k <= S; ++k) {
        const int s = S - k;
        const int64_t streams = B * p.Cs[s];
        CODEC_TRY(enc_intervals(*d->model_host, f, p, s, iv, stream));
        const bool full = p.n[s] > 1;
        uint32_t *iv_f = full ? reinterpret_cast<uint32_t *>(cs + p.iv_f[s]) : nullptr, *iv_l = reinterpret_cast<uint32_t *>(cs + p.iv_l[s]);
        CODEC_TRY(l3c_ac_band_intervals(iv, streams, p.hw[s], p.L[s], iv_f, iv_l, stream));
        uint8_t *out_f = full ? reinterpret_cast<uint8_t *>(cs + p.out_f[s]) : nullptr, *out_l = reinterpret_cast<uint8_t *>(cs + p.out_l[s]);
        uint32_t *nb_f = full ? reinterpret_cast<uint32_t *>(ws + p.nb_f[s]) : nullptr, *nb_l = reinterpret_cast<uint32_t *>(ws + p.nb_l[s]);
        uint32_t *clean_f = full ? reinterpret_cast<uint32_t *>(ws + p.clean_f[s]) : nullptr, *clean_l = reinterpret_cast<uint32_t *>(ws + p.clean_l[s]);
        if (full) groups[n_groups++] = l3c_ac_group{iv_f, out_f, nb_f, streams * (p.n[s] - 1), p.L[s], p.stride_f[s]};
        groups[n_groups++] = l3c_ac_group{iv_l, out_l, nb_l, streams, p.last[s], p.stride_l[s]};
        scales[k] = l3c_banded_scale{out_f, clean_f, p.stride_f[s], out_l, clean_l, p.stride_l[s], p.Cs[s], d->H >> s, d->W >> s, p.L[s]};
        la.nb_full[k] = nb_f;
        la.nb_last[k] = nb_l;
        la.clean_full[k] = clean_f;
        la.clean_last[k] = clean_l;
        la.C[k] = p.Cs[s];
        la.n[k] = p.n[s];
    }
    CODEC_TRY(l3c_ac_encode_groups(groups, n_groups, cs + p.ac_ws, stream));
    // file sizes and offsets; a band that overran (L3C_AC_OVERRUN) marks its file -1 and is written as an empty payload, so that the
    // writer below stays inside the file's slot whatever the coder reported
    layout_batch(la, S + 1, B, d->file_stride, reinterpret_cast<int64_t *>(ws + p.file_offset), d->file_bytes);
    la.framing = p.framing;
    CODEC_TRY(launch_layout_banded(la, stream));
    const uint16_t *padding = d->padding ? d->padding : reinterpret_cast<const uint16_t *>(ws + p.zero_pad);
    if (scales_out) memcpy(scales_out, scales, sizeof(l3c_banded_scale) * (size_t)(S + 1));
    return l3c_container_write_banded(scales, S + 1, B, padding, la.file_offset, d->files, cs + p.pos, B * p.streams_per_image * 8, stream);
}

// ---- the parity-sealed banded encode (l3c_encode_batch_banded_parity): what follows enc_banded_run on the same stream ---------------------
//
// The buffers of the seal lie BEHIND the plan's workspace (p.bytes - ALIGN from its 256-byte aligned base): the coder's outputs, which the
// parity kernels read, are still live in the scratch region.  The formulas are stated in include/l3c_hip.h and decided in seal_parity_plan.h.
struct ParityPlan {
    l3c_parity_seal::Plan seal;
    int64_t max_payload[MAX_REC];       // per record, coarsest first: the longest band payload the coder can write
    int64_t tail;                       // the most bytes a seal adds to a file
    int64_t frame_crc, band_crc, crc_ws, crc_ws_bytes, slots, slot_stride, slot_nb, seal_ws;
    int64_t head_slots, head_stride, head_offset[MAX_REC], head_nb, head_crc;
    int64_t bytes;                      // the whole workspace of the entry
};

int parity_plan(const l3c_parity_opts *o, int64_t B, int H, int W, const EncPlan &p, ParityPlan *out) {
    namespace sp = l3c_parity_seal;
    ParityPlan q{};
    sp::Shape shapes[MAX_REC];
    const int S = p.S;
    for (int k = 0; k <= S; ++k) {
        const int s = S - k;
        shapes[k] = sp::Shape{p.Cs[s], H >> s, W >> s, p.L[s]};
        q.max_payload[k] = p.n[s] > 1 && p.stride_f[s] > p.stride_l[s] ? p.stride_f[s] : p.stride_l[s];
    }
    CODEC_TRY(sp::make_plan(shapes, S + 1, B, o->G, o->R, o->head, q.max_payload, &q.seal, l3c::error_buffer(), 512));
    const sp::Plan &t = q.seal;
    q.tail = sp::tail_bound(t, q.max_payload + (S + 1 - t.n_records));
    const int64_t n0 = p.n[0], m0 = t.rec[t.n_records - 1].m;
    int64_t at = p.bytes - ALIGN;
    q.frame_crc = take(at, 4 * B);
    q.band_crc = take(at, 12 * B * n0);
    q.crc_ws_bytes = l3c_u8_crc32_bands_workspace_bytes(B, 3, p.hw[0], p.L[0]);
    if (q.crc_ws_bytes < 0) return (int)q.crc_ws_bytes;
    q.crc_ws = take(at, q.crc_ws_bytes);
    q.slot_stride = sp::round16(q.max_payload[S]);
    q.slots = take(at, 3 * B * m0 * t.R * q.slot_stride);
    q.slot_nb = take(at, 12 * B * m0);
    q.seal_ws = take(at, t.ws_bytes);
    if (t.head) {
        int64_t groups = 0, fields = 0;
        for (int k = 0; k < S; ++k) q.head_stride = q.max_payload[k] > q.head_stride ? q.max_payload[k] : q.head_stride;
        q.head_stride = sp::round16(q.head_stride);
        for (int k = 0; k < S; ++k) {
            q.head_offset[k] = groups * t.R * q.head_stride;
            groups += B * t.rec[k].C * t.rec[k].m;
            fields += B * t.rec[k].C * t.rec[k].n;
        }
        q.head_slots = take(at, groups * t.R * q.head_stride);
        q.head_nb = take(at, 4 * groups);
        q.head_crc = take(at, 4 * fields);
    }
    q.bytes = at + ALIGN;
    *out = q;
    return L3C_OK;
}

// the size functions of the parity entry: the file stride (B == 0), or the workspace of a batch
int64_t parity_size(const l3c_net_config *cfg, int64_t B, int H, int W, int bands, const l3c_parity_opts *o) {
    L3C_REQUIRE(o, "null pointer: opts_host");
    CODEC_TRY(l3c_parity_seal::check_opts(o->G, o->R, o->head, o->reserved, l3c::error_buffer(), 512));
    CODEC_TRY(codec_config(cfg));
    CODEC_TRY(check_sides(*cfg, H, W));
    CODEC_TRY(check_bands(bands));
    EncPlan p;
    CODEC_TRY(enc_plan(*cfg, B ? B : 1, H, W, bands, &p));
    ParityPlan q;
    CODEC_TRY(parity_plan(o, B ? B : 1, H, W, p, &q));
    return B ? q.bytes : file_stride_of(*cfg, H, W, bands) + (q.tail + 31) / 32 * 32;
}

int enc_parity_run(const l3c_encode_batch_desc *d, const EncPlan &p, const ParityPlan &q, const l3c_parity_opts *o, l3c_stream_t stream) {
    const int64_t B = d->B;
    const int S = p.S;
    l3c_banded_scale scales[MAX_REC];
    CODEC_TRY(enc_banded_run(d, p, stream, scales));
    char *ws = base256(d->workspace);
    const l3c_parity_seal::Plan &t = q.seal;
    uint32_t *frame_crc = reinterpret_cast<uint32_t *>(ws + q.frame_crc), *band_crc = reinterpret_cast<uint32_t *>(ws + q.band_crc);
    uint8_t *slots = reinterpret_cast<uint8_t *>(ws + q.slots), *head_slots = reinterpret_cast<uint8_t *>(ws + q.head_slots);
    uint32_t *slot_nb = reinterpret_cast<uint32_t *>(ws + q.slot_nb), *head_nb = reinterpret_cast<uint32_t *>(ws + q.head_nb);
    uint32_t *head_crc = reinterpret_cast<uint32_t *>(ws + q.head_crc);
    CODEC_TRY(l3c_u8_crc32_bands(d->img, B, 3, p.hw[0], p.L[0], 3 * p.hw[0], band_crc, frame_crc, ws + q.crc_ws, q.crc_ws_bytes, stream));
    CODEC_TRY(l3c_band_parity_rs(&scales[S], B, t.rec[t.n_records - 1].G, t.R, slots, q.slot_stride, slot_nb, stream));
    if (t.head) {
        CODEC_TRY(l3c_head_parity(scales, S, B, o->G, t.R, head_slots, q.head_offset, q.head_stride, head_nb, stream));
        CODEC_TRY(l3c_band_payload_crc32(scales, S, B, head_crc, stream));
    }
    l3c_seal_parity_desc sd;
    memset(&sd, 0, sizeof(sd));
    sd.files = d->files, sd.file_stride = d->file_stride, sd.file_bytes = d->file_bytes, sd.B = B;
    sd.scales_host = scales, sd.n_scales = S + 1;
    sd.G = o->G, sd.R = o->R, sd.head = o->head;
    sd.padding = d->padding ? d->padding : reinterpret_cast<const uint16_t *>(ws + p.zero_pad);
    sd.model_id = o->model_id;
    sd.frame_crc = frame_crc, sd.band_crc = band_crc;
    sd.parity = slots, sd.parity_stride = q.slot_stride, sd.parity_nbytes = slot_nb;
    if (t.head) {
        sd.head_parity = head_slots, sd.head_parity_offset_host = q.head_offset, sd.head_parity_stride = q.head_stride;
        sd.head_parity_nbytes = head_nb, sd.payload_crc = head_crc;
    }
    sd.workspace = ws + q.seal_ws, sd.workspace_bytes = t.ws_bytes;
    return l3c_seal_append_parity(&sd, stream);
}

// ---- decode: one plan, one check and one walk over either plan header --------------------------------------------------------------

using l3c_plan::BandedHeader, l3c_plan::Header;

struct DecPlan {
    int64_t streams, sym[MAX_REC], bn, F[MAX_REC], P, flags, scratch, table_bytes[MAX_REC], getp_ws, rgb_ws;
    int64_t bytes;
};

// what differs between the two headers before the walk: the parser of the blob, the RGB record's workspace, the rule of the side stream
inline int check_blob_of(const l3c_net_config &c, const void *plan_host, int64_t cap, Header *h) {
    return l3c_plan::check_blob(c, plan_host, cap, h, l3c::error_buffer(), 512);
}
inline int check_blob_of(const l3c_net_config &c, const void *plan_host, int64_t cap, BandedHeader *h) {
    return l3c_plan::check_blob_banded(c, plan_host, cap, h, l3c::error_buffer(), 512);
}
inline int64_t rgb_ws_of(const Header &h) { return l3c_decode_rgb_workspace_bytes(h.B, h.max_chunk_npix, (int)h.n_chunks, (int)h.lag); }
inline int64_t rgb_ws_of(const BandedHeader &h) {
    return l3c_decode_rgb_banded_workspace_bytes(h.B, h.H * h.W, h.rgb_band_len, (int)h.rgb_chunks, (int)h.lag);
}
inline const char *lag_rule_of(const Header &) {
    return "a batch of 16 images or more decodes on two streams (lag 2): side_stream must be a stream of its own";
}
inline const char *lag_rule_of(const BandedHeader &) {
    return "16 bands per channel or more decode on two streams (lag 2): side_stream must be a stream of its own";
}

template <class Hdr>
int dec_plan(const l3c_net_config &c, const Hdr &h, DecPlan *out) {
    DecPlan p{};
    const int S = c.num_scales, n_rec = (int)h.n_records;
    const int64_t B = h.B, rgb_ws = rgb_ws_of(h);          // negative: a bad plan
    int64_t at = 0, scratch = 0;
    p.streams = take(at, h.dst_bytes);
    int64_t bn = 0, P = 0;
    for (int k = 0; k < n_rec; ++k) {
        const auto &r = h.rec[k];
        const int64_t hw = r.H * r.W;
        if (r.H < 1 || r.W < 1 || r.C < 1 || r.C > 8 || (k && (r.H != 2 * h.rec[k - 1].H || r.W != 2 * h.rec[k - 1].W)))
            return CODEC_FAIL(L3C_ERR_INVALID_ARG, "plan blob: inconsistent record %d", k);
        p.sym[k] = take(at, B * r.C * hw * 2);         // (the finest record's: unused when the caller takes the symbols)
        if (k + 1 < n_rec) bn = B * r.C * hw * 4 > bn ? B * r.C * hw * 4 : bn;
        if (k) {
            const int s = S - k;                       // the network that predicts this record
            const int64_t ws = l3c_net_get_p_workspace_bytes(&c, B, (int)h.rec[k - 1].H, (int)h.rec[k - 1].W);
            if (ws < 0) return (int)ws;
            p.getp_ws = ws > p.getp_ws ? ws : p.getp_ws;
            const int64_t Pk = B * hw * kp_of(c, s) * 4;
            P = Pk > P ? Pk : P;
            if (s > 0) {
                p.F[k] = take(at, B * hw * c.Cf * 4);
                p.table_bytes[k] = up(B * hw * (c.L + 1) * 2);
                scratch = r.C * p.table_bytes[k] > scratch ? r.C * p.table_bytes[k] : scratch;
            }
        }
    }
    if (h.rec[n_rec - 1].H != h.H || h.rec[n_rec - 1].W != h.W) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "plan blob: inconsistent image size");
    p.bn = take(at, bn);
    p.P = take(at, P);
    p.flags = take(at, MAX_REC * 4);
    p.rgb_ws = rgb_ws;
    if (p.rgb_ws < 0) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "plan blob: bad chunk list");
    scratch = p.getp_ws > scratch ? p.getp_ws : scratch;
    scratch = p.rgb_ws > scratch ? p.rgb_ws : scratch;
    p.scratch = at;                                    // get_p's workspace, then the scale's tables / the RGB pipeline's workspace
    p.bytes = at + up(scratch) + ALIGN;
    *out = p;
    return L3C_OK;
}

// the tail of l3c_decode_plan / l3c_decode_plan_banded: the header's sizes against the network schedule itself (the planners restate
// its limits; this is the schedule's own answer)
template <class Hdr>
int plan_recheck(const l3c_net_config &c, void *plan_host) {
    Hdr h;
    memcpy(&h, plan_host, sizeof(h));
    DecPlan p;
    if (dec_plan(c, h, &p) == L3C_OK) return L3C_OK;
    char why[400];
    snprintf(why, sizeof(why), "%s", l3c::error_buffer());
    memset(plan_host, 0, sizeof(int64_t));     // no plan
    return CODEC_FAIL(L3C_ERR_INVALID_ARG, "invalid file: %lld x %lld pixels: %s", (long long)h.H, (long long)h.W, why);
}

// a size or an offset of the decode's workspace, from the checked plan
template <class Hdr>
int64_t dec_plan_field(const l3c_net_config *cfg, const void *plan_host, int64_t DecPlan::*field) {
    CODEC_TRY(codec_config(cfg));
    Hdr h;
    CODEC_TRY(check_blob_of(*cfg, plan_host, -1, &h));
    DecPlan p;
    CODEC_TRY(dec_plan(*cfg, h, &p));
    return p.*field;
}
template <class Hdr>
int64_t dec_workspace_bytes(const l3c_net_config *cfg, const void *plan_host) {
    return dec_plan_field<Hdr>(cfg, plan_host, &DecPlan::bytes);
}

template <class Hdr>
int dec_check(const l3c_decode_batch_desc *d, l3c_stream_t main_stream, l3c_stream_t side_stream, Hdr *hdr, DecPlan *plan) {
    L3C_REQUIRE(d, "null descriptor");
    CODEC_TRY(check_model(d->model_host));
    const l3c_net_config &c = *d->model_host->cfg_host;
    L3C_REQUIRE(d->files && d->plan_host && d->plan && d->pixels && d->workspace, "null pointer");
    L3C_REQUIRE(aligned16(d->files) && aligned16(d->plan) && aligned16(d->pixels) && aligned16(d->sym) && aligned16(d->workspace),
                "every pointer must be 16-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(d->plan_host) & 7) == 0, "plan_host must be 8-byte aligned");
    Hdr &h = *hdr;
    CODEC_TRY(check_blob_of(c, d->plan_host, d->plan_bytes, &h));
    L3C_REQUIRE(h.lag == 1 || (side_stream && side_stream != main_stream), lag_rule_of(h));
    CODEC_TRY(dec_plan(c, h, plan));
    if (d->workspace_bytes < plan->bytes)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)d->workspace_bytes, (long long)plan->bytes);
    return L3C_OK;
}

// what the steps of the walk read
struct DecWalk {
    const l3c_codec_model &m;
    const l3c_net_config &c;
    const DecPlan &p;
    const char *plan, *plan_h;                 // the blob on the device and on the host
    const int64_t *dst_off;                    // of the blob: where the streams lie in `streams`, and how long they are
    const uint32_t *nbytes;
    uint8_t *streams;                          // of the workspace
    int32_t *flags;
    float *P;
    char *scratch;
    l3c_stream_t main_stream, side_stream;
    int16_t *sym[MAX_REC];
};

// the coarsest record: the uniform prior
int dec_coarsest(const DecWalk &x, const Header &h) {
    const l3c_plan::Record &r = h.rec[0];
    return l3c_ac_decode(x.m.uniform_row, 0, x.c.L + 1, x.streams, x.dst_off + r.first, x.nbytes + r.first, h.B * r.C, r.H * r.W, 1, x.sym[0], x.main_stream);
}

// ... every band of every plane in one launch
int dec_coarsest(const DecWalk &x, const BandedHeader &h) {
    const l3c_plan::BandedRecord &r = h.rec[0];
    return l3c_ac_decode_bands(x.m.uniform_row, x.c.L + 1, x.streams, x.dst_off + r.first, x.nbytes + r.first, h.B * r.C, r.H * r.W, r.L, 1, x.sym[0],
                               x.main_stream);
}

// channel ch of bottleneck record k: its table in the scratch, and the decoder part of its n_streams streams from `first` on
inline uint16_t *table_of(const DecWalk &x, int k, int ch) { return reinterpret_cast<uint16_t *>(x.scratch + ch * x.p.table_bytes[k]); }

l3c_ac_decode_part decode_part_of(const DecWalk &x, int k, int ch, int64_t first, int64_t n_streams, int64_t n_sym) {
    l3c_ac_decode_part q;
    memset(&q, 0, sizeof(q));
    q.cdf = table_of(x, k, ch);
    q.Lp = x.c.L + 1;
    q.in = x.streams;
    q.in_offsets = x.dst_off + first;
    q.in_nbytes = x.nbytes + first;
    q.n_streams = n_streams;
    q.n_sym = n_sym;
    q.not_monotone_flag = x.flags + k;
    q.final_chunk = 1;
    q.sym_out = x.sym[k];
    return q;
}

// a bottleneck record: its channels are independent given P.  get_p's workspace is dead and holds the record's tables
int dec_bottleneck(const DecWalk &x, const Header &h, int k) {
    const l3c_plan::Record &r = h.rec[k];
    const l3c_net_config &c = x.c;
    const int64_t B = h.B, hw = r.H * r.W;
    for (int c0 = 0; c0 < (int)r.C; c0 += 8) {
        const int n = (int)r.C - c0 < 8 ? (int)r.C - c0 : 8;
        l3c_table_part tp[8];
        l3c_ac_decode_part dp[8];
        for (int i = 0; i < n; ++i) {
            const int ch = c0 + i;
            tp[i] = l3c_table_part{ch, 0, hw, table_of(x, k, ch), x.flags + k, nullptr};
            l3c_ac_decode_part &q = dp[i] = decode_part_of(x, k, ch, r.first + ch * B, B, hw);
            q.sym_stride = r.C * hw;
            q.sym_offset = ch * hw;
        }
        CODEC_TRY(l3c_dmll_cdf_table_parts(x.P, nullptr, x.m.targets_z, B, hw, (int)r.C, c.K, 0, c.L + 1, tp, n, x.main_stream));
        CODEC_TRY(l3c_ac_decode_chunks(dp, n, x.main_stream));
    }
    return L3C_OK;
}

// ... every band (b, j) a ragged entry
int dec_bottleneck(const DecWalk &x, const BandedHeader &h, int k) {
    const l3c_plan::BandedRecord &r = h.rec[k];
    const l3c_net_config &c = x.c;
    const int Lp = c.L + 1;
    const int64_t B = h.B, hw = r.H * r.W;
    const int64_t E = B * r.n, max_npix = r.L < hw ? r.L : hw;
    const int64_t *ent = reinterpret_cast<const int64_t *>(x.plan + h.entries_off[k]);      // pixbase | hw | pix0 | npix | table_off
    const l3c_ragged_batch batch{E, hw, ent, ent + E};
    for (int c0 = 0; c0 < (int)r.C; c0 += 8) {
        const int n = (int)r.C - c0 < 8 ? (int)r.C - c0 : 8;
        l3c_table_part tp[8];
        l3c_ragged_part rp[8];
        l3c_ac_decode_part dp[8];
        for (int i = 0; i < n; ++i) {
            const int ch = c0 + i;
            tp[i] = l3c_table_part{ch, 0, max_npix, table_of(x, k, ch), x.flags + k, nullptr};
            rp[i] = l3c_ragged_part{ent + 2 * E, ent + 3 * E, ent + 4 * E};
            l3c_ac_decode_part &q = dp[i] = decode_part_of(x, k, ch, r.first + ch * E, E, max_npix);
            q.r_npix = ent + 3 * E;
            q.r_table_off = ent + 4 * E;
            q.r_pixbase = ent;
            q.r_hw = ent + E;
            q.r_pix0 = ent + 2 * E;
            q.r_C = (int)r.C;
            q.r_c = ch;
            q.r_table_bytes = B * hw * Lp * 2;
        }
        CODEC_TRY(l3c_dmll_cdf_table_ragged(x.P, nullptr, x.m.targets_z, &batch, (int)r.C, c.K, 0, Lp, tp, rp, n, x.main_stream));
        CODEC_TRY(l3c_ac_decode_chunks(dp, n, x.main_stream));
    }
    return L3C_OK;
}

// the RGB record: what either pipeline's descriptor says of it
template <class Desc, class Hdr>
void rgb_desc_of(const DecWalk &x, const Hdr &h, int k, Desc *out) {
    const auto &r = h.rec[k];
    Desc &q = *out;
    memset(&q, 0, sizeof(q));
    q.P = x.P;
    q.targets = x.m.targets_rgb;
    q.sym = x.sym[k];
    q.B = h.B;
    q.HW = r.H * r.W;
    q.K = x.c.K;
    q.in = x.streams;
    q.in_offsets = x.dst_off + r.first;
    q.in_nbytes = x.nbytes + r.first;
    q.lag = (int)h.lag;
    q.window_mode = 1;
    q.workspace = x.scratch;
    q.workspace_bytes = x.p.rgb_ws;
}

// the chunk pipeline
int dec_rgb(const DecWalk &x, const Header &h, int k) {
    l3c_rgb_decode_desc q;
    rgb_desc_of(x, h, k, &q);
    q.n_chunks = (int)h.n_chunks;
    q.chunk_pix0_host = reinterpret_cast<const int64_t *>(x.plan_h + h.chunk_pix0_off);
    q.chunk_npix_host = reinterpret_cast<const int64_t *>(x.plan_h + h.chunk_npix_off);
    return l3c_decode_rgb(&q, x.main_stream, h.lag == 2 ? x.side_stream : nullptr);
}

// ... over all B n bands of each channel in lock step
int dec_rgb(const DecWalk &x, const BandedHeader &h, int k) {
    l3c_rgb_banded_desc q;
    rgb_desc_of(x, h, k, &q);
    q.band_len = h.rgb_band_len;
    q.n_chunks = (int)h.rgb_chunks;
    return l3c_decode_rgb_banded(&q, x.main_stream, h.lag == 2 ? x.side_stream : nullptr);
}

// the input of the network that predicts record k: the symbols of the record above it as bottleneck values
template <class Hdr>
int dec_bn(const DecWalk &x, const Hdr &h, int k, float *bn) {
    const auto &above = h.rec[k - 1];
    return l3c_sym_to_bn(x.sym[k - 1], h.B * above.C * above.H * above.W, x.m.z_bin_width, x.m.z_x_min, bn, x.main_stream);
}

// P of record k (and, for a bottleneck record, the features the next record's decoder fuses); ws: the workspace the plan's offsets count from
template <class Hdr>
int dec_get_p(const DecWalk &x, const Hdr &h, int k, const float *bn, char *ws) {
    const auto &above = h.rec[k - 1];
    const int s = x.c.num_scales - k;
    l3c_net_get_p_desc g;
    memset(&g, 0, sizeof(g));
    g.cfg_host = &x.c;
    g.packed = x.m.packed;
    g.packed_bytes = x.m.packed_bytes;
    g.net = s;
    g.bn_q = bn;
    g.B = h.B;
    g.h = (int)above.H;
    g.w = (int)above.W;
    g.fuse = k == 1 ? nullptr : reinterpret_cast<const float *>(ws + x.p.F[k - 1]);
    g.P = x.P;
    g.F = s > 0 ? reinterpret_cast<float *>(ws + x.p.F[k]) : nullptr;      // the finest scale's features feed nothing
    g.workspace = x.scratch;
    g.workspace_bytes = x.p.getp_ws;
    return l3c_net_get_p(&g, x.main_stream);
}

// the walk over the records of a checked plan: nothing below fails on an argument
template <class Hdr>
int dec_run(const l3c_decode_batch_desc *d, const Hdr &h, const DecPlan &p, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    const l3c_codec_model &m = *d->model_host;
    const l3c_net_config &c = *m.cfg_host;
    const int64_t B = h.B;
    const int n_rec = (int)h.n_records, S = c.num_scales;
    char *ws = base256(d->workspace);
    const hipStream_t st = l3c::as_stream(main_stream);
    const char *plan = static_cast<const char *>(d->plan);
    const int64_t *src_off = reinterpret_cast<const int64_t *>(plan + h.src_off);
    DecWalk x{m, c, p, plan, static_cast<const char *>(d->plan_host), reinterpret_cast<const int64_t *>(plan + h.dst_off),
              reinterpret_cast<const uint32_t *>(plan + h.nbytes_off), reinterpret_cast<uint8_t *>(ws + p.streams),
              reinterpret_cast<int32_t *>(ws + p.flags), reinterpret_cast<float *>(ws + p.P), ws + p.scratch, main_stream, side_stream, {}};
    CODEC_TRY(l3c::check_hip(hipMemsetAsync(x.flags, 0, MAX_REC * 4, st), "hipMemsetAsync"));
    for (int k = 0; k < n_rec; ++k)
        for (int64_t a = h.rec[k].first, e = a + h.rec[k].n_streams; a < e; a += 65535) {
            const int64_t n = e - a < 65535 ? e - a : 65535;
            CODEC_TRY(l3c_container_read(d->files, src_off + a, x.dst_off + a, x.nbytes + a, n, (uint32_t)h.rec[k].max_nbytes, x.streams, main_stream));
        }
    for (int k = 0; k < n_rec; ++k) x.sym[k] = reinterpret_cast<int16_t *>(ws + p.sym[k]);
    if (d->sym) x.sym[n_rec - 1] = d->sym;
    float *bn = reinterpret_cast<float *>(ws + p.bn);
    CODEC_TRY(dec_coarsest(x, h));
    for (int k = 1; k < n_rec; ++k) {
        const auto &r = h.rec[k];
        const int s = S - k;
        CODEC_TRY(dec_bn(x, h, k, bn));
        CODEC_TRY(dec_get_p(x, h, k, bn, ws));
        // P is complete: get_p's workspace is dead and holds this record's tables / the RGB pipeline's workspace from here on
        if (s == 0) CODEC_TRY(l3c::check_hip(hipMemsetAsync(x.sym[k], 0, (size_t)(B * 3 * r.H * r.W * 2), st), "hipMemsetAsync"));
        CODEC_TRY(s > 0 ? dec_bottleneck(x, h, k) : dec_rgb(x, h, k));
    }
    return l3c_sym_to_u8(x.sym[n_rec - 1], B * 3 * h.H * h.W, d->pixels, main_stream);
}

template <class Hdr>
int dec_batch(const l3c_decode_batch_desc *d, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    Hdr h;
    DecPlan p;
    CODEC_TRY(dec_check(d, main_stream, side_stream, &h, &p));
    return dec_run(d, h, p, main_stream, side_stream);     // everything checked: enqueue
}

// which of the two decoders reads a plan blob (its first word), and the batch and padded image size it was made for: the checked header's
int plan_dims(const l3c_net_config &c, const void *plan_host, int64_t plan_bytes, bool *banded, int64_t *B, int64_t *H, int64_t *W) {
    L3C_REQUIRE(plan_host, "null pointer: plan_host");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(plan_host) & 7) == 0, "plan_host must be 8-byte aligned");
    int64_t magic;
    memcpy(&magic, plan_host, sizeof(magic));
    *banded = magic == l3c_plan::BANDED_MAGIC;
    auto dims = [&](auto h) {
        CODEC_TRY(check_blob_of(c, plan_host, plan_bytes, &h));
        *B = h.B, *H = h.H, *W = h.W;
        return (int)L3C_OK;
    };
    return *banded ? dims(BandedHeader{}) : dims(Header{});
}

// ---- region decode: the walk ended one record early, then the finest step on a row window (codec_plan_region.h) ---------------------------

using l3c_plan::RegionHeader;

struct RegPlan {
    DecPlan p;          // what the shared steps of the walk read: the coarser records' streams, symbols, features and tables, bn, P, flags, scratch
    int64_t coarse_bytes, picked, sym_win, u8_win, rows_ws, entries_ws;
};

template <class Hdr>
int reg_plan(const l3c_net_config &c, const Hdr &h, const RegionHeader &g, const void *plan_host, const void *region_host, RegPlan *out) {
    RegPlan q{};
    DecPlan &p = q.p;
    const int S = c.num_scales, n_rec = (int)h.n_records;
    const int64_t B = h.B;
    // the stream buffer of the walk ends where the finest record's streams would begin
    q.coarse_bytes = reinterpret_cast<const int64_t *>(static_cast<const char *>(plan_host) + h.dst_off)[h.rec[n_rec - 1].first];
    if (q.coarse_bytes < 0 || q.coarse_bytes > h.dst_bytes) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "plan blob: inconsistent stream offsets");
    int64_t at = 0, scratch = 0, bn = 0, P = 0;
    p.streams = take(at, q.coarse_bytes);
    q.picked = take(at, g.dst_bytes);
    for (int k = 0; k < n_rec - 1; ++k) {
        const auto &r = h.rec[k];
        const int64_t hw = r.H * r.W;
        if (r.H < 1 || r.W < 1 || r.H >= 65536 || r.W >= 65536 || r.C < 1 || r.C > 8 || (k && (r.H != 2 * h.rec[k - 1].H || r.W != 2 * h.rec[k - 1].W)))
            return CODEC_FAIL(L3C_ERR_INVALID_ARG, "plan blob: inconsistent record %d", k);
        p.sym[k] = take(at, B * r.C * hw * 2);
        bn = B * r.C * hw * 4 > bn ? B * r.C * hw * 4 : bn;
        if (k) {
            const int64_t ws = l3c_net_get_p_workspace_bytes(&c, B, (int)h.rec[k - 1].H, (int)h.rec[k - 1].W);
            if (ws < 0) return (int)ws;
            p.getp_ws = ws > p.getp_ws ? ws : p.getp_ws;
            const int64_t Pk = B * hw * kp_of(c, S - k) * 4;
            P = Pk > P ? Pk : P;
            p.F[k] = take(at, B * hw * c.Cf * 4);
            p.table_bytes[k] = up(B * hw * (c.L + 1) * 2);
            scratch = r.C * p.table_bytes[k] > scratch ? r.C * p.table_bytes[k] : scratch;
        }
    }
    const auto &above = h.rec[n_rec - 2];
    if (g.H != 2 * above.H || g.W != 2 * above.W) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "plan blob: inconsistent image size");
    const int64_t rows = g.rows.c1 - g.rows.c0;
    q.rows_ws = l3c_net_get_p_rows_workspace_bytes(&c, B, (int)above.H, (int)above.W, (int)g.rows.c0, (int)g.rows.c1);
    if (q.rows_ws < 0) return (int)q.rows_ws;
    const int64_t Pw = B * rows * g.W * kp_of(c, 0) * 4;
    P = Pw > P ? Pw : P;
    q.entries_ws = l3c_decode_rgb_entries_workspace_bytes(g.S, reinterpret_cast<const int64_t *>(static_cast<const char *>(region_host) + g.entries_off) + 3 * g.S,
                                                          (int)g.n_chunks, (int)g.lag);
    if (q.entries_ws < 0) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "region blob: bad entry table");
    p.bn = take(at, bn);
    p.P = take(at, P);
    q.sym_win = take(at, B * 3 * rows * g.W * 2);
    q.u8_win = take(at, B * 3 * rows * g.W);
    p.flags = take(at, MAX_REC * 4);
    scratch = p.getp_ws > scratch ? p.getp_ws : scratch;
    scratch = q.rows_ws > scratch ? q.rows_ws : scratch;
    scratch = q.entries_ws > scratch ? q.entries_ws : scratch;
    p.scratch = at;
    p.bytes = at + up(scratch) + ALIGN;
    *out = q;
    return L3C_OK;
}

// both blobs, each against its own rules and the region blob against the plan blob; then the plan of the workspace
template <class Hdr>
int reg_blobs(const l3c_net_config &c, const void *plan_host, int64_t plan_bytes, const void *region_host, int64_t region_bytes, Hdr *h,
              RegionHeader *g, RegPlan *q) {
    CODEC_TRY(l3c_plan::region_config(&c, l3c::error_buffer(), 512));
    L3C_REQUIRE(plan_host && region_host, "null pointer: plan_host / region_host");
    L3C_REQUIRE(((reinterpret_cast<uintptr_t>(plan_host) | reinterpret_cast<uintptr_t>(region_host)) & 7) == 0, "plan_host and region_host must be 8-byte aligned");
    CODEC_TRY(check_blob_of(c, plan_host, plan_bytes, h));
    CODEC_TRY(l3c_plan::region_check(c, plan_host, plan_bytes, region_host, region_bytes, g, l3c::error_buffer(), 512));
    return reg_plan(c, *h, *g, plan_host, region_host, q);
}

template <class Hdr>
int reg_run(const l3c_decode_region_desc *d, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    L3C_REQUIRE(d, "null descriptor");
    CODEC_TRY(check_model(d->model_host));
    const l3c_codec_model &m = *d->model_host;
    const l3c_net_config &c = *m.cfg_host;
    L3C_REQUIRE(d->files && d->plan_host && d->plan && d->region_host && d->region && d->pixels && d->workspace, "null pointer");
    L3C_REQUIRE(aligned16(d->files) && aligned16(d->plan) && aligned16(d->region) && aligned16(d->pixels) && aligned16(d->workspace),
                "every pointer must be 16-byte aligned");
    Hdr h;
    RegionHeader g;
    RegPlan q;
    CODEC_TRY(reg_blobs(c, d->plan_host, d->plan_bytes, d->region_host, d->region_bytes, &h, &g, &q));
    L3C_REQUIRE(g.lag == 1 || (side_stream && side_stream != main_stream),
                "16 entries or more decode on two streams (lag 2): side_stream must be a stream of its own");
    const DecPlan &p = q.p;
    if (d->workspace_bytes < p.bytes)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)d->workspace_bytes, (long long)p.bytes);
    const int64_t B = h.B, W = g.W, rows = g.rows.c1 - g.rows.c0, S = g.S;
    const int64_t box_bytes = B * 3 * (g.box[1] - g.box[0]) * (g.box[3] - g.box[2]);
    const char *region = static_cast<const char *>(d->region), *region_h = static_cast<const char *>(d->region_host);
    const l3c_u8_image *crop = reinterpret_cast<const l3c_u8_image *>(region + g.crop_off);
    const l3c_u8_image *crop_h = reinterpret_cast<const l3c_u8_image *>(region_h + g.crop_off);
    CODEC_TRY(l3c::images_check(crop_h, crop, B, (int)rows, (int)W, box_bytes));

    // ---- everything checked: enqueue.  The walk of dec_run over every record but the finest ...
    const int n_rec = (int)h.n_records;
    char *ws = base256(d->workspace);
    const hipStream_t st = l3c::as_stream(main_stream);
    const char *plan = static_cast<const char *>(d->plan);
    const int64_t *src_off = reinterpret_cast<const int64_t *>(plan + h.src_off);
    DecWalk x{m, c, p, plan, static_cast<const char *>(d->plan_host), reinterpret_cast<const int64_t *>(plan + h.dst_off),
              reinterpret_cast<const uint32_t *>(plan + h.nbytes_off), reinterpret_cast<uint8_t *>(ws + p.streams),
              reinterpret_cast<int32_t *>(ws + p.flags), reinterpret_cast<float *>(ws + p.P), ws + p.scratch, main_stream, side_stream, {}};
    CODEC_TRY(l3c::check_hip(hipMemsetAsync(x.flags, 0, MAX_REC * 4, st), "hipMemsetAsync"));
    for (int k = 0; k < n_rec - 1; ++k)
        for (int64_t a = h.rec[k].first, e = a + h.rec[k].n_streams; a < e; a += 65535) {
            const int64_t n = e - a < 65535 ? e - a : 65535;
            CODEC_TRY(l3c_container_read(d->files, src_off + a, x.dst_off + a, x.nbytes + a, n, (uint32_t)h.rec[k].max_nbytes, x.streams, main_stream));
        }
    for (int k = 0; k < n_rec - 1; ++k) x.sym[k] = reinterpret_cast<int16_t *>(ws + p.sym[k]);
    float *bn = reinterpret_cast<float *>(ws + p.bn);
    CODEC_TRY(dec_coarsest(x, h));
    for (int k = 1; k < n_rec - 1; ++k) {
        CODEC_TRY(dec_bn(x, h, k, bn));
        CODEC_TRY(dec_get_p(x, h, k, bn, ws));
        CODEC_TRY(dec_bottleneck(x, h, k));
    }

    // ... and the finest step on the window: the picked streams, P of the conv rows, ONE entries call, the box out of the window frames
    const int64_t *pk_src = reinterpret_cast<const int64_t *>(region + g.src_off), *pk_dst = reinterpret_cast<const int64_t *>(region + g.dst_off);
    const uint32_t *pk_nbytes = reinterpret_cast<const uint32_t *>(region + g.nbytes_off);
    uint8_t *picked = reinterpret_cast<uint8_t *>(ws + q.picked);
    for (int64_t a = 0; a < 3 * S; a += 65535) {
        const int64_t n = 3 * S - a < 65535 ? 3 * S - a : 65535;
        CODEC_TRY(l3c_container_read(d->files, pk_src + a, pk_dst + a, pk_nbytes + a, n, (uint32_t)g.max_nbytes, picked, main_stream));
    }
    const auto &above = h.rec[n_rec - 2];
    CODEC_TRY(dec_bn(x, h, n_rec - 1, bn));
    l3c_net_get_p_rows_desc w;
    memset(&w, 0, sizeof(w));
    w.cfg_host = &c;
    w.packed = m.packed;
    w.packed_bytes = m.packed_bytes;
    w.net = 0;
    w.bn_q = bn;
    w.B = B;
    w.h = (int)above.H;
    w.w = (int)above.W;
    w.fuse = reinterpret_cast<const float *>(ws + p.F[n_rec - 2]);
    w.c0 = (int)g.rows.c0;
    w.c1 = (int)g.rows.c1;
    w.P = x.P;
    w.workspace = x.scratch;
    w.workspace_bytes = q.rows_ws;
    CODEC_TRY(l3c_net_get_p_rows(&w, main_stream));
    int16_t *sym = reinterpret_cast<int16_t *>(ws + q.sym_win);
    CODEC_TRY(l3c::check_hip(hipMemsetAsync(sym, 0, (size_t)(B * 3 * rows * W * 2), st), "hipMemsetAsync"));
    l3c_rgb_entries_desc e;
    memset(&e, 0, sizeof(e));
    e.P = x.P;
    e.targets = m.targets_rgb;
    e.sym = sym;
    e.S = S;
    e.total_pix = B * rows * W;
    e.entries_dev = reinterpret_cast<const int64_t *>(region + g.entries_off);
    e.entries_host = reinterpret_cast<const int64_t *>(region_h + g.entries_off);
    e.K = c.K;
    e.in = picked;
    e.in_offsets = pk_dst;
    e.in_nbytes = pk_nbytes;
    e.n_chunks = (int)g.n_chunks;
    e.lag = (int)g.lag;
    e.window_mode = 1;
    e.workspace = x.scratch;          // P is complete: get_p_rows' workspace is dead
    e.workspace_bytes = q.entries_ws;
    CODEC_TRY(l3c_decode_rgb_entries(&e, main_stream, g.lag == 2 ? side_stream : nullptr));
    uint8_t *u8 = reinterpret_cast<uint8_t *>(ws + q.u8_win);
    CODEC_TRY(l3c_sym_to_u8(sym, B * 3 * rows * W, u8, main_stream));
    return l3c_u8_scatter(u8, B, (int)rows, (int)W, d->pixels, box_bytes, crop_h, crop, main_stream);
}

// which walk reads a plan blob
int plan_is_banded(const void *plan_host, bool *banded) {
    L3C_REQUIRE(plan_host, "null pointer: plan_host");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(plan_host) & 7) == 0, "plan_host must be 8-byte aligned");
    int64_t magic;
    memcpy(&magic, plan_host, sizeof(magic));
    *banded = magic == l3c_plan::BANDED_MAGIC;
    return L3C_OK;
}

template <class Hdr>
int64_t reg_workspace_bytes(const l3c_net_config &c, const void *plan_host, const void *region_host) {
    Hdr h;
    RegionHeader g;
    RegPlan q;
    CODEC_TRY(reg_blobs(c, plan_host, -1, region_host, -1, &h, &g, &q));
    return q.p.bytes;
}

// the size functions of an encode (bands 0: legacy): the file stride, or the workspace of a batch
int64_t enc_size(const l3c_net_config *cfg, int64_t B, int H, int W, bool banded, int bands, bool workspace) {
    CODEC_TRY(codec_config(cfg));
    CODEC_TRY(check_sides(*cfg, H, W));
    if (banded) CODEC_TRY(check_bands(bands));
    if (!workspace) return file_stride_of(*cfg, H, W, bands);
    EncPlan p;
    CODEC_TRY(enc_plan(*cfg, B, H, W, bands, &p));
    return p.bytes;
}

}  // namespace

extern "C" {

int l3c_container_layout(const l3c_container_scale *scales, int n_scales, int64_t B, int64_t file_stride, int64_t *file_offset,
                         int64_t *file_bytes, l3c_stream_t stream) {
    CODEC_TRY(check_layout_args(scales, n_scales, B, file_stride, file_offset, file_bytes));
    LayoutArgs a{};
    layout_batch(a, n_scales, B, file_stride, file_offset, file_bytes);
    for (int k = 0; k < n_scales; ++k) {
        L3C_REQUIRE(scales[k].nbytes && scales[k].C > 0 && scales[k].C < 256, "bad scale descriptor");
        L3C_REQUIRE((reinterpret_cast<uintptr_t>(scales[k].nbytes) & 3) == 0, "nbytes arrays must be 4-byte aligned");
        a.nbytes[k] = scales[k].nbytes;
        a.C[k] = scales[k].C;
    }
    return launch_layout(a, stream);
}

int l3c_container_layout_banded(const l3c_banded_scale *scales, int n_scales, int64_t B, int64_t file_stride, int64_t *file_offset,
                                int64_t *file_bytes, l3c_stream_t stream) {
    CODEC_TRY(check_layout_args(scales, n_scales, B, file_stride, file_offset, file_bytes));
    BandedLayoutArgs a{};
    layout_batch(a, n_scales, B, file_stride, file_offset, file_bytes);
    a.framing = 14;
    for (int k = 0; k < n_scales; ++k) {
        const l3c_banded_scale &q = scales[k];
        L3C_REQUIRE(q.C > 0 && q.C < 256 && q.H > 0 && q.H < 65536 && q.W > 0 && q.W < 65536, "bad scale descriptor (C < 256, H and W fit u16)");
        L3C_REQUIRE(q.band_len >= 64 && q.band_len % 64 == 0, "band_len must be a positive multiple of 64");
        const int64_t n = ((int64_t)q.H * q.W + q.band_len - 1) / q.band_len;
        L3C_REQUIRE(n <= l3c_plan::MAX_BANDS, "more than 1024 bands per channel");
        L3C_REQUIRE(q.nbytes_last && (n == 1 || q.nbytes_full), "bad scale descriptor (null nbytes array)");
        L3C_REQUIRE(((reinterpret_cast<uintptr_t>(q.nbytes_last) | (n == 1 ? 0 : reinterpret_cast<uintptr_t>(q.nbytes_full))) & 3) == 0,
                    "nbytes arrays must be 4-byte aligned");
        a.nb_full[k] = n == 1 ? nullptr : q.nbytes_full;
        a.nb_last[k] = q.nbytes_last;
        a.C[k] = q.C;
        a.n[k] = n;
        a.framing += 9 + 4 * q.C * n + 4;
    }
    return launch_layout_banded(a, stream);
}

int l3c_sym_to_u8(const int16_t *sym, int64_t n, uint8_t *out, l3c_stream_t stream) {
    L3C_REQUIRE(sym && out, "null pointer");
    L3C_REQUIRE(n > 0, "empty input");
    L3C_REQUIRE(aligned16(sym) && aligned16(out), "every pointer must be 16-byte aligned");
    const int64_t blocks = ((n >> 4) + 255) / 256;
    hipLaunchKernelGGL(sym_to_u8_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks))), dim3(256), 0,
                       l3c::as_stream(stream), sym, n, out);
    return l3c::check_launch("sym_to_u8_kernel");
}

int64_t l3c_encode_file_stride(const l3c_net_config *cfg, int H, int W) { return enc_size(cfg, 0, H, W, false, 0, false); }

int64_t l3c_encode_batch_workspace_bytes(const l3c_net_config *cfg, int64_t B, int H, int W) { return enc_size(cfg, B, H, W, false, 0, true); }

int l3c_encode_batch(const l3c_encode_batch_desc *d, l3c_stream_t stream) {
    EncPlan p;
    CODEC_TRY(enc_check_desc(d, false, 0, &p));
    return enc_run(d, p, stream);     // everything checked: enqueue
}

int64_t l3c_decode_plan_bytes(const l3c_net_config *cfg, int64_t B) {
    CODEC_TRY(codec_config(cfg));
    if (B < 1 || B >= 65536) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "bad batch size: B = %lld, must be 1 .. 65535", (long long)B);
    return l3c_plan::plan_bytes(*cfg, B);
}

int l3c_decode_plan(const l3c_net_config *cfg, const uint8_t *files_host, const int64_t *file_offset_host, int64_t B, void *plan_host,
                    int64_t plan_bytes, int *H_out, int *W_out, uint16_t *padding_host_out) {
    CODEC_TRY(codec_config(cfg));
    CODEC_TRY(l3c_plan::make_plan(cfg, files_host, file_offset_host, B, plan_host, plan_bytes, H_out, W_out, padding_host_out,
                                  l3c::error_buffer(), 512));
    return plan_recheck<Header>(*cfg, plan_host);
}

int64_t l3c_decode_batch_workspace_bytes(const l3c_net_config *cfg, const void *plan_host) { return dec_workspace_bytes<Header>(cfg, plan_host); }

int l3c_decode_batch(const l3c_decode_batch_desc *d, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    return dec_batch<Header>(d, main_stream, side_stream);
}

// ---- banded files ------------------------------------------------------------------------------------------------------------

int64_t l3c_encode_banded_file_stride(const l3c_net_config *cfg, int H, int W, int bands) { return enc_size(cfg, 0, H, W, true, bands, false); }

int64_t l3c_encode_batch_banded_workspace_bytes(const l3c_net_config *cfg, int64_t B, int H, int W, int bands) {
    return enc_size(cfg, B, H, W, true, bands, true);
}

int l3c_encode_batch_banded(const l3c_encode_batch_desc *d, int bands, l3c_stream_t stream) {
    EncPlan p;
    CODEC_TRY(enc_check_desc(d, true, bands, &p));
    return enc_banded_run(d, p, stream);     // everything checked: enqueue
}

int64_t l3c_encode_banded_parity_file_stride(const l3c_net_config *cfg, int H, int W, int bands, const l3c_parity_opts *opts_host) {
    return parity_size(cfg, 0, H, W, bands, opts_host);
}

int64_t l3c_encode_batch_banded_parity_workspace_bytes(const l3c_net_config *cfg, int64_t B, int H, int W, int bands,
                                                       const l3c_parity_opts *opts_host) {
    if (B < 1 || B >= 65536) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "bad batch size: B = %lld, must be 1 .. 65535", (long long)B);
    return parity_size(cfg, B, H, W, bands, opts_host);
}

int l3c_encode_batch_banded_parity(const l3c_encode_batch_desc *d, int bands, const l3c_parity_opts *o, l3c_stream_t stream) {
    L3C_REQUIRE(d, "null descriptor");
    L3C_REQUIRE(o, "null pointer: opts_host");
    CODEC_TRY(l3c_parity_seal::check_opts(o->G, o->R, o->head, o->reserved, l3c::error_buffer(), 512));
    EncPlan p;
    CODEC_TRY(enc_check_desc(d, true, bands, &p));
    ParityPlan q;
    CODEC_TRY(parity_plan(o, d->B, d->H, d->W, p, &q));
    const int64_t stride = file_stride_of(*d->model_host->cfg_host, d->H, d->W, bands) + (q.tail + 31) / 32 * 32;
    if (d->file_stride < stride)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "file_stride %lld: must be at least l3c_encode_banded_parity_file_stride = %lld",
                          (long long)d->file_stride, (long long)stride);
    if (d->workspace_bytes < q.bytes)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)d->workspace_bytes, (long long)q.bytes);
    return enc_parity_run(d, p, q, o, stream);     // everything checked: enqueue
}

int64_t l3c_decode_plan_banded_bytes(const l3c_net_config *cfg, const uint8_t *files_host, const int64_t *file_offset_host, int64_t B) {
    CODEC_TRY(codec_config(cfg));
    return l3c_plan::plan_banded_bytes(cfg, files_host, file_offset_host, B, l3c::error_buffer(), 512);
}

int l3c_decode_plan_banded(const l3c_net_config *cfg, const uint8_t *files_host, const int64_t *file_offset_host, int64_t B, void *plan_host,
                           int64_t plan_bytes, int *H_out, int *W_out, uint16_t *padding_host_out) {
    CODEC_TRY(codec_config(cfg));
    CODEC_TRY(l3c_plan::make_plan_banded(cfg, files_host, file_offset_host, B, plan_host, plan_bytes, H_out, W_out, padding_host_out,
                                         l3c::error_buffer(), 512));
    return plan_recheck<BandedHeader>(*cfg, plan_host);
}

int64_t l3c_decode_batch_banded_workspace_bytes(const l3c_net_config *cfg, const void *plan_host) {
    return dec_workspace_bytes<BandedHeader>(cfg, plan_host);
}

// (every record's P goes to the one P area, coarse to fine: the finest record's is what a finished decode leaves there)
int64_t l3c_decode_batch_banded_p_offset(const l3c_net_config *cfg, const void *plan_host) {
    return dec_plan_field<BandedHeader>(cfg, plan_host, &DecPlan::P);
}

// (the stream area is the first thing in the workspace; the accessor below says where a stream lies inside it)
int64_t l3c_decode_batch_banded_streams_offset(const l3c_net_config *cfg, const void *plan_host) {
    return dec_plan_field<BandedHeader>(cfg, plan_host, &DecPlan::streams);
}

int l3c_decode_plan_banded_stream(const void *plan_host, int record, int64_t index, int64_t *src_offset_out, int64_t *dst_offset_out,
                                  uint32_t *nbytes_out) {
    return l3c_plan::banded_stream(plan_host, record, index, src_offset_out, dst_offset_out, nbytes_out, l3c::error_buffer(), 512);
}

int l3c_decode_batch_banded(const l3c_decode_batch_desc *d, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    return dec_batch<BandedHeader>(d, main_stream, side_stream);
}

// ---- repair of parity-sealed files: the planner of a round (csrc/repair_plan.h) and the round on the device ----------------------------------

int l3c_repair_coefficients(const int32_t *erased, int t, int r0, const int32_t *present, int n_present, uint8_t *rows_out, uint8_t *members_out) {
    L3C_REQUIRE(erased && rows_out && (n_present == 0 || (present && members_out)), "null pointer");
    L3C_REQUIRE(t >= 1 && t <= l3c_repair::MAX_T && r0 >= 0 && r0 <= l3c_repair::MAX_T - t && n_present >= 0, "t must be in 1..4, r0 in 0..4 - t");
    int64_t ks[l3c_repair::MAX_T];
    for (int e = 0; e < t; ++e) {
        L3C_REQUIRE(erased[e] >= 0 && erased[e] < l3c_sealing::MAX_RS_GROUP, "members must be in 0..254");
        ks[e] = erased[e];
    }
    for (int p = 0; p < n_present; ++p) {
        L3C_REQUIRE(present[p] >= 0 && present[p] < l3c_sealing::MAX_RS_GROUP, "members must be in 0..254");
        for (int e = 0; e < t; ++e) L3C_REQUIRE(present[p] != erased[e], "a member is erased or present, not both");
    }
    uint8_t inv[l3c_repair::MAX_T][l3c_repair::MAX_T];
    if (!l3c_repair::rs_invert(ks, t, r0, inv)) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "singular system: the erased members must be distinct");
    for (int e = 0; e < t; ++e) {
        for (int i = 0; i < t; ++i) rows_out[e * t + i] = inv[e][i];
        for (int p = 0; p < n_present; ++p) members_out[e * n_present + p] = l3c_repair::rs_member_weight(inv, e, t, r0, present[p]);
    }
    return L3C_OK;
}

int64_t l3c_repair_round_plan_bytes(const l3c_net_config *cfg, const void *plan_host) {
    CODEC_TRY(codec_config(cfg));
    BandedHeader h;
    CODEC_TRY(check_blob_of(*cfg, plan_host, -1, &h));
    return l3c_repair::round_bytes_bound(h);
}

int l3c_repair_round_plan(const l3c_net_config *cfg, const void *plan_host, const uint8_t *const *files_host, const int64_t *file_bytes_host,
                          const uint32_t *band_words_host, const int64_t *section_at_host, const l3c_repair_group *tried_host, int64_t n_tried,
                          void *round_host, int64_t round_bytes, int64_t *n_groups_out) {
    L3C_REQUIRE(n_groups_out, "null pointer: n_groups_out");
    CODEC_TRY(codec_config(cfg));
    CODEC_TRY(l3c_repair::make_round_plan(cfg, plan_host, files_host, file_bytes_host, band_words_host, section_at_host, tried_host, n_tried, round_host,
                                          round_bytes, l3c::error_buffer(), 512));
    *n_groups_out = static_cast<const l3c_repair::RoundHeader *>(round_host)->n_groups;
    return L3C_OK;
}

int l3c_repair_round_groups(const void *round_host, const l3c_repair_group **groups_out, int64_t *n_groups_out, const int32_t **positions_out,
                            int64_t *n_positions_out) {
    L3C_REQUIRE(round_host && groups_out && n_groups_out && positions_out && n_positions_out, "null pointer");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(round_host) & 7) == 0, "round_host must be 8-byte aligned");
    l3c_repair::RoundHeader h, want;
    memcpy(&h, round_host, sizeof(h));
    L3C_REQUIRE(h.magic == l3c_repair::ROUND_MAGIC, "round blob: wrong magic word (not written by l3c_repair_round_plan)");
    L3C_REQUIRE(h.B >= 1 && h.B < 65536 && h.n_groups >= 0 && h.n_groups <= 65535 && h.S >= 0 && h.S <= 65535 && h.n_src >= 0 &&
                    h.n_src <= l3c_repair::MAX_BANDS * 65535,
                "round blob: inconsistent header");
    want = h;
    l3c_repair::round_layout(want);
    L3C_REQUIRE(memcmp(&want, &h, sizeof(h)) == 0, "round blob: inconsistent header");
    const char *blob = static_cast<const char *>(round_host);
    *groups_out = reinterpret_cast<const l3c_repair_group *>(blob + h.groups_off);
    *n_groups_out = h.n_groups;
    *positions_out = reinterpret_cast<const int32_t *>(blob + h.pos_off);
    *n_positions_out = h.S;
    return L3C_OK;
}

namespace {

struct RoundPlan {
    BandedHeader h;
    DecPlan p;
    l3c_repair::RoundHeader r;
    int64_t entries_ws, crc_ws, bytes;
};

// both blobs -- the round blob's header against the plan; with `check` everything that follows from its groups, made again and compared --
// and the plan of the round's workspace
int round_blobs(const l3c_net_config *cfg, const void *plan_host, const void *round_host, int64_t round_bytes, bool check, RoundPlan *q) {
    CODEC_TRY(codec_config(cfg));
    L3C_REQUIRE(plan_host && round_host, "null pointer: plan_host / round_host");
    L3C_REQUIRE(((reinterpret_cast<uintptr_t>(plan_host) | reinterpret_cast<uintptr_t>(round_host)) & 7) == 0, "plan_host and round_host must be 8-byte aligned");
    CODEC_TRY(check_blob_of(*cfg, plan_host, -1, &q->h));
    CODEC_TRY(dec_plan(*cfg, q->h, &q->p));
    CODEC_TRY(l3c_repair::round_check(*cfg, q->h, plan_host, round_host, round_bytes, &q->r, nullptr, 0, l3c::error_buffer(), 512));
    if (check) {
        std::vector<int64_t> again;
        try {
            again.resize((size_t)(q->r.bytes + 7) / 8);
        } catch (const std::exception &) {
            return CODEC_FAIL(L3C_ERR_INVALID_ARG, "no host memory to check a round blob of %lld bytes", (long long)q->r.bytes);
        }
        CODEC_TRY(l3c_repair::round_check(*cfg, q->h, plan_host, round_host, round_bytes, &q->r, reinterpret_cast<uint8_t *>(again.data()), q->r.bytes,
                                          l3c::error_buffer(), 512));
    }
    const l3c_repair::RoundHeader &r = q->r;
    q->entries_ws = q->crc_ws = 0;
    if (r.n_groups > 0) {
        const char *blob = static_cast<const char *>(round_host);
        L3C_REQUIRE(r.S >= 1 && r.S < 65536, "round blob: 1 .. 65535 positions");
        q->entries_ws = l3c_decode_rgb_entries_workspace_bytes(r.S, reinterpret_cast<const int64_t *>(blob + r.entries_off) + 3 * r.S, (int)r.n_chunks, (int)r.lag);
        if (q->entries_ws < 0) return CODEC_FAIL(L3C_ERR_INVALID_ARG, "round blob: bad entry table");
        q->crc_ws = l3c_u8_crc32_spans_workspace_bytes(reinterpret_cast<const l3c_u8_span *>(blob + r.crc_off), 3 * r.S);
        if (q->crc_ws < 0) return (int)q->crc_ws;
    }
    q->bytes = up(q->entries_ws) + up(q->crc_ws) + ALIGN;
    return L3C_OK;
}

}  // namespace

int64_t l3c_decode_repair_round_workspace_bytes(const l3c_net_config *cfg, const void *plan_host, const void *round_host) {
    RoundPlan q;
    CODEC_TRY(round_blobs(cfg, plan_host, round_host, -1, false, &q));
    return q.bytes;
}

int l3c_decode_repair_round(const l3c_decode_repair_round_desc *d, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    L3C_REQUIRE(d, "null descriptor");
    CODEC_TRY(check_model(d->model_host));
    const l3c_codec_model &m = *d->model_host;
    const l3c_net_config &c = *m.cfg_host;
    L3C_REQUIRE(d->round && d->rows && d->workspace && d->sym && d->pixels && d->crc_out && d->round_workspace, "null pointer");
    L3C_REQUIRE(aligned16(d->round) && aligned16(d->workspace) && aligned16(d->sym) && aligned16(d->pixels) && aligned16(d->crc_out) &&
                    aligned16(d->round_workspace),
                "every pointer but rows must be 16-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(d->rows) & 3) == 0 && d->rows_bytes >= 0, "rows must be 4-byte aligned, rows_bytes not negative");
    RoundPlan q;
    CODEC_TRY(round_blobs(&c, d->plan_host, d->round_host, d->round_bytes, true, &q));
    const l3c_repair::RoundHeader &r = q.r;
    if (d->workspace_bytes < q.p.bytes)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld (the decode's workspace)", (long long)d->workspace_bytes,
                          (long long)q.p.bytes);
    if (d->round_workspace_bytes < q.bytes)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "round_workspace_bytes too small: %lld < %lld", (long long)d->round_workspace_bytes, (long long)q.bytes);
    if (r.n_groups == 0) return L3C_OK;                            // nothing left to try
    L3C_REQUIRE(r.lag == 1 || (side_stream && side_stream != main_stream),
                "16 positions or more decode on two streams (lag 2): side_stream must be a stream of its own");
    L3C_REQUIRE(r.HW % 2 == 0, "an odd number of pixels per plane");
    const int64_t B = r.B, HW = r.HW, S = r.S;
    const char *blob = static_cast<const char *>(d->round), *blob_h = static_cast<const char *>(d->round_host);
    char *ws = base256(d->workspace), *rws = base256(d->round_workspace);
    uint8_t *streams = reinterpret_cast<uint8_t *>(ws + q.p.streams);

    // ---- everything the blobs say is checked; the calls below check their own tables (the row spans among them) before they launch
    CODEC_TRY(l3c_band_rebuild(d->rows, d->rows_bytes, streams, r.dst_bytes, reinterpret_cast<const l3c_u8_span *>(blob_h + r.src_off),
                               reinterpret_cast<const l3c_u8_span *>(blob + r.src_off), reinterpret_cast<const uint8_t *>(blob_h + r.coef_off),
                               reinterpret_cast<const uint8_t *>(blob + r.coef_off), r.n_src,
                               reinterpret_cast<const l3c_rebuild_group *>(blob_h + r.rebuild_off),
                               reinterpret_cast<const l3c_rebuild_group *>(blob + r.rebuild_off), r.n_groups, main_stream));
    const int64_t *entries = reinterpret_cast<const int64_t *>(blob + r.entries_off);
    hipLaunchKernelGGL(zero_entries_kernel, dim3((unsigned)S), dim3(256), 0, l3c::as_stream(main_stream), entries, S, d->sym);
    CODEC_TRY(l3c::check_launch("zero_entries_kernel"));
    l3c_rgb_entries_desc e;
    memset(&e, 0, sizeof(e));
    e.P = reinterpret_cast<const float *>(ws + q.p.P);
    e.targets = m.targets_rgb;
    e.sym = d->sym;
    e.S = S;
    e.total_pix = B * HW;
    e.entries_dev = entries;
    e.entries_host = reinterpret_cast<const int64_t *>(blob_h + r.entries_off);
    e.K = c.K;
    e.in = streams;
    e.in_offsets = reinterpret_cast<const int64_t *>(blob + r.in_off);
    e.in_nbytes = reinterpret_cast<const uint32_t *>(blob + r.in_nbytes_off);
    e.n_chunks = (int)r.n_chunks;
    e.lag = (int)r.lag;
    e.window_mode = 1;
    e.workspace = rws;
    e.workspace_bytes = q.entries_ws;
    CODEC_TRY(l3c_decode_rgb_entries(&e, main_stream, r.lag == 2 ? side_stream : nullptr));
    CODEC_TRY(l3c_sym_to_u8(d->sym, B * 3 * HW, d->pixels, main_stream));
    return l3c_u8_crc32_spans(d->pixels, B * 3 * HW, reinterpret_cast<const l3c_u8_span *>(blob_h + r.crc_off),
                              reinterpret_cast<const l3c_u8_span *>(blob + r.crc_off), 3 * S, d->crc_out, rws + up(q.entries_ws), q.crc_ws, main_stream);
}

// ---- pictures as they come: a table of views, padded and cropped on the device (csrc/images.hip) -----------------------------------
//
// Both calls put the planar frames in front of the workspace of the entry they wrap:  frames [B][3][Hp][Wp] | padding uint16 [B][4]
// (encode) | the wrapped entry's workspace.  + ALIGN: the caller's pointer is 16-byte aligned, the frames start at the next multiple of 256.

int64_t l3c_encode_images_workspace_bytes(const l3c_net_config *cfg, int64_t B, int Hp, int Wp, int bands) {
    const int64_t inner = bands ? l3c_encode_batch_banded_workspace_bytes(cfg, B, Hp, Wp, bands) : l3c_encode_batch_workspace_bytes(cfg, B, Hp, Wp);
    if (inner < 0) return inner;
    return up(B * 3 * (int64_t)Hp * Wp) + up(B * 8) + inner + ALIGN;
}

int l3c_encode_images(const l3c_encode_images_desc *d, l3c_stream_t stream) {
    L3C_REQUIRE(d, "null descriptor");
    CODEC_TRY(check_model(d->model_host));
    const l3c_net_config &c = *d->model_host->cfg_host;
    L3C_REQUIRE(d->src && d->images_host && d->images && d->files && d->file_bytes && d->workspace, "null pointer");
    L3C_REQUIRE(aligned16(d->images) && aligned16(d->files) && aligned16(d->file_bytes) && aligned16(d->workspace),
                "every pointer but src must be 16-byte aligned");
    L3C_REQUIRE(d->B > 0 && d->B < 65536, "bad batch size (1 .. 65535)");
    CODEC_TRY(check_sides(c, d->Hp, d->Wp));
    if (d->bands) CODEC_TRY(check_bands(d->bands));
    const int64_t need = l3c_encode_images_workspace_bytes(&c, d->B, d->Hp, d->Wp, d->bands);
    if (need < 0) return (int)need;
    if (d->workspace_bytes < need)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)d->workspace_bytes, (long long)need);
    char *ws = base256(d->workspace);
    const int64_t frames = up(d->B * 3 * (int64_t)d->Hp * d->Wp), head = frames + up(d->B * 8);
    uint8_t *img = reinterpret_cast<uint8_t *>(ws);
    uint16_t *padding = reinterpret_cast<uint16_t *>(ws + frames);
    l3c_encode_batch_desc e;
    memset(&e, 0, sizeof(e));
    e.model_host = d->model_host;
    e.img = img;
    e.B = d->B;
    e.H = d->Hp;
    e.W = d->Wp;
    e.padding = padding;
    e.files = d->files;
    e.file_stride = d->file_stride;
    e.file_bytes = d->file_bytes;
    e.workspace = ws + head;
    e.workspace_bytes = d->workspace_bytes - head - (ws - static_cast<char *>(d->workspace));
    EncPlan p;
    CODEC_TRY(enc_check_desc(&e, d->bands != 0, d->bands, &p));
    CODEC_TRY(l3c::images_check(d->images_host, d->images, d->B, d->Hp, d->Wp, d->src_bytes));

    // ---- everything checked: enqueue
    CODEC_TRY(l3c_u8_gather(d->src, d->src_bytes, d->images_host, d->images, d->B, d->Hp, d->Wp, img, padding, stream));
    return d->bands ? enc_banded_run(&e, p, stream) : enc_run(&e, p, stream);
}

int64_t l3c_decode_images_workspace_bytes(const l3c_net_config *cfg, const void *plan_host) {
    CODEC_TRY(codec_config(cfg));
    bool banded;
    int64_t B, H, W;
    CODEC_TRY(plan_dims(*cfg, plan_host, -1, &banded, &B, &H, &W));
    const int64_t inner = banded ? l3c_decode_batch_banded_workspace_bytes(cfg, plan_host) : l3c_decode_batch_workspace_bytes(cfg, plan_host);
    if (inner < 0) return inner;
    return up(B * 3 * H * W) + inner + ALIGN;
}

int l3c_decode_images(const l3c_decode_images_desc *d, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    L3C_REQUIRE(d, "null descriptor");
    CODEC_TRY(check_model(d->model_host));
    const l3c_net_config &c = *d->model_host->cfg_host;
    L3C_REQUIRE(d->files && d->plan_host && d->plan && d->dst && d->images_host && d->images && d->workspace, "null pointer");
    L3C_REQUIRE(aligned16(d->files) && aligned16(d->plan) && aligned16(d->images) && aligned16(d->sym) && aligned16(d->workspace),
                "every pointer but dst must be 16-byte aligned");
    bool banded;
    int64_t B, H, W;
    CODEC_TRY(plan_dims(c, d->plan_host, d->plan_bytes, &banded, &B, &H, &W));
    const int64_t need = l3c_decode_images_workspace_bytes(&c, d->plan_host);
    if (need < 0) return (int)need;
    if (d->workspace_bytes < need)
        return CODEC_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)d->workspace_bytes, (long long)need);
    CODEC_TRY(l3c::images_check(d->images_host, d->images, B, (int)H, (int)W, d->dst_bytes));
    char *ws = base256(d->workspace);
    const int64_t head = up(B * 3 * H * W);
    l3c_decode_batch_desc q;
    memset(&q, 0, sizeof(q));
    q.model_host = d->model_host;
    q.files = d->files;
    q.plan_host = d->plan_host;
    q.plan = d->plan;
    q.plan_bytes = d->plan_bytes;
    q.pixels = reinterpret_cast<uint8_t *>(ws);
    q.sym = d->sym;
    q.workspace = ws + head;
    q.workspace_bytes = d->workspace_bytes - head - (ws - static_cast<char *>(d->workspace));
    // the wrapped entry checks its own arguments (the side stream among them) before it enqueues anything, the scatter's are checked above
    CODEC_TRY(banded ? l3c_decode_batch_banded(&q, main_stream, side_stream) : l3c_decode_batch(&q, main_stream, side_stream));
    return l3c_u8_scatter(q.pixels, B, (int)H, (int)W, d->dst, d->dst_bytes, d->images_host, d->images, main_stream);
}

// ---- region decode -----------------------------------------------------------------------------------------------------------

int64_t l3c_decode_region_plan_bytes(const l3c_net_config *cfg, const void *plan_host) {
    CODEC_TRY(codec_config(cfg));
    return l3c_plan::region_plan_bytes(cfg, plan_host, l3c::error_buffer(), 512);
}

int l3c_decode_region_plan(const l3c_net_config *cfg, const void *plan_host, int64_t plan_bytes, const uint16_t *padding_host,
                           const l3c_region_box *box_host, void *region_host, int64_t region_bytes, l3c_region_info *info_out) {
    CODEC_TRY(codec_config(cfg));
    return l3c_plan::make_region_plan(cfg, plan_host, plan_bytes, padding_host, box_host, region_host, region_bytes, info_out, l3c::error_buffer(),
                                      512);
}

int64_t l3c_decode_region_workspace_bytes(const l3c_net_config *cfg, const void *plan_host, const void *region_host) {
    CODEC_TRY(codec_config(cfg));
    bool banded;
    CODEC_TRY(plan_is_banded(plan_host, &banded));
    return banded ? reg_workspace_bytes<BandedHeader>(*cfg, plan_host, region_host) : reg_workspace_bytes<Header>(*cfg, plan_host, region_host);
}

int l3c_decode_region(const l3c_decode_region_desc *d, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    L3C_REQUIRE(d, "null descriptor");
    bool banded;
    CODEC_TRY(plan_is_banded(d->plan_host, &banded));
    return banded ? reg_run<BandedHeader>(d, main_stream, side_stream) : reg_run<Header>(d, main_stream, side_stream);
}
}
