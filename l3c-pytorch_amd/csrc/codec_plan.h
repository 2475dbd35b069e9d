// codec_plan.h -- the validating parser of the legacy `.l3c` framing and the decode plan it writes (include/l3c_hip.h: l3c_decode_plan).
//
// Plain C++17 on purpose: no HIP include, no library call, no allocation -- the way ac_core.h serves the host simulation -- so that the
// half of the decoder that reads UNTRUSTED bytes compiles into a stand-alone program (tests/cabi/plan_check_main.cpp, built with the
// address and undefined-behaviour sanitizers) as well as into libl3c_hip.so (csrc/codec.hip).
//
// The format (bitcoding/container.py; reference bitcoding.py:326-375), little-endian:
//     u16 x4 padding | for scale = coarsest .. 0:  u8 C, u16 H, u16 W | per channel: u32 nbytes, payload | 46 E2 84 92
// What is rejected is what the Python readers reject before their first upload: container.parse_containers / count_scale_records
// (framing), Bitcoding._n_predicted (record count), _check_coarsest and _check_header (the shapes the decoder kernels will index with).
//
// THE PLAN BLOB: int64 words throughout.  A Header, then at the byte offsets it names
//     src_offset int64 [n_streams] | dst_offset int64 [n_streams] | nbytes uint32 [n_streams] | chunk_pix0 int64 [n_chunks] | chunk_npix int64 [n_chunks]
// Streams are numbered record after record, coarsest first; inside the coarsest record stream (b, c) is b * C + c (what the uniform-prior
// decoder writes as [B][C][h][w]), inside every other record c * B + b (a channel's B streams adjacent: bitcoding/upload.py).
// src_offset is the payload's byte position inside the caller's file buffer, dst_offset its position in the stream buffer the decoder
// reads: a multiple of 4, ((nbytes + 3) / 4) * 4 + 4 bytes per stream, back to back in stream order.
#ifndef L3C_CODEC_PLAN_H_
#define L3C_CODEC_PLAN_H_

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/l3c_hip.h"

namespace l3c_plan {

constexpr int64_t MAGIC = 0x4e414c505f43334cll;   // the bytes "L3C_PLAN"
constexpr int MAX_RECORDS = L3C_NET_MAX_SCALES + 1;
constexpr int MAX_CHUNKS = 34;                    // 2 probes + 32 chunks
constexpr int64_t RGB_PROBE = 1024, RGB_CHUNKS = 32;

struct Record {
    int64_t C, H, W;           // the record's header
    int64_t first, n_streams;  // its streams: [first, first + n_streams) of the blob's arrays
    int64_t max_nbytes;        // the longest of them
};

struct Header {
    int64_t magic, bytes;      // MAGIC; size of the blob
    int64_t B, n_records;
    int64_t H, W;              // the (padded) image: the finest record's
    int64_t n_streams;         // over all records
    int64_t files_bytes;       // file_offset[B]: the file buffer the src offsets point into
    int64_t dst_bytes;         // size of the stream buffer
    int64_t n_chunks, max_chunk_npix, lag;   // the RGB chunk pipeline
    int64_t cfg[9];            // the l3c_net_config the plan was made for
    int64_t src_off, dst_off, nbytes_off, chunk_pix0_off, chunk_npix_off;   // byte offsets of the arrays inside the blob
    Record rec[MAX_RECORDS];
};

inline int fail(char *err, size_t cap, int code, const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    if (err && cap) snprintf(err, cap, fmt, a, b, c, d);
    return code;
}

inline void cfg_words(const l3c_net_config &c, int64_t *w) {
    const int v[9] = {c.num_scales, c.Cf, c.C, c.L, c.K, c.enc_blocks, c.dec_blocks, c.rgb_baseline, c.dec_skip};
    for (int i = 0; i < 9; ++i) w[i] = v[i];
}

// The model family l3c_encode_batch / l3c_decode_batch cover (the library checks the config against the network schedule as well).
inline int check_config(const l3c_net_config *c, char *err, size_t cap) {
    if (!c) return fail(err, cap, L3C_ERR_INVALID_ARG, "null config");
    if (c->rgb_baseline)
        return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported config: the RGB / RGB Shared baselines (rgb_baseline = 1) and auto_recurse are "
                    "outside the native codec, which covers the L3C family");
    if (c->num_scales < 1 || c->num_scales > L3C_NET_MAX_SCALES) return fail(err, cap, L3C_ERR_INVALID_ARG, "num_scales must be 1 .. L3C_NET_MAX_SCALES");
    if (c->Cf != 64) return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported config: Cf = %lld, the network schedule needs Cf == 64", c->Cf);
    if (c->C < 1 || c->C > 8) return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported config: C = %lld, outside 1 .. 8", c->C);
    if (c->L < 2 || c->L > 256) return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported config: L = %lld, outside 2 .. 256 (257-entry table rows)", c->L);
    if (c->K < 1 || c->K > 16) return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported config: K = %lld, outside 1 .. 16", c->K);
    return L3C_OK;
}

inline int64_t streams_per_image(const l3c_net_config &c) { return (int64_t)c.C * c.num_scales + 3; }

inline int64_t plan_bytes(const l3c_net_config &c, int64_t B) {
    const int64_t S = B * streams_per_image(c);
    return ((int64_t)sizeof(Header) + 16 * S + (4 * S + 7) / 8 * 8 + 16 * MAX_CHUNKS + 15) / 16 * 16;
}

// Bitcoding._decode_rgb_pipelined's default chunk list of an image of HW pixels -> number of chunks
inline int rgb_chunks(int64_t HW, int64_t *pix0, int64_t *npix) {
    int64_t n = HW / 4096;
    n = n < 1 ? 1 : (n > RGB_CHUNKS ? RGB_CHUNKS : n);
    int64_t step = (HW + n - 1) / n;
    step = (step + 63) / 64 * 64;
    int k = 0;
    int64_t p0 = 0;
    if (HW >= 16 * RGB_PROBE) {
        pix0[0] = 0;          npix[0] = RGB_PROBE;
        pix0[1] = RGB_PROBE;  npix[1] = RGB_PROBE;
        k = 2;
        p0 = 2 * RGB_PROBE;
    }
    for (; p0 < HW; p0 += step) {
        pix0[k] = p0;
        npix[k++] = step < HW - p0 ? step : HW - p0;
    }
    return k;
}

inline uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }

// The limits of the network schedule on the finest scale (csrc/net.hip: check_image), so that a header cannot ask for more.
inline bool image_supported(const l3c_net_config &c, int64_t B, int64_t H, int64_t W) {
    return H * W * c.Cf * 4 < 0x7ffffff0ll && B * H * W < (1ll << 31) && 80ll * (W + 256) * 3 * c.Cf * 4 < 0x7ffffff0ll;
}

/*
 * files_host + file_offset_host[b] .. file_offset_host[b + 1]: file b.  Reads framing bytes only.  -> L3C_OK and the blob in plan_host,
 * L3C_ERR_INVALID_ARG ("invalid file: ..." for everything the bytes say; the arguments otherwise), L3C_ERR_UNSUPPORTED (banded files).
 */
inline int make_plan(const l3c_net_config *cfg, const uint8_t *files, const int64_t *file_offset, int64_t B, void *plan_host, int64_t plan_cap,
                     int *H_out, int *W_out, uint16_t *padding_out, char *err, size_t cap) {
    const int rc = check_config(cfg, err, cap);
    if (rc != L3C_OK) return rc;
    if (!files || !file_offset || !plan_host) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer");
    if (B < 1 || B >= 65536) return fail(err, cap, L3C_ERR_INVALID_ARG, "bad batch size: B = %lld, must be 1 .. 65535", B);
    if (reinterpret_cast<uintptr_t>(plan_host) & 7) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_host must be 8-byte aligned");
    const l3c_net_config &c = *cfg;
    const int64_t need = plan_bytes(c, B);
    if (plan_cap < need) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_bytes too small: %lld < %lld (l3c_decode_plan_bytes)", plan_cap, need);
    if (file_offset[0] < 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "file offsets must be non-negative and ascending");
    for (int64_t b = 0; b < B; ++b)
        if (file_offset[b + 1] < file_offset[b]) return fail(err, cap, L3C_ERR_INVALID_ARG, "file offsets must be non-negative and ascending");
    for (int64_t b = 0; b < B; ++b)
        if (file_offset[b + 1] - file_offset[b] >= 4 && memcmp(files + file_offset[b], "L3CB", 4) == 0)
            return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported file: file %lld is a banded .l3c file (L3CB format); the native codec reads the "
                        "legacy format only", b);

    const int n_rec = c.num_scales + 1;
    const int64_t S = B * streams_per_image(c);
    Header h;
    memset(&h, 0, sizeof(h));
    h.magic = MAGIC;
    h.bytes = need;
    h.B = B;
    h.n_records = n_rec;
    h.n_streams = S;
    h.files_bytes = file_offset[B];
    cfg_words(c, h.cfg);
    h.src_off = (int64_t)sizeof(Header);
    h.dst_off = h.src_off + 8 * S;
    h.nbytes_off = h.dst_off + 8 * S;
    h.chunk_pix0_off = h.nbytes_off + (4 * S + 7) / 8 * 8;
    h.chunk_npix_off = h.chunk_pix0_off + 8 * MAX_CHUNKS;
    uint8_t *blob = static_cast<uint8_t *>(plan_host);
    int64_t *src = reinterpret_cast<int64_t *>(blob + h.src_off);
    int64_t *dst = reinterpret_cast<int64_t *>(blob + h.dst_off);
    uint32_t *nbytes = reinterpret_cast<uint32_t *>(blob + h.nbytes_off);

    // the stream tables' shape is the MODEL's: a file that disagrees with it is rejected before anything is stored at an index it names
    int64_t first = 0;
    for (int k = 0; k < n_rec; ++k) {
        h.rec[k].C = k == n_rec - 1 ? 3 : c.C;
        h.rec[k].first = first;
        h.rec[k].n_streams = B * h.rec[k].C;
        first += h.rec[k].n_streams;
    }
    for (int64_t b = 0; b < B; ++b) {
        const uint8_t *f = files + file_offset[b];
        const int64_t n = file_offset[b + 1] - file_offset[b];
        int64_t p = 0;
        if (n < 8) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld truncated (%lld bytes)", b, n);
        if (padding_out)
            for (int i = 0; i < 4; ++i) padding_out[b * 4 + i] = (uint16_t)rd16(f + 2 * i);
        p = 8;
        int k = 0;
        while (p < n) {
            if (k == n_rec) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld has more than %lld scale records, the model codes %lld "
                                        "(or bytes behind the last record)", b, n_rec, n_rec);
            if (n - p < 5) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld truncated in the header of record %lld", b, k);
            const int64_t C = f[p], H = rd16(f + p + 1), W = rd16(f + p + 3);
            p += 5;
            if (C == 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, scale record %lld with C == 0", b, k);
            Record &r = h.rec[k];
            if (k == 0) {
                if (C != c.C || H < 1 || W < 1)
                    return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: coarsest scale header (C=%lld, H=%lld, W=%lld) of file %lld", C, H, W, b);
                if (b == 0) {
                    r.H = H;
                    r.W = W;
                }
            } else if (b == 0) {
                if (C != r.C || H != 2 * h.rec[k - 1].H || W != 2 * h.rec[k - 1].W)
                    return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: record %lld header (C, H, W) = (%lld, %lld, %lld) is not what the network "
                                "predicts from the record above it", k, C, H, W);
                r.H = H;
                r.W = W;
            }
            if (C != r.C || H != r.H || W != r.W)
                return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld differs from file 0 in the shape of record %lld (equally sized images "
                            "only)", b, k);
            for (int64_t ch = 0; ch < C; ++ch) {
                if (n - p < 4) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld truncated in a length field of record %lld", b, k);
                const int64_t nb = rd32(f + p);
                p += 4;
                if (nb > n - p) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, record %lld: a payload of %lld bytes runs past the end "
                                            "of the file", b, k, nb);
                const int64_t s = r.first + (k == 0 ? b * C + ch : ch * B + b);
                src[s] = file_offset[b] + p;
                nbytes[s] = (uint32_t)nb;
                if (nb > r.max_nbytes) r.max_nbytes = nb;
                p += nb;
            }
            if (n - p < 4) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld truncated at the separator of record %lld", b, k);
            if (f[p] != 0x46 || f[p + 1] != 0xE2 || f[p + 2] != 0x84 || f[p + 3] != 0x92)
                return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, scale separator missing behind record %lld", b, k);
            p += 4;
            ++k;
        }
        if (k < 2) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld has %lld scale record(s)", b, k);
        if (k != n_rec) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld has %lld scale records, the model codes %lld", b, k, n_rec);
    }
    if (h.rec[0].max_nbytes > 2 * h.rec[0].H * h.rec[0].W + 64)     // > 16 bits per symbol: not a stream of this coder
        return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: coarsest scale payload of %lld bytes, longer than %lld symbols can be", h.rec[0].max_nbytes,
                    h.rec[0].H * h.rec[0].W);
    h.H = h.rec[n_rec - 1].H;
    h.W = h.rec[n_rec - 1].W;
    if (!image_supported(c, B, h.H, h.W))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: a batch of %lld images of %lld x %lld pixels is outside what the network schedule supports",
                    B, h.H, h.W);
    int64_t pos = 0;
    for (int64_t s = 0; s < S; ++s) {
        dst[s] = pos;
        pos += ((int64_t)nbytes[s] + 3) / 4 * 4 + 4;
    }
    h.dst_bytes = pos;
    int64_t *pix0 = reinterpret_cast<int64_t *>(blob + h.chunk_pix0_off), *npix = reinterpret_cast<int64_t *>(blob + h.chunk_npix_off);
    memset(pix0, 0, 16 * MAX_CHUNKS);
    h.n_chunks = rgb_chunks(h.H * h.W, pix0, npix);
    for (int j = 0; j < h.n_chunks; ++j) h.max_chunk_npix = npix[j] > h.max_chunk_npix ? npix[j] : h.max_chunk_npix;
    h.lag = B >= 16 ? 2 : 1;
    memcpy(blob, &h, sizeof(h));
    if (H_out) *H_out = (int)h.H;
    if (W_out) *W_out = (int)h.W;
    return L3C_OK;
}

// What l3c_decode_batch checks of a blob before it trusts the header's numbers: written by make_plan for this config, complete.
inline int check_blob(const l3c_net_config &c, const void *plan_host, int64_t plan_cap, Header *out, char *err, size_t cap) {
    if (!plan_host) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer: plan_host");
    if (plan_cap >= 0 && plan_cap < (int64_t)sizeof(Header))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_bytes too small: %lld < %lld", plan_cap, (long long)sizeof(Header));
    memcpy(out, plan_host, sizeof(Header));
    if (out->magic != MAGIC) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: wrong magic word (not written by l3c_decode_plan)");
    int64_t w[9];
    cfg_words(c, w);
    if (memcmp(w, out->cfg, sizeof(w)) != 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: made for another config");
    if (out->B < 1 || out->B >= 65536 || out->n_records != c.num_scales + 1 || out->bytes != plan_bytes(c, out->B) ||
        out->n_streams != out->B * streams_per_image(c) || out->n_chunks < 1 || out->n_chunks > MAX_CHUNKS || (out->lag != 1 && out->lag != 2))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: inconsistent header");
    const int64_t S = out->n_streams;
    bool ok = out->src_off == (int64_t)sizeof(Header) && out->dst_off == out->src_off + 8 * S && out->nbytes_off == out->dst_off + 8 * S &&
              out->chunk_pix0_off == out->nbytes_off + (4 * S + 7) / 8 * 8 && out->chunk_npix_off == out->chunk_pix0_off + 8 * MAX_CHUNKS &&
              out->dst_bytes >= 4 * S && out->files_bytes >= 0;
    int64_t first = 0;
    for (int k = 0; k < c.num_scales + 1; ++k) {
        const Record &r = out->rec[k];
        ok = ok && r.C == (k == c.num_scales ? 3 : c.C) && r.first == first && r.n_streams == out->B * r.C && r.max_nbytes >= 0 &&
             r.max_nbytes <= 0xFFFFFFFFll;
        first += r.n_streams;
    }
    if (!ok) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: inconsistent header");
    if (plan_cap >= 0 && plan_cap < out->bytes)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_bytes too small: %lld < %lld", plan_cap, out->bytes);
    return L3C_OK;
}

}  // namespace l3c_plan

#endif
