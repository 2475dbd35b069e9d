// codec_plan_region.h -- the planner of a REGION decode (include/l3c_hip.h: l3c_decode_region_plan) and the row arithmetic the windowed
// network step shares with it (csrc/net.hip: l3c_net_get_p_rows).  The third sibling of codec_plan.h under the same rules: plain C++17, no
// HIP include, no library call, no allocation, so that it compiles into a stand-alone program (tests/cabi/region_plan_check_main.cpp, built
// with the address and undefined-behaviour sanitizers) as well as into libl3c_hip.so.
//
// It restates bitcoding/region.py (region_plan with cut=True, entry_table, halo_rows, apron_rows, decoder_rows) and the second half of
// Bitcoding.decode_region (the pick of the band streams, the chunk count, the lag); tests/test_native_region_abi.py compares the two element
// for element.  It reads NO file bytes: its input is the blob of l3c_decode_plan or l3c_decode_plan_banded (the magic word says which),
// re-checked with that blob's own check function, so the two planners stay the only code that parses a file.
//
// THE REGION BLOB: int64 words throughout, every array at a multiple of 16 bytes.  A RegionHeader, then at the byte offsets it names, with
// S = B (j1 - j0) entries per channel:
//     src_offset int64 [3 S] | dst_offset int64 [3 S] | nbytes uint32 [3 S]     the picked streams of the finest record for
//                                                     l3c_container_read, CHANNEL-major: stream (c, e) at c S + e, e = b (j1 - j0) + (j - j0);
//                                                     dst_offset is compact (((nbytes + 3) / 4) * 4 + 4 bytes per stream, back to back)
//     entries int64 [4][S] = pixbase | hw | pix0 | len                          region.entry_table: l3c_decode_rgb_entries reads it from the
//                                                     host and the device copy
//     crop l3c_u8_image [B]                                                     l3c_u8_scatter: the box out of the window frames [B][3][c1 - c0][W]
// A region blob can be CHECKED against its plan blob without trusting a word of it: the header names the shared padding and the box, and
// region_check makes the blob again from them and compares (no second buffer: element by element).
#ifndef L3C_CODEC_PLAN_REGION_H_
#define L3C_CODEC_PLAN_REGION_H_

#include "codec_plan_banded.h"

namespace l3c_plan {

constexpr int64_t REGION_MAGIC = 0x4e414c505243334cll;   // the bytes "L3CRPLAN"
constexpr int64_t REGION_GRANULE = 64;                   // region.GRANULE
constexpr int64_t REGION_MAX_ENTRIES = 65535;            // l3c_decode_rgb_entries: entries per call
constexpr int64_t REGION_BAND_CHUNKS = RGB_BAND_CHUNKS, REGION_LEGACY_CHUNKS = RGB_CHUNKS;

// region.halo_rows / apron_rows / decoder_rows
inline int64_t region_halo_rows(int64_t dec_blocks) { return 2 * (2 * dec_blocks + 2) + 4; }
inline int64_t region_apron_rows(int64_t dec_blocks) {
    const int64_t half = 4 * (2 * dec_blocks + 2), g = REGION_GRANULE / 2;
    return 2 * ((half + g - 1) / g * g);
}
inline void region_decoder_rows(int64_t H, int64_t c0, int64_t c1, int64_t apron, int64_t *a0, int64_t *a1) {
    *a0 = c0 - apron < 0 ? 0 : c0 - apron;
    *a1 = c1 + apron > H ? H : c1 + apron;
}

struct RegionRows {
    int64_t j0, j1;      // bands
    int64_t p0, p1;      // symbol rows
    int64_t c0, c1;      // conv rows
    int64_t v0, v1;      // valid rows
};

// region.region_plan(H, W, L, (y0, y1), halo, cut=True) for 0 <= y0 < y1 <= H; H, W in 1 .. 65535, 1 <= L < 2^33
inline RegionRows region_rows(int64_t H, int64_t W, int64_t L, int64_t y0, int64_t y1, int64_t halo) {
    const int64_t G = REGION_GRANULE;
    RegionRows r;
    r.j0 = y0 * W / L;
    r.j1 = (y1 * W + L - 1) / L;
    r.p0 = r.j0 * L / W;
    r.p1 = y1;
    r.c0 = r.p0 < halo ? 0 : (r.p0 - halo) / G * G;
    r.c1 = (r.p1 + halo + G - 1) / G * G;
    if (r.c1 > H) r.c1 = H;
    r.v0 = r.c0 == 0 ? 0 : r.c0 + halo;
    r.v1 = r.c1 == H ? H : r.c1 - halo;
    return r;
}
// band j of that plan: its first pixel inside the window image, and its symbols (the last band ends with row p1 - 1)
inline int64_t region_pix0(const RegionRows &r, int64_t W, int64_t L, int64_t j) { return j * L - r.c0 * W; }
inline int64_t region_len(const RegionRows &r, int64_t H, int64_t W, int64_t L, int64_t j) {
    int64_t end = (j + 1) * L < H * W ? (j + 1) * L : H * W;
    if (end > r.p1 * W) end = r.p1 * W;
    return end - j * L;
}

struct RegionHeader {
    int64_t magic, bytes;              // REGION_MAGIC; size of the blob
    int64_t plan_magic;                // of the plan blob it was made from
    int64_t B, H, W, L, n;             // the frames, the finest record's band length (legacy: H W) and bands per channel
    int64_t pad[4];                    // the files' one padding tuple: left, right, top, bottom
    int64_t box[4];                    // y0, y1, x0, x1 in UNPADDED image coordinates
    RegionRows rows;
    int64_t a0, a1;                    // decoder rows
    int64_t S;                         // entries (and picked streams per channel): B (j1 - j0)
    int64_t n_chunks, lag;             // of the l3c_decode_rgb_entries call
    int64_t max_nbytes, dst_bytes;     // of the picked streams: the longest, and the size of their stream buffer
    int64_t streams_total, bytes_used, bytes_total;
    int64_t cfg[9];
    int64_t src_off, dst_off, nbytes_off, entries_off, crop_off;
};

inline int64_t up16(int64_t n) { return (n + 15) / 16 * 16; }

// offsets and size from h.B and h.S
inline void region_layout(RegionHeader &h) {
    const int64_t T = 3 * h.S;
    h.src_off = up16((int64_t)sizeof(RegionHeader));
    h.dst_off = h.src_off + up16(8 * T);
    h.nbytes_off = h.dst_off + up16(8 * T);
    h.entries_off = h.nbytes_off + up16(4 * T);
    h.crop_off = h.entries_off + up16(4 * 8 * h.S);
    h.bytes = h.crop_off + up16((int64_t)sizeof(l3c_u8_image) * h.B);
}

// What the region planner reads of either plan blob: the frames and the streams of the finest record.
struct RegionView {
    int64_t magic, B, H, W, L, n, first, files_bytes;
    const int64_t *src;
    const uint32_t *nbytes;
};

inline int region_config(const l3c_net_config *cfg, char *err, size_t cap) {
    const int rc = check_config(cfg, err, cap);
    if (rc != L3C_OK) return rc;
    if (cfg->num_scales < 2)
        return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported config: a region decode windows the finest of at least two predicted scales, "
                    "num_scales = %lld", cfg->num_scales);
    if (cfg->dec_blocks < 0 || cfg->dec_blocks > 64) return fail(err, cap, L3C_ERR_INVALID_ARG, "dec_blocks must be 0 .. 64");
    return L3C_OK;
}

// plan_cap < 0: the size is not known (the blob is trusted to be complete, as in the workspace functions of the decoders)
inline int region_view(const l3c_net_config &c, const void *plan_host, int64_t plan_cap, RegionView *v, char *err, size_t cap) {
    if (!plan_host) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer: plan_host");
    if (reinterpret_cast<uintptr_t>(plan_host) & 7) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_host must be 8-byte aligned");
    if (plan_cap >= 0 && plan_cap < (int64_t)sizeof(int64_t))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_bytes too small: %lld < %lld", plan_cap, (long long)sizeof(int64_t));
    const uint8_t *blob = static_cast<const uint8_t *>(plan_host);
    const int n_rec = c.num_scales + 1;
    memcpy(&v->magic, plan_host, sizeof(int64_t));
    if (v->magic == BANDED_MAGIC) {
        BandedHeader h;
        const int rc = check_blob_banded(c, plan_host, plan_cap, &h, err, cap);
        if (rc != L3C_OK) return rc;
        const BandedRecord &r = h.rec[n_rec - 1];
        *v = RegionView{v->magic, h.B, r.H, r.W, r.L, r.n, r.first, h.files_bytes, reinterpret_cast<const int64_t *>(blob + h.src_off),
                        reinterpret_cast<const uint32_t *>(blob + h.nbytes_off)};
        return L3C_OK;
    }
    Header h;
    const int rc = check_blob(c, plan_host, plan_cap, &h, err, cap);
    if (rc != L3C_OK) return rc;
    const Record &r = h.rec[n_rec - 1];
    if (r.H < 1 || r.H >= 65536 || r.W < 1 || r.W >= 65536 || r.H != h.H || r.W != h.W)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: inconsistent header");
    *v = RegionView{v->magic, h.B, r.H, r.W, r.H * r.W, 1, r.first, h.files_bytes, reinterpret_cast<const int64_t *>(blob + h.src_off),
                    reinterpret_cast<const uint32_t *>(blob + h.nbytes_off)};
    return L3C_OK;
}

// writes a word of the blob, or compares it with the word that is there
struct RegionPut {
    bool write, same;
    template <class T>
    void operator()(T *at, T v) {
        if (write) *at = v;
        else same = same && *at == v;
    }
};

/*
 * The blob for `box` of the frames of `v` whose one padding tuple is `pad`: written into blob (write), or compared with it.  blob_cap is
 * checked against the size the box needs.  -> L3C_OK and the header in *out, or a status and a message.
 */
inline int region_make(const l3c_net_config &c, const RegionView &v, const int64_t pad[4], const int64_t box[4], uint8_t *blob, int64_t blob_cap,
                       bool write, RegionHeader *out, char *err, size_t cap) {
    const int64_t B = v.B, H = v.H, W = v.W, L = v.L, n = v.n;
    if (W % 4) return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported shape: a frame of %lld columns (l3c_u8_scatter moves whole dwords)", W);
    const int64_t left = pad[0], right = pad[1], top = pad[2], bottom = pad[3];
    const int64_t h_img = H - top - bottom, w_img = W - left - right;
    const int64_t y0 = box[0], y1 = box[1], x0 = box[2], x1 = box[3];
    if (!(0 <= y0 && y0 < y1 && y1 <= h_img && 0 <= x0 && x0 < x1 && x1 <= w_img)) {
        if (err && cap)
            snprintf(err, cap, "box rows [%lld, %lld) x columns [%lld, %lld) is empty or not inside the %lldx%lld image", (long long)y0, (long long)y1,
                     (long long)x0, (long long)x1, (long long)h_img, (long long)w_img);
        return L3C_ERR_INVALID_ARG;
    }
    RegionHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = REGION_MAGIC;
    h.plan_magic = v.magic;
    h.B = B;  h.H = H;  h.W = W;  h.L = L;  h.n = n;
    for (int i = 0; i < 4; ++i) h.pad[i] = pad[i], h.box[i] = box[i];
    const RegionRows r = h.rows = region_rows(H, W, L, top + y0, top + y1, region_halo_rows(c.dec_blocks));
    region_decoder_rows(H, r.c0, r.c1, region_apron_rows(c.dec_blocks), &h.a0, &h.a1);
    const int64_t nj = r.j1 - r.j0, S = h.S = B * nj;
    if (S > REGION_MAX_ENTRIES)
        return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported batch: %lld images x %lld bands of the region, more than 65535 entries in one call: "
                    "slice the batch", B, nj);
    cfg_words(c, h.cfg);
    region_layout(h);
    if (blob_cap < h.bytes)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "region_bytes too small: %lld < %lld (l3c_decode_region_plan_bytes)", blob_cap, h.bytes);
    RegionPut put{write, true};
    if (write) memset(blob, 0, (size_t)h.bytes);
    int64_t *src = reinterpret_cast<int64_t *>(blob + h.src_off), *dst = reinterpret_cast<int64_t *>(blob + h.dst_off);
    uint32_t *nbytes = reinterpret_cast<uint32_t *>(blob + h.nbytes_off);
    int64_t pos = 0;
    for (int64_t ch = 0; ch < 3; ++ch)
        for (int64_t b = 0; b < B; ++b)
            for (int64_t j = r.j0; j < r.j1; ++j) {
                const int64_t s = v.first + (ch * B + b) * n + j, t = ch * S + b * nj + (j - r.j0);
                const int64_t at = v.src[s], nb = v.nbytes[s];
                if (at < 0 || nb > v.files_bytes || at > v.files_bytes - nb)
                    return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: stream %lld of the finest record lies outside the files", s - v.first);
                put(src + t, at);
                put(dst + t, pos);
                put(nbytes + t, (uint32_t)nb);
                pos += (nb + 3) / 4 * 4 + 4;
                h.bytes_used += nb;
                if (nb > h.max_nbytes) h.max_nbytes = nb;
            }
    h.dst_bytes = pos;
    h.streams_total = 3 * B * n;
    for (int64_t s = 0; s < h.streams_total; ++s) h.bytes_total += v.nbytes[v.first + s];
    int64_t *e = reinterpret_cast<int64_t *>(blob + h.entries_off);
    const int64_t hw = (r.c1 - r.c0) * W;
    int64_t min_len = H * W;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t j = r.j0; j < r.j1; ++j) {
            const int64_t i = b * nj + (j - r.j0), len = region_len(r, H, W, L, j);
            put(e + i, b * hw);
            put(e + S + i, hw);
            put(e + 2 * S + i, region_pix0(r, W, L, j));
            put(e + 3 * S + i, len);
            if (len < min_len) min_len = len;
        }
    const int64_t per = v.magic == BANDED_MAGIC ? 64 : 4096, most = v.magic == BANDED_MAGIC ? REGION_BAND_CHUNKS : REGION_LEGACY_CHUNKS;
    h.n_chunks = min_len / per < 1 ? 1 : (min_len / per > most ? most : min_len / per);
    h.lag = S >= 16 ? 2 : 1;
    l3c_u8_image *crop = reinterpret_cast<l3c_u8_image *>(blob + h.crop_off);
    const int64_t bh = y1 - y0, bw = x1 - x0;
    for (int64_t b = 0; b < B; ++b) {
        put(&crop[b].offset, b * 3 * bh * bw);
        put(&crop[b].row_stride, bw);
        put(&crop[b].chan_stride, bh * bw);
        put(&crop[b].pix_stride, (int32_t)1);
        put(&crop[b].h, (int32_t)bh);
        put(&crop[b].w, (int32_t)bw);
        put(&crop[b].top, (int32_t)(y0 + top - r.c0));
        put(&crop[b].left, (int32_t)(x0 + left));
    }
    if (write) memcpy(blob, &h, sizeof(h));
    else if (!put.same || memcmp(blob, &h, sizeof(h)) != 0)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "region blob: not what l3c_decode_region_plan writes for this plan blob");
    *out = h;
    return L3C_OK;
}

inline void region_info(const RegionHeader &h, l3c_region_info *info) {
    const RegionRows &r = h.rows;
    memset(info, 0, sizeof(*info));
    info->bands[0] = (int32_t)r.j0;         info->bands[1] = (int32_t)r.j1;
    info->n_bands = (int32_t)h.n;
    info->sym_rows[0] = (int32_t)r.p0;      info->sym_rows[1] = (int32_t)r.p1;
    info->conv_rows[0] = (int32_t)r.c0;     info->conv_rows[1] = (int32_t)r.c1;
    info->valid_rows[0] = (int32_t)r.v0;    info->valid_rows[1] = (int32_t)r.v1;
    info->decoder_rows[0] = (int32_t)h.a0;  info->decoder_rows[1] = (int32_t)h.a1;
    info->frame_rows = (int32_t)h.H;
    info->n_chunks = (int32_t)h.n_chunks;
    info->lag = (int32_t)h.lag;
    info->out_rows = (int32_t)(h.box[1] - h.box[0]);
    info->out_cols = (int32_t)(h.box[3] - h.box[2]);
    info->streams_used = 3 * h.S;
    info->streams_total = h.streams_total;
    info->bytes_used = h.bytes_used;
    info->bytes_total = h.bytes_total;
}

/* The size that holds the region blob of ANY box of these files (every band picked).  -> bytes, or a negative status. */
inline int64_t region_plan_bytes(const l3c_net_config *cfg, const void *plan_host, char *err, size_t cap) {
    int rc = region_config(cfg, err, cap);
    if (rc != L3C_OK) return rc;
    RegionView v;
    rc = region_view(*cfg, plan_host, -1, &v, err, cap);
    if (rc != L3C_OK) return rc;
    RegionHeader h;
    memset(&h, 0, sizeof(h));
    h.B = v.B;
    h.S = v.B * v.n;
    region_layout(h);
    return h.bytes;
}

/*
 * plan_host: the blob of l3c_decode_plan or l3c_decode_plan_banded; padding_host: the uint16 [B][4] either planner gave.  -> L3C_OK, the
 * region blob in region_host and the plan's numbers in *info_out (may be null); L3C_ERR_INVALID_ARG (an empty box or one that leaves the
 * image, files of different padding tuples, a blob that fails its check, region_bytes too small); L3C_ERR_UNSUPPORTED (the RGB baselines,
 * fewer than two scales, more than 65535 entries).
 */
inline int make_region_plan(const l3c_net_config *cfg, const void *plan_host, int64_t plan_cap, const uint16_t *padding_host, const l3c_region_box *box,
                            void *region_host, int64_t region_cap, l3c_region_info *info_out, char *err, size_t cap) {
    int rc = region_config(cfg, err, cap);
    if (rc != L3C_OK) return rc;
    if (!padding_host || !box || !region_host) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer");
    if (reinterpret_cast<uintptr_t>(region_host) & 7) return fail(err, cap, L3C_ERR_INVALID_ARG, "region_host must be 8-byte aligned");
    if (plan_cap < 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_bytes too small: %lld < %lld", plan_cap, (long long)sizeof(int64_t));
    RegionView v;
    rc = region_view(*cfg, plan_host, plan_cap, &v, err, cap);
    if (rc != L3C_OK) return rc;
    for (int64_t b = 1; b < v.B; ++b)
        if (memcmp(padding_host, padding_host + 4 * b, 4 * sizeof(uint16_t)) != 0) {
            const uint16_t *p = padding_host, *q = padding_host + 4 * b;
            if (err && cap)
                snprintf(err, cap, "decode_region needs files of one padding tuple, got (%d, %d, %d, %d) and (%d, %d, %d, %d)", p[0], p[1], p[2], p[3],
                         q[0], q[1], q[2], q[3]);
            return L3C_ERR_INVALID_ARG;
        }
    const int64_t pad[4] = {padding_host[0], padding_host[1], padding_host[2], padding_host[3]};
    const int64_t bx[4] = {box->y0, box->y1, box->x0, box->x1};
    RegionHeader h;
    rc = region_make(*cfg, v, pad, bx, static_cast<uint8_t *>(region_host), region_cap, true, &h, err, cap);
    if (rc != L3C_OK) return rc;
    if (info_out) region_info(h, info_out);
    return L3C_OK;
}

/*
 * What l3c_decode_region checks of a region blob before it trusts a word of it: the header's own padding and box, planned again from the
 * plan blob, must give this very blob.  region_cap < 0: the size is not known (the workspace function).
 */
inline int region_check(const l3c_net_config &c, const void *plan_host, int64_t plan_cap, const void *region_host, int64_t region_cap,
                        RegionHeader *out, char *err, size_t cap) {
    RegionView v;
    int rc = region_view(c, plan_host, plan_cap, &v, err, cap);
    if (rc != L3C_OK) return rc;
    if (!region_host) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer: region_host");
    if (reinterpret_cast<uintptr_t>(region_host) & 7) return fail(err, cap, L3C_ERR_INVALID_ARG, "region_host must be 8-byte aligned");
    if (region_cap >= 0 && region_cap < (int64_t)sizeof(RegionHeader))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "region_bytes too small: %lld < %lld", region_cap, (long long)sizeof(RegionHeader));
    RegionHeader h;
    memcpy(&h, region_host, sizeof(h));
    if (h.magic != REGION_MAGIC) return fail(err, cap, L3C_ERR_INVALID_ARG, "region blob: wrong magic word (not written by l3c_decode_region_plan)");
    int64_t w[9];
    cfg_words(c, w);
    if (memcmp(w, h.cfg, sizeof(w)) != 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "region blob: made for another config");
    bool ok = true;
    for (int i = 0; i < 4; ++i) ok = ok && h.pad[i] >= 0 && h.pad[i] < 65536 && h.box[i] >= INT32_MIN && h.box[i] <= INT32_MAX;
    if (!ok || h.bytes < (int64_t)sizeof(RegionHeader)) return fail(err, cap, L3C_ERR_INVALID_ARG, "region blob: inconsistent header");
    // the size the header's box needs is checked against the caller's buffer first; an unknown size is the header's own
    return region_make(c, v, h.pad, h.box, const_cast<uint8_t *>(static_cast<const uint8_t *>(region_host)), region_cap < 0 ? h.bytes : region_cap, false,
                       out, err, cap);
}

}  // namespace l3c_plan

#endif
