// codec_plan_banded.h -- the validating parser of the BANDED `.l3c` framing and the decode plan it writes (include/l3c_hip.h:
// l3c_decode_plan_banded).  The sibling of codec_plan.h under the same rules: plain C++17, no HIP include, no library call, no allocation,
// so that it compiles into a stand-alone program (tests/cabi/plan_banded_check_main.cpp, built with the address and undefined-behaviour
// sanitizers) as well as into libl3c_hip.so (csrc/codec.hip).
//
// The format (bitcoding/container.py), little-endian:
//     'L3CB' | u8 version = 1 | u8 0 | u16 x4 padding
//     for scale = coarsest .. 0:  u8 C, u16 H, u16 W, u32 L | for channel c: for band j < n = ceil(H W / L): u32 nbytes, payload | 46 E2 84 92
// What is rejected is what the Python readers reject before their first upload: container.parse_banded / parse_batch (framing, files that
// disagree), Bitcoding._n_predicted (record count), _check_coarsest and _check_header (the shapes the decoder kernels will index with).
//
// THE PLAN BLOB: int64 words throughout.  A BandedHeader, then at the byte offsets it names
//     src_offset int64 [n_streams] | dst_offset int64 [n_streams] | nbytes uint32 [n_streams] | per bottleneck record k, at entries_off[k]:
//     the entry table int64 [5][B n_k] = pixbase | hw | pix0 | npix | table_off of container.band_entry_table, entry (b, j) at b n_k + j
// The number of bands is a property of the FILES, so the size of the blob is too (plan_banded_bytes walks file 0).  Streams are numbered
// record after record, coarsest first; inside the coarsest record band (b, c, j) is (b C + c) n + j (l3c_ac_decode_bands writes [B][C][h w]),
// inside every other record (c B + b) n + j (a channel's B n bands adjacent: the ragged decoders and l3c_decode_rgb_banded).  src_offset /
// dst_offset / nbytes as in codec_plan.h.  table_off = (pixbase + pix0) * (L_model + 1) * 2: the byte offset of a band's rows in a
// channel's table of B h w rows.
#ifndef L3C_CODEC_PLAN_BANDED_H_
#define L3C_CODEC_PLAN_BANDED_H_

#include "codec_plan.h"

namespace l3c_plan {

constexpr int64_t BANDED_MAGIC = 0x4e414c504243334cll;   // the bytes "L3CBPLAN"
constexpr int64_t MAX_BANDS = 1024, MAX_BAND_STREAMS = 65535, RGB_BAND_CHUNKS = 8;

struct BandedRecord {
    int64_t C, H, W, L, n;     // the record's header; n = ceil(H W / L) bands per channel
    int64_t first, n_streams;  // its streams: [first, first + B C n) of the blob's arrays
    int64_t max_nbytes;        // the longest of them
};

struct BandedHeader {
    int64_t magic, bytes;      // BANDED_MAGIC; size of the blob
    int64_t B, n_records;
    int64_t H, W;              // the (padded) image: the finest record's
    int64_t n_streams;         // over all records
    int64_t files_bytes;       // file_offset[B]
    int64_t dst_bytes;         // size of the stream buffer
    int64_t rgb_band_len, rgb_chunks, lag;   // l3c_decode_rgb_banded of the finest record
    int64_t cfg[9];            // the l3c_net_config the plan was made for
    int64_t src_off, dst_off, nbytes_off;    // byte offsets of the arrays inside the blob
    int64_t entries_off[MAX_RECORDS];        // of the entry table of record k; 0 for the coarsest and the RGB record
    BandedRecord rec[MAX_RECORDS];
};

inline bool is_banded_file(const uint8_t *f, int64_t n) { return n >= 4 && memcmp(f, "L3CB", 4) == 0; }

inline int64_t rgb_band_chunks(int64_t HW, int64_t L, int64_t n) {
    const int64_t c = (HW - (n - 1) * L) / 64;
    return c < 1 ? 1 : (c > RGB_BAND_CHUNKS ? RGB_BAND_CHUNKS : c);
}

// offsets and size of the blob from B and the records' C and n (h.B, h.n_records, h.rec[k].C / .n set): fills first / n_streams, n_streams,
// src_off .. entries_off, bytes
inline void banded_layout(BandedHeader &h) {
    int64_t first = 0;
    for (int k = 0; k < (int)h.n_records; ++k) {
        h.rec[k].first = first;
        h.rec[k].n_streams = h.B * h.rec[k].C * h.rec[k].n;
        first += h.rec[k].n_streams;
    }
    const int64_t S = h.n_streams = first;
    h.src_off = (int64_t)sizeof(BandedHeader);
    h.dst_off = h.src_off + 8 * S;
    h.nbytes_off = h.dst_off + 8 * S;
    int64_t at = h.nbytes_off + (4 * S + 7) / 8 * 8;
    for (int k = 0; k < MAX_RECORDS; ++k) {
        h.entries_off[k] = 0;
        if (k > 0 && k < (int)h.n_records - 1) {
            h.entries_off[k] = at;
            at += 5 * 8 * h.B * h.rec[k].n;
        }
    }
    h.bytes = (at + 15) / 16 * 16;
}

// The arguments every entry point shares, then the format of every file: all banded, or L3C_ERR_UNSUPPORTED.
inline int banded_check_args(const l3c_net_config *cfg, const uint8_t *files, const int64_t *file_offset, int64_t B, char *err, size_t cap) {
    const int rc = check_config(cfg, err, cap);
    if (rc != L3C_OK) return rc;
    if (!files || !file_offset) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer");
    if (B < 1 || B >= 65536) return fail(err, cap, L3C_ERR_INVALID_ARG, "bad batch size: B = %lld, must be 1 .. 65535", B);
    if (file_offset[0] < 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "file offsets must be non-negative and ascending");
    for (int64_t b = 0; b < B; ++b)
        if (file_offset[b + 1] < file_offset[b]) return fail(err, cap, L3C_ERR_INVALID_ARG, "file offsets must be non-negative and ascending");
    for (int64_t b = 0; b < B; ++b)      // too short for a signature: a file of neither format
        if (file_offset[b + 1] - file_offset[b] < 4)
            return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld truncated (%lld bytes)", b, file_offset[b + 1] - file_offset[b]);
    int64_t n_banded = 0;
    for (int64_t b = 0; b < B; ++b) n_banded += is_banded_file(files + file_offset[b], file_offset[b + 1] - file_offset[b]) ? 1 : 0;
    if (n_banded == 0)
        return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported file: a legacy .l3c file (no L3CB signature); l3c_decode_plan / l3c_decode_batch read "
                    "the legacy format");
    if (n_banded != B)
        return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported batch: it mixes banded and legacy .l3c files (%lld of %lld are banded)", n_banded, B);
    return L3C_OK;
}

/*
 * The walk over file b's framing.  b == 0 sets h.rec[k].C / H / W / L / n from the headers (checked against the model), every other file
 * must repeat them.  src / nbytes: where the streams' positions and lengths go, or null (the sizing walk: h's `first` fields are then not
 * read).  h.rec[k].max_nbytes is raised as the walk goes.
 */
inline int banded_walk(const l3c_net_config &c, const uint8_t *f, int64_t n, int64_t file_base, int64_t b, int64_t B, BandedHeader &h,
                       int64_t *src, uint32_t *nbytes, uint16_t *padding_out, char *err, size_t cap) {
    const int n_rec = c.num_scales + 1;
    if (n < 14) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld truncated (%lld bytes)", b, n);
    if (f[4] != 1) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, unknown banded format version %lld", b, f[4]);
    if (f[5] != 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, reserved byte is %lld", b, f[5]);
    if (padding_out)
        for (int i = 0; i < 4; ++i) padding_out[b * 4 + i] = (uint16_t)rd16(f + 6 + 2 * i);
    int64_t p = 14;
    int k = 0;
    while (p < n) {
        if (k == n_rec) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld has more than %lld scale records, the model codes %lld "
                                    "(or bytes behind the last record)", b, n_rec, n_rec);
        if (n - p < 9) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld truncated in the header of record %lld", b, k);
        const int64_t C = f[p], H = rd16(f + p + 1), W = rd16(f + p + 3), L = rd32(f + p + 5);
        p += 9;
        if (C == 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, scale record %lld with C == 0", b, k);
        if (H == 0 || W == 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, record %lld: empty scale %lld x %lld", b, k, H, W);
        if (L == 0 || L % 64) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, record %lld: band length %lld is not a positive "
                                          "multiple of 64", b, k, L);
        const int64_t nb_ = (H * W + L - 1) / L;
        if (nb_ > MAX_BANDS) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, record %lld: %lld bands per channel (at most 1024)",
                                         b, k, nb_);
        BandedRecord &r = h.rec[k];
        if (b == 0) {
            const int64_t Cs = k == n_rec - 1 ? 3 : c.C;
            if (k == 0 && C != Cs)
                return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: coarsest scale header (C=%lld, H=%lld, W=%lld) of file %lld", C, H, W, b);
            if (k > 0 && (C != Cs || H != 2 * h.rec[k - 1].H || W != 2 * h.rec[k - 1].W))
                return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: record %lld header (C, H, W) = (%lld, %lld, %lld) is not what the network "
                            "predicts from the record above it", k, C, H, W);
            r.C = C;  r.H = H;  r.W = W;  r.L = L;  r.n = nb_;
            if (B * nb_ > MAX_BAND_STREAMS)
                return fail(err, cap, L3C_ERR_UNSUPPORTED, "unsupported batch: record %lld has %lld images x %lld bands, more than 65535 band streams "
                            "per channel in one call: slice the batch", k, B, nb_);
        } else if (C != r.C || H != r.H || W != r.W) {
            return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld differs from file 0 in the shape of record %lld (equally sized images "
                        "only)", b, k);
        } else if (L != r.L) {
            return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld differs from file 0 in the band length of record %lld (%lld, not %lld)",
                        b, k, L, r.L);
        }
        for (int64_t ch = 0; ch < C; ++ch)
            for (int64_t j = 0; j < nb_; ++j) {
                if (n - p < 4) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld truncated in a length field of record %lld", b, k);
                const int64_t nb = rd32(f + p);
                p += 4;
                if (nb > n - p) return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: file %lld, record %lld: a payload of %lld bytes runs past the "
                                            "end of the file", b, k, nb);
                if (src) {
                    const int64_t s = r.first + ((k == 0 ? b * C + ch : ch * B + b) * nb_ + j);
                    src[s] = file_base + p;
                    nbytes[s] = (uint32_t)nb;
                }
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
    return L3C_OK;
}

// what only the whole of a file's records say: the coarsest bound (Bitcoding._check_coarsest, banded form) and the schedule's limits
inline int banded_check_records(const l3c_net_config &c, BandedHeader &h, char *err, size_t cap) {
    const int n_rec = c.num_scales + 1;
    if (h.rec[0].max_nbytes > 2 * h.rec[0].L + 64)     // > 16 bits per symbol: not a stream of this coder
        return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: coarsest scale band payload of %lld bytes, longer than %lld symbols can be",
                    h.rec[0].max_nbytes, h.rec[0].L);
    h.H = h.rec[n_rec - 1].H;
    h.W = h.rec[n_rec - 1].W;
    if (!image_supported(c, h.B, h.H, h.W))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "invalid file: a batch of %lld images of %lld x %lld pixels is outside what the network schedule supports",
                    h.B, h.H, h.W);
    return L3C_OK;
}

inline void banded_header_init(const l3c_net_config &c, int64_t B, int64_t files_bytes, BandedHeader &h) {
    memset(&h, 0, sizeof(h));
    h.magic = BANDED_MAGIC;
    h.B = B;
    h.n_records = c.num_scales + 1;
    h.files_bytes = files_bytes;
    cfg_words(c, h.cfg);
}

/* Size of the blob of these files: walks file 0's framing, validating as it goes.  -> bytes, or a negative status. */
inline int64_t plan_banded_bytes(const l3c_net_config *cfg, const uint8_t *files, const int64_t *file_offset, int64_t B, char *err, size_t cap) {
    int rc = banded_check_args(cfg, files, file_offset, B, err, cap);
    if (rc != L3C_OK) return rc;
    BandedHeader h;
    banded_header_init(*cfg, B, file_offset[B], h);
    rc = banded_walk(*cfg, files + file_offset[0], file_offset[1] - file_offset[0], file_offset[0], 0, B, h, nullptr, nullptr, nullptr, err, cap);
    if (rc != L3C_OK) return rc;
    banded_layout(h);
    return h.bytes;
}

/*
 * files_host + file_offset_host[b] .. file_offset_host[b + 1]: file b.  Reads framing bytes only.  -> L3C_OK and the blob in plan_host,
 * L3C_ERR_INVALID_ARG ("invalid file: ..." for everything the bytes say; the arguments otherwise), L3C_ERR_UNSUPPORTED (legacy files, a mix,
 * more than 65535 band streams per channel).
 */
inline int make_plan_banded(const l3c_net_config *cfg, const uint8_t *files, const int64_t *file_offset, int64_t B, void *plan_host,
                            int64_t plan_cap, int *H_out, int *W_out, uint16_t *padding_out, char *err, size_t cap) {
    int rc = banded_check_args(cfg, files, file_offset, B, err, cap);
    if (rc != L3C_OK) return rc;
    if (!plan_host) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer");
    if (reinterpret_cast<uintptr_t>(plan_host) & 7) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_host must be 8-byte aligned");
    const l3c_net_config &c = *cfg;
    const int n_rec = c.num_scales + 1;
    BandedHeader h;
    banded_header_init(c, B, file_offset[B], h);
    // file 0 says how many streams there are: sized and checked before anything is stored at an index a file names
    rc = banded_walk(c, files + file_offset[0], file_offset[1] - file_offset[0], file_offset[0], 0, B, h, nullptr, nullptr, nullptr, err, cap);
    if (rc != L3C_OK) return rc;
    banded_layout(h);
    if (plan_cap < h.bytes)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_bytes too small: %lld < %lld (l3c_decode_plan_banded_bytes)", plan_cap, h.bytes);
    for (int k = 0; k < n_rec; ++k) h.rec[k].max_nbytes = 0;
    uint8_t *blob = static_cast<uint8_t *>(plan_host);
    int64_t *src = reinterpret_cast<int64_t *>(blob + h.src_off);
    int64_t *dst = reinterpret_cast<int64_t *>(blob + h.dst_off);
    uint32_t *nbytes = reinterpret_cast<uint32_t *>(blob + h.nbytes_off);
    memset(blob, 0, (size_t)h.bytes);
    for (int64_t b = 0; b < B; ++b) {
        rc = banded_walk(c, files + file_offset[b], file_offset[b + 1] - file_offset[b], file_offset[b], b, B, h, src, nbytes, padding_out, err,
                         cap);
        if (rc != L3C_OK) {
            memset(blob, 0, sizeof(int64_t));      // no plan
            return rc;
        }
    }
    rc = banded_check_records(c, h, err, cap);
    if (rc != L3C_OK) {
        memset(blob, 0, sizeof(int64_t));
        return rc;
    }
    int64_t pos = 0;
    for (int64_t s = 0; s < h.n_streams; ++s) {
        dst[s] = pos;
        pos += ((int64_t)nbytes[s] + 3) / 4 * 4 + 4;
    }
    h.dst_bytes = pos;
    for (int k = 1; k < n_rec - 1; ++k) {
        const BandedRecord &r = h.rec[k];
        const int64_t HW = r.H * r.W, E = B * r.n;
        int64_t *e = reinterpret_cast<int64_t *>(blob + h.entries_off[k]);
        for (int64_t b = 0; b < B; ++b)
            for (int64_t j = 0; j < r.n; ++j) {
                const int64_t i = b * r.n + j, pix0 = j * r.L;
                e[i] = b * HW;
                e[E + i] = HW;
                e[2 * E + i] = pix0;
                e[3 * E + i] = r.L < HW - pix0 ? r.L : HW - pix0;
                e[4 * E + i] = (b * HW + pix0) * (c.L + 1) * 2;
            }
    }
    const BandedRecord &rgb = h.rec[n_rec - 1];
    h.rgb_band_len = rgb.L;
    h.rgb_chunks = rgb_band_chunks(rgb.H * rgb.W, rgb.L, rgb.n);
    h.lag = B * rgb.n >= 16 ? 2 : 1;
    memcpy(blob, &h, sizeof(h));
    if (H_out) *H_out = (int)h.H;
    if (W_out) *W_out = (int)h.W;
    return L3C_OK;
}

// What l3c_decode_batch_banded checks of a blob before it trusts the header's numbers: written by make_plan_banded for this config, every
// record and offset what the records' own (C, H, W, L) and B imply.
inline int check_blob_banded(const l3c_net_config &c, const void *plan_host, int64_t plan_cap, BandedHeader *out, char *err, size_t cap) {
    if (!plan_host) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer: plan_host");
    if (plan_cap >= 0 && plan_cap < (int64_t)sizeof(int64_t))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_bytes too small: %lld < %lld", plan_cap, (long long)sizeof(BandedHeader));
    int64_t magic;
    memcpy(&magic, plan_host, sizeof(magic));
    if (magic == MAGIC) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: wrong magic word (a legacy plan of l3c_decode_plan: l3c_decode_batch reads it)");
    if (magic != BANDED_MAGIC) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: wrong magic word (not written by l3c_decode_plan_banded)");
    if (plan_cap >= 0 && plan_cap < (int64_t)sizeof(BandedHeader))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_bytes too small: %lld < %lld", plan_cap, (long long)sizeof(BandedHeader));
    memcpy(out, plan_host, sizeof(BandedHeader));
    int64_t w[9];
    cfg_words(c, w);
    if (memcmp(w, out->cfg, sizeof(w)) != 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: made for another config");
    const int n_rec = c.num_scales + 1;
    if (out->B < 1 || out->B >= 65536 || out->n_records != n_rec || (out->lag != 1 && out->lag != 2))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: inconsistent header");
    bool ok = true;
    for (int k = 0; k < n_rec && ok; ++k) {
        const BandedRecord &r = out->rec[k];
        ok = r.C == (k == n_rec - 1 ? 3 : c.C) && r.H >= 1 && r.H < 65536 && r.W >= 1 && r.W < 65536 && r.L >= 64 && r.L % 64 == 0 &&
             r.L <= 0xFFFFFFFFll && r.n == (r.H * r.W + r.L - 1) / r.L && r.n <= MAX_BANDS && out->B * r.n <= MAX_BAND_STREAMS &&
             r.max_nbytes >= 0 && r.max_nbytes <= 0xFFFFFFFFll && (k == 0 || (r.H == 2 * out->rec[k - 1].H && r.W == 2 * out->rec[k - 1].W));
    }
    if (!ok) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: inconsistent header");
    BandedHeader want = *out;
    banded_layout(want);
    const BandedRecord &rgb = out->rec[n_rec - 1];
    ok = want.bytes == out->bytes && want.n_streams == out->n_streams && want.src_off == out->src_off && want.dst_off == out->dst_off &&
         want.nbytes_off == out->nbytes_off && memcmp(want.entries_off, out->entries_off, sizeof(want.entries_off)) == 0 &&
         out->dst_bytes >= 4 * out->n_streams && out->files_bytes >= 0 && out->H == rgb.H && out->W == rgb.W && out->rgb_band_len == rgb.L &&
         out->rgb_chunks == rgb_band_chunks(rgb.H * rgb.W, rgb.L, rgb.n) && out->lag == (out->B * rgb.n >= 16 ? 2 : 1);
    for (int k = 0; k < n_rec && ok; ++k) ok = want.rec[k].first == out->rec[k].first && want.rec[k].n_streams == out->rec[k].n_streams;
    if (!ok) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: inconsistent header");
    if (plan_cap >= 0 && plan_cap < out->bytes)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_bytes too small: %lld < %lld", plan_cap, out->bytes);
    return L3C_OK;
}

// One stream entry of a blob, for callers that must not restate the layout above: stream `index` of record `record` (coarsest first), numbered
// inside the record as the blob numbers them -- band (b, c, j) of the finest record is (c B + b) n + j.  The header is checked against the layout
// its own B and records imply before an offset of it is used, and the entry against dst_bytes.
inline int banded_stream(const void *plan_host, int record, int64_t index, int64_t *src_out, int64_t *dst_out, uint32_t *nbytes_out, char *err,
                         size_t cap) {
    if (!plan_host || !src_out || !dst_out || !nbytes_out) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer");
    if (reinterpret_cast<uintptr_t>(plan_host) & 7) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_host must be 8-byte aligned");
    int64_t magic;
    memcpy(&magic, plan_host, sizeof(magic));
    if (magic != BANDED_MAGIC) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: wrong magic word (not written by l3c_decode_plan_banded)");
    BandedHeader h;
    memcpy(&h, plan_host, sizeof(h));
    bool ok = h.B >= 1 && h.B < 65536 && h.n_records >= 2 && h.n_records <= MAX_RECORDS && h.dst_bytes >= 0;
    for (int k = 0; ok && k < (int)h.n_records; ++k)
        ok = h.rec[k].C >= 1 && h.rec[k].C <= 255 && h.rec[k].n >= 1 && h.rec[k].n <= MAX_BANDS && h.B * h.rec[k].n <= MAX_BAND_STREAMS;
    if (ok) {
        BandedHeader want = h;
        banded_layout(want);
        ok = want.bytes == h.bytes && want.n_streams == h.n_streams && want.src_off == h.src_off && want.dst_off == h.dst_off &&
             want.nbytes_off == h.nbytes_off;
        for (int k = 0; ok && k < (int)h.n_records; ++k) ok = want.rec[k].first == h.rec[k].first && want.rec[k].n_streams == h.rec[k].n_streams;
    }
    if (!ok) return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: inconsistent header");
    if (record < 0 || record >= (int)h.n_records)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "record %lld: the plan has %lld records", (long long)record, h.n_records);
    const BandedRecord &r = h.rec[record];
    if (index < 0 || index >= r.n_streams)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "stream %lld: record %lld has %lld streams", index, (long long)record, r.n_streams);
    const uint8_t *blob = static_cast<const uint8_t *>(plan_host);
    const int64_t s = r.first + index;
    int64_t src, dst;
    uint32_t nb;
    memcpy(&src, blob + h.src_off + 8 * s, 8);
    memcpy(&dst, blob + h.dst_off + 8 * s, 8);
    memcpy(&nb, blob + h.nbytes_off + 4 * s, 4);
    if (src < 0 || dst < 0 || dst % 4 != 0 || dst > h.dst_bytes || ((int64_t)nb + 3) / 4 * 4 + 4 > h.dst_bytes - dst)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: stream %lld lies outside the stream buffer", s);
    *src_out = src, *dst_out = dst, *nbytes_out = nb;
    return L3C_OK;
}

}  // namespace l3c_plan

#endif
