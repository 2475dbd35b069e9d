// repair_plan.h -- the planner of one ROUND of a parity repair (include/l3c_hip.h: l3c_repair_round_plan, l3c_decode_repair_round).  A sibling
// of codec_plan_region.h under the same rules: plain C++17, no HIP include, no library call, no allocation, so that it compiles into a
// stand-alone program (tests/cabi/repair_plan_check_main.cpp, built with the address and undefined-behaviour sanitizers) as well as into
// libl3c_hip.so.
//
// It restates the planning half of Bitcoding._repair (bitcoding/bitcoding.py): which groups a round rebuilds, from which window of parity
// rows, and with which coefficients (container.rs_repair_coefficients); tests/test_native_repair_abi.py compares the two.  It reads the
// files with l3c_sealing::find_parity_rs only, and the banded plan blob re-checked with that blob's own check function.
//
// THE ROUND BLOB: every array at a multiple of 16 bytes.  A RoundHeader, then at the byte offsets it names
//     files    int32 [B][2] = m | R                   the parity geometry of every file (0 | 0: no parity section)
//     groups   l3c_repair_group [n_groups]            what the round rebuilds; the caller appends them to `tried`
//     rebuild  l3c_rebuild_group [n_groups]           } the tables of l3c_band_rebuild: per group its t rows (spans of the caller's `rows`
//     src      l3c_u8_span [n_src]                    } buffer), then its present members (spans of the decode's stream area, at the plan's
//     coef     uint8 [n_src][4]                       } dst_offset); the outputs are the erased members' own slots of the stream area
//     pos      int32 [S][2] = file | band             the S distinct positions of the round, ascending
//     entries  int64 [4][S] = pixbase | hw | pix0 | len       of l3c_decode_rgb_entries: b HW | HW | j L | min(L, HW - j L)
//     in       int64 [3 S], in_nbytes uint32 [3 S]    the positions' streams in the stream area, CHANNEL-major: (c, e) at c S + e
//     crc      l3c_u8_span [3 S]                      their bands in the frames, channel-major: ((b 3 + c) HW + j L, len)
// Everything but the groups, the file geometry and the row spans follows from those three and the plan blob: round_derive writes it, the
// planner calls it, and round_check calls it again on a copy and compares, so that l3c_decode_repair_round trusts no derived word of a blob.
// The row spans are checked against `rows_bytes` by l3c_band_rebuild's own table check: a wrong one reads wrong bytes of the caller's buffer
// and the band CRCs refuse the result.
#ifndef L3C_REPAIR_PLAN_H_
#define L3C_REPAIR_PLAN_H_

#include <algorithm>

#include "codec_plan_banded.h"
#include "seal.h"

namespace l3c_repair {

using l3c_plan::BandedHeader;
using l3c_plan::fail;

constexpr int64_t ROUND_MAGIC = 0x444e554f5243334cll;     // the bytes "L3CROUND"
constexpr int MAX_T = 4;                                  // rows per group, erasures per group
constexpr int64_t MAX_BANDS = l3c_plan::MAX_BANDS;

struct RoundHeader {
    int64_t magic, bytes;          // ROUND_MAGIC; size of the blob
    int64_t B, n, HW, L;           // the frames' finest record
    int64_t n_groups, n_src, S;    // S = the sum of the groups' t: a position is the erasure of one group
    int64_t n_chunks, lag;         // of the l3c_decode_rgb_entries call
    int64_t dst_bytes;             // size of the decode's stream area
    int64_t cfg[9];
    int64_t files_off, groups_off, rebuild_off, src_off, coef_off, pos_off, entries_off, in_off, in_nbytes_off, crc_off;
};

// ---- GF(2^8), polynomial 0x11D, alpha = 0x02 (container.gf_mul / gf_pow_alpha / gf_inv) ----------------------------------------------------

inline uint8_t gf_mul(uint8_t a, uint8_t b) {
    uint8_t r = 0;
    while (b) {
        if (b & 1) r ^= a;
        b >>= 1;
        a = (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1d : 0));
    }
    return r;
}
inline uint8_t gf_pow_alpha(int64_t e) {
    uint8_t v = 1;
    for (e %= 255; e > 0; --e) v = gf_mul(v, 2);
    return v;
}
inline uint8_t gf_inv(uint8_t a) {                         // a^254; a != 0
    uint8_t r = 1;
    for (int i = 0; i < 254; ++i) r = gf_mul(r, a);
    return r;
}

// container.rs_repair_coefficients, the row half: inv[e][i] = the weight of row r0 + i in erased member ks[e] -- the inverse of the t x t
// matrix A[i][e] = alpha^(ks[e] (r0 + i)) by Gauss-Jordan.  false: singular (members that are not distinct).
inline bool rs_invert(const int64_t *ks, int t, int64_t r0, uint8_t inv[MAX_T][MAX_T]) {
    uint8_t A[MAX_T][2 * MAX_T];
    for (int i = 0; i < t; ++i)
        for (int e = 0; e < t; ++e) A[i][e] = gf_pow_alpha(ks[e] * (r0 + i)), A[i][t + e] = i == e;
    for (int col = 0; col < t; ++col) {
        int piv = col;
        while (piv < t && !A[piv][col]) ++piv;
        if (piv == t) return false;
        for (int v = 0; v < 2 * t; ++v) std::swap(A[col][v], A[piv][v]);
        const uint8_t s = gf_inv(A[col][col]);
        for (int v = 0; v < 2 * t; ++v) A[col][v] = gf_mul(s, A[col][v]);
        for (int i = 0; i < t; ++i) {
            const uint8_t f = A[i][col];
            if (i == col || !f) continue;
            for (int v = 0; v < 2 * t; ++v) A[i][v] ^= gf_mul(f, A[col][v]);
        }
    }
    for (int e = 0; e < t; ++e)
        for (int i = 0; i < t; ++i) inv[e][i] = A[e][t + i];
    return true;
}
// ... and the member half: the weight of present member k in erased member e
inline uint8_t rs_member_weight(const uint8_t inv[MAX_T][MAX_T], int e, int t, int64_t r0, int64_t k) {
    uint8_t w = 0;
    for (int i = 0; i < t; ++i) w ^= gf_mul(inv[e][i], gf_pow_alpha(k * (r0 + i)));
    return w;
}

// ---- the blob -----------------------------------------------------------------------------------------------------------------------------

inline int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }

// offsets and size from B, n_groups, n_src and S
inline void round_layout(RoundHeader &h) {
    int64_t at = up16((int64_t)sizeof(RoundHeader));
    auto take = [&](int64_t bytes) { const int64_t o = at; at = up16(at + bytes); return o; };
    h.files_off = take(8 * h.B);
    h.groups_off = take((int64_t)sizeof(l3c_repair_group) * h.n_groups);
    h.rebuild_off = take((int64_t)sizeof(l3c_rebuild_group) * h.n_groups);
    h.src_off = take(16 * h.n_src);
    h.coef_off = take(4 * h.n_src);
    h.pos_off = take(8 * h.S);
    h.entries_off = take(32 * h.S);
    h.in_off = take(24 * h.S);
    h.in_nbytes_off = take(12 * h.S);
    h.crc_off = take(48 * h.S);
    h.bytes = at;
}

// the largest blob a round over these files can take: every position the erasure of a group of its own; a group's sources are as many as its
// members (t rows stand in for the t erased ones), and a channel's groups share its n bands
inline int64_t round_bytes_bound(const BandedHeader &bh) {
    const l3c_plan::BandedRecord &r = bh.rec[bh.n_records - 1];
    RoundHeader h{};
    h.B = bh.B;
    h.n_groups = h.S = bh.B * r.n;
    h.n_src = bh.B * 3 * r.n;
    round_layout(h);
    return h.bytes;
}

struct PlanView {                 // the finest record's streams in the plan blob
    const int64_t *dst;
    const uint32_t *nbytes;
    int64_t first, B, n;
    int64_t at(int64_t c, int64_t b, int64_t j) const { return first + (c * B + b) * n + j; }
};
inline PlanView plan_view(const BandedHeader &bh, const void *plan_host) {
    const uint8_t *p = static_cast<const uint8_t *>(plan_host);
    const l3c_plan::BandedRecord &r = bh.rec[bh.n_records - 1];
    return PlanView{reinterpret_cast<const int64_t *>(p + bh.dst_off), reinterpret_cast<const uint32_t *>(p + bh.nbytes_off), r.first, bh.B, r.n};
}

// The header with B .. S, dst_bytes, cfg and the offsets set, and the files, the groups and every group's row spans in place -> everything
// else of the blob (and n_chunks, lag of the header).  The groups are untrusted here: every field is checked before it indexes anything.
inline int round_derive(const BandedHeader &bh, const void *plan_host, RoundHeader &h, uint8_t *blob, char *err, size_t cap) {
    const PlanView pv = plan_view(bh, plan_host);
    const int64_t B = h.B, n = h.n, HW = h.HW, L = h.L, S = h.S;
    const int32_t *files = reinterpret_cast<const int32_t *>(blob + h.files_off);
    const l3c_repair_group *groups = reinterpret_cast<const l3c_repair_group *>(blob + h.groups_off);
    l3c_rebuild_group *rebuild = reinterpret_cast<l3c_rebuild_group *>(blob + h.rebuild_off);
    l3c_u8_span *src = reinterpret_cast<l3c_u8_span *>(blob + h.src_off);
    uint8_t *coef = blob + h.coef_off;
    int32_t *pos = reinterpret_cast<int32_t *>(blob + h.pos_off);
    int64_t k_src = 0, k_pos = 0;
    for (int64_t q = 0; q < h.n_groups; ++q) {
        const l3c_repair_group &G = groups[q];
        if (G.file < 0 || G.file >= B || G.c < 0 || G.c > 2) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: group %lld names no channel of a file", q);
        const int64_t m = files[2 * G.file], R = files[2 * G.file + 1];
        if (m < 1 || m > n || R < 1 || R > MAX_T || G.g < 0 || G.g >= m || G.t < 1 || G.t > R || G.r0 < 0 || G.r0 > R - G.t)
            return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: group %lld does not fit the parity section of its file", q);
        const int64_t count = (n - G.g + m - 1) / m;               // members of the group: bands g, g + m, ..
        if (R > 1 && count > l3c_sealing::MAX_RS_GROUP) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: group %lld has more than 255 members", q);
        int64_t ks[MAX_T];
        for (int e = 0; e < G.t; ++e) {
            const int64_t j = G.bands[e];
            if (j < 0 || j >= n || j % m != G.g || (e && j <= G.bands[e - 1]))
                return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: group %lld: its bands must ascend inside the group", q);
            ks[e] = (j - G.g) / m;
        }
        for (int e = G.t; e < MAX_T; ++e)
            if (G.bands[e] != 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: group %lld: unused bands must be 0", q);
        if (k_src + G.t + count - G.t > h.n_src || k_pos + G.t > S) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: group %lld exceeds the blob's counts", q);
        uint8_t inv[MAX_T][MAX_T] = {};
        if (R == 1) inv[0][0] = 1;
        else if (!rs_invert(ks, G.t, G.r0, inv)) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: group %lld: singular system", q);
        l3c_rebuild_group &rb = rebuild[q];
        memset(&rb, 0, sizeof(rb));
        rb.first_src = k_src, rb.n_rows = G.t, rb.n_members = (int32_t)(count - G.t), rb.t = G.t;
        for (int i = 0; i < G.t; ++i, ++k_src)                     // the row spans are the planner's
            for (int e = 0; e < MAX_T; ++e) coef[4 * k_src + e] = e < G.t ? inv[e][i] : 0;
        for (int64_t k = 0, e_next = 0; k < count; ++k) {
            const int64_t s = pv.at(G.c, G.file, G.g + k * m);
            const l3c_u8_span span{pv.dst[s], (int64_t)pv.nbytes[s]};
            if (e_next < G.t && ks[e_next] == k) {                 // an erased member: its slot is the output
                rb.out[e_next] = span;
                pos[2 * k_pos] = G.file, pos[2 * k_pos + 1] = (int32_t)(G.g + k * m), ++k_pos, ++e_next;
                continue;
            }
            src[k_src] = span;
            for (int e = 0; e < MAX_T; ++e) coef[4 * k_src + e] = e >= G.t ? 0 : R == 1 ? 1 : rs_member_weight(inv, e, G.t, G.r0, k);
            ++k_src;
        }
    }
    if (k_src != h.n_src || k_pos != S) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: the groups do not add up to the blob's counts");
    // the positions, ascending: a position is the erasure of ONE group
    struct Pos { int32_t file, band; };
    Pos *ps = reinterpret_cast<Pos *>(pos);
    std::sort(ps, ps + S, [](const Pos &a, const Pos &b) { return a.file != b.file ? a.file < b.file : a.band < b.band; });
    for (int64_t e = 1; e < S; ++e)
        if (ps[e].file == ps[e - 1].file && ps[e].band == ps[e - 1].band) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: position %lld is in two groups", e);
    int64_t *entries = reinterpret_cast<int64_t *>(blob + h.entries_off), *in = reinterpret_cast<int64_t *>(blob + h.in_off);
    uint32_t *in_nbytes = reinterpret_cast<uint32_t *>(blob + h.in_nbytes_off);
    l3c_u8_span *crc = reinterpret_cast<l3c_u8_span *>(blob + h.crc_off);
    int64_t shortest = L;
    for (int64_t e = 0; e < S; ++e) {
        const int64_t b = ps[e].file, j = ps[e].band, len = L < HW - j * L ? L : HW - j * L;
        entries[e] = b * HW, entries[S + e] = HW, entries[2 * S + e] = j * L, entries[3 * S + e] = len;
        shortest = len < shortest ? len : shortest;
        for (int64_t c = 0; c < 3; ++c) {
            const int64_t s = pv.at(c, b, j);
            in[c * S + e] = pv.dst[s], in_nbytes[c * S + e] = pv.nbytes[s];
            crc[c * S + e] = l3c_u8_span{(b * 3 + c) * HW + j * L, len};
        }
    }
    h.n_chunks = shortest / 64 < 1 ? 1 : (shortest / 64 > l3c_plan::RGB_BAND_CHUNKS ? l3c_plan::RGB_BAND_CHUNKS : shortest / 64);
    h.lag = S >= 16 ? 2 : 1;
    memcpy(blob, &h, sizeof(h));
    return L3C_OK;
}

// the header a blob of these counts has for this plan
inline void round_header(const l3c_net_config &c, const BandedHeader &bh, int64_t n_groups, int64_t n_src, int64_t S, RoundHeader &h) {
    const l3c_plan::BandedRecord &r = bh.rec[bh.n_records - 1];
    memset(&h, 0, sizeof(h));
    h.magic = ROUND_MAGIC;
    h.B = bh.B, h.n = r.n, h.HW = r.H * r.W, h.L = r.L;
    h.n_groups = n_groups, h.n_src = n_src, h.S = S;
    h.dst_bytes = bh.dst_bytes;
    l3c_plan::cfg_words(c, h.cfg);
    round_layout(h);
}

// every stream of the finest record inside the stream area, 4-byte aligned: what round_derive copies into the tables the kernels index with
inline int check_finest_streams(const BandedHeader &bh, const void *plan_host, char *err, size_t cap) {
    const PlanView pv = plan_view(bh, plan_host);
    for (int64_t s = pv.first, e = pv.first + 3 * pv.B * pv.n; s < e; ++s)
        if (pv.dst[s] < 0 || pv.dst[s] % 4 != 0 || pv.dst[s] > bh.dst_bytes || ((int64_t)pv.nbytes[s] + 3) / 4 * 4 + 4 > bh.dst_bytes - pv.dst[s])
            return fail(err, cap, L3C_ERR_INVALID_ARG, "plan blob: stream %lld lies outside the stream buffer", s);
    return L3C_OK;
}

/*
 * One round.  files[b], file_bytes[b]: the WHOLE sealed file b as the caller holds it (after any head healing); band_words [B][3][n]: the
 * CRC words of the decoded frames' bands as they stand; section_at[b]: where the caller put the bytes of file b's parity section -- from the
 * section's signature on, i.e. file bytes [body_bytes of l3c_seal_find_parity_rs, ...) -- inside its device buffer `rows`, or -1;
 * tried[0 .. n_tried): the groups of all earlier rounds.  -> L3C_OK and the blob in round_host (n_groups == 0: nothing left to try).
 * The rule is Bitcoding._repair's: a band fails where its word differs from the file's table; the erasure of a failing position is its
 * lowest failing channel; a group (file, c, g) is taken when it holds 1..R erasures and every other member verifies at c; the window is the
 * first r0 in 0..R - t that (file, c, g, bands, r0) has not been tried with; groups in (file, c, g) order, the files of one row first.
 */
inline int make_round_plan(const l3c_net_config *cfg, const void *plan_host, const uint8_t *const *files, const int64_t *file_bytes,
                           const uint32_t *band_words, const int64_t *section_at, const l3c_repair_group *tried, int64_t n_tried, void *round_host,
                           int64_t round_cap, char *err, size_t cap) {
    int rc = l3c_plan::check_config(cfg, err, cap);
    if (rc != L3C_OK) return rc;
    if (!plan_host || !files || !file_bytes || !band_words || !section_at || !round_host || (n_tried > 0 && !tried))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer");
    if ((reinterpret_cast<uintptr_t>(plan_host) & 7) || (reinterpret_cast<uintptr_t>(round_host) & 7))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "plan_host and round_host must be 8-byte aligned");
    if (n_tried < 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "n_tried must not be negative");
    BandedHeader bh;
    rc = l3c_plan::check_blob_banded(*cfg, plan_host, -1, &bh, err, cap);
    if (rc != L3C_OK) return rc;
    rc = check_finest_streams(bh, plan_host, err, cap);
    if (rc != L3C_OK) return rc;
    const l3c_plan::BandedRecord &fr = bh.rec[bh.n_records - 1];
    const int64_t B = bh.B, n = fr.n;
    RoundHeader h;
    round_header(*cfg, bh, 0, 0, 0, h);
    if (round_cap < h.groups_off) return fail(err, cap, L3C_ERR_INVALID_ARG, "round_bytes too small: %lld < %lld (l3c_repair_round_plan_bytes)", round_cap, h.groups_off);
    uint8_t *blob = static_cast<uint8_t *>(round_host);
    memset(blob, 0, (size_t)h.groups_off);
    int32_t *geometry = reinterpret_cast<int32_t *>(blob + h.files_off);
    l3c_repair_group *groups = reinterpret_cast<l3c_repair_group *>(blob + h.groups_off);
    const int64_t groups_cap = (round_cap - h.groups_off) / (int64_t)sizeof(l3c_repair_group);
    int64_t n_groups = 0, n_src = 0, S = 0;
    // ---- the selection: the files of one row first, then the others (Python's stable sort of the groups)
    for (int pass = 0; pass < 2; ++pass)
        for (int64_t i = 0; i < B; ++i) {
            if (!files[i] || file_bytes[i] < 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "file %lld: null pointer or negative size", i);
            l3c_seal_bands bands;
            l3c_seal_parity_rs par;
            rc = l3c_sealing::find_parity_rs(files[i], file_bytes[i], nullptr, nullptr, &bands, &par, err, cap);
            if (rc < 0) return rc;
            if (rc != 1 || par.m == 0) continue;                   // unsealed, or sealed without parity: nothing to rebuild from
            if (bands.n != n || bands.band_len != (uint32_t)fr.L)
                return fail(err, cap, L3C_ERR_INVALID_ARG, "file %lld: its band table is not the plan's finest record (%lld bands)", i, n);
            const int64_t m = par.m, R = par.R;
            geometry[2 * i] = (int32_t)m, geometry[2 * i + 1] = (int32_t)R;
            if ((R > 1) != (pass == 1)) continue;
            int8_t era[MAX_BANDS];                                 // the lowest failing channel of a position, -1: all three verify
            uint8_t bad[MAX_BANDS];                                // its failing channels, a bit each
            for (int64_t j = 0; j < n; ++j) {
                era[j] = -1, bad[j] = 0;
                for (int c = 2; c >= 0; --c)
                    if (band_words[(i * 3 + c) * n + j] != (uint32_t)l3c_sealing::get(bands.crc + 4 * (c * n + j), 4)) era[j] = (int8_t)c, bad[j] |= (uint8_t)(1 << c);
            }
            for (int c = 0; c < 3; ++c)
                for (int64_t g = 0; g < m; ++g) {
                    l3c_repair_group G{};
                    bool others = false;
                    int64_t t = 0;
                    for (int64_t j = g; j < n; j += m) {
                        if (era[j] == c) {
                            if (t < MAX_T) G.bands[t] = (int32_t)j;
                            ++t;
                        } else if (bad[j] & (1 << c)) {
                            others = true;
                        }
                    }
                    if (t < 1 || t > R || others) continue;
                    G.file = (int32_t)i, G.c = c, G.g = (int32_t)g, G.t = (int32_t)t;
                    int64_t r0 = 0;
                    for (; r0 <= R - t; ++r0) {
                        G.r0 = (int32_t)r0;
                        bool seen = false;
                        for (int64_t q = 0; q < n_tried && !seen; ++q) seen = memcmp(&tried[q], &G, sizeof(G)) == 0;
                        if (!seen) break;
                    }
                    if (r0 > R - t) continue;                      // every window has been tried
                    if (section_at[i] < 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "file %lld has a group to rebuild and no section in `rows` (section_at)", i);
                    if (n_groups == groups_cap)
                        return fail(err, cap, L3C_ERR_INVALID_ARG, "round_bytes too small for more than %lld groups (l3c_repair_round_plan_bytes)", n_groups);
                    groups[n_groups++] = G;
                    n_src += (n - g + m - 1) / m;                  // t rows and the count - t present members
                    S += t;
                }
        }
    // ---- the blob: layout, the row spans, then everything that follows from them
    round_header(*cfg, bh, n_groups, n_src, S, h);                 // (the layout moves nothing in front of the rebuild table)
    if (round_cap < h.bytes) return fail(err, cap, L3C_ERR_INVALID_ARG, "round_bytes too small: %lld < %lld (l3c_repair_round_plan_bytes)", round_cap, h.bytes);
    memset(blob + h.rebuild_off, 0, (size_t)(h.bytes - h.rebuild_off));
    l3c_u8_span *src = reinterpret_cast<l3c_u8_span *>(blob + h.src_off);
    int64_t k_src = 0;
    for (int64_t q = 0; q < n_groups; ++q) {
        const l3c_repair_group &G = groups[q];
        int64_t body = 0;
        l3c_seal_parity_rs par;
        rc = l3c_sealing::find_parity_rs(files[G.file], file_bytes[G.file], &body, nullptr, nullptr, &par, err, cap);
        if (rc != 1) return rc < 0 ? rc : fail(err, cap, L3C_ERR_INVALID_ARG, "file %lld changed while it was planned", G.file);
        int64_t at = par.payloads - (files[G.file] + body), plen = 0;          // of the group's row 0 inside the section
        for (int64_t u = 0; u <= (int64_t)G.c * par.m + G.g; ++u) {
            at += par.R * plen;
            plen = (int64_t)l3c_sealing::get(par.plen + 4 * u, 4);
        }
        for (int i = 0; i < G.t; ++i) src[k_src + i] = l3c_u8_span{section_at[G.file] + at + (G.r0 + i) * plen, plen};
        k_src += (n - G.g + par.m - 1) / par.m;
    }
    return round_derive(bh, plan_host, h, blob, err, cap);
}

// What l3c_decode_repair_round checks of a round blob before it trusts a word of it: the header against the plan blob, then everything
// round_derive writes, made again in `scratch` (h.bytes bytes, 8-byte aligned) and compared.
inline int round_check(const l3c_net_config &c, const BandedHeader &bh, const void *plan_host, const void *round_host, int64_t round_cap, RoundHeader *out,
                       uint8_t *scratch, int64_t scratch_bytes, char *err, size_t cap) {
    if (!round_host) return fail(err, cap, L3C_ERR_INVALID_ARG, "null pointer: round_host");
    if (round_cap >= 0 && round_cap < (int64_t)sizeof(RoundHeader))
        return fail(err, cap, L3C_ERR_INVALID_ARG, "round_bytes too small: %lld < %lld", round_cap, (long long)sizeof(RoundHeader));
    RoundHeader h;
    memcpy(&h, round_host, sizeof(h));
    if (h.magic != ROUND_MAGIC) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: wrong magic word (not written by l3c_repair_round_plan)");
    const int64_t positions = bh.B * bh.rec[bh.n_records - 1].n;
    if (h.n_groups < 0 || h.n_groups > positions || h.S < 0 || h.S > positions || h.n_src < 0 || h.n_src > MAX_BANDS * positions)
        return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: inconsistent header");
    RoundHeader want;
    round_header(c, bh, h.n_groups, h.n_src, h.S, want);
    want.n_chunks = h.n_chunks, want.lag = h.lag;
    if (memcmp(&want, &h, sizeof(h)) != 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: inconsistent header (made for another plan or config)");
    if (round_cap >= 0 && round_cap < h.bytes) return fail(err, cap, L3C_ERR_INVALID_ARG, "round_bytes too small: %lld < %lld", round_cap, h.bytes);
    if (out) *out = h;
    if (!scratch) return L3C_OK;                                   // (the sizing call: the header alone)
    if (scratch_bytes < h.bytes) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: no room to check it (%lld < %lld)", scratch_bytes, h.bytes);
    int rc = check_finest_streams(bh, plan_host, err, cap);
    if (rc != L3C_OK) return rc;
    memcpy(scratch, round_host, (size_t)h.bytes);
    RoundHeader again = h;
    rc = round_derive(bh, plan_host, again, scratch, err, cap);
    if (rc != L3C_OK) return rc;
    if (memcmp(scratch, round_host, (size_t)h.bytes) != 0) return fail(err, cap, L3C_ERR_INVALID_ARG, "round blob: it is not what its groups and the plan imply");
    return L3C_OK;
}

}  // namespace l3c_repair

#endif
