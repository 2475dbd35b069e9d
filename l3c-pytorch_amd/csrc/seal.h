// seal.h -- the 24-byte seal behind a `.l3c` file's last separator (include/l3c_hip.h: l3c_seal_find / l3c_seal_write; the Python mirror is
// bitcoding/container.py: split_seal / make_seal).
//
// Plain C++17 on purpose, as codec_plan.h and image_table.h: no HIP include, no library call, no allocation, so that the code that reads
// untrusted file bytes compiles into a stand-alone program (tests/cabi/seal_check_main.cpp, built with the address and undefined-behaviour
// sanitizers) as well as into libl3c_hip.so (csrc/crc.hip).
//
//     0 'L3CS' | 4 u8 version = 1 | 5 u8 flags = 0 | 6 u16 generation | 8 u32 frame CRC | 12 u64 model id | 20 u32 check        little-endian
//
// check = CRC-32 (zlib) of the file's 8 padding bytes -- file bytes 0..7, in a banded file ('L3CB') bytes 6..13 -- followed by seal bytes
// 0..19.  A file is SEALED exactly when it has at least 28 bytes, bytes [-24, -20) are 'L3CS' and bytes [-28, -24) are the scale separator
// every unsealed file ends with; a recognised seal that is damaged is an error, never "unsealed".
//
// Version 2, the BAND SEAL (banded files only): body | BAND TABLE | the 24 seal bytes with version = 2.  The table, T = 20 + 12 n bytes:
//
//     0 'L3CT' | 4 u16 n | 6 u16 0 | 8 u32 L | 12 u32 crc[3][n] (channel-major) | 12 + 12 n u32 T | 16 + 12 n separator 46 E2 84 92
//
// n, L: bands per channel and band length of the finest record; crc[c][j]: the CRC-32 of bytes [c HW + j L, c HW + min((j + 1) L, HW)) of
// the padded planar frame.  The table ends with the separator, so the recognition rule above holds for both versions, and T lies at
// file[-32:-28]: the table is found from the end.  check = CRC-32 of the 8 padding bytes, the whole table, seal bytes 0..19.  The frame CRC
// stays in the seal and must be the combination of the band CRCs (crc32_combine's arithmetic, crc_spans.h).
//
// Version 3, PARITY BANDS: body | PARITY SECTION | BAND TABLE | the 24 seal bytes with version = 3.  The section, S = 16 + 12 m + sum(plen):
//
//     0 'L3CP' | 4 u16 G | 6 u16 m | 8 u32 plen[3][m] (channel-major) | 8 + 12 m the 3 m parity payloads, (c, g) order | S - 8 u32 S | S - 4 separator
//
// m = ceil(n / G); group g of channel c holds the bands { j : j % m == g }; its payload is the XOR of the members' payloads, each
// zero-extended to plen[c][g], the longest member's byte count.  check = CRC-32 of the 8 padding bytes, section bytes [0, 8 + 12 m), the
// section's last 8 bytes, the band table, seal bytes 0..19: the parity payloads are NOT under it.
//
// Version 3 with R = 2..4 parity streams per group carries a section of a second kind, S = 20 + 12 m + R sum(plen):
//
//     0 'L3CQ' | 4 u16 G | 6 u16 m | 8 u16 R | 10 u16 0 | 12 u32 plen[3][m] | 12 + 12 m the 3 m R payloads, (c, g, r) order, plen[c][g] bytes each | S - 8 u32 S | S - 4 separator
//
// Row r of group g is the XOR over its members k (band j = g + k m) of (alpha^k)^r d_k in GF(2^8), polynomial 0x11D, alpha = 0x02; row 0 is the
// 'L3CP' payload.  G <= 255 so that the points alpha^k of a group are distinct.  check covers section bytes [0, 12 + 12 m) and the last 8.
// R = 1 is always written as 'L3CP'.  find_parity reports an 'L3CQ' section as m = 0 (the band-sealed file it contains); find_parity_rs
// reports both kinds, 'L3CP' as R = 1.
//
// Version 3 with HEAD PARITY carries a section of a third kind, 'L3CH': the 'L3CQ' layout for every R in 1..4, with a HEAD PART between the
// finest record's rows and the section's last 8 bytes.  "Head" is everything in the body that is not a band payload of the finest record.
//
//     0 'L3CH' | 4 u16 G | 6 u16 m | 8 u16 R (1..4) | 10 u16 0 | 12 u32 plen[3][m] | 12 + 12 m the 3 m R finest rows, (c, g, r) order |
//     A = 12 + 12 m + R sum(plen): HEAD PART | S - 8 u32 S | S - 4 separator
//
//     HEAD PART:  u16 n_records (all scale records, the finest included) | u16 0
//                 FRAMING COPY: body[0:14]; per record, coarsest first: its 9 header bytes (u8 C, u16 H, u16 W, u32 L) and u32 nbytes[C][n]
//                 u32 head_crc = CRC-32 of body[0, P0), P0 where the finest record's header starts
//                 per head record k (every record but the finest): u32 crc[C][n_k], the CRC-32 of each band PAYLOAD | u16 G_k = min(G, n_k) |
//                     u16 m_k = ceil(n_k / G_k) | u32 hplen[C][m_k], the longest member of each group
//                 the rows: per head record, (c, g, r) order, hplen[k][c][g] bytes each -- groups, points and zero extension as above
//                 u32 head_check = CRC-32 of the head part from A up to the first row byte
//
// check covers what it covers for 'L3CQ' -- section bytes [0, 12 + 12 m) and the last 8 --, the head part is guarded by head_check alone.
// A head part that cannot be walked or whose head_check fails is DAMAGED, never an error: every reader goes on as for the 'L3CQ' file
// (find_parity: m = 0; find_parity_rs: the finest rows; find_head: check_ok = 0).  One whose check holds but whose content contradicts
// itself, the band table or the body's size is "invalid file: seal head ..." (check_head).  This header reads the section; writing it and
// healing a file from it are container.make_seal(head=...) and container.heal_head.
//
// ONE writer (write_tail) lays down every tail -- [section] [table] seal, whatever is present -- and ONE reader (find_tail) takes it
// apart; the sections are one layout whose signature and head length (section_head_bytes) depend on the kind.  write, write_bands,
// write_parity, write_parity_rs and find, find_bands, find_parity, find_parity_rs, find_head are those two under the names of the format's
// versions.
#ifndef L3C_SEAL_H_
#define L3C_SEAL_H_

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/l3c_hip.h"
#include "crc_spans.h"

namespace l3c_sealing {

constexpr int VERSION = 1, VERSION_BANDS = 2, VERSION_PARITY = 3, MAX_BANDS = 1024;
constexpr uint8_t TABLE_SIGNATURE[4] = {'L', '3', 'C', 'T'};
constexpr uint8_t PARITY_SIGNATURE[4] = {'L', '3', 'C', 'P'};
constexpr uint8_t PARITY_RS_SIGNATURE[4] = {'L', '3', 'C', 'Q'};
constexpr uint8_t HEAD_SIGNATURE[4] = {'L', '3', 'C', 'H'};
constexpr int MAX_PARITY_STREAMS = 4, MAX_RS_GROUP = 255;
constexpr uint8_t SIGNATURE[4] = {'L', '3', 'C', 'S'};
constexpr uint8_t SEPARATOR[4] = {0x46, 0xE2, 0x84, 0x92};
constexpr uint8_t BANDED_SIGNATURE[4] = {'L', '3', 'C', 'B'};

// zlib's CRC-32, bit by bit: the seal hashes 28 bytes
inline uint32_t crc32(uint32_t crc, const uint8_t *p, int64_t n) {
    crc = ~crc;
    for (int64_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

inline void put(uint8_t *dst, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; ++i) dst[i] = (uint8_t)(v >> (8 * i));
}

inline uint64_t get(const uint8_t *src, int bytes) {
    uint64_t v = 0;
    for (int i = 0; i < bytes; ++i) v |= (uint64_t)src[i] << (8 * i);
    return v;
}

inline int fail(char *err, size_t cap, const char *what) {
    if (err && cap) snprintf(err, cap, "invalid file: seal %s", what);
    return L3C_ERR_INVALID_ARG;
}

// `what` is a format with one %d
inline int fail_d(char *err, size_t cap, const char *what, int d) {
    if (err && cap) {
        const int at = snprintf(err, cap, "invalid file: seal ");
        if (at > 0 && (size_t)at < cap) snprintf(err + at, cap - (size_t)at, what, d);
    }
    return L3C_ERR_INVALID_ARG;
}

// the tail of a file behind its body: [parity section] [band table] the 24 seal bytes.  table_bytes(n): the table of n bands per channel;
// section_head_bytes(R): the section's bytes in front of its plen fields, 8 ('L3CP', R = 1) or 12 ('L3CQ', R = 2..4) -- with the signature
// the only difference between the two sections; parity_section_bytes(m, R, sum of plen): a section of m groups per channel and R rows per group
constexpr int64_t table_bytes(int64_t n) { return 20 + 12 * n; }
constexpr int64_t section_head_bytes(int64_t R) { return R == 1 ? 8 : 12; }
constexpr int64_t parity_section_bytes(int64_t m, int64_t R, int64_t plen_sum) { return section_head_bytes(R) + 12 * m + R * plen_sum + 8; }
// (the names the two sections' sizes had before there was one function)
constexpr int64_t section_bytes(int64_t m, int64_t payload_bytes) { return parity_section_bytes(m, 1, payload_bytes); }
constexpr int64_t rs_section_bytes(int64_t m, int64_t R, int64_t plen_sum) { return parity_section_bytes(m, R, plen_sum); }

// zlib's crc32_combine over the bands of a frame of 3 planes of hw bytes: crc(A | B) = crc(A) x^(8 |B|) + crc(B), from crc() = 0.
// crc: 12 n bytes, [3][n] little-endian words, unaligned
inline uint32_t combine_bands(const uint8_t *crc, int64_t n, uint32_t band_len, int64_t hw) {
    const uint32_t k_full = l3c_crc::powmod(l3c_crc::X8, band_len), k_last = l3c_crc::powmod(l3c_crc::X8, (uint64_t)(hw - (n - 1) * (int64_t)band_len));
    uint32_t a = 0;
    for (int c = 0; c < 3; ++c)
        for (int64_t j = 0; j < n; ++j) a = l3c_crc::mulmod(a, j + 1 < n ? k_full : k_last) ^ (uint32_t)get(crc + 4 * (c * n + j), 4);
    return a;
}

// The finest (last) scale record of the banded file in [0, body): its H W, band length and bands per channel, walked by the length fields.
// false: not a banded file whose records end exactly at `body`.
inline bool finest_record(const uint8_t *f, int64_t body, int64_t *hw_out, uint32_t *band_len_out, int64_t *n_out, int64_t *C_out = nullptr,
                          int64_t *first_len_at_out = nullptr) {
    if (body < 14 || memcmp(f, BANDED_SIGNATURE, 4) != 0) return false;
    int64_t p = 14;
    bool found = false;
    while (p < body) {
        if (body - p < 9) return false;
        const int64_t C = f[p], hw = (int64_t)get(f + p + 1, 2) * (int64_t)get(f + p + 3, 2), L = (int64_t)get(f + p + 5, 4);
        p += 9;
        if (C == 0 || hw == 0 || L == 0 || L % 64) return false;
        const int64_t n = (hw + L - 1) / L;
        if (n > MAX_BANDS) return false;
        if (C_out) *C_out = C;
        if (first_len_at_out) *first_len_at_out = p;
        for (int64_t k = 0; k < C * n; ++k) {
            if (body - p < 4) return false;
            const int64_t len = (int64_t)get(f + p, 4);
            p += 4;
            if (len > body - p) return false;
            p += len;
        }
        if (body - p < 4 || memcmp(f + p, SEPARATOR, 4) != 0) return false;
        p += 4;
        *hw_out = hw, *band_len_out = (uint32_t)L, *n_out = n;
        found = true;
    }
    return found;
}

// The band table of a tail: band_crc, 12 n bytes, [3][n] little-endian words (unaligned is fine; may already lie where the table puts them)
struct TailTable {
    const uint8_t *band_crc;
    int n;
    uint32_t band_len;
};

// The parity section of a tail: m groups per channel, R rows per group; plen: [3][m] host words; payloads: the 3 m R payloads back to back,
// (c, g, r) order, plen[c][g] bytes each.  R == 1 is the 'L3CP' section, R in 2..4 the 'L3CQ' one.
struct TailSection {
    int G, m, R;
    const uint32_t *plen;
    const uint8_t *payloads;
};

// THE writer of every tail: [section] [table] seal at dst, of the version that what is present makes (1: neither, 2: a table, 3: both; a
// section needs a table).  check = CRC-32 of padding8, the section's head and its last 8 bytes, the table, seal bytes 0..19.  dst must not
// overlap the payloads; the band CRCs may lie at their place in dst already.
inline void write_tail(const l3c_seal &s, const uint8_t *padding8, const TailTable *table, const TailSection *section, uint8_t *dst) {
    uint32_t check = crc32(0, padding8, 8);
    if (section) {
        const int64_t m = section->m, R = section->R, fields_at = section_head_bytes(R), head = fields_at + 12 * m;
        int64_t sum = 0;
        for (int i = 0; i < 3 * m; ++i) sum += section->plen[i];
        const int64_t S = parity_section_bytes(m, R, sum);
        memcpy(dst, R == 1 ? PARITY_SIGNATURE : PARITY_RS_SIGNATURE, 4);
        put(dst + 4, (uint64_t)section->G, 2);
        put(dst + 6, (uint64_t)m, 2);
        if (R != 1) put(dst + 8, (uint64_t)R, 4);                     // u16 R | u16 0
        for (int i = 0; i < 3 * m; ++i) put(dst + fields_at + 4 * i, section->plen[i], 4);
        if (sum) memcpy(dst + head, section->payloads, (size_t)(R * sum));
        put(dst + S - 8, (uint64_t)S, 4);
        memcpy(dst + S - 4, SEPARATOR, 4);
        check = crc32(crc32(check, dst, head), dst + S - 8, 8);
        dst += S;
    }
    if (table) {
        const int64_t n = table->n, T = table_bytes(n);
        memcpy(dst, TABLE_SIGNATURE, 4);
        put(dst + 4, (uint64_t)n, 2);
        put(dst + 6, 0, 2);
        put(dst + 8, table->band_len, 4);
        memmove(dst + 12, table->band_crc, 12 * (size_t)n);
        put(dst + 12 + 12 * n, (uint64_t)T, 4);
        memcpy(dst + 16 + 12 * n, SEPARATOR, 4);
        check = crc32(check, dst, T);
        dst += T;
    }
    memcpy(dst, SIGNATURE, 4);
    dst[4] = section ? VERSION_PARITY : table ? VERSION_BANDS : VERSION;
    dst[5] = 0;
    put(dst + 6, s.generation, 2);
    put(dst + 8, s.frame_crc, 4);
    put(dst + 12, s.model_id, 8);
    put(dst + 20, crc32(check, dst, 20), 4);
}

// the four tails by name: the 24 seal bytes; table_bytes(n) + 24 bytes; parity_section_bytes(m, R, sum of plen) + table_bytes(n) + 24 bytes
inline void write(const l3c_seal &s, const uint8_t *padding8, uint8_t *dst) { write_tail(s, padding8, nullptr, nullptr, dst); }

inline void write_bands(const l3c_seal &s, const uint8_t *padding8, const uint8_t *band_crc, int n, uint32_t band_len, uint8_t *dst) {
    const TailTable table{band_crc, n, band_len};
    write_tail(s, padding8, &table, nullptr, dst);
}

inline void write_parity_rs(const l3c_seal &s, const uint8_t *padding8, const uint8_t *band_crc, int n, uint32_t band_len, int G, int m, int R,
                            const uint32_t *plen, const uint8_t *payloads, uint8_t *dst) {
    const TailTable table{band_crc, n, band_len};
    const TailSection section{G, m, R, plen, payloads};
    write_tail(s, padding8, &table, &section, dst);
}

inline void write_parity(const l3c_seal &s, const uint8_t *padding8, const uint8_t *band_crc, int n, uint32_t band_len, int G, int m,
                         const uint32_t *plen, const uint8_t *payloads, uint8_t *dst) {
    write_parity_rs(s, padding8, band_crc, n, band_len, G, m, 1, plen, payloads, dst);
}

// The HEAD PART of an 'L3CH' section, hp[0, hbytes): walked field by field.  *check_ok = 0 (and L3C_OK) where it cannot be walked -- a
// count or a header no writer produces, a field past its end -- or its head_check does not hold: a DAMAGED head part never makes a file
// unreadable.  A head part whose check holds but whose content contradicts itself, the band table (n, band_len) or the body's size is
// L3C_ERR_INVALID_ARG, "invalid file: seal head ...".  G, R: the section's.
constexpr int MAX_HEAD_RECORDS = 16;
inline int check_head(const uint8_t *hp, int64_t hbytes, int64_t body, int64_t G, int64_t R, int64_t n, uint32_t band_len, int *check_ok,
                      int *n_records_out, char *err, size_t cap) {
    *check_ok = 0;
    if (n_records_out) *n_records_out = 0;
    const int64_t end = hbytes - 4;                                // where head_check lies
    int64_t pos = 4 + 14;
    if (pos > end) return L3C_OK;
    const int64_t records = (int64_t)get(hp, 2);
    if (records < 1 || records > MAX_HEAD_RECORDS) return L3C_OK;
    int64_t C[MAX_HEAD_RECORDS], bands[MAX_HEAD_RECORDS], lens_at[MAX_HEAD_RECORDS], total = 14;
    uint32_t L_finest = 0;
    for (int64_t k = 0; k < records; ++k) {
        if (pos + 9 > end) return L3C_OK;
        const int64_t hw = (int64_t)get(hp + pos + 1, 2) * (int64_t)get(hp + pos + 3, 2), L = (int64_t)get(hp + pos + 5, 4);
        C[k] = hp[pos];
        if (C[k] == 0 || hw == 0 || L == 0 || L % 64) return L3C_OK;
        bands[k] = (hw + L - 1) / L;
        if (bands[k] > MAX_BANDS) return L3C_OK;
        pos += 9;
        lens_at[k] = pos;
        if (4 * C[k] * bands[k] > end - pos) return L3C_OK;
        total += 9 + 4 * C[k] * bands[k] + 4;
        for (int64_t i = 0; i < C[k] * bands[k]; ++i) total += (int64_t)get(hp + pos + 4 * i, 4);
        pos += 4 * C[k] * bands[k];
        L_finest = (uint32_t)L;
    }
    pos += 4;                                                      // head_crc
    int64_t rows = 0, groups_at[MAX_HEAD_RECORDS];
    for (int64_t k = 0; k + 1 < records; ++k) {
        if (4 * C[k] * bands[k] + 4 > end - pos) return L3C_OK;
        pos += 4 * C[k] * bands[k];
        groups_at[k] = pos;
        const int64_t m = (int64_t)get(hp + pos + 2, 2);
        pos += 4;
        if (m < 1 || m > bands[k] || 4 * C[k] * m > end - pos) return L3C_OK;
        for (int64_t i = 0; i < C[k] * m; ++i) rows += R * (int64_t)get(hp + pos + 4 * i, 4);
        pos += 4 * C[k] * m;
    }
    if (pos > end || crc32(0, hp, pos) != (uint32_t)get(hp + end, 4)) return L3C_OK;
    *check_ok = 1;
    if (n_records_out) *n_records_out = (int)records;
    if (get(hp + 2, 2) != 0) return fail(err, cap, "head with a non-zero reserved field");
    if (records < 2) return fail_d(err, cap, "head states %d scale record(s)", (int)records);
    if (pos + rows != end) return fail(err, cap, "head length is not the one its fields add up to");
    if (C[records - 1] != 3 || bands[records - 1] != n || L_finest != band_len)
        return fail(err, cap, "head copy of the finest record does not match the band table");
    if (total != body) return fail(err, cap, "head copy adds up to another body length");
    for (int64_t k = 0; k + 1 < records; ++k) {
        const int64_t Gk = G < bands[k] ? G : bands[k], m = (bands[k] + Gk - 1) / Gk;
        if ((int64_t)get(hp + groups_at[k], 2) != Gk || (int64_t)get(hp + groups_at[k] + 2, 2) != m)
            return fail(err, cap, "head states a group size or count that is not min(G, n) and ceil(n / G)");
        for (int64_t c = 0; c < C[k]; ++c)
            for (int64_t g = 0; g < m; ++g) {
                uint32_t longest = 0;
                for (int64_t j = g; j < bands[k]; j += m) {
                    const uint32_t len = (uint32_t)get(hp + lens_at[k] + 4 * (c * bands[k] + j), 4);
                    if (len > longest) longest = len;
                }
                if ((uint32_t)get(hp + groups_at[k] + 4 + 4 * (c * m + g), 4) != longest)
                    return fail(err, cap, "head states a payload length that is not its longest member's");
            }
    }
    return L3C_OK;
}

// where the head part of an 'L3CH' section lies in its file; at = 0: the file has none
struct HeadAt {
    int64_t at, bytes;
    int check_ok, n_records;
};

// 1: sealed, 0: unsealed, L3C_ERR_INVALID_ARG (message in err): a recognised seal that is damaged.  *body_bytes_out: the bytes in front of
// the seal, in front of the band table where the seal has one, in front of the parity section where it has one.  bands_out (may be null):
// n = 0 for a version-1 seal.  parity_out (may be null): m = 0 unless the seal is of version 3; R = 1 for an 'L3CP' section, 2..4 for 'L3CQ',
// 1..4 for 'L3CH' (the finest record's rows).  head_out (may be null): the head part of an 'L3CH' section.
inline int find_tail(const uint8_t *file, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out,
                     l3c_seal_parity_rs *parity_out, HeadAt *head_out, char *err, size_t cap) {
    if (head_out) head_out->at = 0, head_out->bytes = 0, head_out->check_ok = 0, head_out->n_records = 0;
    if (body_bytes_out) *body_bytes_out = file_bytes;
    if (bands_out) bands_out->n = 0, bands_out->band_len = 0, bands_out->crc = nullptr;
    if (parity_out)
        parity_out->G = 0, parity_out->m = 0, parity_out->R = 0, parity_out->plen = nullptr, parity_out->payloads = nullptr, parity_out->payload_bytes = 0;
    if (file_bytes < L3C_SEAL_BYTES + 4) return 0;
    const uint8_t *s = file + file_bytes - L3C_SEAL_BYTES;
    if (memcmp(s, SIGNATURE, 4) != 0 || memcmp(s - 4, SEPARATOR, 4) != 0) return 0;
    int64_t body = file_bytes - L3C_SEAL_BYTES;
    const bool banded = memcmp(file, BANDED_SIGNATURE, 4) == 0;
    const int64_t padding_at = banded ? 6 : 0;
    const int version = s[4];
    if (version != VERSION && version != VERSION_BANDS && version != VERSION_PARITY) return fail(err, cap, "of an unknown version");
    int64_t T = 0, n = 0, S = 0, m = 0, G = 0, R = 0, fields_at = section_head_bytes(1), table_at = 0;      // fields_at: where plen starts inside the section
    int64_t plen_sum = 0;
    bool hd = false;                                           // an 'L3CH' section: a head part follows the finest record's rows
    if (version != VERSION) {
        if (!banded)
            return fail(err, cap, version == VERSION_BANDS ? "of an unknown version for a legacy file (version 2, the band seal, needs a banded file)"
                                                           : "of an unknown version for a legacy file (version 3, the parity seal, needs a banded file)");
        if (body < 20 + 12 + 4) return fail_d(err, cap, "of an unknown version: %d needs a band table, and the file is too short for one", version);
        T = (int64_t)get(s - 8, 4);
        n = (T - 20) / 12;
        if (T < 20 || (T - 20) % 12 != 0 || n < 1 || n > MAX_BANDS)
            return fail_d(err, cap, "of an unknown version: %d needs a band table, and its length field is not 20 + 12 n with 1 <= n <= 1024", version);
        if (T > body - 14 - 4 || memcmp(file + body - T - 4, SEPARATOR, 4) != 0)
            return fail(err, cap, "band table does not start behind the file's last scale separator");
        body -= T;
        table_at = body;
        const uint8_t *t = file + body;
        if (memcmp(t, TABLE_SIGNATURE, 4) != 0) return fail(err, cap, "band table without its 'L3CT' signature");
        if (get(t + 6, 2) != 0) return fail(err, cap, "band table with a non-zero reserved field");
    }
    if (version == VERSION_PARITY) {
        S = (int64_t)get(file + body - 8, 4);                  // (the separator at [body - 4, body) is the one the table starts behind)
        if (S < parity_section_bytes(1, 1, 0) || S > body - 14 - 4 || memcmp(file + body - S - 4, SEPARATOR, 4) != 0)
            return fail(err, cap, "parity section does not start behind the file's last scale separator");
        body -= S;
        const uint8_t *p = file + body;
        hd = memcmp(p, HEAD_SIGNATURE, 4) == 0;
        const bool rs = hd || memcmp(p, PARITY_RS_SIGNATURE, 4) == 0;
        if (!rs && memcmp(p, PARITY_SIGNATURE, 4) != 0) return fail(err, cap, "parity section without its 'L3CP' signature");
        G = (int64_t)get(p + 4, 2), m = (int64_t)get(p + 6, 2), R = 1;
        if (rs) fields_at = section_head_bytes(2);
        if (m < 1 || fields_at + 8 + 12 * m > S) return fail_d(err, cap, "parity section is too short for its %d x 3 length fields", (int)m);
        if (rs) {
            R = (int64_t)get(p + 8, 2);
            if (hd && (R < 1 || R > MAX_PARITY_STREAMS))
                return fail_d(err, cap, "parity section states %d parity streams, an 'L3CH' section holds 1..4", (int)R);
            if (!hd && (R < 2 || R > MAX_PARITY_STREAMS))
                return fail_d(err, cap, "parity section states %d parity streams, an 'L3CQ' section holds 2..4", (int)R);
            if (get(p + 10, 2) != 0) return fail(err, cap, "parity section with a non-zero reserved field");
        }
        for (int64_t i = 0; i < 3 * m; ++i) plen_sum += (int64_t)get(p + fields_at + 4 * i, 4);
        if (hd && S < parity_section_bytes(m, R, plen_sum))
            return fail(err, cap, "parity section length is less than 20 + 12 m + R times the sum of its payload lengths");
        if (!hd && S != parity_section_bytes(m, R, plen_sum))
            return fail(err, cap, rs ? "parity section length is not 20 + 12 m + R times the sum of its payload lengths"
                                     : "parity section length is not 16 + 12 m + the sum of its payload lengths");
    }
    if (s[5] != 0) return fail(err, cap, "with non-zero flags");
    if (padding_at + 8 > body) return fail(err, cap, "on a file too short for its padding fields");
    {
        uint32_t c = crc32(0, file + padding_at, 8);
        if (S) c = crc32(crc32(c, file + body, fields_at + 12 * m), file + body + S - 8, 8);
        if (get(s + 20, 4) != crc32(crc32(c, file + table_at, T), s, 20))
            return fail(err, cap, "check word does not match (damaged seal or padding fields)");
    }
    if (T) {
        const uint8_t *t = file + table_at;
        int64_t hw = 0, rec_n = 0, rec_C = 0, first = 0;
        uint32_t rec_len = 0;
        if ((int64_t)get(t + 4, 2) != n) return fail(err, cap, "band table states another band count than its length");
        if (!finest_record(file, body, &hw, &rec_len, &rec_n, &rec_C, &first) || rec_n != n || rec_len != (uint32_t)get(t + 8, 4))
            return fail(err, cap, "band table does not match the bands of the file's finest scale record");
        if ((uint32_t)get(s + 8, 4) != combine_bands(t + 12, n, rec_len, hw)) return fail(err, cap, "frame CRC is not the combination of its band CRCs");
        if (S) {
            const uint8_t *p = file + body;
            if (rec_C != 3 || G < 1 || G > n || m != (n + G - 1) / G)
                return fail(err, cap, "parity section does not match the bands of the file's finest scale record");
            if (R > 1 && G > MAX_RS_GROUP) return fail(err, cap, "parity section with more than one stream over groups of more than 255 bands");
            // every plen[c][g] against the length fields of its members, band j of channel c in group j % m (finest_record has walked them)
            int64_t at = first;
            for (int64_t c = 0; c < 3; ++c) {
                uint32_t longest[MAX_BANDS];
                for (int64_t g = 0; g < m; ++g) longest[g] = 0;
                for (int64_t j = 0; j < n; ++j) {
                    const uint32_t len = (uint32_t)get(file + at, 4);
                    at += 4 + (int64_t)len;
                    if (len > longest[j % m]) longest[j % m] = len;
                }
                for (int64_t g = 0; g < m; ++g)
                    if ((uint32_t)get(p + fields_at + 4 * (c * m + g), 4) != longest[g])
                        return fail(err, cap, "parity section states a payload length that is not its longest member's");
            }
            if (hd) {
                const int64_t A = fields_at + 12 * m + R * plen_sum;              // the head part: section bytes [A, S - 8)
                int ok = 0, records = 0;
                const int rc = check_head(p + A, S - 8 - A, body, G, R, n, rec_len, &ok, &records, err, cap);
                if (rc != L3C_OK) return rc;
                if (head_out) head_out->at = body + A, head_out->bytes = S - 8 - A, head_out->check_ok = ok, head_out->n_records = records;
            }
            if (parity_out)
                parity_out->G = (int32_t)G, parity_out->m = (int32_t)m, parity_out->R = (int32_t)R, parity_out->plen = p + fields_at,
                parity_out->payloads = p + fields_at + 12 * m, parity_out->payload_bytes = R * plen_sum;
        }
        if (bands_out) bands_out->n = (int32_t)n, bands_out->band_len = rec_len, bands_out->crc = t + 12;
    }
    if (body_bytes_out) *body_bytes_out = body;
    if (seal_out) {
        seal_out->generation = (uint16_t)get(s + 6, 2);
        seal_out->frame_crc = (uint32_t)get(s + 8, 4);
        seal_out->model_id = get(s + 12, 8);
    }
    return 1;
}

// find_tail without the head part: the finest record's rows of every section kind
inline int find_parity_rs(const uint8_t *file, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out,
                          l3c_seal_parity_rs *parity_out, char *err, size_t cap) {
    return find_tail(file, file_bytes, body_bytes_out, seal_out, bands_out, parity_out, nullptr, err, cap);
}

// 1: a sealed file with an 'L3CH' section (head_out: its head part), 0: any other file, L3C_ERR_INVALID_ARG: as find_tail
inline int find_head(const uint8_t *file, int64_t file_bytes, HeadAt *head_out, char *err, size_t cap) {
    HeadAt head;
    const int rc = find_tail(file, file_bytes, nullptr, nullptr, nullptr, nullptr, &head, err, cap);
    if (head_out) *head_out = head;
    return rc == 1 ? (head.at != 0 ? 1 : 0) : rc;
}

// find_tail for callers that know the 'L3CP' section alone: an 'L3CQ' or 'L3CH' file reads as the band-sealed file it contains, m = 0
inline int find_parity(const uint8_t *file, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out,
                       l3c_seal_parity *parity_out, char *err, size_t cap) {
    l3c_seal_parity_rs rs;
    HeadAt head;
    const int rc = find_tail(file, file_bytes, body_bytes_out, seal_out, bands_out, &rs, &head, err, cap);
    if (parity_out) {
        parity_out->G = 0, parity_out->m = 0, parity_out->plen = nullptr, parity_out->payloads = nullptr, parity_out->payload_bytes = 0;
        if (rc == 1 && rs.R == 1 && head.at == 0)
            parity_out->G = rs.G, parity_out->m = rs.m, parity_out->plen = rs.plen, parity_out->payloads = rs.payloads,
            parity_out->payload_bytes = rs.payload_bytes;
    }
    return rc;
}

inline int find_bands(const uint8_t *file, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out, char *err,
                      size_t cap) {
    return find_parity(file, file_bytes, body_bytes_out, seal_out, bands_out, nullptr, err, cap);
}

inline int find(const uint8_t *file, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, char *err, size_t cap) {
    return find_parity(file, file_bytes, body_bytes_out, seal_out, nullptr, nullptr, err, cap);
}

}  // namespace l3c_sealing

#endif
