// seal_parity_plan.h -- what csrc/seal_parity.hip and the parity entry of csrc/codec.hip decide on the host: the options of a parity seal,
// the geometry of the tail l3c_seal_append_parity writes (include/l3c_hip.h; the format is csrc/seal.h, seal version 3), the layout of
// its head part's meta bytes and of its workspace, and the bound on a tail that l3c_encode_banded_parity_file_stride adds to a slot.
//
// Plain C++17 on purpose, as parity_plan.h: no HIP include, no library call, no allocation, so that the code that decides which bytes the
// kernels may read and write compiles into a stand-alone program (tests/cabi/seal_parity_plan_check_main.cpp, built with the address and
// undefined-behaviour sanitizers) as well as into libl3c_hip.so.  The kernels trust a plan that passed.
#ifndef L3C_SEAL_PARITY_PLAN_H_
#define L3C_SEAL_PARITY_PLAN_H_

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/l3c_hip.h"

namespace l3c_parity_seal {

constexpr int MAX_RECORDS = 8;                         // records of one file: what l3c_container_write_banded and l3c_head_parity take
constexpr int THREADS = 256, TILE_DWORDS = 4 * THREADS;      // a copy block moves 1024 destination dwords of one row
constexpr int64_t MAX_STREAMS = 65535;                 // the limits of l3c_band_parity_rs and l3c_head_parity, and a grid's y and z
constexpr int MAX_BANDS = 1024;

struct Shape {                 // a record's header
    int32_t C, H, W;
    int64_t L;
};

struct Record {
    int32_t C, H, W, n, G, m;      // n bands per channel in groups of G = min(G asked for, n), m = ceil(n / G) groups per channel
    int64_t L;
};

struct Plan {
    int32_t n_records;             // the records the kernels walk, the finest LAST: all of the file with a head part, else the finest alone
    int32_t R, head;
    Record rec[MAX_RECORDS];
    int32_t front_bytes;           // the section in front of the finest rows: 8 ('L3CP') or 12 bytes, then plen[3][m]
    int32_t plen_at;               // 8 or 12
    int32_t table_bytes;           // 20 + 12 n
    int32_t check_words;           // what the seal's check word covers: padding, front, the section's last 8 bytes, table, seal words 0..4
    uint32_t signature;            // of the section, as a little-endian word
    // copy units of one file, in file order: the 3 m groups of the finest record; with a head part the meta bytes, then every group of
    // every head record.  A group is R rows of one length
    int32_t units;
    int32_t unit_first[MAX_RECORDS + 1];   // head record k: the head groups in front of it; [n_records - 1]: all
    int64_t len_first[MAX_RECORDS];        // head record k: the lengths in front of it in head_parity_nbytes (B sum C m)
    int64_t crc_first[MAX_RECORDS];        // head record k: the words in front of it in payload_crc (B sum C n)
    // the head part's meta bytes (everything in front of its rows): u16 n_records | u16 0 | body[0:14] | per record 9 header bytes and
    // u32 nbytes[C][n] | u32 head_crc | per head record u32 crc[C][n], u16 G_k, u16 m_k, u32 hplen[C][m_k]
    int32_t meta_bytes, meta_head_crc_at;
    int32_t meta_hdr_at[MAX_RECORDS], meta_crc_at[MAX_RECORDS];
    int32_t fields, field_first[MAX_RECORDS + 1];      // length fields of one file, and those in front of record k
    int64_t head_framing, finest_framing;              // body bytes that are not payload: in front of the finest record, of the finest record
    // the workspace: tail_at int64 [B] (where a file's tail starts; -1: refused) | unit_off int64 [B][units] (a unit's place in the tail) |
    // meta [B][meta_stride], each part 16-byte aligned
    int64_t ws_tail_at, ws_unit_off, ws_meta, meta_stride, ws_bytes;
    int64_t longest;               // the longest row a copy block may meet, in bytes: sizes grid.x
};

inline int plan_fail(int code, char *err, size_t cap, const char *what) {
    if (err && cap) snprintf(err, cap, "%s", what);
    return code;
}

constexpr int64_t round16(int64_t n) { return (n + 15) / 16 * 16; }
constexpr int64_t copy_tiles(int64_t longest) { return ((longest + 3) / 4 + 1 + TILE_DWORDS - 1) / TILE_DWORDS; }

// G, R, head and the reserved field of a parity seal, before anything else is looked at
inline int check_opts(int G, int R, int head, int reserved, char *err, size_t cap) {
    if (G < 1) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: G must be at least 1");
    if (R < 1 || R > 4) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: R must be in 1..4");
    if (head != 0 && head != 1) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: head must be 0 or 1");
    if (reserved != 0) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: the reserved field must be 0");
    return L3C_OK;
}

// The plan of a batch of B files whose records have these headers (coarsest first, the finest -- C == 3 -- last) -> L3C_OK, or
// L3C_ERR_INVALID_ARG / L3C_ERR_UNSUPPORTED with a message.  max_payload[k]: the largest payload of record k's bands (a coder stride);
// only `longest` depends on it.
inline int make_plan(const Shape *shapes, int n_shapes, int64_t B, int G, int R, int head, const int64_t *max_payload, Plan *out, char *err,
                     size_t cap) {
    if (!shapes || !max_payload || !out) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: null pointer");
    const int rc = check_opts(G, R, head, 0, err, cap);
    if (rc != L3C_OK) return rc;
    if (n_shapes < 1) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: at least one scale record");
    if (n_shapes > MAX_RECORDS) return plan_fail(L3C_ERR_UNSUPPORTED, err, cap, "unsupported: a parity seal takes files of at most 8 scale records");
    if (head && n_shapes < 2) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: a head part needs a record in front of the finest");
    if (B < 1 || B > MAX_STREAMS) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "bad batch size (1 .. 65535)");
    Plan p{};
    p.R = R, p.head = head;
    p.n_records = head ? n_shapes : 1;
    const int fin = p.n_records - 1;
    int64_t head_streams = 0, head_fields = 0;
    p.head_framing = 14;
    for (int k = 0; k < p.n_records; ++k) {
        const Shape &s = shapes[n_shapes - p.n_records + k];
        if (s.C < 1 || s.C > 255 || s.H < 1 || s.H > 65535 || s.W < 1 || s.W > 65535)
            return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: bad scale shape (C in 1..255, H and W fit u16)");
        if (s.L < 64 || s.L % 64 || s.L > 0xFFFFFFFFll)
            return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: band_len must be a positive multiple of 64");
        const int64_t n = ((int64_t)s.H * s.W + s.L - 1) / s.L;
        if (n > MAX_BANDS) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: more than 1024 bands per channel");
        if (k == fin && s.C != 3) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: the finest record must have 3 channels");
        if (max_payload[n_shapes - p.n_records + k] < 0) return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: negative stride");
        const int64_t Gk = G < n ? G : n, m = (n + Gk - 1) / Gk;
        if (R > 1 && Gk > 255)
            return plan_fail(L3C_ERR_INVALID_ARG, err, cap, "parity: more than one parity stream needs groups of at most 255 bands (G <= 255)");
        p.rec[k] = Record{s.C, s.H, s.W, (int32_t)n, (int32_t)Gk, (int32_t)m, s.L};
        p.field_first[k + 1] = p.field_first[k] + (int32_t)(s.C * n);
        if (k < fin) {
            p.unit_first[k + 1] = p.unit_first[k] + (int32_t)(s.C * m);
            p.len_first[k] = head_streams, p.crc_first[k] = head_fields;
            head_streams += B * s.C * m, head_fields += B * s.C * n;
            p.head_framing += 13 + 4 * s.C * n;
            if (head_streams > MAX_STREAMS)
                return plan_fail(L3C_ERR_UNSUPPORTED, err, cap,
                                 "unsupported batch: more than 65535 head parity groups (the sum of B C m over the coarser records) in one call: "
                                 "slice the batch");
        } else {
            p.finest_framing = 13 + 12 * n;
            if (B * 3 * m > MAX_STREAMS)
                return plan_fail(L3C_ERR_UNSUPPORTED, err, cap,
                                 "unsupported batch: more than 65535 parity groups (B * 3 * m) in one call: slice the batch");
        }
        if (max_payload[n_shapes - p.n_records + k] > p.longest) p.longest = max_payload[n_shapes - p.n_records + k];
    }
    p.fields = p.field_first[p.n_records];
    const Record &f = p.rec[fin];
    p.plen_at = R == 1 && !head ? 8 : 12;
    p.front_bytes = p.plen_at + 12 * f.m;
    p.table_bytes = 20 + 12 * f.n;
    p.check_words = 2 + p.front_bytes / 4 + 2 + p.table_bytes / 4 + 5;
    p.signature = head ? 0x4843334Cu : R == 1 ? 0x5043334Cu : 0x5143334Cu;      // 'L3CH', 'L3CP', 'L3CQ'
    p.units = 3 * f.m;
    if (head) {
        p.units += 1 + p.unit_first[fin];
        int32_t at = 4 + 14;
        for (int k = 0; k <= fin; ++k) {
            p.meta_hdr_at[k] = at;
            at += 9 + 4 * p.rec[k].C * p.rec[k].n;
        }
        p.meta_head_crc_at = at;
        at += 4;
        for (int k = 0; k < fin; ++k) {
            p.meta_crc_at[k] = at;
            at += 4 * p.rec[k].C * p.rec[k].n + 4 + 4 * p.rec[k].C * p.rec[k].m;
        }
        p.meta_bytes = at;
        if (p.meta_bytes > p.longest) p.longest = p.meta_bytes;
    }
    if (p.units > MAX_STREAMS)
        return plan_fail(L3C_ERR_UNSUPPORTED, err, cap, "unsupported: more than 65535 parity groups in one file");
    p.meta_stride = head ? round16(p.meta_bytes) + 16 : 0;
    p.ws_tail_at = 0;
    p.ws_unit_off = round16(8 * B);
    p.ws_meta = p.ws_unit_off + round16(8 * B * p.units);
    p.ws_bytes = p.ws_meta + B * p.meta_stride;
    *out = p;
    return L3C_OK;
}

// The most bytes l3c_seal_append_parity writes behind one file of this plan when no payload of record k exceeds max_payload[k] (indexed as
// the plan's records):
//     front_bytes + 3 m R max_payload[finest] + 8 + table_bytes + 24
//     and with a head part  + meta_bytes + sum over the head records of C_k m_k R max_payload[k] + 4
inline int64_t tail_bound(const Plan &p, const int64_t *max_payload) {
    const int fin = p.n_records - 1;
    int64_t total = p.front_bytes + 3 * (int64_t)p.rec[fin].m * p.R * max_payload[fin] + 8 + p.table_bytes + L3C_SEAL_BYTES;
    if (p.head) {
        total += p.meta_bytes + 4;
        for (int k = 0; k < fin; ++k) total += (int64_t)p.rec[k].C * p.rec[k].m * p.R * max_payload[k];
    }
    return total;
}

}  // namespace l3c_parity_seal

#endif
