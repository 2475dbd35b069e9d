// parity_plan.h -- what csrc/parity.hip decides on the host: the tables of l3c_u8_xor_spans and of l3c_band_rebuild (include/l3c_hip.h)
// against the buffers they index, and the launch width they ask for.
//
// Plain C++17 on purpose, as crc_spans.h: no HIP include, no library call, no allocation, so that the code that decides which bytes a kernel
// may read and write compiles into a stand-alone program as well as into libl3c_hip.so.  The kernels trust tables that passed.
#ifndef L3C_PARITY_PLAN_H_
#define L3C_PARITY_PLAN_H_

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/l3c_hip.h"

namespace l3c_parity {

constexpr int THREADS = 256, TILE_BYTES = THREADS * 16;      // a block folds 4096 bytes of one output stream, 16 per thread
constexpr int64_t MAX_STREAMS = 65535;                       // grid.y
constexpr int HEAD_MAX_RECORDS = 8;                          // records of one l3c_head_parity / l3c_band_payload_crc32 call (they travel by value)

constexpr int64_t round4(int64_t n) { return (n + 3) / 4 * 4; }
constexpr int64_t slot_bytes(int64_t bytes) { return round4(bytes) + 4; }      // what l3c_u8_xor_spans writes of a slot of `bytes` bytes
constexpr int64_t tiles_of(int64_t bytes) { return (bytes + TILE_BYTES - 1) / TILE_BYTES; }

inline int64_t plan_fail(char *err, size_t cap, const char *table, long long at, const char *what) {
    if (err && cap) snprintf(err, cap, "%s %lld: %s", table, at, what);
    return L3C_ERR_INVALID_ARG;
}

// The tables of one l3c_u8_xor_spans call -> the tiles of the longest slot (>= 1: grid.x), or L3C_ERR_INVALID_ARG with a message naming the
// table, the entry and the field.  n_groups >= 1.
inline int64_t check_xor_spans(const l3c_u8_span *spans, int64_t n_spans, const int64_t *group_first, int64_t n_groups, const l3c_u8_span *out_spans,
                               int64_t data_bytes, int64_t out_bytes, char *err, size_t cap) {
    if (!group_first || !out_spans || (n_spans > 0 && !spans)) return plan_fail(err, cap, "table", -1, "null pointer (a host table)");
    if (n_groups < 1 || n_groups > MAX_STREAMS) return plan_fail(err, cap, "group", -1, "n_groups must be in 0..65535");
    if (n_spans < 0) return plan_fail(err, cap, "span", -1, "n_spans must not be negative");
    if (data_bytes < 0 || out_bytes < 0) return plan_fail(err, cap, "table", -1, "data_bytes and out_bytes must not be negative");
    for (int64_t k = 0; k < n_spans; ++k) {
        int64_t end;
        if (spans[k].offset < 0) return plan_fail(err, cap, "span", k, "offset must not be negative");
        if (spans[k].bytes < 0) return plan_fail(err, cap, "span", k, "bytes must not be negative");
        if (spans[k].offset % 4 != 0) return plan_fail(err, cap, "span", k, "offset must be a multiple of 4");
        if (__builtin_add_overflow(spans[k].offset, spans[k].bytes, &end) || end > INT64_MAX - 3)
            return plan_fail(err, cap, "span", k, "offset + bytes overflows 64 bits");
        if (round4(end) > data_bytes) return plan_fail(err, cap, "span", k, "its 4-byte-rounded end exceeds data_bytes");
    }
    if (group_first[0] != 0) return plan_fail(err, cap, "group", 0, "group_first must start at 0");
    int64_t longest = 0;
    for (int64_t g = 0; g < n_groups; ++g) {
        int64_t end;
        if (group_first[g + 1] < group_first[g]) return plan_fail(err, cap, "group", g, "group_first must not descend");
        if (group_first[g + 1] > n_spans) return plan_fail(err, cap, "group", g, "group_first exceeds n_spans");
        if (out_spans[g].offset < 0) return plan_fail(err, cap, "out span", g, "offset must not be negative");
        if (out_spans[g].bytes < 0) return plan_fail(err, cap, "out span", g, "bytes must not be negative");
        if (out_spans[g].offset % 4 != 0) return plan_fail(err, cap, "out span", g, "offset must be a multiple of 4");
        if (out_spans[g].bytes > INT64_MAX - 8 || __builtin_add_overflow(out_spans[g].offset, slot_bytes(out_spans[g].bytes), &end))
            return plan_fail(err, cap, "out span", g, "offset + bytes overflows 64 bits");
        if (end > out_bytes) return plan_fail(err, cap, "out span", g, "the slot (bytes rounded up to 4, and 4 zero bytes) exceeds out_bytes");
        if (slot_bytes(out_spans[g].bytes) > longest) longest = slot_bytes(out_spans[g].bytes);
    }
    if (group_first[n_groups] != n_spans) return plan_fail(err, cap, "group", n_groups, "group_first must end at n_spans");
    if (tiles_of(longest) > 0x7fffffff) return plan_fail(err, cap, "out span", -1, "a slot of 2^43 bytes or more");
    return tiles_of(longest);
}

// ---- l3c_band_rebuild ---------------------------------------------------------------------------------------------------------------------

constexpr int REBUILD_MAX = 4;                                // rows and outputs of a group

struct RebuildInterval {                                     // bytes [lo, hi) of `members` that group `group` reads (out 0) or writes (out 1)
    int64_t lo, hi;
    int32_t group, out;
};

// how many RebuildInterval check_rebuild needs room for, or L3C_ERR_INVALID_ARG (counts that cannot be summed: check_rebuild says why)
inline int64_t rebuild_intervals(const l3c_rebuild_group *groups, int64_t n_groups) {
    if (!groups || n_groups < 1 || n_groups > MAX_STREAMS) return L3C_ERR_INVALID_ARG;
    int64_t n = 0;
    for (int64_t g = 0; g < n_groups; ++g) {
        if (groups[g].n_members < 0 || groups[g].t < 1 || groups[g].t > REBUILD_MAX) return L3C_ERR_INVALID_ARG;
        n += (int64_t)groups[g].n_members + groups[g].t;
    }
    return n;
}

// The tables of one l3c_band_rebuild call against the two buffers -> the tiles of the longest slot (>= 1: grid.x), or L3C_ERR_INVALID_ARG with
// a message naming the table, the entry and the field.  n_groups >= 1; scratch: room for rebuild_intervals(groups, n_groups) entries (null
// where that failed).  A slot may not overlap a member source of any group, nor another slot: the intervals are sorted by their first byte
// and swept once, with the furthest end of the slots and of everything seen so far.
inline int64_t check_rebuild(const l3c_u8_span *src, int64_t n_src, const l3c_rebuild_group *groups, int64_t n_groups, int64_t rows_bytes,
                             int64_t members_bytes, RebuildInterval *scratch, char *err, size_t cap) {
    if (!groups || (n_src > 0 && !src)) return plan_fail(err, cap, "table", -1, "null pointer (a host table)");
    if (n_groups < 1 || n_groups > MAX_STREAMS) return plan_fail(err, cap, "group", -1, "n_groups must be in 0..65535");
    if (n_src < 0) return plan_fail(err, cap, "source", -1, "n_src must not be negative");
    if (rows_bytes < 0 || members_bytes < 0) return plan_fail(err, cap, "table", -1, "rows_bytes and members_bytes must not be negative");
    for (int64_t g = 0; g < n_groups; ++g) {                     // the counts first: what the size of `scratch` was taken from
        const l3c_rebuild_group &q = groups[g];
        if (q.reserved != 0) return plan_fail(err, cap, "group", g, "reserved must be 0");
        if (q.t < 1 || q.t > REBUILD_MAX) return plan_fail(err, cap, "group", g, "t must be in 1..4");
        if (q.n_rows < 1 || q.n_rows > REBUILD_MAX) return plan_fail(err, cap, "group", g, "n_rows must be in 1..4");
        if (q.n_members < 0) return plan_fail(err, cap, "group", g, "n_members must not be negative");
    }
    if (!scratch) return plan_fail(err, cap, "table", -1, "null pointer (the scratch of the overlap check)");
    int64_t longest = 0, n_iv = 0;
    for (int64_t g = 0; g < n_groups; ++g) {
        const l3c_rebuild_group &q = groups[g];
        const int64_t count = (int64_t)q.n_rows + q.n_members;
        if (q.first_src < 0 || q.first_src > n_src || count > n_src - q.first_src)
            return plan_fail(err, cap, "group", g, "its sources [first_src, first_src + n_rows + n_members) exceed n_src");
        for (int64_t k = q.first_src; k < q.first_src + count; ++k) {
            const bool row = k < q.first_src + q.n_rows;
            int64_t end;
            if (src[k].offset < 0) return plan_fail(err, cap, "source", k, "offset must not be negative");
            if (src[k].bytes < 0) return plan_fail(err, cap, "source", k, "bytes must not be negative");
            if (__builtin_add_overflow(src[k].offset, src[k].bytes, &end) || end > INT64_MAX - 3)
                return plan_fail(err, cap, "source", k, "offset + bytes overflows 64 bits");
            if (row) {
                if (end > rows_bytes) return plan_fail(err, cap, "source", k, "a row: its end exceeds rows_bytes");
                continue;
            }
            if (src[k].offset % 4 != 0) return plan_fail(err, cap, "source", k, "a member: offset must be a multiple of 4");
            if (round4(end) > members_bytes) return plan_fail(err, cap, "source", k, "a member: its 4-byte-rounded end exceeds members_bytes");
            if (src[k].bytes > 0) scratch[n_iv++] = RebuildInterval{src[k].offset, round4(end), (int32_t)g, 0};
        }
        for (int e = 0; e < q.t; ++e) {
            const l3c_u8_span &o = q.out[e];
            int64_t end;
            if (o.offset < 0) return plan_fail(err, cap, "group", g, "an output slot: offset must not be negative");
            if (o.bytes < 0) return plan_fail(err, cap, "group", g, "an output slot: bytes must not be negative");
            if (o.offset % 4 != 0) return plan_fail(err, cap, "group", g, "an output slot: offset must be a multiple of 4");
            if (o.bytes > INT64_MAX - 8 || __builtin_add_overflow(o.offset, slot_bytes(o.bytes), &end))
                return plan_fail(err, cap, "group", g, "an output slot: offset + bytes overflows 64 bits");
            if (end > members_bytes)
                return plan_fail(err, cap, "group", g, "an output slot (bytes rounded up to 4, and 4 zero bytes) exceeds members_bytes");
            if (slot_bytes(o.bytes) > longest) longest = slot_bytes(o.bytes);
            scratch[n_iv++] = RebuildInterval{o.offset, end, (int32_t)g, 1};
        }
    }
    if (tiles_of(longest) > 0x7fffffff) return plan_fail(err, cap, "group", -1, "a slot of 2^43 bytes or more");
    std::sort(scratch, scratch + n_iv, [](const RebuildInterval &a, const RebuildInterval &b) { return a.lo < b.lo; });
    int64_t any_hi = INT64_MIN, out_hi = INT64_MIN;              // the furthest end so far: of every interval, of the slots
    for (int64_t i = 0; i < n_iv; ++i) {
        const RebuildInterval &v = scratch[i];
        if (v.out && v.lo < any_hi) return plan_fail(err, cap, "group", v.group, "an output slot overlaps a member source or another slot of the call");
        if (!v.out && v.lo < out_hi) return plan_fail(err, cap, "group", v.group, "a member source overlaps an output slot of the call");
        if (v.hi > any_hi) any_hi = v.hi;
        if (v.out && v.hi > out_hi) out_hi = v.hi;
    }
    return tiles_of(longest);
}

}  // namespace l3c_parity

#endif
