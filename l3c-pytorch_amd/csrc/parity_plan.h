// parity_plan.h -- what csrc/parity.hip decides on the host: the tables of l3c_u8_xor_spans (include/l3c_hip.h) against the buffers they
// index, and the launch width they ask for.
//
// Plain C++17 on purpose, as crc_spans.h: no HIP include, no library call, no allocation, so that the code that decides which bytes a kernel
// may read and write compiles into a stand-alone program as well as into libl3c_hip.so.  The kernels trust tables that passed.
#ifndef L3C_PARITY_PLAN_H_
#define L3C_PARITY_PLAN_H_

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

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

}  // namespace l3c_parity

#endif
