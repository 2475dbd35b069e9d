// crc_spans.h -- what csrc/crc.hip decides on the host and what its kernels share with the host: the GF(2) arithmetic of zlib's CRC-32, the
// tile geometry, the constants that depend on a run's length, and the span table of l3c_u8_crc32_spans (include/l3c_hip.h: l3c_u8_span)
// with its validator and its workspace layout.
//
// Plain C++17 on purpose, as image_table.h: no HIP include, no library call, no allocation, so that the code that decides which bytes a
// kernel may read -- and the arithmetic that turns the remainders of zero-filled tiles into zlib's word -- compiles into a stand-alone
// program (tests/cabi/span_table_check_main.cpp, built with the address and undefined-behaviour sanitizers) as well as into
// libl3c_hip.so.  Under hipcc the arithmetic is __host__ __device__: the device derives a span's constants with the very functions the
// host program replays.
#ifndef L3C_CRC_SPANS_H_
#define L3C_CRC_SPANS_H_

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/l3c_hip.h"

#ifdef __HIPCC__
#define L3C_CRC_HD __host__ __device__
#else
#define L3C_CRC_HD
#endif

namespace l3c_crc {

constexpr uint32_t POLY = 0xEDB88320u;
constexpr uint32_t ONE = 0x80000000u, X1 = 0x40000000u, X_INV = 0xDB710641u;
constexpr int THREADS = 256, ROW_BYTES = THREADS * 16, ROWS = 32, TILE_BYTES = ROWS * ROW_BYTES, THREAD_BYTES = ROWS * 16;

// a b mod P (zlib's multmodp)
L3C_CRC_HD constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
    }
    return p;
}

// base^e mod P
L3C_CRC_HD constexpr uint32_t powmod(uint32_t base, uint64_t e) {
    uint32_t r = ONE;
    while (e) {
        if (e & 1) r = mulmod(r, base);
        base = mulmod(base, base);
        e >>= 1;
    }
    return r;
}

constexpr uint32_t X8 = powmod(X1, 8), X8_INV = powmod(X_INV, 8);
constexpr uint32_t K_ROW = powmod(X8, ROW_BYTES), K_TILE = powmod(X8, TILE_BYTES);
// l3c_u8_crc32_bands: a wavefront's row (64 lanes x 16 bytes) and the chunk of a band one wavefront folds
constexpr int WROW = 64 * 16, WROWS = 16, WCHUNK = WROWS * WROW;
constexpr uint32_t K_WROW = powmod(X8, WROW), K_WCHUNK = powmod(X8, WCHUNK);
static_assert(mulmod(X1, X_INV) == ONE && mulmod(X8, X8_INV) == ONE, "x^-1 mod P");
static_assert(powmod(X1, 32) == POLY, "x^32 mod P is the polynomial's low part");

L3C_CRC_HD constexpr int64_t tiles_of(int64_t item_bytes) { return item_bytes / TILE_BYTES + (item_bytes % TILE_BYTES != 0); }

// The three constants of a run of `bytes` > 0 bytes whose last tile was filled up with zero bytes to whole rows:
// k_last = x^(8 * bytes of the last tile's rows), unfill = x^(-8 * zero bytes it was filled up with), z = Z(bytes).  0 bytes: z alone, 0.
struct SpanConsts {
    uint32_t k_last, unfill, z, reserved;      // 16 bytes: one load per span
};
L3C_CRC_HD constexpr uint32_t span_k_last(int64_t bytes) {
    return powmod(X8, (uint64_t)((bytes - (tiles_of(bytes) - 1) * TILE_BYTES + ROW_BYTES - 1) / ROW_BYTES * ROW_BYTES));
}
L3C_CRC_HD constexpr uint32_t span_unfill(int64_t bytes) { return powmod(X8_INV, (uint64_t)((bytes + ROW_BYTES - 1) / ROW_BYTES * ROW_BYTES - bytes)); }
L3C_CRC_HD constexpr uint32_t span_z(int64_t bytes) { return mulmod(powmod(X8, (uint64_t)bytes), 0xFFFFFFFFu) ^ 0xFFFFFFFFu; }

// zlib's word from the remainders of a run's tiles (`full` whole tiles in front of the last one, each remainder taken from a zero
// register, the last tile zero-filled to whole rows): Horner with x^(8 TILE), then the last tile, the fill undone, Z added
L3C_CRC_HD constexpr uint32_t finish(uint32_t horner_of_full_tiles, uint32_t last_tile, uint32_t k_last, uint32_t unfill, uint32_t z) {
    return mulmod(mulmod(horner_of_full_tiles, k_last) ^ last_tile, unfill) ^ z;
}

// A wavefront combines the `full` whole tiles of a run: lane `lane` of 64 runs Horner over its contiguous share of their remainders and
// weighs it with the tiles behind the share; the XOR over the lanes is Horner over all of them.
L3C_CRC_HD inline uint32_t lane_share(const uint32_t *partial, int64_t full, int lane) {
    const int64_t share = (full + 63) / 64;
    const int64_t lo = lane * share < full ? lane * share : full, hi = lo + share < full ? lo + share : full;
    uint32_t a = 0;
    for (int64_t b = lo; b < hi; ++b) a = mulmod(a, K_TILE) ^ partial[b];
    if (hi > lo && hi < full) a = mulmod(a, powmod(K_TILE, (uint64_t)(full - hi)));
    return a;
}

// The span of tile `unit` of a call: the k with first[k] <= unit < first[k + 1], where first[k] is the number of tiles in front of span k
// and first[n] the number of all tiles (> unit).  A span of no tiles is never the answer.
L3C_CRC_HD inline int64_t span_of_unit(const int64_t *first, int64_t n, int64_t unit) {
    int64_t lo = 0, hi = n;                          // first[lo] <= unit < first[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

constexpr int64_t MAX_TILES = (int64_t)1 << 40;      // total tiles of one call (exclusive)

inline int64_t span_fail(char *err, size_t cap, long long span, const char *what) {
    if (err && cap) snprintf(err, cap, "span %lld: %s", span, what);
    return L3C_ERR_INVALID_ARG;
}

// The sizes of a table alone (what the workspace depends on) -> tiles of all spans, or L3C_ERR_INVALID_ARG with a message naming the span.
inline int64_t count_tiles(const l3c_u8_span *t, int64_t n, char *err, size_t cap) {
    if (!t) return span_fail(err, cap, -1, "null table (spans_host)");
    if (n < 1) return span_fail(err, cap, -1, "n_spans must be at least 1");
    int64_t total = 0;
    for (int64_t k = 0; k < n; ++k) {
        if (t[k].bytes < 0) return span_fail(err, cap, k, "bytes must not be negative");
        total += tiles_of(t[k].bytes);                   // < 2^47 each, checked against 2^40 before the next is added
        if (total >= MAX_TILES) return span_fail(err, cap, k, "the spans up to this one have 2^40 tiles or more");
    }
    return total;
}

// Every span of the table against the buffer of data_bytes bytes -> tiles of all spans (>= 0), or L3C_ERR_INVALID_ARG with a message
// naming the first offending span and field.  The kernels trust a table that passed.
inline int64_t check_spans(const l3c_u8_span *t, int64_t n, int64_t data_bytes, char *err, size_t cap) {
    if (!t) return span_fail(err, cap, -1, "null table (spans_host)");
    if (n < 1) return span_fail(err, cap, -1, "n_spans must be at least 1");
    if (data_bytes < 0) return span_fail(err, cap, -1, "data_bytes must not be negative");
    for (int64_t k = 0; k < n; ++k) {
        int64_t end;
        if (t[k].offset < 0) return span_fail(err, cap, k, "offset must not be negative");
        if (t[k].bytes < 0) return span_fail(err, cap, k, "bytes must not be negative");
        if (t[k].offset % 4 != 0) return span_fail(err, cap, k, "offset must be a multiple of 4");
        if (__builtin_add_overflow(t[k].offset, t[k].bytes, &end)) return span_fail(err, cap, k, "offset + bytes overflows 64 bits");
        if (end > data_bytes) return span_fail(err, cap, k, "offset + bytes exceeds data_bytes");
    }
    return count_tiles(t, n, err, cap);
}

// The workspace of l3c_u8_crc32_spans: first[n + 1] int64 (tiles in front of every span, then all) | consts[n] | partial[tiles] uint32,
// each part 16-byte aligned.
struct SpanWorkspace {
    int64_t first_at, consts_at, partial_at, bytes;
};
inline SpanWorkspace span_workspace(int64_t n, int64_t tiles) {
    SpanWorkspace w{};
    w.first_at = 0;
    w.consts_at = (8 * (n + 1) + 15) / 16 * 16;
    w.partial_at = w.consts_at + (int64_t)sizeof(SpanConsts) * n;
    w.bytes = w.partial_at + (4 * tiles + 15) / 16 * 16 + 16;
    return w;
}

}  // namespace l3c_crc

#endif
