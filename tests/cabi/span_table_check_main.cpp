// csrc/crc_spans.h alone, as a program of its own (built with the address and undefined-behaviour sanitizers by tests/test_crc_spans_host.py):
//   1. the validator of l3c_u8_crc32_spans over accepted tables and over every kind of table it must refuse, int64 edges among them; the
//      table lives in a heap block of exactly its size, so that a read past its end is a sanitizer report;
//   2. the prefix of tile counts and the unit -> span lookup the tile launch bisects, for random tables with empty spans in every place;
//   3. the combine arithmetic, replayed on the host for a list of lengths: the remainder of every zero-filled tile from a bitwise register,
//      the 64 lane shares XORed as the wavefront XORs them, then k_last, unfill and z -- each derived from the span's length by the
//      functions the device calls -- against a bitwise CRC-32 of the same bytes written here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../l3c-pytorch_amd/csrc/crc_spans.h"

using namespace l3c_crc;

static int fail(const char *what, long long a, long long b) {
    printf("span_table_check: FAILED %s (%lld, %lld)\n", what, a, b);
    return 1;
}

// the register after `n` more bytes, bit by bit (reflected, as zlib keeps it)
static uint32_t bitwise(uint32_t reg, const uint8_t *p, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        reg ^= p[i];
        for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (POLY & (0u - (reg & 1u)));
    }
    return reg;
}
static uint32_t crc32_bitwise(const uint8_t *p, int64_t n) { return ~bitwise(0xFFFFFFFFu, p, n); }

static int64_t check(const std::vector<l3c_u8_span> &t, int64_t data_bytes, char *err) {
    l3c_u8_span *exact = static_cast<l3c_u8_span *>(malloc(t.size() ? t.size() * sizeof(l3c_u8_span) : 1));
    if (!t.empty()) memcpy(exact, t.data(), t.size() * sizeof(l3c_u8_span));
    err[0] = 0;
    const int64_t rc = check_spans(exact, (int64_t)t.size(), data_bytes, err, 128);
    free(exact);
    return rc;
}

static uint32_t next(uint32_t *s) {
    *s = *s * 1664525u + 1013904223u;
    return *s >> 8;
}

// zlib's word of `n` bytes at p the way l3c_u8_crc32_spans gets it
static uint32_t replay(const uint8_t *p, int64_t n) {
    const int64_t tiles = tiles_of(n);
    if (tiles == 0) return span_z(n);
    std::vector<uint32_t> partial((size_t)tiles);
    std::vector<uint8_t> zeros(ROW_BYTES, 0);
    for (int64_t b = 0; b < tiles; ++b) {
        const int64_t at = b * TILE_BYTES, len = n - at < TILE_BYTES ? n - at : TILE_BYTES;
        uint32_t r = bitwise(0u, p + at, len);
        r = bitwise(r, zeros.data(), (len + ROW_BYTES - 1) / ROW_BYTES * ROW_BYTES - len);      // filled up to whole rows
        partial[(size_t)b] = r;
    }
    uint32_t a = 0;
    for (int lane = 0; lane < 64; ++lane) a ^= lane_share(partial.data(), tiles - 1, lane);
    return finish(a, partial[(size_t)(tiles - 1)], span_k_last(n), span_unfill(n), span_z(n));
}

int main() {
    char err[128];
    const int64_t I64_MAX = INT64_MAX, T = TILE_BYTES;

    // ---- 1. the validator -----------------------------------------------------------------------------------------------------------
    long long refused = 0;
    {
        // any order, overlapping, with gaps, empty, ending with the buffer: 8 spans, 7 of one tile each
        const std::vector<l3c_u8_span> ok = {{64, 100}, {0, 64}, {32, 64}, {4096, 0}, {1000, 3096}, {0, 4096}, {4096 - 4, 4}, {8, 1}};
        if (check(ok, 4096, err) != 7) return fail("the accepted table", check(ok, 4096, err), 0);
        if (check({{0, T}, {T, T + 1}, {0, 3 * T}}, 3 * T, err) != 1 + 2 + 3) return fail("tile counts", 0, 0);
        if (check({{0, 0}}, 0, err) != 0) return fail("one empty span of an empty buffer", 0, 0);
        if (check({{I64_MAX - 2, 0}}, I64_MAX, err) != L3C_ERR_INVALID_ARG || !strstr(err, "multiple of 4")) return fail("an odd offset at the int64 edge", 0, 0);
        if (check({{I64_MAX - 7, 7}}, I64_MAX, err) != 1) return fail("a span that ends with an int64-max buffer", 0, 0);
        const SpanWorkspace w = span_workspace(8, 7);
        if (w.consts_at % 16 || w.partial_at % 16 || w.bytes % 16 || w.consts_at < 8 * 9 || w.partial_at - w.consts_at < 16 * 8 || w.bytes - w.partial_at < 4 * 7)
            return fail("the workspace layout", w.partial_at, w.bytes);
    }
    struct Bad {
        std::vector<l3c_u8_span> t;
        int64_t data_bytes;
        const char *span, *what;
    };
    const Bad bad[] = {
        {{}, 100, "span -1", "n_spans"},
        {{{0, 4}}, -1, "span -1", "data_bytes"},
        {{{0, 4}, {-4, 4}}, 100, "span 1", "offset must not be negative"},
        {{{0, 4}, {0, 4}, {0, -1}}, 100, "span 2", "bytes must not be negative"},
        {{{0, 4}, {INT64_MIN, 4}}, 100, "span 1", "offset must not be negative"},
        {{{0, INT64_MIN}}, 100, "span 0", "bytes must not be negative"},
        {{{2, 4}}, 100, "span 0", "multiple of 4"},
        {{{0, 4}, {5, 4}}, 100, "span 1", "multiple of 4"},
        {{{96, 5}}, 100, "span 0", "exceeds data_bytes"},
        {{{0, 100}, {100, 1}}, 100, "span 1", "exceeds data_bytes"},
        {{{104, 0}}, 100, "span 0", "exceeds data_bytes"},
        {{{I64_MAX - 3, 4}}, I64_MAX, "span 0", "overflows"},
        {{{8, I64_MAX}}, I64_MAX, "span 0", "overflows"},
        {{{0, I64_MAX}}, I64_MAX, "span 0", "2^40 tiles"},                                      // 2^46 tiles in one span
        {{{0, T * (MAX_TILES - 1)}, {0, 1}}, I64_MAX, "span 1", "2^40 tiles"},                    // the sum reaches 2^40 with the second
    };
    for (const Bad &b : bad) {
        if (check(b.t, b.data_bytes, err) != L3C_ERR_INVALID_ARG || !strstr(err, b.span) || !strstr(err, b.what)) {
            printf("span_table_check: '%s' where '%s ... %s' was expected\n", err, b.span, b.what);
            return fail("a table that must be refused", refused, 0);
        }
        ++refused;
    }
    if (check({{0, T * (MAX_TILES - 1)}}, I64_MAX, err) != MAX_TILES - 1) return fail("2^40 - 1 tiles", 0, 0);
    if (check_spans(nullptr, 1, 100, err, 128) != L3C_ERR_INVALID_ARG || !strstr(err, "null table")) return fail("a null table", 0, 0);
    if (count_tiles(nullptr, 1, err, 128) != L3C_ERR_INVALID_ARG || check_spans(nullptr, 1, 100, nullptr, 0) != L3C_ERR_INVALID_ARG) return fail("null arguments", 0, 0);

    // ---- 2. prefix and lookup -------------------------------------------------------------------------------------------------------
    long long tables = 0, units_seen = 0;
    uint32_t seed = 12345u;
    for (int round = 0; round < 300; ++round) {
        const int n = 1 + (int)(next(&seed) % 40);
        std::vector<l3c_u8_span> t((size_t)n);
        int64_t at = 0;
        for (auto &s : t) {
            const uint32_t kind = next(&seed) % 4;               // empty, below a tile, exactly tiles, tiles and a rest
            s.bytes = kind == 0 ? 0 : kind == 1 ? 1 + next(&seed) % (T - 1) : kind == 2 ? T * (1 + next(&seed) % 3) : T * (next(&seed) % 3) + 1 + next(&seed) % T;
            s.offset = at;
            at += (s.bytes + 3) / 4 * 4 + 4 * (next(&seed) % 3);
        }
        const int64_t units = check(t, at, err);
        if (units < 0) return fail("a random table was refused", round, 0);
        std::vector<int64_t> first((size_t)n + 1);
        first[0] = 0;
        for (int k = 0; k < n; ++k) first[(size_t)k + 1] = first[(size_t)k] + tiles_of(t[(size_t)k].bytes);
        if (first[(size_t)n] != units) return fail("the prefix's last entry is not the validator's total", first[(size_t)n], units);
        for (int64_t u = 0; u < units; ++u) {
            const int64_t k = span_of_unit(first.data(), n, u);
            if (k < 0 || k >= n || first[(size_t)k] > u || u >= first[(size_t)k + 1]) return fail("span_of_unit", u, k);
            if ((u - first[(size_t)k]) * T >= t[(size_t)k].bytes) return fail("a tile that starts behind its span", u, k);
            ++units_seen;
        }
        ++tables;
    }

    // ---- 3. the combine arithmetic --------------------------------------------------------------------------------------------------
    const int64_t S = TILE_BYTES, TH = THREAD_BYTES, R = ROW_BYTES;
    const int64_t lengths[] = {0, 1, 3, 4, 5, 15, 16, 17, TH - 1, TH, TH + 1, R - 1, R, R + 1, S - R, S - 1, S, S + 1, 2 * S + 7, 192, 18432, 3 * 24 * 40,
                               64 * S, 64 * S + 1, 66 * S + 5, 130 * S + 4097};
    long long checked = 0;
    for (int fill = 0; fill < 3; ++fill)                                                      // random bytes, all zero, all 0xFF
        for (int64_t n : lengths) {
            if (fill && n > 3 * S) continue;
            uint8_t *p = static_cast<uint8_t *>(malloc(n ? (size_t)n : 1));                   // exactly n bytes: a read behind them is a report
            for (int64_t i = 0; i < n; ++i) p[i] = fill == 0 ? (uint8_t)next(&seed) : fill == 1 ? 0 : 0xFF;
            const uint32_t want = crc32_bitwise(p, n), got = replay(p, n);
            free(p);
            if (got != want) return fail("the replayed combine differs from the bitwise CRC-32", n, fill);
            ++checked;
        }
    const uint8_t check_msg[] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
    if (crc32_bitwise(check_msg, 9) != 0xCBF43926u || replay(check_msg, 9) != 0xCBF43926u) return fail("the CRC-32 check value", 0, 0);
    if (span_z(0) != 0) return fail("Z(0)", span_z(0), 0);

    printf("span_table_check: %lld tables refused, %lld random tables with %lld tiles looked up\n", refused, tables, units_seen);
    printf("span_table_check: %lld runs replayed, equal to the bitwise CRC-32\n", checked);
    return 0;
}
