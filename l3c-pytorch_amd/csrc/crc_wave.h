// crc_wave.h -- the device code a WAVEFRONT needs to hash a byte run of any length with zlib's CRC-32, shared by csrc/crc.hip (the tile and
// band kernels use its tables; l3c_band_payload_crc32 is wave_crc32 per payload) and csrc/seal_parity.hip (head_crc and head_check of an
// 'L3CH' section).  The arithmetic is csrc/crc_spans.h's; csrc/crc.hip explains it.
//
// The nibble tables lie in LDS 32 times, entry e of lane l at dword 32 e + (l & 31): every lane of a 32-lane half reads a bank of its own.
#ifndef L3C_CRC_WAVE_H_
#define L3C_CRC_WAVE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc_spans.h"

namespace l3c_crc_wave {

using l3c_crc::K_ROW, l3c_crc::K_WROW, l3c_crc::mulmod, l3c_crc::ONE, l3c_crc::POLY, l3c_crc::powmod, l3c_crc::THREADS, l3c_crc::WROW, l3c_crc::X8,
    l3c_crc::X8_INV;

// [0]: MULK, [1]: MUL32, [2]: MULW (a wavefront's row, l3c_u8_crc32_bands) -- entry 16 k + n is (n << 4 k) times the constant
struct NibbleTables {
    uint32_t v[3][128];
};
constexpr NibbleTables make_tables() {
    NibbleTables t{};
    for (int k = 0; k < 8; ++k)
        for (uint32_t n = 0; n < 16; ++n) {
            t.v[0][16 * k + n] = mulmod(n << (4 * k), K_ROW);
            t.v[1][16 * k + n] = mulmod(n << (4 * k), POLY);
            t.v[2][16 * k + n] = mulmod(n << (4 * k), K_WROW);
        }
    return t;
}
// SHIFT[t] = x^(8 * 16 (255 - t)): the bytes of a row behind thread t's 16
struct ShiftTable {
    uint32_t v[THREADS];
};
constexpr ShiftTable make_shifts() {
    ShiftTable s{};
    const uint32_t step = powmod(X8, 16);
    uint32_t c = ONE;
    for (int t = THREADS - 1; t >= 0; --t) {
        s.v[t] = c;
        c = mulmod(c, step);
    }
    return s;
}
__device__ const NibbleTables g_tables = make_tables();
__device__ const ShiftTable g_shifts = make_shifts();

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// v times the table's constant; tab: the lane's column of one table in LDS
__device__ __forceinline__ uint32_t times(const uint32_t *tab, uint32_t v) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) r ^= tab[(16 * k + ((v >> (4 * k)) & 15u)) * 32];
    return r;
}

// one row: a_j = a_j K + d_j for the four remainders.  All 32 lookups are issued before the first is used: the four chains are independent,
// and one LDS round trip per row instead of four is what the loop's time is made of
__device__ __forceinline__ void row_step(const uint32_t *tab, uint32_t (&a)[4], u32x4 d) {
    uint32_t r[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) r[j][k] = tab[(16 * k + ((a[j] >> (4 * k)) & 15u)) * 32];
    const uint32_t in[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = ((r[j][0] ^ r[j][1] ^ r[j][2]) ^ (r[j][3] ^ r[j][4] ^ r[j][5])) ^ (r[j][6] ^ r[j][7] ^ in[j]);
}

// ---- a wavefront on one byte run whose length is known on the device alone ------------------------------------------------------------
//
// Rows of WROW bytes and the MULW step; the run is only 4-byte aligned and may hold garbage behind its length: dword loads in front of the
// 4-byte-rounded end (one 16-byte load where the address allows it), the bytes of the last dword behind the length masked.  The length's
// two constants, x^(8 len) for Z and x^(-8 fill) for the zero fill of the last row, are products over the set bits of len and fill: lanes
// 0..31 and 32..63 each hold one factor (X8_POW2) and a five-step butterfly multiplies them.
struct Pow2Table {
    uint32_t v[64];      // [i]: x^(8 2^i), [32 + i]: x^(-8 2^i)
};
constexpr Pow2Table make_pow2() {
    Pow2Table t{};
    uint32_t a = X8, b = X8_INV;
    for (int i = 0; i < 32; ++i) {
        t.v[i] = a, t.v[32 + i] = b;
        a = mulmod(a, a), b = mulmod(b, b);
    }
    return t;
}
__device__ const Pow2Table g_pow2 = make_pow2();

// bytes [off, off + 16) of the payload at p (4-byte aligned) of len bytes, zero from byte len on; nothing at or behind its 4-byte-rounded end is read
__device__ __forceinline__ u32x4 load16_masked(const uint8_t *p, int64_t len, int64_t off) {
    const int64_t end4 = (len + 3) & ~(int64_t)3;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (off + 16 <= end4 && (reinterpret_cast<uintptr_t>(p + off) & 15) == 0) {
        const u32x4 q = *reinterpret_cast<const u32x4 *>(p + off);
        w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (off + 4 * i < end4) w[i] = *reinterpret_cast<const uint32_t *>(p + off + 4 * i);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t keep = len - (off + 4 * i);
        if (keep < 4) w[i] = keep <= 0 ? 0u : w[i] & (0xFFFFFFFFu >> (8 * (4 - (int)keep)));
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}

constexpr int WAVE_TABLE_WORDS = 2 * 128 * 32;      // MULW, then MUL32, each 32 times: the LDS of a block whose waves call wave_crc32

// MULW and MUL32 into `lds` (WAVE_TABLE_WORDS words) by the block's THREADS threads; a barrier must follow
__device__ __forceinline__ void stage_wave_tables(uint32_t *lds, int t) {
    for (int i = 0; i < 32; ++i) {
        const int idx = i * THREADS + t;
        lds[idx] = idx < 128 * 32 ? g_tables.v[2][idx >> 5] : g_tables.v[1][(idx >> 5) - 128];
    }
}

// zlib's CRC-32 of the len bytes at p (4-byte aligned; len 0 gives 0), computed by one whole wavefront: every lane returns the word.
// lds: the tables of stage_wave_tables; lane: the thread's lane.  The word does not depend on the launch geometry.
__device__ __forceinline__ uint32_t wave_crc32(const uint32_t *lds, int lane, const uint8_t *p, int64_t len) {
    const uint32_t *mulw = lds + (lane & 31), *mul32 = lds + 128 * 32 + (lane & 31);
    const uint32_t shift = g_shifts.v[THREADS - 64 + lane];
    const int64_t rows = (len + WROW - 1) / WROW;
    uint32_t a[4] = {0u, 0u, 0u, 0u};
    for (int64_t r = 0; r < rows; r += 4) {
        u32x4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = load16_masked(p, len, (r + u) * WROW + 16 * lane);      // (behind the last row: len masks all)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r + u < rows) row_step(mulw, a, q[u]);
    }
    uint32_t v = times(mul32, a[0]);
    v = times(mul32, v ^ a[1]);
    v = times(mul32, v ^ a[2]);
    v = times(mul32, v ^ a[3]);
    v = mulmod(v, shift);
    // lanes 0..31: bit i of len -> x^(8 2^i); lanes 32..63: bit i of the fill -> x^(-8 2^i); the butterfly leaves both products everywhere in their half
    const uint32_t bits = lane < 32 ? (uint32_t)len : (uint32_t)(rows * WROW - len);
    uint32_t f = (bits >> (lane & 31)) & 1u ? g_pow2.v[lane] : ONE;
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) f = mulmod(f, __shfl_xor(f, d, 64));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    const uint32_t unfill = __shfl(f, 32, 64), zpow = __shfl(f, 0, 64);
    return mulmod(v, unfill) ^ mulmod(zpow, 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
}

}  // namespace l3c_crc_wave

#endif
