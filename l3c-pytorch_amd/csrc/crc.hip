// crc.hip -- sealed files (include/l3c_hip.h: l3c_u8_crc32, l3c_seal_append, l3c_seal_find / l3c_seal_write; the format is csrc/seal.h) and band
// seals (l3c_u8_crc32_bands, l3c_seal_append_bands, l3c_seal_find_bands / l3c_seal_write_bands: the second half of this file); the CRC-32
// of every band PAYLOAD of a banded encode's coarser records (l3c_band_payload_crc32, for the head part of the 'L3CH' section).
//
// l3c_u8_crc32: zlib's CRC-32 of n_items byte runs, integer only, the same words whatever the launch geometry, no atomics.
//
// Arithmetic.  A CRC register is a polynomial over GF(2) modulo P, reflected as zlib keeps it: bit 31 is x^0, `x` is 0x40000000, "times x" is
// a right shift with a conditional XOR of 0xEDB88320.  With R(A) the remainder of a message from a zero register and without the final
// XOR, R is linear, leading zero bytes do not change it, and
//     R(A | B) = R(A) x^(8 |B|) + R(B)              zlib.crc32(A) = R(A) + Z(|A|),  Z(n) = 0xFFFFFFFF x^(8 n) + 0xFFFFFFFF
// so a little-endian dword D that starts m bytes before the end of the message contributes D x^(8 m), wherever it is folded.
//
// First launch: a block per TILE of ROWS rows of 4096 bytes.  Thread t loads bytes 16 t .. 16 t + 15 of every row -- a wave reads whole
// cache lines -- and keeps one remainder per dword j of that load: acc_j = acc_j K + D_j per row, K = x^(8 * 4096).  "Times K" is linear in
// the 32 register bits, so it is the XOR of 8 table entries, one per nibble (MULK); the table lies in LDS 32 times, entry e of lane l at
// dword 32 e + (l & 31), so every lane of a 32-lane half reads a bank of its own: 8 conflict-free ds_read_b32 per dword, where a 256-entry
// byte table would be 4 reads that serialise about 3.4-fold on random indices.  The lookups of a row are cheap next to the latency of its
// load, so a whole tile is straight-line code with DEPTH rows of loads in flight per thread (fold_rows).  After the last row the four remainders are folded like the
// dwords of slice-by-4 (MUL32: "times x^32", the second table), the thread shifts its value over the 16 (255 - t) bytes that follow its
// column in a row (a bitwise multiplication with the constant SHIFT[t]), and the block XORs the 256 values: the remainder of the tile's rows,
// a last tile filled up with zero bytes to whole rows.  It goes to partial[item][tile].
// Second launch: a wavefront per item.  Lane l runs Horner over its share of the full tiles with x^(8 * TILE), weighs it with the tiles behind
// it, the wave XORs; lane 0 adds the last tile, multiplies by x^(-8 fill) to undo the zero fill, and XORs Z(item_bytes).
// The constants that depend on item_bytes come from the host as kernel arguments; all others are compile-time tables.
//
// l3c_u8_crc32_spans: the same for runs of DIFFERENT lengths anywhere in one buffer (a ragged group's frames), in three launches however many
// runs.  The tile code is shared (fold_tile); what the uniform form knows from its arguments -- which run a tile belongs to, the three
// length-dependent constants -- a first launch computes on the device from the span table (crc_spans.h holds the arithmetic and the
// table's validator, HIP-free), and the tile launch bisects a prefix of tile counts.
#include "l3c_common.h"
#include "crc_spans.h"
#include "crc_wave.h"
#include "seal.h"
#include "parity_plan.h"
#include "banded_rows.h"

namespace {

using namespace l3c_crc;      // crc_spans.h: mulmod, powmod, the tile geometry, the constants of a run's length
constexpr int MAX_GRID = 4096, DEPTH = 8;
constexpr int BAND_GRID = 1024;      // blocks of the band chunk launch: four a CU, each stages the tables once for many chunks

using namespace l3c_crc_wave;   // crc_wave.h: the nibble tables, times, row_step, and a wavefront on one byte run (wave_crc32)

struct __attribute__((aligned(4))) Quad {      // a 16-byte load that needs no more than the data's 4-byte alignment
    uint32_t d[4];
};

// the 16 bytes at item + off as four little-endian dwords, zero from byte `len` on; nothing at or behind item + len is read
__device__ __forceinline__ u32x4 load16(const uint8_t *item, int64_t off, int64_t len) {
    u32x4 r = {0u, 0u, 0u, 0u};
    if (off + 16 <= len) {
        const Quad q = *reinterpret_cast<const Quad *>(item + off);
        r = u32x4{q.d[0], q.d[1], q.d[2], q.d[3]};
    } else if (off < len) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        const int n = (int)(len - off);
#pragma unroll
        for (int i = 0; i < 15; ++i)
            if (i < n) w[i >> 2] |= (uint32_t)item[off + i] << (8 * (i & 3));
        r = u32x4{w[0], w[1], w[2], w[3]};
    }
    return r;
}

__device__ __forceinline__ u32x4 load_quad(const uint8_t *p) {
    const Quad q = *reinterpret_cast<const Quad *>(p);
    return u32x4{q.d[0], q.d[1], q.d[2], q.d[3]};
}

// N whole rows from p on, straight-line code: up to DEPTH rows of loads in flight per thread -- 16 waves x DEPTH KiB per CU, what it takes to
// hide the memory latency behind a row's arithmetic -- and, with no branch in between, a wait for exactly the load a row needs
template <int N, int STRIDE = ROW_BYTES>
__device__ __forceinline__ void fold_rows(const uint32_t *tab, uint32_t (&a)[4], const uint8_t *p) {
    constexpr int D = N < DEPTH ? N : DEPTH;
    u32x4 q[D];
#pragma unroll
    for (int i = 0; i < D; ++i) q[i] = load_quad(p + i * STRIDE);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const u32x4 cur = q[i % D];
        if (i + D < N) q[i % D] = load_quad(p + (i + D) * STRIDE);
        row_step(tab, a, cur);
    }
}

// What the tile launches of l3c_u8_crc32 and l3c_u8_crc32_spans share.  Tables: the two nibble tables into LDS (a barrier follows).
__device__ __forceinline__ void stage_tables(uint32_t *lds, int t) {
    for (int i = 0; i < 32; ++i) {
        const int idx = i * THREADS + t;
        lds[idx] = (&g_tables.v[0][0])[idx >> 5];
    }
}

// Tile `tile` of the run of item_bytes bytes at `base`, filled up with zero bytes to whole rows: the block's 256 threads fold it and thread 0
// stores its remainder to *out.  Ends with a barrier: wave_xor is free again.
__device__ __forceinline__ void fold_tile(const uint32_t *mulk, const uint32_t *mul32, uint32_t shift, uint32_t *wave_xor, int t,
                                          const uint8_t *base, int64_t item_bytes, int64_t tile, uint32_t *out) {
    const int64_t tile_at = tile * TILE_BYTES;
    const int64_t left = item_bytes - tile_at;                                          // > 0
    const int whole = left >= TILE_BYTES ? ROWS : (int)(left / ROW_BYTES);              // rows that lie inside the item: plain loads
    uint32_t a[4] = {0u, 0u, 0u, 0u};
    const uint8_t *p = base + tile_at + 16 * t;
    if (whole == ROWS) {
        fold_rows<ROWS>(mulk, a, p);
    } else {                                                                             // an item's last tile
        int g = 0;
        for (; g + DEPTH <= whole; g += DEPTH) fold_rows<DEPTH>(mulk, a, p + (int64_t)g * ROW_BYTES);
        for (; g < whole; ++g) fold_rows<1>(mulk, a, p + (int64_t)g * ROW_BYTES);
    }
    if (whole < ROWS && left > (int64_t)whole * ROW_BYTES)                               // the item ends inside this row
        row_step(mulk, a, load16(base, tile_at + (int64_t)whole * ROW_BYTES + 16 * t, item_bytes));
    uint32_t v = times(mul32, a[0]);
    v = times(mul32, v ^ a[1]);
    v = times(mul32, v ^ a[2]);
    v = times(mul32, v ^ a[3]);
    v = mulmod(v, shift);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    if ((t & 63) == 0) wave_xor[t >> 6] = v;
    __syncthreads();
    if (t == 0) *out = wave_xor[0] ^ wave_xor[1] ^ wave_xor[2] ^ wave_xor[3];
    __syncthreads();
}

__global__ __launch_bounds__(THREADS) void u8_crc32_tiles_kernel(const uint8_t *__restrict__ data, int64_t item_bytes, int64_t item_stride,
                                                                int64_t tiles_per_item, int64_t units, uint32_t *__restrict__ partial) {
    __shared__ uint32_t lds[2 * 128 * 32];
    __shared__ uint32_t wave_xor[THREADS / 64];
    const int t = threadIdx.x;
    stage_tables(lds, t);
    const uint32_t shift = g_shifts.v[t];
    const uint32_t *mulk = lds + (t & 31), *mul32 = lds + 128 * 32 + (t & 31);
    __syncthreads();
    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int64_t item = unit / tiles_per_item, tile = unit - item * tiles_per_item;
        fold_tile(mulk, mul32, shift, wave_xor, t, data + item * item_stride, item_bytes, tile, partial + unit);
    }
}

// l3c_u8_crc32_spans, first launch.  Block 0: first[k] = tiles of the spans in front of span k, first[n] = all tiles -- every thread sums a
// contiguous share of the spans, the block scans the 256 sums.  The other blocks: a thread per span and constant, the three words that
// depend on a span's length (crc_spans.h: span_k_last, span_unfill, span_z), which l3c_u8_crc32 computes on the host.
constexpr int PREP_THREADS = 256;
__global__ __launch_bounds__(PREP_THREADS) void u8_crc32_spans_prepare_kernel(const l3c_u8_span *__restrict__ spans, int64_t n,
                                                                              int64_t *__restrict__ first, uint32_t *__restrict__ consts) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        __shared__ int64_t sum[PREP_THREADS];
        const int64_t share = (n + PREP_THREADS - 1) / PREP_THREADS;
        const int64_t lo = t * share < n ? t * share : n, hi = lo + share < n ? lo + share : n;
        int64_t mine = 0;
        for (int64_t k = lo; k < hi; ++k) mine += tiles_of(spans[k].bytes);
        sum[t] = mine;
        __syncthreads();
        for (int d = 1; d < PREP_THREADS; d <<= 1) {
            const int64_t v = t >= d ? sum[t - d] : 0;
            __syncthreads();
            sum[t] += v;
            __syncthreads();
        }
        int64_t at = sum[t] - mine;
        for (int64_t k = lo; k < hi; ++k) {
            first[k] = at;
            at += tiles_of(spans[k].bytes);
        }
        if (t == PREP_THREADS - 1) first[n] = sum[t];
        return;
    }
    const int64_t step = (int64_t)(gridDim.x - 1) * PREP_THREADS;
    for (int64_t i = (int64_t)(blockIdx.x - 1) * PREP_THREADS + t; i < 3 * n; i += step) {      // constant-major: a wavefront runs ONE of the three loops
        const int c = (int)(i / n);
        const int64_t k = i - c * n, bytes = spans[k].bytes;
        consts[4 * k + c] = c == 0 ? span_k_last(bytes) : c == 1 ? span_unfill(bytes) : span_z(bytes);
    }
}

// Second launch: u8_crc32_tiles_kernel with the run looked up per tile.  Unit u is tile u - first[k] of the span k with
// first[k] <= u < first[k + 1] (a span of no tiles is never found); the bisection is uniform over the block.
__global__ __launch_bounds__(THREADS) void u8_crc32_span_tiles_kernel(const uint8_t *__restrict__ data, const l3c_u8_span *__restrict__ spans,
                                                                     const int64_t *__restrict__ first, int64_t n_spans, int64_t units,
                                                                     uint32_t *__restrict__ partial) {
    __shared__ uint32_t lds[2 * 128 * 32];
    __shared__ uint32_t wave_xor[THREADS / 64];
    const int t = threadIdx.x;
    stage_tables(lds, t);
    const uint32_t shift = g_shifts.v[t];
    const uint32_t *mulk = lds + (t & 31), *mul32 = lds + 128 * 32 + (t & 31);
    __syncthreads();
    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int64_t k = span_of_unit(first, n_spans, unit);
        const l3c_u8_span s = spans[k];
        fold_tile(mulk, mul32, shift, wave_xor, t, data + s.offset, s.bytes, unit - first[k], partial + unit);
    }
}

// k_last = x^(8 * bytes of the last tile's rows), unfill = x^(-8 * zero bytes it was filled up with), z = Z(item_bytes)
__global__ __launch_bounds__(64) void u8_crc32_combine_kernel(const uint32_t *__restrict__ partial, int64_t n_items, int64_t tiles_per_item,
                                                              uint32_t k_last, uint32_t unfill, uint32_t z, uint32_t *__restrict__ crc_out) {
    const int lane = threadIdx.x;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        if (tiles_per_item == 0) {
            if (lane == 0) crc_out[item] = z;
            continue;
        }
        const uint32_t *p = partial + item * tiles_per_item;
        const int64_t full = tiles_per_item - 1, share = (full + 63) / 64;
        const int64_t lo = lane * share < full ? lane * share : full, hi = lo + share < full ? lo + share : full;
        uint32_t a = 0;
        for (int64_t b = lo; b < hi; ++b) a = mulmod(a, K_TILE) ^ p[b];
        if (hi > lo && hi < full) a = mulmod(a, powmod(K_TILE, (uint64_t)(full - hi)));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a ^= __shfl_xor(a, d, 64);
        if (lane == 0) crc_out[item] = mulmod(mulmod(a, k_last) ^ p[full], unfill) ^ z;
    }
}

// Third launch: u8_crc32_combine_kernel with a span's tiles and constants read from the workspace.
__global__ __launch_bounds__(64) void u8_crc32_spans_combine_kernel(const uint32_t *__restrict__ partial, const int64_t *__restrict__ first,
                                                                    const SpanConsts *__restrict__ consts, int64_t n_spans,
                                                                    uint32_t *__restrict__ crc_out) {
    const int lane = threadIdx.x;
    for (int64_t span = blockIdx.x; span < n_spans; span += gridDim.x) {
        const int64_t at = first[span], tiles = first[span + 1] - at;
        const SpanConsts c = consts[span];
        if (tiles == 0) {
            if (lane == 0) crc_out[span] = c.z;
            continue;
        }
        const uint32_t *p = partial + at;
        const int64_t full = tiles - 1;
        uint32_t a = lane_share(p, full, lane);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a ^= __shfl_xor(a, d, 64);
        if (lane == 0) crc_out[span] = finish(a, p[full], c.k_last, c.unfill, c.z);
    }
}

// one thread per file: the 24 seal bytes as six words in registers, the check word bitwise over padding | words 0..4
__global__ __launch_bounds__(64) void seal_append_kernel(uint8_t *__restrict__ files, int64_t file_stride, int64_t *__restrict__ file_bytes,
                                                         const uint32_t *__restrict__ frame_crc, const uint16_t *__restrict__ padding,
                                                         uint64_t model_id, uint32_t generation, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int64_t n = file_bytes[b];
    if (n < 0) return;
    if (n > file_stride - L3C_SEAL_BYTES) {
        file_bytes[b] = -1;
        return;
    }
    uint32_t w[8];
    w[0] = padding ? (uint32_t)padding[4 * b] | (uint32_t)padding[4 * b + 1] << 16 : 0u;
    w[1] = padding ? (uint32_t)padding[4 * b + 2] | (uint32_t)padding[4 * b + 3] << 16 : 0u;
    w[2] = 0x5343334Cu;                                                // 'L3CS'
    w[3] = (uint32_t)l3c_sealing::VERSION | generation << 16;             // version, flags = 0, generation
    w[4] = frame_crc[b];
    w[5] = (uint32_t)model_id;
    w[6] = (uint32_t)(model_id >> 32);
    uint32_t crc = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        crc ^= w[i];
        for (int k = 0; k < 32; ++k) crc = (crc >> 1) ^ (POLY & (0u - (crc & 1u)));
    }
    w[7] = ~crc;
    uint8_t *dst = files + b * file_stride + n;
#pragma unroll
    for (int i = 0; i < L3C_SEAL_BYTES; ++i) dst[i] = (uint8_t)(w[2 + (i >> 2)] >> (8 * (i & 3)));
    file_bytes[b] = n + L3C_SEAL_BYTES;
}

// ---- l3c_u8_crc32_bands: every band of every plane of every frame, and every frame, from one pass over the bytes -------------------------
//
// A band is 64 bytes to a few hundred KiB, small next to the 128 KiB tile above, so the unit here is a WAVEFRONT on a chunk of WCHUNK
// bytes of one band: rows of WROW = 64 x 16 bytes, lane l on bytes 16 l .. 16 l + 15 of every row, the row step through MULW (x^(8 WROW))
// in LDS, a bank per lane as above.  The four waves of a block work on four chunks and never meet: no barrier behind the staging.
// The constants of a band length (BandConsts) exist twice per call -- every band but a plane's last has one length -- and come from the
// host; nothing is prepared on the device.
struct BandConsts {
    int64_t bytes;                    // of the band
    int64_t chunks;                   // ceil(bytes / WCHUNK)
    uint32_t k_last, unfill, z;       // as SpanConsts, for rows of WROW bytes and chunks of WCHUNK
    uint32_t k_band;                  // x^(8 bytes): Horner over the bands of a plane
};
struct BandsCall {
    BandConsts full, last;            // bands 0 .. n - 2 of a plane, band n - 1
    int64_t n_frames, planes, n, cpb; // cpb: partial words per band (the chunks of the longest band)
    int64_t plane_bytes, band_bytes, frame_stride;
    uint32_t k_plane, z_frame;        // x^(8 plane_bytes), Z(planes * plane_bytes)
};

__global__ __launch_bounds__(THREADS) void u8_crc32_band_chunks_kernel(const uint8_t *__restrict__ frames, BandsCall g, int64_t units,
                                                                      uint32_t *__restrict__ partial) {
    __shared__ uint32_t lds[2 * 128 * 32];
    const int t = threadIdx.x, lane = t & 63;
    for (int i = 0; i < 32; ++i) {                                           // MULW, then MUL32
        const int idx = i * THREADS + t;
        lds[idx] = idx < 128 * 32 ? g_tables.v[2][idx >> 5] : g_tables.v[1][(idx >> 5) - 128];
    }
    const uint32_t shift = g_shifts.v[THREADS - 64 + lane];                  // x^(8 * 16 (63 - lane)): the bytes of a row behind the lane's 16
    const uint32_t *mulw = lds + (t & 31), *mul32 = lds + 128 * 32 + (t & 31);
    __syncthreads();
    for (int64_t unit = (int64_t)blockIdx.x * (THREADS / 64) + (t >> 6); unit < units; unit += (int64_t)gridDim.x * (THREADS / 64)) {
        const int64_t band = unit / g.cpb, chunk = unit - band * g.cpb;      // band: (frame, plane, j) flattened
        const int64_t fp = band / g.n, j = band - fp * g.n, f = fp / g.planes, c = fp - f * g.planes;
        const int64_t bytes = j + 1 < g.n ? g.full.bytes : g.last.bytes;
        const int64_t chunk_at = chunk * WCHUNK;
        if (chunk_at >= bytes) continue;                                     // a shorter last band: the word is never read
        const uint8_t *base = frames + f * g.frame_stride + c * g.plane_bytes + j * g.band_bytes;
        const int64_t left = bytes - chunk_at;
        const int whole = left >= WCHUNK ? WROWS : (int)(left / WROW);
        uint32_t a[4] = {0u, 0u, 0u, 0u};
        const uint8_t *p = base + chunk_at + 16 * lane;
        if (whole == WROWS) {
            fold_rows<WROWS, WROW>(mulw, a, p);
        } else {
            int r = 0;
            for (; r + 4 <= whole; r += 4) fold_rows<4, WROW>(mulw, a, p + r * WROW);
            for (; r < whole; ++r) fold_rows<1, WROW>(mulw, a, p + r * WROW);
            if (left > (int64_t)whole * WROW) row_step(mulw, a, load16(base, chunk_at + (int64_t)whole * WROW + 16 * lane, bytes));
        }
        uint32_t v = times(mul32, a[0]);
        v = times(mul32, v ^ a[1]);
        v = times(mul32, v ^ a[2]);
        v = times(mul32, v ^ a[3]);
        v = mulmod(v, shift);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
        if (lane == 0) partial[unit] = v;
    }
}

// the remainder of one band from its chunks' (from a zero register, without Z)
__device__ __forceinline__ uint32_t band_raw(const uint32_t *p, const BandConsts &k) {
    uint32_t a = 0;
    for (int64_t i = 0; i + 1 < k.chunks; ++i) a = mulmod(a, K_WCHUNK) ^ p[i];
    if (k.chunks > 1) a = mulmod(a, k.k_last);
    return mulmod(a ^ p[k.chunks - 1], k.unfill);
}

// Second launch, a wavefront per frame.  Per plane: lane l finishes its contiguous share of the full bands, stores their words, and runs
// Horner over their remainders with x^(8 band_bytes), weighs it with the full bands behind the share, the wave XORs; lane 0 adds the last band
// and the plane to the frame's remainder.  raw(A | B) = raw(A) x^(8 |B|) + raw(B); Z(frame length) once at the end.
__global__ __launch_bounds__(64) void u8_crc32_bands_combine_kernel(const uint32_t *__restrict__ partial, BandsCall g, uint32_t *__restrict__ band_crc,
                                                                    uint32_t *__restrict__ frame_crc) {
    const int lane = threadIdx.x;
    const int64_t full = g.n - 1, share = (full + 63) / 64;
    const int64_t lo = lane * share < full ? lane * share : full, hi = lo + share < full ? lo + share : full;
    const bool weigh = hi > lo && hi < full;
    const uint32_t weight = weigh ? powmod(g.full.k_band, (uint64_t)(full - hi)) : ONE;
    for (int64_t f = blockIdx.x; f < g.n_frames; f += gridDim.x) {
        uint32_t frame = 0;
        for (int64_t c = 0; c < g.planes; ++c) {
            const int64_t band0 = (f * g.planes + c) * g.n;
            uint32_t a = 0;
            for (int64_t j = lo; j < hi; ++j) {
                const uint32_t r = band_raw(partial + (band0 + j) * g.cpb, g.full);
                band_crc[band0 + j] = r ^ g.full.z;
                a = mulmod(a, g.full.k_band) ^ r;
            }
            if (weigh) a = mulmod(a, weight);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) a ^= __shfl_xor(a, d, 64);
            if (lane == 0) {
                const uint32_t r = band_raw(partial + (band0 + full) * g.cpb, g.last);
                band_crc[band0 + full] = r ^ g.last.z;
                frame = mulmod(frame, g.k_plane) ^ mulmod(a, g.last.k_band) ^ r;
            }
        }
        if (lane == 0 && frame_crc) frame_crc[f] = frame ^ g.z_frame;
    }
}

// l3c_seal_append_bands, a wavefront per file.  The check word runs over M = 12 + 3 n little-endian words: the padding (2), the table
// (5 + 3 n), seal words 0..4.  Lane l folds its contiguous share bit by bit, weighs it with x^(32 * words behind the share), the wave
// XORs, Z(4 M) comes from the host.  Every lane stores the bytes of the words it walks: byte stores, a file ends anywhere.
__global__ __launch_bounds__(64) void seal_append_bands_kernel(uint8_t *__restrict__ files, int64_t file_stride, int64_t *__restrict__ file_bytes,
                                                               const uint32_t *__restrict__ frame_crc, const uint32_t *__restrict__ band_crc,
                                                               int n, uint32_t band_len, const uint16_t *__restrict__ padding, uint64_t model_id,
                                                               uint32_t generation, uint32_t z_check, int64_t B) {
    const int lane = threadIdx.x;
    const int M = 12 + 3 * n, T = 20 + 12 * n;
    const int share = (M + 63) / 64;
    const int lo = lane * share < M ? lane * share : M, hi = lo + share < M ? lo + share : M;
    const uint32_t weight = powmod(POLY, (uint64_t)(M - hi));                      // POLY is x^32
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const int64_t at = file_bytes[b];
        if (at < 0) continue;
        if (at > file_stride - (T + L3C_SEAL_BYTES)) {
            if (lane == 0) file_bytes[b] = -1;
            continue;
        }
        uint8_t *dst = files + b * file_stride + at;                              // word i of the message lies at dst + 4 (i - 2)
        uint32_t a = 0;
        for (int i = lo; i < hi; ++i) {
            uint32_t w;
            if (i < 2) w = padding ? (uint32_t)padding[4 * b + 2 * i] | (uint32_t)padding[4 * b + 2 * i + 1] << 16 : 0u;
            else if (i == 2) w = 0x5443334Cu;                                      // 'L3CT'
            else if (i == 3) w = (uint32_t)n;                                      // n, reserved = 0
            else if (i == 4) w = band_len;
            else if (i < 5 + 3 * n) w = band_crc[b * 3 * n + (i - 5)];
            else if (i == 5 + 3 * n) w = (uint32_t)T;
            else if (i == 6 + 3 * n) w = 0x9284E246u;                              // the separator 46 E2 84 92
            else if (i == 7 + 3 * n) w = 0x5343334Cu;                              // 'L3CS'
            else if (i == 8 + 3 * n) w = (uint32_t)l3c_sealing::VERSION_BANDS | generation << 16;
            else if (i == 9 + 3 * n) w = frame_crc[b];
            else if (i == 10 + 3 * n) w = (uint32_t)model_id;
            else w = (uint32_t)(model_id >> 32);
            if (i >= 2)
                for (int k = 0; k < 4; ++k) dst[4 * (i - 2) + k] = (uint8_t)(w >> (8 * k));
            a ^= w;
            for (int k = 0; k < 32; ++k) a = (a >> 1) ^ (POLY & (0u - (a & 1u)));
        }
        a = mulmod(a, weight);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a ^= __shfl_xor(a, d, 64);
        if (lane == 0) {
            const uint32_t check = a ^ z_check;
            for (int k = 0; k < 4; ++k) dst[T + 20 + k] = (uint8_t)(check >> (8 * k));
            file_bytes[b] = at + T + L3C_SEAL_BYTES;
        }
    }
}

// ---- l3c_band_payload_crc32: every band PAYLOAD of the coder output of several records, lengths known on the device alone ----------------
//
// A wavefront per payload (tens of bytes to a few KiB: the coarser records), the rows of WROW bytes and the MULW step of the band chunks
// above; the four waves of a block never meet.  A payload's slot is only 4-byte aligned and holds garbage behind its length: dword loads
// in front of the 4-byte-rounded end (one 16-byte load where the address allows it), the bytes of the last dword behind the length masked.
// The length's two constants, x^(8 len) for Z and x^(-8 fill) for the zero fill of the last row, are products over the set bits of len and
// fill: lanes 0..31 and 32..63 each hold one factor (X8_POW2) and a five-step butterfly multiplies them.
struct PayloadRecords {
    l3c_banded_scale sc[l3c_parity::HEAD_MAX_RECORDS];
    int64_t first[l3c_parity::HEAD_MAX_RECORDS + 1];      // payloads (b, c, j) in front of the record; [count]: all
    int32_t n[l3c_parity::HEAD_MAX_RECORDS];
    int32_t count;
};

__global__ __launch_bounds__(THREADS) void band_payload_crc32_kernel(PayloadRecords h, uint32_t *__restrict__ crc_out) {
    __shared__ uint32_t lds[WAVE_TABLE_WORDS];
    const int t = threadIdx.x, lane = t & 63;
    stage_wave_tables(lds, t);
    __syncthreads();
    const int64_t total = h.first[h.count];
    for (int64_t unit = (int64_t)blockIdx.x * (THREADS / 64) + (t >> 6); unit < total; unit += (int64_t)gridDim.x * (THREADS / 64)) {
        int k = 0;
        while (k + 1 < h.count && unit >= h.first[k + 1]) ++k;
        const l3c_banded_scale &sc = h.sc[k];
        const int64_t n = h.n[k], at = unit - h.first[k], s = at / n, j = at - s * n;
        const uint32_t stated = band_nbytes(sc, n, s, j);
        const int64_t stride = j + 1 < n ? sc.stride_full : sc.stride_last;
        if (stated == L3C_AC_OVERRUN || (int64_t)stated > stride) {          // (its file is refused anyway)
            if (lane == 0) crc_out[unit] = 0u;
            continue;
        }
        const uint8_t *p = band_row(sc, n, s, j);
        const uint32_t crc = wave_crc32(lds, lane, p, (int64_t)stated);
        if (lane == 0) crc_out[unit] = crc;
    }
}

}  // namespace

extern "C" {

int l3c_band_payload_crc32(const l3c_banded_scale *scales_host, int n_scales, int64_t B, uint32_t *crc_out, l3c_stream_t stream) {
    L3C_REQUIRE(scales_host && crc_out, "null pointer");
    L3C_REQUIRE(n_scales >= 1 && n_scales <= l3c_parity::HEAD_MAX_RECORDS, "n_scales must be in 1..8");
    L3C_REQUIRE(B >= 1 && B < 65536, "bad batch size (1 .. 65535)");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(crc_out) & 3) == 0, "crc_out must be 4-byte aligned");
    PayloadRecords h{};
    h.count = n_scales;
    for (int k = 0; k < n_scales; ++k) {
        const l3c_banded_scale &sc = scales_host[k];
        L3C_REQUIRE(sc.C >= 1 && sc.C <= 1024 && sc.H > 0 && sc.W > 0, "C must be in 1..1024, H and W positive");
        L3C_REQUIRE(sc.band_len > 0 && sc.band_len % 64 == 0, "band_len must be a positive multiple of 64");
        const int64_t hw = (int64_t)sc.H * sc.W, n = (hw + sc.band_len - 1) / sc.band_len;
        L3C_REQUIRE(n <= 1024, "more than 1024 bands per channel");
        L3C_REQUIRE(sc.out_last && sc.nbytes_last && (n == 1 || (sc.out_full && sc.nbytes_full)), "null pointer in a scale");
        L3C_REQUIRE(sc.stride_last > 0 && sc.stride_last % 4 == 0 && (n == 1 || (sc.stride_full > 0 && sc.stride_full % 4 == 0)),
                    "the coder strides must be positive multiples of 4");
        L3C_REQUIRE((reinterpret_cast<uintptr_t>(sc.out_last) & 3) == 0 && (reinterpret_cast<uintptr_t>(sc.out_full) & 3) == 0 &&
                        (reinterpret_cast<uintptr_t>(sc.nbytes_last) & 3) == 0 && (reinterpret_cast<uintptr_t>(sc.nbytes_full) & 3) == 0,
                    "the coder outputs and the length arrays must be 4-byte aligned");
        h.sc[k] = sc, h.n[k] = (int32_t)n, h.first[k + 1] = h.first[k] + B * sc.C * n;
    }
    const int64_t blocks = (h.first[n_scales] + THREADS / 64 - 1) / (THREADS / 64);
    hipLaunchKernelGGL(band_payload_crc32_kernel, dim3((unsigned)(blocks < BAND_GRID ? blocks : BAND_GRID)), dim3(THREADS), 0, l3c::as_stream(stream), h,
                       crc_out);
    return l3c::check_launch("band_payload_crc32_kernel");
}

int l3c_seal_find(const uint8_t *file_host, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out) {
    L3C_REQUIRE(file_host && file_bytes >= 0, "null pointer or negative size");
    return l3c_sealing::find(file_host, file_bytes, body_bytes_out, seal_out, l3c::error_buffer(), 512);
}

int l3c_seal_write(const l3c_seal *seal_host, const uint8_t *padding8_host, uint8_t *dst_host) {
    L3C_REQUIRE(seal_host && padding8_host && dst_host, "null pointer");
    l3c_sealing::write(*seal_host, padding8_host, dst_host);
    return L3C_OK;
}

int l3c_u8_crc32_tile(int *thread_bytes_out, int *block_bytes_out) {
    L3C_REQUIRE(thread_bytes_out && block_bytes_out, "null pointer");
    *thread_bytes_out = THREAD_BYTES;
    *block_bytes_out = TILE_BYTES;
    return L3C_OK;
}

int64_t l3c_u8_crc32_workspace_bytes(int64_t n_items, int64_t item_bytes) {
    if (n_items < 1 || item_bytes < 0 || tiles_of(item_bytes) >= ((int64_t)1 << 40) / n_items)
        return l3c::fail(L3C_ERR_INVALID_ARG, "%s", "bad sizes: n_items >= 1, item_bytes >= 0, n_items * tiles below 2^40");
    return (4 * n_items * tiles_of(item_bytes) + 15) / 16 * 16 + 16;
}

int l3c_u8_crc32(const uint8_t *data, int64_t n_items, int64_t item_bytes, int64_t item_stride, uint32_t *crc_out, void *workspace,
                 int64_t workspace_bytes, l3c_stream_t stream) {
    L3C_REQUIRE(data && crc_out && workspace, "null pointer");
    const int64_t need = l3c_u8_crc32_workspace_bytes(n_items, item_bytes);
    if (need < 0) return (int)need;
    L3C_REQUIRE(item_stride % 4 == 0 && item_stride >= item_bytes, "item_stride must be a multiple of 4 and at least item_bytes");
    L3C_REQUIRE(n_items == 1 || item_stride <= INT64_MAX / n_items, "n_items * item_stride overflows");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(data) & 3) == 0 && (reinterpret_cast<uintptr_t>(crc_out) & 3) == 0, "data and crc_out must be 4-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "the workspace must be 16-byte aligned");
    L3C_REQUIRE(workspace_bytes >= need, "workspace_bytes too small");
    const hipStream_t st = l3c::as_stream(stream);
    const int64_t tiles = tiles_of(item_bytes), units = n_items * tiles;
    uint32_t *partial = static_cast<uint32_t *>(workspace);
    uint32_t k_last = 0, unfill = 0, z = 0;
    if (tiles) {
        const int64_t last_rows_bytes = (item_bytes - (tiles - 1) * TILE_BYTES + ROW_BYTES - 1) / ROW_BYTES * ROW_BYTES;
        k_last = powmod(X8, (uint64_t)last_rows_bytes);
        unfill = powmod(X8_INV, (uint64_t)((tiles - 1) * TILE_BYTES + last_rows_bytes - item_bytes));
        z = mulmod(powmod(X8, (uint64_t)item_bytes), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
        hipLaunchKernelGGL(u8_crc32_tiles_kernel, dim3((unsigned)(units < MAX_GRID ? units : MAX_GRID)), dim3(THREADS), 0, st, data, item_bytes,
                           item_stride, tiles, units, partial);
        const int rc = l3c::check_launch("u8_crc32_tiles_kernel");
        if (rc != L3C_OK) return rc;
    }
    hipLaunchKernelGGL(u8_crc32_combine_kernel, dim3((unsigned)(n_items < MAX_GRID ? n_items : MAX_GRID)), dim3(64), 0, st, partial, n_items, tiles,
                       k_last, unfill, z, crc_out);
    return l3c::check_launch("u8_crc32_combine_kernel");
}

int64_t l3c_u8_crc32_spans_workspace_bytes(const l3c_u8_span *spans_host, int64_t n_spans) {
    const int64_t tiles = count_tiles(spans_host, n_spans, l3c::error_buffer(), 512);
    return tiles < 0 ? tiles : span_workspace(n_spans, tiles).bytes;
}

int l3c_u8_crc32_spans(const uint8_t *data, int64_t data_bytes, const l3c_u8_span *spans_host, const l3c_u8_span *spans, int64_t n_spans,
                       uint32_t *crc_out, void *workspace, int64_t workspace_bytes, l3c_stream_t stream) {
    L3C_REQUIRE(data && spans_host && spans && crc_out && workspace, "null pointer");
    const int64_t units = check_spans(spans_host, n_spans, data_bytes, l3c::error_buffer(), 512);
    if (units < 0) return (int)units;
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(data) & 3) == 0 && (reinterpret_cast<uintptr_t>(crc_out) & 3) == 0, "data and crc_out must be 4-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(spans) & 7) == 0, "spans (the device table) must be 8-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "the workspace must be 16-byte aligned");
    const SpanWorkspace w = span_workspace(n_spans, units);
    L3C_REQUIRE(workspace_bytes >= w.bytes, "workspace_bytes too small");
    const hipStream_t st = l3c::as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    int64_t *first = reinterpret_cast<int64_t *>(ws + w.first_at);
    SpanConsts *consts = reinterpret_cast<SpanConsts *>(ws + w.consts_at);
    uint32_t *partial = reinterpret_cast<uint32_t *>(ws + w.partial_at);
    const int64_t prep = (3 * n_spans + PREP_THREADS - 1) / PREP_THREADS;
    hipLaunchKernelGGL(u8_crc32_spans_prepare_kernel, dim3(1 + (unsigned)(prep < MAX_GRID ? prep : MAX_GRID)), dim3(PREP_THREADS), 0, st, spans, n_spans,
                       first, reinterpret_cast<uint32_t *>(consts));
    int rc = l3c::check_launch("u8_crc32_spans_prepare_kernel");
    if (rc != L3C_OK) return rc;
    if (units) {
        hipLaunchKernelGGL(u8_crc32_span_tiles_kernel, dim3((unsigned)(units < MAX_GRID ? units : MAX_GRID)), dim3(THREADS), 0, st, data, spans, first,
                           n_spans, units, partial);
        rc = l3c::check_launch("u8_crc32_span_tiles_kernel");
        if (rc != L3C_OK) return rc;
    }
    hipLaunchKernelGGL(u8_crc32_spans_combine_kernel, dim3((unsigned)(n_spans < MAX_GRID ? n_spans : MAX_GRID)), dim3(64), 0, st, partial, first, consts,
                       n_spans, crc_out);
    return l3c::check_launch("u8_crc32_spans_combine_kernel");
}

int l3c_seal_append(uint8_t *files, int64_t file_stride, int64_t *file_bytes, const uint32_t *frame_crc, const uint16_t *padding,
                    uint64_t model_id, int64_t B, l3c_stream_t stream) {
    L3C_REQUIRE(files && file_bytes && frame_crc, "null pointer");
    L3C_REQUIRE(B > 0 && B < 65536, "bad batch size (1 .. 65535)");
    L3C_REQUIRE(file_stride > 0 && file_stride <= INT64_MAX / B, "bad file_stride");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(file_bytes) & 7) == 0 && (reinterpret_cast<uintptr_t>(frame_crc) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(padding) & 1) == 0,
                "file_bytes, frame_crc and padding must be aligned to their element size");
    hipLaunchKernelGGL(seal_append_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, l3c::as_stream(stream), files, file_stride, file_bytes,
                       frame_crc, padding, model_id, (uint32_t)L3C_BITSTREAM_GENERATION, B);
    return l3c::check_launch("seal_append_kernel");
}

int64_t l3c_seal_bands_bytes(int n) {
    if (n < 1 || n > l3c_sealing::MAX_BANDS) return l3c::fail(L3C_ERR_INVALID_ARG, "%s", "n must be in 1..1024");
    return l3c_sealing::table_bytes(n) + L3C_SEAL_BYTES;
}

int l3c_seal_find_bands(const uint8_t *file_host, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out) {
    L3C_REQUIRE(file_host && file_bytes >= 0, "null pointer or negative size");
    return l3c_sealing::find_bands(file_host, file_bytes, body_bytes_out, seal_out, bands_out, l3c::error_buffer(), 512);
}

int l3c_seal_write_bands(const l3c_seal *seal_host, const uint8_t *padding8_host, const uint32_t *band_crc_host, int n, uint32_t band_len,
                         uint8_t *dst_host) {
    L3C_REQUIRE(seal_host && padding8_host && band_crc_host && dst_host, "null pointer");
    L3C_REQUIRE(n >= 1 && n <= l3c_sealing::MAX_BANDS && band_len > 0, "n must be in 1..1024 and band_len positive");
    uint8_t *crc = dst_host + 12;                                            // the table's words, little-endian, where write_bands puts them
    for (int i = 0; i < 3 * n; ++i) l3c_sealing::put(crc + 4 * i, band_crc_host[i], 4);
    l3c_sealing::write_bands(*seal_host, padding8_host, crc, n, band_len, dst_host);
    return L3C_OK;
}

// l3c_seal_parity_bytes and l3c_seal_parity_rs_bytes: payload_bytes = R times the sum of plen; `what`: the caller's message
static int64_t parity_tail_bytes(int n, int m, int R, int64_t payload_bytes, const char *what) {
    if (n < 1 || n > l3c_sealing::MAX_BANDS || m < 1 || m > n || R < 1 || R > l3c_sealing::MAX_PARITY_STREAMS || payload_bytes < 0 ||
        payload_bytes % R != 0 || payload_bytes > (int64_t)UINT32_MAX - l3c_sealing::parity_section_bytes(m, R, 0))
        return l3c::fail(L3C_ERR_INVALID_ARG, "%s", what);
    return l3c_sealing::parity_section_bytes(m, R, payload_bytes / R) + l3c_sealing::table_bytes(n) + L3C_SEAL_BYTES;
}

// l3c_seal_write_parity (R = 1) and l3c_seal_write_parity_rs
static int write_parity_tail(const l3c_seal *seal_host, const uint8_t *padding8_host, const uint32_t *band_crc_host, int n, uint32_t band_len, int G,
                             int R, const uint32_t *plen_host, const uint8_t *payloads_host, uint8_t *dst_host) {
    L3C_REQUIRE(seal_host && padding8_host && band_crc_host && plen_host && dst_host, "null pointer");
    L3C_REQUIRE(n >= 1 && n <= l3c_sealing::MAX_BANDS && band_len > 0, "n must be in 1..1024 and band_len positive");
    L3C_REQUIRE(R >= 1 && R <= l3c_sealing::MAX_PARITY_STREAMS, "R must be in 1..4");
    L3C_REQUIRE(G >= 1 && G <= n, "G must be in 1..n");
    L3C_REQUIRE(R == 1 || G <= l3c_sealing::MAX_RS_GROUP, "more than one parity stream needs groups of at most 255 bands");
    const int m = (n + G - 1) / G;
    int64_t sum = 0;
    for (int i = 0; i < 3 * m; ++i) sum += plen_host[i];
    L3C_REQUIRE(sum == 0 || payloads_host, "null pointer (payloads_host)");
    L3C_REQUIRE(R * sum <= (int64_t)UINT32_MAX - l3c_sealing::parity_section_bytes(m, R, 0), "the section must stay below 2^32 bytes");
    uint8_t *crc = dst_host + l3c_sealing::parity_section_bytes(m, R, sum) + 12;   // the table's words, little-endian, where write_tail puts them
    for (int i = 0; i < 3 * n; ++i) l3c_sealing::put(crc + 4 * i, band_crc_host[i], 4);
    l3c_sealing::write_parity_rs(*seal_host, padding8_host, crc, n, band_len, G, m, R, plen_host, payloads_host, dst_host);
    return L3C_OK;
}

static const char PARITY_BYTES_WHAT[] = "n must be in 1..1024, m in 1..n, and the section must stay below 2^32 bytes";
static const char PARITY_RS_BYTES_WHAT[] =
    "n must be in 1..1024, m in 1..n, R in 1..4, payload_bytes a multiple of R, and the section must stay below 2^32 bytes";

int64_t l3c_seal_parity_bytes(int n, int m, int64_t payload_bytes) { return parity_tail_bytes(n, m, 1, payload_bytes, PARITY_BYTES_WHAT); }

int l3c_seal_find_parity(const uint8_t *file_host, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out,
                         l3c_seal_parity *parity_out) {
    L3C_REQUIRE(file_host && file_bytes >= 0, "null pointer or negative size");
    return l3c_sealing::find_parity(file_host, file_bytes, body_bytes_out, seal_out, bands_out, parity_out, l3c::error_buffer(), 512);
}

int l3c_seal_write_parity(const l3c_seal *seal_host, const uint8_t *padding8_host, const uint32_t *band_crc_host, int n, uint32_t band_len, int G,
                          const uint32_t *plen_host, const uint8_t *payloads_host, uint8_t *dst_host) {
    return write_parity_tail(seal_host, padding8_host, band_crc_host, n, band_len, G, 1, plen_host, payloads_host, dst_host);
}

int64_t l3c_seal_parity_rs_bytes(int n, int m, int R, int64_t payload_bytes) {
    return parity_tail_bytes(n, m, R, payload_bytes, R == 1 ? PARITY_BYTES_WHAT : PARITY_RS_BYTES_WHAT);
}

int l3c_seal_find_parity_rs(const uint8_t *file_host, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out,
                            l3c_seal_parity_rs *parity_out) {
    L3C_REQUIRE(file_host && file_bytes >= 0, "null pointer or negative size");
    return l3c_sealing::find_parity_rs(file_host, file_bytes, body_bytes_out, seal_out, bands_out, parity_out, l3c::error_buffer(), 512);
}

int l3c_seal_write_parity_rs(const l3c_seal *seal_host, const uint8_t *padding8_host, const uint32_t *band_crc_host, int n, uint32_t band_len, int G,
                             int R, const uint32_t *plen_host, const uint8_t *payloads_host, uint8_t *dst_host) {
    return write_parity_tail(seal_host, padding8_host, band_crc_host, n, band_len, G, R, plen_host, payloads_host, dst_host);
}

int l3c_seal_find_head(const uint8_t *file_host, int64_t file_bytes, l3c_seal_head *head_out) {
    L3C_REQUIRE(file_host && file_bytes >= 0 && head_out, "null pointer or negative size");
    l3c_sealing::HeadAt head;
    const int rc = l3c_sealing::find_head(file_host, file_bytes, &head, l3c::error_buffer(), 512);
    head_out->at = head.at, head_out->bytes = head.bytes, head_out->check_ok = head.check_ok, head_out->n_records = head.n_records;
    return rc;
}

namespace {
// the constants of a band of `bytes` bytes
BandConsts band_consts(int64_t bytes) {
    BandConsts k{};
    k.bytes = bytes;
    k.chunks = (bytes + WCHUNK - 1) / WCHUNK;
    const int64_t last_rows_bytes = (bytes - (k.chunks - 1) * WCHUNK + WROW - 1) / WROW * WROW;
    k.k_last = powmod(X8, (uint64_t)last_rows_bytes);
    k.unfill = powmod(X8_INV, (uint64_t)((k.chunks - 1) * WCHUNK + last_rows_bytes - bytes));
    k.z = span_z(bytes);
    k.k_band = powmod(X8, (uint64_t)bytes);
    return k;
}
// the arguments of l3c_u8_crc32_bands that size its work -> units (partial words), or L3C_ERR_INVALID_ARG
int64_t bands_call(int64_t n_frames, int planes, int64_t plane_bytes, int64_t band_bytes, BandsCall *g) {
    if (n_frames < 1 || planes < 1 || planes > 1024 || plane_bytes < 4 || plane_bytes % 4 || band_bytes < 4 || band_bytes % 4)
        return l3c::fail(L3C_ERR_INVALID_ARG, "%s", "bad sizes: n_frames >= 1, planes in 1..1024, plane_bytes and band_bytes positive multiples of 4");
    const int64_t n = (plane_bytes - 1) / band_bytes + 1, longest = n > 1 ? band_bytes : plane_bytes;
    const int64_t cpb = (longest - 1) / WCHUNK + 1;                          // n cpb < plane_bytes / 2 + 2: no overflow below
    if (plane_bytes > INT64_MAX / 4 / planes || planes * n * cpb >= ((int64_t)1 << 40) / n_frames)
        return l3c::fail(L3C_ERR_INVALID_ARG, "%s", "bad sizes: n_frames * planes * bands * chunks per band must stay below 2^40");
    if (g) {
        g->full = band_consts(longest);
        g->last = band_consts(plane_bytes - (n - 1) * band_bytes);
        g->n_frames = n_frames, g->planes = planes, g->n = n, g->cpb = cpb;
        g->plane_bytes = plane_bytes, g->band_bytes = band_bytes;
        g->k_plane = powmod(X8, (uint64_t)plane_bytes);
        g->z_frame = span_z(planes * plane_bytes);
    }
    return n_frames * planes * n * cpb;
}
}  // namespace

int64_t l3c_u8_crc32_bands_workspace_bytes(int64_t n_frames, int planes, int64_t plane_bytes, int64_t band_bytes) {
    const int64_t units = bands_call(n_frames, planes, plane_bytes, band_bytes, nullptr);
    return units < 0 ? units : (4 * units + 15) / 16 * 16 + 16;
}

int l3c_u8_crc32_bands(const uint8_t *frames, int64_t n_frames, int planes, int64_t plane_bytes, int64_t band_bytes, int64_t frame_stride,
                       uint32_t *band_crc_out, uint32_t *frame_crc_out, void *workspace, int64_t workspace_bytes, l3c_stream_t stream) {
    L3C_REQUIRE(frames && band_crc_out && workspace, "null pointer");
    BandsCall g{};
    const int64_t units = bands_call(n_frames, planes, plane_bytes, band_bytes, &g);
    if (units < 0) return (int)units;
    L3C_REQUIRE(frame_stride % 4 == 0 && frame_stride >= planes * plane_bytes, "frame_stride must be a multiple of 4 and at least planes * plane_bytes");
    L3C_REQUIRE(n_frames == 1 || frame_stride <= INT64_MAX / n_frames, "n_frames * frame_stride overflows");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (reinterpret_cast<uintptr_t>(band_crc_out) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(frame_crc_out) & 3) == 0,
                "frames, band_crc_out and frame_crc_out must be 4-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "the workspace must be 16-byte aligned");
    L3C_REQUIRE(workspace_bytes >= (4 * units + 15) / 16 * 16 + 16, "workspace_bytes too small");
    g.frame_stride = frame_stride;
    const hipStream_t st = l3c::as_stream(stream);
    uint32_t *partial = static_cast<uint32_t *>(workspace);
    const int64_t blocks = (units + THREADS / 64 - 1) / (THREADS / 64);
    hipLaunchKernelGGL(u8_crc32_band_chunks_kernel, dim3((unsigned)(blocks < BAND_GRID ? blocks : BAND_GRID)), dim3(THREADS), 0, st, frames, g, units,
                       partial);
    const int rc = l3c::check_launch("u8_crc32_band_chunks_kernel");
    if (rc != L3C_OK) return rc;
    hipLaunchKernelGGL(u8_crc32_bands_combine_kernel, dim3((unsigned)(n_frames < MAX_GRID ? n_frames : MAX_GRID)), dim3(64), 0, st, partial, g,
                       band_crc_out, frame_crc_out);
    return l3c::check_launch("u8_crc32_bands_combine_kernel");
}

int l3c_seal_append_bands(uint8_t *files, int64_t file_stride, int64_t *file_bytes, const uint32_t *frame_crc, const uint32_t *band_crc, int n,
                          uint32_t band_len, const uint16_t *padding, uint64_t model_id, int64_t B, l3c_stream_t stream) {
    L3C_REQUIRE(files && file_bytes && frame_crc && band_crc, "null pointer");
    L3C_REQUIRE(B > 0 && B < 65536, "bad batch size (1 .. 65535)");
    L3C_REQUIRE(n >= 1 && n <= l3c_sealing::MAX_BANDS && band_len > 0, "n must be in 1..1024 and band_len positive");
    L3C_REQUIRE(file_stride > 0 && file_stride <= INT64_MAX / B, "bad file_stride");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(file_bytes) & 7) == 0 && (reinterpret_cast<uintptr_t>(frame_crc) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(band_crc) & 3) == 0 && (reinterpret_cast<uintptr_t>(padding) & 1) == 0,
                "file_bytes, frame_crc, band_crc and padding must be aligned to their element size");
    hipLaunchKernelGGL(seal_append_bands_kernel, dim3((unsigned)(B < MAX_GRID ? B : MAX_GRID)), dim3(64), 0, l3c::as_stream(stream), files, file_stride,
                       file_bytes, frame_crc, band_crc, n, band_len, padding, model_id, (uint32_t)L3C_BITSTREAM_GENERATION,
                       span_z(4 * (int64_t)(12 + 3 * n)), B);
    return l3c::check_launch("seal_append_bands_kernel");
}
}
