// parity.hip -- parity bands (include/l3c_hip.h: l3c_band_parity, l3c_u8_xor_spans, l3c_band_rebuild; the format is csrc/seal.h, version 3).
//
// Both kernels are streaming XORs over byte streams of different lengths and share one fold: a block owns a TILE of 4096 bytes of ONE
// output stream (grid.y = the stream), a thread 16 bytes of it, and walks the stream's members, eight at a time (fold_members): one 16-byte
// load per member where the member starts 16-byte aligned and the 16 bytes lie in front of its 4-byte-rounded end, dword loads otherwise (the
// coder's rows are only guaranteed a stride that is a multiple of 4).  Nothing at or behind a member's 4-byte-rounded end is read; the bytes
// of its last dword behind its length are masked to zero (the coder's slots hold garbage there), so every member counts as zero-extended.
// A wave reads 1 KiB of a member per step; the members of a group are independent loads, issued eight deep.
// Stores are 16 bytes where the slot is 16-byte aligned and the 16 bytes lie inside what the call writes, dwords otherwise; nothing outside
// that range is written.  No atomics, no LDS, no allocation, no host synchronisation.
//
// l3c_band_parity_rs and l3c_u8_gf_spans are the same two kernels over GF(2^8) (polynomial 0x11D, alpha = 0x02: the 'L3CQ' section of
// csrc/seal.h), with the same loads, masks and stores.  The only field operation is "times alpha" on four packed bytes (xtime: 5 VALU
// instructions per dword): the encoder keeps R accumulators and applies Horner's rule over the members, so a member is loaded once for all
// rows; the repair side multiplies each member by a coefficient that is uniform over the block, by shift and add under scalar branches.
//
// l3c_head_parity (the head part of the 'L3CH' section) is l3c_band_parity_rs over SEVERAL records of any channel count in one launch:
// grid.y runs over (record, b, c, g), the records travel by value, and a block does the work of its record's band_parity_rs block (rs_stream).
//
// l3c_band_rebuild is the repair-side counterpart of rs_stream: where l3c_u8_gf_spans rebuilds ONE payload per output group, a block of
// band_rebuild_kernel loads every source of a group once and keeps an accumulator per erased member (at most four); its parity rows are
// read where they lie in the file's section, at any byte offset (the aligned dwords around a run, funnel-shifted), and it writes IN PLACE:
// outputs and member sources are spans of one buffer, so the host check refuses any overlap between them (parity_plan.h: check_rebuild).
//
// XOR is the R = 1 / every-coefficient-1 case of the GF(2^8) kernels and could be their instantiation; it keeps kernels of its own because
// that instantiation measured 8 to 10 % slower (profiles/r23_parity_one_path_latency.log).  The host side is one path: the entry points of a
// family share their argument checks (check_band_parity, u8_spans).
#include <exception>
#include <vector>

#include "l3c_common.h"
#include "parity_plan.h"
#include "banded_rows.h"

namespace {

using namespace l3c_parity;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Member {
    const uint8_t *p;      // 4-byte aligned
    int64_t len;           // bytes that count; the rest of the last dword is masked
};

// bytes [off, off + 16) of a member as four dwords, zero at and behind its 4-byte-rounded end (the bytes of its last dword behind `len`
// still as they lie in memory: mask16); off % 16 == 0
__device__ __forceinline__ u32x4 load16(const Member &m, int64_t off) {
    const int64_t end4 = (m.len + 3) & ~(int64_t)3;
    u32x4 q = {0u, 0u, 0u, 0u};
    if (off + 16 <= end4 && (reinterpret_cast<uintptr_t>(m.p) & 15) == 0) {
        q = *reinterpret_cast<const u32x4 *>(m.p + off);
    } else if (off < end4) {
        if (off < end4) q.x = *reinterpret_cast<const uint32_t *>(m.p + off);
        if (off + 4 < end4) q.y = *reinterpret_cast<const uint32_t *>(m.p + off + 4);
        if (off + 8 < end4) q.z = *reinterpret_cast<const uint32_t *>(m.p + off + 8);
        if (off + 12 < end4) q.w = *reinterpret_cast<const uint32_t *>(m.p + off + 12);
    }
    return q;
}

// the dwords of load16 with the bytes at and behind `len` cleared
__device__ __forceinline__ u32x4 mask16(u32x4 q, int64_t len, int64_t off) {
    uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t keep = len - (off + 4 * i);                  // bytes of dword i that belong to the member
        if (keep < 4) w[i] = keep <= 0 ? 0u : w[i] & (0xFFFFFFFFu >> (8 * (4 - (int)keep)));
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}

// The XOR over members 0 .. count - 1 (member(k) -> Member, uniform over the block) of their bytes [off, off + 16).  DEPTH members at a time:
// their descriptors are read first, then their loads issued, then folded -- two memory latencies per DEPTH members, not per member; a
// group's members are independent streams, so that is all the latency there is to hide.
constexpr int DEPTH = 8;
template <typename F>
__device__ __forceinline__ u32x4 fold_members(int64_t count, int64_t off, F member) {
    u32x4 acc = {0u, 0u, 0u, 0u};
    for (int64_t k = 0; k < count; k += DEPTH) {
        Member m[DEPTH];
        u32x4 q[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) m[u] = k + u < count ? member(k + u) : Member{nullptr, 0};
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) q[u] = load16(m[u], off);
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) acc ^= mask16(q[u], m[u].len, off);
    }
    return acc;
}

// bytes [off, off + 16) of the slot at dst, as far as they lie in front of `end` (a multiple of 4); off % 16 == 0
__device__ __forceinline__ void store16(uint8_t *dst, int64_t off, int64_t end, u32x4 v) {
    if (off + 16 <= end && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<u32x4 *>(dst + off) = v;
        return;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (off + 4 * i < end) *reinterpret_cast<uint32_t *>(dst + off + 4 * i) = w[i];
}

// grid (tiles of the longest possible stream, B 3 m): block (x, y) folds tile x of parity stream y = s m + g, the bands j = g, g + m, .. < n
__global__ __launch_bounds__(THREADS) void band_parity_kernel(l3c_banded_scale sc, int64_t n, int64_t m, uint8_t *__restrict__ parity,
                                                             int64_t parity_stride, uint32_t *__restrict__ parity_nbytes) {
    const int64_t y = blockIdx.y, s = y / m, g = y - s * m;
    const int64_t count = (n - g + m - 1) / m;
    uint32_t plen = 0;
    bool overrun = false;
    for (int64_t k = 0; k < count; ++k) {                          // uniform over the block: scalar loads, independent of each other
        const uint32_t len = band_nbytes(sc, n, s, g + k * m);
        overrun |= len == L3C_AC_OVERRUN;
        plen = len > plen ? len : plen;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) parity_nbytes[y] = overrun ? L3C_AC_OVERRUN : plen;
    if (overrun) return;
    const int64_t end4 = ((int64_t)plen + 3) & ~(int64_t)3;
    const int64_t off = (int64_t)blockIdx.x * TILE_BYTES + 16 * threadIdx.x;
    if (off >= end4) return;
    const u32x4 acc = fold_members(count, off, [&](int64_t k) {
        const int64_t j = g + k * m;
        return Member{band_row(sc, n, s, j), (int64_t)band_nbytes(sc, n, s, j)};
    });
    store16(parity + y * parity_stride, off, end4, acc);
}

// grid (tiles of the longest slot, n_groups): block (x, g) folds tile x of output slot g
__global__ __launch_bounds__(THREADS) void u8_xor_spans_kernel(const uint8_t *__restrict__ data, const l3c_u8_span *__restrict__ spans,
                                                              const int64_t *__restrict__ group_first,
                                                              const l3c_u8_span *__restrict__ out_spans, uint8_t *__restrict__ out) {
    const int64_t g = blockIdx.y;
    const l3c_u8_span slot = out_spans[g];
    const int64_t end = slot_bytes(slot.bytes);                    // the payload rounded up to 4, then 4 zero bytes
    const int64_t off = (int64_t)blockIdx.x * TILE_BYTES + 16 * threadIdx.x;
    if (off >= end) return;
    const int64_t k0 = group_first[g];
    const u32x4 acc = fold_members(group_first[g + 1] - k0, off, [&](int64_t k) {
        const l3c_u8_span src = spans[k0 + k];
        return Member{data + src.offset, src.bytes < slot.bytes ? src.bytes : slot.bytes};
    });
    store16(out + slot.offset, off, end, acc);
}

// ---- GF(2^8), polynomial 0x11D, alpha = 0x02, on four packed bytes per dword ------------------------------------------------------------------

// alpha times each byte of v: the byte shifted left, 0x1D added where its top bit was set
__device__ __forceinline__ uint32_t xtime(uint32_t v) { return ((v & 0x7f7f7f7fu) << 1) ^ (((v >> 7) & 0x01010101u) * 0x1du); }
__device__ __forceinline__ u32x4 xtime(u32x4 q) { return u32x4{xtime(q.x), xtime(q.y), xtime(q.z), xtime(q.w)}; }

// c times each byte of q, c uniform over the block: shift and add, one uniform branch per bit of c
__device__ __forceinline__ u32x4 gf_scale(u32x4 q, uint32_t c) {
    u32x4 r = {0u, 0u, 0u, 0u};
    while (c) {
        if (c & 1u) r ^= q;
        c >>= 1;
        if (c) q = xtime(q);
    }
    return r;
}

// band_parity_kernel for R rows per group: row r = XOR over members k of alpha^(k r) d_k, by Horner from the last member to the first,
// acc_r = alpha^r acc_r ^ d_k -- every member is loaded once for all rows.  Members eight at a time as in fold_members, the batches taken from
// the top; the batch that holds the last member is filled up with empty members ABOVE it, where every acc is still zero.
// grid (tiles, B 3 m); the slot of row r of stream y is parity + (y R + r) parity_stride
// (rs_stream: the block's work for output stream y of ONE record, shared with head_parity_kernel below)
template <int R>
__device__ __forceinline__ void rs_stream(const l3c_banded_scale &sc, int64_t n, int64_t m, int64_t y, uint8_t *__restrict__ parity,
                                          int64_t parity_stride, uint32_t *__restrict__ parity_nbytes) {
    const int64_t s = y / m, g = y - s * m;
    const int64_t count = (n - g + m - 1) / m;
    uint32_t plen = 0;
    bool overrun = false;
    for (int64_t k = 0; k < count; ++k) {
        const uint32_t len = band_nbytes(sc, n, s, g + k * m);
        overrun |= len == L3C_AC_OVERRUN;
        plen = len > plen ? len : plen;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) parity_nbytes[y] = overrun ? L3C_AC_OVERRUN : plen;
    if (overrun) return;
    const int64_t end4 = ((int64_t)plen + 3) & ~(int64_t)3;
    const int64_t off = (int64_t)blockIdx.x * TILE_BYTES + 16 * threadIdx.x;
    if (off >= end4) return;
    u32x4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = u32x4{0u, 0u, 0u, 0u};
    for (int64_t k0 = (count - 1) / DEPTH * DEPTH; k0 >= 0; k0 -= DEPTH) {
        Member mem[DEPTH];
        u32x4 q[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const int64_t j = g + (k0 + u) * m;
            mem[u] = k0 + u < count ? Member{band_row(sc, n, s, j), (int64_t)band_nbytes(sc, n, s, j)} : Member{nullptr, 0};
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) q[u] = load16(mem[u], off);
#pragma unroll
        for (int u = DEPTH - 1; u >= 0; --u) {
            const u32x4 d = mask16(q[u], mem[u].len, off);
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int i = 0; i < r; ++i) acc[r] = xtime(acc[r]);
                acc[r] ^= d;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) store16(parity + (y * R + r) * parity_stride, off, end4, acc[r]);
}

template <int R>
__global__ __launch_bounds__(THREADS) void band_parity_rs_kernel(l3c_banded_scale sc, int64_t n, int64_t m, uint8_t *__restrict__ parity,
                                                                int64_t parity_stride, uint32_t *__restrict__ parity_nbytes) {
    rs_stream<R>(sc, n, m, blockIdx.y, parity, parity_stride, parity_nbytes);
}

// l3c_head_parity: rs_stream over SEVERAL records of any C in one launch.  The records travel by value; block (x, y) finds its record by
// the first stream of each (uniform over the block: scalar compares), then is block (x, y - first) of that record's band_parity_rs launch
// with G_k = min(G, n_k), its slots at parity + offset[k] and its lengths at parity_nbytes + first[k].
struct HeadRecords {
    l3c_banded_scale sc[HEAD_MAX_RECORDS];
    int64_t offset[HEAD_MAX_RECORDS];      // of the record's slots inside `parity`, a multiple of 16
    int32_t first[HEAD_MAX_RECORDS + 1];   // streams (b, c, g) in front of the record; [count]: all
    int32_t n[HEAD_MAX_RECORDS], m[HEAD_MAX_RECORDS];
    int32_t count;
};
template <int R>
__global__ __launch_bounds__(THREADS) void head_parity_kernel(HeadRecords h, uint8_t *__restrict__ parity, int64_t parity_stride,
                                                             uint32_t *__restrict__ parity_nbytes) {
    const int y = (int)blockIdx.y;
    int k = 0;
    while (k + 1 < h.count && y >= h.first[k + 1]) ++k;
    rs_stream<R>(h.sc[k], h.n[k], h.m[k], y - h.first[k], parity + h.offset[k], parity_stride, parity_nbytes + h.first[k]);
}

// u8_xor_spans_kernel with a coefficient per span: slot g = XOR of coef[k] * span k.  A span with coef 0 becomes an empty member: not read.
__global__ __launch_bounds__(THREADS) void u8_gf_spans_kernel(const uint8_t *__restrict__ data, const l3c_u8_span *__restrict__ spans,
                                                             const uint8_t *__restrict__ coef, const int64_t *__restrict__ group_first,
                                                             const l3c_u8_span *__restrict__ out_spans, uint8_t *__restrict__ out) {
    const int64_t g = blockIdx.y;
    const l3c_u8_span slot = out_spans[g];
    const int64_t end = slot_bytes(slot.bytes);
    const int64_t off = (int64_t)blockIdx.x * TILE_BYTES + 16 * threadIdx.x;
    if (off >= end) return;
    const int64_t k0 = group_first[g], count = group_first[g + 1] - k0;
    u32x4 acc = {0u, 0u, 0u, 0u};
    for (int64_t k = 0; k < count; k += DEPTH) {
        Member mem[DEPTH];
        uint32_t c[DEPTH];
        u32x4 q[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            c[u] = k + u < count ? coef[k0 + k + u] : 0u;
            mem[u] = Member{nullptr, 0};
            if (c[u]) {
                const l3c_u8_span src = spans[k0 + k + u];
                mem[u] = Member{data + src.offset, src.bytes < slot.bytes ? src.bytes : slot.bytes};
            }
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) q[u] = load16(mem[u], off);
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) acc ^= gf_scale(mask16(q[u], mem[u].len, off), c[u]);
    }
    store16(out + slot.offset, off, end, acc);
}

// ---- l3c_band_rebuild: all t erased members of a group in one pass ------------------------------------------------------------------------

// A source of band_rebuild_kernel: `len` bytes that start `shift` bytes (0..3) behind the 4-byte aligned p.  A member has shift 0; a parity
// row lies where the file's section put it.
struct Source {
    const uint8_t *p;
    int64_t len;
    uint32_t shift;
};

// load16 for a source at any byte offset: bytes [off, off + 16) of it, zero at and behind the end of its last dword.  With a shift the five
// aligned dwords around the 16 bytes are read -- none that holds no byte of the source -- and funnel-shifted by whole bytes.
__device__ __forceinline__ u32x4 load16(const Source &s, int64_t off) {
    if (s.shift == 0) return load16(Member{s.p, s.len}, off);
    const int64_t end = (int64_t)s.shift + s.len;                  // of the source, in bytes from p
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = off + 4 * i < end ? *reinterpret_cast<const uint32_t *>(s.p + off + 4 * i) : 0u;
    u32x4 q;
    q.x = __builtin_amdgcn_alignbyte(w[1], w[0], s.shift);
    q.y = __builtin_amdgcn_alignbyte(w[2], w[1], s.shift);
    q.z = __builtin_amdgcn_alignbyte(w[3], w[2], s.shift);
    q.w = __builtin_amdgcn_alignbyte(w[4], w[3], s.shift);
    return q;
}

// acc[e] ^= (byte e of cw) * q for the four packed coefficients of cw, uniform over the block: the powers alpha^i q are formed once for
// all accumulators, one uniform branch per accumulator and bit.  A coefficient of 1 takes q as it is.
__device__ __forceinline__ void gf_scale4(u32x4 (&acc)[REBUILD_MAX], u32x4 q, uint32_t cw) {
    while (cw) {
        if (cw & 0x00000001u) acc[0] ^= q;
        if (cw & 0x00000100u) acc[1] ^= q;
        if (cw & 0x00010000u) acc[2] ^= q;
        if (cw & 0x01000000u) acc[3] ^= q;
        cw = (cw >> 1) & 0x7f7f7f7fu;
        if (cw) q = xtime(q);
    }
}

// grid (tiles of the longest slot, n_groups): block (x, g) rebuilds tile x of the t outputs of group g.  Every source is read once, cut to
// the longest output; an output shorter than that is cut when it is stored (the field operations work byte by byte, so the cut commutes).
__global__ __launch_bounds__(THREADS) void band_rebuild_kernel(const uint8_t *__restrict__ rows, uint8_t *members,
                                                              const l3c_u8_span *__restrict__ src, const uint32_t *__restrict__ coef,
                                                              const l3c_rebuild_group *__restrict__ groups) {
    const l3c_rebuild_group &grp = groups[blockIdx.y];
    const int t = grp.t;
    int64_t bytes[REBUILD_MAX], longest = 0;
#pragma unroll
    for (int e = 0; e < REBUILD_MAX; ++e) {
        bytes[e] = e < t ? grp.out[e].bytes : -1;
        longest = bytes[e] > longest ? bytes[e] : longest;
    }
    const int64_t off = (int64_t)blockIdx.x * TILE_BYTES + 16 * threadIdx.x;
    if (off >= slot_bytes(longest)) return;
    const uint32_t used = 0xFFFFFFFFu >> (8 * (REBUILD_MAX - t));   // the coefficients of the outputs there are
    const int64_t k0 = grp.first_src, n_rows = grp.n_rows, count = n_rows + grp.n_members;
    u32x4 acc[REBUILD_MAX];
#pragma unroll
    for (int e = 0; e < REBUILD_MAX; ++e) acc[e] = u32x4{0u, 0u, 0u, 0u};
    for (int64_t k = 0; k < count; k += DEPTH) {
        Source s[DEPTH];
        uint32_t c[DEPTH];
        u32x4 q[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            c[u] = k + u < count ? coef[k0 + k + u] & used : 0u;
            s[u] = Source{nullptr, 0, 0u};
            if (c[u]) {
                const l3c_u8_span sp = src[k0 + k + u];
                const int64_t len = sp.bytes < longest ? sp.bytes : longest;
                if (k + u < n_rows) {
                    const uint8_t *at = rows + sp.offset;
                    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(at) & 3);
                    s[u] = Source{at - shift, len, shift};
                } else {
                    s[u] = Source{members + sp.offset, len, 0u};
                }
            }
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) q[u] = load16(s[u], off);
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) gf_scale4(acc, mask16(q[u], s[u].len, off), c[u]);
    }
#pragma unroll
    for (int e = 0; e < REBUILD_MAX; ++e) {
        if (e >= t) break;
        const int64_t end = slot_bytes(bytes[e]);
        if (off < end) store16(members + grp.out[e].offset, off, end, mask16(acc[e], bytes[e], off));
    }
}

}  // namespace

extern "C" {

int l3c_band_rebuild(const uint8_t *rows, int64_t rows_bytes, uint8_t *members, int64_t members_bytes, const l3c_u8_span *src_host,
                     const l3c_u8_span *src, const uint8_t *coef_host, const uint8_t *coef, int64_t n_src, const l3c_rebuild_group *groups_host,
                     const l3c_rebuild_group *groups, int64_t n_groups, l3c_stream_t stream) {
    L3C_REQUIRE(n_groups >= 0, "n_groups must not be negative");
    if (n_groups == 0) return L3C_OK;
    // (room for the sweep over the member sources and the slots; where the counts are bad the check itself says which)
    const int64_t n_iv = rebuild_intervals(groups_host, n_groups);
    std::vector<RebuildInterval> scratch;
    try {
        scratch.resize(n_iv > 0 ? (size_t)n_iv : 0);
    } catch (const std::exception &) {
        return l3c::fail(L3C_ERR_INVALID_ARG, "%s: no host memory for the overlap check of %lld spans", "l3c_band_rebuild", (long long)n_iv);
    }
    const int64_t tiles = check_rebuild(src_host, n_src, groups_host, n_groups, rows_bytes, members_bytes, scratch.data(), l3c::error_buffer(), 512);
    if (tiles < 0) return (int)tiles;
    L3C_REQUIRE(rows && members && src && coef_host && coef && groups, "null pointer");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 3) == 0 && (reinterpret_cast<uintptr_t>(members) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(coef) & 3) == 0,
                "rows, members and coef must be 4-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(src) & 7) == 0 && (reinterpret_cast<uintptr_t>(groups) & 7) == 0,
                "src and groups (the device tables) must be 8-byte aligned");
    L3C_REQUIRE(members + members_bytes <= rows || rows + round4(rows_bytes) <= members, "members must not overlap rows");
    hipLaunchKernelGGL(band_rebuild_kernel, dim3((unsigned)tiles, (unsigned)n_groups), dim3(THREADS), 0, l3c::as_stream(stream), rows, members, src,
                       reinterpret_cast<const uint32_t *>(coef), groups);
    return l3c::check_launch("band_rebuild_kernel");
}

int l3c_band_parity_groups(int n, int G) {
    L3C_REQUIRE(n >= 1 && n <= 1024 && G >= 1 && G <= n, "n must be in 1..1024 and G in 1..n");
    return (n + G - 1) / G;
}

// the argument checks of l3c_band_parity and l3c_band_parity_rs, all before the launch -> L3C_OK with n, m and the longest coder stride
static int check_band_parity(const l3c_banded_scale *scale_host, int64_t B, int G, int R, const uint8_t *parity, int64_t parity_stride,
                             const uint32_t *parity_nbytes, int64_t *n_out, int64_t *m_out, int64_t *longest_out) {
    L3C_REQUIRE(scale_host && parity && parity_nbytes, "null pointer");
    const l3c_banded_scale sc = *scale_host;
    L3C_REQUIRE(sc.C == 3 && sc.H > 0 && sc.W > 0, "the parity covers the finest record: C must be 3, H and W positive");
    L3C_REQUIRE(sc.band_len > 0 && sc.band_len % 64 == 0, "band_len must be a positive multiple of 64");
    const int64_t hw = (int64_t)sc.H * sc.W, n = (hw + sc.band_len - 1) / sc.band_len;
    L3C_REQUIRE(n <= 1024, "more than 1024 bands per channel");
    L3C_REQUIRE(G >= 1 && G <= n, "G must be in 1..n");
    L3C_REQUIRE(R >= 1 && R <= 4, "R must be in 1..4");
    L3C_REQUIRE(R == 1 || G <= 255, "more than one parity stream needs groups of at most 255 bands");
    const int64_t m = (n + G - 1) / G;
    L3C_REQUIRE(B >= 1 && B <= MAX_STREAMS / (3 * m), "bad batch size: B * 3 * m must be in 1..65535");
    L3C_REQUIRE(sc.out_last && sc.nbytes_last && (n == 1 || (sc.out_full && sc.nbytes_full)), "null pointer in the scale");
    L3C_REQUIRE(sc.stride_last > 0 && sc.stride_last % 4 == 0 && (n == 1 || (sc.stride_full > 0 && sc.stride_full % 4 == 0)),
                "the coder strides must be positive multiples of 4");
    const int64_t longest = n > 1 && sc.stride_full > sc.stride_last ? sc.stride_full : sc.stride_last;
    L3C_REQUIRE(parity_stride % 16 == 0 && parity_stride >= longest, "parity_stride must be a multiple of 16 and at least the coder strides");
    L3C_REQUIRE(parity_stride <= INT64_MAX / (MAX_STREAMS * 4) && tiles_of(longest) <= 0x7fffffff, "stride out of range");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(sc.out_last) & 3) == 0 && (reinterpret_cast<uintptr_t>(sc.out_full) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(sc.nbytes_last) & 3) == 0 && (reinterpret_cast<uintptr_t>(sc.nbytes_full) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(parity_nbytes) & 3) == 0,
                "the coder outputs and the length arrays must be 4-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(parity) & 15) == 0, "parity must be 16-byte aligned");
    *n_out = n, *m_out = m, *longest_out = longest;
    return L3C_OK;
}

int l3c_band_parity(const l3c_banded_scale *scale_host, int64_t B, int G, uint8_t *parity, int64_t parity_stride, uint32_t *parity_nbytes,
                    l3c_stream_t stream) {
    int64_t n, m, longest;
    const int rc = check_band_parity(scale_host, B, G, 1, parity, parity_stride, parity_nbytes, &n, &m, &longest);
    if (rc != L3C_OK) return rc;
    hipLaunchKernelGGL(band_parity_kernel, dim3((unsigned)tiles_of(longest), (unsigned)(B * 3 * m)), dim3(THREADS), 0, l3c::as_stream(stream),
                       *scale_host, n, m, parity, parity_stride, parity_nbytes);
    return l3c::check_launch("band_parity_kernel");
}

int l3c_band_parity_rs(const l3c_banded_scale *scale_host, int64_t B, int G, int R, uint8_t *parity, int64_t parity_stride, uint32_t *parity_nbytes,
                       l3c_stream_t stream) {
    int64_t n, m, longest;
    const int rc = check_band_parity(scale_host, B, G, R, parity, parity_stride, parity_nbytes, &n, &m, &longest);
    if (rc != L3C_OK) return rc;
    const dim3 grid((unsigned)tiles_of(longest), (unsigned)(B * 3 * m));
    const hipStream_t st = l3c::as_stream(stream);
    switch (R) {
    case 1: hipLaunchKernelGGL(band_parity_rs_kernel<1>, grid, dim3(THREADS), 0, st, *scale_host, n, m, parity, parity_stride, parity_nbytes); break;
    case 2: hipLaunchKernelGGL(band_parity_rs_kernel<2>, grid, dim3(THREADS), 0, st, *scale_host, n, m, parity, parity_stride, parity_nbytes); break;
    case 3: hipLaunchKernelGGL(band_parity_rs_kernel<3>, grid, dim3(THREADS), 0, st, *scale_host, n, m, parity, parity_stride, parity_nbytes); break;
    default: hipLaunchKernelGGL(band_parity_rs_kernel<4>, grid, dim3(THREADS), 0, st, *scale_host, n, m, parity, parity_stride, parity_nbytes); break;
    }
    return l3c::check_launch("band_parity_rs_kernel");
}

// l3c_u8_xor_spans (gf false: no coefficients, the XOR kernel) and l3c_u8_gf_spans: the argument checks, all before the launch, and the launch
static int u8_spans(bool gf, const uint8_t *data, int64_t data_bytes, const l3c_u8_span *spans_host, const l3c_u8_span *spans, const uint8_t *coef_host,
                    const uint8_t *coef, int64_t n_spans, const int64_t *group_first_host, const int64_t *group_first, int64_t n_groups,
                    const l3c_u8_span *out_spans_host, const l3c_u8_span *out_spans, uint8_t *out, int64_t out_bytes, l3c_stream_t stream) {
    L3C_REQUIRE(n_groups >= 0, "n_groups must not be negative");
    if (n_groups == 0) return L3C_OK;
    const int64_t tiles = check_xor_spans(spans_host, n_spans, group_first_host, n_groups, out_spans_host, data_bytes, out_bytes, l3c::error_buffer(), 512);
    if (tiles < 0) return (int)tiles;
    L3C_REQUIRE(out && group_first && out_spans && (n_spans == 0 || (data && spans && (!gf || (coef_host && coef)))), "null pointer");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(data) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "data and out must be 4-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(spans) & 7) == 0 && (reinterpret_cast<uintptr_t>(group_first) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(out_spans) & 7) == 0,
                "spans, group_first and out_spans (the device tables) must be 8-byte aligned");
    L3C_REQUIRE(n_spans == 0 || out + out_bytes <= data || data + data_bytes <= out, "out must not overlap data");
    const dim3 grid((unsigned)tiles, (unsigned)n_groups);
    if (gf)
        hipLaunchKernelGGL(u8_gf_spans_kernel, grid, dim3(THREADS), 0, l3c::as_stream(stream), data, spans, coef, group_first, out_spans, out);
    else
        hipLaunchKernelGGL(u8_xor_spans_kernel, grid, dim3(THREADS), 0, l3c::as_stream(stream), data, spans, group_first, out_spans, out);
    return l3c::check_launch(gf ? "u8_gf_spans_kernel" : "u8_xor_spans_kernel");
}

int l3c_u8_xor_spans(const uint8_t *data, int64_t data_bytes, const l3c_u8_span *spans_host, const l3c_u8_span *spans, int64_t n_spans,
                     const int64_t *group_first_host, const int64_t *group_first, int64_t n_groups, const l3c_u8_span *out_spans_host,
                     const l3c_u8_span *out_spans, uint8_t *out, int64_t out_bytes, l3c_stream_t stream) {
    return u8_spans(false, data, data_bytes, spans_host, spans, nullptr, nullptr, n_spans, group_first_host, group_first, n_groups, out_spans_host,
                    out_spans, out, out_bytes, stream);
}

int l3c_u8_gf_spans(const uint8_t *data, int64_t data_bytes, const l3c_u8_span *spans_host, const l3c_u8_span *spans, const uint8_t *coef_host,
                    const uint8_t *coef, int64_t n_spans, const int64_t *group_first_host, const int64_t *group_first, int64_t n_groups,
                    const l3c_u8_span *out_spans_host, const l3c_u8_span *out_spans, uint8_t *out, int64_t out_bytes, l3c_stream_t stream) {
    return u8_spans(true, data, data_bytes, spans_host, spans, coef_host, coef, n_spans, group_first_host, group_first, n_groups, out_spans_host,
                    out_spans, out, out_bytes, stream);
}

int l3c_head_parity(const l3c_banded_scale *scales_host, int n_scales, int64_t B, int G, int R, uint8_t *parity, const int64_t *parity_offset_host,
                    int64_t parity_stride, uint32_t *parity_nbytes, l3c_stream_t stream) {
    L3C_REQUIRE(scales_host && parity && parity_offset_host && parity_nbytes, "null pointer");
    L3C_REQUIRE(n_scales >= 1 && n_scales <= HEAD_MAX_RECORDS, "n_scales must be in 1..8");
    L3C_REQUIRE(G >= 1, "G must be at least 1");
    L3C_REQUIRE(R >= 1 && R <= 4, "R must be in 1..4");
    L3C_REQUIRE(B >= 1 && B <= MAX_STREAMS, "bad batch size");
    L3C_REQUIRE(parity_stride > 0 && parity_stride % 16 == 0, "parity_stride must be a positive multiple of 16");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(parity) & 15) == 0 && (reinterpret_cast<uintptr_t>(parity_nbytes) & 3) == 0,
                "parity must be 16-byte aligned, parity_nbytes 4-byte aligned");
    HeadRecords h{};
    h.count = n_scales;
    int64_t streams = 0, longest = 0;
    for (int k = 0; k < n_scales; ++k) {
        const l3c_banded_scale &sc = scales_host[k];
        L3C_REQUIRE(sc.C >= 1 && sc.C <= 1024 && sc.H > 0 && sc.W > 0, "C must be in 1..1024, H and W positive");
        L3C_REQUIRE(sc.band_len > 0 && sc.band_len % 64 == 0, "band_len must be a positive multiple of 64");
        const int64_t hw = (int64_t)sc.H * sc.W, n = (hw + sc.band_len - 1) / sc.band_len;
        L3C_REQUIRE(n <= 1024, "more than 1024 bands per channel");
        const int64_t Gk = G < n ? G : n, m = (n + Gk - 1) / Gk;
        L3C_REQUIRE(R == 1 || Gk <= 255, "more than one parity stream needs groups of at most 255 bands");
        L3C_REQUIRE(sc.out_last && sc.nbytes_last && (n == 1 || (sc.out_full && sc.nbytes_full)), "null pointer in a scale");
        L3C_REQUIRE(sc.stride_last > 0 && sc.stride_last % 4 == 0 && (n == 1 || (sc.stride_full > 0 && sc.stride_full % 4 == 0)),
                    "the coder strides must be positive multiples of 4");
        L3C_REQUIRE((reinterpret_cast<uintptr_t>(sc.out_last) & 3) == 0 && (reinterpret_cast<uintptr_t>(sc.out_full) & 3) == 0 &&
                        (reinterpret_cast<uintptr_t>(sc.nbytes_last) & 3) == 0 && (reinterpret_cast<uintptr_t>(sc.nbytes_full) & 3) == 0,
                    "the coder outputs and the length arrays must be 4-byte aligned");
        const int64_t stride = n > 1 && sc.stride_full > sc.stride_last ? sc.stride_full : sc.stride_last;
        L3C_REQUIRE(parity_stride >= stride, "parity_stride must be at least the coder strides");
        L3C_REQUIRE(parity_offset_host[k] >= 0 && parity_offset_host[k] % 16 == 0, "the parity offsets must be non-negative multiples of 16");
        streams += B * sc.C * m;
        L3C_REQUIRE(streams <= MAX_STREAMS, "bad sizes: the sum of B * C * m over the records must be in 1..65535");
        longest = stride > longest ? stride : longest;
        h.sc[k] = sc, h.offset[k] = parity_offset_host[k], h.n[k] = (int32_t)n, h.m[k] = (int32_t)m, h.first[k + 1] = (int32_t)streams;
    }
    L3C_REQUIRE(parity_stride <= INT64_MAX / (MAX_STREAMS * 4) && tiles_of(longest) <= 0x7fffffff, "stride out of range");
    const dim3 grid((unsigned)tiles_of(longest), (unsigned)streams);
    const hipStream_t st = l3c::as_stream(stream);
    switch (R) {
    case 1: hipLaunchKernelGGL(head_parity_kernel<1>, grid, dim3(THREADS), 0, st, h, parity, parity_stride, parity_nbytes); break;
    case 2: hipLaunchKernelGGL(head_parity_kernel<2>, grid, dim3(THREADS), 0, st, h, parity, parity_stride, parity_nbytes); break;
    case 3: hipLaunchKernelGGL(head_parity_kernel<3>, grid, dim3(THREADS), 0, st, h, parity, parity_stride, parity_nbytes); break;
    default: hipLaunchKernelGGL(head_parity_kernel<4>, grid, dim3(THREADS), 0, st, h, parity, parity_stride, parity_nbytes); break;
    }
    return l3c::check_launch("head_parity_kernel");
}
}
