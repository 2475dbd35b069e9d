// seal_parity.hip -- l3c_seal_append_parity (include/l3c_hip.h): the tail of a parity-sealed file -- section 'L3CP' / 'L3CQ' / 'L3CH', band
// table, version-3 seal; the format is csrc/seal.h -- assembled behind every file of a banded encode on the device, where alone the
// lengths are known.  The bytes are container.make_seal's; the geometry, the meta layout and the workspace are seal_parity_plan.h's.
//
// Two launches, no atomics, no allocation, no host synchronisation, integer only, the same bytes whatever the launch geometry.
//
// seal_parity_plan_kernel, a block per file.  Its 256 threads scan the file's copy units (a unit: the R rows of one parity group, or the
// head part's meta bytes) into their places in the tail, decide whether the file takes its tail at all (a file of -1, a group marked
// L3C_AC_OVERRUN or longer than its slot, a body that is not what the records add up to, a slot without room: -1, and nothing is written),
// and write everything of the tail that is not a row: the section's front and its last 8 bytes, the band table, the seal and its check
// word (one wavefront shares the words as seal_append_bands_kernel does), and with a head part the meta bytes, staged in the workspace --
// the framing copy is rebuilt from the records and the padding, which is what l3c_container_write_banded wrote into the body; the body's
// size is checked against them -- with head_crc over the body in front of the finest record (a wavefront per quarter of it, the four words
// combined as zlib's crc32_combine does) and head_check over the staged meta bytes (one wavefront); crc_wave.h: the code of
// l3c_band_payload_crc32.
//
// seal_parity_copy_kernel, grid (tiles x R, units, B): block (x, u, b) copies tile x % tiles of row x / tiles of unit u from its 16-byte
// aligned slot to its place in file b, which has ANY byte alignment.  A thread owns destination-aligned dwords: a dword that lies inside
// the row is one dword store of two source dwords shifted together, the up to three bytes at either edge are byte stores.  Nothing outside
// [old end, new end) of a slot is stored by either kernel.
#include "l3c_common.h"
#include "crc_spans.h"
#include "crc_wave.h"
#include "seal.h"
#include "seal_parity_plan.h"
#include "banded_rows.h"

namespace {

using namespace l3c_parity_seal;
using l3c_crc::mulmod, l3c_crc::POLY, l3c_crc::powmod;
using l3c_crc_wave::stage_wave_tables, l3c_crc_wave::wave_crc32, l3c_crc_wave::WAVE_TABLE_WORDS;

struct Args {
    Plan p;
    l3c_banded_scale sc[MAX_RECORDS];      // the plan's records (read with a head part only)
    int64_t hp_offset[MAX_RECORDS];        // head record k: its slots inside head_parity
    uint8_t *files;
    int64_t file_stride;
    int64_t *file_bytes;
    const uint32_t *frame_crc, *band_crc;
    const uint16_t *padding;
    uint64_t model_id;
    uint32_t generation, z_check;
    const uint8_t *parity;
    int64_t parity_stride;
    const uint32_t *parity_nbytes;
    const uint8_t *head_parity;
    int64_t head_stride;
    const uint32_t *head_nbytes, *payload_crc;
    char *ws;
};

struct Unit {
    const uint8_t *src;        // row 0; row r lies r * stride further
    int64_t len, stride;       // bytes of a row, bytes of a slot
    int rows;                  // R, or 1 for the meta bytes
    int k, idx;                // a head group: its record and (c, g) index; else k = -1
};

__device__ __forceinline__ uint8_t *meta_of(const Args &a, int64_t b) { return reinterpret_cast<uint8_t *>(a.ws + a.p.ws_meta) + b * a.p.meta_stride; }

// unit u of file b: where its rows lie and how long they are (as the parity kernels stated it: not yet checked against the slot)
__device__ __forceinline__ Unit unit_of(const Args &a, int64_t b, int u) {
    const Plan &p = a.p;
    const int fin = p.n_records - 1, m3 = 3 * p.rec[fin].m;
    if (u < m3) {
        const int64_t i = b * m3 + u;
        return Unit{a.parity + i * p.R * a.parity_stride, (int64_t)a.parity_nbytes[i], a.parity_stride, p.R, -1, 0};
    }
    if (u == m3) return Unit{meta_of(a, b), p.meta_bytes, p.meta_stride, 1, -1, 0};
    const int hu = u - m3 - 1;
    int k = 0;
    while (k + 1 < fin && hu >= p.unit_first[k + 1]) ++k;
    const int idx = hu - p.unit_first[k];
    const int64_t i = b * (p.rec[k].C * p.rec[k].m) + idx;
    return Unit{a.head_parity + a.hp_offset[k] + i * p.R * a.head_stride, (int64_t)a.head_nbytes[p.len_first[k] + i], a.head_stride, p.R, k, idx};
}

__device__ __forceinline__ void put32(uint8_t *dst, uint32_t v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = (uint8_t)(v >> (8 * k));
}

// the sum of v over the block's 256 threads, in every thread; red: 4 words of LDS, free again on return
__device__ __forceinline__ int64_t block_sum(int64_t v, int64_t *red, int t) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(THREADS) void seal_parity_plan_kernel(const Args a) {
    __shared__ uint32_t lds[WAVE_TABLE_WORDS];
    __shared__ int64_t part[THREADS];
    __shared__ int64_t red[4];
    __shared__ uint32_t part_crc[THREADS / 64];
    const Plan &p = a.p;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t b = blockIdx.x;
    const int fin = p.n_records - 1, m3 = 3 * p.rec[fin].m;
    int64_t *tail_at = reinterpret_cast<int64_t *>(a.ws + p.ws_tail_at);
    int64_t *unit_off = reinterpret_cast<int64_t *>(a.ws + p.ws_unit_off) + b * p.units;
    uint8_t *meta = meta_of(a, b);
    const int64_t at = a.file_bytes[b];
    if (at < 0) {                                                            // (uniform over the block) stays -1
        if (t == 0) tail_at[b] = -1;
        return;
    }
    int bad = 0;
    int64_t coarse = 0, finest = 0;
    if (p.head) {
        stage_wave_tables(lds, t);
        // every length field of the file: the framing copy, the body's size, and beside a head record's lengths its payload CRC words
        for (int i = t; i < p.fields; i += THREADS) {
            int k = 0;
            while (k < fin && i >= p.field_first[k + 1]) ++k;
            const Record &r = p.rec[k];
            const int f = i - p.field_first[k], c = f / r.n, j = f - c * r.n;
            const uint32_t len = band_nbytes(a.sc[k], r.n, b * r.C + c, j);
            bad |= (int64_t)len > (j + 1 < r.n ? a.sc[k].stride_full : a.sc[k].stride_last);       // (L3C_AC_OVERRUN among them)
            if (k == fin) finest += len;
            else coarse += len;
            put32(meta + p.meta_hdr_at[k] + 9 + 4 * f, len);
            if (k < fin) put32(meta + p.meta_crc_at[k] + 4 * f, a.payload_crc[p.crc_first[k] + b * (r.C * r.n) + f]);
        }
    }
    // the units' places: a thread sums its contiguous share, the block scans the 256 sums
    const int per = (p.units + THREADS - 1) / THREADS;
    const int lo = t * per < p.units ? t * per : p.units, hi = lo + per < p.units ? lo + per : p.units;
    int64_t mine = 0;
    for (int u = lo; u < hi; ++u) {
        const Unit q = unit_of(a, b, u);
        bad |= q.len > q.stride;                                             // L3C_AC_OVERRUN, or a length no slot holds
        mine += q.rows * q.len;
    }
    part[t] = mine;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const int64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const int64_t rows_bytes = part[THREADS - 1];                            // every unit of the file
    bad = __syncthreads_or(bad);
    int64_t P0 = 0, quarter = 0;
    if (p.head) {
        coarse = block_sum(coarse, red, t);
        finest = block_sum(finest, red, t);
        P0 = p.head_framing + coarse;
        quarter = (P0 + 255) / 256 * 64;
        bad |= P0 + p.finest_framing + finest != at;                         // the body is not what the records add up to
    }
    const int64_t S = p.front_bytes + rows_bytes + (p.head ? 4 : 0) + 8, tail = S + p.table_bytes + L3C_SEAL_BYTES;
    if (bad || S > 0xFFFFFFFFll || at > a.file_stride - tail) {
        if (t == 0) tail_at[b] = -1, a.file_bytes[b] = -1;
        return;
    }
    int64_t off = p.front_bytes + part[t] - mine;
    for (int u = lo; u < hi; ++u) {
        const Unit q = unit_of(a, b, u);
        unit_off[u] = off;
        off += q.rows * q.len;
        if (q.k >= 0) put32(meta + p.meta_crc_at[q.k] + 4 * p.rec[q.k].C * p.rec[q.k].n + 4 + 4 * q.idx, (uint32_t)q.len);
    }
    uint8_t *file = a.files + b * a.file_stride, *dst = file + at;
    const uint32_t pad0 = a.padding ? (uint32_t)a.padding[4 * b] | (uint32_t)a.padding[4 * b + 1] << 16 : 0u;
    const uint32_t pad1 = a.padding ? (uint32_t)a.padding[4 * b + 2] | (uint32_t)a.padding[4 * b + 3] << 16 : 0u;
    if (p.head && t == 0) {                                                  // the fixed fields of the meta bytes
        put32(meta, (uint32_t)p.n_records);
        put32(meta + 4, 0x4243334Cu);                                        // 'L3CB', version 1, 0: body[0:14]
        meta[8] = 1, meta[9] = 0;
        put32(meta + 10, pad0);
        put32(meta + 14, pad1);
        for (int k = 0; k <= fin; ++k) {
            const Record &r = p.rec[k];
            uint8_t *h = meta + p.meta_hdr_at[k];
            h[0] = (uint8_t)r.C, h[1] = (uint8_t)r.H, h[2] = (uint8_t)(r.H >> 8), h[3] = (uint8_t)r.W, h[4] = (uint8_t)(r.W >> 8);
            put32(h + 5, (uint32_t)r.L);
            if (k < fin) put32(meta + p.meta_crc_at[k] + 4 * r.C * r.n, (uint32_t)r.G | (uint32_t)r.m << 16);
        }
    }
    __syncthreads();                                                         // the tables and the meta bytes but head_crc
    if (p.head) {                                                            // head_crc: a wavefront per quarter of body[0, P0), rounded up to 64 bytes
        const int64_t lo = wave * quarter < P0 ? wave * quarter : P0, hi = lo + quarter < P0 ? lo + quarter : P0;
        const uint32_t crc = wave_crc32(lds, lane, file + lo, hi - lo);
        if (lane == 0) part_crc[wave] = crc;
    }
    __syncthreads();
    if (p.head && wave == 0) {
        uint32_t head_crc = part_crc[0];                                     // crc(A | B) = crc(A) x^(8 |B|) + crc(B): zlib's crc32_combine
        for (int w = 1; w < THREADS / 64; ++w) {
            const int64_t lo = w * quarter < P0 ? w * quarter : P0, hi = lo + quarter < P0 ? lo + quarter : P0;
            head_crc = mulmod(head_crc, powmod(l3c_crc::X8, (uint64_t)(hi - lo))) ^ part_crc[w];
        }
        if (lane == 0) put32(meta + p.meta_head_crc_at, head_crc);
        __threadfence_block();
        const uint32_t head_check = wave_crc32(lds, lane, meta, p.meta_bytes);
        if (lane == 0) put32(dst + p.front_bytes + rows_bytes, head_check);
    }
    if (wave == (p.head ? 1 : 0)) {
        // the check word over M little-endian words: padding (2), the section's front, its last 8 bytes, the table, seal words 0..4.  Lane l
        // folds its contiguous share bit by bit, weighs it with x^(32 * words behind the share), the wave XORs, Z(4 M) comes from the host
        const int fw = p.front_bytes / 4, hw = p.plen_at / 4, n3 = 3 * p.rec[fin].n, M = p.check_words;
        const int share = (M + 63) / 64;
        const int w0 = lane * share < M ? lane * share : M, w1 = w0 + share < M ? w0 + share : M;
        uint32_t acc = 0;
        for (int i = w0; i < w1; ++i) {
            uint32_t w;
            uint8_t *to = nullptr;
            if (i < 2) {
                w = i == 0 ? pad0 : pad1;
            } else if (i < 2 + fw) {
                const int q = i - 2;
                to = dst + 4 * q;
                if (q == 0) w = p.signature;
                else if (q == 1) w = (uint32_t)p.rec[fin].G | (uint32_t)p.rec[fin].m << 16;
                else if (q < hw) w = (uint32_t)p.R;                           // R, reserved = 0
                else w = a.parity_nbytes[b * m3 + (q - hw)];
            } else {
                const int q = i - 2 - fw;                                     // from the section's last 8 bytes on
                to = dst + S - 8 + 4 * q;
                if (q == 0) w = (uint32_t)S;
                else if (q == 1) w = 0x9284E246u;                             // the separator 46 E2 84 92
                else if (q == 2) w = 0x5443334Cu;                             // 'L3CT'
                else if (q == 3) w = (uint32_t)p.rec[fin].n;                  // n, reserved = 0
                else if (q == 4) w = (uint32_t)p.rec[fin].L;
                else if (q < 5 + n3) w = a.band_crc[b * n3 + (q - 5)];
                else if (q == 5 + n3) w = (uint32_t)p.table_bytes;
                else if (q == 6 + n3) w = 0x9284E246u;
                else if (q == 7 + n3) w = 0x5343334Cu;                        // 'L3CS'
                else if (q == 8 + n3) w = (uint32_t)l3c_sealing::VERSION_PARITY | a.generation << 16;
                else if (q == 9 + n3) w = a.frame_crc[b];
                else if (q == 10 + n3) w = (uint32_t)a.model_id;
                else w = (uint32_t)(a.model_id >> 32);
            }
            if (to) put32(to, w);
            acc ^= w;
            for (int k = 0; k < 32; ++k) acc = (acc >> 1) ^ (POLY & (0u - (acc & 1u)));
        }
        acc = mulmod(acc, powmod(POLY, (uint64_t)(M - w1)));                  // POLY is x^32
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d, 64);
        if (lane == 0) put32(dst + tail - 4, acc ^ a.z_check);
    }
    if (t == 0) tail_at[b] = at, a.file_bytes[b] = at + tail;
}

// row bytes [0, len) from src (16-byte aligned; readable up to its 4-byte-rounded end) to dst (any alignment), the destination dwords
// [tile * TILE_DWORDS, ...) of it: dword w of the destination, counted from dst rounded DOWN to 4, holds row bytes [4 w - sh, 4 w - sh + 4)
__device__ __forceinline__ void copy_tile(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t len, int64_t tile, int t) {
    const int sh = (int)(reinterpret_cast<uintptr_t>(dst) & 3), rb = (4 - sh) & 3;
    uint8_t *base = dst - sh;                                                 // 4-byte aligned; only bytes of [dst, dst + len) are stored
    const int64_t dwords = (sh + len + 3) / 4;
#pragma unroll
    for (int i = 0; i < TILE_DWORDS / THREADS; ++i) {
        const int64_t w = tile * TILE_DWORDS + i * THREADS + t;
        if (w >= dwords) break;
        const int64_t i0 = 4 * w - sh;                                        // the row byte at the dword's first byte
        if (i0 >= 0 && i0 + 4 <= len) {
            const int64_t s0 = i0 - rb;                                       // i0 rounded down to 4
            uint32_t v = *reinterpret_cast<const uint32_t *>(src + s0);
            if (rb) v = __builtin_amdgcn_alignbyte(*reinterpret_cast<const uint32_t *>(src + s0 + 4), v, rb);
            *reinterpret_cast<uint32_t *>(base + 4 * w) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k >= 0 && i0 + k < len) base[4 * w + k] = src[i0 + k];
        }
    }
}

__global__ __launch_bounds__(THREADS) void seal_parity_copy_kernel(const Args a, int tiles) {
    const int64_t b = blockIdx.z;
    const int u = (int)blockIdx.y, r = (int)(blockIdx.x / tiles);
    const int64_t tile = blockIdx.x % tiles;
    const int64_t at = reinterpret_cast<const int64_t *>(a.ws + a.p.ws_tail_at)[b];
    if (at < 0) return;                                                       // a refused file: nothing is stored
    const Unit q = unit_of(a, b, u);
    if (r >= q.rows || tile * TILE_DWORDS * 4 >= q.len + 7) return;          // (uniform) no such row, or the row ends in front of the tile
    const int64_t off = (reinterpret_cast<const int64_t *>(a.ws + a.p.ws_unit_off) + b * a.p.units)[u];
    copy_tile(q.src + r * q.stride, a.files + b * a.file_stride + at + off + r * q.len, q.len, tile, threadIdx.x);
}

bool aligned(const void *ptr, uintptr_t to) { return (reinterpret_cast<uintptr_t>(ptr) & (to - 1)) == 0; }

// the records of a descriptor -> the plan's inputs; the checks of the records that do not depend on a device
int shapes_of(const l3c_banded_scale *scales, int n_scales, Shape *shapes) {
    L3C_REQUIRE(scales, "null pointer: scales_host");
    if (n_scales > MAX_RECORDS)
        return l3c::fail(L3C_ERR_UNSUPPORTED, "%s", "unsupported: a parity seal takes files of at most 8 scale records");
    L3C_REQUIRE(n_scales >= 1, "n_scales must be at least 1");
    for (int k = 0; k < n_scales; ++k) shapes[k] = Shape{scales[k].C, scales[k].H, scales[k].W, scales[k].band_len};
    return L3C_OK;
}

}  // namespace

extern "C" {

int64_t l3c_seal_append_parity_workspace_bytes(const l3c_banded_scale *scales_host, int n_scales, int64_t B, int G, int R, int head) {
    Shape shapes[MAX_RECORDS];
    const int64_t none[MAX_RECORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc = check_opts(G, R, head, 0, l3c::error_buffer(), 512);
    if (rc == L3C_OK) rc = shapes_of(scales_host, n_scales, shapes);
    Plan p;
    if (rc == L3C_OK) rc = make_plan(shapes, n_scales, B, G, R, head, none, &p, l3c::error_buffer(), 512);
    return rc != L3C_OK ? rc : p.ws_bytes;
}

int l3c_seal_append_parity(const l3c_seal_parity_desc *d, l3c_stream_t stream) {
    L3C_REQUIRE(d, "null descriptor");
    int rc = check_opts(d->G, d->R, d->head, d->reserved, l3c::error_buffer(), 512);
    if (rc != L3C_OK) return rc;
    Shape shapes[MAX_RECORDS];
    rc = shapes_of(d->scales_host, d->n_scales, shapes);
    if (rc != L3C_OK) return rc;
    L3C_REQUIRE(d->parity_stride > 0 && d->parity_stride % 16 == 0, "parity_stride must be a positive multiple of 16");
    L3C_REQUIRE(!d->head || (d->head_parity_stride > 0 && d->head_parity_stride % 16 == 0), "head_parity_stride must be a positive multiple of 16");
    int64_t strides[MAX_RECORDS];
    for (int k = 0; k < d->n_scales; ++k) strides[k] = k + 1 < d->n_scales ? d->head_parity_stride : d->parity_stride;
    Args a{};
    rc = make_plan(shapes, d->n_scales, d->B, d->G, d->R, d->head, strides, &a.p, l3c::error_buffer(), 512);
    if (rc != L3C_OK) return rc;
    const Plan &p = a.p;
    L3C_REQUIRE(d->files && d->file_bytes && d->frame_crc && d->band_crc && d->parity && d->parity_nbytes && d->workspace, "null pointer");
    L3C_REQUIRE(!d->head || (d->head_parity && d->head_parity_offset_host && d->head_parity_nbytes && d->payload_crc), "null pointer (head part)");
    L3C_REQUIRE(d->file_stride > 0 && d->file_stride <= INT64_MAX / d->B, "bad file_stride");
    L3C_REQUIRE(aligned(d->file_bytes, 8) && aligned(d->frame_crc, 4) && aligned(d->band_crc, 4) && aligned(d->parity_nbytes, 4) &&
                    aligned(d->head_parity_nbytes, 4) && aligned(d->payload_crc, 4) && aligned(d->padding, 2),
                "file_bytes, the CRC words, the length arrays and padding must be aligned to their element size");
    L3C_REQUIRE(aligned(d->parity, 16) && aligned(d->head_parity, 16) && aligned(d->workspace, 16), "parity, head_parity and workspace must be 16-byte aligned");
    L3C_REQUIRE(!d->head || (aligned(d->files, 4) && d->file_stride % 4 == 0), "with a head part files and file_stride must be multiples of 4");
    L3C_REQUIRE(d->workspace_bytes >= p.ws_bytes, "workspace too small (l3c_seal_append_parity_workspace_bytes)");
    L3C_REQUIRE(d->parity_stride <= INT64_MAX / (MAX_STREAMS * 4) && d->head_parity_stride <= INT64_MAX / (MAX_STREAMS * 4), "stride out of range");
    const int64_t tiles = copy_tiles(p.longest);
    L3C_REQUIRE(tiles * p.R <= 0x7fffffff, "stride out of range");
    if (d->head) {
        const int shift = d->n_scales - p.n_records;       // 0
        for (int k = 0; k < p.n_records; ++k) {
            const l3c_banded_scale &sc = d->scales_host[shift + k];
            const int n = p.rec[k].n;
            L3C_REQUIRE(sc.nbytes_last && (n == 1 || sc.nbytes_full), "null pointer in a scale");
            L3C_REQUIRE(aligned(sc.nbytes_last, 4) && aligned(sc.nbytes_full, 4), "the length arrays must be 4-byte aligned");
            L3C_REQUIRE(sc.stride_last > 0 && (n == 1 || sc.stride_full > 0), "the coder strides must be positive");
            a.sc[k] = sc;
            if (k + 1 < p.n_records) {
                L3C_REQUIRE(d->head_parity_offset_host[k] >= 0 && d->head_parity_offset_host[k] % 16 == 0,
                            "the parity offsets must be non-negative multiples of 16");
                a.hp_offset[k] = d->head_parity_offset_host[k];
            }
        }
    }
    a.files = d->files, a.file_stride = d->file_stride, a.file_bytes = d->file_bytes;
    a.frame_crc = d->frame_crc, a.band_crc = d->band_crc, a.padding = d->padding, a.model_id = d->model_id;
    a.generation = (uint32_t)L3C_BITSTREAM_GENERATION, a.z_check = l3c_crc::span_z(4 * (int64_t)p.check_words);
    a.parity = d->parity, a.parity_stride = d->parity_stride, a.parity_nbytes = d->parity_nbytes;
    a.head_parity = d->head_parity, a.head_stride = d->head_parity_stride, a.head_nbytes = d->head_parity_nbytes, a.payload_crc = d->payload_crc;
    a.ws = static_cast<char *>(d->workspace);
    const hipStream_t st = l3c::as_stream(stream);
    hipLaunchKernelGGL(seal_parity_plan_kernel, dim3((unsigned)d->B), dim3(THREADS), 0, st, a);
    rc = l3c::check_launch("seal_parity_plan_kernel");
    if (rc != L3C_OK) return rc;
    hipLaunchKernelGGL(seal_parity_copy_kernel, dim3((unsigned)(tiles * p.R), (unsigned)p.units, (unsigned)d->B), dim3(THREADS), 0, st, a, (int)tiles);
    return l3c::check_launch("seal_parity_copy_kernel");
}
}
