// container.hip -- `.l3c` file assembly on the GPU (replaces the host-side byte shuffling of bitcoding.py:326-375 for batches).
//
// The range coder leaves every stream's bytes in its own row of a per-scale buffer.  A file is
//     u16 x4 padding | for scale = coarsest .. 0:  u8 C, u16 H, u16 W | per channel: u32 nbytes, payload | magic 46 E2 84 92
// (all little-endian).  Given the per-image file offsets (an exclusive scan of the file sizes, done by the caller), ONE launch
// writes all files of a batch back to back into one buffer: block (stream j, image b) finds its place from the byte counts of
// the streams before it, writes its length field (+ the scale header / magic / padding header it is next to) and copies its
// payload -- dword-wise, re-aligned with v_alignbyte_b32, since file offsets are byte-granular.  One D2H copy of exactly the
// files' bytes then replaces the per-scale padded copies and the host-side joins.
//
// BANDED files (round 7, include/l3c_hip.h): every channel's stream cut into bands of L symbols.  l3c_ac_band_intervals re-lays a scale's
// coding intervals into the coder groups of its full and its last bands; l3c_container_write_banded assembles the files, with a scan of
// the length fields first (a file holds up to 1024 bands per channel: a block per stream can no longer walk the streams in front of it).
#include "l3c_common.h"

namespace {

struct ScaleDesc {
    const uint8_t *out;        // [B * C][stride] coder output rows (4-byte aligned rows)
    const uint32_t *nbytes;    // [B * C]
    int64_t stride;
    int C, H, W;
};

struct ContainerArgs {
    static constexpr int MAX_SCALES = 8;
    ScaleDesc scale[MAX_SCALES];   // coarsest first: file order
    int n_scales;
    int streams_per_image;
    const uint16_t *padding;       // [B][4] left, right, top, bottom
    const int64_t *file_offset;    // [B]
    uint8_t *dst;
};

__device__ __forceinline__ void put_bytes(uint8_t *p, uint32_t v, int n) {
    for (int i = 0; i < n; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

// one stream's payload by the whole block: src rows are 4-byte aligned, the destination is wherever the bytes before it ended
__device__ __forceinline__ void copy_payload(const uint8_t *src, uint8_t *dst, uint32_t n) {
    const uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);   // bytes up to the first aligned dword
    const uint32_t h = head < n ? head : n;
    if (threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
    const uint32_t body = (n - h) / 4;                        // aligned destination dwords
    const uint32_t *src_w = reinterpret_cast<const uint32_t *>(src);
    uint32_t *dst_w = reinterpret_cast<uint32_t *>(dst + h);
    const uint32_t last_word = (n + 3) / 4;                   // source words holding valid bytes: [0, last_word)
    for (uint32_t i = threadIdx.x; i < body; i += blockDim.x) {
        // destination dword i holds source bytes h + 4 i .. h + 4 i + 3
        const uint32_t q = (h + 4 * i) >> 2;
        const uint32_t lo = src_w[q];
        const uint32_t hi = (q + 1 < last_word) ? src_w[q + 1] : 0u;
        dst_w[i] = h ? __builtin_amdgcn_alignbyte(hi, lo, h) : lo;
    }
    const uint32_t tail0 = h + 4 * body;
    if (threadIdx.x < n - tail0) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
}

__global__ __launch_bounds__(256) void container_write_kernel(const ContainerArgs a) {
    const int64_t b = blockIdx.y;
    int j = blockIdx.x;            // stream of this image, file order
    // locate (scale k, channel c) and the byte position of this stream's length field inside the file
    int64_t pos = 8;
    int k = 0;
    for (; k < a.n_scales; ++k) {
        const ScaleDesc &s = a.scale[k];
        if (j < s.C) break;
        pos += 5 + 4;
        for (int c = 0; c < s.C; ++c) pos += 4 + (int64_t)s.nbytes[b * s.C + c];
        j -= s.C;
    }
    const ScaleDesc &s = a.scale[k];
    const int c = j;
    pos += 5;
    for (int cc = 0; cc < c; ++cc) pos += 4 + (int64_t)s.nbytes[b * s.C + cc];
    const uint32_t n = s.nbytes[b * s.C + c];
    uint8_t *file = a.dst + a.file_offset[b];
    if (threadIdx.x == 0) {
        if (k == 0 && c == 0)
            for (int i = 0; i < 4; ++i) put_bytes(file + 2 * i, a.padding[b * 4 + i], 2);
        if (c == 0) {
            file[pos - 5] = (uint8_t)s.C;
            put_bytes(file + pos - 4, (uint32_t)s.H, 2);
            put_bytes(file + pos - 2, (uint32_t)s.W, 2);
        }
        put_bytes(file + pos, n, 4);
        if (c == s.C - 1) put_bytes(file + pos + 4 + n, 0x9284E246u, 4);   // 46 E2 84 92
    }
    copy_payload(s.out + (b * s.C + c) * s.stride, file + pos + 4, n);
}

// ---- banded files ----------------------------------------------------------------------------------------------------

// interval runs: per 64-symbol block and stream 128 words (two roles), contiguous -- 32 uint4 (include/l3c_hip.h, l3c_interval_words)
__global__ __launch_bounds__(256) void band_intervals_kernel(const uint4 *__restrict__ src, int64_t n_streams, int64_t dst_streams,
                                                             int64_t dst_blocks, int64_t per_stream, int64_t first_band,
                                                             int64_t band_blocks, uint4 *__restrict__ dst) {
    const int64_t total = dst_blocks * dst_streams * 32;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t run = q >> 5, w = q & 31;
        const int64_t blk = run / dst_streams, sd = run - blk * dst_streams;
        const int64_t s = sd / per_stream, j = first_band + (sd - s * per_stream);
        dst[q] = src[((j * band_blocks + blk) * n_streams + s) * 32 + w];
    }
}

struct BandedScaleDesc {
    const uint8_t *out_full;
    const uint32_t *nbytes_full;
    int64_t stride_full;
    const uint8_t *out_last;
    const uint32_t *nbytes_last;
    int64_t stride_last;
    int C, H, W;
    int64_t L, n;                  // band length, bands per channel
    int64_t first;                 // index of the scale's first stream in file order
};

struct BandedArgs {
    static constexpr int MAX_SCALES = 8;
    BandedScaleDesc scale[MAX_SCALES];
    int n_scales;
    int64_t streams_per_image;
    const uint16_t *padding;
    const int64_t *file_offset;
    uint8_t *dst;
    int64_t *pos;                  // [B][streams_per_image]: byte position of every length field inside its file
};

// stream i of an image in file order -> (scale k, channel c, band j)
__device__ __forceinline__ int banded_locate(const BandedArgs &a, int64_t i, int64_t &c, int64_t &j) {
    int k = 0;
    while (k + 1 < a.n_scales && i >= a.scale[k + 1].first) ++k;
    const int64_t r = i - a.scale[k].first;
    c = r / a.scale[k].n;
    j = r - c * a.scale[k].n;
    return k;
}

__device__ __forceinline__ uint32_t banded_nbytes(const BandedScaleDesc &s, int64_t b, int64_t c, int64_t j) {
    return j + 1 < s.n ? s.nbytes_full[(b * s.C + c) * (s.n - 1) + j] : s.nbytes_last[b * s.C + c];
}

// one block per image: exclusive scan of (4 + nbytes) over the file's streams, plus the headers in front of each
__global__ __launch_bounds__(256) void banded_positions_kernel(const BandedArgs a) {
    __shared__ int64_t part[256];
    const int64_t b = blockIdx.x;
    int64_t carry = 0;
    for (int64_t base = 0; base < a.streams_per_image; base += 256) {
        const int64_t i = base + threadIdx.x;
        int64_t v = 0;
        int k = 0;
        if (i < a.streams_per_image) {
            int64_t c, j;
            k = banded_locate(a, i, c, j);
            v = 4 + (int64_t)banded_nbytes(a.scale[k], b, c, j);
        }
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {     // inclusive Hillis-Steele scan
            const int64_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < a.streams_per_image)            // 14-byte file header; 9-byte header of scales 0..k, 4-byte magic of scales 0..k-1
            a.pos[b * a.streams_per_image + i] = 14 + 13 * (int64_t)k + 9 + carry + part[threadIdx.x] - v;
        carry += part[255];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void container_write_banded_kernel(const BandedArgs a) {
    const int64_t b = blockIdx.y;
    const int64_t i = blockIdx.x;
    int64_t c, j;
    const int k = banded_locate(a, i, c, j);
    const BandedScaleDesc &s = a.scale[k];
    const int64_t pos = a.pos[b * a.streams_per_image + i];
    const uint32_t n = banded_nbytes(s, b, c, j);
    uint8_t *file = a.dst + a.file_offset[b];
    if (threadIdx.x == 0) {
        if (i == 0) {
            put_bytes(file, 0x4243334Cu, 4);           // 'L3CB'
            file[4] = 1;                                // version
            file[5] = 0;                                // reserved
            for (int q = 0; q < 4; ++q) put_bytes(file + 6 + 2 * q, a.padding[b * 4 + q], 2);
        }
        if (c == 0 && j == 0) {
            file[pos - 9] = (uint8_t)s.C;
            put_bytes(file + pos - 8, (uint32_t)s.H, 2);
            put_bytes(file + pos - 6, (uint32_t)s.W, 2);
            put_bytes(file + pos - 4, (uint32_t)s.L, 4);
        }
        put_bytes(file + pos, n, 4);
        if (c == s.C - 1 && j == s.n - 1) put_bytes(file + pos + 4 + n, 0x9284E246u, 4);   // 46 E2 84 92
    }
    const uint8_t *src = j + 1 < s.n ? s.out_full + ((b * s.C + c) * (s.n - 1) + j) * s.stride_full
                                     : s.out_last + (b * s.C + c) * s.stride_last;
    copy_payload(src, file + pos + 4, n);
}

// one block per (stream, 16 KB slice of its padded length): output dword i = source bytes 4 i .. 4 i + 3 (zero beyond the payload)
__global__ __launch_bounds__(256) void container_read_kernel(const uint8_t *__restrict__ files, const int64_t *__restrict__ src_offset,
                                                             const int64_t *__restrict__ dst_offset, const uint32_t *__restrict__ nbytes,
                                                             uint8_t *__restrict__ dst) {
    const int64_t s = blockIdx.y;
    const uint32_t n = nbytes[s];
    const uint32_t words = (n + 3) / 4 + 1;                  // the padded stream: payload, zeros up to a dword, one zero dword
    const uint8_t *src = files + src_offset[s];
    uint32_t *out = reinterpret_cast<uint32_t *>(dst + dst_offset[s]);
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3);
    const uint32_t *src_w = reinterpret_cast<const uint32_t *>(src - mis);   // aligned words around the payload (inside the file buffer)
    const uint32_t last = (mis + n + 3) / 4;                 // aligned source words holding payload bytes: [0, last)
    for (uint32_t i = blockIdx.x * 4096u + threadIdx.x; i < words && i < (blockIdx.x + 1) * 4096u; i += 256u) {
        uint32_t v = 0;
        if (4 * i < n) {
            const uint32_t lo = src_w[i];
            const uint32_t hi = (i + 1 < last) ? src_w[i + 1] : 0u;
            v = mis ? __builtin_amdgcn_alignbyte(hi, lo, mis) : lo;
            const uint32_t left = n - 4 * i;                 // payload bytes in this dword (1..4 of them when left < 4)
            if (left < 4) v &= (1u << (8 * left)) - 1u;
        }
        out[i] = v;
    }
}

}  // namespace

extern "C" {

int l3c_container_read(const uint8_t *files, const int64_t *src_offset, const int64_t *dst_offset, const uint32_t *nbytes,
                       int64_t n_streams, uint32_t max_nbytes, uint8_t *dst, l3c_stream_t stream) {
    L3C_REQUIRE(files && src_offset && dst_offset && nbytes && dst, "null pointer");
    L3C_REQUIRE(n_streams > 0 && n_streams < 65536, "1..65535 streams per call");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(files) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0, "buffers must be 4-byte aligned");
    // grid.x covers the longest stream (the host has read every length field); a block whose slice lies beyond its own stream does nothing
    const unsigned slices = (unsigned)(((uint64_t)max_nbytes + 3) / 4 + 1 + 4095) / 4096;
    hipLaunchKernelGGL(container_read_kernel, dim3(slices, (unsigned)n_streams), dim3(256), 0, l3c::as_stream(stream), files, src_offset,
                       dst_offset, nbytes, dst);
    return l3c::check_launch("container_read_kernel");
}

int l3c_container_write(const l3c_container_scale *scales, int n_scales, int64_t B, const uint16_t *padding,
                        const int64_t *file_offset, uint8_t *dst, l3c_stream_t stream) {
    L3C_REQUIRE(scales && padding && file_offset && dst, "null pointer");
    L3C_REQUIRE(n_scales > 0 && n_scales <= ContainerArgs::MAX_SCALES, "1..8 scales");
    L3C_REQUIRE(B > 0 && B < 65536, "bad batch size");
    ContainerArgs a{};
    a.n_scales = n_scales;
    a.padding = padding;
    a.file_offset = file_offset;
    a.dst = dst;
    for (int k = 0; k < n_scales; ++k) {
        L3C_REQUIRE(scales[k].out && scales[k].nbytes && scales[k].C > 0 && scales[k].C < 256, "bad scale descriptor");
        L3C_REQUIRE(scales[k].H > 0 && scales[k].H < 65536 && scales[k].W > 0 && scales[k].W < 65536, "scale shape does not fit u16");
        L3C_REQUIRE(scales[k].stride % 4 == 0 && (reinterpret_cast<uintptr_t>(scales[k].out) & 3) == 0, "stream rows must be 4-byte aligned");
        a.scale[k] = ScaleDesc{scales[k].out, scales[k].nbytes, scales[k].stride, scales[k].C, scales[k].H, scales[k].W};
        a.streams_per_image += scales[k].C;
    }
    hipLaunchKernelGGL(container_write_kernel, dim3((unsigned)a.streams_per_image, (unsigned)B), dim3(256), 0,
                       l3c::as_stream(stream), a);
    return l3c::check_launch("container_write_kernel");
}

int l3c_ac_band_intervals(const uint32_t *intervals, int64_t n_streams, int64_t n_sym, int64_t band_len, uint32_t *full_out,
                          uint32_t *last_out, l3c_stream_t stream) {
    L3C_REQUIRE(intervals && last_out, "null pointer");
    L3C_REQUIRE(n_streams > 0 && n_sym > 0 && band_len >= 64 && band_len % 64 == 0, "bad shape (band_len: a positive multiple of 64)");
    const int64_t n = (n_sym + band_len - 1) / band_len;
    L3C_REQUIRE(n == 1 || full_out, "null pointer (full bands)");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(intervals) & 15) == 0 && (reinterpret_cast<uintptr_t>(last_out) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(full_out) & 15) == 0, "interval buffers must be 16-byte aligned");
    const int64_t band_blocks = band_len / 64;
    const hipStream_t st = l3c::as_stream(stream);
    auto launch = [&](uint32_t *dst, int64_t dst_streams, int64_t dst_blocks, int64_t per_stream, int64_t first_band) {
        const int64_t total = dst_blocks * dst_streams * 32;
        const int64_t blocks = (total + 255) / 256;
        hipLaunchKernelGGL(band_intervals_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st,
                           reinterpret_cast<const uint4 *>(intervals), n_streams, dst_streams, dst_blocks, per_stream, first_band,
                           band_blocks, reinterpret_cast<uint4 *>(dst));
        return l3c::check_launch("band_intervals_kernel");
    };
    int rc = L3C_OK;
    if (n > 1) rc = launch(full_out, n_streams * (n - 1), band_blocks, n - 1, 0);
    const int64_t last = n_sym - (n - 1) * band_len;
    if (rc == L3C_OK) rc = launch(last_out, n_streams, (last + 63) / 64, 1, n - 1);
    return rc;
}

static int banded_args(const l3c_banded_scale *scales, int n_scales, int64_t B, BandedArgs *a) {
    L3C_REQUIRE(scales, "null pointer");
    L3C_REQUIRE(n_scales > 0 && n_scales <= BandedArgs::MAX_SCALES, "1..8 scales");
    L3C_REQUIRE(B > 0 && B < 65536, "bad batch size");
    a->n_scales = n_scales;
    int64_t first = 0;
    for (int k = 0; k < n_scales; ++k) {
        const l3c_banded_scale &q = scales[k];
        L3C_REQUIRE(q.C > 0 && q.C < 256 && q.H > 0 && q.H < 65536 && q.W > 0 && q.W < 65536, "bad scale shape (C < 256, H and W fit u16)");
        L3C_REQUIRE(q.band_len >= 64 && q.band_len % 64 == 0 && q.band_len <= 0xFFFFFFFFll, "band_len must be a positive multiple of 64");
        const int64_t n = ((int64_t)q.H * q.W + q.band_len - 1) / q.band_len;
        L3C_REQUIRE(n <= 1024, "more than 1024 bands per channel");
        L3C_REQUIRE(q.out_last && q.nbytes_last && (n == 1 || (q.out_full && q.nbytes_full)), "null pointer in scale descriptor");
        L3C_REQUIRE(q.stride_last % 4 == 0 && (n == 1 || q.stride_full % 4 == 0) &&
                        ((reinterpret_cast<uintptr_t>(q.out_last) | reinterpret_cast<uintptr_t>(q.out_full)) & 3) == 0,
                    "stream rows must be 4-byte aligned");
        a->scale[k] = BandedScaleDesc{q.out_full, q.nbytes_full, q.stride_full, q.out_last, q.nbytes_last, q.stride_last,
                                      q.C, q.H, q.W, q.band_len, n, first};
        first += q.C * n;
    }
    a->streams_per_image = first;
    return L3C_OK;
}

int64_t l3c_container_write_banded_workspace_bytes(const l3c_banded_scale *scales, int n_scales, int64_t B) {
    BandedArgs a{};
    const int rc = banded_args(scales, n_scales, B, &a);
    return rc != L3C_OK ? rc : B * a.streams_per_image * 8;
}

int l3c_container_write_banded(const l3c_banded_scale *scales, int n_scales, int64_t B, const uint16_t *padding,
                               const int64_t *file_offset, uint8_t *dst, void *workspace, int64_t workspace_bytes,
                               l3c_stream_t stream) {
    L3C_REQUIRE(padding && file_offset && dst && workspace, "null pointer");
    BandedArgs a{};
    const int rc = banded_args(scales, n_scales, B, &a);
    if (rc != L3C_OK) return rc;
    L3C_REQUIRE(workspace_bytes >= B * a.streams_per_image * 8 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                "workspace too small or misaligned (l3c_container_write_banded_workspace_bytes)");
    L3C_REQUIRE(a.streams_per_image < (1ll << 31), "too many streams per file");
    a.padding = padding;
    a.file_offset = file_offset;
    a.dst = dst;
    a.pos = static_cast<int64_t *>(workspace);
    const hipStream_t st = l3c::as_stream(stream);
    hipLaunchKernelGGL(banded_positions_kernel, dim3((unsigned)B), dim3(256), 0, st, a);
    int r = l3c::check_launch("banded_positions_kernel");
    if (r != L3C_OK) return r;
    hipLaunchKernelGGL(container_write_banded_kernel, dim3((unsigned)a.streams_per_image, (unsigned)B), dim3(256), 0, st, a);
    return l3c::check_launch("container_write_banded_kernel");
}
}
