// images.hip -- pictures as they come, to and from the planar frames the codec reads and writes (include/l3c_hip.h: l3c_u8_gather /
// l3c_u8_scatter).  A per-image table (csrc/image_table.h: l3c_u8_image) says where each image lies in ONE caller-owned byte buffer --
// planar, RGB, RGBX or BGR(X), any row pitch, every image its own size -- and where it sits in its Hp x Wp frame:
//     gather    buffer -> uint8 planar [B][3][Hp][Wp], zero outside the image (helpers/pad.py with mode 'constant': what encode_set pads
//               with), and the (left, right, top, bottom) array l3c_encode_batch_desc.padding expects
//     scatter   the inverse crop: exactly the 3 h w bytes each view addresses are written
// One launch for the whole batch, whatever the mix.  A thread owns 4 V consecutive pixels of one frame row, all three channels: the FRAME
// side moves as one V-dword access per channel (V = 4, 2 or 1: the widest that divides Wp, so every access is naturally aligned); the
// strided side moves as whole dwords too where the thread's pixels are ONE run of bytes -- a planar row (pix_stride == 1) that is dword
// aligned; packed pixels (chan_stride == +-1, pix_stride 3 or 4), whatever their alignment: the aligned dwords around the run, realigned
// with funnel shifts and taken apart (put together) in registers -- and byte by byte otherwise: frame edges, other strides, RGBX on the way
// back (its X bytes are not the kernel's to write).
// The table is validated on the host before a launch (image_table.h).  Stores touch nothing but what it validated; the packed loads may
// read up to 3 bytes on either side of a run, inside the buffer: a run too close to the buffer's ends for that goes byte by byte.
#include "image_table.h"
#include "l3c_common.h"

namespace {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int V>
struct Vec;
template <>
struct Vec<1> {
    typedef uint32_t type;
};
template <>
struct Vec<2> {
    typedef uint2 type;
};
template <>
struct Vec<4> {
    typedef uint4 type;
};

// the thread's place: image b, frame row y, first column x0 of its 4 V pixels
struct Place {
    int64_t b;
    int y, x0;
};

__device__ __forceinline__ Place place_of(int64_t unit, int per_row, int Hp, int px) {
    const int64_t row = unit / per_row;
    Place p;
    p.x0 = (int)(unit - row * per_row) * px;
    p.b = row / Hp;
    p.y = (int)(row - p.b * Hp);
    return p;
}

// byte `idx` of a run held as little-endian dwords
template <int N>
__device__ __forceinline__ uint32_t run_byte(const uint32_t (&d)[N], int idx) {
    return (d[idx >> 2] >> (8 * (idx & 3))) & 0xffu;
}

// PACKED pixels: the 4 V pixels of a thread are one run of 4 V PS bytes from `lo` (the pixels' lowest byte) on, N = V PS dwords.  Loads the
// N + 1 aligned dwords around the run and shifts them into place; the caller has checked that they lie inside the buffer.
template <int N>
__device__ __forceinline__ void load_run(const uint8_t *lo, uint32_t (&d)[N]) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(lo);
    const uint32_t *a = reinterpret_cast<const uint32_t *>(p & ~static_cast<uintptr_t>(3));
    const uint32_t shift = 8 * static_cast<uint32_t>(p & 3);
    uint32_t raw[N + 1];
#pragma unroll
    for (int i = 0; i <= N; ++i) raw[i] = a[i];
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = __funnelshift_r(raw[i], raw[i + 1], shift);
}

// the run as three words per dword of frame: position q of every pixel (q = 0, 1, 2: R, G, B of RGB(X); B, G, R of BGR(X))
template <int V, int PS>
__device__ __forceinline__ void split_run(const uint32_t (&d)[V * PS], uint32_t (&word)[3][V]) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int v = 0; v < V; ++v) {
            uint32_t acc = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc |= run_byte(d, (4 * v + j) * PS + q) << (8 * j);
            word[q][v] = acc;
        }
}

// the inverse for PS == 3: the 12 V bytes of the run from the three words per dword of frame
template <int V>
__device__ __forceinline__ void join_run(const uint32_t (&word)[3][V], uint32_t (&d)[3 * V]) {
#pragma unroll
    for (int i = 0; i < 3 * V; ++i) {
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = 4 * i + k, pixel = idx / 3, q = idx % 3;
            acc |= ((word[q][pixel >> 2] >> (8 * (pixel & 3))) & 0xffu) << (8 * k);
        }
        d[i] = acc;
    }
}

// stores the run at `lo`, whatever its alignment: whole dwords inside, up to 3 single bytes at either end.  Only the run's bytes are written.
template <int N>
__device__ __forceinline__ void store_run(uint8_t *lo, const uint32_t (&d)[N]) {
    const uint32_t off = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lo) & 3);
    if (off == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) reinterpret_cast<uint32_t *>(lo)[i] = d[i];
        return;
    }
    const uint32_t head = 4 - off;                       // bytes in front of the first aligned dword; `off` bytes behind the last one
#pragma unroll
    for (uint32_t t = 0; t < 3; ++t)
        if (t < head) lo[t] = static_cast<uint8_t>(d[0] >> (8 * t));
    uint32_t *mid = reinterpret_cast<uint32_t *>(lo + head);
#pragma unroll
    for (int i = 0; i + 1 < N; ++i) mid[i] = __funnelshift_r(d[i], d[i + 1], 8 * head);
    uint8_t *tail = lo + 4 * N - off;
#pragma unroll
    for (uint32_t t = 0; t < 3; ++t)
        if (t < off) tail[t] = static_cast<uint8_t>(d[N - 1] >> (8 * (head + t)));
}

template <int V>
__global__ __launch_bounds__(256) void u8_gather_kernel(const uint8_t *__restrict__ src, int64_t src_bytes, const l3c_u8_image *__restrict__ images,
                                                        int64_t B, int Hp, int Wp, uint8_t *__restrict__ dst, uint16_t *__restrict__ padding_out) {
    typedef typename Vec<V>::type vec_t;
    constexpr int PX = 4 * V;
    const int per_row = Wp / PX;
    const int64_t units = B * Hp * per_row, stride = (int64_t)gridDim.x * 256;
    for (int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x; unit < units; unit += stride) {
        const Place p = place_of(unit, per_row, Hp, PX);
        const l3c_u8_image m = images[p.b];
        if (padding_out && p.y == 0 && p.x0 == 0) {
            const uint32_t left = (uint32_t)m.left, right = (uint32_t)(Wp - m.left - m.w), top = (uint32_t)m.top, bottom = (uint32_t)(Hp - m.top - m.h);
            *reinterpret_cast<uint2 *>(padding_out + 4 * p.b) = make_uint2(left | right << 16, top | bottom << 16);
        }
        const int yi = p.y - m.top, xi = p.x0 - m.left;              // the thread's pixels in the image's own coordinates
        const bool row_in = yi >= 0 && yi < m.h;
        const bool whole = row_in && xi >= 0 && xi + PX <= m.w;      // all 4 V pixels inside the image
        const int64_t at = m.offset + (int64_t)yi * m.row_stride + (int64_t)xi * m.pix_stride;
        uint8_t *out = dst + ((p.b * 3 * Hp + p.y) * (int64_t)Wp + p.x0);
        const bool packed = whole && (m.chan_stride == 1 || m.chan_stride == -1) && (m.pix_stride == 3 || m.pix_stride == 4);
        if (packed) {
            const uint8_t *lo = src + at + (m.chan_stride < 0 ? -2 : 0);
            const uintptr_t first = reinterpret_cast<uintptr_t>(lo) & ~static_cast<uintptr_t>(3);
            const uintptr_t last = first + 4 * (V * (uintptr_t)m.pix_stride + 1);            // behind the N + 1 aligned dwords
            if (first >= reinterpret_cast<uintptr_t>(src) && last <= reinterpret_cast<uintptr_t>(src) + (uintptr_t)src_bytes) {
                uint32_t word[3][V];
                if (m.pix_stride == 3) {
                    uint32_t run[3 * V];
                    load_run(lo, run);
                    split_run<V, 3>(run, word);
                } else {
                    uint32_t run[4 * V];
                    load_run(lo, run);
                    split_run<V, 4>(run, word);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    vec_t *o = reinterpret_cast<vec_t *>(out + (int64_t)c * Hp * Wp);
                    uint32_t w[V];
#pragma unroll
                    for (int v = 0; v < V; ++v) w[v] = m.chan_stride < 0 ? word[2 - c][v] : word[c][v];
                    if constexpr (V == 1) *o = w[0];
                    if constexpr (V == 2) *o = make_uint2(w[0], w[1]);
                    if constexpr (V == 4) *o = make_uint4(w[0], w[1], w[2], w[3]);
                }
                continue;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t word[V];
            const uint8_t *in = src + at + c * m.chan_stride;
            if (whole && m.pix_stride == 1 && (reinterpret_cast<uintptr_t>(in) & 3) == 0) {
#pragma unroll
                for (int v = 0; v < V; ++v) word[v] = reinterpret_cast<const uint32_t *>(in)[v];
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    uint32_t acc = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = xi + 4 * v + j;
                        if (row_in && x >= 0 && x < m.w) acc |= (uint32_t)in[(int64_t)(4 * v + j) * m.pix_stride] << (8 * j);
                    }
                    word[v] = acc;
                }
            }
            vec_t *o = reinterpret_cast<vec_t *>(out + (int64_t)c * Hp * Wp);
            if constexpr (V == 1) *o = word[0];
            if constexpr (V == 2) *o = make_uint2(word[0], word[1]);
            if constexpr (V == 4) *o = make_uint4(word[0], word[1], word[2], word[3]);
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void u8_scatter_kernel(const uint8_t *__restrict__ src, const l3c_u8_image *__restrict__ images, int64_t B, int Hp,
                                                         int Wp, uint8_t *__restrict__ dst) {
    typedef typename Vec<V>::type vec_t;
    constexpr int PX = 4 * V;
    const int per_row = Wp / PX;
    const int64_t units = B * Hp * per_row, stride = (int64_t)gridDim.x * 256;
    for (int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x; unit < units; unit += stride) {
        const Place p = place_of(unit, per_row, Hp, PX);
        const l3c_u8_image m = images[p.b];
        const int yi = p.y - m.top, xi = p.x0 - m.left;
        if (yi < 0 || yi >= m.h || xi + PX <= 0 || xi >= m.w) continue;      // nothing of the image in these pixels
        const bool whole = xi >= 0 && xi + PX <= m.w;
        const int64_t at = m.offset + (int64_t)yi * m.row_stride + (int64_t)xi * m.pix_stride;
        const uint8_t *in = src + ((p.b * 3 * Hp + p.y) * (int64_t)Wp + p.x0);
        uint32_t frame[3][V];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const vec_t got = *reinterpret_cast<const vec_t *>(in + (int64_t)c * Hp * Wp);
            if constexpr (V == 1) frame[c][0] = got;
            if constexpr (V == 2) frame[c][0] = got.x, frame[c][1] = got.y;
            if constexpr (V == 4) frame[c][0] = got.x, frame[c][1] = got.y, frame[c][2] = got.z, frame[c][3] = got.w;
        }
        if (whole && m.pix_stride == 3 && (m.chan_stride == 1 || m.chan_stride == -1)) {      // packed RGB / BGR: the run is all the thread's
            uint32_t word[3][V], run[3 * V];
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int v = 0; v < V; ++v) word[q][v] = m.chan_stride < 0 ? frame[2 - q][v] : frame[q][v];
            join_run<V>(word, run);
            store_run(dst + at + (m.chan_stride < 0 ? -2 : 0), run);
            continue;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t(&word)[V] = frame[c];
            uint8_t *out = dst + at + c * m.chan_stride;
            if (whole && m.pix_stride == 1 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
#pragma unroll
                for (int v = 0; v < V; ++v) reinterpret_cast<uint32_t *>(out)[v] = word[v];
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = xi + 4 * v + j;
                        if (x >= 0 && x < m.w) out[(int64_t)(4 * v + j) * m.pix_stride] = (uint8_t)(word[v] >> (8 * j));
                    }
            }
        }
    }
}

inline unsigned grid_of(int64_t B, int Hp, int Wp, int px) {
    const int64_t blocks = (B * Hp * (Wp / px) + 255) / 256;
    return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

}  // namespace

namespace l3c {

int images_check(const l3c_u8_image *images_host, const l3c_u8_image *images, int64_t B, int Hp, int Wp, int64_t buffer_bytes) {
    L3C_REQUIRE(images_host && images, "null pointer");
    L3C_REQUIRE(B > 0 && B < 65536, "bad batch size (1 .. 65535)");
    L3C_REQUIRE(Hp > 0 && Hp < 65536 && Wp > 0 && Wp < 65536, "bad frame: Hp and Wp must be 1 .. 65535");
    L3C_REQUIRE(Wp % 4 == 0, "bad frame: Wp must be a multiple of 4 (the frames move as whole dwords)");
    L3C_REQUIRE(aligned16(images), "the device table must be 16-byte aligned");
    L3C_REQUIRE(buffer_bytes > 0, "empty buffer");
    return l3c_images::check_table(images_host, B, Hp, Wp, buffer_bytes, error_buffer(), 512);
}

}  // namespace l3c

extern "C" {

int l3c_image_padding(int h, int w, int fac, uint16_t *pad_out) {
    L3C_REQUIRE(pad_out, "null pointer");
    L3C_REQUIRE(l3c_images::padding(h, w, fac, pad_out) == L3C_OK, "h, w and fac must be 1 .. 65535");
    return L3C_OK;
}

int l3c_image_table_check(const l3c_u8_image *images_host, int64_t B, int Hp, int Wp, int64_t buffer_bytes) {
    L3C_REQUIRE(images_host, "null pointer");
    L3C_REQUIRE(B > 0 && B < 65536, "bad batch size (1 .. 65535)");
    return l3c_images::check_table(images_host, B, Hp, Wp, buffer_bytes, l3c::error_buffer(), 512);
}

int l3c_u8_gather(const uint8_t *src, int64_t src_bytes, const l3c_u8_image *images_host, const l3c_u8_image *images, int64_t B, int Hp, int Wp,
                  uint8_t *dst, uint16_t *padding_out, l3c_stream_t stream) {
    L3C_REQUIRE(src && dst, "null pointer");
    const int rc = l3c::images_check(images_host, images, B, Hp, Wp, src_bytes);
    if (rc != L3C_OK) return rc;
    L3C_REQUIRE(aligned16(dst) && aligned16(padding_out), "the planar frames and padding_out must be 16-byte aligned");
    const hipStream_t st = l3c::as_stream(stream);
    if (Wp % 16 == 0)
        hipLaunchKernelGGL(u8_gather_kernel<4>, dim3(grid_of(B, Hp, Wp, 16)), dim3(256), 0, st, src, src_bytes, images, B, Hp, Wp, dst, padding_out);
    else if (Wp % 8 == 0)
        hipLaunchKernelGGL(u8_gather_kernel<2>, dim3(grid_of(B, Hp, Wp, 8)), dim3(256), 0, st, src, src_bytes, images, B, Hp, Wp, dst, padding_out);
    else
        hipLaunchKernelGGL(u8_gather_kernel<1>, dim3(grid_of(B, Hp, Wp, 4)), dim3(256), 0, st, src, src_bytes, images, B, Hp, Wp, dst, padding_out);
    return l3c::check_launch("u8_gather_kernel");
}

int l3c_u8_scatter(const uint8_t *src, int64_t B, int Hp, int Wp, uint8_t *dst, int64_t dst_bytes, const l3c_u8_image *images_host,
                   const l3c_u8_image *images, l3c_stream_t stream) {
    L3C_REQUIRE(src && dst, "null pointer");
    const int rc = l3c::images_check(images_host, images, B, Hp, Wp, dst_bytes);
    if (rc != L3C_OK) return rc;
    L3C_REQUIRE(aligned16(src), "the planar frames must be 16-byte aligned");
    const hipStream_t st = l3c::as_stream(stream);
    if (Wp % 16 == 0)
        hipLaunchKernelGGL(u8_scatter_kernel<4>, dim3(grid_of(B, Hp, Wp, 16)), dim3(256), 0, st, src, images, B, Hp, Wp, dst);
    else if (Wp % 8 == 0)
        hipLaunchKernelGGL(u8_scatter_kernel<2>, dim3(grid_of(B, Hp, Wp, 8)), dim3(256), 0, st, src, images, B, Hp, Wp, dst);
    else
        hipLaunchKernelGGL(u8_scatter_kernel<1>, dim3(grid_of(B, Hp, Wp, 4)), dim3(256), 0, st, src, images, B, Hp, Wp, dst);
    return l3c::check_launch("u8_scatter_kernel");
}
}
