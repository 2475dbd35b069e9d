// image_table.h -- the per-image table of l3c_u8_gather / l3c_u8_scatter (include/l3c_hip.h: l3c_u8_image), its validator and the padding rule.
//
// Plain C++17 on purpose, as codec_plan.h: no HIP include, no library call, no allocation, so that the code that decides which bytes a
// kernel may touch compiles into a stand-alone program (tests/cabi/image_table_check_main.cpp, built with the address and
// undefined-behaviour sanitizers) as well as into libl3c_hip.so (csrc/images.hip, csrc/codec.hip).
//
// A VIEW addresses byte  offset + y * row_stride + x * pix_stride + c * chan_stride  of one caller-owned buffer for y < h, x < w, c < 3.
// Only pix_stride must be positive; row_stride and chan_stride are signed (a bottom-up image, BGR seen from its R byte).  The address is
// linear in (y, x, c), so its extremes are at the corners: the validator sums the per-axis minima and maxima with overflow-checked 64-bit
// arithmetic and accepts a view only if every byte of it lies inside [0, buffer_bytes).  The kernels trust a table that passed.
#ifndef L3C_IMAGE_TABLE_H_
#define L3C_IMAGE_TABLE_H_

#include <stdint.h>
#include <stdio.h>

#include "../../include/l3c_hip.h"

namespace l3c_images {

constexpr int MAX_SIDE = 65535;      // the u16 fields of a `.l3c` file

inline int fail(char *err, size_t cap, long long image, const char *what) {
    if (err && cap) snprintf(err, cap, "image %lld: %s", image, what);
    return L3C_ERR_INVALID_ARG;
}

// helpers/pad.py: padding_for -- centre padding to the next multiple of fac, the smaller half first.  pad_out: left, right, top, bottom.
inline int padding(int h, int w, int fac, uint16_t pad_out[4]) {
    if (!pad_out || h < 1 || w < 1 || h > MAX_SIDE || w > MAX_SIDE || fac < 1 || fac > MAX_SIDE) return L3C_ERR_INVALID_ARG;
    const int ph = (fac - h % fac) % fac, pw = (fac - w % fac) % fac;
    pad_out[0] = (uint16_t)(pw / 2);
    pad_out[1] = (uint16_t)(pw - pw / 2);
    pad_out[2] = (uint16_t)(ph / 2);
    pad_out[3] = (uint16_t)(ph - ph / 2);
    return L3C_OK;
}

// lo += min(0, n * stride), hi += max(0, n * stride); false on overflow
inline bool extend(int64_t n, int64_t stride, int64_t *lo, int64_t *hi) {
    int64_t span;
    if (__builtin_mul_overflow(n, stride, &span)) return false;
    return span < 0 ? !__builtin_add_overflow(*lo, span, lo) : !__builtin_add_overflow(*hi, span, hi);
}

// [lo, hi]: the lowest and the highest byte the view addresses; false on overflow
inline bool extent(const l3c_u8_image &m, int64_t *lo, int64_t *hi) {
    *lo = *hi = m.offset;
    return extend((int64_t)m.h - 1, m.row_stride, lo, hi) && extend((int64_t)m.w - 1, m.pix_stride, lo, hi) && extend(2, m.chan_stride, lo, hi);
}

// Every image of the table against the Hp x Wp frame and the buffer of buffer_bytes bytes.  L3C_OK, or L3C_ERR_INVALID_ARG with a message
// naming the first offending image and field.
inline int check_table(const l3c_u8_image *t, int64_t B, int64_t Hp, int64_t Wp, int64_t buffer_bytes, char *err, size_t cap) {
    if (!t) return fail(err, cap, -1, "null table");
    for (int64_t k = 0; k < B; ++k) {
        const l3c_u8_image &m = t[k];
        if (m.h < 1 || m.h > MAX_SIDE) return fail(err, cap, k, "h must be 1 .. 65535");
        if (m.w < 1 || m.w > MAX_SIDE) return fail(err, cap, k, "w must be 1 .. 65535");
        if (m.pix_stride < 1) return fail(err, cap, k, "pix_stride must be positive");
        if (m.top < 0 || (int64_t)m.top + m.h > Hp) return fail(err, cap, k, "top + h exceeds the frame's Hp");
        if (m.left < 0 || (int64_t)m.left + m.w > Wp) return fail(err, cap, k, "left + w exceeds the frame's Wp");
        int64_t lo, hi;
        if (!extent(m, &lo, &hi)) return fail(err, cap, k, "offset and strides overflow 64 bits");
        if (lo < 0) return fail(err, cap, k, "the view starts before the buffer (offset, row_stride, chan_stride)");
        if (hi >= buffer_bytes) return fail(err, cap, k, "the view ends behind the buffer (offset, row_stride, pix_stride, chan_stride)");
    }
    return L3C_OK;
}

}  // namespace l3c_images

#endif
