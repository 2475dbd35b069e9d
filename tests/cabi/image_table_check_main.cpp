// The image-table validator of l3c_u8_gather / l3c_u8_scatter (l3c-pytorch_amd/csrc/image_table.h: plain C++17, no HIP) as a stand-alone
// program meant to be built with the address and undefined-behaviour sanitizers (the sibling of plan_check_main.cpp):
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/cabi/image_table_check_main.cpp -o image_table_check
//   image_table_check
//
// The validator decides which bytes the kernels may touch, so it is checked against the definition itself: for 4000 seeded random small
// views (every layout, signed strides, offsets on either side of both ends of the buffer) a host walk touches every byte the view
// addresses in a heap buffer of EXACTLY buffer_bytes bytes when the validator accepted it -- a byte outside is a sanitizer report -- and
// looks for a byte outside or a bad field when it refused: a refusal must have a reason.  Then adversarial tables -- strides and offsets
// at the ends of int64, whose products and sums overflow -- must get the answer 128-bit arithmetic gives, without any undefined arithmetic.  Exit status 0: nothing to report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../l3c-pytorch_amd/csrc/image_table.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;      // seeded: the same tables every run
static int64_t rnd(int64_t lo, int64_t hi) {         // uniform in [lo, hi]
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (int64_t)((state >> 33) % (uint64_t)(hi - lo + 1));
}

// the definition: every (y, x, c) of the view; with `buf` the bytes are touched, without it they are only compared with the buffer's ends
static bool walk(const l3c_u8_image &m, int64_t bytes, uint8_t *buf) {
    bool inside = true;
    for (int y = 0; y < m.h; ++y)
        for (int x = 0; x < m.w; ++x)
            for (int c = 0; c < 3; ++c) {
                const int64_t at = m.offset + y * m.row_stride + x * (int64_t)m.pix_stride + c * m.chan_stride;      // small numbers here
                if (at < 0 || at >= bytes)
                    inside = false;
                else if (buf)
                    buf[at] ^= 0x5a;
            }
    return inside;
}

int main() {
    char err[512] = "";
    // ---- the padding rule against its definition: centre padding, the smaller half first
    for (int fac = 1; fac <= 64; ++fac)
        for (int h = 1; h <= 70; ++h) {
            uint16_t p[4];
            if (l3c_images::padding(h, 2 * h + 1, fac, p) != L3C_OK) return fprintf(stderr, "image_table_check: padding refused %d %d\n", h, fac), 1;
            const int H = h + p[2] + p[3], W = 2 * h + 1 + p[0] + p[1];
            if (H % fac || W % fac || H - h >= fac || W - (2 * h + 1) >= fac || p[2] > p[3] || p[3] - p[2] > 1 || p[0] > p[1] || p[1] - p[0] > 1)
                return fprintf(stderr, "image_table_check: padding of %d x %d to %d is wrong\n", h, 2 * h + 1, fac), 1;
        }
    uint16_t p4[4];
    if (l3c_images::padding(0, 5, 8, p4) == L3C_OK || l3c_images::padding(5, 65536, 8, p4) == L3C_OK || l3c_images::padding(5, 5, 0, p4) == L3C_OK ||
        l3c_images::padding(5, 5, 8, nullptr) == L3C_OK)
        return fprintf(stderr, "image_table_check: padding accepted a bad argument\n"), 1;

    // ---- random small views
    int accepted = 0, refused = 0;
    for (int i = 0; i < 4000; ++i) {
        l3c_u8_image m;
        m.h = (int32_t)rnd(i % 50 == 0 ? 0 : 1, 9);
        m.w = (int32_t)rnd(i % 50 == 1 ? 0 : 1, 9);
        m.pix_stride = (int32_t)rnd(i % 50 == 2 ? -1 : 1, 5);
        m.row_stride = rnd(-64, 64);
        const int64_t plane = rnd(0, 600);
        const int64_t cs[6] = {1, -1, plane, -plane, 0, rnd(-700, 700)};
        m.chan_stride = cs[rnd(0, 5)];
        const int64_t bytes = rnd(1, 3000);
        m.offset = rnd(-20, bytes + 20);
        const int Hp = (int)rnd(7, 16), Wp = (int)rnd(7, 16);
        m.top = (int32_t)rnd(-1, 7);
        m.left = (int32_t)rnd(-1, 7);
        const int rc = l3c_images::check_table(&m, 1, Hp, Wp, bytes, err, sizeof(err));
        const bool fields = m.h >= 1 && m.w >= 1 && m.pix_stride >= 1 && m.top >= 0 && m.left >= 0 && m.top + m.h <= Hp && m.left + m.w <= Wp;
        if (rc == L3C_OK) {
            uint8_t *buf = static_cast<uint8_t *>(malloc((size_t)bytes));      // exactly the buffer the validator was told about
            memset(buf, 0, (size_t)bytes);
            const bool inside = walk(m, bytes, buf);
            free(buf);
            if (!fields || !inside) return fprintf(stderr, "image_table_check: table %d was accepted but %s\n", i, fields ? "leaves the buffer" : "has a bad field"), 1;
            ++accepted;
        } else if (rc == L3C_ERR_INVALID_ARG && strncmp(err, "image 0: ", 9) == 0) {
            if (fields && walk(m, bytes, nullptr)) return fprintf(stderr, "image_table_check: table %d was refused without a reason: %s\n", i, err), 1;
            ++refused;
        } else {
            return fprintf(stderr, "image_table_check: table %d: status %d, %s\n", i, rc, err), 1;
        }
    }
    printf("image_table_check: 4000 random tables: %d accepted, %d refused\n", accepted, refused);
    if (accepted < 200 || refused < 200) return fprintf(stderr, "image_table_check: the random tables are one-sided\n"), 1;

    // ---- adversarial: the ends of int64 in every field and pair of fields, the image index in the message
    const int64_t big[] = {INT64_MAX, INT64_MIN, INT64_MAX / 2 + 1, INT64_MIN / 2 - 1, INT64_MAX / 65534, -(INT64_MAX / 65534) - 7, (int64_t)1 << 62, -((int64_t)1 << 62)};
    const int n_big = (int)(sizeof(big) / sizeof(big[0]));
    int adversarial = 0, kept = 0;
    for (int a = 0; a < n_big; ++a)
        for (int b = -1; b < n_big; ++b)
            for (int field = 0; field < 6; ++field) {
                l3c_u8_image t[3];
                for (int k = 0; k < 3; ++k) t[k] = l3c_u8_image{0, 24, 1, 3, 8, 8, 0, 0};      // three good 8 x 8 RGB images in 192 bytes
                l3c_u8_image &m = t[2];
                m.h = m.w = 65535;
                int64_t *f[3] = {&m.offset, &m.row_stride, &m.chan_stride};
                *f[field % 3] = big[a];
                if (b >= 0) *f[(field + 1 + field / 3) % 3] = big[b];
                if (field >= 3) m.pix_stride = INT32_MAX;
                const int64_t bytes = (a + b) % 2 ? INT64_MAX : 192;
                const int rc = l3c_images::check_table(t, 3, 65535, 65535, bytes, err, sizeof(err));
                // the same extremes in 128-bit arithmetic, where nothing here overflows
                __int128 lo = m.offset, hi = m.offset;
                const __int128 span[3] = {(__int128)65534 * m.row_stride, (__int128)65534 * m.pix_stride, (__int128)2 * m.chan_stride};
                for (int k = 0; k < 3; ++k) (span[k] < 0 ? lo : hi) += span[k];
                const bool fits = lo >= 0 && hi < bytes;
                if (fits ? rc != L3C_OK : (rc != L3C_ERR_INVALID_ARG || strncmp(err, "image 2: ", 9) != 0))
                    return fprintf(stderr, "image_table_check: adversarial table (%d, %d, %d): status %d, %s\n", a, b, field, rc, err), 1;
                ++adversarial;
                kept += fits;
            }
    // the largest view there is, exactly filling its buffer, is accepted; one byte less is not
    l3c_u8_image full = {2, (int64_t)65535 * 4, -1, 4, 65535, 65535, 0, 0};                 // BGRX
    const int64_t full_bytes = (int64_t)65535 * 65535 * 4 - 1;                               // the last pixel's X byte is outside every view
    if (l3c_images::check_table(&full, 1, 65535, 65535, full_bytes, err, sizeof(err)) != L3C_OK ||
        l3c_images::check_table(&full, 1, 65535, 65535, full_bytes - 1, err, sizeof(err)) != L3C_ERR_INVALID_ARG)
        return fprintf(stderr, "image_table_check: the 65535 x 65535 view: %s\n", err), 1;
    printf("image_table_check: %d adversarial tables: %d fit their buffer, %d refused\n", adversarial, kept, adversarial - kept);
    return 0;
}
