// The region planner (l3c-pytorch_amd/csrc/codec_plan_region.h: plain C++17, no HIP) as a stand-alone program meant to be built with the
// address and undefined-behaviour sanitizers (the sibling of plan_banded_check_main.cpp):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/cabi/region_plan_check_main.cpp -o region_plan_check
//   region_plan_check
//
// It frames banded files of a 328 x 88 and a 712 x 88 image itself (K = 1, 16, 64; the planners read no payload byte), plans them, and
//   1. plans EVERY box (y0, y1) of each and checks the plan's invariants: v0 <= p0, p1 <= v1, every entry inside the window, the lengths
//      summing to the symbol rows, the picked streams inside the file, the crop inside the window -- and that region_check accepts the blob;
//   2. feeds the region planner truncated and bit-flipped PLAN blobs (either answer; an accepted one must pass the same invariants);
//   3. feeds it boxes of extreme values (must be refused), and region_check bit-flipped REGION blobs (refused, or still a blob the planner
//      would have written: the same invariants).
// Every buffer is heap memory of exactly the size the planner is told, so a read or write past an end is a sanitizer report.  Exit status
// 0: nothing to report.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../l3c-pytorch_amd/csrc/codec_plan_region.h"

using namespace l3c_plan;

static const l3c_net_config CFG = {3, 64, 5, 25, 10, 8, 8, 0, 1};      // configs/ms/cr.cf
static const int W = 88;

static void put16(std::vector<uint8_t> &f, unsigned v) { f.push_back(v & 255); f.push_back(v >> 8 & 255); }
static void put32(std::vector<uint8_t> &f, unsigned v) { put16(f, v & 65535); put16(f, v >> 16); }

// bitcoding/container.py: write_file(banded=True) of an H x W image with K bands, payloads of a few bytes
static std::vector<uint8_t> banded_file(int H, int K, const uint16_t pad[4]) {
    std::vector<uint8_t> f = {'L', '3', 'C', 'B', 1, 0};
    for (int i = 0; i < 4; ++i) put16(f, pad[i]);
    for (int s = CFG.num_scales; s >= 0; --s) {
        const int C = s ? CFG.C : 3, h = H >> s, w = W >> s;
        const int64_t hw = (int64_t)h * w, L = 64 * ((hw + 64 * K - 1) / (64 * K)), n = (hw + L - 1) / L;
        f.push_back((uint8_t)C);
        put16(f, h);
        put16(f, w);
        put32(f, (unsigned)L);
        for (int c = 0; c < C; ++c)
            for (int64_t j = 0; j < n; ++j) {
                const unsigned nb = (unsigned)((j * 7 + c * 3 + s) % 6);
                put32(f, nb);
                for (unsigned i = 0; i < nb; ++i) f.push_back((uint8_t)(i + j));
            }
        const uint8_t sep[4] = {0x46, 0xE2, 0x84, 0x92};
        f.insert(f.end(), sep, sep + 4);
    }
    return f;
}

struct Planned {
    std::vector<uint8_t> file;
    int64_t *blob;
    int64_t bytes;
    uint16_t pad[4];
    int H;
};

static bool plan_file(int H, int K, const uint16_t pad[4], Planned *out, char *err) {
    out->file = banded_file(H, K, pad);
    const int64_t offs[2] = {0, (int64_t)out->file.size()};
    out->bytes = plan_banded_bytes(&CFG, out->file.data(), offs, 1, err, 512);
    if (out->bytes < 0) return false;
    out->blob = static_cast<int64_t *>(malloc((size_t)out->bytes));
    int h = 0, w = 0;
    out->H = H;
    return make_plan_banded(&CFG, out->file.data(), offs, 1, out->blob, out->bytes, &h, &w, out->pad, err, 512) == L3C_OK && h == H && w == W;
}

// the invariants of an accepted region blob of exactly `bytes` bytes
static bool consistent(const void *region, int64_t bytes, const l3c_region_info &info, int64_t files_bytes) {
    RegionHeader h;
    memcpy(&h, region, sizeof(h));
    const RegionRows &r = h.rows;
    if (h.magic != REGION_MAGIC || h.bytes != bytes || h.B < 1 || h.S != h.B * (r.j1 - r.j0) || h.S < 1) return false;
    if (!(0 <= r.c0 && r.c0 <= r.v0 && r.v0 <= r.p0 && r.p0 < r.p1 && r.p1 <= r.v1 && r.v1 <= r.c1 && r.c1 <= h.H)) return false;
    if (r.c0 % 64 || (r.c1 % 64 && r.c1 != h.H) || r.c0 % 2 || r.c1 % 2) return false;
    if (!(0 <= h.a0 && h.a0 <= r.c0 && r.c1 <= h.a1 && h.a1 <= h.H && h.a0 % 2 == 0 && h.a1 % 2 == 0)) return false;
    if (!(0 <= r.j0 && r.j0 < r.j1 && r.j1 <= h.n) || h.n_chunks < 1 || h.n_chunks > 32 || (h.lag != 1 && h.lag != 2)) return false;
    if (info.bands[0] != r.j0 || info.conv_rows[1] != r.c1 || info.streams_used != 3 * h.S || info.lag != h.lag) return false;
    const char *base = static_cast<const char *>(region);
    const int64_t *src = reinterpret_cast<const int64_t *>(base + h.src_off), *dst = reinterpret_cast<const int64_t *>(base + h.dst_off);
    const uint32_t *nb = reinterpret_cast<const uint32_t *>(base + h.nbytes_off);
    int64_t used = 0;
    for (int64_t t = 0; t < 3 * h.S; ++t) {
        if (src[t] < 0 || src[t] > files_bytes - (int64_t)nb[t] || dst[t] < 0 || dst[t] % 4 || dst[t] + (int64_t)nb[t] + 4 > h.dst_bytes) return false;
        if ((int64_t)nb[t] > h.max_nbytes) return false;
        used += nb[t];
    }
    if (used != h.bytes_used || h.bytes_used > h.bytes_total) return false;
    const int64_t *e = reinterpret_cast<const int64_t *>(base + h.entries_off);
    const int64_t hw = (r.c1 - r.c0) * h.W, S = h.S;
    for (int64_t b = 0; b < h.B; ++b) {
        int64_t sum = 0;
        for (int64_t i = b * (r.j1 - r.j0); i < (b + 1) * (r.j1 - r.j0); ++i) {
            if (e[i] != b * hw || e[S + i] != hw || e[2 * S + i] < 0 || e[3 * S + i] < 1 || e[2 * S + i] + e[3 * S + i] > hw) return false;
            if (i > b * (r.j1 - r.j0) && e[2 * S + i] != e[2 * S + i - 1] + e[3 * S + i - 1]) return false;      // the bands follow one another
            sum += e[3 * S + i];
        }
        // from the first band's first pixel to the last pixel of row p1 - 1: the symbol rows, less the start of row p0 that lies in band j0 - 1
        if (sum != r.p1 * h.W - r.j0 * h.L || r.j0 * h.L / h.W != r.p0) return false;
    }
    const l3c_u8_image *crop = reinterpret_cast<const l3c_u8_image *>(base + h.crop_off);
    for (int64_t b = 0; b < h.B; ++b) {
        const l3c_u8_image &m = crop[b];
        if (m.h != info.out_rows || m.w != info.out_cols || m.top < 0 || m.top + m.h > r.c1 - r.c0 || m.left < 0 || m.left + m.w > h.W) return false;
        if (m.top + r.c0 < r.p0 || m.top + m.h + r.c0 != r.p1 || m.offset != b * 3 * (int64_t)m.h * m.w) return false;
    }
    return true;
}

// plan one box with buffers of exactly the sizes told -> status; *ok: the invariants of an accepted plan, and region_check's agreement
// (exact: `plan` is heap memory of exactly plan_bytes bytes already; otherwise a copy of that size is planned from)
static int plan_box(const int64_t *plan, int64_t plan_bytes, const uint16_t *pad, l3c_region_box box, int64_t files_bytes, bool *ok, char *err,
                    bool exact = false) {
    int64_t *copy = exact ? const_cast<int64_t *>(plan) : static_cast<int64_t *>(malloc(plan_bytes ? (size_t)plan_bytes : 1));
    if (!exact && plan_bytes) memcpy(copy, plan, (size_t)plan_bytes);
    *ok = false;
    RegionView v;
    int rc = region_view(CFG, copy, plan_bytes, &v, err, 512);
    if (rc == L3C_OK) {
        // the size of THIS box's blob: the largest one is what l3c_decode_region_plan_bytes gives, a buffer one byte short must be refused
        const int64_t cap = region_plan_bytes(&CFG, copy, err, 512);
        int64_t *region = static_cast<int64_t *>(malloc((size_t)cap));
        l3c_region_info info;
        rc = make_region_plan(&CFG, copy, plan_bytes, pad, &box, region, cap, &info, err, 512);
        if (rc == L3C_OK) {
            RegionHeader h, again;
            memcpy(&h, region, sizeof(h));
            int64_t *exact = static_cast<int64_t *>(malloc((size_t)h.bytes));
            memcpy(exact, region, (size_t)h.bytes);
            *ok = h.bytes <= cap && consistent(exact, h.bytes, info, files_bytes) &&
                  region_check(CFG, copy, plan_bytes, exact, h.bytes, &again, err, 512) == L3C_OK && memcmp(&h, &again, sizeof(h)) == 0 &&
                  make_region_plan(&CFG, copy, plan_bytes, pad, &box, region, h.bytes - 1, &info, err, 512) == L3C_ERR_INVALID_ARG;
            free(exact);
        }
        free(region);
    }
    if (!exact) free(copy);
    return rc;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;      // seeded: the same mutations every run
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 33;
}

int main() {
    char err[512] = "";
    long boxes = 0;
    const uint16_t pads[2][4] = {{0, 0, 0, 0}, {2, 3, 1, 2}};
    std::vector<Planned> plans;
    for (int H : {328, 712})
        for (int K : {1, 16, 64}) {
            Planned p;
            if (!plan_file(H, K, pads[K == 16], &p, err)) {
                fprintf(stderr, "region_plan_check: %d rows, K = %d: the file is refused: %s\n", H, K, err);
                return 1;
            }
            plans.push_back(p);
            const int h_img = H - p.pad[2] - p.pad[3], w_img = W - p.pad[0] - p.pad[1];
            for (int y0 = 0; y0 < h_img; ++y0)
                for (int y1 = y0 + 1; y1 <= h_img; ++y1) {
                    bool ok;
                    const l3c_region_box box = {y0, y1, (y0 * 5) % w_img, (y0 * 5) % w_img + 1 + (y1 * 3) % (w_img - (y0 * 5) % w_img)};
                    if (plan_box(p.blob, p.bytes, p.pad, box, (int64_t)p.file.size(), &ok, err, true) != L3C_OK || !ok) {
                        fprintf(stderr, "region_plan_check: %d rows, K = %d, box [%d, %d) x [%d, %d): %s\n", H, K, y0, y1, box.x0, box.x1, err);
                        return 1;
                    }
                    ++boxes;
                }
        }
    printf("region_plan_check: %ld boxes planned and checked\n", boxes);

    // 2. truncated and bit-flipped plan blobs
    int accepted = 0, refused = 0;
    for (const Planned &p : plans) {
        const l3c_region_box box = {100, 140, 5, 60};
        bool ok;
        for (int64_t n = 0; n < p.bytes; n += 8) {
            const int rc = plan_box(p.blob, n, p.pad, box, (int64_t)p.file.size(), &ok, err);
            if (rc != L3C_ERR_INVALID_ARG) {
                fprintf(stderr, "region_plan_check: a plan blob cut to %lld bytes: status %d, %s\n", (long long)n, rc, err);
                return 1;
            }
        }
        for (int i = 0; i < 3000; ++i) {
            std::vector<int64_t> m(p.blob, p.blob + p.bytes / 8);
            // the header's words decide what is read where: most flips go there, the rest anywhere
            const size_t words = (i % 4) ? sizeof(BandedHeader) / 8 : m.size();
            m[rnd() % words] ^= (int64_t)(1ull << (rnd() % 64));
            const int rc = plan_box(m.data(), p.bytes, p.pad, box, INT64_MAX, &ok, err);
            if (rc == L3C_OK && !ok) {
                fprintf(stderr, "region_plan_check: mutation %d: an inconsistent region plan was accepted\n", i);
                return 1;
            }
            if (rc != L3C_OK && rc != L3C_ERR_INVALID_ARG && rc != L3C_ERR_UNSUPPORTED) {
                fprintf(stderr, "region_plan_check: mutation %d: status %d\n", i, rc);
                return 1;
            }
            ++(rc == L3C_OK ? accepted : refused);
        }
    }
    printf("region_plan_check: plan blob mutations: %d planned, %d refused\n", accepted, refused);

    // 3. extreme boxes, and mutated region blobs
    const int ext[] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 327, 328, 329, INT32_MAX - 1, INT32_MAX};
    const Planned &p = plans[1];
    const int h_img = p.H - p.pad[2] - p.pad[3], w_img = W - p.pad[0] - p.pad[1];
    int extreme = 0;
    for (int a : ext)
        for (int b : ext)
            for (int c : ext)
                for (int d : {INT32_MIN, 0, w_img, INT32_MAX}) {
                    const l3c_region_box box = {a, b, c, d};
                    const bool inside = 0 <= a && a < b && b <= h_img && 0 <= c && c < d && d <= w_img;
                    bool ok;
                    const int rc = plan_box(p.blob, p.bytes, p.pad, box, (int64_t)p.file.size(), &ok, err);
                    if (inside ? (rc != L3C_OK || !ok) : rc != L3C_ERR_INVALID_ARG) {
                        fprintf(stderr, "region_plan_check: box (%d, %d, %d, %d): status %d, %s\n", a, b, c, d, rc, err);
                        return 1;
                    }
                    ++extreme;
                }
    {
        const l3c_region_box box = {100, 140, 5, 60};
        const int64_t cap = region_plan_bytes(&CFG, p.blob, err, 512);
        std::vector<int64_t> region((size_t)cap / 8);
        l3c_region_info info;
        if (make_region_plan(&CFG, p.blob, p.bytes, p.pad, &box, region.data(), cap, &info, err, 512) != L3C_OK) return 1;
        RegionHeader h;
        memcpy(&h, region.data(), sizeof(h));
        int same = 0, caught = 0;
        for (int i = 0; i < 5000; ++i) {
            int64_t *m = static_cast<int64_t *>(malloc((size_t)h.bytes));
            memcpy(m, region.data(), (size_t)h.bytes);
            m[rnd() % ((i % 2) ? sizeof(RegionHeader) / 8 : (size_t)h.bytes / 8)] ^= (int64_t)(1ull << (rnd() % 64));
            RegionHeader g;
            const int rc = region_check(CFG, p.blob, p.bytes, m, h.bytes, &g, err, 512);
            // what may pass: a flip in the padding between two arrays, and one that makes the blob of ANOTHER box or padding tuple that happens
            // to need the same words (the right or bottom padding only bounds the box) -- a blob the planner would have written, then
            if (rc == L3C_OK) {
                l3c_region_info mi;
                region_info(g, &mi);
                if (!consistent(m, h.bytes, mi, (int64_t)p.file.size())) {
                    fprintf(stderr, "region_plan_check: region blob mutation %d was accepted and is inconsistent\n", i);
                    return 1;
                }
            }
            ++(rc == L3C_OK ? same : caught);
            free(m);
        }
        printf("region_plan_check: %d extreme boxes answered; region blob mutations: %d caught, %d harmless\n", extreme, caught, same);
    }
    for (Planned &q : plans) free(q.blob);
    return 0;
}
