// csrc/seal_parity_plan.h alone, as a program of its own (built with the address and undefined-behaviour sanitizers by
// tests/test_native_parity_abi.py): the plan of l3c_seal_append_parity over accepted geometries and over everything it must refuse.
//   1. for random record lists (1..8 records, C in 1..8, 1..1024 bands, G in 1..300, R in 1..4, head on and off, B in 1..40) the plan's parts
//      against an independent restatement: the section kind and its front, the words under the check word, the copy units and the places
//      of the head records in the length and CRC arrays, the meta bytes laid out back to back exactly as container._head_part joins them,
//      the workspace parts 16-byte aligned and disjoint, and tail_bound equal to the tail of a file whose every payload has the largest
//      length.  The shape and stride arrays live in heap blocks of exactly their size, so that a read past their end is a sanitizer report;
//   2. the refusals: every bad option, a null pointer, 9 records, a head part without a coarser record, C = 0, a finest record of 4
//      channels, L = 96, more than 1024 bands, G > 255 with R > 1, a negative stride, and the three 65535 limits with their messages.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../l3c-pytorch_amd/csrc/seal_parity_plan.h"

using namespace l3c_parity_seal;

static int fail(const char *what, long long a, long long b) {
    printf("seal_parity_plan_check: FAILED %s (%lld, %lld)\n", what, a, b);
    return 1;
}

static uint32_t next(uint32_t *s) {
    *s = *s * 1664525u + 1013904223u;
    return *s >> 8;
}

static int plan(const std::vector<Shape> &shapes, const std::vector<int64_t> &strides, int64_t B, int G, int R, int head, Plan *out, char *err) {
    Shape *s = static_cast<Shape *>(malloc(shapes.size() ? shapes.size() * sizeof(Shape) : 1));
    int64_t *t = static_cast<int64_t *>(malloc(strides.size() ? strides.size() * sizeof(int64_t) : 1));
    if (!shapes.empty()) memcpy(s, shapes.data(), shapes.size() * sizeof(Shape));
    if (!strides.empty()) memcpy(t, strides.data(), strides.size() * sizeof(int64_t));
    err[0] = 0;
    const int rc = make_plan(s, (int)shapes.size(), B, G, R, head, t, out, err, 256);
    free(s);
    free(t);
    return rc;
}

#define CHECK(cond, a, b) \
    do {                  \
        if (!(cond)) return fail(#cond, (long long)(a), (long long)(b)); \
    } while (0)

static int accepted(uint32_t *seed, long long *plans) {
    char err[256];
    for (int round = 0; round < 4000; ++round) {
        const int records = 1 + (int)(next(seed) % 8), R = 1 + (int)(next(seed) % 4), head = records > 1 && (next(seed) & 1);
        const int64_t B = 1 + next(seed) % 40;
        int G = 1 + (int)(next(seed) % 300);
        std::vector<Shape> shapes;
        std::vector<int64_t> strides;
        for (int k = 0; k < records; ++k) {
            const int64_t n = 1 + next(seed) % (next(seed) % 8 ? 24 : 1024), L = 64 * (1 + next(seed) % 3);
            const int64_t hw = (n - 1) * L + 1 + next(seed) % L;                  // exactly n bands
            int H = 1, W = (int)hw;
            for (int d = 2; d < 400 && W > 65535; ++d)
                while (W % d == 0 && W > 65535 && H * d <= 65535) W /= d, H *= d;
            if (W > 65535) H = 64, W = (int)(n * L / 64);                           // a last band of L symbols
            shapes.push_back(Shape{k + 1 == records ? 3 : 1 + (int)(next(seed) % 8), H, W, L});
            strides.push_back(16 * (int64_t)(1 + next(seed) % 600));
        }
        if (R > 1) {                                                                // keep min(G, n) <= 255 for the records that count
            for (int k = head ? 0 : records - 1; k < records; ++k) {
                const int64_t n = ((int64_t)shapes[k].H * shapes[k].W + shapes[k].L - 1) / shapes[k].L;
                if ((G < n ? G : n) > 255) G = 255;
            }
        }
        Plan p;
        const int rc = plan(shapes, strides, B, G, R, head, &p, err);
        // the limits, restated
        int64_t head_groups = 0, finest_groups = 0;
        for (int k = 0; k < records; ++k) {
            const int64_t n = ((int64_t)shapes[k].H * shapes[k].W + shapes[k].L - 1) / shapes[k].L, Gk = G < n ? G : n, m = (n + Gk - 1) / Gk;
            if (k + 1 == records) finest_groups = B * 3 * m;
            else if (head) head_groups += B * shapes[k].C * m;
        }
        if (finest_groups > 65535 || head_groups > 65535) {
            CHECK(rc == L3C_ERR_UNSUPPORTED && strstr(err, "slice the batch"), round, rc);
            continue;
        }
        CHECK(rc == L3C_OK, round, rc);
        ++*plans;
        const int first = head ? 0 : records - 1, fin = p.n_records - 1;
        CHECK(p.n_records == records - first && p.R == R && p.head == head, round, p.n_records);
        int64_t meta = 4 + 14, units = 0, lens = 0, crcs = 0, fields = 0, framing = 14, worst = 0, longest = 0;
        for (int k = 0; k <= fin; ++k) {
            const Shape &s = shapes[(size_t)(first + k)];
            const Record &r = p.rec[k];
            const int64_t n = ((int64_t)s.H * s.W + s.L - 1) / s.L, Gk = G < n ? G : n, m = (n + Gk - 1) / Gk;
            CHECK(r.C == s.C && r.H == s.H && r.W == s.W && r.L == s.L && r.n == n && r.G == Gk && r.m == m, round, k);
            CHECK(p.field_first[k] == fields, round, k);
            fields += s.C * n;
            if (head) {
                CHECK(p.meta_hdr_at[k] == meta, round, k);
                meta += 9 + 4 * s.C * n;
            }
            if (k < fin) {
                CHECK(p.unit_first[k] == units && p.len_first[k] == lens && p.crc_first[k] == crcs, round, k);
                units += s.C * m, lens += B * s.C * m, crcs += B * s.C * n;
                framing += 9 + 4 * s.C * n + 4;
                worst += s.C * m * R * strides[(size_t)(first + k)];
            }
            if (strides[(size_t)(first + k)] > longest) longest = strides[(size_t)(first + k)];
        }
        const Record &f = p.rec[fin];
        CHECK(p.fields == fields && p.field_first[p.n_records] == fields, round, fields);
        CHECK(p.plen_at == (R == 1 && !head ? 8 : 12) && p.front_bytes == p.plen_at + 12 * f.m && p.table_bytes == 20 + 12 * f.n, round, p.front_bytes);
        CHECK(p.check_words * 4 == 8 + p.front_bytes + 8 + p.table_bytes + 20, round, p.check_words);
        const char *sig = head ? "L3CH" : R == 1 ? "L3CP" : "L3CQ";
        CHECK(memcmp(&p.signature, sig, 4) == 0, round, p.signature);
        CHECK(p.finest_framing == 9 + 12 * f.n + 4, round, p.finest_framing);
        int64_t tail = p.front_bytes + 3 * (int64_t)f.m * R * strides[(size_t)(first + fin)] + 8 + p.table_bytes + 24;
        if (head) {
            CHECK(p.meta_head_crc_at == meta && p.unit_first[fin] == units && p.head_framing == framing, round, meta);
            meta += 4;
            for (int k = 0; k < fin; ++k) {
                CHECK(p.meta_crc_at[k] == meta, round, k);
                meta += 4 * p.rec[k].C * p.rec[k].n + 4 + 4 * p.rec[k].C * p.rec[k].m;
            }
            CHECK(p.meta_bytes == meta && p.units == 3 * f.m + 1 + units && p.meta_stride >= meta + 4 && p.meta_stride % 16 == 0, round, meta);
            tail += meta + worst + 4;
            if (meta > longest) longest = meta;
        } else {
            CHECK(p.units == 3 * f.m && p.meta_bytes == 0 && p.meta_stride == 0, round, p.units);
        }
        CHECK(p.longest == longest && copy_tiles(longest) * TILE_DWORDS * 4 >= longest + 7, round, longest);
        CHECK(tail_bound(p, strides.data() + first) == tail, round, tail);
        CHECK(p.ws_tail_at == 0 && p.ws_unit_off >= 8 * B && p.ws_meta >= p.ws_unit_off + 8 * B * p.units &&
                  p.ws_bytes == p.ws_meta + B * p.meta_stride && p.ws_unit_off % 16 == 0 && p.ws_meta % 16 == 0, round, p.ws_bytes);
    }
    return 0;
}

static int refused() {
    char err[256];
    Plan p;
    const std::vector<Shape> two = {Shape{5, 8, 16, 64}, Shape{3, 16, 32, 64}};
    const std::vector<int64_t> strides = {160, 160};
    CHECK(plan(two, strides, 2, 4, 2, 1, &p, err) == L3C_OK, 0, 0);
    const int opts[][4] = {{0, 1, 0, 0}, {-3, 1, 0, 0}, {4, 0, 0, 0}, {4, 5, 0, 0}, {4, 1, 2, 0}, {4, 1, -1, 0}, {4, 1, 0, 1}};
    for (const auto &o : opts) CHECK(check_opts(o[0], o[1], o[2], o[3], err, 256) == L3C_ERR_INVALID_ARG && strstr(err, "parity"), o[0], o[1]);
    CHECK(check_opts(1, 1, 0, 0, err, 256) == L3C_OK && check_opts(1 << 30, 4, 1, 0, err, 256) == L3C_OK, 0, 0);
    CHECK(plan(two, strides, 2, 0, 1, 0, &p, err) == L3C_ERR_INVALID_ARG && plan(two, strides, 2, 4, 5, 0, &p, err) == L3C_ERR_INVALID_ARG, 1, 0);
    CHECK(make_plan(nullptr, 2, 2, 4, 1, 0, strides.data(), &p, err, 256) == L3C_ERR_INVALID_ARG && strstr(err, "null"), 2, 0);
    CHECK(make_plan(two.data(), 2, 2, 4, 1, 0, nullptr, &p, err, 256) == L3C_ERR_INVALID_ARG, 2, 1);
    CHECK(make_plan(two.data(), 2, 2, 4, 1, 0, strides.data(), nullptr, err, 256) == L3C_ERR_INVALID_ARG, 2, 2);
    CHECK(make_plan(two.data(), 2, 2, 4, 1, 0, strides.data(), &p, nullptr, 0) == L3C_OK, 2, 3);
    CHECK(plan({}, {}, 2, 4, 1, 0, &p, err) == L3C_ERR_INVALID_ARG, 3, 0);
    CHECK(plan(std::vector<Shape>(9, two[1]), std::vector<int64_t>(9, 160), 1, 4, 1, 0, &p, err) == L3C_ERR_UNSUPPORTED && strstr(err, "8 scale records"), 3, 1);
    CHECK(plan({two[1]}, {160}, 2, 4, 1, 1, &p, err) == L3C_ERR_INVALID_ARG && strstr(err, "head"), 4, 0);
    CHECK(plan({two[1]}, {160}, 2, 4, 1, 0, &p, err) == L3C_OK && p.n_records == 1, 4, 1);
    for (int64_t B : {(int64_t)0, (int64_t)-1, (int64_t)65536}) CHECK(plan(two, strides, B, 4, 1, 1, &p, err) == L3C_ERR_INVALID_ARG && strstr(err, "batch"), 5, B);
    CHECK(plan({Shape{0, 8, 16, 64}, two[1]}, strides, 2, 4, 1, 1, &p, err) == L3C_ERR_INVALID_ARG && strstr(err, "shape"), 6, 0);
    CHECK(plan({Shape{0, 8, 16, 64}, two[1]}, strides, 2, 4, 1, 0, &p, err) == L3C_OK, 6, 1);       // without a head part the coarser records are not read
    CHECK(plan({two[0], Shape{3, 70000, 1, 64}}, strides, 2, 4, 1, 0, &p, err) == L3C_ERR_INVALID_ARG && strstr(err, "u16"), 6, 2);
    CHECK(plan({two[0], Shape{4, 16, 32, 64}}, strides, 2, 4, 1, 0, &p, err) == L3C_ERR_INVALID_ARG && strstr(err, "3 channels"), 7, 0);
    for (int64_t L : {(int64_t)0, (int64_t)96, (int64_t)-64, (int64_t)1 << 32})
        CHECK(plan({two[0], Shape{3, 16, 32, L}}, strides, 2, 4, 1, 0, &p, err) == L3C_ERR_INVALID_ARG && strstr(err, "multiple of 64"), 8, L);
    CHECK(plan({two[0], Shape{3, 1025, 64, 64}}, strides, 1, 4, 1, 0, &p, err) == L3C_ERR_INVALID_ARG && strstr(err, "1024 bands"), 9, 0);
    CHECK(plan({two[0], Shape{3, 1024, 64, 64}}, strides, 1, 256, 2, 0, &p, err) == L3C_ERR_INVALID_ARG && strstr(err, "255"), 10, 0);
    CHECK(plan({two[0], Shape{3, 1024, 64, 64}}, strides, 1, 256, 1, 0, &p, err) == L3C_OK && p.rec[0].G == 256 && p.rec[0].m == 4, 10, 1);
    CHECK(plan({two[0], Shape{3, 1024, 64, 64}}, strides, 1, 255, 4, 0, &p, err) == L3C_OK && p.rec[0].m == 5, 10, 2);
    CHECK(plan({two[0], Shape{3, 16, 64, 64}}, strides, 1, 300, 4, 1, &p, err) == L3C_OK && p.rec[1].G == 16 && p.rec[0].G == 2, 10, 3);      // G clamps to n
    CHECK(plan(two, {160, -16}, 2, 4, 1, 0, &p, err) == L3C_ERR_INVALID_ARG && strstr(err, "stride"), 11, 0);
    // B * 3 * m: 1024 bands in groups of 1 are 3072 groups a file
    CHECK(plan({two[0], Shape{3, 1024, 64, 64}}, strides, 21, 1, 1, 0, &p, err) == L3C_OK, 12, 0);
    CHECK(plan({two[0], Shape{3, 1024, 64, 64}}, strides, 22, 1, 1, 0, &p, err) == L3C_ERR_UNSUPPORTED && strstr(err, "slice the batch"), 12, 1);
    // the head sum: 8 channels of 1024 bands are 8192 groups a file
    CHECK(plan({Shape{8, 1024, 64, 64}, two[1]}, strides, 7, 1, 1, 1, &p, err) == L3C_OK, 13, 0);
    CHECK(plan({Shape{8, 1024, 64, 64}, two[1]}, strides, 8, 1, 1, 1, &p, err) == L3C_ERR_UNSUPPORTED && strstr(err, "slice the batch"), 13, 1);
    CHECK(plan({Shape{8, 1024, 64, 64}, two[1]}, strides, 8, 1, 1, 0, &p, err) == L3C_OK, 13, 2);
    return 0;
}

int main() {
    uint32_t seed = 25;
    long long plans = 0;
    if (accepted(&seed, &plans) || refused()) return 1;
    printf("seal_parity_plan_check: %lld plans checked\n", plans);
    printf("seal_parity_plan_check: refusals checked\n");
    return 0;
}
