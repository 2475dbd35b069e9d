// The repair planner (l3c-pytorch_amd/csrc/repair_plan.h and seal.h: plain C++17, no HIP) as a stand-alone program meant to be built with the
// address and undefined-behaviour sanitizers (the sibling of region_plan_check_main.cpp):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/cabi/repair_plan_check_main.cpp -o repair_plan_check
//   repair_plan_check
//
// It frames a banded file of a 328 x 88 image itself (K = 16), seals it with a parity section of R = 1..4 rows (l3c_sealing::write_parity_rs;
// the planner reads no payload byte), plans the body, and
//   1. plans rounds over random damage until nothing is left to try, and checks every blob: round_check accepts it, every row span lies
//      inside the section where the caller put it, every member span and slot inside the stream area, every entry inside its frame;
//   2. feeds the planner TRUNCATED files (either answer, no report);
//   3. feeds it files with a bit of the SECTION's head, the table or the seal flipped (either answer; an accepted plan passes the invariants);
//   4. feeds it SHORT blobs (refused), and round_check bit-flipped ROUND blobs (refused, or byte for byte the blob its groups imply).
// Every buffer is heap memory of exactly the size the planner is told, so a read or write past an end is a sanitizer report.  Exit status
// 0: nothing to report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../l3c-pytorch_amd/csrc/parity_plan.h"
#include "../../l3c-pytorch_amd/csrc/repair_plan.h"

using namespace l3c_repair;

static const l3c_net_config CFG = {3, 64, 5, 25, 10, 8, 8, 0, 1};      // configs/ms/cr.cf
static const int H = 328, W = 88, K = 16;

static void put16(std::vector<uint8_t> &f, unsigned v) { f.push_back(v & 255); f.push_back(v >> 8 & 255); }
static void put32(std::vector<uint8_t> &f, unsigned v) { put16(f, v & 65535); put16(f, v >> 16); }

static unsigned rnd() {
    static uint64_t s = 0x9E3779B97F4A7C15ull;
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (unsigned)(s >> 32);
}

// bitcoding/container.py: write_file(banded=True), payloads of a few bytes; the finest record's lengths go to lens[3][n]
static std::vector<uint8_t> banded_body(std::vector<uint32_t> *lens, int64_t *n_out, uint32_t *L_out) {
    std::vector<uint8_t> f = {'L', '3', 'C', 'B', 1, 0};
    for (int i = 0; i < 4; ++i) put16(f, 0);
    for (int s = CFG.num_scales; s >= 0; --s) {
        const int C = s ? CFG.C : 3, h = H >> s, w = W >> s;
        const int64_t hw = (int64_t)h * w, L = 64 * ((hw + 64 * K - 1) / (64 * K)), n = (hw + L - 1) / L;
        f.push_back((uint8_t)C);
        put16(f, h);
        put16(f, w);
        put32(f, (unsigned)L);
        for (int c = 0; c < C; ++c)
            for (int64_t j = 0; j < n; ++j) {
                const unsigned nb = (unsigned)((j * 7 + c * 3 + s) % 23);
                put32(f, nb);
                for (unsigned i = 0; i < nb; ++i) f.push_back((uint8_t)(i + j));
                if (s == 0) lens->push_back(nb);
            }
        const uint8_t sep[4] = {0x46, 0xE2, 0x84, 0x92};
        f.insert(f.end(), sep, sep + 4);
        if (s == 0) *n_out = n, *L_out = (uint32_t)L;
    }
    return f;
}

struct Sealed {
    uint8_t *file;              // exactly `bytes` bytes of heap
    int64_t bytes, body, n;
    int m, R;
    std::vector<uint32_t> table;    // [3][n]
};

static Sealed seal_file(int G, int R) {
    std::vector<uint32_t> lens;
    Sealed s{};
    uint32_t L = 0;
    const std::vector<uint8_t> body = banded_body(&lens, &s.n, &L);
    const int n = (int)s.n, m = (n + G - 1) / G;
    s.m = m, s.R = R, s.body = (int64_t)body.size();
    std::vector<uint32_t> plen(3 * m, 0);
    for (int c = 0; c < 3; ++c)
        for (int j = 0; j < n; ++j)
            if (lens[c * n + j] > plen[c * m + j % m]) plen[c * m + j % m] = lens[c * n + j];
    int64_t sum = 0;
    for (uint32_t v : plen) sum += v;
    std::vector<uint8_t> payloads((size_t)(R * sum) + 1);
    for (auto &v : payloads) v = (uint8_t)rnd();
    s.table.resize(3 * n);
    for (auto &v : s.table) v = rnd();
    std::vector<uint8_t> crc(12 * n);
    for (int i = 0; i < 3 * n; ++i) l3c_sealing::put(crc.data() + 4 * i, s.table[i], 4);
    const l3c_seal seal{7, l3c_sealing::combine_bands(crc.data(), n, L, (int64_t)H * W), 0x1122334455667788ull};
    const int64_t tail = l3c_sealing::parity_section_bytes(m, R, sum) + l3c_sealing::table_bytes(n) + L3C_SEAL_BYTES;
    s.bytes = s.body + tail;
    s.file = static_cast<uint8_t *>(malloc((size_t)s.bytes));
    memcpy(s.file, body.data(), body.size());
    l3c_sealing::write_parity_rs(seal, s.file + 6, crc.data(), n, L, G, m, R, plen.data(), payloads.data(), s.file + s.body);
    return s;
}

struct Planned {
    int64_t *blob;
    int64_t bytes;
    l3c_plan::BandedHeader h;
};

static bool plan_body(const Sealed &s, Planned *out, char *err) {
    const int64_t offs[2] = {0, s.body};
    out->bytes = l3c_plan::plan_banded_bytes(&CFG, s.file, offs, 1, err, 512);
    if (out->bytes < 0) return false;
    out->blob = static_cast<int64_t *>(malloc((size_t)out->bytes));
    int h = 0, w = 0;
    if (l3c_plan::make_plan_banded(&CFG, s.file, offs, 1, out->blob, out->bytes, &h, &w, nullptr, err, 512) != L3C_OK) return false;
    return l3c_plan::check_blob_banded(CFG, out->blob, out->bytes, &out->h, err, 512) == L3C_OK;
}

// the invariants of an accepted round blob of exactly `bytes` bytes: round_check makes it again, and nothing it names leaves its buffer
static bool consistent(const Planned &p, const void *round, int64_t bytes, int64_t section_at, int64_t section_bytes, char *err) {
    RoundHeader h;
    uint8_t *scratch = static_cast<uint8_t *>(malloc((size_t)bytes));
    const int rc = round_check(CFG, p.h, p.blob, round, bytes, &h, scratch, bytes, err, 512);
    free(scratch);
    if (rc != L3C_OK || h.bytes != bytes) return false;
    const uint8_t *b = static_cast<const uint8_t *>(round);
    const l3c_rebuild_group *rb = reinterpret_cast<const l3c_rebuild_group *>(b + h.rebuild_off);
    const l3c_u8_span *src = reinterpret_cast<const l3c_u8_span *>(b + h.src_off);
    for (int64_t q = 0; q < h.n_groups; ++q) {
        if (rb[q].first_src < 0 || rb[q].first_src + rb[q].n_rows + rb[q].n_members > h.n_src || rb[q].t < 1 || rb[q].t > 4 || rb[q].n_rows != rb[q].t) return false;
        for (int64_t k = rb[q].first_src; k < rb[q].first_src + rb[q].n_rows + rb[q].n_members; ++k) {
            const bool row = k < rb[q].first_src + rb[q].n_rows;
            if (src[k].offset < 0 || src[k].bytes < 0) return false;
            if (row && (src[k].offset < section_at || src[k].offset + src[k].bytes > section_at + section_bytes)) return false;
            if (!row && (src[k].offset % 4 || src[k].offset + (src[k].bytes + 3) / 4 * 4 > h.dst_bytes)) return false;
        }
        for (int e = 0; e < rb[q].t; ++e)
            if (rb[q].out[e].offset < 0 || rb[q].out[e].offset % 4 || rb[q].out[e].offset + (rb[q].out[e].bytes + 3) / 4 * 4 + 4 > h.dst_bytes) return false;
    }
    const int64_t *e = reinterpret_cast<const int64_t *>(b + h.entries_off);
    for (int64_t i = 0; i < h.S; ++i)
        if (e[i] < 0 || e[i] + e[h.S + i] > h.B * h.HW || e[2 * h.S + i] < 0 || e[3 * h.S + i] < 1 || e[2 * h.S + i] + e[3 * h.S + i] > e[h.S + i]) return false;
    return h.n_chunks >= 1 && h.n_chunks <= 8 && (h.lag == 1 || h.lag == 2);
}

// one planner call on heap buffers of exact sizes -> the status; *blob_out (to free) and *bytes_out where it succeeded
static int plan_round(const Planned &p, const uint8_t *file, int64_t file_bytes, const std::vector<uint32_t> &words, int64_t section_at,
                      const std::vector<l3c_repair_group> &tried, int64_t cap, uint8_t **blob_out, int64_t *bytes_out, char *err) {
    uint8_t *copy = static_cast<uint8_t *>(malloc(file_bytes > 0 ? (size_t)file_bytes : 1));
    if (file_bytes > 0) memcpy(copy, file, (size_t)file_bytes);
    uint8_t *blob = static_cast<uint8_t *>(malloc(cap > 0 ? (size_t)cap : 1));
    const uint8_t *files[1] = {copy};
    const int rc = make_round_plan(&CFG, p.blob, files, &file_bytes, words.data(), &section_at, tried.empty() ? nullptr : tried.data(), (int64_t)tried.size(),
                                   blob, cap, err, 512);
    free(copy);
    *blob_out = nullptr;
    if (rc == L3C_OK) {
        RoundHeader h;
        memcpy(&h, blob, sizeof(h));
        *bytes_out = h.bytes;
        *blob_out = static_cast<uint8_t *>(malloc((size_t)h.bytes));      // exactly its size: what round_check is told
        memcpy(*blob_out, blob, (size_t)h.bytes);
    }
    free(blob);
    return rc;
}

int main() {
    char err[512] = "";
    int64_t rounds = 0, truncated = 0, flipped = 0, flipped_ok = 0, blobs = 0, blobs_ok = 0;
    for (int R = 1; R <= 4; ++R) {
        const int G = R == 1 ? 4 : (R == 2 ? 3 : 16);
        Sealed s = seal_file(G, R);
        Planned p;
        if (!plan_body(s, &p, err)) return printf("FAIL: plan: %s\n", err), 1;
        const int64_t cap = round_bytes_bound(p.h), section_at = 48, section_bytes = s.bytes - s.body;
        // 1. rounds over random damage, until nothing is left to try
        for (int trial = 0; trial < 40; ++trial) {
            std::vector<uint32_t> words = s.table;
            for (unsigned k = rnd() % 7; k > 0; --k) words[rnd() % words.size()] ^= 1 + rnd() % 255;
            std::vector<l3c_repair_group> tried;
            for (int round = 0;; ++round) {
                uint8_t *blob;
                int64_t bytes;
                if (plan_round(p, s.file, s.bytes, words, section_at, tried, cap, &blob, &bytes, err) != L3C_OK) return printf("FAIL: round: %s\n", err), 1;
                if (!consistent(p, blob, bytes, section_at, section_bytes, err)) return printf("FAIL: an inconsistent round blob (R %d trial %d): %s\n", R, trial, err), 1;
                RoundHeader h;
                memcpy(&h, blob, sizeof(h));
                const l3c_repair_group *g = reinterpret_cast<const l3c_repair_group *>(blob + h.groups_off);
                tried.insert(tried.end(), g, g + h.n_groups);
                // 4. a short blob is refused; a bit-flipped one is refused or is the blob its groups imply
                if (h.n_groups && trial % 8 == 0) {
                    uint8_t *none;
                    int64_t nb;
                    for (int64_t c2 = 0; c2 < bytes; c2 += 24)
                        if (plan_round(p, s.file, s.bytes, words, section_at, std::vector<l3c_repair_group>(tried.begin(), tried.end() - h.n_groups), c2, &none, &nb, err) == L3C_OK)
                            return printf("FAIL: a blob of %lld bytes planned into %lld\n", (long long)bytes, (long long)c2), 1;
                    for (int64_t bit = 0; bit < 8 * bytes; bit += 1 + rnd() % 5) {
                        blob[bit / 8] ^= (uint8_t)(1 << (bit % 8));
                        RoundHeader hh;
                        uint8_t *scratch = static_cast<uint8_t *>(malloc((size_t)bytes));
                        ++blobs;
                        if (round_check(CFG, p.h, p.blob, blob, bytes, &hh, scratch, bytes, err, 512) == L3C_OK) {
                            ++blobs_ok;                                    // a padding byte, or a row span: those l3c_band_rebuild's table check bounds
                            const int64_t n_iv = l3c_parity::rebuild_intervals(reinterpret_cast<const l3c_rebuild_group *>(blob + hh.rebuild_off), hh.n_groups);
                            if (n_iv < 0) return printf("FAIL: an accepted blob whose rebuild table cannot be counted\n"), 1;
                            l3c_parity::RebuildInterval *iv = static_cast<l3c_parity::RebuildInterval *>(malloc((size_t)n_iv * sizeof(l3c_parity::RebuildInterval)));
                            const int64_t tiles = l3c_parity::check_rebuild(reinterpret_cast<const l3c_u8_span *>(blob + hh.src_off), hh.n_src,
                                                                            reinterpret_cast<const l3c_rebuild_group *>(blob + hh.rebuild_off), hh.n_groups,
                                                                            section_at + section_bytes, hh.dst_bytes, iv, err, 512);
                            free(iv);
                            if (tiles < 0 && bit / 8 < hh.src_off) return printf("FAIL: an accepted blob that the rebuild check refuses: %s\n", err), 1;
                        }
                        free(scratch);
                        blob[bit / 8] ^= (uint8_t)(1 << (bit % 8));
                    }
                }
                free(blob);
                ++rounds;
                if (h.n_groups == 0) break;
                if (round > 16) return printf("FAIL: rounds do not end\n"), 1;
            }
        }
        // 2. truncated files, 3. a bit of the tail flipped
        std::vector<uint32_t> words = s.table;
        words[5] ^= 1, words[s.n + 2] ^= 7;
        const std::vector<l3c_repair_group> none;
        for (int64_t cut = 0; cut < s.bytes; cut += (cut < s.body ? 97 : 1)) {
            uint8_t *blob;
            int64_t bytes;
            if (plan_round(p, s.file, cut, words, section_at, none, cap, &blob, &bytes, err) == L3C_OK) {
                if (!consistent(p, blob, bytes, section_at, section_bytes, err)) return printf("FAIL: a truncated file planned inconsistently\n"), 1;
                free(blob);
            }
            ++truncated;
        }
        const int64_t head = l3c_sealing::section_head_bytes(R) + 12 * s.m;
        for (int64_t bit = 0; bit < 8 * (s.bytes - s.body); ++bit) {
            const int64_t at = bit / 8;
            if (at >= head && at < section_bytes - l3c_sealing::table_bytes(s.n) - L3C_SEAL_BYTES - 8 && bit % 64) continue;      // (the payloads: one bit in 64)
            s.file[s.body + at] ^= (uint8_t)(1 << (bit % 8));
            uint8_t *blob;
            int64_t bytes;
            ++flipped;
            if (plan_round(p, s.file, s.bytes, words, section_at, none, cap, &blob, &bytes, err) == L3C_OK) {
                ++flipped_ok;
                if (!consistent(p, blob, bytes, section_at, section_bytes, err)) return printf("FAIL: a flipped file planned inconsistently\n"), 1;
                free(blob);
            }
            s.file[s.body + at] ^= (uint8_t)(1 << (bit % 8));
        }
        free(p.blob);
        free(s.file);
    }
    printf("repair_plan_check: %lld rounds planned and checked\n", (long long)rounds);
    printf("repair_plan_check: %lld truncated files answered\n", (long long)truncated);
    printf("repair_plan_check: file mutations: %lld answered, %lld still planned\n", (long long)flipped, (long long)flipped_ok);
    printf("repair_plan_check: round blob mutations: %lld answered, %lld still the blob their groups imply\n", (long long)blobs, (long long)blobs_ok);
    return 0;
}
