// The decode planner of BANDED files (l3c-pytorch_amd/csrc/codec_plan_banded.h: plain C++17, no HIP) on broken input, as a stand-alone
// program meant to be built with the address and undefined-behaviour sanitizers (the sibling of plan_check_main.cpp):
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/cabi/plan_banded_check_main.cpp -o plan_banded_check
//   plan_banded_check FILE.l3c [num_scales Cf C L K enc_blocks dec_blocks rgb_baseline dec_skip]        (default: configs/ms/cr.cf)
//
// It plans the file itself (must succeed), every truncation of it (must be refused) and 10 000 seeded single-byte mutations (either
// answer, but a plan that is accepted must be consistent with the file's size and with its own records).  Every buffer is heap memory of exactly the size the
// planner is told, so a read or write past an end is a sanitizer report.  Exit status 0: nothing to report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../l3c-pytorch_amd/csrc/codec_plan_banded.h"

static bool consistent(const l3c_plan::BandedHeader &h, const int64_t *blob, size_t n);

static int plan(const l3c_net_config &cfg, const std::vector<uint8_t> &bytes, size_t n, l3c_plan::BandedHeader *h, char *err, bool *ok) {
    uint8_t *file = static_cast<uint8_t *>(malloc(n ? n : 1));      // exactly n bytes: the planner must not read past them
    if (n) memcpy(file, bytes.data(), n);
    const int64_t offs[2] = {0, (int64_t)n};
    const int64_t cap = l3c_plan::plan_banded_bytes(&cfg, file, offs, 1, err, 512);
    if (cap < 0) {
        free(file);
        return (int)cap;
    }
    int64_t *blob = static_cast<int64_t *>(malloc((size_t)cap));    // exactly the size the sizing walk gave: the planner must not write past it
    int H = 0, W = 0;
    uint16_t padding[4];
    int rc = l3c_plan::make_plan_banded(&cfg, file, offs, 1, blob, cap, &H, &W, padding, err, 512);
    if (rc == L3C_OK) rc = l3c_plan::check_blob_banded(cfg, blob, cap, h, err, 512);      // what l3c_decode_batch_banded checks of it
    *ok = rc == L3C_OK && consistent(*h, blob, n);
    free(blob);
    free(file);
    return rc;
}

// every stream inside the file, every slot inside the stream buffer, every entry inside its image
static bool consistent(const l3c_plan::BandedHeader &h, const int64_t *blob, size_t n) {
    if (h.magic != l3c_plan::BANDED_MAGIC || h.files_bytes != (int64_t)n || h.dst_bytes > (int64_t)n + 8 * h.n_streams || h.H < 1 || h.W < 1 ||
        h.rgb_chunks < 1 || h.rgb_chunks > l3c_plan::RGB_BAND_CHUNKS)
        return false;
    const char *base = reinterpret_cast<const char *>(blob);
    const int64_t *src = reinterpret_cast<const int64_t *>(base + h.src_off), *dst = reinterpret_cast<const int64_t *>(base + h.dst_off);
    const uint32_t *nb = reinterpret_cast<const uint32_t *>(base + h.nbytes_off);
    for (int64_t s = 0; s < h.n_streams; ++s)
        if (src[s] < 14 || src[s] + (int64_t)nb[s] > (int64_t)n || dst[s] < 0 || dst[s] % 4 || dst[s] + (int64_t)nb[s] + 4 > h.dst_bytes) return false;
    for (int k = 1; k < (int)h.n_records - 1; ++k) {
        const l3c_plan::BandedRecord &r = h.rec[k];
        const int64_t E = h.B * r.n, HW = r.H * r.W;
        const int64_t *e = reinterpret_cast<const int64_t *>(base + h.entries_off[k]);
        for (int64_t i = 0; i < E; ++i)
            if (e[i] < 0 || e[i] + HW > h.B * HW || e[E + i] != HW || e[2 * E + i] < 0 || e[3 * E + i] < 1 || e[2 * E + i] + e[3 * E + i] > HW ||
                e[4 * E + i] != (e[i] + e[2 * E + i]) * (h.cfg[3] + 1) * 2)
                return false;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2 && argc != 11) {
        fprintf(stderr, "usage: plan_banded_check FILE.l3c [num_scales Cf C L K enc_blocks dec_blocks rgb_baseline dec_skip]\n");
        return 2;
    }
    l3c_net_config cfg = {3, 64, 5, 25, 10, 8, 8, 0, 1};
    if (argc == 11) {
        int *fields[9] = {&cfg.num_scales, &cfg.Cf, &cfg.C, &cfg.L, &cfg.K, &cfg.enc_blocks, &cfg.dec_blocks, &cfg.rgb_baseline, &cfg.dec_skip};
        for (int i = 0; i < 9; ++i) *fields[i] = atoi(argv[2 + i]);
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "plan_banded_check: cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<uint8_t> bytes;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
    fclose(f);

    char err[512] = "";
    l3c_plan::BandedHeader h;
    bool ok = false;
    if (plan(cfg, bytes, bytes.size(), &h, err, &ok) != L3C_OK || !ok) {
        fprintf(stderr, "plan_banded_check: the file itself is refused: %s\n", err);
        return 1;
    }
    printf("plan_banded_check: %zu bytes, %lld x %lld, %lld band streams, %lld chunk(s) per RGB band\n", bytes.size(), (long long)h.H, (long long)h.W,
           (long long)h.n_streams, (long long)h.rgb_chunks);
    for (size_t n = 0; n < bytes.size(); ++n) {
        const int rc = plan(cfg, bytes, n, &h, err, &ok);
        if (rc != L3C_ERR_INVALID_ARG || strncmp(err, "invalid file", 12) != 0) {
            fprintf(stderr, "plan_banded_check: truncation at %zu: status %d, %s\n", n, rc, err);
            return 1;
        }
    }
    printf("plan_banded_check: %zu truncations refused\n", bytes.size());
    uint64_t state = 0x9E3779B97F4A7C15ull;      // seeded: the same 10 000 mutations every run
    int accepted = 0, refused = 0;
    for (int i = 0; i < 10000; ++i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const size_t at = (size_t)((state >> 33) % bytes.size());
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const uint8_t flip = (uint8_t)(1 + (state >> 33) % 255);
        std::vector<uint8_t> m = bytes;
        m[at] ^= flip;
        const int rc = plan(cfg, m, m.size(), &h, err, &ok);
        if (rc == L3C_OK) {
            if (!ok) {
                fprintf(stderr, "plan_banded_check: mutation %d (byte %zu ^ %u): an inconsistent plan was accepted\n", i, at, (unsigned)flip);
                return 1;
            }
            ++accepted;
        } else if (rc == L3C_ERR_INVALID_ARG || rc == L3C_ERR_UNSUPPORTED) {
            ++refused;
        } else {
            fprintf(stderr, "plan_banded_check: mutation %d: status %d\n", i, rc);
            return 1;
        }
    }
    printf("plan_banded_check: 10000 mutations: %d planned (payload bytes), %d refused\n", accepted, refused);
    return 0;
}
