// csrc/seal.h alone, as a program of its own (built with the address and undefined-behaviour sanitizers by tests/test_head_parity_format.py):
// the seal reader on files whose PARITY SECTION is of the 'L3CH' kind (a head part behind the finest record's rows).  argv[1]: the cases of the
// Python test, [u32 size | bytes] records back to back, the first of them an intact file.  Every file is copied into a heap block of exactly
// its size, so that a read past its end is a sanitizer report.
// Per case one line, which the test compares with container.split_seal's answer:  "1 <body bytes> <has a head section> <head_check holds>",
// "0 <file bytes> 0 0" for an unsealed file, "-1 <message>" for a refused one -- find, find_bands, find_parity, find_parity_rs and find_head
// must agree on it.  Then every truncation and a single-byte change at every position of the first case: each call returns 1, 0 or
// L3C_ERR_INVALID_ARG, what it hands out lies inside the file, and a changed byte of the HEAD PART never makes the file unreadable.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../l3c-pytorch_amd/csrc/seal.h"

static volatile uint32_t sink;      // keeps the reads of what was handed out

struct Answer {
    int rc;
    int64_t body;
    l3c_sealing::HeadAt head;
    char err[256];
};

// every reader on an exactly sized copy -> 0 when they agree and what they hand out lies inside the file
static int probe(const uint8_t *file, int64_t n, Answer *a) {
    uint8_t *exact = static_cast<uint8_t *>(malloc(n ? n : 1));
    memcpy(exact, file, n);
    char err2[256];
    int bad = 0;
    l3c_seal seal = {0, 0, 0};
    l3c_seal_bands bands = {-1, 0, nullptr};
    l3c_seal_parity_rs par = {-1, -1, -1, nullptr, nullptr, -1};
    l3c_seal_parity old = {-1, -1, nullptr, nullptr, -1};
    a->err[0] = 0, a->body = -1;
    a->rc = l3c_sealing::find_parity_rs(exact, n, &a->body, &seal, &bands, &par, a->err, sizeof a->err);
    if (a->rc != 1 && a->rc != 0 && a->rc != L3C_ERR_INVALID_ARG) bad = 1;
    if (a->rc == L3C_ERR_INVALID_ARG && strncmp(a->err, "invalid file: seal ", 19) != 0) bad = 1;
    for (int which = 0; which < 4; ++which) {
        int64_t body2 = -1;
        err2[0] = 0;
        int rc2;
        if (which == 0) rc2 = l3c_sealing::find(exact, n, &body2, nullptr, err2, sizeof err2);
        else if (which == 1) rc2 = l3c_sealing::find_bands(exact, n, &body2, nullptr, nullptr, err2, sizeof err2);
        else if (which == 2) rc2 = l3c_sealing::find_parity(exact, n, &body2, nullptr, nullptr, &old, err2, sizeof err2);
        else rc2 = l3c_sealing::find_tail(exact, n, &body2, nullptr, nullptr, nullptr, &a->head, err2, sizeof err2);
        if (rc2 != a->rc || body2 != a->body || strcmp(a->err, err2) != 0) bad = 1;
    }
    l3c_sealing::HeadAt head2;
    const int rch = l3c_sealing::find_head(exact, n, &head2, err2, sizeof err2);
    if (rch != (a->rc == 1 ? (a->head.at != 0) : a->rc) || head2.at != a->head.at || head2.bytes != a->head.bytes || head2.check_ok != a->head.check_ok)
        bad = 1;
    if (a->rc == 1 && !bad) {
        uint32_t x = 0;
        if (a->body < 0 || a->body > n - L3C_SEAL_BYTES) bad = 1;
        if (a->head.at) {
            if (old.m != 0 || par.m < 1 || par.R < 1 || par.R > 4) bad = 1;                     // reads as a band-sealed file where 'L3CP' alone is known
            if (!bad && (par.plen != exact + a->body + 12 || par.payloads != par.plen + 12 * par.m)) bad = 1;
            if (!bad && (a->head.at != (par.payloads - exact) + par.payload_bytes || a->head.bytes < 0 ||
                         exact + a->head.at + a->head.bytes + 8 != bands.crc - 12))
                bad = 1;
            for (int64_t i = 0; i < a->head.bytes && !bad; ++i) x ^= exact[a->head.at + i];      // the head part can be read
            if (a->head.check_ok && (a->head.n_records < 2 || a->head.n_records > l3c_sealing::MAX_HEAD_RECORDS)) bad = 1;
        }
        for (int64_t i = 0; par.m > 0 && i < par.payload_bytes && !bad; ++i) x ^= par.payloads[i];
        sink = x;
    }
    free(exact);
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) return printf("usage: head_seal_check CASES\n"), 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return printf("head_seal_check: cannot open %s\n", argv[1]), 2;
    std::vector<std::vector<uint8_t>> cases;
    for (;;) {
        uint8_t size4[4];
        if (fread(size4, 1, 4, fp) != 4) break;
        std::vector<uint8_t> f((size_t)l3c_sealing::get(size4, 4));
        if (!f.empty() && fread(f.data(), 1, f.size(), fp) != f.size()) return printf("head_seal_check: a short case\n"), 2;
        cases.push_back(f);
    }
    fclose(fp);
    if (cases.empty()) return printf("head_seal_check: no cases\n"), 2;
    Answer a;
    for (size_t i = 0; i < cases.size(); ++i) {
        if (probe(cases[i].data(), (int64_t)cases[i].size(), &a)) return printf("head_seal_check: FAILED case %d\n", (int)i), 1;
        if (a.rc == L3C_ERR_INVALID_ARG) printf("-1 %s\n", a.err);
        else printf("%d %lld %d %d\n", a.rc, (long long)a.body, a.head.at != 0, a.head.check_ok);
    }
    std::vector<uint8_t> f = cases[0];
    const int64_t n = (int64_t)f.size();
    if (probe(f.data(), n, &a) || a.rc != 1 || !a.head.at || !a.head.check_ok) return printf("head_seal_check: FAILED, the first case must be intact\n"), 1;
    const int64_t head_at = a.head.at, head_end = a.head.at + a.head.bytes;
    long long truncations = 0, changes = 0, in_head = 0;
    for (int64_t k = 0; k < n; ++k, ++truncations)
        if (probe(f.data(), k, &a) || a.rc == 1) return printf("head_seal_check: FAILED truncation to %lld\n", (long long)k), 1;
    for (int64_t at = 0; at < n; ++at, ++changes) {
        f[at] ^= 0xff;
        if (probe(f.data(), n, &a)) return printf("head_seal_check: FAILED change at %lld\n", (long long)at), 1;
        if (at >= head_at && at < head_end) {
            ++in_head;
            if (a.rc != 1 || !a.head.at) return printf("head_seal_check: FAILED, a changed head byte at %lld made the file unreadable\n", (long long)at), 1;
        }
        f[at] ^= 0xff;
    }
    printf("head_seal_check: %lld truncations, %lld single-byte changes (%lld in the head part), every changed head byte left the file readable\n",
           truncations, changes, in_head);
    return 0;
}
