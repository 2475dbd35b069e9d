// csrc/seal.h alone, as a program of its own (built with the address and undefined-behaviour sanitizers by tests/test_seal_format.py):
// the seal reader on every truncation of a small sealed file and on every single-byte change of its last 32 bytes, legacy and banded.
// Every file is copied into a heap block of exactly its size, so that a read past its end is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../l3c-pytorch_amd/csrc/seal.h"

static int find(const std::vector<uint8_t> &file, int64_t n, int64_t *body, l3c_seal *seal, char *err) {
    uint8_t *exact = static_cast<uint8_t *>(malloc(n ? n : 1));
    memcpy(exact, file.data(), n);
    err[0] = 0;
    const int rc = l3c_sealing::find(exact, n, body, seal, err, 128);
    free(exact);
    return rc;
}

static int fail(const char *what, long long a, long long b) {
    printf("seal_check: FAILED %s (%lld, %lld)\n", what, a, b);
    return 1;
}

int main() {
    long long truncations = 0, changes = 0, refused = 0, unsealed = 0;
    for (int banded = 0; banded < 2; ++banded) {
        // a small file: header (8 padding bytes, or 'L3CB' 1 0 + padding), some payload bytes, the separator
        std::vector<uint8_t> body;
        if (banded) body = {'L', '3', 'C', 'B', 1, 0};
        for (int i = 0; i < 8; ++i) body.push_back((uint8_t)(i + 1));
        for (int i = 0; i < 23; ++i) body.push_back((uint8_t)(37 * i + 5));
        body.insert(body.end(), l3c_sealing::SEPARATOR, l3c_sealing::SEPARATOR + 4);
        const l3c_seal want = {3, 0xDEADBEEFu, 0x0123456789ABCDEFull};
        std::vector<uint8_t> file = body;
        file.resize(body.size() + L3C_SEAL_BYTES);
        l3c_sealing::write(want, body.data() + (banded ? 6 : 0), file.data() + body.size());
        const int64_t n = (int64_t)file.size();
        char err[128];
        int64_t got_body = -1;
        l3c_seal got = {0, 0, 0};
        if (find(file, n, &got_body, &got, err) != 1 || got_body != (int64_t)body.size() || got.generation != want.generation ||
            got.frame_crc != want.frame_crc || got.model_id != want.model_id)
            return fail("the intact file", banded, got_body);
        if (find(body, (int64_t)body.size(), &got_body, &got, err) != 0 || got_body != (int64_t)body.size()) return fail("the unsealed body", banded, got_body);
        // every truncation: never sealed, never an error, the size handed back unchanged
        for (int64_t cut = 0; cut < n; ++cut) {
            if (find(file, cut, &got_body, &got, err) != 0 || got_body != cut) return fail("truncation", banded, cut);
            ++truncations;
        }
        // every single-byte change of the last 32 bytes: the separator or the signature gone -> unsealed; anything else -> refused
        for (int64_t at = n - 32; at < n; ++at)
            for (int v = 1; v < 256; ++v) {
                std::vector<uint8_t> bad = file;
                bad[at] ^= (uint8_t)v;
                const int rc = find(bad, n, &got_body, &got, err);
                const bool marker = at >= n - 28 && at < n - 20;
                if (marker ? (rc != 0 || got_body != n) : at < n - 28 ? (rc != 1) : (rc != L3C_ERR_INVALID_ARG || strncmp(err, "invalid file: seal", 18) != 0))
                    return fail("single-byte change", at - n, v);
                ++changes;
                refused += rc == L3C_ERR_INVALID_ARG;
                unsealed += rc == 0;
            }
        // a damaged padding field under a valid seal is refused too
        for (int i = 0; i < 8; ++i) {
            std::vector<uint8_t> bad = file;
            bad[(banded ? 6 : 0) + i] ^= 0x40;
            if (find(bad, n, &got_body, &got, err) != L3C_ERR_INVALID_ARG) return fail("padding byte", banded, i);
        }
    }
    printf("seal_check: %lld truncations unsealed; %lld single-byte changes: %lld refused, %lld unsealed\n", truncations, changes, refused, unsealed);
    return 0;
}
