// csrc/seal.h alone, as a program of its own (built with the address and undefined-behaviour sanitizers by tests/test_band_seal_format.py):
// the seal reader on a small BAND-SEALED file -- every truncation, every single-byte change of the whole file, and crafted length and count
// fields.  Every file is copied into a heap block of exactly its size, so that a read past its end is a sanitizer report.  Every call
// must return 1, 0 or L3C_ERR_INVALID_ARG (with an "invalid file: seal" message), and a file it accepts must hand out a table that lies
// inside the file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../l3c-pytorch_amd/csrc/seal.h"

static long long accepted = 0, refused = 0, unsealed = 0;
static volatile uint32_t sink;      // keeps the reads of a table that was handed out

static int fail(const char *what, long long a, long long b) {
    printf("band_seal_check: FAILED %s (%lld, %lld)\n", what, a, b);
    return 1;
}

// one call on an exactly sized copy -> 0 when the answer is one of the three allowed ones and consistent
static int probe(const std::vector<uint8_t> &file, int64_t n, const char *what, long long a, int *rc_out = nullptr) {
    uint8_t *exact = static_cast<uint8_t *>(malloc(n ? n : 1));
    memcpy(exact, file.data(), n);
    char err[160];
    err[0] = 0;
    int64_t body = -1;
    l3c_seal seal = {0, 0, 0};
    l3c_seal_bands bands = {-1, 0, nullptr};
    const int rc = l3c_sealing::find_bands(exact, n, &body, &seal, &bands, err, sizeof err);
    int bad = 0;
    if (rc == 1) {
        ++accepted;
        if (body < 0 || body > n - L3C_SEAL_BYTES) bad = 1;
        if (bands.n < 0 || bands.n > l3c_sealing::MAX_BANDS) bad = 1;
        if (bands.n > 0 && (bands.crc < exact + body + 12 || bands.crc + 12 * bands.n > exact + n - L3C_SEAL_BYTES - 8)) bad = 1;
        if (bands.n > 0) {                                    // the words can be read
            uint32_t x = 0;
            for (int i = 0; i < 3 * bands.n; ++i) x ^= (uint32_t)l3c_sealing::get(bands.crc + 4 * i, 4);
            sink = x;
        }
    } else if (rc == 0) {
        ++unsealed;
        if (body != n || bands.n != 0) bad = 1;
    } else if (rc == L3C_ERR_INVALID_ARG) {
        ++refused;
        if (strncmp(err, "invalid file: seal", 18) != 0) bad = 1;
    } else {
        bad = 1;
    }
    free(exact);
    if (rc_out) *rc_out = rc;
    return bad ? fail(what, a, rc) : 0;
}

static void put32(std::vector<uint8_t> &f, size_t at, uint32_t v) { l3c_sealing::put(f.data() + at, v, 4); }

int main() {
    // a banded file of two records: 8x8 with one band of 64, 16x16 with n = 4 bands of 64 per channel, three channels
    std::vector<uint8_t> body = {'L', '3', 'C', 'B', 1, 0};
    for (int i = 0; i < 8; ++i) body.push_back((uint8_t)(i + 1));
    auto record = [&](int C, int H, int W, uint32_t L, int n) {
        body.push_back((uint8_t)C);
        body.push_back((uint8_t)H), body.push_back(0), body.push_back((uint8_t)W), body.push_back(0);
        for (int k = 0; k < 4; ++k) body.push_back((uint8_t)(L >> (8 * k)));
        for (int s = 0; s < C * n; ++s) {
            const int len = 1 + s % 3;
            body.push_back((uint8_t)len), body.push_back(0), body.push_back(0), body.push_back(0);
            for (int i = 0; i < len; ++i) body.push_back((uint8_t)(37 * s + 11 * i + 5));
        }
        body.insert(body.end(), l3c_sealing::SEPARATOR, l3c_sealing::SEPARATOR + 4);
    };
    record(1, 8, 8, 64, 1);
    record(3, 16, 16, 64, 4);
    const int n = 4;
    const uint32_t L = 64;
    uint8_t crc[12 * n];
    for (int i = 0; i < 3 * n; ++i) l3c_sealing::put(crc + 4 * i, 0x9E3779B9u * (uint32_t)(i + 1), 4);
    l3c_seal want = {3, 0, 0x0123456789ABCDEFull};
    want.frame_crc = l3c_sealing::combine_bands(crc, n, L, 256);
    const int64_t T = l3c_sealing::table_bytes(n);
    std::vector<uint8_t> file = body;
    file.resize(body.size() + T + L3C_SEAL_BYTES);
    l3c_sealing::write_bands(want, body.data() + 6, crc, n, L, file.data() + body.size());
    const int64_t size = (int64_t)file.size();

    // the intact file, through both entries
    {
        int64_t got_body = -1;
        l3c_seal got = {0, 0, 0};
        l3c_seal_bands bands = {0, 0, nullptr};
        char err[160];
        if (l3c_sealing::find_bands(file.data(), size, &got_body, &got, &bands, err, sizeof err) != 1 || got_body != (int64_t)body.size() ||
            got.generation != 3 || got.frame_crc != want.frame_crc || got.model_id != want.model_id || bands.n != n || bands.band_len != L ||
            bands.crc != file.data() + body.size() + 12 || memcmp(bands.crc, crc, sizeof crc) != 0)
            return fail("the intact file", got_body, bands.n);
        if (l3c_sealing::find(file.data(), size, &got_body, &got, err, sizeof err) != 1 || got_body != (int64_t)body.size())
            return fail("the intact file through the version-1 entry", got_body, 0);
    }
    // every truncation: never sealed unless the cut leaves another recognisable end, never a read past the end
    for (int64_t cut = 0; cut < size; ++cut)
        if (probe(file, cut, "truncation", cut)) return 1;
    const long long truncations = size;
    // every single-byte change of the whole file
    long long changes = 0, slipped = 0;
    for (int64_t at = 0; at < size; ++at)
        for (int v = 1; v < 256; ++v) {
            std::vector<uint8_t> bad = file;
            bad[at] ^= (uint8_t)v;
            int rc = -9;
            if (probe(bad, size, "single-byte change", at, &rc)) return 1;
            ++changes;
            const bool payload = (at >= 4 && at < 6) || (at >= 14 && at < (int64_t)body.size());      // format version and records: not under the check word
            const bool marker = at >= size - 28 && at < size - 20;
            if (rc == 1 && !payload) ++slipped;
            if (marker && rc != 0) return fail("a changed marker must read as unsealed", at, rc);
        }
    if (slipped) return fail("a changed header, table or seal byte was accepted", slipped, 0);
    // crafted length and count fields, the check word made right again so that the field itself is what the reader meets
    const size_t table = body.size(), seal = body.size() + T;
    auto reseal = [&](std::vector<uint8_t> &f) {
        const size_t s = f.size() - L3C_SEAL_BYTES;
        const uint32_t t = (uint32_t)l3c_sealing::get(f.data() + s - 8, 4);
        const uint8_t *tab = t <= s ? f.data() + s - t : f.data();
        put32(f, s + 20, l3c_sealing::crc32(l3c_sealing::crc32(l3c_sealing::crc32(0, f.data() + 6, 8), tab, t <= s ? t : 0), f.data() + s, 20));
    };
    long long crafted = 0;
    const uint32_t lengths[] = {0, 8, 19, 20, 21, 31, 32, 20 + 12 * 3, 20 + 12 * 5, (uint32_t)T + 1, (uint32_t)T + 12, 20 + 12 * 1024, 20 + 12 * 1025,
                                (uint32_t)size, (uint32_t)size + 20, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 0xFFFFFFF8u};
    for (uint32_t t : lengths) {
        std::vector<uint8_t> bad = file;
        put32(bad, seal - 8, t);
        int rc = -9;
        if (probe(bad, size, "crafted T", t, &rc) || rc == 1) return fail("crafted T accepted", t, rc);
        reseal(bad);
        if (probe(bad, size, "crafted T, resealed", t, &rc) || rc == 1) return fail("crafted T accepted", t, rc);
        crafted += 2;
    }
    const uint32_t counts[] = {0, 1, 3, 5, 1024, 1025, 0xFFFF};
    for (uint32_t c : counts) {
        std::vector<uint8_t> bad = file;
        l3c_sealing::put(bad.data() + table + 4, c, 2);
        reseal(bad);
        int rc = -9;
        if (probe(bad, size, "crafted n", c, &rc) || rc == 1) return fail("crafted n accepted", c, rc);
        ++crafted;
    }
    {   // another L, a non-zero reserved field, a version-2 seal on a legacy body, a frame CRC that is not the combination
        std::vector<uint8_t> bad = file;
        int rc = -9;
        put32(bad, table + 8, 128);
        reseal(bad);
        if (probe(bad, size, "crafted L", 128, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("crafted L", 128, rc);
        bad = file;
        bad[table + 6] = 1;
        reseal(bad);
        if (probe(bad, size, "reserved", 1, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("reserved", 1, rc);
        bad = file;
        put32(bad, seal + 8, want.frame_crc ^ 1u);
        reseal(bad);
        if (probe(bad, size, "frame CRC", 0, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("frame CRC", 0, rc);
        bad = file;
        bad[0] = 1, bad[1] = 0, bad[2] = 2, bad[3] = 0;       // no longer 'L3CB': a legacy file's padding fields
        if (probe(bad, size, "legacy body", 0, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("legacy body", 0, rc);
        crafted += 4;
    }
    printf("band_seal_check: %lld truncations, %lld single-byte changes, %lld crafted fields: %lld accepted, %lld refused, %lld unsealed\n", truncations,
           changes, crafted, accepted, refused, unsealed);
    return 0;
}
