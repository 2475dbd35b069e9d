// csrc/seal.h alone, as a program of its own (built with the address and undefined-behaviour sanitizers by tests/test_rs_parity_format.py):
// the seal reader on a small file whose PARITY SECTION is of the 'L3CQ' kind (R = 2 rows per group over GF(2^8)) -- every truncation, single-byte
// changes at every position of the file, and crafted S, G, m, R, reserved and plen fields.  Every file is copied into a heap block of exactly
// its size, so that a read past its end is a sanitizer report.  Every call must return 1, 0 or L3C_ERR_INVALID_ARG (with an
// "invalid file: seal" message); a file it accepts must hand out a table and a section that lie inside the file, and the entry that knows
// the 'L3CP' section alone must report the same body with m = 0.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../l3c-pytorch_amd/csrc/seal.h"

static long long accepted = 0, refused = 0, unsealed = 0;
static volatile uint32_t sink;      // keeps the reads of what was handed out

static int fail(const char *what, long long a, long long b) {
    printf("parity_rs_check: FAILED %s (%lld, %lld)\n", what, a, b);
    return 1;
}

// a b in GF(2^8), polynomial 0x11D, bit by bit
static uint8_t gf_mul(uint8_t a, uint8_t b) {
    unsigned p = 0, x = a;
    for (int i = 0; i < 8; ++i) {
        if (b & (1u << i)) p ^= x;
        x <<= 1;
        if (x & 0x100) x ^= 0x11D;
    }
    return (uint8_t)p;
}

// one call on an exactly sized copy -> 0 when the answer is one of the three allowed ones and consistent
static int probe(const std::vector<uint8_t> &file, int64_t n, const char *what, long long a, int *rc_out = nullptr) {
    uint8_t *exact = static_cast<uint8_t *>(malloc(n ? n : 1));
    memcpy(exact, file.data(), n);
    char err[200], err2[200];
    err[0] = err2[0] = 0;
    int64_t body = -1, body2 = -1;
    l3c_seal seal = {0, 0, 0};
    l3c_seal_bands bands = {-1, 0, nullptr}, bands2 = {-1, 0, nullptr};
    l3c_seal_parity_rs par = {-1, -1, -1, nullptr, nullptr, -1};
    l3c_seal_parity old = {-1, -1, nullptr, nullptr, -1};
    const int rc = l3c_sealing::find_parity_rs(exact, n, &body, &seal, &bands, &par, err, sizeof err);
    const int rc2 = l3c_sealing::find_parity(exact, n, &body2, nullptr, &bands2, &old, err2, sizeof err2);
    int bad = rc2 != rc || body2 != body || bands2.n != bands.n || strcmp(err, err2) != 0;
    if (rc == 1) {
        ++accepted;
        if (body < 0 || body > n - L3C_SEAL_BYTES) bad = 1;
        if (bands.n < 0 || bands.n > l3c_sealing::MAX_BANDS || par.m < 0 || par.m > bands.n) bad = 1;
        if (par.m > 0 && !bad) {
            uint32_t x = 0;
            int64_t sum = 0;
            if (par.R < 1 || par.R > 4) bad = 1;
            if (old.m != (par.R == 1 ? par.m : 0)) bad = 1;                                   // 'L3CQ' reads as a band-sealed file there
            if (par.plen != exact + body + (par.R == 1 ? 8 : 12) || par.payloads != par.plen + 12 * par.m) bad = 1;
            for (int i = 0; i < 3 * par.m; ++i) sum += (int64_t)l3c_sealing::get(par.plen + 4 * i, 4);
            if (par.R * sum != par.payload_bytes || par.payloads + par.payload_bytes + 8 > bands.crc - 12) bad = 1;
            for (int64_t i = 0; i < par.payload_bytes && !bad; ++i) x ^= par.payloads[i];     // the payloads can be read
            sink = x;
        }
        if (bands.n > 0 && !bad) {
            uint32_t x = 0;
            for (int i = 0; i < 3 * bands.n; ++i) x ^= (uint32_t)l3c_sealing::get(bands.crc + 4 * i, 4);
            sink = x;
        }
    } else if (rc == 0) {
        ++unsealed;
        if (body != n || bands.n != 0 || par.m != 0) bad = 1;
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
    // the known answer: one-byte members 0x01, 0x02, 0x80 at the points 1, alpha, alpha^2
    {
        const uint8_t d[3] = {0x01, 0x02, 0x80}, want[4] = {0x83, 0x3F, 0xE1, 0x96};
        for (int r = 0; r < 4; ++r) {
            uint8_t p = 0, x = 1;
            for (int k = 0; k < 3; ++k) {
                uint8_t xr = 1;
                for (int i = 0; i < r; ++i) xr = gf_mul(xr, x);
                p ^= gf_mul(xr, d[k]);
                x = gf_mul(x, 2);
            }
            if (p != want[r]) return fail("the known answer", r, p);
        }
    }
    // a banded file of two records: 8x8 with one band of 64, 16x24 with n = 6 bands of 64 per channel, three channels; G = 4: m = 2; R = 2
    std::vector<uint8_t> body = {'L', '3', 'C', 'B', 1, 0};
    for (int i = 0; i < 8; ++i) body.push_back((uint8_t)(i + 1));
    std::vector<std::vector<uint8_t>> finest;
    auto record = [&](int C, int H, int W, uint32_t L, int n, bool keep) {
        body.push_back((uint8_t)C);
        body.push_back((uint8_t)H), body.push_back(0), body.push_back((uint8_t)W), body.push_back(0);
        for (int k = 0; k < 4; ++k) body.push_back((uint8_t)(L >> (8 * k)));
        for (int s = 0; s < C * n; ++s) {
            const int len = (5 * s + 2) % 7;                                               // 0 .. 6 bytes: empty members among them
            body.push_back((uint8_t)len), body.push_back(0), body.push_back(0), body.push_back(0);
            std::vector<uint8_t> p;
            for (int i = 0; i < len; ++i) p.push_back((uint8_t)(37 * s + 11 * i + 5));
            body.insert(body.end(), p.begin(), p.end());
            if (keep) finest.push_back(p);
        }
        body.insert(body.end(), l3c_sealing::SEPARATOR, l3c_sealing::SEPARATOR + 4);
    };
    record(1, 8, 8, 64, 1, false);
    record(3, 16, 24, 64, 6, true);
    const int n = 6, G = 4, m = 2, R = 2;
    const uint32_t L = 64;
    uint8_t crc[12 * n];
    for (int i = 0; i < 3 * n; ++i) l3c_sealing::put(crc + 4 * i, 0x9E3779B9u * (uint32_t)(i + 1), 4);
    l3c_seal want = {3, 0, 0x0123456789ABCDEFull};
    want.frame_crc = l3c_sealing::combine_bands(crc, n, L, 16 * 24);
    uint32_t plen[3 * m];
    std::vector<uint8_t> payloads;
    int64_t plen_sum = 0;
    for (int c = 0; c < 3; ++c)
        for (int g = 0; g < m; ++g) {
            size_t longest = 0;
            for (int j = g; j < n; j += m) longest = finest[c * n + j].size() > longest ? finest[c * n + j].size() : longest;
            plen[c * m + g] = (uint32_t)longest;
            plen_sum += (int64_t)longest;
            for (int r = 0; r < R; ++r) {
                std::vector<uint8_t> x(longest, 0);
                uint8_t point = 1;                                                         // alpha^k
                for (int j = g; j < n; j += m) {
                    const std::vector<uint8_t> &p = finest[c * n + j];
                    for (size_t i = 0; i < p.size(); ++i) x[i] ^= r ? gf_mul(point, p[i]) : p[i];
                    point = gf_mul(point, 2);
                }
                payloads.insert(payloads.end(), x.begin(), x.end());
            }
        }
    const int64_t S = l3c_sealing::rs_section_bytes(m, R, plen_sum), T = l3c_sealing::table_bytes(n);
    if ((int64_t)payloads.size() != R * plen_sum) return fail("the payload bytes", (long long)payloads.size(), R * plen_sum);
    std::vector<uint8_t> file = body;
    file.resize(body.size() + S + T + L3C_SEAL_BYTES);
    l3c_sealing::write_parity_rs(want, body.data() + 6, crc, n, L, G, m, R, plen, payloads.data(), file.data() + body.size());
    const int64_t size = (int64_t)file.size();
    const size_t section = body.size(), table = body.size() + S;

    // the intact file, through the four entries
    {
        int64_t got_body = -1;
        l3c_seal got = {0, 0, 0};
        l3c_seal_bands bands = {0, 0, nullptr};
        l3c_seal_parity_rs par = {0, 0, 0, nullptr, nullptr, 0};
        l3c_seal_parity old = {-1, -1, nullptr, nullptr, -1};
        char err[200];
        err[0] = 0;
        if (l3c_sealing::find_parity_rs(file.data(), size, &got_body, &got, &bands, &par, err, sizeof err) != 1 || got_body != (int64_t)body.size() ||
            got.generation != 3 || got.frame_crc != want.frame_crc || got.model_id != want.model_id || bands.n != n || bands.band_len != L ||
            bands.crc != file.data() + table + 12 || par.G != G || par.m != m || par.R != R || par.payload_bytes != (int64_t)payloads.size() ||
            par.plen != file.data() + section + 12 || memcmp(par.payloads, payloads.data(), payloads.size()) != 0) {
            printf("%s\n", err);
            return fail("the intact file", got_body, par.m);
        }
        if (l3c_sealing::find_parity(file.data(), size, &got_body, &got, &bands, &old, err, sizeof err) != 1 || got_body != (int64_t)body.size() ||
            bands.n != n || old.m != 0 || old.G != 0 || old.payloads != nullptr)
            return fail("the intact file through the 'L3CP' entry", got_body, old.m);
        if (l3c_sealing::find_bands(file.data(), size, &got_body, &got, &bands, err, sizeof err) != 1 || got_body != (int64_t)body.size() || bands.n != n)
            return fail("the intact file through the version-2 entry", got_body, bands.n);
        if (l3c_sealing::find(file.data(), size, &got_body, &got, err, sizeof err) != 1 || got_body != (int64_t)body.size())
            return fail("the intact file through the version-1 entry", got_body, 0);
    }
    // R = 1 through the new writer: write_parity's bytes
    {
        std::vector<uint8_t> a(l3c_sealing::section_bytes(m, plen_sum) + T + L3C_SEAL_BYTES), b(a.size());
        std::vector<uint8_t> row0;
        const uint8_t *at = payloads.data();
        for (int i = 0; i < 3 * m; ++i) row0.insert(row0.end(), at, at + plen[i]), at += R * plen[i];
        l3c_sealing::write_parity(want, body.data() + 6, crc, n, L, G, m, plen, row0.data(), a.data());
        l3c_sealing::write_parity_rs(want, body.data() + 6, crc, n, L, G, m, 1, plen, row0.data(), b.data());
        if (a != b || memcmp(a.data(), "L3CP", 4) != 0) return fail("R = 1 must be written as 'L3CP'", 0, 0);
    }
    for (int64_t cut = 0; cut < size; ++cut)
        if (probe(file, cut, "truncation", cut)) return 1;
    const long long truncations = size;
    // every single-byte change: only the records and the parity PAYLOADS are outside the check word
    long long changes = 0, slipped = 0, payload_changes_accepted = 0;
    const int64_t pay0 = (int64_t)section + 12 + 12 * m, pay1 = (int64_t)section + S - 8;
    for (int64_t at = 0; at < size; ++at)
        for (int v = 1; v < 256; v += 7) {
            std::vector<uint8_t> bad = file;
            bad[at] ^= (uint8_t)v;
            int rc = -9;
            if (probe(bad, size, "single-byte change", at, &rc)) return 1;
            ++changes;
            const bool records = (at >= 4 && at < 6) || (at >= 14 && at < (int64_t)body.size());
            const bool parity_payload = at >= pay0 && at < pay1;
            const bool marker = at >= size - 28 && at < size - 20;
            if (parity_payload) {
                if (rc != 1) return fail("a changed parity payload byte must not make the file unreadable", at, rc);
                ++payload_changes_accepted;
            } else if (rc == 1 && !records) {
                ++slipped;
            }
            if (marker && rc != 0) return fail("a changed marker must read as unsealed", at, rc);
        }
    if (slipped) return fail("a changed header, section head, table or seal byte was accepted", slipped, 0);
    // crafted fields, the check word made right again so that the field itself is what the reader meets
    auto reseal = [&](std::vector<uint8_t> &f) {
        const size_t s = f.size() - L3C_SEAL_BYTES;
        const uint32_t mm = (uint32_t)l3c_sealing::get(f.data() + section + 6, 2);
        uint32_t c = l3c_sealing::crc32(0, f.data() + 6, 8);
        const int64_t head = 12 + 12 * (int64_t)mm;
        if (section + head <= table - 8) c = l3c_sealing::crc32(c, f.data() + section, head);
        c = l3c_sealing::crc32(c, f.data() + table - 8, 8);
        put32(f, s + 20, l3c_sealing::crc32(l3c_sealing::crc32(c, f.data() + table, T), f.data() + s, 20));
    };
    long long crafted = 0;
    const uint32_t lengths[] = {0, 8, 27, 28, 31, 32, (uint32_t)S - 1, (uint32_t)S + 1, (uint32_t)S + 4, (uint32_t)size, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    for (uint32_t t : lengths) {
        std::vector<uint8_t> bad = file;
        put32(bad, table - 8, t);
        int rc = -9;
        if (probe(bad, size, "crafted S", t, &rc) || rc == 1) return fail("crafted S accepted", t, rc);
        reseal(bad);
        if (probe(bad, size, "crafted S, resealed", t, &rc) || rc == 1) return fail("crafted S accepted", t, rc);
        crafted += 2;
    }
    const uint32_t groups[] = {0, 1, 2, 3, 5, 6, 7, 255, 256, 1024, 0xFFFF};    // G: 3 and 5 give m = 2 as well and are consistent; the others are not
    for (uint32_t g : groups) {
        std::vector<uint8_t> bad = file;
        l3c_sealing::put(bad.data() + section + 4, g, 2);
        reseal(bad);
        int rc = -9;
        if (probe(bad, size, "crafted G", g, &rc)) return 1;
        const bool consistent = g >= 1 && g <= (uint32_t)n && (n + g - 1) / g == (uint32_t)m;
        if ((rc == 1) != consistent) return fail("crafted G", g, rc);
        ++crafted;
    }
    const uint32_t counts[] = {0, 1, 3, 6, 1024, 0xFFFF};
    for (uint32_t c : counts) {
        std::vector<uint8_t> bad = file;
        l3c_sealing::put(bad.data() + section + 6, c, 2);
        reseal(bad);
        int rc = -9;
        if (probe(bad, size, "crafted m", c, &rc) || rc == 1) return fail("crafted m accepted", c, rc);
        ++crafted;
    }
    const uint32_t streams[] = {0, 1, 3, 4, 5, 255, 0xFFFF};                      // R: another count does not fit S, or lies outside 2..4
    for (uint32_t r : streams) {
        std::vector<uint8_t> bad = file;
        l3c_sealing::put(bad.data() + section + 8, r, 2);
        reseal(bad);
        int rc = -9;
        if (probe(bad, size, "crafted R", r, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("crafted R", r, rc);
        ++crafted;
    }
    for (uint32_t v : {1u, 0x100u, 0xFFFFu}) {
        std::vector<uint8_t> bad = file;
        l3c_sealing::put(bad.data() + section + 10, v, 2);
        reseal(bad);
        int rc = -9;
        if (probe(bad, size, "crafted reserved field", v, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("crafted reserved field", v, rc);
        ++crafted;
    }
    for (int i = 0; i < 3 * m; ++i) {                                           // a plen moved by one, the next one moved back: S still fits
        std::vector<uint8_t> bad = file;
        const int k = (i + 1) % (3 * m);
        put32(bad, section + 12 + 4 * i, plen[i] + 1);
        put32(bad, section + 12 + 4 * k, plen[k] - 1);
        reseal(bad);
        int rc = -9;
        if (probe(bad, size, "crafted plen", i, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("crafted plen", i, rc);
        ++crafted;
    }
    {
        std::vector<uint8_t> bad = file;
        int rc = -9;
        bad[0] = 1, bad[1] = 0, bad[2] = 2, bad[3] = 0;       // no longer 'L3CB': a legacy file's padding fields
        if (probe(bad, size, "legacy body", 0, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("legacy body", 0, rc);
        bad = file;
        bad[section + 3] = 'X';
        reseal(bad);
        if (probe(bad, size, "signature", 0, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("signature", 0, rc);
        bad = file;
        bad[section + 3] = 'P';                               // the other kind's signature on this layout
        reseal(bad);
        if (probe(bad, size, "the 'L3CP' signature on an 'L3CQ' section", 0, &rc) || rc != L3C_ERR_INVALID_ARG) return fail("signature P", 0, rc);
        crafted += 3;
    }
    printf("parity_rs_check: %lld truncations, %lld single-byte changes (%lld in parity payloads, all readable), %lld crafted fields: %lld accepted, "
           "%lld refused, %lld unsealed\n", truncations, changes, payload_changes_accepted, crafted, accepted, refused, unsealed);
    return 0;
}
