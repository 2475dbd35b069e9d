// tests/hostsim/chunk_hostsim.cpp -- TEST INFRASTRUCTURE: a stream decoded CHUNK BY CHUNK on the host with the rules the HIP decoders
// share (l3c-pytorch_amd/csrc/ac_core.h: chunk_is_empty, chunk_no_advance, the entry_* chunking of l3c_decode_rgb_entries) and the record
// they carry between two launches (low, high, value, bits consumed).  Not part of the product path.  Shared with the kernels are those
// predicates; the loop below that skips an empty chunk and keeps its record is this file's own (the kernels return early and copy
// state_in to state_out themselves: tests/test_gpu_banded_set.py runs that).
//
// Build: g++ -O2 -shared -fPIC -I l3c-pytorch_amd/csrc -o tests/hostsim/_build/libchunk_hostsim.so tests/hostsim/chunk_hostsim.cpp
#include <cstring>

#include "ac_core.h"

namespace {
struct MemFetch {
    const uint8_t *p;
    uint32_t nbytes;
    uint32_t operator()(uint32_t i) const {
        uint32_t w = 0;
        for (int k = 0; k < 4; ++k) {
            const uint64_t off = (uint64_t)i * 4 + k;
            w = (w << 8) | (off < nbytes ? p[off] : 0u);
        }
        return w;
    }
};
struct Record {
    uint32_t low, high, value, pos;
};
}  // namespace

extern "C" {

long long hostsim_entry_step(long long len, long long chunks) { return l3c::entry_step(len, chunks); }
long long hostsim_entry_npix(long long len, long long chunks, long long k) { return l3c::entry_npix(len, chunks, k); }
long long hostsim_entry_final_chunk(long long len, long long chunks) { return l3c::entry_final_chunk(len, chunks); }

// Decode n_chunks chunks of chunk_len[k] symbols each (0: an empty chunk), the stream ending with chunk `final_chunk`; every chunk starts
// from the record the previous one left, as a launch does.  sym_out is written only where a chunk decodes; records_out [n_chunks][4]
// receives the record after every chunk.  Returns the number of symbols written.
long long hostsim_decode_chunks(const uint16_t *cdf, long long row_stride, int Lp, const uint8_t *in, long long in_len,
                                const long long *chunk_len, int n_chunks, int final_chunk, int16_t *sym_out, uint32_t *records_out) {
    const uint32_t top = (uint32_t)(Lp - 2);
    Record rec{0u, 0xFFFFFFFFu, 0u, 0u};
    bool started = false;
    long long first = 0, written = 0;
    for (int k = 0; k < n_chunks; ++k) {
        const uint32_t n_sym = (uint32_t)chunk_len[k];
        if (!l3c::chunk_is_empty(n_sym)) {
            l3c::WordSource<MemFetch> src(MemFetch{in, (uint32_t)in_len});
            uint32_t low = rec.low, high = rec.high, value = rec.value;
            if (started) {
                for (uint32_t skip = rec.pos; skip;) {   // resume where the previous chunk stopped
                    const int c = skip > 32u ? 32 : (int)skip;
                    src.take(c);
                    skip -= (uint32_t)c;
                }
            } else {
                value = src.take(32);
                started = true;
            }
            const uint32_t no_advance = l3c::chunk_no_advance(n_sym, k == final_chunk);
            for (uint32_t i = 0; i < n_sym; ++i) {
                const uint16_t *row = cdf + (first + i) * row_stride;
                const uint32_t count = l3c::decode_count(low, high, value);
                uint32_t rank = 0;
                for (uint32_t m = 0; m <= top; ++m) rank += row[m] <= count;
                const uint32_t x = rank ? rank - 1 : 0;
                sym_out[first + i] = (int16_t)x;
                ++written;
                if (i == no_advance) continue;
                l3c::decode_advance(low, high, value, row[x], x == top ? 0x10000u : row[x + 1], src);
            }
            rec = Record{low, high, value, src.next * 32u - (uint32_t)src.nb};
            first += n_sym;
        }
        std::memcpy(records_out + 4 * k, &rec, sizeof(rec));
    }
    return written;
}
}
