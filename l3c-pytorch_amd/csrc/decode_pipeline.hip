// decode_pipeline.hip -- the chunk-pipelined decode of the RGB scale, issued by ONE host call (round 6).
//
// Reference: the decoder's per-channel loop (src/bitcoding/bitcoding.py:212-266: for every channel, build the CDF from the channels
// decoded so far, then torchac.decode_logistic_mixture -> torchac.cpp:299-381).  Channel c's means depend on the decoded values of the
// channels < c AT THE SAME PIXEL only (src/criterion/logistic_mixture.py:262-272), so R, G and B are three serial chains that only have
// to stay a chunk of pixels apart: pipeline step t handles chunk t - D c of channel c -- its table rows are built straight from P and the
// symbols decoded so far (ONE grouped table launch, l3c_dmll_cdf_table_parts), then ONE grouped decoder launch (l3c_ac_decode_chunks)
// resumes the range decoders of all active channels side by side.
//
// Until round 5 the host layer (bitcoding.py: _decode_rgb_pipelined) issued these ~150 launches one by one through ctypes, allocating
// a table tensor per launch: 0.24 s of host time for a 0.35 s decode of 128 images -- within 30 % of being bound by the host.  Here the
// whole schedule is a C loop over a caller-owned workspace: a few microseconds per launch, no allocation, no host synchronisation.
//
//   D = 1: everything on `main`.
//   D = 2: the channels stay TWO chunks apart, so the tables of step t + 1 need only the symbols of step t - 1 and are built on `main`
//          WHILE `side` decodes step t: max(table, decode) per step instead of their sum.  Two table slot sets (step parity): the tables
//          of step t are written after `main` has waited for the decode of step t - 2, the last reader of that slot set.
#include "ac_core.h"
#include "l3c_common.h"

#include <string.h>

#include <vector>

namespace {

constexpr int C3 = 3;
constexpr int LP = 257;
constexpr int64_t ALIGN = 256;

inline int64_t up(int64_t n) { return (n + ALIGN - 1) / ALIGN * ALIGN; }

struct Layout {
    int64_t flags, states, stats, scratch, tables, table_bytes, state_bytes, total;
};

// rectangular: B images, max_npix pixels in the longest chunk; ragged (streams > 0): B = 1, max_npix = the largest chunk's TOTAL over the images
Layout layout(int64_t B, int64_t max_npix, int n_chunks, int lag, int64_t streams = 0) {
    Layout l{};
    const int64_t S = streams > 0 ? streams : B;
    l.state_bytes = up(S * l3c_ac_decode_state_bytes());
    l.table_bytes = up(B * max_npix * LP * 2);
    int64_t p = 0;
    l.flags = p;    p += up(C3 * 4);
    l.states = p;   p += C3 * 2 * l.state_bytes;
    l.stats = p;    p += up((int64_t)C3 * (n_chunks + 2) * S * 4);
    l.scratch = p;  p += up(S * 4);
    l.tables = p;   p += (lag == 2 ? 2 : 1) * C3 * l.table_bytes;
    l.total = p;
    return l;
}

// A handful of events per device and host thread, created on first use and reused: an event may be recorded again as soon as every wait
// on its previous record has been ISSUED (hipStreamWaitEvent captures the record it finds), which the schedule below guarantees.
struct EventPool {
    static constexpr int N = 4;
    hipEvent_t ev[N] = {};
    bool made = false;
};
thread_local EventPool g_pool[64];

int events_for_current_device(EventPool **out) {
    int dev = 0;
    int rc = l3c::check_hip(hipGetDevice(&dev), "hipGetDevice");
    if (rc != L3C_OK) return rc;
    if (dev < 0 || dev >= 64) return l3c::fail(L3C_ERR_INVALID_ARG, "%s", "device index out of range");
    EventPool &p = g_pool[dev];
    if (!p.made) {
        for (int i = 0; i < EventPool::N; ++i) {
            rc = l3c::check_hip(hipEventCreateWithFlags(&p.ev[i], hipEventDisableTiming), "hipEventCreateWithFlags");
            if (rc != L3C_OK) return rc;
        }
        p.made = true;
    }
    *out = &p;
    return L3C_OK;
}

}  // namespace

extern "C" {

int64_t l3c_decode_rgb_workspace_bytes(int64_t B, int64_t max_chunk_npix, int n_chunks, int lag) {
    if (B <= 0 || max_chunk_npix <= 0 || n_chunks <= 0 || (lag != 1 && lag != 2)) return -1;
    return layout(B, max_chunk_npix, n_chunks, lag).total;
}

int64_t l3c_decode_rgb_stats_offset(int64_t B, int64_t max_chunk_npix, int n_chunks, int lag) {
    if (B <= 0 || max_chunk_npix <= 0 || n_chunks <= 0 || (lag != 1 && lag != 2)) return -1;
    return layout(B, max_chunk_npix, n_chunks, lag).stats;
}
}

namespace {

// one schedule for both forms: `rag` == nullptr -> the rectangular batch of `d`
struct Ragged {
    const int64_t *hw_host;        // [B]
    const int64_t *pix0_host;      // [n_chunks][B]
    const int64_t *npix_host;      // [n_chunks][B]
    const int64_t *tables_dev;     // pixbase [B] | hw [B] | pix0 [n_chunks][B] | npix [n_chunks][B] | table_off [n_chunks][B]
    const int32_t *final_dev;      // [B] the chunk every stream ends with (l3c_decode_rgb_entries; chunks of npix 0 allowed), nullptr: the last one
};

int decode_rgb_impl(const l3c_rgb_decode_desc *d, const Ragged *rag, int64_t max_npix, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    const Layout l = layout(rag ? 1 : d->B, max_npix, d->n_chunks, d->lag, rag ? d->B : 0);
    L3C_REQUIRE(d->workspace_bytes >= l.total, "workspace too small (l3c_decode_rgb(_ragged)_workspace_bytes)");
    const hipStream_t main = l3c::as_stream(main_stream), side = d->lag == 2 ? l3c::as_stream(side_stream) : main;
    EventPool *pool = nullptr;
    int rc = events_for_current_device(&pool);
    if (rc != L3C_OK) return rc;
    hipEvent_t ev_tables = pool->ev[0];                 // main -> side: the tables of a step (waited for right after its record)
    hipEvent_t *ev_decoded = &pool->ev[1];              // side -> main: step t's symbols, ring of three (waited for at step t + 2)

    uint8_t *ws = static_cast<uint8_t *>(d->workspace);
    int32_t *flags = reinterpret_cast<int32_t *>(ws + l.flags);
    int32_t *stats = reinterpret_cast<int32_t *>(ws + l.stats);
    int32_t *scratch = reinterpret_cast<int32_t *>(ws + l.scratch);
    const int64_t B = d->B, HW = d->HW;
    const int n_ch = d->n_chunks, D = d->lag;
    // flags[c] is only ever SET by the table kernels (a decode launch that sees it mid-way re-decodes its chunk from state_in with the
    // generic path); stats: -1 = unknown = full rows (auto), 0 = window rows from the start (always)
    rc = l3c::check_hip(hipMemsetAsync(flags, 0, C3 * 4, main), "hipMemsetAsync");
    if (rc != L3C_OK) return rc;
    if (d->window_mode) {
        rc = l3c::check_hip(hipMemsetAsync(stats, d->window_mode == 1 ? 0xFF : 0, (size_t)C3 * (n_ch + 2) * B * 4, main), "hipMemsetAsync");
        if (rc != L3C_OK) return rc;
    }
    if (D == 2) {   // the workspace initialisation and whatever the caller enqueued on `main` (sym, the packed streams) before the side stream reads it
        rc = l3c::check_hip(hipEventRecord(ev_tables, main), "hipEventRecord");
        if (rc == L3C_OK) rc = l3c::check_hip(hipStreamWaitEvent(side, ev_tables, 0), "hipStreamWaitEvent");
        if (rc != L3C_OK) return rc;
    }
    l3c_ragged_batch rb{};
    const int64_t *dev_pix0 = nullptr, *dev_npix = nullptr, *dev_off = nullptr;
    if (rag) {
        int64_t max_hw = 0;
        for (int64_t b = 0; b < B; ++b) max_hw = rag->hw_host[b] > max_hw ? rag->hw_host[b] : max_hw;
        rb = l3c_ragged_batch{B, max_hw, rag->tables_dev, rag->tables_dev + B};
        dev_pix0 = rag->tables_dev + 2 * B;
        dev_npix = dev_pix0 + (int64_t)n_ch * B;
        dev_off = dev_npix + (int64_t)n_ch * B;
    }
    const int n_steps = n_ch + D * (C3 - 1);
    int last_decoded = -1;
    for (int t = 0; t < n_steps; ++t) {
        l3c_table_part tp[C3];
        l3c_ragged_part rp[C3];
        l3c_ac_decode_part dp[C3];
        int chunk_of[C3];
        int n = 0;
        uint8_t *slot = ws + l.tables + (D == 2 ? (t & 1) : 0) * C3 * l.table_bytes;
        for (int c = 0; c < C3; ++c) {
            const int j = t - D * c;
            if (j < 0 || j >= n_ch) continue;
            int64_t p0 = 0, np = 0, total = 0;
            if (rag) {
                for (int64_t b = 0; b < B; ++b) {
                    const int64_t nb = rag->npix_host[(int64_t)j * B + b];
                    np = nb > np ? nb : np;
                    total += nb;
                }
                if (total == 0) continue;   // (entries: a trailing chunk that is empty in every stream)
            } else {
                p0 = d->chunk_pix0_host[j];
                np = d->chunk_npix_host[j];
            }
            uint16_t *table = reinterpret_cast<uint16_t *>(slot + c * l.table_bytes);
            int32_t *st_in = d->window_mode ? stats + ((int64_t)c * (n_ch + 2) + j) * B : nullptr;
            int32_t *st_out = d->window_mode == 2 ? scratch : d->window_mode == 1 ? stats + ((int64_t)c * (n_ch + 2) + j + 2) * B : nullptr;
            tp[n] = l3c_table_part{c, p0, np, table, flags + c, st_in};
            l3c_ac_decode_part q;
            memset(&q, 0, sizeof(q));
            q.cdf = table;
            q.Lp = LP;
            q.in = d->in;
            q.in_offsets = d->in_offsets + (int64_t)c * B;
            q.in_nbytes = d->in_nbytes + (int64_t)c * B;
            q.n_streams = B;
            q.n_sym = np;
            q.not_monotone_flag = flags + c;
            q.state_in = j ? ws + l.states + (c * 2 + ((j + 1) & 1)) * l.state_bytes : nullptr;
            q.state_out = ws + l.states + (c * 2 + (j & 1)) * l.state_bytes;
            q.final_chunk = j == n_ch - 1;
            q.sym_out = d->sym;
            q.sym_stride = C3 * HW;
            q.sym_offset = c * HW + p0;
            if (rag) {
                rp[n] = l3c_ragged_part{dev_pix0 + (int64_t)j * B, dev_npix + (int64_t)j * B, dev_off + (int64_t)j * B};
                q.r_npix = rp[n].npix;
                q.r_table_off = rp[n].table_off;
                q.r_pixbase = rb.pixbase;
                q.r_hw = rb.hw;
                q.r_pix0 = rp[n].pix0;
                q.r_C = C3;
                q.r_c = c;
                q.r_table_bytes = total * LP * 2;
            }
            if (d->window_mode) {
                q.window_stats_in = st_in;
                q.window_stats_out = st_out;
                q.P = d->P;
                q.sym_all = d->sym;
                q.targets = d->targets;
                q.HW = HW;
                q.pix0 = p0;
                q.C = C3;
                q.K = d->K;
                q.c = c;
            }
            chunk_of[n] = j;
            dp[n++] = q;
        }
        if (!n) continue;
        if (D == 2 && t >= 2 && last_decoded >= t - 2) {   // the symbols of step t - 2 (older steps are ordered before it on the side stream)
            rc = l3c::check_hip(hipStreamWaitEvent(main, ev_decoded[(t - 2) % 3], 0), "hipStreamWaitEvent");
            if (rc != L3C_OK) return rc;
        }
        rc = rag ? l3c_dmll_cdf_table_ragged(d->P, d->sym, d->targets, &rb, C3, d->K, 1, LP, tp, rp, n, main)
                 : l3c_dmll_cdf_table_parts(d->P, d->sym, d->targets, B, HW, C3, d->K, 1, LP, tp, n, main);
        if (rc != L3C_OK) return rc;
        if (D == 2) {
            rc = l3c::check_hip(hipEventRecord(ev_tables, main), "hipEventRecord");
            if (rc == L3C_OK) rc = l3c::check_hip(hipStreamWaitEvent(side, ev_tables, 0), "hipStreamWaitEvent");
            if (rc != L3C_OK) return rc;
        }
        rc = rag && rag->final_dev ? l3c::ac_decode_chunks_entries(dp, n, rag->final_dev, chunk_of, side) : l3c_ac_decode_chunks(dp, n, side);
        if (rc != L3C_OK) return rc;
        if (D == 2) {
            rc = l3c::check_hip(hipEventRecord(ev_decoded[t % 3], side), "hipEventRecord");
            if (rc != L3C_OK) return rc;
            last_decoded = t;
        }
    }
    if (D == 2 && last_decoded >= 0) {   // the caller's stream continues after the last symbols
        rc = l3c::check_hip(hipStreamWaitEvent(main, ev_decoded[last_decoded % 3], 0), "hipStreamWaitEvent");
        if (rc != L3C_OK) return rc;
    }
    return L3C_OK;
}

}  // namespace

extern "C" {

int l3c_decode_rgb(const l3c_rgb_decode_desc *d, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    L3C_REQUIRE(d, "null descriptor");
    L3C_REQUIRE(d->P && d->targets && d->sym && d->in && d->in_offsets && d->in_nbytes && d->workspace, "null pointer in descriptor");
    L3C_REQUIRE(d->B > 0 && d->B < 65536 && d->HW > 0 && d->K > 0 && d->K <= 16, "bad shape");
    L3C_REQUIRE(d->n_chunks > 0 && d->n_chunks <= 4096 && d->chunk_pix0_host && d->chunk_npix_host, "bad chunk list");
    L3C_REQUIRE(d->lag == 1 || d->lag == 2, "lag must be 1 (one stream) or 2 (tables and decoders overlapped on two streams)");
    L3C_REQUIRE(d->lag == 1 || side_stream != main_stream, "lag 2 needs a side stream that is not the main stream");
    L3C_REQUIRE(d->window_mode >= 0 && d->window_mode <= 2, "window_mode: 0 never, 1 auto, 2 always");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(d->workspace) & (ALIGN - 1)) == 0, "workspace must be 256-byte aligned");
    int64_t max_npix = 0, next = 0;
    for (int j = 0; j < d->n_chunks; ++j) {
        L3C_REQUIRE(d->chunk_pix0_host[j] == next && d->chunk_npix_host[j] > 0, "chunks must tile [0, HW) in order");
        L3C_REQUIRE(j + 1 == d->n_chunks || d->chunk_npix_host[j] % 64 == 0, "chunk boundaries must lie on the 64-symbol store blocks");
        next += d->chunk_npix_host[j];
        max_npix = d->chunk_npix_host[j] > max_npix ? d->chunk_npix_host[j] : max_npix;
    }
    L3C_REQUIRE(next == d->HW, "chunks must tile [0, HW) in order");
    return decode_rgb_impl(d, nullptr, max_npix, main_stream, side_stream);
}

int64_t l3c_decode_rgb_ragged_workspace_bytes(int64_t B, int64_t max_chunk_total_npix, int n_chunks, int lag) {
    if (B <= 0 || max_chunk_total_npix <= 0 || n_chunks <= 0 || (lag != 1 && lag != 2)) return -1;
    return layout(1, max_chunk_total_npix, n_chunks, lag, B).total;
}

int l3c_decode_rgb_ragged(const l3c_rgb_ragged_desc *r, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    L3C_REQUIRE(r, "null descriptor");
    L3C_REQUIRE(r->P && r->targets && r->sym && r->in && r->in_offsets && r->in_nbytes && r->workspace && r->hw_host && r->tables_dev,
                "null pointer in descriptor");
    L3C_REQUIRE(r->B > 0 && r->B < 65536 && r->K > 0 && r->K <= 16, "bad shape");
    L3C_REQUIRE(r->n_chunks > 0 && r->n_chunks <= 4096 && r->chunk_pix0_host && r->chunk_npix_host, "bad chunk list");
    L3C_REQUIRE(r->lag == 1 || r->lag == 2, "lag must be 1 (one stream) or 2 (tables and decoders overlapped on two streams)");
    L3C_REQUIRE(r->lag == 1 || side_stream != main_stream, "lag 2 needs a side stream that is not the main stream");
    L3C_REQUIRE(r->window_mode >= 0 && r->window_mode <= 2, "window_mode: 0 never, 1 auto, 2 always");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(r->workspace) & (ALIGN - 1)) == 0, "workspace must be 256-byte aligned");
    int64_t max_total = 0;
    for (int64_t b = 0; b < r->B; ++b) {
        int64_t next = 0;
        for (int j = 0; j < r->n_chunks; ++j) {
            const int64_t p0 = r->chunk_pix0_host[(int64_t)j * r->B + b], np = r->chunk_npix_host[(int64_t)j * r->B + b];
            L3C_REQUIRE(p0 == next && np > 0, "every image's chunks must tile [0, HW_b) in order, none empty");
            L3C_REQUIRE(j + 1 == r->n_chunks || np % 64 == 0, "chunk boundaries must lie on the 64-symbol store blocks");
            next += np;
        }
        L3C_REQUIRE(next == r->hw_host[b], "every image's chunks must tile [0, HW_b) in order");
    }
    for (int j = 0; j < r->n_chunks; ++j) {
        int64_t total = 0;
        for (int64_t b = 0; b < r->B; ++b) total += r->chunk_npix_host[(int64_t)j * r->B + b];
        max_total = total > max_total ? total : max_total;
    }
    l3c_rgb_decode_desc d{};
    d.P = r->P;  d.targets = r->targets;  d.sym = r->sym;  d.B = r->B;  d.HW = 0;  d.K = r->K;
    d.in = r->in;  d.in_offsets = r->in_offsets;  d.in_nbytes = r->in_nbytes;
    d.n_chunks = r->n_chunks;  d.lag = r->lag;  d.window_mode = r->window_mode;
    d.workspace = r->workspace;  d.workspace_bytes = r->workspace_bytes;
    const Ragged rag{r->hw_host, r->chunk_pix0_host, r->chunk_npix_host, r->tables_dev, nullptr};
    return decode_rgb_impl(&d, &rag, max_total, main_stream, side_stream);
}
}

// ---- banded files: every band a ragged entry ---------------------------------------------------------------------------------------
//
// Entry e = b * n + j (band j of image b) is pixels [j L, j L + len_j) of image b: pixbase = b HW and hw = HW (P and sym are the
// rectangular batch's; no kernel assumes pixbase = the sum of the hw before it), chunk k at j L + k step_j with step_j = len_j / chunks
// rounded down to 64 symbols, the last chunk taking the rest.  All bands but the last of an image are L long, so chunk k's rows of entry e
// start at 514 (b T_k + j f_k) bytes of the step's table, T_k = (n - 1) f_k + l_k (f_k / l_k: chunk k's length in a full / the last band).
namespace {

struct BandPlan {
    int64_t HW, L, n, chunks;
    __host__ __device__ int64_t len(int64_t j) const { return j + 1 < n ? L : HW - (n - 1) * L; }
    __host__ __device__ int64_t step(int64_t j) const { return len(j) / chunks / 64 * 64; }
    __host__ __device__ int64_t npix(int64_t j, int64_t k) const { return k + 1 < chunks ? step(j) : len(j) - k * step(j); }
};

// tables: pixbase [S] | hw [S] | pix0 [chunks][S] | npix [chunks][S] | table_off [chunks][S]   (the layout of l3c_rgb_ragged_desc.tables_dev)
__global__ __launch_bounds__(256) void band_plan_kernel(const BandPlan p, int64_t S, int64_t *__restrict__ tables) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= p.chunks * S) return;
    const int64_t k = q / S, e = q - k * S;
    const int64_t b = e / p.n, j = e - b * p.n;
    const int64_t f = p.npix(0, k), T = (p.n - 1) * f + p.npix(p.n - 1, k);
    if (k == 0) {
        tables[e] = b * p.HW;
        tables[S + e] = p.HW;
    }
    tables[2 * S + q] = j * p.L + k * p.step(j);
    tables[(2 + p.chunks) * S + q] = p.npix(j, k);
    tables[(2 + 2 * p.chunks) * S + q] = (b * T + j * f) * (int64_t)(LP * 2);
}

int64_t band_total(const BandPlan &p, int64_t B, int64_t k) { return B * ((p.n - 1) * p.npix(0, k) + p.npix(p.n - 1, k)); }

int64_t banded_max_total(const BandPlan &p, int64_t B) {
    int64_t m = 0;
    for (int64_t k = 0; k < p.chunks; ++k) m = band_total(p, B, k) > m ? band_total(p, B, k) : m;
    return m;
}

}  // namespace

extern "C" {

int64_t l3c_decode_rgb_banded_workspace_bytes(int64_t B, int64_t HW, int64_t band_len, int n_chunks, int lag) {
    if (B <= 0 || HW <= 0 || band_len < 64 || band_len % 64 || n_chunks <= 0 || n_chunks > 64 || (lag != 1 && lag != 2)) return -1;
    const BandPlan p{HW, band_len, (HW + band_len - 1) / band_len, n_chunks};
    const int64_t S = B * p.n;
    return layout(1, banded_max_total(p, B), n_chunks, lag, S).total + up((2 + 3 * (int64_t)n_chunks) * S * 8);
}

int l3c_decode_rgb_banded(const l3c_rgb_banded_desc *r, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    L3C_REQUIRE(r, "null descriptor");
    L3C_REQUIRE(r->P && r->targets && r->sym && r->in && r->in_offsets && r->in_nbytes && r->workspace, "null pointer in descriptor");
    L3C_REQUIRE(r->B > 0 && r->HW > 0 && r->K > 0 && r->K <= 16, "bad shape");
    L3C_REQUIRE(r->band_len >= 64 && r->band_len % 64 == 0, "band_len must be a positive multiple of 64");
    L3C_REQUIRE(r->n_chunks > 0 && r->n_chunks <= 64, "1..64 chunks per band");
    L3C_REQUIRE(r->lag == 1 || r->lag == 2, "lag must be 1 (one stream) or 2 (tables and decoders overlapped on two streams)");
    L3C_REQUIRE(r->lag == 1 || side_stream != main_stream, "lag 2 needs a side stream that is not the main stream");
    L3C_REQUIRE(r->window_mode >= 0 && r->window_mode <= 2, "window_mode: 0 never, 1 auto, 2 always");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(r->workspace) & (ALIGN - 1)) == 0, "workspace must be 256-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(r->in) & 3) == 0 && (reinterpret_cast<uintptr_t>(r->sym) & 1) == 0 &&
                    ((reinterpret_cast<uintptr_t>(r->P) | reinterpret_cast<uintptr_t>(r->targets)) & 3) == 0,
                "misaligned input (streams 4-byte aligned, l3c_container_read)");
    const BandPlan p{r->HW, r->band_len, (r->HW + r->band_len - 1) / r->band_len, r->n_chunks};
    const int64_t S = r->B * p.n;
    L3C_REQUIRE(p.n <= 1024 && S < 65536, "at most 1024 bands per channel and 65535 bands per call");
    L3C_REQUIRE(p.chunks == 1 || p.len(p.n - 1) >= 64 * p.chunks, "every band must hold 64 symbols per chunk");
    const int64_t need = l3c_decode_rgb_banded_workspace_bytes(r->B, r->HW, r->band_len, r->n_chunks, r->lag);
    L3C_REQUIRE(r->workspace_bytes >= need, "workspace too small (l3c_decode_rgb_banded_workspace_bytes)");
    const int64_t max_total = banded_max_total(p, r->B);
    const Layout l = layout(1, max_total, r->n_chunks, r->lag, S);
    int64_t *tables = reinterpret_cast<int64_t *>(static_cast<uint8_t *>(r->workspace) + l.total);
    // the host side of the ragged schedule: every entry's hw (only its maximum is used) and chunk lengths (per step: the longest, the total)
    std::vector<int64_t> hw((size_t)S, r->HW), npix((size_t)(p.chunks * S));
    for (int64_t k = 0; k < p.chunks; ++k)
        for (int64_t e = 0; e < S; ++e) npix[(size_t)(k * S + e)] = p.npix(e % p.n, k);
    const int64_t n_items = p.chunks * S;
    hipLaunchKernelGGL(band_plan_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, l3c::as_stream(main_stream), p, S, tables);
    const int rc = l3c::check_launch("band_plan_kernel");
    if (rc != L3C_OK) return rc;
    l3c_rgb_decode_desc d{};
    d.P = r->P;  d.targets = r->targets;  d.sym = r->sym;  d.B = S;  d.HW = r->HW;  d.K = r->K;
    d.in = r->in;  d.in_offsets = r->in_offsets;  d.in_nbytes = r->in_nbytes;
    d.n_chunks = r->n_chunks;  d.lag = r->lag;  d.window_mode = r->window_mode;
    d.workspace = r->workspace;  d.workspace_bytes = l.total;
    const Ragged rag{hw.data(), nullptr, npix.data(), tables, nullptr};
    return decode_rgb_impl(&d, &rag, max_total, main_stream, side_stream);
}
}

// ---- a set of banded files: every band of every image an ENTRY ---------------------------------------------------------------------
//
// Entry e is pixels [pix0_e, pix0_e + len_e) of an image of hw_e pixels at pixel pixbase_e of the ragged P / symbol buffers: any mix of
// image sizes and band lengths.  All entries step through n_chunks chunks together, entry e in steps of step_e = 64 ceil(len_e / (64 n_chunks))
// symbols: chunk k is [k step_e, min((k + 1) step_e, len_e)) -- EMPTY for the trailing chunks of a short entry (a 64-symbol last band has
// one chunk whatever n_chunks is), and the entry's stream ends with its last non-empty chunk, (len_e - 1) / step_e.
namespace {

using l3c::entry_final_chunk;   // the chunking rule itself: csrc/ac_core.h (tests/hostsim runs it on the host)
using l3c::entry_npix;
using l3c::entry_step;

// One block per chunk k: table_off[k][e] = 514 * (sum of npix[k][e'] over e' < e) needs a scan over the entries -- every thread sums a
// contiguous run of them, thread 0 scans the 256 sums.  ent: pixbase [S] | hw [S] | pix0 [S] | len [S];  tables: the layout of
// l3c_rgb_ragged_desc.tables_dev;  final_chunk [S].  An empty chunk's pix0 stays inside the entry (nothing is read or written there).
__global__ __launch_bounds__(256) void entry_plan_kernel(const int64_t *__restrict__ ent, int64_t S, int64_t chunks,
                                                         int64_t *__restrict__ tables, int32_t *__restrict__ final_chunk) {
    __shared__ int64_t run[256];
    const int64_t k = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t per = (S + 255) / 256;
    const int64_t e0 = t * per < S ? t * per : S, e1 = e0 + per < S ? e0 + per : S;
    const int64_t *len = ent + 3 * S;
    int64_t sum = 0;
    for (int64_t e = e0; e < e1; ++e) sum += entry_npix(len[e], chunks, k);
    run[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t acc = 0;
        for (int i = 0; i < 256; ++i) {
            const int64_t v = run[i];
            run[i] = acc;
            acc += v;
        }
    }
    __syncthreads();
    int64_t off = run[t];
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t n = len[e], st = entry_step(n, chunks), np = entry_npix(n, chunks, k);
        if (k == 0) {
            tables[e] = ent[e];
            tables[S + e] = ent[S + e];
            final_chunk[e] = (int32_t)entry_final_chunk(n, chunks);
        }
        tables[(2 + k) * S + e] = ent[2 * S + e] + (k * st < n ? k * st : n - 1);
        tables[(2 + chunks + k) * S + e] = np;
        tables[(2 + 2 * chunks + k) * S + e] = off * (int64_t)(LP * 2);
        off += np;
    }
}

// per step the total over the entries: the largest sizes the table slots
int64_t entries_max_total(const int64_t *len, int64_t S, int64_t chunks) {
    int64_t m = 0;
    for (int64_t k = 0; k < chunks; ++k) {
        int64_t total = 0;
        for (int64_t e = 0; e < S; ++e) total += entry_npix(len[e], chunks, k);
        m = total > m ? total : m;
    }
    return m;
}

// the workspace: the pipeline's own (its tables sized by max_total), then the plan arrays, then every entry's final chunk
int64_t entries_workspace(int64_t S, int64_t max_total, int n_chunks, int lag) {
    return layout(1, max_total, n_chunks, lag, S).total + up((2 + 3 * (int64_t)n_chunks) * S * 8) + up(S * 4);
}

bool entries_shape_ok(int64_t S, const int64_t *len_host, int n_chunks, int lag) {
    if (S <= 0 || S >= 65536 || !len_host || n_chunks <= 0 || n_chunks > 4096 || (lag != 1 && lag != 2)) return false;
    for (int64_t e = 0; e < S; ++e)
        if (len_host[e] <= 0) return false;
    return true;
}

}  // namespace

extern "C" {

int64_t l3c_decode_rgb_entries_workspace_bytes(int64_t S, const int64_t *len_host, int n_chunks, int lag) {
    if (!entries_shape_ok(S, len_host, n_chunks, lag)) return -1;
    return entries_workspace(S, entries_max_total(len_host, S, n_chunks), n_chunks, lag);
}

int l3c_decode_rgb_entries(const l3c_rgb_entries_desc *r, l3c_stream_t main_stream, l3c_stream_t side_stream) {
    L3C_REQUIRE(r, "null descriptor");
    L3C_REQUIRE(r->P && r->targets && r->sym && r->in && r->in_offsets && r->in_nbytes && r->workspace && r->entries_host && r->entries_dev,
                "null pointer in descriptor");
    L3C_REQUIRE(r->S > 0 && r->S < 65536, "1..65535 entries per call (slice a larger set)");
    L3C_REQUIRE(r->total_pix > 0 && r->K > 0 && r->K <= 16, "bad shape");
    L3C_REQUIRE(r->n_chunks > 0 && r->n_chunks <= 4096, "1..4096 chunks per entry");
    L3C_REQUIRE(r->lag == 1 || r->lag == 2, "lag must be 1 (one stream) or 2 (tables and decoders overlapped on two streams)");
    L3C_REQUIRE(r->lag == 1 || side_stream != main_stream, "lag 2 needs a side stream that is not the main stream");
    L3C_REQUIRE(r->window_mode >= 0 && r->window_mode <= 2, "window_mode: 0 never, 1 auto, 2 always");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(r->workspace) & (ALIGN - 1)) == 0, "workspace must be 256-byte aligned");
    L3C_REQUIRE((reinterpret_cast<uintptr_t>(r->in) & 3) == 0 && (reinterpret_cast<uintptr_t>(r->sym) & 1) == 0 &&
                    ((reinterpret_cast<uintptr_t>(r->P) | reinterpret_cast<uintptr_t>(r->targets)) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(r->entries_dev) & 7) == 0,
                "misaligned input (streams 4-byte aligned, l3c_container_read)");
    const int64_t S = r->S;
    const int64_t *pixbase = r->entries_host, *hw = pixbase + S, *pix0 = hw + S, *len = pix0 + S;
    for (int64_t e = 0; e < S; ++e) {
        L3C_REQUIRE(pixbase[e] >= 0 && hw[e] > 0 && hw[e] <= r->total_pix && pixbase[e] <= r->total_pix - hw[e], "entry: image outside the P / symbol buffers");
        L3C_REQUIRE(pix0[e] >= 0 && len[e] > 0 && len[e] <= hw[e] && pix0[e] <= hw[e] - len[e], "entry: pixel range outside its image, or empty");
    }
    // the host side of the ragged schedule, computed once: every chunk's symbols per entry (the longest sizes a step's launches) and from
    // them the largest total of a step (the table slots, hence the workspace)
    const int64_t chunks = r->n_chunks;
    std::vector<int64_t> npix((size_t)(chunks * S));
    int64_t max_total = 0;
    for (int64_t k = 0; k < chunks; ++k) {
        int64_t total = 0;
        for (int64_t e = 0; e < S; ++e) total += npix[(size_t)(k * S + e)] = entry_npix(len[e], chunks, k);
        max_total = total > max_total ? total : max_total;
    }
    L3C_REQUIRE(r->workspace_bytes >= entries_workspace(S, max_total, r->n_chunks, r->lag), "workspace too small (l3c_decode_rgb_entries_workspace_bytes)");
    const Layout l = layout(1, max_total, r->n_chunks, r->lag, S);
    int64_t *tables = reinterpret_cast<int64_t *>(static_cast<uint8_t *>(r->workspace) + l.total);
    int32_t *final_chunk = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(tables) + up((2 + 3 * chunks) * S * 8));
    hipLaunchKernelGGL(entry_plan_kernel, dim3((unsigned)chunks), dim3(256), 0, l3c::as_stream(main_stream), r->entries_dev, S, chunks, tables,
                       final_chunk);
    const int rc = l3c::check_launch("entry_plan_kernel");
    if (rc != L3C_OK) return rc;
    l3c_rgb_decode_desc d{};
    d.P = r->P;  d.targets = r->targets;  d.sym = r->sym;  d.B = S;  d.HW = 0;  d.K = r->K;
    d.in = r->in;  d.in_offsets = r->in_offsets;  d.in_nbytes = r->in_nbytes;
    d.n_chunks = r->n_chunks;  d.lag = r->lag;  d.window_mode = r->window_mode;
    d.workspace = r->workspace;  d.workspace_bytes = l.total;
    const Ragged rag{hw, nullptr, npix.data(), tables, final_chunk};
    return decode_rgb_impl(&d, &rag, max_total, main_stream, side_stream);
}
}
