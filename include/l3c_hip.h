/*
 * l3c_hip.h -- C ABI of libl3c_hip.so: the MI355X-native (gfx950) L3C inference path.
 *
 * This is the drop-in boundary.  The reference's native FFI for this path is the pybind11 torch
 * extension `torchac_backend_gpu` / `torchac_backend_cpu` (src/torchac/torchac_backend/torchac.cpp:433-443) plus the cuDNN
 * convolutions it reaches through torch.nn; everything below replaces one of those call sites with a HIP kernel behind
 * plain pointers and sizes -- no torch types, no hidden allocation, no hidden synchronisation.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued asynchronously;
 *   - every function returns L3C_OK (0) or a negative status; l3c_last_error() returns a thread-local message;
 *   - buffers are caller-owned; sizes are element counts unless the name says `_bytes`;
 *   - activations are fp32 "pixel-major" (NHWC): element (b, y, x, c) lives at ((b*H + y)*W + x)*cstride + coff + c,
 *     where `cstride` is the number of channels per pixel in memory (lets a conv write a channel slice of a wider tensor);
 *   - symbols are int16, planar (b, c, y*W + x) like the reference hands them to its coder (bitcoding/coders.py:46-51).
 */
#ifndef L3C_HIP_H_
#define L3C_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L3C_OK 0
#define L3C_ERR_INVALID_ARG (-1)
#define L3C_ERR_HIP (-2)
#define L3C_ERR_UNSUPPORTED (-3)

#define L3C_ABI_VERSION 4

typedef void *l3c_stream_t;

/* ---- library ------------------------------------------------------------------------------------------------------ */

int l3c_abi_version(void);
/*
 * Generation of the BITSTREAM this build reads and writes.  The `.l3c` container has no version field (reference:
 * src/bitcoding/bitcoding.py:326-375) and the format is only decodable by a decoder whose kernels reproduce the encoder's P -- and
 * from it the 16-bit table entries -- BIT FOR BIT (the reference's own check is the round trip of
 * src/test/multiscale_tester.py:373).  So every change that alters a bit of P on purpose (a different summation order in a decoder-side
 * convolution, a different transcendental in the mixture head, another compiler contraction setting) bumps this number, and files of
 * an older generation are NOT readable by this build.  tests/golden/hip_*.l3c + hip_bitstream.json are files and P hashes written by the
 * generation they name; tests/test_gpu_bitstream.py fails when today's build no longer decodes them or no longer reproduces the hashes
 * (i.e. when a kernel changed P bits WITHOUT the bump).  `l3c.py enc` prints it.
 *   1  rounds 1-2 (F(2x2,3x3) convolutions)        2  round 3 (F(4x4,3x3), polyphase 5x5)        3  round 5 (fused multiply-adds in the 3->64 head)
 */
#define L3C_BITSTREAM_GENERATION 3
int l3c_bitstream_generation(void);
/* Thread-local description of the last failing call ("" if none). */
const char *l3c_last_error(void);
/* Name / CU count / gcnArchName of the current HIP device; fails when no GPU is visible (there is no CPU fallback). */
int l3c_device_info(char *name_host, int name_cap, int *num_cu_host, char *arch_host, int arch_cap);

/*
 * A HIP stream whose kernels only run on compute units [first_cu, first_cu + n_cu) (hipExtStreamCreateWithCUMask).
 * Used to give the latency-bound range-coder wavefronts CUs of their own while the MFMA-bound conv kernels of the next
 * batch run on the complementary range: co-resident MFMA waves slow the coder's serial chain down 2.3x otherwise.
 */
int l3c_stream_create_cu_range(int first_cu, int n_cu, l3c_stream_t *stream_out_host);
/* The general form: bit i of the mask (32 CUs per word, `mask_host` is a HOST array of n_words words) = compute unit i may run this stream's
 * kernels.  The dispatcher deals workgroups to the 8 XCDs round robin whatever the mask says, so a mask should hold the same number of
 * CUs of every XCD (helpers/runtime.balanced_cu_mask). */
int l3c_stream_create_cu_mask(const uint32_t *mask_host, int n_words, l3c_stream_t *stream_out_host);
int l3c_stream_destroy(l3c_stream_t stream);

/* ---- arithmetic coder (replaces torchac.cpp) ---------------------------------------------------------------------- */

/*
 * Coding interval of one symbol: TWO words, one per role of the lane pair that codes the stream (csrc/ac_core.h):
 * role 0 = c_low, role 1 = 65536 - c_high (c_high in 1..65536).  Interval streams are stored in blocks of 64 symbols,
 * per block and stream one 64-word run per role: word(stream s, symbol t, role r) = iv[(((t/64)*n_streams + s)*2 + r)*64 + t%64],
 * so the kernel that writes them and the lane that codes role r of stream s both touch contiguous 256-byte runs.
 * The buffer is opaque between the l3c_*intervals* call that fills it and the l3c_ac_encode* call that consumes it;
 * l3c_interval_words(n_streams, n_sym) gives its size in uint32 words.
 */
int64_t l3c_interval_words(int64_t n_streams, int64_t n_sym);

/*
 * Intervals from an explicit CDF table (the reference's encode_cdf path, torchac.cpp:263-269 -> encode() :174-182:
 * c_low = cdf[i*Lp + s], c_high = s == Lp-2 ? 0x10000 : cdf[i*Lp + s + 1]).
 *   cdf        uint16 [n_streams][n_sym][Lp] when row_stride == Lp; row_stride == 0 broadcasts ONE row of Lp entries
 *              to every symbol of every stream (uniform prior of the coarsest scale, bitcoding.py:297-323)
 *   sym        int16 [n_streams][n_sym]
 */
int l3c_ac_intervals_from_table(const uint16_t *cdf, int64_t row_stride, int Lp, const int16_t *sym,
                                int64_t n_streams, int64_t n_sym, uint32_t *intervals, l3c_stream_t stream);

/*
 * Range-encode n_streams independent symbol streams of equal length.  Bit-exact restatement of encode()
 * (torchac.cpp:152-227): 32-bit low/high, 16-bit precision, pending-bit carry handling, final flush of `pending+1`
 * bits, zero padding to a byte boundary, MSB-first.  Two launches:
 *   phase 1  one stream per lane PAIR (32 per wavefront; one lane updates low, its neighbour ~high, with the same
 *            ~15 instructions per symbol): the serial interval recurrence only; every interval word is REPLACED IN PLACE
 *            by the bound right after the interval update (low' / ~high'), from which phase 2 derives what is emitted
 *   phase 2  one stream per wavefront, 64 symbols per step: records -> bits (wave scans + LDS merge), coalesced stores
 * Precondition: c_high > c_low for every symbol (strictly increasing table rows), as for the reference.  Intervals that violate it
 * (the entry points cannot validate device-side intervals) produce garbage, as the reference does, but never a store outside the
 * stream's own out_stride_bytes slot: such a stream reports out_nbytes = L3C_AC_OVERRUN when it asked for more.
 *   intervals  in/out, CLOBBERED
 *   out        uint8 [n_streams][out_stride_bytes]; out_stride_bytes % 4 == 0 and >= l3c_ac_max_bytes(n_sym)
 *   out_nbytes uint32 [n_streams]   number of bytes produced per stream, or L3C_AC_OVERRUN
 *   workspace  l3c_ac_encode_workspace_bytes(n_streams) bytes, 4-byte aligned
 */
#define L3C_AC_OVERRUN 0xFFFFFFFFu
int64_t l3c_ac_max_bytes(int64_t n_sym);
int64_t l3c_ac_encode_workspace_bytes(int64_t n_streams);
int l3c_ac_encode(uint32_t *intervals, int64_t n_streams, int64_t n_sym, uint8_t *out, int64_t out_stride_bytes,
                  uint32_t *out_nbytes, void *workspace, l3c_stream_t stream);

/*
 * Grouped form of l3c_ac_encode: ONE phase-1 launch and ONE phase-2 launch cover any number of groups of equally long
 * streams (the four scales of a batch; or every batch of a heterogeneous image set), so all of them are coded concurrently
 * without relying on stream-level concurrency.  Descriptors are given in HOST memory; pointers inside are device pointers.
 *   workspace  l3c_ac_encode_groups_workspace_bytes(n_groups, total number of streams) bytes, 16-byte aligned
 */
typedef struct {
    uint32_t *intervals;       /* in/out, clobbered; l3c_interval_words(n_streams, n_sym) words */
    uint8_t *out;              /* [n_streams][out_stride_bytes] */
    uint32_t *out_nbytes;      /* [n_streams] */
    int64_t n_streams, n_sym, out_stride_bytes;
} l3c_ac_group;
int64_t l3c_ac_encode_groups_workspace_bytes(int n_groups, int64_t total_streams);
int l3c_ac_encode_groups(const l3c_ac_group *groups_host, int n_groups, void *workspace, l3c_stream_t stream);

/*
 * Range-decode n_streams streams, one wavefront per stream (the 64 lanes hold the CDF row of the current symbol and
 * rank the decoder's `count` against it).  Bit-exact restatement of decode() (torchac.cpp:299-381) including the
 * reference binary search (binsearch :276-296) and the skipped state update of the last symbol.
 *   cdf         uint16 rows as above (row_stride == Lp or 0), Lp <= 257
 *   in          uint8, stream s occupies in[in_offsets[s] .. in_offsets[s] + in_nbytes[s]); bits past the end read 0
 *   monotone    1: every row is known to be strictly increasing over [0, Lp-2] (rank == reference binsearch; fast path)
 *               0: use the literal binary search of the reference for every symbol
 *   sym_out     int16 [n_streams][n_sym]
 */
int l3c_ac_decode(const uint16_t *cdf, int64_t row_stride, int Lp, const uint8_t *in, const int64_t *in_offsets,
                  const uint32_t *in_nbytes, int64_t n_streams, int64_t n_sym, int monotone, int16_t *sym_out,
                  l3c_stream_t stream);

/* flag_out[0] |= 1 when some row of the table is not strictly increasing over entries [0, Lp-2]. */
/*
 * Chunked, grouped form of l3c_ac_decode for streams whose tables become available piecewise (the RGB scale: the table of G
 * at a pixel needs R decoded at that pixel, logistic_mixture.py:262-272).  Each part decodes symbols [sym_offset, sym_offset +
 * n_sym) of its streams from the table rows of exactly that range, resuming from / saving the coder state; the 1..8 parts
 * of a call are independent and run side by side in ONE launch pair (R chunk j+2, G chunk j+1, B chunk j of a pipeline step).
 *   cdf                [n_streams][n_sym][Lp] rows of THIS chunk
 *   not_monotone_flag  device int32 (as written by l3c_cdf_check_monotone / l3c_dmll_cdf_table), read by the kernel -- no host
 *                      synchronisation; null: the table is treated as not validated (reference's literal search)
 *   state_in / _out    [n_streams] x l3c_ac_decode_state_bytes(); state_in null = start of the streams; must differ
 *   final_chunk        non-zero when the streams end with this chunk (their last symbol skips the update, torchac.cpp:335-337)
 *   sym_out            stream s writes sym_out[s * sym_stride + sym_offset + i], i < n_sym
 * WINDOW ROWS (ABI version 3; all fields NULL / 0: classic rows).  With window_stats_in set, `cdf` was built by l3c_dmll_cdf_table
 * with the same window_stats array: stream s's rows -- at its full-size slot cdf + s * n_sym * Lp -- are 65-entry WINDOW rows around
 * the mixture's mean when window_stats_in[s] says the stream missed at most 1/64 of the symbols two chunks earlier (0 <= value < 2^30; a
 * quarter of the table arithmetic and bytes of the 257-entry rows), and full rows otherwise.  A symbol outside its window makes the decoder wavefront
 * evaluate the full row of that pixel itself from P / sym_all / targets (the table kernel's device functions: the same bits), so
 * the decoded symbols never depend on the row form.  window_stats_out[s] receives the stream's miss count of THIS chunk (what a window
 * would have missed when the rows were full), bit 30 set when that is more than 1/64 of the chunk's symbols (INT32_MAX when the stream went
 * through the generic pass): feed it to the table call and the
 * decode part of the chunk after the next one.  RGB scale only (Lp == 257, C == 3), one stream per image: stream s = image s of P.
 *   P, sym_all, targets, HW, C, K, c   as for l3c_dmll_cdf_table;   pix0   first pixel of this chunk (sym_all index of symbol 0)
 */
typedef struct {
    const uint16_t *cdf;
    int Lp;
    const uint8_t *in;
    const int64_t *in_offsets;
    const uint32_t *in_nbytes;
    int64_t n_streams, n_sym;
    const int32_t *not_monotone_flag;
    const void *state_in;
    void *state_out;
    int final_chunk;
    int16_t *sym_out;
    int64_t sym_stride, sym_offset;
    const int32_t *window_stats_in;
    int32_t *window_stats_out;
    const float *P;
    const int16_t *sym_all;
    const float *targets;
    int64_t HW, pix0;
    int C, K, c;
    /* RAGGED batches (round 6; all NULL / 0: the rectangular form above).  Streams of DIFFERENT lengths -- the images of a set decode have
     * different sizes -- in one launch: stream s decodes r_npix[s] symbols from the rows at BYTE offset r_table_off[s] of `cdf` (its full-size
     * slot of r_npix[s] * Lp entries) and writes them to sym_out + r_C * r_pixbase[s] + r_c * r_hw[s] + r_pix0[s], i.e. into channel r_c of an
     * image whose r_C planes of r_hw[s] symbols start at element r_C * r_pixbase[s]; P / sym_all of the window fields are indexed the same way
     * (image s: pixels r_pixbase[s] .. + r_hw[s]).  n_sym / sym_stride / sym_offset / HW / pix0 are ignored; r_table_bytes = size of the table. */
    const int64_t *r_npix, *r_table_off, *r_pixbase, *r_hw, *r_pix0;   /* device, [n_streams] each */
    int r_C, r_c;
    int64_t r_table_bytes;
} l3c_ac_decode_part;
int64_t l3c_ac_decode_state_bytes(void);
int l3c_ac_decode_chunks(const l3c_ac_decode_part *parts, int n_parts, l3c_stream_t stream);

int l3c_cdf_check_monotone(const uint16_t *cdf, int64_t n_rows, int Lp, int32_t *flag_out, l3c_stream_t stream);

/*
 * The whole RGB scale of a batch in ONE host call (round 6): the chunk-pipelined decode of R, G and B -- channel c's table at a pixel
 * needs the channels < c decoded at that pixel (reference: criterion/logistic_mixture.py:262-272; the per-channel decoder loop it
 * replaces: bitcoding/bitcoding.py:212-266 -> torchac.cpp:299-381).  Pipeline step t handles chunk t - lag * c of channel c: ONE
 * grouped table launch (l3c_dmll_cdf_table_parts) on `main_stream`, then ONE grouped decoder launch (l3c_ac_decode_chunks) on
 * `side_stream` (lag 2: the tables of step t + 1 are built while step t decodes; lag 1: everything on main_stream, side_stream unused).
 * Returns with everything enqueued and main_stream ordered after the last symbols; no host synchronisation, no allocation: table
 * slots, coder states, validity flags and window statistics live in the caller's workspace (l3c_decode_rgb_workspace_bytes).
 *   P            fp32 pixel-major [B][HW][120] (K = 10: 4 * 3 * K)      targets  fp32 [257]
 *   sym          int16 planar [B][3][HW], ZEROED by the caller; receives the symbols, read back for the lambda coupling
 *   in / in_offsets / in_nbytes   the streams, CHANNEL-major: stream (c, b) at index c * B + b (4-byte aligned, zero padded: l3c_container_read)
 *   chunks       n_chunks (pix0, npix) ranges tiling [0, HW) in order, boundaries on multiples of 64; HOST arrays
 *   window_mode  0: full 257-entry rows; 1: 65-entry window rows wherever the stream's statistics two chunks earlier say that pays
 *                (see l3c_ac_decode_part; the first two chunks of a channel are then decoded on full rows: make them short probes);
 *                2: window rows from the first chunk on (tests)
 */
typedef struct {
    const float *P;
    const float *targets;
    int16_t *sym;
    int64_t B, HW;
    int K;
    const uint8_t *in;
    const int64_t *in_offsets;
    const uint32_t *in_nbytes;
    int n_chunks;
    const int64_t *chunk_pix0_host;
    const int64_t *chunk_npix_host;
    int lag;
    int window_mode;
    void *workspace;
    int64_t workspace_bytes;
} l3c_rgb_decode_desc;
/*
 * The same for a RAGGED batch (round 6): B images of DIFFERENT sizes decoded in lock step -- one grouped table launch and one decoder
 * launch per pipeline step for all of them -- so that a set of differently sized images (the reference's folder evaluation,
 * test/multiscale_tester.py:353-381) is not decoded one latency-bound image after the other.  Every image has the same NUMBER of chunks;
 * image b's chunk j is pixels [chunk_pix0_host[j * B + b], + chunk_npix_host[j * B + b]).  P / sym ragged as for
 * l3c_dmll_cdf_table_ragged with pixbase[b] = sum of hw_host[0 .. b).  `tables_dev`: device int64 array the CALLER has uploaded:
 * pixbase [B] | hw [B] | pix0 [n_chunks][B] | npix [n_chunks][B] | table_off [n_chunks][B], table_off[j][b] = 514 * sum of npix[j][0 .. b).
 */
typedef struct {
    const float *P;
    const float *targets;
    int16_t *sym;
    int64_t B;
    const int64_t *hw_host;
    int K;
    const uint8_t *in;
    const int64_t *in_offsets;
    const uint32_t *in_nbytes;
    int n_chunks;
    const int64_t *chunk_pix0_host;
    const int64_t *chunk_npix_host;
    const int64_t *tables_dev;
    int lag;
    int window_mode;
    void *workspace;
    int64_t workspace_bytes;
} l3c_rgb_ragged_desc;
int64_t l3c_decode_rgb_ragged_workspace_bytes(int64_t B, int64_t max_chunk_total_npix, int n_chunks, int lag);
int l3c_decode_rgb_ragged(const l3c_rgb_ragged_desc *desc_host, l3c_stream_t main_stream, l3c_stream_t side_stream);
int64_t l3c_decode_rgb_workspace_bytes(int64_t B, int64_t max_chunk_npix, int n_chunks, int lag);
/* byte offset, inside the workspace, of the window statistics int32 [3][n_chunks + 2][B] (slot j + 2 = what chunk j's decoders reported; tests) */
int64_t l3c_decode_rgb_stats_offset(int64_t B, int64_t max_chunk_npix, int n_chunks, int lag);
int l3c_decode_rgb(const l3c_rgb_decode_desc *desc_host, l3c_stream_t main_stream, l3c_stream_t side_stream);
/*
 * The RGB scale of a batch of BANDED files (see l3c_ac_band_intervals): every band of every image is a stream of its own, and the chunk
 * pipeline above runs over all of them in lock step -- pipeline step t builds the tables of chunk t - lag * c of channel c for EVERY band
 * in one launch and resumes every band's decoder in one launch.  Band j of image b is decoded as the ragged entry (pixbase b * HW,
 * hw HW, chunk k at pixel j * L + k * step_j), so P / sym / window rows are indexed exactly as for the rectangular batch.
 *   P, targets, sym, B, HW, K, lag, window_mode   as for l3c_rgb_decode_desc
 *   in / in_offsets / in_nbytes   the B * 3 * n band streams: stream (c, b, j) at index (c * B + b) * n + j, n = ceil(HW / band_len)
 *   band_len     L, a multiple of 64;  n_chunks  chunks per band (1 .. 64): every band must hold at least 64 * n_chunks symbols when n_chunks > 1
 * B * n < 65536.  Nothing is read from the host after the call returns; the per-band descriptors live in the workspace and are written by
 * a kernel on main_stream.
 */
typedef struct {
    const float *P;
    const float *targets;
    int16_t *sym;
    int64_t B, HW;
    int K;
    const uint8_t *in;
    const int64_t *in_offsets;
    const uint32_t *in_nbytes;
    int64_t band_len;
    int n_chunks;
    int lag;
    int window_mode;
    void *workspace;
    int64_t workspace_bytes;
} l3c_rgb_banded_desc;
int64_t l3c_decode_rgb_banded_workspace_bytes(int64_t B, int64_t HW, int64_t band_len, int n_chunks, int lag);
int l3c_decode_rgb_banded(const l3c_rgb_banded_desc *desc_host, l3c_stream_t main_stream, l3c_stream_t side_stream);
/*
 * The RGB scale of a SET of banded files -- images of different sizes, band lengths that differ from image to image -- as S arbitrary
 * ENTRIES in lock step: entry e is pixels [pix0_e, pix0_e + len_e) of an image of hw_e pixels that starts at pixel pixbase_e of the ragged
 * P ([total_pix][120]) and symbol buffers (the image's 3 planes of hw_e symbols from element 3 * pixbase_e; ZEROED by the caller).  Every
 * entry is cut into n_chunks chunks of step_e = 64 * ceil(len_e / (64 * n_chunks)) symbols: chunk k covers [k step_e, min((k + 1) step_e,
 * len_e)), the trailing chunks of a short entry are EMPTY (its decoder only carries its state on) and its stream ends with its last
 * non-empty chunk -- so a 64-symbol band beside a 32 768-symbol one does not pull the whole call down to one chunk.
 *   entries_dev / entries_host   the same int64 table on the device and on the host: pixbase [S] | hw [S] | pix0 [S] | len [S]; the host copy
 *                is checked against total_pix and sizes the launches, and is not read after the call returns
 *   in / in_offsets / in_nbytes   the 3 S streams, CHANNEL-major: stream (c, e) at index c * S + e (4-byte aligned, zero padded)
 *   K, lag, window_mode   as for l3c_rgb_decode_desc (window rows follow every entry's own statistics two of ITS chunks earlier)
 * S < 65536 (slice a larger set).  The chunk plan (the layout of l3c_rgb_ragged_desc.tables_dev, then every entry's final chunk) is written
 * into the workspace by a kernel on main_stream; nothing synchronises with the host.
 */
typedef struct {
    const float *P;
    const float *targets;
    int16_t *sym;
    int64_t S;
    int64_t total_pix;
    const int64_t *entries_dev;
    const int64_t *entries_host;
    int K;
    const uint8_t *in;
    const int64_t *in_offsets;
    const uint32_t *in_nbytes;
    int n_chunks;
    int lag;
    int window_mode;
    void *workspace;
    int64_t workspace_bytes;
} l3c_rgb_entries_desc;
int64_t l3c_decode_rgb_entries_workspace_bytes(int64_t S, const int64_t *len_host, int n_chunks, int lag);
int l3c_decode_rgb_entries(const l3c_rgb_entries_desc *desc_host, l3c_stream_t main_stream, l3c_stream_t side_stream);

/* ---- logistic-mixture head (replaces torchac_kernel.cu + criterion/logistic_mixture.py on the coding path) --------- */

/*
 * Per-channel mixture parameters, the reference's CDFOut (logistic_mixture.py:134-141, :248-275):
 *   P      fp32 pixel-major [B][HW][Kp], Kp = (rgb ? 4 : 3) * C * K, channel index p*(C*K) + c*K + k
 *   sym    int16 planar [B][C][HW]; only read for rgb && c > 0 (lambda coupling with the ACTUAL values of the previous
 *          channels: mu_G += sigmoid(lam_0) x_R, mu_B += sigmoid(lam_1) x_R + sigmoid(lam_2) x_G)
 *   out    pi (softmax over K), mu, log_sigma (clamped at -7): fp32 planar [B][K][HW] each -- the 1KHW layout of CDFOut
 */
int l3c_dmll_channel_params(const float *P, const int16_t *sym, int64_t B, int64_t HW, int C, int K, int rgb, int c,
                            float *pi, float *mu, float *log_sigma, l3c_stream_t stream);

/*
 * uint16 CDF table of a logistic mixture -- calculate_cdf_kernel (torchac_kernel.cu:26-76) / _get_uint16_cdf
 * (torchac.py:174-213):  cdf[n][l] = uint16(lrintf(sum_k pi[k][n] * sigmoid((t[l] - mu[k][n]) * exp(-ls[k][n]))
 *                                                  * (65536 - (Lp - 1))) + l)
 *   targets fp32 [Lp]; pi, mu, log_sigma fp32 planar [n_img][K][HW]; cdf uint16 [n_img][HW][Lp]
 *   not_monotone (may be NULL) int32, |= 1 if a row is not strictly increasing over [0, Lp-2]
 */
int l3c_cdf_table_mixture(const float *targets, const float *pi, const float *mu, const float *log_sigma,
                          int64_t n_img, int64_t HW, int K, int Lp, uint16_t *cdf, int32_t *not_monotone,
                          l3c_stream_t stream);

/*
 * Decoder, fused: the uint16 table rows of channel c for pixels [pix0, pix0 + npix) of every image, straight from P and the
 * symbols of the channels decoded so far (l3c_dmll_channel_params + l3c_cdf_table_mixture in one pass; identical entries).
 *   cdf [B][npix][Lp];  not_monotone: optional flag, set (never cleared) if a row is not strictly increasing
 *   window_stats (ABI version 3; NULL: every row a full row): int32 [B], see l3c_ac_decode_part -- image b's rows are 65-entry
 *   window rows (entries 0..63 = cdf[w0 .. w0 + 63], entry 64 = the window's offset w0) packed from the start of its full-size slot
 *   cdf + b * npix * Lp when 0 <= window_stats[b] < 2^30; otherwise full rows whose (never read) entry Lp - 1
 *   carries w0.  Lp must be 257.
 */
int l3c_dmll_cdf_table(const float *P, const int16_t *sym, const float *targets, int64_t B, int64_t HW, int C, int K, int rgb,
                       int c, int64_t pix0, int64_t npix, int Lp, uint16_t *cdf, int32_t *not_monotone, const int32_t *window_stats,
                       l3c_stream_t stream);

/*
 * Grouped form (round 6): the tables of 1..8 parts -- the channels of one pipeline step of the RGB decode, each over its own pixel
 * range, or the C channels of a bottleneck scale -- in ONE launch.  Parts share P, sym, targets and the shape; every part's arguments as
 * for l3c_dmll_cdf_table.  `parts_host` is a HOST array.
 */
typedef struct {
    int c;
    int64_t pix0, npix;
    uint16_t *cdf;               /* [B][npix][Lp] */
    int32_t *not_monotone;       /* may be NULL */
    const int32_t *window_stats; /* may be NULL */
} l3c_table_part;
int l3c_dmll_cdf_table_parts(const float *P, const int16_t *sym, const float *targets, int64_t B, int64_t HW, int C, int K, int rgb,
                             int Lp, const l3c_table_part *parts_host, int n_parts, l3c_stream_t stream);
/*
 * RAGGED form (round 6): the images of the batch have DIFFERENT sizes -- P is [sum_b HW_b][Kp] with image b's pixels from pixel pixbase[b]
 * on, sym holds image b's C planes of HW_b symbols from element C * pixbase[b] on -- and every part gives, per image, its own pixel
 * range and the byte offset of its rows in the part's table.  parts_host[i].pix0 is ignored, .npix = the LONGEST range of the part.
 */
typedef struct {
    int64_t B;                 /* images */
    int64_t max_hw;            /* the largest HW_b */
    const int64_t *pixbase;    /* device [B] */
    const int64_t *hw;         /* device [B] */
} l3c_ragged_batch;
typedef struct {
    const int64_t *pix0;       /* device [B]: first pixel of image b's range of this part */
    const int64_t *npix;       /* device [B]: its length (0: nothing for this image) */
    const int64_t *table_off;  /* device [B]: BYTE offset of image b's rows inside the part's table */
} l3c_ragged_part;
int l3c_dmll_cdf_table_ragged(const float *P, const int16_t *sym, const float *targets, const l3c_ragged_batch *batch_host, int C, int K,
                              int rgb, int Lp, const l3c_table_part *parts_host, const l3c_ragged_part *ragged_parts_host, int n_parts,
                              l3c_stream_t stream);

/*
 * Fused encoder head: straight from the network output P and the symbols to the packed coding intervals of every
 * channel of one scale -- only the two table entries the encoder reads (torchac.cpp:180-181) are evaluated, with the
 * same per-entry arithmetic as l3c_cdf_table_mixture, so the result is bit-identical to building the table first.
 *   stream index = b*C + c, n_streams = B*C, n_sym = HW; intervals sized by l3c_interval_words(B*C, HW)
 */
int l3c_dmll_encode_intervals(const float *P, const int16_t *sym, const float *targets, int64_t B, int64_t HW, int C,
                              int K, int rgb, int Lp, uint32_t *intervals, l3c_stream_t stream);

/*
 * Negative log-likelihood map of DiscretizedMixLogisticLoss.forward (logistic_mixture.py:146-207):
 *   x      fp32 planar [B][C][HW] targets (pixel values for rgb, bottleneck values for z scales)
 *   nll    fp32 planar [B][C][HW], nats
 */
int l3c_dmll_nll(const float *P, const float *x, int64_t B, int64_t HW, int C, int K, int rgb, float x_min,
                 float x_max, int L, float *nll, l3c_stream_t stream);

/*
 * Sample from the mixture (DiscretizedMixLogisticLoss._non_shared_sample, logistic_mixture.py:277-323): component by
 * Gumbel-max over the logits, value by the inverse logistic CDF; rgb: lambda coupling with the chosen components + clamp to
 * [0, 255].  The uniforms are inputs (the reference draws them with uniform_(1e-5, 1 - 1e-5), :286, :300):
 *   u_mix       fp32 planar [B][C][K][HW]        u_logistic  fp32 planar [B][C][HW]        x  fp32 planar [B][C][HW] (not rounded)
 */
int l3c_dmll_sample(const float *P, const float *u_mix, const float *u_logistic, int64_t B, int64_t HW, int C, int K,
                    int rgb, float *x, l3c_stream_t stream);

/*
 * The mixture's MEAN as symbols: the estimator of the preview decode (INTEGRATION.md "Preview decode"), for a scale whose record is not
 * decoded.  It stands beside the reference's sampling (logistic_mixture.py:277-323, driven by multiscale_network.py:328-406), which
 * draws a value per pixel where this takes the expectation.  Per pixel, channels in order c = 0 .. C-1:
 *   pi_k = softmax_k(logit_c,k)     m_c = sum_k pi_k mu'_c,k     mu' = mu (+ the lambda coupling of l3c_dmll_channel_params, rgb only,
 *                                                                      evaluated on the ESTIMATED values of the channels below c)
 *   v = fminf(fmaxf(m_c, x_min), x_max)  (a NaN becomes x_min)     sym_c = clamp(rintf((v - x_min) / bin_width), 0, L-1)  (ties to even)
 *   value fed on: sym_c * bin_width + x_min (l3c_sym_to_bn)        bin_width = (x_max - x_min) / (L - 1);  log_sigma plays no part
 *   sym_out    int16 planar [B][C][HW]: the form the range decoders write.  2 <= L <= 32768.
 * The kernel is pixel-wise: a ragged P [sum_b HW_b][Kp] is B = 1, HW = sum_b HW_b.  Not part of the bitstream.
 */
int l3c_dmll_mean(const float *P, int64_t B, int64_t HW, int C, int K, int rgb, float x_min, float x_max, int L,
                  int16_t *sym_out, l3c_stream_t stream);

/*
 * CONCEALMENT (INTEGRATION.md "Salvage decode"): the estimator of l3c_dmll_mean on pixel SPANS of decoded RGB symbols, conditioned on the
 * channels that are kept.  RGB scale only: C = 3, lambda-coupled, P [B][HW][12 K].  Per pixel of a span, channels in the order R, G, B:
 *   bit c of `replace` clear   x_c = sym_c * bin_width + x_min of the symbol already in `sym`; that symbol is read, never written
 *   bit c set                  sym_c = the snapped m_c of l3c_dmll_mean, its coupling evaluated on the x_c' of the channels below -- kept or
 *                              estimated --, x_c = sym_c * bin_width + x_min; sym_c is stored
 * The device code is l3c_dmll_mean's: a span with replace == 7 gives, bit for bit, what l3c_dmll_mean gives on those pixels.
 * One launch serves all spans: a block takes 64 pixels of one span (grid.y = the span, grid.x = the tiles of the longest).  Nothing outside
 * the spans is read from `sym` or written, and no record of P outside them is fetched.  Overlapping spans are the caller's error.
 *   spans_host   the table on the host, validated before anything is launched (an error names the span)
 *   spans        the caller's device copy of the same table, 8-byte aligned
 *   span         0 <= image < B, pix0 % 64 == 0 and >= 0, npix >= 0, pix0 + npix <= HW, replace < 8, reserved == 0
 *   sym          int16 planar [B][3][HW], in/out
 * n_spans in 0 .. 65535.  n_spans == 0, or every span empty or with replace == 0: success, nothing is launched.
 */
typedef struct l3c_conceal_span {
    int64_t image, pix0, npix;
    uint32_t replace, reserved;     /* replace: bit c set = channel c is overwritten */
} l3c_conceal_span;
int l3c_dmll_conceal(const float *P, int64_t B, int64_t HW, int K, float x_min, float x_max, int L, const l3c_conceal_span *spans_host,
                     const l3c_conceal_span *spans, int64_t n_spans, int16_t *sym /* in/out, planar [B][3][HW] */, l3c_stream_t stream);

/* ---- convolution stack (replaces the cuDNN convs behind modules/{net,edsr,head,prob_clf}.py) ---------------------- */

/*
 * Weight pre-packing for l3c_conv_mfma: w_oihw fp32 [Cout][Cin][KS][KS] (the checkpoint layout) -> MFMA fragment
 * order.  l3c_conv_packed_words gives the size of `packed` in floats.  Cin % 16 == 0.
 */
int64_t l3c_conv_packed_words(int Cout, int Cin, int KS);
int l3c_conv_pack_weights(const float *w_oihw, int Cout, int Cin, int KS, float *packed, l3c_stream_t stream);

#define L3C_EPI_RELU 1         /* max(0, .) after the bias */
#define L3C_EPI_RESIDUAL 2     /* += residual[pixel][cout] after bias (and relu) */
#define L3C_EPI_PIXEL_SHUFFLE 4 /* out[(2y+i, 2x+j)][n>>2] = conv[(y,x)][n], i = (n>>1)&1, j = n&1 (nn.PixelShuffle(2)) */

typedef struct {
    const float *in;       /* [B][Hin][Win][in_cstride], channels in_coff .. in_coff+Cin */
    int in_cstride, in_coff;
    const float *packed_w; /* from l3c_conv_pack_weights */
    const float *bias;     /* [Cout] */
    const float *residual; /* [B][Hout][Wout][res_cstride] (+res_coff), or NULL */
    int res_cstride, res_coff;
    float *out;            /* [B][Hout][Wout][out_cstride] (+out_coff); with PIXEL_SHUFFLE: [B][2Hout][2Wout][..] */
    int out_cstride, out_coff;
    int B, Hin, Win, Cin, Cout;
    int KS;                /* 1, 3 or 5 */
    int stride;            /* 1, or 2 (KS == 5 only) */
    int dilation;          /* 1, 2 or 4 (KS == 3 only); padding is KS/2 when dilation == 1 else dilation */
    int epilogue;          /* L3C_EPI_* flags */
} l3c_conv_desc;

/* fp32 implicit-GEMM convolution on v_mfma_f32_32x32x2_f32; Cin % 16 == 0 (64 or 192 on this path). */
int l3c_conv_mfma(const l3c_conv_desc *desc_host, l3c_stream_t stream);
/*
 * The same convolution by Winograd F(4x4, 3x3) (interpolation points 0, 1, -1, 1/2, -2, inf): 4x fewer multiplications than the
 * direct form; the 36 per-position GEMMs on v_mfma_f32_16x16x4_f32, output transform in registers.
 * `packed_w` must come from l3c_conv_wino4_pack_weights (G g G^T computed in double precision, l3c_conv_wino4_packed_words(Cout,
 * Cin) floats).  Replaces the cuDNN call sites of the 3x3 layers (modules/edsr.py:63-89, net.py:136-148, :173-184,
 * prob_clf.py:71-74); differs from the direct convolution by fp32 rounding (measured: the L3C forward stays within 5e-6 of the
 * fp32 reference relative to each tensor's largest magnitude, profiles/r03_wino_f43_numerics.log).  Cin % 16 == 0; input and
 * packed weights 16-byte aligned, input channel stride / offset multiples of 4; output / residual: any channel slice.
 * L3C_EPI_PIXEL_SHUFFLE (the 64 -> 256 tail of edsr.Upsampler + nn.PixelShuffle(2), ABI version 3): Cout == 256, and `packed_w` must be
 * packed from the weights in SUB-PIXEL-MAJOR order -- row 64 s + oc of the tensor handed to l3c_conv_wino4_pack_weights = row 4 oc + s of
 * the layer's OIHW weights (s = 2 i + j: the sub-pixel, oc: the output channel) -- so that block s of a tile computes 64 adjacent output
 * channels of one sub-pixel and stores 64-byte runs; `bias` stays in the layer's own order.
 */
int64_t l3c_conv_wino4_packed_words(int Cout, int Cin);
int l3c_conv_wino4_pack_weights(const float *w_oihw, int Cout, int Cin, float *packed, l3c_stream_t stream);
int l3c_conv_wino4(const l3c_conv_desc *desc_host, l3c_stream_t stream);
/*
 * One phase of a STRIDE-2 convolution in its polyphase form (the 5x5 stride-2 padding-2 `down` layers, reference net.py:102,141):
 *     out[y][x] = sum_{i,j} w[i][j] in[2y-2+i][2x-2+j]  =  sum over the four input phases (a, b) of a 3x3, padding-1, stride-1
 * convolution of the sub-grid in[2r+a][2c+b] with the phase kernel w_ab[u][v] = w[2u+a][2v+b] (zero where 2u+a or 2v+b > 4) -- each
 * of which runs on the F(4x4,3x3) kernel: 9 instead of 25 multiplications per output (4 x 36/16).  desc: KS = 3, stride = 2,
 * dilation 1, Hin / Win = the FULL-resolution input (even), `packed_w` = l3c_conv_wino4_pack_weights of the phase kernel, output
 * [B][Hin/2][Win/2][..]; epilogue 0 or L3C_EPI_RESIDUAL (the caller accumulates the phases: the first launch carries the bias, the
 * other three a zero bias and residual == out, in place).
 */
int l3c_conv_wino4_phase(const l3c_conv_desc *desc_host, int phase_y, int phase_x, l3c_stream_t stream);
/*
 * The same 5x5 stride-2 padding-2 convolution with ALL FOUR phases in one launch: the kernel's chunk sequence runs through the phases
 * (input channels of phase (0,0), then (0,1), (1,0), (1,1)), so there is one output transform and no read-modify-write of the
 * output.  desc: KS = 5, stride = 2, Cin = the input's channels, bias-only epilogue; `packed_w` = l3c_conv_wino4_pack_weights(w_cat,
 * Cout, 4 * Cin) of the four phase kernels concatenated along the INPUT-channel axis, phase-major: w_cat[:, (2a+b) Cin + ci] = w_ab[:, ci].
 */
int l3c_conv_wino4_stride2(const l3c_conv_desc *desc_host, l3c_stream_t stream);
int l3c_conv_wino4_set_tiles_per_block(int n);
/*
 * Pointwise (KS == 1, stride 1) convolution Cin -> Cout <= 160 as a pixel x channel GEMM on the fp32 MFMA: the 192 -> Kp layer that
 * ends every probability classifier (reference prob_clf.py:71-74).  `packed_w` must come from l3c_conv_pw_pack_weights
 * (l3c_conv_pw_packed_words(Cout, Cin) floats).  Cin % 64 == 0; bias only (epilogue == 0); input / weights 16-byte aligned and
 * input channel stride / offset multiples of 4.  Differs from l3c_conv_mfma by the order of the Cin-term sums only.
 */
int64_t l3c_conv_pw_packed_words(int Cout, int Cin);
int l3c_conv_pw_pack_weights(const float *w_oi, int Cout, int Cin, float *packed, l3c_stream_t stream);
int l3c_conv_pw(const l3c_conv_desc *desc_host, l3c_stream_t stream);
/* Same contract on plain VALU FMAs with unpacked OIHW weights (packed_w = w_oihw): a device-side cross-check. */
int l3c_conv_direct(const l3c_conv_desc *desc_host, l3c_stream_t stream);

/*
 * RGB head: img planar fp32 [B][3][H][W] (0..255) -> sub_rgb_mean (1x1, 3->3) -> MeanShift(1/128) (1x1, 3->3) ->
 * conv 3x3 3->Cf, zero padding applied to the mean-shifted image.  (multiscale_network.py:241, head.py:26-41)
 *   w1,b1  sub_rgb_mean [3][3],[3];  w2,b2 heads.0.head.0 [3][3],[3];  w3 [Cf][3][3][3], b3 [Cf];  out pixel-major
 * shifted_out (may be NULL): planar [B][3][H][W], the input of the 3x3 conv, for stage-wise parity tests.
 */
int l3c_rgb_head(const float *img, const float *w1, const float *b1, const float *w2, const float *b2,
                 const float *w3, const float *b3, int B, int H, int W, int Cf, float *out, float *shifted_out,
                 l3c_stream_t stream);

/*
 * Encoder output: 1x1 conv Cf -> C (`to_q`, net.py:113-121) fused with the hard quantiser (quantizer.py:72-87:
 * symbols = argmin_l (x - levels_l)^2, first minimum wins; x_hard = levels[symbols]).
 *   feat pixel-major [B][HW][Cf]; w [C][Cf], b [C], levels [L]
 *   sym int16 planar [B][C][HW]; bn_q fp32 planar [B][C][HW]; bn (may be NULL) pre-quantisation values, planar
 */
int l3c_to_q_quantize(const float *feat, const float *w, const float *b, const float *levels, int64_t B, int64_t HW,
                      int Cf, int C, int L, int16_t *sym, float *bn_q, float *bn, l3c_stream_t stream);

/*
 * Decoder input: 1x1 conv C -> Cf on the quantised bottleneck (+ the coarser decoder's features), net.py:178-180.
 *   bn_q planar [B][C][HW]; w [Cf][C], b [Cf]; fuse pixel-major [B][HW][Cf] or NULL; out pixel-major [B][HW][Cf]
 *   Limits: C <= 8 (the bottleneck's weights live in registers; q.C is 5 or 3 in every shipped config), Cf % 4 == 0 and
 *   256 % (Cf / 4) == 0, HW < 2^31.  Anything else returns L3C_ERR_INVALID_ARG.
 */
int l3c_dec_head(const float *bn_q, const float *w, const float *b, const float *fuse, int64_t B, int64_t HW, int C,
                 int Cf, float *out, l3c_stream_t stream);

/*
 * RGB baselines (BicubicSubsampling encoder, modules/net.py:65-80): the reference leaves the GPU for PIL's BICUBIC resize
 * (dataloaders/images_loader.py:277-288).  Here the pyramid stays on the device and is bit-exact with Pillow:
 *   l3c_meanshift_planar  1x1 conv 3->3 on a planar image (sub_rgb_mean, multiscale_network.py:241); w [3][3], b [3] on device
 *   l3c_rgb_to_u8         uint8(round(clamp(x + mean, 0, 255)))                      planar fp32 [B][3][HW] -> uint8
 *   l3c_resample_u8       ONE pass of Pillow's ImagingResample (8 bpc, 22-bit fixed point) along W (axis 0) or H (axis 1);
 *                         bounds int32 [out_size][2] = (first, count), kk int32 [out_size][ksize], both on the device,
 *                         computed on the host exactly as Pillow does (helpers/pil_resample.py)
 *   l3c_u8_to_sym_bn      symbols (int16) = pixel values, bn = value - mean
 * `mean3_host` is a HOST pointer to the three channel means (0.4488, 0.4371, 0.4040) * 255 as fp32.
 */
int l3c_meanshift_planar(const float *img, const float *w, const float *b, int64_t B, int64_t HW, float *out,
                         l3c_stream_t stream);
int l3c_rgb_to_u8(const float *x, const float *mean3_host, int64_t B, int64_t HW, uint8_t *out, l3c_stream_t stream);
int l3c_resample_u8(const uint8_t *in, int64_t planes, int H, int W, int axis, int out_size, const int32_t *bounds,
                    const int32_t *kk, int ksize, uint8_t *out, l3c_stream_t stream);
int l3c_u8_to_sym_bn(const uint8_t *in, const float *mean3_host, int64_t B, int64_t HW, int16_t *sym, float *bn,
                     l3c_stream_t stream);

/*
 * `.l3c` file assembly on the device (the byte format of bitcoding/bitcoding.py:326-375): writes the B files of a batch back
 * to back into `dst` -- file b at dst + file_offset[b] -- from the coder's per-scale output rows:
 *     u16 x4 padding | for scale = coarsest .. 0:  u8 C, u16 H, u16 W | per channel: u32 nbytes, payload | 46 E2 84 92
 *   scales       coarsest first (file order), HOST array; pointers inside are device pointers
 *   padding      device uint16 [B][4]: left, right, top, bottom          file_offset  device int64 [B]
 * File b is 8 + sum_scales (5 + 4*C + 4) + its payload bytes long; the caller sizes `dst` and scans the offsets.
 */
typedef struct {
    const uint8_t *out;       /* [B*C][stride], as written by l3c_ac_encode(_groups) */
    const uint32_t *nbytes;   /* [B*C] */
    int64_t stride;
    int C, H, W;
} l3c_container_scale;
int l3c_container_write(const l3c_container_scale *scales, int n_scales, int64_t B, const uint16_t *padding,
                        const int64_t *file_offset, uint8_t *dst, l3c_stream_t stream);

/*
 * The inverse for the decoder (round 6): the entropy-coded streams of MANY files, which lie at arbitrary byte offsets inside the files
 * (bitcoding.py:326-375: u32 nbytes + payload per channel), copied out of ONE device buffer holding the raw files into the form the
 * range decoder reads -- every stream 4-byte aligned and followed by at least 4 zero bytes (bits past the end read 0, torchac.cpp:96-128).
 * The host parses only the framing (a few length fields per file) and uploads the files as they are, in one copy.
 *   files        the raw bytes of the files, back to back (device), 4-byte aligned and readable up to the next multiple of 4 of its size
 *   src_offset   int64 [n_streams]: byte position of stream s's payload inside `files`
 *   dst_offset   int64 [n_streams]: byte position of stream s inside `dst`, a multiple of 4; the caller leaves ((nbytes + 3) / 4) * 4 + 4
 *                bytes per stream, all of which are written (payload, then zeros)
 *   nbytes       uint32 [n_streams];   max_nbytes   the largest of them (the host has read every length field: it sizes the launch)
 */
int l3c_container_read(const uint8_t *files, const int64_t *src_offset, const int64_t *dst_offset, const uint32_t *nbytes,
                       int64_t n_streams, uint32_t max_nbytes, uint8_t *dst, l3c_stream_t stream);

/*
 * BANDED files ("Banded .l3c files"): a channel's raster-order stream of H*W symbols is cut into n = ceil(H*W / L) bands of L
 * consecutive pixels (L % 64 == 0), each coded as a stream of its own -- the same symbols and table rows, n independent chains.
 *
 * l3c_ac_band_intervals re-lays the interval buffer of n_streams streams of n_sym symbols (as filled by l3c_dmll_encode_intervals /
 * l3c_ac_intervals_from_table) into the two groups l3c_ac_encode_groups codes: the FULL bands -- stream (s, j) at index s * (n - 1) + j,
 * L symbols, l3c_interval_words(n_streams * (n - 1), L) words; NULL when n == 1 -- and the LAST band of every stream -- stream s,
 * n_sym - (n - 1) * L symbols, l3c_interval_words(n_streams, that) words.  A pure copy of 512-byte runs; `intervals` is not modified.
 */
int l3c_ac_band_intervals(const uint32_t *intervals, int64_t n_streams, int64_t n_sym, int64_t band_len, uint32_t *full_out,
                          uint32_t *last_out, l3c_stream_t stream);

/*
 * The banded file assembly:  'L3CB' | u8 version 1 | u8 0 | u16 x4 padding | for scale = coarsest .. 0:  u8 C, u16 H, u16 W, u32 L |
 * for channel c: for band j: u32 nbytes, payload | 46 E2 84 92.   Per scale the coder output of the two groups of l3c_ac_band_intervals;
 * file b is 14 + sum_scales (9 + 4 * C * n + 4) + its payload bytes long.  `workspace`: l3c_container_write_banded_workspace_bytes(scales,
 * n_scales, B) bytes (the length fields' positions), 8-byte aligned.
 */
typedef struct {
    const uint8_t *out_full;        /* [B*C*(n-1)][stride_full], NULL when n == 1 */
    const uint32_t *nbytes_full;    /* [B*C*(n-1)] */
    int64_t stride_full;
    const uint8_t *out_last;        /* [B*C][stride_last] */
    const uint32_t *nbytes_last;    /* [B*C] */
    int64_t stride_last;
    int C, H, W;
    int64_t band_len;               /* L: L % 64 == 0, ceil(H*W / L) <= 1024 */
} l3c_banded_scale;
int64_t l3c_container_write_banded_workspace_bytes(const l3c_banded_scale *scales, int n_scales, int64_t B);
int l3c_container_write_banded(const l3c_banded_scale *scales, int n_scales, int64_t B, const uint16_t *padding,
                               const int64_t *file_offset, uint8_t *dst, void *workspace, int64_t workspace_bytes,
                               l3c_stream_t stream);

/* symbols -> bottleneck values, to_bn (quantizer.py:44-47): float(S) * bin + x_min, two separately rounded fp32 ops. */
int l3c_sym_to_bn(const int16_t *sym, int64_t n, float bin_width, float x_min, float *bn, l3c_stream_t stream);

/* ---- the whole network (replaces modules/multiscale_network.py forward / get_P) ------------------------------------ */

/*
 * MultiscaleNetwork.forward and .get_P (reference modules/multiscale_network.py:226-306, :308-322) as ONE library call each: the
 * library runs the layer schedule of l3c-pytorch_amd/modules/multiscale_network.py -- the same entry points with the same descriptors
 * in the same order (l3c_rgb_head, l3c_conv_wino4 for every 3x3 layer, l3c_conv_wino4_stride2 for the 5x5 stride-2 `down` layers,
 * l3c_conv_pw for the 1x1 192 -> Kp classifier outputs, l3c_to_q_quantize, l3c_dec_head) -- so P is bit-identical to the Python
 * schedule's and files written through either decode with the other.
 *
 * Model families: L3C (EDSRLikeEnc with enc.feed_F and dec.skip, configs/ms/cr.cf) and the RGB / RGB Shared baselines
 * (BicubicSubsampling, cr_rgb.cf / cr_rgb_shared.cf: no heads and no encoders, q.C == 3, Kp = 12 K at every scale).  l3c_net_forward
 * covers L3C only (the baselines' bicubic pyramid is driven by tables computed on the host); l3c_net_get_p covers both.
 * Supported shapes (anything else: L3C_ERR_UNSUPPORTED): Cf == 64, C <= 8, Kp <= 160 at every scale, image sides multiples of
 * 2^num_scales, H * W * Cf * 4 < 0x7ffffff0 bytes per image, B < 65536 and B * H * W < 2^31.
 * Every pointer must be 16-byte aligned; all arguments are checked before anything is enqueued.  The only global state read is that
 * of the convolution entries (l3c_conv_wino4_set_tiles_per_block); two calls on two streams with separate workspaces and outputs may
 * share one packed buffer.
 */
#define L3C_NET_MAX_SCALES 4
typedef struct {
    int num_scales;            /* 3 in cr.cf, 1 in cr_rgb_shared.cf */
    int Cf, C, L, K;           /* Cf, q.C, q.L, prob.K */
    int enc_blocks, dec_blocks;
    int rgb_baseline;          /* 1: BicubicSubsampling configs (cr_rgb*.cf): no heads / encoders, Kp = 12 K at every scale */
    int dec_skip;              /* dec.skip */
} l3c_net_config;

/* The checkpoint's tensors: name, rank and shape of tensor i in the reference's state-dict order (= modules/schema.param_schema).
 * name_host receives a NUL-terminated string of at most name_cap bytes; shape_host holds up to 4 entries. */
int l3c_net_param_count(const l3c_net_config *cfg_host);
int l3c_net_param(const l3c_net_config *cfg_host, int i, char *name_host, int name_cap, int *ndim_host, int64_t *shape_host);

/*
 * ONE caller-owned device buffer holding every layer in the form its kernel reads (Winograd / polyphase / sub-pixel-major / pointwise
 * packings, biases, the small 1x1 weights, the quantiser levels `enc.levels`).  params_host: HOST array of l3c_net_param_count DEVICE
 * pointers, fp32 contiguous, in l3c_net_param order; read by the enqueued work only (keep them alive until it has run).
 * The size functions return a negative status for a config outside the supported set.
 */
int64_t l3c_net_packed_bytes(const l3c_net_config *cfg_host);
int64_t l3c_net_pack_workspace_bytes(const l3c_net_config *cfg_host);
int l3c_net_pack(const l3c_net_config *cfg_host, const float *const *params_host, void *packed, int64_t packed_bytes, void *workspace,
                 int64_t workspace_bytes, l3c_stream_t stream);

/*
 * MultiscaleNetwork.forward of the L3C family.  Scale s of the outputs is the reference's Out index s (raw fields of modules/
 * multiscale_network.Out); h_s = H >> s, w_s = W >> s.  The outputs are also used as scratch before they are written.
 */
typedef struct {
    const l3c_net_config *cfg_host;
    const void *packed;
    int64_t packed_bytes;
    const float *img;                               /* planar fp32 [B][3][H][W], 0..255 */
    int64_t B;
    int H, W;
    int16_t *sym[L3C_NET_MAX_SCALES + 1];           /* [0] image symbols [B][3][H][W] (round half to even); [s] [B][C][h_s][w_s] */
    float *bn_q[L3C_NET_MAX_SCALES + 1];            /* [s >= 1] planar [B][C][h_s][w_s]; [0] unused */
    float *P[L3C_NET_MAX_SCALES];                   /* [s] pixel-major [B][h_s][w_s][Kp_s] */
    float *F_enc[L3C_NET_MAX_SCALES];               /* optional: [s] pixel-major [B][h_(s+1)][w_(s+1)][Cf], encoder features */
    float *F_dec[L3C_NET_MAX_SCALES];               /* optional: [s] pixel-major [B][h_s][w_s][Cf], decoder features */
    void *workspace;
    int64_t workspace_bytes;
} l3c_net_forward_desc;
int64_t l3c_net_forward_workspace_bytes(const l3c_net_config *cfg_host, int64_t B, int H, int W);
int l3c_net_forward(const l3c_net_forward_desc *desc_host, l3c_stream_t stream);

/*
 * MultiscaleNetwork.get_P: one scale's decoder + probability classifier, both model families.  `net` names the scale whose networks
 * run (0 .. num_scales - 1; the recursive scales of the RGB Shared baseline map to num_scales - 1: the caller maps them).
 */
typedef struct {
    const l3c_net_config *cfg_host;
    const void *packed;
    int64_t packed_bytes;
    int net;
    const float *bn_q;                              /* planar [B][C][h][w] */
    int64_t B;
    int h, w;
    const float *fuse;                              /* pixel-major [B][h][w][Cf] coarser decoder features, or NULL (dec_skip == 0: NULL) */
    float *P;                                       /* pixel-major [B][2h][2w][Kp] */
    float *F;                                       /* pixel-major [B][2h][2w][Cf], or NULL */
    void *workspace;
    int64_t workspace_bytes;
} l3c_net_get_p_desc;
int64_t l3c_net_get_p_workspace_bytes(const l3c_net_config *cfg_host, int64_t B, int h, int w);
int l3c_net_get_p(const l3c_net_get_p_desc *desc_host, l3c_stream_t stream);

/*
 * MultiscaleNetwork.get_P_rows: l3c_net_get_p of scale 0 on a ROW WINDOW -- P of full-resolution rows [c0, c1) of the 2h x 2w frame, from
 * the FULL bn_q and fuse.  The schedule is the Python one, so P equals get_P_rows' on every row, bit for bit, and the frame's own P
 * l3c_net_halo_rows rows inside every cut edge (none at a frame border):
 *   decoder      on the half-resolution rows of [a0, a1) = [max(0, c0 - apron), min(2h, c1 + apron)), apron = l3c_net_apron_rows: a
 *                Winograd tile's rounding depends on all of its input rows, so the decoder stage runs that far beyond a cut edge
 *   classifier   on rows [c0, c1) of the decoder's features
 * The row slices that are not contiguous -- every bn_q plane; fuse and the features when B > 1 -- are gathered with strided device-to-device
 * copies on `stream` (one image: fuse and the features are used where they lie); a window whose decoder rows are the whole frame copies
 * no input.  With halo = 2 (2 dec_blocks + 2) + 4 and apron = 2 * 32 * ceil(4 (2 dec_blocks + 2) / 32): 40 and 192 for cr.cf.
 * Checked before anything is enqueued: the L3C family (an RGB baseline: L3C_ERR_UNSUPPORTED), net == 0, c0 and c1 even and inside the
 * frame, c0 a multiple of 64, c1 a multiple of 64 or the frame's end (every kept value keeps its tile and its place in it), fuse non-null,
 * the FULL frame within the limits of l3c_net_get_p (a window must run the kernels the frame would), 16-byte aligned pointers.
 * The workspace is sized for the window and the apron, not for the frame:
 *   max(3 B (c1 - c0) 2w Cf, 4 B (a1 - a0)/2 w Cf) floats | bn_q rows B C (a1 - a0)/2 w (a cut decoder stage only) | fuse rows (likewise,
 *   B > 1) | features B (a1 - a0) 2w Cf | their window rows (B > 1, a window smaller than the decoder rows), each rounded up to 256 bytes
 */
typedef struct {
    const l3c_net_config *cfg_host;
    const void *packed;
    int64_t packed_bytes;
    int net;                                        /* 0 */
    const float *bn_q;                              /* planar [B][C][h][w]: the whole frame's */
    int64_t B;
    int h, w;
    const float *fuse;                              /* pixel-major [B][h][w][Cf]: the whole frame's */
    int c0, c1;                                     /* full-resolution rows of the 2h x 2w frame */
    float *P;                                       /* pixel-major [B][c1 - c0][2w][Kp] */
    void *workspace;
    int64_t workspace_bytes;
} l3c_net_get_p_rows_desc;
int l3c_net_halo_rows(int dec_blocks);
int l3c_net_apron_rows(int dec_blocks);
int64_t l3c_net_get_p_rows_workspace_bytes(const l3c_net_config *cfg_host, int64_t B, int h, int w, int c0, int c1);
int l3c_net_get_p_rows(const l3c_net_get_p_rows_desc *desc_host, l3c_stream_t stream);

/* ---- the whole codec: pixels in, `.l3c` bytes out, and back (replaces bitcoding/bitcoding.py encode / decode) ------------------ */

/*
 * Bitcoding.encode_batch(...).to_bytes() and Bitcoding.decode_batch (reference bitcoding.py:50-123, :125-161) as ONE library call each,
 * for the L3C family (configs/ms/cr.cf: what l3c_net_forward supports), batches of equally sized, already padded images, and the LEGACY
 * `.l3c` format (banded files: the l3c_*_banded entry points at the end of this header).  The library runs the schedule of l3c-pytorch_amd/bitcoding/bitcoding.py over the entry points above, so a file equals
 * the Python path's byte for byte and either side reads the other's.  Outside the scope -- L3C_ERR_UNSUPPORTED, with a message naming it,
 * before anything is enqueued: banded files, the RGB / RGB Shared baselines and auto_recurse; auto-crop parts and preview decode have no
 * entry here.  A BOX of the pictures without decoding the rest of their finest record (Bitcoding.decode_region): l3c_decode_region_plan /
 * l3c_decode_region behind l3c_decode_images, on top of l3c_net_get_p_rows.  Images that are NOT planar, padded or equally sized -- interleaved RGB(X) / BGR(X), a row pitch, any size from 1 x 1, several
 * sizes that pad to one shape in one call -- go through l3c_encode_images / l3c_decode_images at the end of this header, which pad and crop
 * on the device (l3c_u8_gather / l3c_u8_scatter) around the same schedule; sizes that pad to DIFFERENT shapes take one call per shape.
 * Conventions as for l3c_net_forward: device pointers 16-byte aligned, every argument checked before anything is enqueued, no allocation,
 * no host synchronisation, no copy from pageable memory; workspaces are caller-owned, sized by a pure host function, and their contents
 * are garbage on entry.  Two calls on two streams with separate workspaces and outputs may share one model.
 *
 * The three tables of the model are INPUTS: their host rounding (torch.linspace, torch.cumsum) is part of the bitstream contract
 * (criterion/logistic_mixture.py: coding_targets; bitcoding.uniform_cdf_row), and a restatement in C differs in a few entries.
 */
typedef struct {
    const l3c_net_config *cfg_host;
    const void *packed;             /* l3c_net_pack */
    int64_t packed_bytes;
    const float *targets_rgb;       /* fp32 [257]:   DiscretizedMixLogisticLoss.coding_targets of the RGB scale */
    const float *targets_z;         /* fp32 [L + 1]: ... of the bottleneck scales */
    const uint16_t *uniform_row;    /* [L + 1]: bitcoding.uniform_cdf_row(L), the coarsest scale's prior */
    float z_x_min, z_bin_width;     /* l3c_sym_to_bn of the bottleneck symbols */
} l3c_codec_model;

/*
 * File sizes and offsets of a batch on the device (the sums of EncodedBatch.file_sizes): one thread per file.
 *   scales       as for l3c_container_write (only nbytes and C are read), coarsest first, HOST array
 *   file_offset  int64 [B] = b * file_stride        file_bytes  int64 [B] = 8 + sum_scales (5 + 4 C + 4) + the file's payload bytes,
 *                or -1 when one of its streams reported L3C_AC_OVERRUN (the other files of the batch are not affected)
 * B < 65536, file_stride a positive multiple of 16.
 */
int l3c_container_layout(const l3c_container_scale *scales, int n_scales, int64_t B, int64_t file_stride, int64_t *file_offset,
                         int64_t *file_bytes, l3c_stream_t stream);

/* int16 symbols -> uint8 (the low byte): the decoded RGB symbols as pixels.  n elements, both pointers 16-byte aligned. */
int l3c_sym_to_u8(const int16_t *sym, int64_t n, uint8_t *out, l3c_stream_t stream);

/*
 * Encode.  File b of the batch is written to files + b * file_stride, file_bytes[b] bytes of it; file_bytes[b] == -1: a stream of the
 * file reported L3C_AC_OVERRUN (table rows not strictly increasing: the marker EncodedBatch._checked_nbytes turns into an error), the
 * slot's contents are then undefined.  Everything runs on `stream`; overlapping the coder with the next batch's convolutions is the caller's
 * business (two calls on two streams).
 *   l3c_encode_file_stride   8 + sum_scales (5 + 4 C_s + 4) + sum_scales C_s * l3c_ac_max_bytes(h_s * w_s), rounded up to 16: the
 *                            smallest slot that holds any file of that shape
 */
typedef struct {
    const l3c_codec_model *model_host;
    const uint8_t *img;             /* uint8 planar [B][3][H][W] */
    int64_t B;
    int H, W;                       /* multiples of 2^num_scales, below 65536 */
    const uint16_t *padding;        /* uint16 [B][4] left, right, top, bottom -- or NULL: zeros */
    uint8_t *files;                 /* [B][file_stride] */
    int64_t file_stride;            /* a multiple of 16, >= l3c_encode_file_stride */
    int64_t *file_bytes;            /* int64 [B] */
    void *workspace;
    int64_t workspace_bytes;
} l3c_encode_batch_desc;
int64_t l3c_encode_file_stride(const l3c_net_config *cfg_host, int H, int W);
int64_t l3c_encode_batch_workspace_bytes(const l3c_net_config *cfg_host, int64_t B, int H, int W);
int l3c_encode_batch(const l3c_encode_batch_desc *desc_host, l3c_stream_t stream);

/*
 * Decode, in two steps so that the half that reads untrusted bytes is pure host code (csrc/codec_plan.h: no HIP, compiles stand-alone).
 *
 * l3c_decode_plan touches no GPU and reads only framing bytes of the B files files_host + file_offset_host[b] .. file_offset_host[b + 1].
 * It rejects -- L3C_ERR_INVALID_ARG, "invalid file: ..." -- what container.parse_containers, count_scale_records and Bitcoding._n_predicted /
 * _check_coarsest / _check_header reject: truncation, a length field or payload past the end of its file, a missing separator, trailing
 * bytes, C == 0, a record count other than num_scales + 1, a coarsest header whose C is not the model's or whose H or W is 0, a coarsest
 * payload longer than 2 H W + 64 bytes, a predicted record that is not (C_s, 2 h, 2 w) of the one above, files that disagree, sizes the
 * network schedule does not support; a banded file is L3C_ERR_UNSUPPORTED.  It writes ONE self-describing blob (layout: codec_plan.h)
 * holding the records, per stream the src_offset / dst_offset / nbytes of l3c_container_read, and the RGB chunk list; the caller copies
 * the blob to the device as it is (the entries_dev / entries_host precedent of l3c_decode_rgb_entries).
 *   plan_host         l3c_decode_plan_bytes(cfg, B) bytes, 8-byte aligned           padding_host_out  uint16 [B][4], may be NULL
 *
 * l3c_decode_batch: the walk over the records.  The RGB chunk policy is Bitcoding._decode_rgb_pipelined's default (32 chunks, two
 * 1024-symbol probes from 16384 pixels on, window mode 1); from 16 images on the decoders run on `side_stream` (lag 2), which must
 * then be a stream of its own -- otherwise it is not used and may be NULL.  main_stream is ordered after the last pixel.
 *   files             the files' bytes on the device at the offsets the plan was made with; 16-byte aligned, readable up to the next
 *                     multiple of 4 of their size
 *   plan_host / plan  the blob and the caller's device copy of it; plan_bytes: the size of either
 *   pixels            uint8 planar [B][3][H][W]           sym   optional: int16 [B][3][H][W], the same values
 */
typedef struct {
    const l3c_codec_model *model_host;
    const uint8_t *files;
    const void *plan_host;
    const void *plan;
    int64_t plan_bytes;
    uint8_t *pixels;
    int16_t *sym;
    void *workspace;
    int64_t workspace_bytes;
} l3c_decode_batch_desc;
int64_t l3c_decode_plan_bytes(const l3c_net_config *cfg_host, int64_t B);
int l3c_decode_plan(const l3c_net_config *cfg_host, const uint8_t *files_host, const int64_t *file_offset_host, int64_t B, void *plan_host,
                    int64_t plan_bytes, int *H_out, int *W_out, uint16_t *padding_host_out);
int64_t l3c_decode_batch_workspace_bytes(const l3c_net_config *cfg_host, const void *plan_host);
int l3c_decode_batch(const l3c_decode_batch_desc *desc_host, l3c_stream_t main_stream, l3c_stream_t side_stream);

/* ---- the whole codec on BANDED files (Bitcoding(bands=K): signature 'L3CB', see l3c_ac_band_intervals) ------------------------------- */

/*
 * The same two directions for the banded format: one library call each, the schedule of Bitcoding.code with enc.bands and of
 * _walk_records with _scale_symbols_banded, so a file equals Bitcoding(bp, bands=K).encode_batch(x).to_bytes(paddings) byte for byte and
 * either side reads the other's.  Scope, conventions, model and descriptors as above; the legacy entry points are unchanged (l3c_decode_plan
 * keeps refusing a banded file, the planner here refuses a legacy one).
 *
 * l3c_ac_decode_bands: the uniform-prior decode of every band of every plane in ONE launch, straight into the planes (the coarsest record;
 * the row_stride == 0 case of l3c_ac_decode, one wavefront per band).  With n = ceil(n_sym / band_len), stream (p, j) is index p * n + j of
 * in_offsets / in_nbytes; it decodes min(band_len, n_sym - j * band_len) symbols -- a complete stream: its last symbol skips the state update
 * -- and stores them at sym_out + p * n_sym + j * band_len: bit for bit what l3c_ac_decode gives for that band alone.
 *   cdf_row   uint16 [Lp], 2 <= Lp <= 257      band_len  a positive multiple of 64      n_planes * n < 2^31      in  4-byte aligned
 */
int l3c_ac_decode_bands(const uint16_t *cdf_row, int Lp, const uint8_t *in, const int64_t *in_offsets, const uint32_t *in_nbytes,
                        int64_t n_planes, int64_t n_sym, int64_t band_len, int monotone, int16_t *sym_out, l3c_stream_t stream);

/*
 * File sizes and offsets of a banded batch on the device, the banded counterpart of l3c_container_layout: a block per file, a wave
 * reduction over its up to C * n length fields per scale.
 *   scales       as for l3c_container_write_banded (only the nbytes arrays, C, H, W and band_len are read), coarsest first, HOST array
 *   file_offset  int64 [B] = b * file_stride      file_bytes  int64 [B] = 14 + sum_scales (9 + 4 C n + 4) + the file's payload bytes, or -1
 *                when one of its bands reported L3C_AC_OVERRUN (the other files of the batch are not affected)
 * B < 65536, file_stride a positive multiple of 16, file_offset / file_bytes 16-byte aligned.
 */
int l3c_container_layout_banded(const l3c_banded_scale *scales, int n_scales, int64_t B, int64_t file_stride, int64_t *file_offset,
                                int64_t *file_bytes, l3c_stream_t stream);

/*
 * Encode: l3c_encode_batch_desc as for l3c_encode_batch, plus the band count K = `bands` (1 .. 1024): every channel of scale s is cut into
 * bands of L_s = 64 ceil(h_s w_s / (64 K)) symbols (container.band_len).  Per scale the interval head, l3c_ac_band_intervals (a full-bands
 * group, absent when n == 1, and a last-bands group), ONE l3c_ac_encode_groups over all groups of all scales, l3c_container_layout_banded,
 * l3c_container_write_banded.  A band that overran marks its file -1 and is written as an empty payload.
 *   l3c_encode_banded_file_stride   14 + sum_scales (9 + 4 C_s n_s + 4) + every band at l3c_ac_max_bytes of its length, rounded up to 16
 */
int64_t l3c_encode_banded_file_stride(const l3c_net_config *cfg_host, int H, int W, int bands);
int64_t l3c_encode_batch_banded_workspace_bytes(const l3c_net_config *cfg_host, int64_t B, int H, int W, int bands);
int l3c_encode_batch_banded(const l3c_encode_batch_desc *desc_host, int bands, l3c_stream_t stream);

/*
 * Decode.  The planner (csrc/codec_plan_banded.h: pure host code, reads framing bytes only) rejects -- L3C_ERR_INVALID_ARG, "invalid file:
 * ..." -- what container.parse_banded rejects (version or reserved byte, C == 0, an empty scale, L == 0 or not a multiple of 64, more than
 * 1024 bands, a length field or payload past the end, a missing separator, trailing bytes), what Bitcoding._n_predicted / _check_coarsest
 * (a coarsest band payload longer than 2 L + 64 bytes) / _check_header reject, and files of a batch that disagree in any (C, H, W, L).
 * L3C_ERR_UNSUPPORTED: a legacy file (l3c_decode_plan reads those), a mix of both formats, a scale with B * n > 65535 bands (slice the batch).
 * The number of bands is a property of the FILES: l3c_decode_plan_banded_bytes walks file 0's framing, validating as it goes, and returns
 * the blob size or a negative status.  The blob (its own magic word; layout: codec_plan_banded.h) holds the records (C, H, W, L, n, first
 * stream, stream count, longest payload), per band stream the src_offset / dst_offset / nbytes of l3c_container_read -- coarsest record
 * image-major (b C + c) n + j, every other record channel-major (c B + b) n + j --, for every bottleneck record the entry table
 * pixbase | hw | pix0 | npix | table_off of its B n bands (read by the ragged kernels from the DEVICE copy of the blob), and for the RGB
 * record the band length, the chunk count max(1, min(8, last band's symbols / 64)) and the lag (2 when B * n >= 16, else 1).
 *
 * l3c_decode_batch_banded: l3c_container_read in slices of 65535 streams; coarsest record l3c_ac_decode_bands; every bottleneck record
 * l3c_sym_to_bn, l3c_net_get_p, l3c_dmll_cdf_table_ragged + l3c_ac_decode_chunks (ragged) over all B n bands, up to 8 channels per call;
 * the RGB record l3c_decode_rgb_banded on zeroed symbols, window mode 1; l3c_sym_to_u8.  side_stream must be a stream of its own whenever
 * the plan says lag 2; main_stream is ordered after the last pixel.
 *
 * l3c_decode_batch_banded_p_offset: where that call leaves the finest record's P [B][H W][12 K] -- the last thing written to the single P
 * area of its workspace -- as a byte offset from the workspace pointer rounded up to the next multiple of 256 (the base the decode itself
 * works from; a 256-byte aligned workspace: from the pointer).  A multiple of 256; valid until the workspace is reused.  Pure host code
 * on the plan l3c_decode_batch_banded_workspace_bytes reads; a negative status for a bad plan.  With desc.sym, the caller then holds what
 * l3c_dmll_conceal needs (INTEGRATION.md "Salvage decode").
 *
 * l3c_decode_batch_banded_streams_offset: the STREAM AREA of that workspace -- every band payload of the files as l3c_container_read left
 * it, 4-byte aligned and followed by zero bytes up to ((nbytes + 3) / 4) * 4 + 4 -- as a byte offset under the base and the rules of
 * l3c_decode_batch_banded_p_offset.  l3c_decode_plan_banded_stream: one stream of the plan without restating the blob's layout -- stream
 * `index` of record `record` (0: the coarsest), numbered inside the record as above ((c B + b) n + j in every record but the coarsest): its
 * first byte in `files` (src_offset), its slot inside the stream area (dst_offset, a multiple of 4) and its length.  The header is checked
 * against the layout its own B and records imply and the entry against the size of the stream area; L3C_ERR_INVALID_ARG for a blob that is
 * not a banded plan, a record or an index out of range, or a null pointer.  Pure host code.  Together they are what an in-place repair of
 * the finest record's streams (l3c_band_rebuild) needs to address.
 */
int64_t l3c_decode_plan_banded_bytes(const l3c_net_config *cfg_host, const uint8_t *files_host, const int64_t *file_offset_host, int64_t B);
int l3c_decode_plan_banded(const l3c_net_config *cfg_host, const uint8_t *files_host, const int64_t *file_offset_host, int64_t B,
                           void *plan_host, int64_t plan_bytes, int *H_out, int *W_out, uint16_t *padding_host_out);
int64_t l3c_decode_batch_banded_workspace_bytes(const l3c_net_config *cfg_host, const void *plan_host);
int64_t l3c_decode_batch_banded_p_offset(const l3c_net_config *cfg_host, const void *plan_host);
int64_t l3c_decode_batch_banded_streams_offset(const l3c_net_config *cfg_host, const void *plan_host);
int l3c_decode_plan_banded_stream(const void *plan_host, int record, int64_t index, int64_t *src_offset_out, int64_t *dst_offset_out,
                                  uint32_t *nbytes_out);
int l3c_decode_batch_banded(const l3c_decode_batch_desc *desc_host, l3c_stream_t main_stream, l3c_stream_t side_stream);

/* ---- pictures as they come: any size and layout, padded and cropped on the device ----------------------------------------------------- */

/*
 * One image inside ONE caller-owned byte buffer, and its place in the padded Hp x Wp frame the codec works on.  The view addresses byte
 *     offset + y * row_stride + x * pix_stride + c * chan_stride          for y < h, x < w, c < 3 (R, G, B)
 * of the buffer:
 *     planar  [3][h][w]             row_stride = w (or a pitch),     pix_stride = 1, chan_stride = the plane size
 *     RGB     [h][w][3]             row_stride = 3 w (or a pitch),   pix_stride = 3, chan_stride = 1
 *     RGBX    [h][w][4]             row_stride = 4 w (or a pitch),   pix_stride = 4, chan_stride = 1   (the X byte is never read or written)
 *     BGR(X)                        as RGB / RGBX with offset at the pixel's R byte (+ 2) and chan_stride = -1
 * Images of one table may differ in size and layout as long as they share the frame.  (top, left) is free inside the frame; the files of
 * Bitcoding use centre padding -- l3c_image_padding: (left, right, top, bottom) exactly as helpers/pad.py: padding_for, the smaller half
 * first; top = pad_out[2], left = pad_out[0].
 *
 * l3c_image_table_check is the pure host validator the entries below run before they enqueue anything: for every image h, w in 1 .. 65535,
 * pix_stride > 0, top + h <= Hp, left + w <= Wp, and -- in overflow-checked 64-bit arithmetic, over the four corners and three channels,
 * with signed strides -- every byte the view addresses inside [0, buffer_bytes).  Anything else: L3C_ERR_INVALID_ARG, the message names
 * the image index and the field.  Views of DIFFERENT images that overlap in a destination buffer are not diagnosed: the bytes they share
 * are unspecified afterwards.
 */
typedef struct {
    int64_t offset;       /* bytes from the base pointer to channel 0 (R) of pixel (0,0) */
    int64_t row_stride;   /* bytes between rows (may exceed w * pix_stride) */
    int64_t chan_stride;  /* bytes between channels: plane size for planar, 1 for RGB/RGBX, -1 for BGR(X) with offset at R */
    int32_t pix_stride;   /* bytes between pixels of a row: 1, 3 or 4 (any positive value is legal) */
    int32_t h, w;         /* the image's own size, 1..65535 */
    int32_t top, left;    /* where it sits in the padded Hp x Wp frame */
} l3c_u8_image;
int l3c_image_padding(int h, int w, int fac, uint16_t *pad_out);
int l3c_image_table_check(const l3c_u8_image *images_host, int64_t B, int Hp, int Wp, int64_t buffer_bytes);

/*
 * l3c_u8_gather: the B views of `src` -> uint8 planar frames dst [B][3][Hp][Wp], ONE launch whatever the mix of sizes and layouts.  Every
 * byte of dst is written: the picture inside its frame, zero outside (padding mode 'constant').  padding_out, unless NULL, receives each
 * image's (left, right, top, bottom) = (left, Wp - left - w, top, Hp - top - h): the device array l3c_encode_batch_desc.padding expects.
 * l3c_u8_scatter: the inverse crop, planar frames src [B][3][Hp][Wp] -> the B views of `dst`.  Exactly the 3 h w bytes each view addresses
 * are written; pitch gaps, the X byte of RGBX and everything between the images stay as they were.
 *   images_host / images   the table and the caller's device copy of it (the entries_host / entries_dev precedent): the host copy is
 *                          validated, the kernels read the device copy
 *   src_bytes / dst_bytes  size of the strided buffer the views lie in; that buffer needs no alignment
 * Conventions as everywhere: all arguments checked before the launch, no allocation, no host synchronisation; B < 65536; Hp, Wp below
 * 65536, Wp a multiple of 4; the planar frames, the device table and padding_out 16-byte aligned.  The frames move as whole 4-, 8- or
 * 16-byte accesses (the widest that divides Wp); the strided side as whole dwords where a thread's 4 to 16 pixels are one run of bytes --
 * a dword-aligned planar row, or packed pixels (chan_stride +-1, pix_stride 3 or 4) at any alignment; RGBX only when read: its X bytes are
 * never written -- and byte by byte otherwise.  Stores touch only validated bytes; the packed loads may read up to 3 bytes on either side of a
 * run, always inside [0, src_bytes).
 */
int l3c_u8_gather(const uint8_t *src, int64_t src_bytes, const l3c_u8_image *images_host, const l3c_u8_image *images, int64_t B, int Hp, int Wp,
                  uint8_t *dst, uint16_t *padding_out, l3c_stream_t stream);
int l3c_u8_scatter(const uint8_t *src, int64_t B, int Hp, int Wp, uint8_t *dst, int64_t dst_bytes, const l3c_u8_image *images_host,
                   const l3c_u8_image *images, l3c_stream_t stream);

/*
 * The codec on such a table.  l3c_encode_images: l3c_u8_gather into the workspace, then exactly the schedule of l3c_encode_batch (bands == 0:
 * the legacy format) or l3c_encode_batch_banded (bands = 1 .. 1024) on that planar batch and padding array -- so file b equals
 * Bitcoding(bp[, bands]).encode_batch(zero-padded batch).to_bytes(paddings)[b] byte for byte.  files / file_stride / file_bytes as for
 * l3c_encode_batch; the file stride is l3c_encode_file_stride / l3c_encode_banded_file_stride of (Hp, Wp).
 * l3c_decode_images: l3c_decode_batch or l3c_decode_batch_banded -- the plan blob's magic word says which; the planners are unchanged --
 * into the workspace, then l3c_u8_scatter on main_stream.  The table is validated against the plan's B, H and W before anything is enqueued;
 * an image's place in the frame is the caller's to set from the planner's padding_host_out (top = padding[2], left = padding[0], h = H -
 * padding[2] - padding[3], w = W - padding[0] - padding[1]).  Stream semantics as for l3c_decode_batch.
 * Outside the scope, as before: a padded shape the network schedule refuses and images that would need auto-crop parts (L3C_ERR_UNSUPPORTED).
 */
typedef struct {
    const l3c_codec_model *model_host;
    const uint8_t *src;             /* the buffer the views lie in (device) */
    int64_t src_bytes;
    const l3c_u8_image *images_host;
    const l3c_u8_image *images;     /* device copy, 16-byte aligned */
    int64_t B;
    int Hp, Wp;                     /* the frame: multiples of 2^num_scales, below 65536 */
    int bands;                      /* 0: legacy format, 1 .. 1024: banded */
    uint8_t *files;                 /* [B][file_stride] */
    int64_t file_stride;
    int64_t *file_bytes;            /* int64 [B] */
    void *workspace;
    int64_t workspace_bytes;
} l3c_encode_images_desc;
int64_t l3c_encode_images_workspace_bytes(const l3c_net_config *cfg_host, int64_t B, int Hp, int Wp, int bands);
int l3c_encode_images(const l3c_encode_images_desc *desc_host, l3c_stream_t stream);

typedef struct {
    const l3c_codec_model *model_host;
    const uint8_t *files;
    const void *plan_host;          /* of l3c_decode_plan or l3c_decode_plan_banded */
    const void *plan;
    int64_t plan_bytes;
    uint8_t *dst;                   /* the buffer the views lie in (device) */
    int64_t dst_bytes;
    const l3c_u8_image *images_host;
    const l3c_u8_image *images;     /* device copy, 16-byte aligned */
    int16_t *sym;                   /* optional: int16 planar [B][3][H][W] */
    void *workspace;
    int64_t workspace_bytes;
} l3c_decode_images_desc;
int64_t l3c_decode_images_workspace_bytes(const l3c_net_config *cfg_host, const void *plan_host);
int l3c_decode_images(const l3c_decode_images_desc *desc_host, l3c_stream_t main_stream, l3c_stream_t side_stream);

/* ---- region decode: a box of the pictures without decoding the rest of their finest record (Bitcoding.decode_region) ------------------ */

/*
 * Four calls: l3c_decode_plan or l3c_decode_plan_banded (unchanged; the only code that reads file bytes), l3c_decode_region_plan_bytes,
 * l3c_decode_region_plan, l3c_decode_region.  L3C family, at least two scales, B files of one padding tuple, either format (a LEGACY file
 * is one band: its rows below the box are saved, the rows above are not).
 *
 * l3c_decode_region_plan is pure host code (csrc/codec_plan_region.h: bitcoding/region.py restated) and reads only the plan blob, which it
 * re-checks.  box: rows [y0, y1) x columns [x0, x1) in the coordinates of the UNPADDED image (frame row = top padding + y).  It writes a
 * second self-describing blob (own magic word, its size, the cfg words; layout: codec_plan_region.h), which the caller copies to the
 * device as it is:
 *   the plan     region.region_plan of the finest record with cut=True -- bands [j0, j1) that hold a pixel of the box rows, the symbol,
 *                conv, valid and decoder rows
 *   streams      of the 3 B (j1 - j0) picked band streams the src_offset / dst_offset / nbytes of l3c_container_read, channel-major
 *                ((c, e) at c S + e, e = b (j1 - j0) + (j - j0)), dst_offset compact; a stream outside the region has no entry and is never read
 *   entries      pixbase | hw | pix0 | len of l3c_decode_rgb_entries: band j of image b is pixels [j L - c0 W, ...) of window image b
 *   chunks, lag  banded max(1, min(8, shortest entry / 64)), legacy max(1, min(32, shortest entry / 4096)); lag 2 from 16 entries on
 *   crop         B l3c_u8_image entries: the box inside the window frames [B][3][c1 - c0][W], planar in `pixels`
 * L3C_ERR_INVALID_ARG with a message: an empty box or one that leaves the image, files whose padding tuples differ, a plan blob that fails
 * its check, region_bytes too small.  L3C_ERR_UNSUPPORTED: the RGB baselines, num_scales < 2, more than 65535 entries.
 * l3c_decode_region_plan_bytes: the size that holds the blob of ANY box of the planned files (a pure function of the plan blob).
 *
 * l3c_decode_region: the walk of l3c_decode_batch / l3c_decode_batch_banded over every record but the finest (l3c_container_read on THEIR
 * streams only), then the finest step on the window: l3c_container_read of the picked streams, l3c_net_get_p_rows on the conv rows, a
 * zeroed window symbol buffer, ONE l3c_decode_rgb_entries call (window mode 1, the blob's chunk count and lag), l3c_sym_to_u8 on the
 * window, l3c_u8_scatter with the blob's crop table.  side_stream is used only at lag 2 and must then be a stream of its own; main_stream
 * is ordered after the last pixel.  The region blob is checked against the plan blob (planned again from its own header and compared)
 * before a word of it is trusted.  Conventions as everywhere: every argument checked before anything is enqueued, no allocation, no host
 * synchronisation, no read of pageable memory.
 * The workspace is sized by the WINDOW -- no full-frame P and no full-frame symbols of the finest scale (at 2048 x 3072 a full-frame P is
 * ~3 GB, a 64-row window's a thirtieth) -- each term rounded up to 256 bytes:
 *   coarser streams | picked streams | per coarser record its symbols B C h w int16 (and features B h w Cf floats between two bottleneck
 *   records) | bn: the largest B C h w floats | P: max(coarser B h w Kp, B (c1 - c0) W Kp_0) floats | window symbols B 3 (c1 - c0) W int16 |
 *   window pixels B 3 (c1 - c0) W | flags | scratch: max(l3c_net_get_p workspaces of the coarser records, their tables,
 *   l3c_net_get_p_rows_workspace_bytes, l3c_decode_rgb_entries_workspace_bytes) | 256
 * SEALS stay the caller's business, as for l3c_decode_batch: strip with l3c_seal_find before planning.  A seal's CRC covers the whole
 * frame: a region decode CANNOT check it (generation and model id can be checked as ever) unless the file is band-sealed ("band seals"
 * below) -- and this entry does not check a band table either: it cuts the last band and keeps the window's pixels in its workspace.
 */
typedef struct {
    int32_t y0, y1, x0, x1;         /* UNPADDED image coordinates: rows [y0, y1), columns [x0, x1) */
} l3c_region_box;
typedef struct {
    int32_t bands[2];               /* [j0, j1) of the finest record's n_bands bands per channel */
    int32_t n_bands;
    int32_t sym_rows[2];            /* frame rows the range decoder produces symbols in */
    int32_t conv_rows[2];           /* frame rows the classifier runs on: the window */
    int32_t valid_rows[2];          /* rows of the window whose P is the frame's */
    int32_t decoder_rows[2];        /* frame rows the decoder stage runs on (at half resolution) */
    int32_t frame_rows;
    int32_t n_chunks, lag;          /* of the l3c_decode_rgb_entries call */
    int32_t out_rows, out_cols;     /* the box's size */
    int64_t streams_used, streams_total, bytes_used, bytes_total;   /* band streams of the finest record and their payload bytes, over the batch */
} l3c_region_info;
typedef struct {
    const l3c_codec_model *model_host;
    const uint8_t *files;           /* as for l3c_decode_batch */
    const void *plan_host;          /* of l3c_decode_plan or l3c_decode_plan_banded */
    const void *plan;
    int64_t plan_bytes;
    const void *region_host;        /* of l3c_decode_region_plan */
    const void *region;             /* device copy, 16-byte aligned */
    int64_t region_bytes;
    uint8_t *pixels;                /* uint8 planar [B][3][y1 - y0][x1 - x0] */
    void *workspace;
    int64_t workspace_bytes;
} l3c_decode_region_desc;
int64_t l3c_decode_region_plan_bytes(const l3c_net_config *cfg_host, const void *plan_host);
int l3c_decode_region_plan(const l3c_net_config *cfg_host, const void *plan_host, int64_t plan_bytes, const uint16_t *padding_host,
                           const l3c_region_box *box_host, void *region_host, int64_t region_bytes, l3c_region_info *info_out);
int64_t l3c_decode_region_workspace_bytes(const l3c_net_config *cfg_host, const void *plan_host, const void *region_host);
int l3c_decode_region(const l3c_decode_region_desc *desc_host, l3c_stream_t main_stream, l3c_stream_t side_stream);

/* ---- sealed files: what the decoded frame must hash to, checked on decode (opt-in; INTEGRATION.md "Sealed files") ---------------------- */

/*
 * A `.l3c` file decodes correctly only with the bitstream generation and the checkpoint that wrote it; anything else, or a damaged payload
 * byte, comes out of the range decoder as a picture of the right size with the wrong pixels.  A SEAL is 24 bytes behind the file's last
 * separator, the same for legacy and banded files, little-endian:
 *     0 'L3CS' | 4 u8 version = 1 | 5 u8 flags = 0 | 6 u16 generation | 8 u32 frame CRC | 12 u64 model id | 20 u32 check
 *   generation   l3c_bitstream_generation() of the writer
 *   frame CRC    CRC-32 (the zlib polynomial: zlib.crc32) of the 3 H W bytes of the PADDED planar frame [3][H][W] the codec codes: the
 *                encoder's l3c_encode_batch_desc.img, the decoder's l3c_decode_batch_desc.pixels -- independent of layout and padding
 *   model id     the first 8 bytes, little-endian, of SHA-256 over every tensor of the checkpoint in l3c_net_param order as contiguous
 *                little-endian fp32; a result of 0 is stored as 1, and 0 means "not stated"
 *   check        CRC-32 of the file's 8 padding bytes (file bytes 0..7; bytes 6..13 of a banded file) followed by seal bytes 0..19: a damaged
 *                padding field would crop the wrong window out of a correct frame
 * A file is sealed exactly when it has at least 28 bytes, file[-24:-20] is 'L3CS' and file[-28:-24] is the scale separator 46 E2 84 92 that
 * every unsealed file of either format ends with.  The planners and parsers are unchanged and go on rejecting trailing bytes: a reader
 * strips the seal (l3c_seal_find) and hands them the body.  A reader checks, in this order: the generation; the model id when both its own
 * and the file's are non-zero -- both before anything is enqueued --; after the decode, l3c_u8_crc32 of `pixels` against the frame CRC.
 *
 * l3c_seal_find / l3c_seal_write are pure host code (csrc/seal.h: no HIP, compiles stand-alone).  l3c_seal_find returns 1: sealed
 * (*body_bytes_out = file_bytes - 24 -- a band-sealed file, below: the size in front of its band table --, *seal_out filled), 0: unsealed (*body_bytes_out = file_bytes), L3C_ERR_INVALID_ARG, "invalid file:
 * seal ...": a recognised seal with an unknown version, non-zero flags or a wrong check word -- never treated as absent.  l3c_seal_write
 * stores the 24 bytes for a file whose 8 padding bytes are padding8_host.
 */
#define L3C_SEAL_BYTES 24
typedef struct {
    uint16_t generation;
    uint32_t frame_crc;
    uint64_t model_id;
} l3c_seal;
int l3c_seal_find(const uint8_t *file_host, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out);
int l3c_seal_write(const l3c_seal *seal_host, const uint8_t *padding8_host, uint8_t *dst_host);

/*
 * l3c_u8_crc32: crc_out[i] = zlib CRC-32 of the item_bytes bytes at data + i * item_stride, for n_items items in two launches.  Integer
 * only; the result does not depend on the launch geometry; no atomics.  A block folds a TILE of block_bytes bytes: each thread keeps four
 * remainders, one per dword of its 16-byte loads (thread t reads bytes 16 t .. 16 t + 15 of every 4096-byte row of the tile: whole cache
 * lines per wave), advances them by one row -- a multiplication with x^(8 * 4096) mod P -- through 4-bit tables in LDS that every lane reads
 * in a bank of its own, then shifts them to the end of the tile (thread_bytes = 16 * rows per tile: what one thread folds) and the block
 * XORs them together; the tile's remainder goes to the workspace.  The second launch, a wavefront per item, combines an item's tiles with
 * multiplications by x^(8 * block_bytes), undoes the zero bytes its last tile was filled up with, and applies zlib's initial and final XOR
 * as one word that depends on the length alone.  The constants of the fixed run lengths are computed at build time, those of the item length
 * on the host per call.
 *   data          4-byte aligned (16-byte aligned data and stride: the full load rate)      item_stride   % 4 == 0 and >= item_bytes
 *   item_bytes    >= 0 (0: CRC 0), n_items >= 1, any int64 sizes with n_items * ceil(item_bytes / block_bytes) < 2^40
 *   workspace     l3c_u8_crc32_workspace_bytes(n_items, item_bytes) bytes, 16-byte aligned; garbage on entry
 * Bytes between items are never read into a result; nothing past the last item's last byte is read.  No allocation, no host sync.
 * l3c_u8_crc32_tile: thread_bytes and block_bytes, the lengths the tests place their cases around.
 */
int64_t l3c_u8_crc32_workspace_bytes(int64_t n_items, int64_t item_bytes);
int l3c_u8_crc32(const uint8_t *data, int64_t n_items, int64_t item_bytes, int64_t item_stride, uint32_t *crc_out, void *workspace,
                 int64_t workspace_bytes, l3c_stream_t stream);
int l3c_u8_crc32_tile(int *thread_bytes_out, int *block_bytes_out);

/*
 * l3c_u8_crc32_spans: crc_out[i] = zlib CRC-32 of bytes [spans[i].offset, spans[i].offset + spans[i].bytes) of `data`, for n_spans spans
 * of DIFFERENT lengths in at most three launches, however many spans: the frames of a ragged group of differently sized images, which lie
 * in one buffer.  Integer only; the result does not depend on the launch geometry; no atomics; no allocation, no host sync.
 * A tile of a span is folded by the tile code of l3c_u8_crc32 (the same rows, tables and loads), so a full tile costs what it costs there.
 * What differs per span is found on the device: the first launch turns `spans` into a prefix of tile counts (one block) and, a thread per
 * span and constant, into the three words that depend on a span's length -- x^(8 * bytes of its last tile's rows), x^(-8 * zero fill) and
 * Z(bytes), which l3c_u8_crc32 gets as kernel arguments -- in the workspace; a block of the second launch finds its tile's span by
 * bisecting that prefix; the third, a wavefront per span, combines a span's tiles as l3c_u8_crc32's second launch does.  A call whose spans
 * are all empty skips the second.
 *   spans_host    the table on the host, validated before anything is launched (an error names the span)
 *   spans         the caller's device copy of the same table, 8-byte aligned
 *   span          offset % 4 == 0 and >= 0, bytes >= 0 (0: CRC 0), offset + bytes <= data_bytes; spans may come in any order, overlap and
 *                 leave gaps; the tiles of all spans together (ceil(bytes / block_bytes) each) stay below 2^40
 *   data          4-byte aligned (16-byte aligned data and offsets: the full load rate)
 *   crc_out       uint32 [n_spans], 4-byte aligned
 *   workspace     l3c_u8_crc32_spans_workspace_bytes(spans_host, n_spans) bytes, 16-byte aligned; garbage on entry
 * Nothing at or behind offset + bytes of a span is read into a result or read at all: a span may end with the buffer.
 */
typedef struct l3c_u8_span {
    int64_t offset;
    int64_t bytes;
} l3c_u8_span;     /* bytes [offset, offset + bytes) of `data` */
int64_t l3c_u8_crc32_spans_workspace_bytes(const l3c_u8_span *spans_host, int64_t n_spans);
int l3c_u8_crc32_spans(const uint8_t *data, int64_t data_bytes, const l3c_u8_span *spans_host, const l3c_u8_span *spans, int64_t n_spans,
                       uint32_t *crc_out, void *workspace, int64_t workspace_bytes, l3c_stream_t stream);

/*
 * l3c_seal_append: this build's seal behind every file of an encode, on the device: 24 bytes at files + b * file_stride + file_bytes[b],
 * file_bytes[b] += 24.  One thread per file, byte stores.  A sealed encode is three calls on one stream with no host round trip:
 * l3c_encode_batch (or _banded), l3c_u8_crc32 on desc.img (n_items = B, item_bytes = item_stride = 3 H W), l3c_seal_append; the body of the
 * sealed file is the unsealed file.  It needs file_stride >= l3c_encode_file_stride(...) + 32 (l3c_encode_banded_file_stride(...) + 32).
 * With pictures as they come: l3c_u8_gather into a frame buffer of the caller's, then the three calls on those frames and on its
 * padding_out -- the files of l3c_encode_images byte for byte, sealed.
 *   frame_crc   uint32 [B], l3c_u8_crc32's crc_out           padding   the uint16 [B][4] array of the encode, NULL = zeros
 *   model_id    0 = not stated                               file_bytes[b] == -1 stays -1; a slot without room for 24 more bytes becomes -1
 *                                                            and nothing is stored outside a slot
 * B < 65536; file_stride > 0.
 */
int l3c_seal_append(uint8_t *files, int64_t file_stride, int64_t *file_bytes, const uint32_t *frame_crc, const uint16_t *padding,
                    uint64_t model_id, int64_t B, l3c_stream_t stream);

/* ---- band seals: a CRC per band of the finest record (opt-in, banded files only; INTEGRATION.md "Band seals") ---------------------------- */

/*
 * The P of the finest scale depends on the coarser records alone, never on other pixels of that scale: a damaged byte in band j of the
 * finest record spoils band j and nothing else.  A BAND SEAL (seal version 2) therefore carries one CRC-32 per band of the finest record,
 * so that a region decode verifies exactly the bands it decoded and a full decode names the damaged bands:
 *     body (the unsealed banded file) | BAND TABLE | the 24 seal bytes above with version = 2
 *     BAND TABLE, little-endian, T = 20 + 12 n bytes:
 *       0 'L3CT' | 4 u16 n | 6 u16 0 | 8 u32 L | 12 u32 crc[3][n] (channel-major) | 12 + 12 n u32 T | 16 + 12 n separator 46 E2 84 92
 *   n, L         bands per channel and band length of the finest record; a reader rejects a table that states others than the record header
 *   crc[c][j]    CRC-32 of bytes [c HW + j L, c HW + min((j + 1) L, HW)) of the padded planar frame
 *   frame CRC    as in version 1; it must be the combination of the band CRCs (crc(A | B) = crc(A) x^(8 |B|) + crc(B) over GF(2))
 *   check        CRC-32 of the 8 padding bytes, then the whole table, then seal bytes 0..19
 * The table ends with the separator, so the recognition rule is the one above for both versions; T lies at file[-32:-28].
 *
 * l3c_seal_find_bands is l3c_seal_find that also hands out the table: *body_bytes_out is the size in front of the TABLE, bands_out->crc
 * points INTO the file (12 n bytes, [3][n] little-endian words, unaligned); a version-1 seal gives n = 0.  "invalid file: seal ..." for a
 * length field that is not 20 + 12 n with 1 <= n <= 1024, a table that would start in front of the body's last separator, a missing
 * 'L3CT', a non-zero reserved field, a wrong check word, a version-2 seal on a legacy file, n or L other than the finest record's, a frame
 * CRC that is not the combination of the band CRCs.  l3c_seal_find on a band-sealed file returns 1 with the same *body_bytes_out: a
 * caller that knows version 1 alone goes on verifying the frame CRC.  l3c_seal_write_bands stores l3c_seal_bands_bytes(n) bytes.
 */
typedef struct {
    int32_t n;                      /* bands per channel; 0: a version-1 seal */
    uint32_t band_len;
    const uint8_t *crc;             /* 12 n bytes inside the file: [3][n] little-endian words, unaligned */
} l3c_seal_bands;
int64_t l3c_seal_bands_bytes(int n);    /* 20 + 12 n + 24: table and seal */
int l3c_seal_find_bands(const uint8_t *file_host, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out);
int l3c_seal_write_bands(const l3c_seal *seal_host, const uint8_t *padding8_host, const uint32_t *band_crc_host, int n, uint32_t band_len,
                         uint8_t *dst_host);

/*
 * l3c_u8_crc32_bands: the CRC-32 of every band of every plane of n_frames frames AND of every frame, the bytes read once, in two launches.
 * Frame f is `planes` planes of plane_bytes bytes back to back at frames + f * frame_stride; band j of a plane is its bytes
 * [j * band_bytes, min((j + 1) * band_bytes, plane_bytes)), n = ceil(plane_bytes / band_bytes) bands per plane.
 * First launch: a WAVEFRONT per 16 KiB chunk of a band (four per block, no barrier behind the table staging): lane l loads bytes
 * 16 l .. 16 l + 15 of every 1024-byte row and advances its four remainders by x^(8 * 1024) through the 4-bit tables of l3c_u8_crc32 in
 * LDS, a bank per lane; a chunk's remainder, zero-filled to whole rows, goes to the workspace.  Second launch, a wavefront per frame: a
 * lane finishes a band (its chunks, the fill undone, Z(length) added) and Horner-combines its share of a plane's band remainders; the
 * wave combines planes into the frame's word.  Only two band lengths exist (the full band, a plane's last): their constants are
 * computed on the host per call.  Integer only, no atomics, the same words whatever the launch geometry, no allocation, no host sync.
 *   frames          4-byte aligned                                 frame_stride   % 4 == 0 and >= planes * plane_bytes
 *   plane_bytes     > 0, % 4 == 0                                  band_bytes     > 0, % 4 == 0 (may exceed plane_bytes: n = 1)
 *   band_crc_out    uint32 [n_frames][planes][n]                   frame_crc_out  uint32 [n_frames], or NULL
 *   workspace       l3c_u8_crc32_bands_workspace_bytes(...) bytes, 16-byte aligned; garbage on entry
 * planes in 1..1024, n_frames >= 1, n_frames * planes * n * chunks per band below 2^40.  Bytes between frames are never read into a result.
 */
int64_t l3c_u8_crc32_bands_workspace_bytes(int64_t n_frames, int planes, int64_t plane_bytes, int64_t band_bytes);
int l3c_u8_crc32_bands(const uint8_t *frames, int64_t n_frames, int planes, int64_t plane_bytes, int64_t band_bytes, int64_t frame_stride,
                       uint32_t *band_crc_out, uint32_t *frame_crc_out, void *workspace, int64_t workspace_bytes, l3c_stream_t stream);

/*
 * l3c_seal_append_bands: l3c_seal_append for band seals: the band table and the version-2 seal, l3c_seal_bands_bytes(n) bytes, behind
 * every file on the device, file_bytes[b] grows by as much.  A wavefront per file: the lanes share the check word's 12 + 3 n words.  A
 * band-sealed encode is l3c_encode_batch_banded, ONE l3c_u8_crc32_bands on desc.img (planes = 3, plane_bytes = H W, band_bytes = the
 * finest record's band length), l3c_seal_append_bands -- no host round trip.  It needs file_stride >=
 * l3c_encode_banded_file_stride(...) + l3c_seal_bands_bytes(n) rounded up to 32.
 *   frame_crc   uint32 [B]          band_crc   uint32 [B][3][n]: the outputs of l3c_u8_crc32_bands          n in 1..1024, band_len > 0
 * padding, model_id, file_bytes[b] == -1, a slot without room, B and file_stride: as for l3c_seal_append.
 */
int l3c_seal_append_bands(uint8_t *files, int64_t file_stride, int64_t *file_bytes, const uint32_t *frame_crc, const uint32_t *band_crc, int n,
                          uint32_t band_len, const uint16_t *padding, uint64_t model_id, int64_t B, l3c_stream_t stream);

/* ---- parity bands: rebuild a damaged band of the finest record (opt-in, band-sealed files only; INTEGRATION.md "Parity bands") ----------- */

/*
 * A band seal turns damage into ERASURES: l3c_u8_crc32_bands says which (channel, band) of the finest record failed.  Seal version 3 adds an
 * XOR parity over that record's band payloads (about 95 % of a file's bytes), RAID-5 style: one parity stream per group of G bands restores
 * one erased band per group exactly.
 *     body (the unsealed banded file) | PARITY SECTION | BAND TABLE (as in version 2) | the 24 seal bytes with version = 3
 *     PARITY SECTION, little-endian, S = 16 + 12 m + sum(plen) bytes:
 *       0 'L3CP' | 4 u16 G | 6 u16 m | 8 u32 plen[3][m] (channel-major) | 8 + 12 m the 3 m parity payloads, (c, g) order, back to back |
 *       S - 8 u32 S | S - 4 separator 46 E2 84 92
 *   n, G, m      n the bands per channel of the finest record, G in 1..n, m = ceil(n / G)
 *   groups       INTERLEAVED: group g of channel c holds the bands { j : j % m == g }; a channel's bands lie back to back in the file, so a
 *                burst over adjacent bands hits different groups
 *   payload      of (c, g): the XOR of its members' payloads, each zero-extended to plen[c][g], the longest member's byte count
 *   check        CRC-32 of the 8 padding bytes, section bytes [0, 8 + 12 m), the section's last 8 bytes, the band table, seal bytes 0..19.
 *                The parity PAYLOADS are not under it: a damaged parity stream must not make an intact file unreadable; it can only make a
 *                repair fail, which the band CRCs of the repaired pixels notice.
 * The section ends with the separator: the band table still starts behind one, and the recognition rule is unchanged.  A reader rejects,
 * "invalid file: seal ...": a section that does not start behind the body's last separator or lacks 'L3CP', an S other than 16 + 12 m +
 * sum(plen), G or m inconsistent with the finest record's n, a plen[c][g] that is not the largest length field of its members, a
 * version-3 seal on a legacy file, and everything a version-2 seal is rejected for.
 *
 * l3c_seal_find_parity is l3c_seal_find_bands that also hands out the section: *body_bytes_out is the size in front of the SECTION;
 * parity_out->plen and ->payloads point INTO the file (unaligned); versions 1 and 2 give m = 0.  l3c_seal_find and l3c_seal_find_bands
 * accept version 3 and return the same *body_bytes_out: every reader of band-sealed files reads a version-3 file as the band-sealed file
 * it contains.  l3c_seal_write_parity stores l3c_seal_parity_bytes(n, m, payload bytes) bytes: section, table and seal.
 *
 * THE REPAIR (Bitcoding.decode_repair; INTEGRATION.md "Parity bands") decodes as the salvage decode does, keeps the finest P and the symbols,
 * and goes in rounds.  The erasure of a failing band position is its lowest failing channel c; a group (file, c, g) is rebuilt when it
 * holds exactly one erasure and every other member verifies at channel c.  A round: the parity payloads needed go up, ONE l3c_u8_xor_spans
 * rebuilds every payload of the round in the decoders' aligned form, the positions' symbols are zeroed, ONE l3c_decode_rgb_entries decodes
 * them against the kept P, l3c_sym_to_u8, and ONE l3c_u8_crc32_spans hashes their bands again.  Rounds repeat while one verified a band
 * more; a payload counts as repaired only when all three channels of its position verify, and what still fails is concealed
 * (l3c_dmll_conceal).
 * The encoder side behind the C ABI is l3c_encode_batch_banded_parity (NativeCodec(parity=G)), at the end of this header.
 * The repair behind the C ABI (NativeCodec.decode_repair) is "REPAIR THROUGH THE C ABI" below: l3c_repair_round_plan + l3c_decode_repair_round.
 * NOT BUILT: repair in the set readers and in the region decode, verification of parity payloads that were never needed.
 */
typedef struct {
    int32_t G, m;                   /* bands per group, groups per channel; m == 0: no parity section */
    const uint8_t *plen;            /* 12 m bytes inside the file: [3][m] little-endian words, unaligned */
    const uint8_t *payloads;        /* the 3 m parity payloads, (c, g) order, back to back */
    int64_t payload_bytes;          /* sum of plen */
} l3c_seal_parity;
int64_t l3c_seal_parity_bytes(int n, int m, int64_t payload_bytes);    /* 16 + 12 m + payload_bytes + 20 + 12 n + 24 */
int l3c_seal_find_parity(const uint8_t *file_host, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out,
                         l3c_seal_parity *parity_out);
int l3c_seal_write_parity(const l3c_seal *seal_host, const uint8_t *padding8_host, const uint32_t *band_crc_host, int n, uint32_t band_len, int G,
                          const uint32_t *plen_host, const uint8_t *payloads_host, uint8_t *dst_host);

/*
 * R PARITY STREAMS PER GROUP (Bitcoding(parity=G, parity_streams=R), R in 2..4): any R damaged bands of a group come back exactly, and a
 * damaged parity row still leaves R - 1 usable.  The arithmetic is GF(2^8), polynomial 0x11D, alpha = 0x02: member k of group g of a channel is
 * band j = g + k m, its evaluation point x_k = alpha^k, and
 *     row r (0 <= r < R) of the group = XOR over its members k of (x_k)^r d_k,     every d_k zero-extended to plen[c][g]
 * so row 0 is the XOR parity above, byte for byte.  Distinct points need G <= 255.  One-byte members 0x01, 0x02, 0x80 give rows 0x83, 0x3F,
 * 0xE1, 0x96.  Any t <= R erased members are solvable from any t CONSECUTIVE rows r0 .. r0 + t - 1 (a diagonal times a Vandermonde matrix).
 * The seal version stays 3; the section is of a second kind, S = 20 + 12 m + R sum(plen) bytes:
 *       0 'L3CQ' | 4 u16 G | 6 u16 m | 8 u16 R | 10 u16 0 | 12 u32 plen[3][m] | 12 + 12 m the 3 m R payloads, (c, g, r) order, plen[c][g] bytes
 *       each | S - 8 u32 S | S - 4 separator
 *   check        the padding bytes, section bytes [0, 12 + 12 m), the section's last 8 bytes, the band table, seal bytes 0..19
 *   R = 1        is never written as 'L3CQ': l3c_seal_write_parity_rs with R = 1 stores l3c_seal_write_parity's bytes
 * A reader rejects R outside 2..4, a non-zero reserved field, G > 255, an S other than 20 + 12 m + R sum(plen), and everything an 'L3CP'
 * section is rejected for.  l3c_seal_find_parity_rs hands out either kind ('L3CP': R = 1; payload_bytes = R sum(plen)).  l3c_seal_find,
 * l3c_seal_find_bands and l3c_seal_find_parity accept an 'L3CQ' file and return the body size in front of the section and the band table;
 * l3c_seal_find_parity gives m = 0: every other reader reads the file as the band-sealed file it contains.
 * The repair rebuilds a group (file, c, g) that holds 1..R erasures while every other member verifies: the rows r0 .. r0 + t - 1 go up,
 * the t x t system is inverted on the host, and each rebuilt payload is ONE linear combination (one l3c_u8_gf_spans group) of those rows and
 * the present members.  r0 = 0 first; where the positions still fail and t < R, r0 = 1 .. R - t in later rounds.
 */
typedef struct {
    int32_t G, m, R;                /* bands per group, groups per channel (0: no parity section), parity streams per group */
    const uint8_t *plen;            /* 12 m bytes inside the file: [3][m] little-endian words, unaligned */
    const uint8_t *payloads;        /* the 3 m R parity payloads, (c, g, r) order, back to back */
    int64_t payload_bytes;          /* R times the sum of plen */
} l3c_seal_parity_rs;
int64_t l3c_seal_parity_rs_bytes(int n, int m, int R, int64_t payload_bytes);  /* section (either kind) + 20 + 12 n + 24; payload_bytes = R sum(plen) */
int l3c_seal_find_parity_rs(const uint8_t *file_host, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, l3c_seal_bands *bands_out,
                            l3c_seal_parity_rs *parity_out);
int l3c_seal_write_parity_rs(const l3c_seal *seal_host, const uint8_t *padding8_host, const uint32_t *band_crc_host, int n, uint32_t band_len, int G,
                             int R, const uint32_t *plen_host, const uint8_t *payloads_host, uint8_t *dst_host);

/*
 * The two kernels share one device fold (csrc/parity.hip): a block XORs a 4096-byte tile of ONE output stream over the stream's members,
 * grid.y = the output stream.  A thread owns 16 bytes of the tile: one 16-byte load per member where the member is 16-byte aligned, dword
 * loads otherwise; nothing at or behind a member's 4-byte-rounded end is read, the bytes of its last dword behind its length count as
 * zero; 16-byte stores where the slot is 16-byte aligned, dword stores otherwise.  Every argument is checked before the launch; no
 * allocation, no host synchronisation, no atomics.
 *
 * l3c_band_parity: the encoder side, lengths known on the device alone.  `scale`: the finest record's coder output, the two groups of
 * l3c_ac_band_intervals as l3c_container_write_banded takes them (C must be 3); band j < n - 1 of stream s = b 3 + c is row s (n - 1) + j
 * of out_full, band n - 1 row s of out_last.
 *   parity          uint8 [B][3][m][parity_stride], m = ceil(n / G): bytes [0, ((parity_nbytes + 3) / 4) * 4) of a slot are written, the
 *                   rest of the slot is the caller's and is not written
 *   parity_nbytes   uint32 [B][3][m]: the longest member's byte count, or L3C_AC_OVERRUN when a member reported L3C_AC_OVERRUN -- such
 *                   a member is not read and the slot is not written (that file is already -1)
 *   parity_stride   % 16 == 0 and >= max(stride_full, stride_last); the coder strides % 4 == 0; G in 1..n; B * 3 * m <= 65535
 * l3c_band_parity_groups: m for n and G, or L3C_ERR_INVALID_ARG.
 */
int l3c_band_parity_groups(int n, int G);
int l3c_band_parity(const l3c_banded_scale *scale_host, int64_t B, int G, uint8_t *parity, int64_t parity_stride, uint32_t *parity_nbytes,
                    l3c_stream_t stream);

/*
 * l3c_u8_xor_spans: the repair side, lengths known on the host.  Output slot g = bytes [out_spans[g].offset, ...) of `out` receives the XOR
 * of the spans [group_first[g], group_first[g + 1]) of `spans` inside `data`, each cut or zero-extended to out_spans[g].bytes, followed by
 * zero bytes up to ((bytes + 3) / 4) * 4 + 4: the aligned, zero-padded form l3c_container_read produces and the range decoders read.  A
 * group of one member is a copy; a group of none is zeros.  n_groups == 0 is a success with nothing launched.
 *   spans_host, out_spans_host, group_first_host    the tables on the host, validated before anything is launched
 *   spans, out_spans, group_first                   the caller's device copies of the same tables, 8-byte aligned
 *   span            offset % 4 == 0 and >= 0, bytes >= 0; the span's 4-byte-rounded end must lie inside data_bytes
 *   out span        offset % 4 == 0 and >= 0, bytes >= 0, offset + ((bytes + 3) / 4) * 4 + 4 <= out_bytes; slots must not overlap
 *                   (not checked) and `out` must not overlap `data`
 *   group_first     [n_groups + 1], ascending from 0 to n_spans; n_groups <= 65535
 * data and out 4-byte aligned (16-byte aligned data, out and offsets: the full load rate).
 */
int l3c_u8_xor_spans(const uint8_t *data, int64_t data_bytes, const l3c_u8_span *spans_host, const l3c_u8_span *spans, int64_t n_spans,
                     const int64_t *group_first_host, const int64_t *group_first, int64_t n_groups, const l3c_u8_span *out_spans_host,
                     const l3c_u8_span *out_spans, uint8_t *out, int64_t out_bytes, l3c_stream_t stream);

/*
 * The same two kernels over GF(2^8) (polynomial 0x11D, alpha = 0x02; the 'L3CQ' section above), four packed bytes per dword, no table, no LDS.
 *
 * l3c_band_parity_rs: l3c_band_parity for R in 1..4 rows per group.  A block reads each member's bytes ONCE for all R rows: Horner over the
 * members from the last to the first, acc_r = alpha^r acc_r ^ d_k.
 *   parity          uint8 [B][3][m][R][parity_stride]: row r of group (b, c, g); what is written of a slot is as in l3c_band_parity
 *   parity_nbytes   uint32 [B][3][m]: one length for the R rows of a group, or L3C_AC_OVERRUN -- then none of its R slots is written
 *   G               in 1..n, and <= 255 when R > 1; B * 3 * m <= 65535; everything else as l3c_band_parity
 *
 * l3c_u8_gf_spans: l3c_u8_xor_spans with one coefficient per span: slot g = XOR over its spans k of coef[k] * span k.  coef_host: the n_spans
 * bytes on the host, coef: the caller's device copy (no alignment asked).  coef = 1 everywhere gives l3c_u8_xor_spans' bytes; a span with
 * coef = 0 contributes nothing and is not read.  Tables, cut / zero-extension, output form, alignment and the no-overlap rule: l3c_u8_xor_spans'.
 */
int l3c_band_parity_rs(const l3c_banded_scale *scale_host, int64_t B, int G, int R, uint8_t *parity, int64_t parity_stride, uint32_t *parity_nbytes,
                       l3c_stream_t stream);
int l3c_u8_gf_spans(const uint8_t *data, int64_t data_bytes, const l3c_u8_span *spans_host, const l3c_u8_span *spans, const uint8_t *coef_host,
                    const uint8_t *coef, int64_t n_spans, const int64_t *group_first_host, const int64_t *group_first, int64_t n_groups,
                    const l3c_u8_span *out_spans_host, const l3c_u8_span *out_spans, uint8_t *out, int64_t out_bytes, l3c_stream_t stream);

/*
 * l3c_band_rebuild: the repair-side counterpart of l3c_band_parity_rs -- ALL t erased members of a group in one pass, in place.  Where
 * l3c_u8_gf_spans rebuilds one payload per output group (a group with t erasures reads its present members and its t rows t times), a block
 * here owns a 4096-byte tile of ONE group, loads every source of the group once, eight at a time, and keeps t accumulators:
 *     output e (e < t) of group g = XOR over the group's sources k of coef[4 k + e] * source k        GF(2^8), polynomial 0x11D
 * every source cut or zero-extended to out[e].bytes, the output followed by zero bytes up to ((bytes + 3) / 4) * 4 + 4 (l3c_u8_gf_spans'
 * form); the t outputs of a group may differ in length.  The powers alpha^i of a source's bytes are formed once for the t accumulators; a
 * source whose t coefficients are all 0 is not read; coefficient 1 costs no multiply.
 *   sources         entries [first_src, first_src + n_rows + n_members) of `src` / `coef`: the n_rows ROW sources first, then the members
 *   row source      a span of `rows` at ANY byte offset (the rows of a parity section lie back to back in the file): the aligned dwords
 *                   around it are read and funnel-shifted.  `rows` is 4-byte aligned and readable up to ((rows_bytes + 3) / 4) * 4 (as the
 *                   files of l3c_container_read); no dword is read that holds no byte of the span, and the bytes of a dword outside the span
 *                   count as zero
 *   member source   a span of `members`, offset % 4 == 0, its 4-byte-rounded end inside members_bytes: l3c_u8_xor_spans' load rules
 *   out[e]          a slot of the SAME `members` buffer (the stream area of a decode workspace): offset % 4 == 0, offset + ((bytes + 3) / 4)
 *                   * 4 + 4 <= members_bytes.  A slot that overlaps a member source of ANY group of the call, or another slot, is refused
 *                   (L3C_ERR_INVALID_ARG naming the group): the spans are sorted and swept on the host.  out[e], e >= t, is not read.
 *                   Nothing outside the slots is stored; 16-byte stores where a slot is 16-byte aligned, dword stores otherwise
 *   coef            uint8 [n_src][4], 4-byte aligned; coef[4 k + e], e >= t of a group that uses entry k, is not read
 *   src_host, coef_host, groups_host    the tables on the host, validated before anything is launched (the sweep allocates host memory:
 *                   3 words per member source and slot)
 *   src, coef, groups                   the caller's device copies, 8-byte aligned (coef: 4-byte)
 * n_groups <= 65535; n_groups == 0 is a success with nothing launched.  rows and members must not overlap.  No atomics, no device
 * allocation, no host synchronisation.
 */
typedef struct l3c_rebuild_group {
    int64_t first_src;                          /* sources [first_src, first_src + n_rows + n_members) of the tables: the rows first */
    int32_t n_rows, n_members, t, reserved;     /* n_rows in 1..4; n_members >= 0; t in 1..4 outputs; reserved 0 */
    l3c_u8_span out[4];                         /* out[e], e < t: a slot inside `members` */
} l3c_rebuild_group;
int l3c_band_rebuild(const uint8_t *rows, int64_t rows_bytes, uint8_t *members, int64_t members_bytes, const l3c_u8_span *src_host,
                     const l3c_u8_span *src, const uint8_t *coef_host, const uint8_t *coef, int64_t n_src, const l3c_rebuild_group *groups_host,
                     const l3c_rebuild_group *groups, int64_t n_groups, l3c_stream_t stream);

/*
 * REPAIR THROUGH THE C ABI (NativeCodec.decode_repair; INTEGRATION.md "Repair through the C ABI"): the rounds of THE REPAIR above as two
 * calls per round, a host planner and ONE device call.  The caller decodes with l3c_decode_batch_banded (desc.sym set), hashes the frames
 * with l3c_u8_crc32_bands, brings the 3 n words per file to the host, copies the parity SECTIONS of the files that have a failing band into
 * a device buffer `rows` (a section: the file's bytes from body_bytes of l3c_seal_find_parity_rs on, at any 4-byte aligned place), and then
 * loops { l3c_repair_round_plan; H2D of the round blob; l3c_decode_repair_round; D2H of crc_out; update the words } until a plan comes back
 * with n_groups == 0.
 *
 * l3c_repair_round_plan: pure host code (csrc/repair_plan.h), Bitcoding._repair's selection word for word.  A band FAILS where its word
 * differs from the file's table; the ERASURE of a failing position is its lowest failing channel; a group (file, c, g) is taken when it
 * holds t = 1..R erasures and every other member verifies at c; its window is the first r0 in 0..R - t that (file, c, g, bands, r0) is not
 * in `tried` with; groups in (file, c, g) order, the files of one row ('L3CP') first.  The coefficients are the inverse of the t x t matrix
 * (alpha^(k_e (r0 + i))) by Gauss-Jordan -- container.rs_repair_coefficients' element for element; l3c_repair_coefficients hands them out.
 *   plan_host        the blob of l3c_decode_plan_banded for these files' BODIES (checked again)
 *   files_host, file_bytes_host    the B WHOLE sealed files as the caller holds them; read with l3c_seal_find_parity_rs only.  A file
 *                    without a parity section plans nothing
 *   band_words_host  uint32 [B][3][n]: the current words of l3c_u8_crc32_bands / l3c_u8_crc32_spans
 *   section_at_host  int64 [B]: where file b's section starts inside `rows`, or -1; a planned group of a file at -1 is L3C_ERR_INVALID_ARG
 *   tried_host       the l3c_repair_group entries of all earlier rounds (the caller appends every blob's list)
 *   round_host       l3c_repair_round_plan_bytes(cfg, plan_host) bytes (an upper bound for any round), 8-byte aligned.  The blob is
 *                    self-describing (magic word, size at word 1, the cfg words; layout: csrc/repair_plan.h); *n_groups_out == 0 is a valid
 *                    result: nothing left to try.  l3c_repair_round_groups hands out its group list and its S positions.
 *
 * l3c_decode_repair_round: on main_stream  1. l3c_band_rebuild of the blob's groups, IN PLACE in the stream area of the decode's workspace
 * (l3c_decode_batch_banded_streams_offset)  2. one launch that zeroes the S positions' symbols in the three planes  3. ONE
 * l3c_decode_rgb_entries against the P the decode left (l3c_decode_batch_banded_p_offset), window mode 1, the blob's chunk count and lag
 * 4. l3c_sym_to_u8 on the frames  5. ONE l3c_u8_crc32_spans of the positions' 3 S bands into crc_out (channel-major: (c, e) at c S + e,
 * e the blob's position index).  The round blob is checked before a word of it is trusted: its header against the plan blob, then every
 * table that follows from its groups is made again on the host and compared (that copy is the one host allocation of the call); the row
 * spans against rows_bytes by l3c_band_rebuild.  side_stream is used only at lag 2 (16 positions or more) and must then be a stream of its
 * own.  Nothing synchronises with the host.  A blob with n_groups == 0 is a success with nothing enqueued.
 *   workspace        the decode's, untouched since l3c_decode_batch_banded returned (with its workspace_bytes)
 *   round, round_host    the blob on the device (16-byte aligned) and on the host
 *   round_workspace  l3c_decode_repair_round_workspace_bytes(cfg, plan_host, round_host) bytes, 16-byte aligned
 * Not built: repair in the set readers and in l3c_decode_region; head healing in C (container.heal_head runs before the decode).
 */
typedef struct l3c_repair_group {
    int32_t file, c, g, t, r0;      /* group g of channel c of file `file`: its t erased bands from the rows r0 .. r0 + t - 1 */
    int32_t bands[4];               /* the erased bands, ascending; bands[e] = 0 for e >= t */
} l3c_repair_group;
typedef struct {
    const l3c_codec_model *model_host;
    const void *plan_host;
    const void *round_host;
    const void *round;
    int64_t round_bytes;
    const uint8_t *rows;
    int64_t rows_bytes;
    void *workspace;
    int64_t workspace_bytes;
    int16_t *sym;                   /* [B][3][H][W], the decode's desc.sym */
    uint8_t *pixels;                /* [B][3][H][W] */
    uint32_t *crc_out;              /* [3 S] */
    void *round_workspace;
    int64_t round_workspace_bytes;
} l3c_decode_repair_round_desc;
int l3c_repair_coefficients(const int32_t *erased_host, int t, int r0, const int32_t *present_host, int n_present, uint8_t *rows_out,
                            uint8_t *members_out);     /* rows_out [t][t], members_out [t][n_present]; members k in 0..254, distinct */
int64_t l3c_repair_round_plan_bytes(const l3c_net_config *cfg_host, const void *plan_host);
int l3c_repair_round_plan(const l3c_net_config *cfg_host, const void *plan_host, const uint8_t *const *files_host, const int64_t *file_bytes_host,
                          const uint32_t *band_words_host, const int64_t *section_at_host, const l3c_repair_group *tried_host, int64_t n_tried,
                          void *round_host, int64_t round_bytes, int64_t *n_groups_out);
int l3c_repair_round_groups(const void *round_host, const l3c_repair_group **groups_out, int64_t *n_groups_out, const int32_t **positions_out,
                            int64_t *n_positions_out);     /* positions: int32 [S][2] = file | band, ascending; pointers into the blob */
int64_t l3c_decode_repair_round_workspace_bytes(const l3c_net_config *cfg_host, const void *plan_host, const void *round_host);
int l3c_decode_repair_round(const l3c_decode_repair_round_desc *desc_host, l3c_stream_t main_stream, l3c_stream_t side_stream);

/*
 * HEAD PARITY (Bitcoding(parity=G, parity_head=True)): the parity above covers the band payloads of the finest record; the HEAD of a file
 * is everything else in its body -- the 14-byte file header, every coarser record whole, and the header, length fields and separator of
 * the finest record.  The seal version stays 3; the section is of a third kind, 'L3CH': an 'L3CQ' section (R = 1 is allowed and written in
 * this shape too) with a HEAD PART between the finest record's rows and the section's last 8 bytes:
 *       0 'L3CH' | 4 u16 G | 6 u16 m | 8 u16 R (1..4) | 10 u16 0 | 12 u32 plen[3][m] | 12 + 12 m the 3 m R finest rows, (c, g, r) order |
 *       A = 12 + 12 m + R sum(plen): HEAD PART | S - 8 u32 S | S - 4 separator
 *   HEAD PART    u16 n_records (all scale records, the finest included) | u16 0
 *                FRAMING COPY: body[0:14]; per record, coarsest first: its 9 header bytes (u8 C, u16 H, u16 W, u32 L) and u32 nbytes[C][n]
 *                u32 head_crc: CRC-32 of body[0, P0), P0 where the finest record's header starts
 *                per head record k (every record but the finest): u32 crc[C][n_k], the CRC-32 of each band PAYLOAD | u16 G_k = min(G, n_k) |
 *                    u16 m_k = ceil(n_k / G_k) | u32 hplen[C][m_k], the longest member of each group
 *                the rows: per head record, (c, g, r) order, hplen[k][c][g] bytes each; groups, points and zero extension as above
 *                u32 head_check: CRC-32 of the head part from A up to the first row byte
 *   check        what it covers for 'L3CQ': the padding bytes, section bytes [0, 12 + 12 m), the section's last 8 bytes, the band table, seal
 *                bytes 0..19 -- the head part is guarded by head_check alone
 * A DAMAGED head part (one that cannot be walked, or whose head_check fails) never makes a file unreadable: every l3c_seal_find* reads
 * the file as the 'L3CQ' file it contains (l3c_seal_find_parity: m = 0, l3c_seal_find_parity_rs: the finest rows).  A head part whose
 * head_check holds but whose content contradicts itself, the band table or the body's size is "invalid file: seal head ...".
 * l3c_seal_find_head: 1 for a sealed file with an 'L3CH' section, 0 for every other file, L3C_ERR_INVALID_ARG as l3c_seal_find.  The section
 * is written on the device by l3c_seal_append_parity (below) and on the host by container.make_seal(head=...); healing a file from it is the
 * Python side's (container.heal_head).
 */
typedef struct {
    int64_t at, bytes;              /* the head part: file bytes [at, at + bytes), head_check in its last 4 */
    int32_t check_ok;               /* 1: head_check holds */
    int32_t n_records;              /* the scale records it states (0 where check_ok is 0) */
} l3c_seal_head;
int l3c_seal_find_head(const uint8_t *file_host, int64_t file_bytes, l3c_seal_head *head_out);

/*
 * The encoder side of the head part, both over ALL head records of a batch in ONE launch each, lengths known on the device alone;
 * scales_host: n_scales in 1..8 records of any C >= 1 as l3c_container_write_banded takes them.  Integer only, no atomics, no allocation,
 * no host synchronisation.
 *
 * l3c_head_parity: l3c_band_parity_rs per record with G_k = min(G, n_k), m_k = ceil(n_k / G_k).  grid.y runs over (record, b, c, g).
 *   parity          record k's slots uint8 [B][C_k][m_k][R][parity_stride] at parity + parity_offset_host[k] (multiples of 16; the caller sizes
 *                   the buffer); what is read of a member and written of a slot is as in l3c_band_parity
 *   parity_nbytes   uint32, record-major, [B][C_k][m_k] per record: one length for the R rows of a group, or L3C_AC_OVERRUN
 *   parity_stride   % 16 == 0 and >= every coder stride; the sum of B C_k m_k over the records <= 65535
 *
 * l3c_band_payload_crc32: zlib's CRC-32 of every band payload, crc_out uint32 record-major, [B][C_k][n_k] per record.  A wavefront per
 * payload; the word does not depend on the launch geometry.  Length 0 gives 0; a band that reported L3C_AC_OVERRUN gives 0 (its file is
 * refused anyway).  Nothing at or behind a payload's 4-byte-rounded end is read, the bytes of its last dword behind its length are masked.
 */
int l3c_head_parity(const l3c_banded_scale *scales_host, int n_scales, int64_t B, int G, int R, uint8_t *parity, const int64_t *parity_offset_host,
                    int64_t parity_stride, uint32_t *parity_nbytes, l3c_stream_t stream);
int l3c_band_payload_crc32(const l3c_banded_scale *scales_host, int n_scales, int64_t B, uint32_t *crc_out, l3c_stream_t stream);

/*
 * l3c_seal_append_parity: l3c_seal_append_bands for seal version 3 (csrc/seal_parity.hip): behind every file of a banded encode, at files +
 * b * file_stride + file_bytes[b], exactly what container.make_seal(body, ..., parity=(G, rows), head=..., head_framing=...) returns --
 * [section][band table][the 24 seal bytes, version 3] -- and file_bytes[b] grows by as much.  All inputs are on the device, where alone
 * the lengths are known; two launches, no host round trip:
 *   a block per file   prefix sums over the file's 3 m (and head) group lengths give every row's place and S; the block writes the
 *                      section's front and last 8 bytes, the table, the seal and the check word (a wavefront shares the words, as
 *                      l3c_seal_append_bands), and with `head` stages the head part's meta bytes in the workspace: the framing copy
 *                      (rebuilt from the records and the padding -- the bytes l3c_container_write_banded wrote; the body's size is
 *                      checked against them), head_crc over body[0, P0), the payload CRC words, G_k, m_k, hplen, then head_check over them
 *   grid (tiles x R, groups + 1, B)   a block copies a tile of ONE row from its 16-byte aligned slot to its place in the file, which has any
 *                      byte alignment: dword stores inside the row, byte stores for the up to three bytes at either edge
 * Section kinds: R == 1 && !head 'L3CP' (8-byte front, no R field), R > 1 && !head 'L3CQ', head 'L3CH' for every R; G as stated in the file is
 * min(G, n), plen[c][g] is parity_nbytes.
 *   scales_host     the records of the encode as l3c_container_write_banded took them, coarsest first, the finest (C == 3) last; without
 *                   `head` only the finest one's C, H, W and band_len are read
 *   frame_crc, band_crc     uint32 [B], uint32 [B][3][n]: the outputs of l3c_u8_crc32_bands on the padded frames
 *   parity, parity_stride, parity_nbytes     the slots [B][3][m][R][parity_stride] and lengths [B][3][m] of l3c_band_parity_rs on the finest
 *                   record with the same G and R (G > n there: pass min(G, n))
 *   head_parity, head_parity_offset_host, head_parity_stride, head_parity_nbytes, payload_crc     with `head`: the slots, offsets and lengths
 *                   of l3c_head_parity and the words of l3c_band_payload_crc32, both over scales_host[0 .. n_scales - 2]; else ignored
 *   padding, model_id     as for l3c_seal_append           G >= 1, R in 1..4, head 0 or 1, reserved 0
 *   workspace       l3c_seal_append_parity_workspace_bytes(...) bytes, 16-byte aligned; garbage on entry
 * file_bytes[b] == -1 stays -1.  A file becomes -1, and nothing of its slot is written, when a group length is L3C_AC_OVERRUN (or exceeds
 * its slot's stride), when -- with `head` -- a band length does or the body is not 14 + sum (9 + 4 C n + 4) + its payload bytes long, when
 * the section would reach 2^32 bytes, and when the slot has no room.  Nothing is stored outside [old end, new end) of a slot.
 * Limits: B * 3 * m <= 65535, with `head` the sum of B C_k m_k over the coarser records <= 65535 (beyond: L3C_ERR_UNSUPPORTED, "slice the
 * batch"), n_scales <= 8 (L3C_ERR_UNSUPPORTED) and >= 2 with `head`, min(G, n_k) <= 255 when R > 1; with `head` files and file_stride are
 * multiples of 4.  Every argument is checked before the first launch.
 */
typedef struct {
    uint8_t *files;                         /* [B][file_stride] */
    int64_t file_stride;
    int64_t *file_bytes;                    /* int64 [B], 8-byte aligned */
    int64_t B;
    const l3c_banded_scale *scales_host;
    int32_t n_scales;
    int32_t G, R, head, reserved;
    const uint16_t *padding;                /* uint16 [B][4] or NULL: zeros */
    uint64_t model_id;
    const uint32_t *frame_crc, *band_crc;
    const uint8_t *parity;
    int64_t parity_stride;
    const uint32_t *parity_nbytes;
    const uint8_t *head_parity;
    const int64_t *head_parity_offset_host;
    int64_t head_parity_stride;
    const uint32_t *head_parity_nbytes, *payload_crc;
    void *workspace;
    int64_t workspace_bytes;
} l3c_seal_parity_desc;
int64_t l3c_seal_append_parity_workspace_bytes(const l3c_banded_scale *scales_host, int n_scales, int64_t B, int G, int R, int head);
int l3c_seal_append_parity(const l3c_seal_parity_desc *desc_host, l3c_stream_t stream);

/*
 * The parity-sealed encode as ONE library call (the files of Bitcoding(bp, bands=K, seal='bands', parity=G, parity_streams=R,
 * parity_head=head) byte for byte): l3c_encode_batch_banded's schedule unchanged, then on the same stream l3c_u8_crc32_bands on desc.img,
 * l3c_band_parity_rs on the finest record, with `head` l3c_head_parity and l3c_band_payload_crc32 on the coarser ones, and
 * l3c_seal_append_parity -- the coder's outputs are still live in the workspace behind l3c_container_write_banded, which is why this is one
 * entry and not a recipe of calls.  l3c_encode_batch_desc as for l3c_encode_batch_banded; opts_host: G >= 1 (the files state min(G, n)),
 * R in 1..4, head 0 or 1, reserved 0, model_id as for l3c_seal_append.  Refusals as l3c_seal_append_parity's, before anything is enqueued.
 *   l3c_encode_banded_parity_file_stride   l3c_encode_banded_file_stride(...) + TAIL rounded up to 32, where with P_s = max(l3c_ac_max_bytes(L_s),
 *       l3c_ac_max_bytes(last band of scale s)), n_s bands per channel, G_s = min(G, n_s), m_s = ceil(n_s / G_s), C_s channels (3 at scale 0):
 *       TAIL = F + 12 m_0 + 3 m_0 R P_0 + 8 + (20 + 12 n_0) + 24,  F = 8 for R == 1 without head, else 12; and with head
 *            + META + sum over s >= 1 of C_s m_s R P_s + 4,  META = 4 + 14 + sum over all s of (9 + 4 C_s n_s) + 4 + sum over s >= 1 of
 *              (4 C_s n_s + 4 + 4 C_s m_s)
 *   l3c_encode_batch_banded_parity_workspace_bytes   l3c_encode_batch_banded_workspace_bytes(...) plus, each rounded up to 256: 4 B (frame
 *       CRCs), 12 B n_0 (band CRCs), l3c_u8_crc32_bands_workspace_bytes(B, 3, H W, L_0), 3 B m_0 R S_0 with S_0 = P_0 rounded up to 16 (the finest
 *       slots), 12 B m_0 (their lengths), l3c_seal_append_parity_workspace_bytes(...), and with head  sum over s >= 1 of B C_s m_s R S_h with
 *       S_h = the largest P_s, s >= 1, rounded up to 16 (the head slots), 4 sum B C_s m_s (their lengths), 4 sum B C_s n_s (the payload CRCs)
 */
typedef struct {
    int32_t G, R, head, reserved;
    uint64_t model_id;
} l3c_parity_opts;
int64_t l3c_encode_banded_parity_file_stride(const l3c_net_config *cfg_host, int H, int W, int bands, const l3c_parity_opts *opts_host);
int64_t l3c_encode_batch_banded_parity_workspace_bytes(const l3c_net_config *cfg_host, int64_t B, int H, int W, int bands,
                                                       const l3c_parity_opts *opts_host);
int l3c_encode_batch_banded_parity(const l3c_encode_batch_desc *desc_host, int bands, const l3c_parity_opts *opts_host, l3c_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* L3C_HIP_H_ */
