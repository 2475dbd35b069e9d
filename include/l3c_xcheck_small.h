/*
 * l3c_xcheck_small.h -- a second part of the C ABI of libl3c_hip_xcheck.so, the TEST-ONLY library of include/l3c_xcheck.h (the product
 * never loads it): the three thin conv kernels of csrc/conv_small.hip in their form from before they were rewritten to stream at
 * the memory rate (csrc/xcheck_small.hip holds their text unchanged).  tests/test_gpu_thin_kernels_bits.py asks the product's
 * l3c_rgb_head / l3c_to_q_quantize / l3c_dec_head for the same bits as these give.  Arguments and conventions of each entry: those of
 * the product entry of the same name in include/l3c_hip.h; l3c_xcheck_to_q_quantize holds the tile kernel only (Cf <= 64).
 * And the encoder's interval head in its earlier form (csrc/xcheck_iv.hip), see below.
 * (A header of its own: include/l3c_xcheck.h is the list tests/test_abi.py counts.)
 */
#ifndef L3C_XCHECK_SMALL_H_
#define L3C_XCHECK_SMALL_H_

#include "l3c_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int l3c_xcheck_rgb_head(const float *img, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                        const float *b3, int B, int H, int W, int Cf, float *out, float *shifted_out, l3c_stream_t stream);
int l3c_xcheck_to_q_quantize(const float *feat, const float *w, const float *b, const float *levels, int64_t B, int64_t HW,
                             int Cf, int C, int L, int16_t *sym, float *bn_q, float *bn, l3c_stream_t stream);
int l3c_xcheck_dec_head(const float *bn_q, const float *w, const float *b, const float *fuse, int64_t B, int64_t HW, int C,
                        int Cf, float *out, l3c_stream_t stream);

/* The encoder's interval head (csrc/dmll_kernels.hip: encode_intervals_kernel and fill_tile) in its form from before the 16-byte fill of
 * the 150-channel tiles and the compile-time shapes; csrc/xcheck_iv.hip holds its text unchanged.  Arguments and output layout: those of
 * l3c_dmll_encode_intervals.  tests/test_gpu_interval_head_bits.py asks the product for the same words. */
int l3c_xcheck_dmll_encode_intervals(const float *P, const int16_t *sym, const float *targets, int64_t B, int64_t HW, int C, int K,
                                     int rgb, int Lp, uint32_t *intervals, l3c_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
