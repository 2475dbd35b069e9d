// banded_rows.h -- where a band's payload and its length lie in the coder output of one record of a banded encode (include/l3c_hip.h:
// l3c_banded_scale, the two groups of l3c_ac_band_intervals).  Shared by csrc/parity.hip and csrc/crc.hip.
#ifndef L3C_BANDED_ROWS_H_
#define L3C_BANDED_ROWS_H_

#include <stdint.h>

#include "../../include/l3c_hip.h"

// band j of stream s (= b C + c) of a record of n bands per channel
__device__ __forceinline__ const uint8_t *band_row(const l3c_banded_scale &sc, int64_t n, int64_t s, int64_t j) {
    return j + 1 < n ? sc.out_full + (s * (n - 1) + j) * sc.stride_full : sc.out_last + s * sc.stride_last;
}
__device__ __forceinline__ uint32_t band_nbytes(const l3c_banded_scale &sc, int64_t n, int64_t s, int64_t j) {
    return j + 1 < n ? sc.nbytes_full[s * (n - 1) + j] : sc.nbytes_last[s];
}

#endif
