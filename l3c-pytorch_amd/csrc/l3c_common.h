// l3c_common.h -- shared host-side plumbing of libl3c_hip.so (error reporting, launch checks).
#ifndef L3C_COMMON_H_
#define L3C_COMMON_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/l3c_hip.h"

namespace l3c {

char *error_buffer();  // thread-local, defined in l3c_api.hip

inline int fail(int code, const char *fmt, const char *a = "", long long b = 0, long long c = 0) {
    snprintf(error_buffer(), 512, fmt, a, b, c);
    return code;
}

inline int check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return L3C_OK;
    snprintf(error_buffer(), 512, "%s: %s", what, hipGetErrorString(e));
    return L3C_ERR_HIP;
}

inline int check_launch(const char *kernel) { return check_hip(hipGetLastError(), kernel); }

inline hipStream_t as_stream(l3c_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// l3c_ac_decode_chunks for ragged parts whose streams end in DIFFERENT chunks (csrc/ac_kernels.hip; the caller is l3c_decode_rgb_entries):
// stream s of every part ends with chunk final_chunk_dev[s] (device int32 [n_streams]), part i is chunk chunk_host[i] of its channel, and
// a stream with r_npix[s] == 0 only carries its state record on.  parts[i].final_chunk is ignored.
int ac_decode_chunks_entries(const l3c_ac_decode_part *parts, int n_parts, const int32_t *final_chunk_dev, const int *chunk_host,
                             l3c_stream_t stream);

// what l3c_u8_gather / l3c_u8_scatter check of their table and frame before a launch (csrc/images.hip), for the codec entries that wrap
// them: B, Hp, Wp in range, Wp a multiple of 4, the device table 16-byte aligned, every view inside [0, buffer_bytes) (csrc/image_table.h)
int images_check(const l3c_u8_image *images_host, const l3c_u8_image *images, int64_t B, int Hp, int Wp, int64_t buffer_bytes);

}  // namespace l3c

#define L3C_REQUIRE(cond, msg)                                                         \
    do {                                                                               \
        if (!(cond)) return l3c::fail(L3C_ERR_INVALID_ARG, "%s (" #cond ")", msg);     \
    } while (0)

#endif
