// seal.h -- the 24-byte seal behind a `.l3c` file's last separator (include/l3c_hip.h: l3c_seal_find / l3c_seal_write; the Python mirror is
// bitcoding/container.py: split_seal / make_seal).
//
// Plain C++17 on purpose, as codec_plan.h and image_table.h: no HIP include, no library call, no allocation, so that the code that reads
// untrusted file bytes compiles into a stand-alone program (tests/cabi/seal_check_main.cpp, built with the address and undefined-behaviour
// sanitizers) as well as into libl3c_hip.so (csrc/crc.hip).
//
//     0 'L3CS' | 4 u8 version = 1 | 5 u8 flags = 0 | 6 u16 generation | 8 u32 frame CRC | 12 u64 model id | 20 u32 check        little-endian
//
// check = CRC-32 (zlib) of the file's 8 padding bytes -- file bytes 0..7, in a banded file ('L3CB') bytes 6..13 -- followed by seal bytes
// 0..19.  A file is SEALED exactly when it has at least 28 bytes, bytes [-24, -20) are 'L3CS' and bytes [-28, -24) are the scale separator
// every unsealed file ends with; a recognised seal that is damaged is an error, never "unsealed".
#ifndef L3C_SEAL_H_
#define L3C_SEAL_H_

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/l3c_hip.h"

namespace l3c_sealing {

constexpr int VERSION = 1;
constexpr uint8_t SIGNATURE[4] = {'L', '3', 'C', 'S'};
constexpr uint8_t SEPARATOR[4] = {0x46, 0xE2, 0x84, 0x92};
constexpr uint8_t BANDED_SIGNATURE[4] = {'L', '3', 'C', 'B'};

// zlib's CRC-32, bit by bit: the seal hashes 28 bytes
inline uint32_t crc32(uint32_t crc, const uint8_t *p, int64_t n) {
    crc = ~crc;
    for (int64_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

inline void put(uint8_t *dst, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; ++i) dst[i] = (uint8_t)(v >> (8 * i));
}

inline uint64_t get(const uint8_t *src, int bytes) {
    uint64_t v = 0;
    for (int i = 0; i < bytes; ++i) v |= (uint64_t)src[i] << (8 * i);
    return v;
}

inline int fail(char *err, size_t cap, const char *what) {
    if (err && cap) snprintf(err, cap, "invalid file: seal %s", what);
    return L3C_ERR_INVALID_ARG;
}

// seal bytes 0..19 of `s`, then the check word over padding8 | those bytes
inline void write(const l3c_seal &s, const uint8_t *padding8, uint8_t *dst) {
    memcpy(dst, SIGNATURE, 4);
    dst[4] = VERSION;
    dst[5] = 0;
    put(dst + 6, s.generation, 2);
    put(dst + 8, s.frame_crc, 4);
    put(dst + 12, s.model_id, 8);
    put(dst + 20, crc32(crc32(0, padding8, 8), dst, 20), 4);
}

// 1: sealed, 0: unsealed, L3C_ERR_INVALID_ARG (message in err): a recognised seal that is damaged
inline int find(const uint8_t *file, int64_t file_bytes, int64_t *body_bytes_out, l3c_seal *seal_out, char *err, size_t cap) {
    if (body_bytes_out) *body_bytes_out = file_bytes;
    if (file_bytes < L3C_SEAL_BYTES + 4) return 0;
    const uint8_t *s = file + file_bytes - L3C_SEAL_BYTES;
    if (memcmp(s, SIGNATURE, 4) != 0 || memcmp(s - 4, SEPARATOR, 4) != 0) return 0;
    const int64_t body = file_bytes - L3C_SEAL_BYTES;
    const int64_t padding_at = memcmp(file, BANDED_SIGNATURE, 4) == 0 ? 6 : 0;
    if (s[4] != VERSION) return fail(err, cap, "of an unknown version");
    if (s[5] != 0) return fail(err, cap, "with non-zero flags");
    if (padding_at + 8 > body) return fail(err, cap, "on a file too short for its padding fields");
    if (get(s + 20, 4) != crc32(crc32(0, file + padding_at, 8), s, 20)) return fail(err, cap, "check word does not match (damaged seal or padding fields)");
    if (body_bytes_out) *body_bytes_out = body;
    if (seal_out) {
        seal_out->generation = (uint16_t)get(s + 6, 2);
        seal_out->frame_crc = (uint32_t)get(s + 8, 4);
        seal_out->model_id = get(s + 12, 8);
    }
    return 1;
}

}  // namespace l3c_sealing

#endif
