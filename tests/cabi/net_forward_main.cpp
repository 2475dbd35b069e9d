// A caller of the network without torch: include/l3c_hip.h, libl3c_hip.so and the HIP runtime only (tests/test_gpu_net_abi.py).
//
//   net_forward_main WEIGHTS IMAGE OUT_DIR num_scales Cf C L K enc_blocks dec_blocks rgb_baseline dec_skip
//
// WEIGHTS  "L3CW", u32 count, then per tensor in l3c_net_param order: u32 name length, name, u32 rank, i64 shape[rank], fp32 data
// IMAGE    i64 B, H, W, then fp32 [B][3][H][W] (0..255)
// writes OUT_DIR/sym<s>.bin (int16, s = 0 .. num_scales) and OUT_DIR/P<s>.bin (fp32 pixel-major [B][H>>s][W>>s][Kp], s < num_scales)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "l3c_hip.h"

static int die(const char *what, const char *detail = "") {
    fprintf(stderr, "net_forward_main: %s %s\n", what, detail);
    return 1;
}

#define HIP_OK(x)                                                         \
    do {                                                                  \
        hipError_t e_ = (x);                                              \
        if (e_ != hipSuccess) return die(#x, hipGetErrorString(e_));      \
    } while (0)
#define L3C_CALL(x)                                                       \
    do {                                                                  \
        if ((x) != L3C_OK) return die(#x, l3c_last_error());              \
    } while (0)

template <typename T>
static bool read_n(FILE *f, T *v, size_t n) { return fread(v, sizeof(T), n, f) == n; }

static bool write_file(const std::string &path, const void *p, size_t bytes) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
    if (argc != 13) return die("usage: WEIGHTS IMAGE OUT_DIR num_scales Cf C L K enc_blocks dec_blocks rgb_baseline dec_skip");
    l3c_net_config cfg;
    int *fields[9] = {&cfg.num_scales, &cfg.Cf, &cfg.C, &cfg.L, &cfg.K, &cfg.enc_blocks, &cfg.dec_blocks, &cfg.rgb_baseline, &cfg.dec_skip};
    for (int i = 0; i < 9; ++i) *fields[i] = atoi(argv[4 + i]);
    const std::string out_dir = argv[3];

    // 1. the weights, checked against the names and shapes the library enumerates
    const int n = l3c_net_param_count(&cfg);
    if (n < 0) return die("l3c_net_param_count", l3c_last_error());
    FILE *f = fopen(argv[1], "rb");
    if (!f) return die("cannot open", argv[1]);
    char magic[4];
    uint32_t count = 0;
    if (!read_n(f, magic, 4) || memcmp(magic, "L3CW", 4) != 0 || !read_n(f, &count, 1) || (int)count != n)
        return die("weights file: bad header or tensor count");
    std::vector<void *> dev(n, nullptr);
    for (int i = 0; i < n; ++i) {
        char name[256];
        int ndim = 0;
        int64_t shape[4];
        L3C_CALL(l3c_net_param(&cfg, i, name, sizeof(name), &ndim, shape));
        uint32_t len = 0, rank = 0;
        if (!read_n(f, &len, 1) || len >= 256) return die("weights file: bad name length at tensor", name);
        std::string got(len, '\0');
        if (!read_n(f, &got[0], len) || got != name) return die("weights file: tensor name differs from", name);
        if (!read_n(f, &rank, 1) || (int)rank != ndim) return die("weights file: rank differs for", name);
        int64_t numel = 1;
        for (int k = 0; k < ndim; ++k) {
            int64_t e = 0;
            if (!read_n(f, &e, 1) || e != shape[k]) return die("weights file: shape differs for", name);
            numel *= e;
        }
        std::vector<float> host((size_t)numel);
        if (!read_n(f, host.data(), host.size())) return die("weights file: truncated at", name);
        HIP_OK(hipMalloc(&dev[i], host.size() * sizeof(float)));
        HIP_OK(hipMemcpy(dev[i], host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    fclose(f);

    // 2. the image
    f = fopen(argv[2], "rb");
    if (!f) return die("cannot open", argv[2]);
    int64_t dims[3];
    if (!read_n(f, dims, 3)) return die("image file: bad header");
    const int64_t B = dims[0];
    const int H = (int)dims[1], W = (int)dims[2];
    std::vector<float> img((size_t)(B * 3 * H * W));
    if (!read_n(f, img.data(), img.size())) return die("image file: truncated");
    fclose(f);

    hipStream_t st;
    HIP_OK(hipStreamCreate(&st));
    // 3. pack
    const int64_t packed_bytes = l3c_net_packed_bytes(&cfg), pack_ws = l3c_net_pack_workspace_bytes(&cfg);
    if (packed_bytes < 0 || pack_ws < 0) return die("size functions:", l3c_last_error());
    void *packed = nullptr, *ws = nullptr, *d_img = nullptr;
    HIP_OK(hipMalloc(&packed, packed_bytes));
    HIP_OK(hipMalloc(&ws, pack_ws));
    L3C_CALL(l3c_net_pack(&cfg, reinterpret_cast<const float *const *>(dev.data()), packed, packed_bytes, ws, pack_ws, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipFree(ws));
    for (void *p : dev) HIP_OK(hipFree(p));

    // 4. forward
    HIP_OK(hipMalloc(&d_img, img.size() * sizeof(float)));
    HIP_OK(hipMemcpy(d_img, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    l3c_net_forward_desc d;
    memset(&d, 0, sizeof(d));
    d.cfg_host = &cfg;
    d.packed = packed;
    d.packed_bytes = packed_bytes;
    d.img = static_cast<const float *>(d_img);
    d.B = B;
    d.H = H;
    d.W = W;
    const int S = cfg.num_scales;
    std::vector<size_t> sym_n(S + 1), P_n(S);
    for (int s = 0; s <= S; ++s) {
        const int64_t hw = (int64_t)(H >> s) * (W >> s);
        sym_n[s] = (size_t)(B * (s ? cfg.C : 3) * hw);
        HIP_OK(hipMalloc(reinterpret_cast<void **>(&d.sym[s]), sym_n[s] * sizeof(int16_t)));
        if (s) HIP_OK(hipMalloc(reinterpret_cast<void **>(&d.bn_q[s]), sym_n[s] * sizeof(float)));
        if (s < S) {
            const int Cp = s == 0 ? 3 : cfg.C;
            P_n[s] = (size_t)(B * hw * (Cp == 3 ? 4 : 3) * Cp * cfg.K);
            HIP_OK(hipMalloc(reinterpret_cast<void **>(&d.P[s]), P_n[s] * sizeof(float)));
        }
    }
    d.workspace_bytes = l3c_net_forward_workspace_bytes(&cfg, B, H, W);
    if (d.workspace_bytes < 0) return die("l3c_net_forward_workspace_bytes", l3c_last_error());
    HIP_OK(hipMalloc(&d.workspace, d.workspace_bytes));
    L3C_CALL(l3c_net_forward(&d, st));
    HIP_OK(hipStreamSynchronize(st));

    // 5. outputs
    for (int s = 0; s <= S; ++s) {
        std::vector<int16_t> sym(sym_n[s]);
        HIP_OK(hipMemcpy(sym.data(), d.sym[s], sym.size() * sizeof(int16_t), hipMemcpyDeviceToHost));
        if (!write_file(out_dir + "/sym" + std::to_string(s) + ".bin", sym.data(), sym.size() * sizeof(int16_t))) return die("cannot write sym");
        if (s < S) {
            std::vector<float> P(P_n[s]);
            HIP_OK(hipMemcpy(P.data(), d.P[s], P.size() * sizeof(float), hipMemcpyDeviceToHost));
            if (!write_file(out_dir + "/P" + std::to_string(s) + ".bin", P.data(), P.size() * sizeof(float))) return die("cannot write P");
        }
    }
    for (int s = 0; s <= S; ++s) {
        HIP_OK(hipFree(d.sym[s]));
        if (s) HIP_OK(hipFree(d.bn_q[s]));
        if (s < S) HIP_OK(hipFree(d.P[s]));
    }
    HIP_OK(hipFree(d.workspace));
    HIP_OK(hipFree(d_img));
    HIP_OK(hipFree(packed));
    HIP_OK(hipStreamDestroy(st));
    printf("net_forward_main: %d tensors, %lld x %d x %d, %d scales\n", n, (long long)B, H, W, S);
    return 0;
}
