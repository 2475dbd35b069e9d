// A caller of the REGION decode without torch: include/l3c_hip.h, libl3c_hip.so and the HIP runtime only (tests/test_gpu_native_region.py;
// the sibling of codec_banded_main.cpp, whose WEIGHTS / TABLES formats it reads).
//
//   codec_region_main WEIGHTS TABLES num_scales Cf C L K enc_blocks dec_blocks rgb_baseline dec_skip
//
// It makes a seeded 328 x 88 image, encodes it to a banded `.l3c` file of 16 bands per channel (l3c_encode_batch_banded), plans the bytes
// (l3c_decode_plan_banded), and region-decodes two boxes of them -- l3c_decode_region_plan, l3c_decode_region: rows [190, 215) of all
// columns, and rows [300, 328) x columns [5, 60) at the frame's short last granule -- comparing each with the same rows of its own input.
// Exit status 0: both boxes equal the image.  Every HIP and library status is checked; the first failure ends the program before
// anything else is started.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "l3c_hip.h"

static int die(const char *what, const char *detail = "") {
    fprintf(stderr, "codec_region_main: %s %s\n", what, detail);
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

template <typename T>
static int to_device(const std::vector<T> &host, void **dev) {
    HIP_OK(hipMalloc(dev, host.size() * sizeof(T) + 16));
    HIP_OK(hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// the weights, checked against the names and shapes the library enumerates, packed into one device buffer
static int load_model(const l3c_net_config &cfg, const char *weights, hipStream_t st, void **packed_out, int64_t *packed_bytes_out) {
    const int n = l3c_net_param_count(&cfg);
    if (n < 0) return die("l3c_net_param_count", l3c_last_error());
    FILE *f = fopen(weights, "rb");
    if (!f) return die("cannot open", weights);
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
        if (to_device(host, &dev[i])) return 1;
    }
    fclose(f);
    const int64_t packed_bytes = l3c_net_packed_bytes(&cfg), pack_ws = l3c_net_pack_workspace_bytes(&cfg);
    if (packed_bytes < 0 || pack_ws < 0) return die("size functions:", l3c_last_error());
    void *ws = nullptr;
    HIP_OK(hipMalloc(packed_out, packed_bytes));
    HIP_OK(hipMalloc(&ws, pack_ws));
    L3C_CALL(l3c_net_pack(&cfg, reinterpret_cast<const float *const *>(dev.data()), *packed_out, packed_bytes, ws, pack_ws, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipFree(ws));
    for (void *p : dev) HIP_OK(hipFree(p));
    *packed_bytes_out = packed_bytes;
    return 0;
}

// one box of the planned file -> 0 when its pixels equal the image's
static int decode_box(const l3c_codec_model &model, const std::vector<int64_t> &plan, const uint16_t *padding, const void *d_files, const void *d_plan,
                      const std::vector<uint8_t> &image, int H, int W, l3c_region_box box, hipStream_t st, hipStream_t side) {
    const l3c_net_config &cfg = *model.cfg_host;
    const int64_t plan_bytes = (int64_t)plan.size() * 8, cap = l3c_decode_region_plan_bytes(&cfg, plan.data());
    if (cap < 0) return die("l3c_decode_region_plan_bytes", l3c_last_error());
    std::vector<int64_t> region((size_t)cap / 8);
    l3c_region_info info;
    L3C_CALL(l3c_decode_region_plan(&cfg, plan.data(), plan_bytes, padding, &box, region.data(), cap, &info));
    const int bh = box.y1 - box.y0, bw = box.x1 - box.x0;
    if (info.out_rows != bh || info.out_cols != bw || info.frame_rows != H) return die("the region plan names another box or frame");
    l3c_decode_region_desc d;
    memset(&d, 0, sizeof(d));
    d.model_host = &model;
    d.files = static_cast<const uint8_t *>(d_files);
    d.plan_host = plan.data();
    d.plan = d_plan;
    d.plan_bytes = plan_bytes;
    d.region_host = region.data();
    d.region_bytes = region[1];          // word 1 of the blob: its size
    d.workspace_bytes = l3c_decode_region_workspace_bytes(&cfg, plan.data(), region.data());
    if (d.workspace_bytes < 0) return die("l3c_decode_region_workspace_bytes", l3c_last_error());
    void *d_region = nullptr, *pixels = nullptr, *ws = nullptr;
    if (to_device(region, &d_region)) return 1;
    HIP_OK(hipMalloc(&pixels, (size_t)3 * bh * bw));
    HIP_OK(hipMalloc(&ws, d.workspace_bytes));
    d.region = d_region;
    d.pixels = static_cast<uint8_t *>(pixels);
    d.workspace = ws;
    L3C_CALL(l3c_decode_region(&d, st, side));      // (the side stream is used when the region plan says lag 2)
    HIP_OK(hipStreamSynchronize(st));
    std::vector<uint8_t> out((size_t)3 * bh * bw);
    HIP_OK(hipMemcpy(out.data(), pixels, out.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_region));
    HIP_OK(hipFree(pixels));
    HIP_OK(hipFree(ws));
    for (int c = 0; c < 3; ++c)
        for (int y = 0; y < bh; ++y)
            if (memcmp(&out[((size_t)c * bh + y) * bw], &image[((size_t)c * H + box.y0 + y) * W + box.x0], (size_t)bw) != 0)
                return die("the decoded box differs from the image");
    printf("codec_region_main: rows [%d, %d) x columns [%d, %d): bands %d..%d of %d, conv rows %d..%d, decoder rows %d..%d, %lld of %lld streams, "
           "%lld of %lld payload bytes, workspace %lld bytes; equal to the image\n", box.y0, box.y1, box.x0, box.x1, info.bands[0], info.bands[1] - 1,
           info.n_bands, info.conv_rows[0], info.conv_rows[1] - 1, info.decoder_rows[0], info.decoder_rows[1] - 1, (long long)info.streams_used,
           (long long)info.streams_total, (long long)info.bytes_used, (long long)info.bytes_total, (long long)d.workspace_bytes);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 12) return die("usage: WEIGHTS TABLES num_scales Cf C L K enc_blocks dec_blocks rgb_baseline dec_skip");
    const int H = 328, W = 88, bands = 16;
    l3c_net_config cfg;
    int *fields[9] = {&cfg.num_scales, &cfg.Cf, &cfg.C, &cfg.L, &cfg.K, &cfg.enc_blocks, &cfg.dec_blocks, &cfg.rgb_baseline, &cfg.dec_skip};
    for (int i = 0; i < 9; ++i) *fields[i] = atoi(argv[3 + i]);

    hipStream_t st, side;
    HIP_OK(hipStreamCreate(&st));
    HIP_OK(hipStreamCreate(&side));
    l3c_codec_model model;
    memset(&model, 0, sizeof(model));
    model.cfg_host = &cfg;
    void *packed = nullptr;
    if (load_model(cfg, argv[1], st, &packed, &model.packed_bytes)) return 1;
    model.packed = packed;

    // the three tables
    FILE *f = fopen(argv[2], "rb");
    if (!f) return die("cannot open", argv[2]);
    char magic[4];
    uint32_t L = 0;
    if (!read_n(f, magic, 4) || memcmp(magic, "L3CT", 4) != 0 || !read_n(f, &L, 1) || (int)L != cfg.L) return die("tables file: bad header");
    std::vector<float> t_rgb(257), t_z(L + 1);
    std::vector<uint16_t> row(L + 1);
    if (!read_n(f, &model.z_x_min, 1) || !read_n(f, &model.z_bin_width, 1) || !read_n(f, t_rgb.data(), t_rgb.size()) ||
        !read_n(f, t_z.data(), t_z.size()) || !read_n(f, row.data(), row.size()))
        return die("tables file: truncated");
    fclose(f);
    void *d_rgb = nullptr, *d_z = nullptr, *d_row = nullptr;
    if (to_device(t_rgb, &d_rgb) || to_device(t_z, &d_z) || to_device(row, &d_row)) return 1;
    model.targets_rgb = static_cast<const float *>(d_rgb);
    model.targets_z = static_cast<const float *>(d_z);
    model.uniform_row = static_cast<const uint16_t *>(d_row);

    // the image: smooth gradients per channel plus seeded noise, planar [3][H][W]
    std::vector<uint8_t> image((size_t)3 * H * W);
    uint32_t seed = 20240607u;
    for (int c = 0; c < 3; ++c)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                seed = seed * 1664525u + 1013904223u;
                image[((size_t)c * H + y) * W + x] = (uint8_t)((y * (c + 2) + x * (3 - c)) / 3 + (seed >> 28));
            }

    // ---- encode
    std::vector<uint8_t> file;
    {
        l3c_encode_batch_desc d;
        memset(&d, 0, sizeof(d));
        d.model_host = &model;
        d.B = 1;
        d.H = H;
        d.W = W;
        d.file_stride = l3c_encode_banded_file_stride(&cfg, H, W, bands);
        d.workspace_bytes = l3c_encode_batch_banded_workspace_bytes(&cfg, 1, H, W, bands);
        if (d.file_stride < 0 || d.workspace_bytes < 0) return die("size functions:", l3c_last_error());
        void *img = nullptr, *files = nullptr, *file_bytes = nullptr, *ws = nullptr;
        if (to_device(image, &img)) return 1;
        HIP_OK(hipMalloc(&files, d.file_stride));
        HIP_OK(hipMalloc(&file_bytes, 16));
        HIP_OK(hipMalloc(&ws, d.workspace_bytes));
        d.img = static_cast<const uint8_t *>(img);
        d.files = static_cast<uint8_t *>(files);
        d.file_bytes = static_cast<int64_t *>(file_bytes);
        d.workspace = ws;
        L3C_CALL(l3c_encode_batch_banded(&d, bands, st));
        HIP_OK(hipStreamSynchronize(st));
        int64_t n = 0;
        HIP_OK(hipMemcpy(&n, file_bytes, 8, hipMemcpyDeviceToHost));
        if (n < 0 || n > d.file_stride) return die("range coder overrun: no file");
        file.resize((size_t)n);
        HIP_OK(hipMemcpy(file.data(), files, file.size(), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(img));
        HIP_OK(hipFree(files));
        HIP_OK(hipFree(file_bytes));
        HIP_OK(hipFree(ws));
        printf("codec_region_main: %d x %d, %d bands -> %lld bytes\n", H, W, bands, (long long)n);
    }

    // ---- plan the bytes just written once, region-decode two boxes of them
    const int64_t offs[2] = {0, (int64_t)file.size()};
    file.resize(file.size() + 8, 0);
    const int64_t plan_bytes = l3c_decode_plan_banded_bytes(&cfg, file.data(), offs, 1);
    if (plan_bytes < 0) return die("l3c_decode_plan_banded_bytes", l3c_last_error());
    std::vector<int64_t> plan((size_t)plan_bytes / 8);
    int h = 0, w = 0;
    uint16_t padding[4];
    L3C_CALL(l3c_decode_plan_banded(&cfg, file.data(), offs, 1, plan.data(), plan_bytes, &h, &w, padding));
    if (h != H || w != W || padding[0] || padding[1] || padding[2] || padding[3]) return die("the plan names another shape or padding");
    void *d_files = nullptr, *d_plan = nullptr;
    if (to_device(file, &d_files) || to_device(plan, &d_plan)) return 1;
    const l3c_region_box boxes[2] = {{190, 215, 0, W}, {300, H, 5, 60}};
    for (const l3c_region_box &box : boxes)
        if (decode_box(model, plan, padding, d_files, d_plan, image, H, W, box, st, side)) return 1;
    HIP_OK(hipFree(d_files));
    HIP_OK(hipFree(d_plan));
    HIP_OK(hipFree(d_rgb));
    HIP_OK(hipFree(d_z));
    HIP_OK(hipFree(d_row));
    HIP_OK(hipFree(packed));
    HIP_OK(hipStreamDestroy(side));
    HIP_OK(hipStreamDestroy(st));
    return 0;
}

