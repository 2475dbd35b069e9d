// net.hip -- the whole network behind two library calls: l3c_net_forward / l3c_net_get_p (include/l3c_hip.h), and the finest scale's
// l3c_net_get_p on a row window: l3c_net_get_p_rows (the row arithmetic: csrc/codec_plan_region.h).
//
// A host loop over the layer schedule of modules/multiscale_network.py: the same entry points, with the descriptors ops.conv builds
// for the same layer, in the same order -- so every kernel sees the same inputs and sums in the same order, and P is bit-identical to
// the Python schedule's.  Three small kernels of its own: the image's symbols, and at pack time the two weight rearrangements that
// ops.PackedConv does with torch indexing (polyphase concatenation of the 5x5 stride-2 kernels, sub-pixel-major rows of the
// PixelShuffle tail).
#include <string.h>

#include <string>
#include <vector>

#include "codec_plan_region.h"
#include "l3c_common.h"

#define NET_FAIL(code, ...) (snprintf(l3c::error_buffer(), 512, __VA_ARGS__), (code))

namespace {

constexpr int64_t NET_ALIGN = 256;
constexpr int MAX_BLOCKS = 64;
inline int64_t align_up(int64_t x) { return (x + NET_ALIGN - 1) / NET_ALIGN * NET_ALIGN; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int grid_for(int64_t total) {
    const int64_t g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// Out.append_input_image: x.round() (half to even) -> int16
__global__ __launch_bounds__(256) void image_symbols_kernel(const float *__restrict__ img, int64_t n, int16_t *__restrict__ sym) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        sym[i] = (int16_t)(long long)rintf(img[i]);
}

// ops.PackedConv, 5x5 stride 2: w_cat[co][(2a+b) Cin + ci][u][v] = w[co][ci][2u+a][2v+b], zero where 2u+a or 2v+b exceeds 4
__global__ __launch_bounds__(256) void polyphase_concat_kernel(const float *__restrict__ w, int Cout, int Cin, float *__restrict__ w_cat) {
    const int64_t total = (int64_t)Cout * 4 * Cin * 9;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int uv = (int)(i % 9);
        const int k = (int)((i / 9) % (4 * Cin));
        const int64_t co = i / (9 * 4 * (int64_t)Cin);
        const int ph = k / Cin, ci = k % Cin;
        const int y = 2 * (uv / 3) + (ph >> 1), x = 2 * (uv % 3) + (ph & 1);
        w_cat[i] = (y <= 4 && x <= 4) ? w[((co * Cin + ci) * 5 + y) * 5 + x] : 0.f;
    }
}

// ops.PackedConv.packed_wino4_shuffle: row (Cout/4) s + oc of the result = row 4 oc + s of the layer's OIHW weights
__global__ __launch_bounds__(256) void subpixel_rows_kernel(const float *__restrict__ w, int Cout, int row_len, float *__restrict__ out) {
    const int64_t total = (int64_t)Cout * row_len;
    const int c4 = Cout / 4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / row_len);
        const int64_t e = i % row_len;
        out[i] = w[(int64_t)((r % c4) * 4 + r / c4) * row_len + e];
    }
}

// ---- the checkpoint's tensors (modules/schema.param_schema) ------------------------------------------------------------------

struct Param {
    std::string name;
    int ndim;
    int64_t shape[4];
};

int kp_of(const l3c_net_config &c, int s) {   // schema.non_shared_get_Kp(K, 3 if (rgb or s == 0) else C)
    const int Cp = (c.rgb_baseline || s == 0) ? 3 : c.C;
    return (Cp == 3 ? 4 : 3) * Cp * c.K;
}

void add_conv(std::vector<Param> &v, const std::string &key, int cout, int cin, int k) {
    v.push_back({key + ".weight", 4, {cout, cin, k, k}});
    v.push_back({key + ".bias", 1, {cout, 0, 0, 0}});
}

void add_body(std::vector<Param> &v, const std::string &prefix, int Cf, int n) {
    for (int i = 0; i < n; ++i) {
        add_conv(v, prefix + "." + std::to_string(i) + ".body.0", Cf, Cf, 3);
        add_conv(v, prefix + "." + std::to_string(i) + ".body.2", Cf, Cf, 3);
    }
    add_conv(v, prefix + "." + std::to_string(n), Cf, Cf, 3);
}

std::vector<Param> schema(const l3c_net_config &c) {
    std::vector<Param> v;
    const int Cf = c.Cf;
    add_conv(v, "sub_rgb_mean", 3, 3, 1);
    if (!c.rgb_baseline) {
        add_conv(v, "heads.0.head.0", 3, 3, 1);
        add_conv(v, "heads.0.head.1.head", Cf, 3, 3);
        for (int s = 1; s < c.num_scales; ++s) add_conv(v, "heads." + std::to_string(s) + ".head", Cf, Cf, 3);   // enc.feed_F
    }
    for (int s = 0; s < c.num_scales; ++s) {
        const std::string p = "nets." + std::to_string(s);
        if (!c.rgb_baseline) {
            v.push_back({p + ".enc.levels", 1, {c.L, 0, 0, 0}});
            add_conv(v, p + ".enc.down", Cf, Cf, 5);
            add_body(v, p + ".enc.body", Cf, c.enc_blocks);
            add_conv(v, p + ".enc.to_q.0", c.C, Cf, 1);
            v.push_back({p + ".enc.q.levels", 1, {c.L, 0, 0, 0}});
        }
        add_conv(v, p + ".dec.head", Cf, c.C, 1);
        add_body(v, p + ".dec.body", Cf, c.dec_blocks);
        add_conv(v, p + ".dec.tail.0", 4 * Cf, Cf, 3);
    }
    for (int s = 0; s < c.num_scales; ++s) {
        const std::string p = "prob_clfs." + std::to_string(s) + ".atrous";
        for (int i = 0; i < 3; ++i) add_conv(v, p + ".atrous." + std::to_string(i), Cf, Cf, 3);
        add_conv(v, p + ".lin", kp_of(c, s), 3 * Cf, 1);
    }
    return v;
}

int check_config(const l3c_net_config *c, bool compute) {
    L3C_REQUIRE(c, "null config");
    L3C_REQUIRE(c->num_scales >= 1 && c->num_scales <= L3C_NET_MAX_SCALES, "num_scales must be 1 .. L3C_NET_MAX_SCALES");
    L3C_REQUIRE(c->Cf > 0 && c->Cf <= 1024 && c->C > 0 && c->C <= 1024 && c->K > 0 && c->K <= 1024 && c->L > 0 && c->L <= 32767,
                "bad config sizes");
    L3C_REQUIRE(c->enc_blocks >= 0 && c->enc_blocks <= MAX_BLOCKS && c->dec_blocks >= 0 && c->dec_blocks <= MAX_BLOCKS,
                "enc_blocks / dec_blocks must be 0 .. 64");
    L3C_REQUIRE((c->rgb_baseline == 0 || c->rgb_baseline == 1) && (c->dec_skip == 0 || c->dec_skip == 1), "flags must be 0 or 1");
    L3C_REQUIRE(!c->rgb_baseline || c->C == 3, "RGB baselines predict RGB symbols: C must be 3");
    if (!compute) return L3C_OK;
    if (c->Cf != 64)
        return NET_FAIL(L3C_ERR_UNSUPPORTED, "unsupported config: Cf = %d, the network schedule needs Cf == 64 (the PixelShuffle tail has "
                        "a Winograd form only at 4 Cf = 256)", c->Cf);
    if (c->C > 8) return NET_FAIL(L3C_ERR_UNSUPPORTED, "unsupported config: C = %d > 8 (l3c_dec_head)", c->C);
    for (int s = 0; s < c->num_scales; ++s)
        if (kp_of(*c, s) > 160)
            return NET_FAIL(L3C_ERR_UNSUPPORTED, "unsupported config: Kp = %d > 160 at scale %d (l3c_conv_pw)", kp_of(*c, s), s);
    if (!c->rgb_baseline && !c->dec_skip) return NET_FAIL(L3C_ERR_UNSUPPORTED, "unsupported config: L3C needs dec_skip");
    return L3C_OK;
}

// ---- packed layout ---------------------------------------------------------------------------------------------------------

enum Kind { RAW, WINO, POLY, SHUF, PW, LEVELS };

struct Item {
    int kind;
    int param;               // index of the weight (RAW / WINO / POLY / SHUF / PW) or of the levels (LEVELS) in schema order
    int Cout, Cin;
    int64_t w_floats;        // weights as the checkpoint holds them (RAW: the floats copied)
    int64_t w_off, b_off;    // byte offsets inside the packed buffer
};

struct Layout {
    std::vector<Item> items;
    int64_t bytes = 0;
    int ms1 = -1, ms2 = -1, head0 = -1;
    int heads[L3C_NET_MAX_SCALES];
    int down[L3C_NET_MAX_SCALES], enc_body[L3C_NET_MAX_SCALES][2 * MAX_BLOCKS + 1], to_q[L3C_NET_MAX_SCALES], levels[L3C_NET_MAX_SCALES];
    int dec_head[L3C_NET_MAX_SCALES], dec_body[L3C_NET_MAX_SCALES][2 * MAX_BLOCKS + 1], up[L3C_NET_MAX_SCALES];
    int atrous[L3C_NET_MAX_SCALES][3], lin[L3C_NET_MAX_SCALES];
};

// Builds the layout of a SUPPORTED config (check_config(c, true) passed); the items follow schema order.
void build_layout(const l3c_net_config &c, Layout &L) {
    int pi = 0;   // running schema index: weight of the next conv
    auto add = [&](int kind, int cout, int cin, int64_t packed_floats, int64_t w_floats = 0) {
        Item it{kind, pi, cout, cin, w_floats, 0, 0};
        it.w_off = L.bytes;
        L.bytes += align_up(packed_floats * 4);
        it.b_off = L.bytes;
        L.bytes += align_up((int64_t)cout * 4);
        L.items.push_back(it);
        pi += 2;
        return (int)L.items.size() - 1;
    };
    auto wino = [&](int cout, int cin) { return add(WINO, cout, cin, l3c_conv_wino4_packed_words(cout, cin)); };
    auto body = [&](int *dst, int n) {
        for (int i = 0; i < 2 * n + 1; ++i) dst[i] = wino(c.Cf, c.Cf);
    };
    auto levels = [&]() {
        Item it{LEVELS, pi, 0, 0, c.L, L.bytes, 0};
        L.bytes += align_up((int64_t)c.L * 4);
        L.items.push_back(it);
        pi += 1;
        return (int)L.items.size() - 1;
    };
    const int Cf = c.Cf;
    if (!c.rgb_baseline) L.ms1 = add(RAW, 3, 3, 9, 9);
    else pi += 2;   // sub_rgb_mean: the baselines' forward (bicubic pyramid) is not in this library
    if (!c.rgb_baseline) {
        L.ms2 = add(RAW, 3, 3, 9, 9);
        L.head0 = add(RAW, Cf, 3, (int64_t)Cf * 27, (int64_t)Cf * 27);
        for (int s = 1; s < c.num_scales; ++s) L.heads[s] = wino(Cf, Cf);
    }
    for (int s = 0; s < c.num_scales; ++s) {
        if (!c.rgb_baseline) {
            L.levels[s] = levels();
            L.down[s] = add(POLY, Cf, Cf, l3c_conv_wino4_packed_words(Cf, 4 * Cf));
            body(L.enc_body[s], c.enc_blocks);
            L.to_q[s] = add(RAW, c.C, Cf, (int64_t)c.C * Cf, (int64_t)c.C * Cf);
            pi += 1;   // enc.q.levels: the same values registered twice (net.py:125-127); the quantiser reads enc.levels
        }
        L.dec_head[s] = add(RAW, Cf, c.C, (int64_t)Cf * c.C, (int64_t)Cf * c.C);
        body(L.dec_body[s], c.dec_blocks);
        L.up[s] = add(SHUF, 4 * Cf, Cf, l3c_conv_wino4_packed_words(4 * Cf, Cf));
    }
    for (int s = 0; s < c.num_scales; ++s) {
        for (int i = 0; i < 3; ++i) L.atrous[s][i] = wino(Cf, Cf);
        L.lin[s] = add(PW, kp_of(c, s), 3 * Cf, l3c_conv_pw_packed_words(kp_of(c, s), 3 * Cf));
    }
}

// ---- the schedule ----------------------------------------------------------------------------------------------------------

struct Run {
    const char *base;   // packed buffer
    const Layout *L;
    int B;
    l3c_stream_t st;
    const float *w(int i) const { return reinterpret_cast<const float *>(base + L->items[i].w_off); }
    const float *b(int i) const { return reinterpret_cast<const float *>(base + L->items[i].b_off); }
};

// one 3x3 stride-1 layer on l3c_conv_wino4, the descriptor of ops.conv
int conv3(const Run &r, int item, const float *in, int in_cstride, int H, int W, float *out, int out_cstride, int out_coff,
          int dilation, int epilogue, const float *residual, int res_cstride) {
    const Item &it = r.L->items[item];
    l3c_conv_desc d{};
    d.in = in;  d.in_cstride = in_cstride;  d.in_coff = 0;
    d.packed_w = r.w(item);  d.bias = r.b(item);
    d.residual = residual;  d.res_cstride = residual ? res_cstride : 0;  d.res_coff = 0;
    d.out = out;  d.out_cstride = out_cstride;  d.out_coff = out_coff;
    d.B = r.B;  d.Hin = H;  d.Win = W;  d.Cin = it.Cin;  d.Cout = it.Cout;
    d.KS = 3;  d.stride = 1;  d.dilation = dilation;  d.epilogue = epilogue;
    return l3c_conv_wino4(&d, r.st);
}

#define NET_TRY(x)                          \
    do {                                    \
        const int rc_ = (x);                \
        if (rc_ != L3C_OK) return rc_;      \
    } while (0)

// MultiscaleNetwork._body: n x ResBlock(conv-ReLU-conv, += input) + conv, + global skip.  Input in S, result in dst (may be T).
int body(const Run &r, const int *layers, int n, int Cf, int H, int W, const float *S, float *X0, float *X1, float *T, float *dst) {
    const float *x = S;
    float *y = X0;
    for (int i = 0; i < n; ++i) {
        NET_TRY(conv3(r, layers[2 * i], x, Cf, H, W, T, Cf, 0, 1, L3C_EPI_RELU, nullptr, 0));
        NET_TRY(conv3(r, layers[2 * i + 1], T, Cf, H, W, y, Cf, 0, 1, L3C_EPI_RESIDUAL, x, Cf));
        x = y;
        y = (y == X0) ? X1 : X0;
    }
    return conv3(r, layers[2 * n], x, Cf, H, W, dst, Cf, 0, 1, L3C_EPI_RESIDUAL, S, Cf);
}

// MultiscaleNetwork._decoder: dec_head (+ fuse) -> body -> 64 -> 256 conv + PixelShuffle(2).  bn_q at (H, W), F at (2H, 2W).
int decoder(const Run &r, const l3c_net_config &c, int s, const float *bn_q, const float *fuse, int H, int W, float *bufs, int64_t buf_stride,
            float *F) {
    const Layout &L = *r.L;
    float *S = bufs, *X0 = bufs + buf_stride, *X1 = bufs + 2 * buf_stride, *T = bufs + 3 * buf_stride;
    NET_TRY(l3c_dec_head(bn_q, r.w(L.dec_head[s]), r.b(L.dec_head[s]), fuse, r.B, (int64_t)H * W, c.C, c.Cf, S, r.st));
    NET_TRY(body(r, L.dec_body[s], c.dec_blocks, c.Cf, H, W, S, X0, X1, T, T));
    return conv3(r, L.up[s], T, c.Cf, H, W, F, c.Cf, 0, 1, L3C_EPI_PIXEL_SHUFFLE, nullptr, 0);
}

// MultiscaleNetwork._prob: three atrous 3x3 branches into channel slices of one 3 Cf buffer, then the 1x1 3 Cf -> Kp on l3c_conv_pw
int prob(const Run &r, const l3c_net_config &c, int s, const float *F, int H, int W, float *cat, float *P) {
    const Layout &L = *r.L;
    static const int dil[3] = {1, 2, 4};
    for (int i = 0; i < 3; ++i) NET_TRY(conv3(r, L.atrous[s][i], F, c.Cf, H, W, cat, 3 * c.Cf, i * c.Cf, dil[i], 0, nullptr, 0));
    const Item &it = L.items[L.lin[s]];
    l3c_conv_desc d{};
    d.in = cat;  d.in_cstride = 3 * c.Cf;  d.in_coff = 0;
    d.packed_w = r.w(L.lin[s]);  d.bias = r.b(L.lin[s]);
    d.residual = nullptr;  d.res_cstride = 0;  d.res_coff = 0;
    d.out = P;  d.out_cstride = it.Cout;  d.out_coff = 0;
    d.B = r.B;  d.Hin = H;  d.Win = W;  d.Cin = it.Cin;  d.Cout = it.Cout;
    d.KS = 1;  d.stride = 1;  d.dilation = 1;  d.epilogue = 0;
    return l3c_conv_pw(&d, r.st);
}

// ---- shapes, workspace plans -----------------------------------------------------------------------------------------------

// The image-size limits of the kernels the schedule runs, checked up front (l3c_conv_wino4: one image of the input below 2 GB, 32-bit
// offsets inside a tile row of the widest output -- the dilation-4 atrous branch into the 3 Cf buffer, the PixelShuffle tail).
int check_image(const l3c_net_config &c, int64_t B, int64_t H, int64_t W) {
    if (!(B > 0 && B < 65536 && H > 0 && W > 0)) return NET_FAIL(L3C_ERR_INVALID_ARG, "bad shape: B = %lld, H = %lld, W = %lld", (long long)B, (long long)H, (long long)W);
    if (H * W * c.Cf * 4 >= 0x7ffffff0ll)
        return NET_FAIL(L3C_ERR_UNSUPPORTED, "unsupported shape: %lld x %lld pixels per image, H * W * Cf * 4 must stay below 0x7ffffff0 "
                        "(32-bit addressing inside one image)", (long long)H, (long long)W);
    if (B * H * W >= (1ll << 31)) return NET_FAIL(L3C_ERR_UNSUPPORTED, "unsupported shape: B * H * W must stay below 2^31");
    if (80ll * (W + 256) * 3 * c.Cf * 4 >= 0x7ffffff0ll || 80ll * (W / 2 + 64) * c.Cf * 4 >= 0x7ffffff0ll)
        return NET_FAIL(L3C_ERR_UNSUPPORTED, "unsupported shape: W = %lld too wide for 32-bit offsets inside a tile row", (long long)W);
    return L3C_OK;
}

struct FwdPlan {            // the workspace of a forward: the cat region from offset 0, then the F_dec slots
    int64_t cat_bytes;
    int64_t fd_off[L3C_NET_MAX_SCALES];   // F_dec[s] slots, s >= 1; s == 0 only when P[0] cannot hold it (Kp_0 < Cf); -1: none
    int64_t bytes;
    int64_t enc_a, enc_body;              // encoder phase inside the cat region: input buffer, then 4 body buffers of enc_body bytes
};

FwdPlan fwd_plan(const l3c_net_config &c, int64_t B, int H, int W) {
    FwdPlan p{};
    const int64_t N0 = B * H * W, N1 = B * (H / 2) * (W / 2);
    p.enc_a = align_up(N0 * c.Cf * 4);
    p.enc_body = align_up(N1 * c.Cf * 4);
    p.cat_bytes = align_up(3 * N0 * c.Cf * 4);
    if (p.cat_bytes < p.enc_a + 4 * p.enc_body) p.cat_bytes = p.enc_a + 4 * p.enc_body;
    p.bytes = p.cat_bytes;
    for (int s = 0; s < L3C_NET_MAX_SCALES; ++s) p.fd_off[s] = -1;
    for (int s = 0; s < c.num_scales; ++s) {
        if (s == 0 && kp_of(c, 0) >= c.Cf) continue;   // F_dec[0] lives in P[0] until the classifier's last layer overwrites it
        p.fd_off[s] = p.bytes;
        p.bytes += align_up(B * (int64_t)(H >> s) * (W >> s) * c.Cf * 4);
    }
    return p;
}

struct GetPPlan {
    int64_t region, body, f_off, bytes;
};

GetPPlan getp_plan(const l3c_net_config &c, int net, int64_t B, int h, int w) {
    GetPPlan p{};
    const int64_t Nin = B * h * w, Nout = 4 * Nin;
    p.body = align_up(Nin * c.Cf * 4);
    p.region = align_up(3 * Nout * c.Cf * 4);
    if (p.region < 4 * p.body) p.region = 4 * p.body;
    p.f_off = -1;
    p.bytes = p.region;
    if (kp_of(c, net) < c.Cf) {
        p.f_off = p.bytes;
        p.bytes += align_up(Nout * c.Cf * 4);
    }
    return p;
}

// l3c_net_get_p_rows: the decoder stage on half-resolution rows [a0 / 2, a1 / 2), the classifier on rows [c0, c1) of its features
struct RowsPlan {
    int64_t a0, a1;
    bool cut;                                   // the decoder rows are not the whole frame: its inputs are row slices
    int64_t body, bn, fuse, F, Fc, bytes;       // offsets (-1: not needed); `body`: one of the four decoder buffers at offset 0
};

RowsPlan rows_plan(const l3c_net_config &c, int64_t B, int h, int w, int c0, int c1) {
    RowsPlan p{};
    l3c_plan::region_decoder_rows(2ll * h, c0, c1, l3c_plan::region_apron_rows(c.dec_blocks), &p.a0, &p.a1);
    p.cut = p.a0 != 0 || p.a1 != 2ll * h;
    const int64_t ha = (p.a1 - p.a0) / 2, W = 2ll * w;
    p.body = align_up(B * ha * w * c.Cf * 4);
    int64_t at = align_up(3 * B * (c1 - c0) * W * c.Cf * 4);
    if (at < 4 * p.body) at = 4 * p.body;
    auto take = [&](bool needed, int64_t n) {
        if (!needed) return (int64_t)-1;
        const int64_t o = at;
        at += align_up(n);
        return o;
    };
    p.bn = take(p.cut, B * c.C * ha * w * 4);
    p.fuse = take(p.cut && B > 1, B * ha * w * c.Cf * 4);
    p.F = take(true, B * (p.a1 - p.a0) * W * c.Cf * 4);
    p.Fc = take(B > 1 && (c0 != p.a0 || c1 != p.a1), B * (c1 - c0) * W * c.Cf * 4);
    p.bytes = at;
    return p;
}

// what both entries of the windowed step ask of the config and the window
int check_rows(const l3c_net_config *cfg, int net, int64_t B, int h, int w, int c0, int c1) {
    NET_TRY(check_config(cfg, true));
    if (cfg->rgb_baseline) return NET_FAIL(L3C_ERR_UNSUPPORTED, "l3c_net_get_p_rows: the RGB baselines are not windowed");
    L3C_REQUIRE(net == 0, "l3c_net_get_p_rows: only scale 0 is windowed (net must be 0)");
    L3C_REQUIRE(h > 0 && w > 0 && h < 32768 && w < 32768, "bad shape");
    NET_TRY(check_image(*cfg, B, 2ll * h, 2ll * w));
    if (!(0 <= c0 && c0 < c1 && c1 <= 2 * h && c0 % 2 == 0 && c1 % 2 == 0))
        return NET_FAIL(L3C_ERR_INVALID_ARG, "conv rows [%d, %d) must be even rows inside the %d frame rows", c0, c1, 2 * h);
    if (c0 % l3c_plan::REGION_GRANULE || (c1 % l3c_plan::REGION_GRANULE && c1 != 2 * h))
        return NET_FAIL(L3C_ERR_INVALID_ARG, "conv rows [%d, %d): c0 must be a multiple of 64, c1 a multiple of 64 or the frame's end %d", c0, c1, 2 * h);
    return L3C_OK;
}

// rows [r0, r0 + rows) of `planes` planes of plane_rows rows of row_bytes bytes each -> dst, packed
int copy_rows(float *dst, const float *src, int64_t planes, int64_t plane_rows, int64_t r0, int64_t rows, int64_t row_bytes, hipStream_t st) {
    return l3c::check_hip(hipMemcpy2DAsync(dst, (size_t)(rows * row_bytes), reinterpret_cast<const char *>(src) + r0 * row_bytes,
                                           (size_t)(plane_rows * row_bytes), (size_t)(rows * row_bytes), (size_t)planes, hipMemcpyDeviceToDevice, st),
                          "hipMemcpy2DAsync");
}

}  // namespace

extern "C" {

int l3c_net_param_count(const l3c_net_config *cfg) {
    NET_TRY(check_config(cfg, false));
    return (int)schema(*cfg).size();
}

int l3c_net_param(const l3c_net_config *cfg, int i, char *name_host, int name_cap, int *ndim_host, int64_t *shape_host) {
    NET_TRY(check_config(cfg, false));
    L3C_REQUIRE(name_host && name_cap > 0 && ndim_host && shape_host, "null pointer");
    const std::vector<Param> v = schema(*cfg);
    L3C_REQUIRE(i >= 0 && i < (int)v.size(), "parameter index out of range");
    const Param &p = v[i];
    L3C_REQUIRE((int)p.name.size() < name_cap, "name_cap too small");
    memcpy(name_host, p.name.c_str(), p.name.size() + 1);
    *ndim_host = p.ndim;
    for (int k = 0; k < p.ndim; ++k) shape_host[k] = p.shape[k];
    return L3C_OK;
}

int64_t l3c_net_packed_bytes(const l3c_net_config *cfg) {
    NET_TRY(check_config(cfg, true));
    Layout L;
    build_layout(*cfg, L);
    return L.bytes;
}

int64_t l3c_net_pack_workspace_bytes(const l3c_net_config *cfg) {
    NET_TRY(check_config(cfg, true));
    return align_up((int64_t)36 * cfg->Cf * cfg->Cf * 4);   // the largest rearranged kernel: Cf x 4 Cf x 3 x 3 (= 4 Cf x Cf x 3 x 3)
}

int l3c_net_pack(const l3c_net_config *cfg, const float *const *params_host, void *packed, int64_t packed_bytes, void *workspace,
                 int64_t workspace_bytes, l3c_stream_t stream) {
    NET_TRY(check_config(cfg, true));
    L3C_REQUIRE(params_host && packed && workspace, "null pointer");
    L3C_REQUIRE(aligned16(packed) && aligned16(workspace), "packed buffer and workspace must be 16-byte aligned");
    const std::vector<Param> v = schema(*cfg);
    for (size_t i = 0; i < v.size(); ++i)
        if (!params_host[i]) return NET_FAIL(L3C_ERR_INVALID_ARG, "null pointer: parameter %d (%s)", (int)i, v[i].name.c_str());
    Layout L;
    build_layout(*cfg, L);
    if (packed_bytes != L.bytes)
        return NET_FAIL(L3C_ERR_INVALID_ARG, "packed_bytes %lld != l3c_net_packed_bytes %lld", (long long)packed_bytes, (long long)L.bytes);
    const int64_t need = l3c_net_pack_workspace_bytes(cfg);
    if (workspace_bytes < need)
        return NET_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)workspace_bytes, (long long)need);
    const hipStream_t st = l3c::as_stream(stream);
    char *base = static_cast<char *>(packed);
    float *ws = static_cast<float *>(workspace);
    for (const Item &it : L.items) {
        const float *w = params_host[it.param];
        float *dst = reinterpret_cast<float *>(base + it.w_off);
        switch (it.kind) {
        case LEVELS:
            NET_TRY(l3c::check_hip(hipMemcpyAsync(dst, w, (size_t)it.w_floats * 4, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync"));
            continue;
        case RAW:
            NET_TRY(l3c::check_hip(hipMemcpyAsync(dst, w, (size_t)it.w_floats * 4, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync"));
            break;
        case WINO:
            NET_TRY(l3c_conv_wino4_pack_weights(w, it.Cout, it.Cin, dst, stream));
            break;
        case POLY:
            hipLaunchKernelGGL(polyphase_concat_kernel, dim3(grid_for((int64_t)it.Cout * 36 * it.Cin)), dim3(256), 0, st, w, it.Cout,
                               it.Cin, ws);
            NET_TRY(l3c::check_launch("polyphase_concat_kernel"));
            NET_TRY(l3c_conv_wino4_pack_weights(ws, it.Cout, 4 * it.Cin, dst, stream));
            break;
        case SHUF:
            hipLaunchKernelGGL(subpixel_rows_kernel, dim3(grid_for((int64_t)it.Cout * it.Cin * 9)), dim3(256), 0, st, w, it.Cout,
                               it.Cin * 9, ws);
            NET_TRY(l3c::check_launch("subpixel_rows_kernel"));
            NET_TRY(l3c_conv_wino4_pack_weights(ws, it.Cout, it.Cin, dst, stream));
            break;
        case PW:
            NET_TRY(l3c_conv_pw_pack_weights(w, it.Cout, it.Cin, dst, stream));
            break;
        }
        NET_TRY(l3c::check_hip(hipMemcpyAsync(base + it.b_off, params_host[it.param + 1], (size_t)it.Cout * 4, hipMemcpyDeviceToDevice, st),
                               "hipMemcpyAsync"));
    }
    return L3C_OK;
}

int64_t l3c_net_forward_workspace_bytes(const l3c_net_config *cfg, int64_t B, int H, int W) {
    NET_TRY(check_config(cfg, true));
    NET_TRY(check_image(*cfg, B, H, W));
    return fwd_plan(*cfg, B, H, W).bytes;
}

int l3c_net_forward(const l3c_net_forward_desc *d, l3c_stream_t stream) {
    L3C_REQUIRE(d, "null descriptor");
    NET_TRY(check_config(d->cfg_host, true));
    const l3c_net_config &c = *d->cfg_host;
    if (c.rgb_baseline)
        return NET_FAIL(L3C_ERR_UNSUPPORTED, "l3c_net_forward of an RGB baseline: its bicubic pyramid is driven by host-side resampling "
                        "tables (use l3c_net_get_p for its decoders)");
    const int S = c.num_scales;
    L3C_REQUIRE(d->packed && d->img, "null pointer");
    for (int s = 0; s <= S; ++s) L3C_REQUIRE(d->sym[s] && (s == 0 || d->bn_q[s]) && (s == S || d->P[s]), "null pointer: outputs");
    bool ok = aligned16(d->packed) && aligned16(d->img) && aligned16(d->workspace);
    for (int s = 0; s <= S; ++s) {
        ok = ok && aligned16(d->sym[s]) && aligned16(d->bn_q[s]);
        if (s < S) ok = ok && aligned16(d->P[s]) && aligned16(d->F_enc[s]) && aligned16(d->F_dec[s]);
    }
    L3C_REQUIRE(ok, "every pointer must be 16-byte aligned");
    NET_TRY(check_image(c, d->B, d->H, d->W));
    if (d->H % (1 << S) || d->W % (1 << S))
        return NET_FAIL(L3C_ERR_UNSUPPORTED, "unsupported shape: %d x %d, H and W must be multiples of 2^num_scales = %d", d->H, d->W, 1 << S);
    Layout L;
    build_layout(c, L);
    if (d->packed_bytes != L.bytes)
        return NET_FAIL(L3C_ERR_INVALID_ARG, "packed_bytes %lld != l3c_net_packed_bytes %lld (packed for another config?)",
                        (long long)d->packed_bytes, (long long)L.bytes);
    const FwdPlan p = fwd_plan(c, d->B, d->H, d->W);
    L3C_REQUIRE(d->workspace || p.bytes == 0, "null pointer: workspace");
    if (d->workspace_bytes < p.bytes)
        return NET_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)d->workspace_bytes, (long long)p.bytes);

    // ---- everything checked: enqueue.  Order of MultiscaleNetwork.forward: image symbols, RGB head, encoders fine -> coarse,
    // decoders coarse -> fine, classifiers fine -> coarse.
    const Run r{static_cast<const char *>(d->packed), &L, (int)d->B, stream};
    const int B = (int)d->B, Cf = c.Cf;
    char *ws = static_cast<char *>(d->workspace);
    const int64_t n_img = (int64_t)B * 3 * d->H * d->W;
    hipLaunchKernelGGL(image_symbols_kernel, dim3(grid_for(n_img)), dim3(256), 0, l3c::as_stream(stream), d->img, n_img, d->sym[0]);
    NET_TRY(l3c::check_launch("image_symbols_kernel"));

    // encoders (inside the cat region, which is free until the classifiers): A = the scale's input, then S, X0, X1, T at half size
    float *A = reinterpret_cast<float *>(ws);
    float *eb[4];
    for (int i = 0; i < 4; ++i) eb[i] = reinterpret_cast<float *>(ws + p.enc_a + i * p.enc_body);
    NET_TRY(l3c_rgb_head(d->img, r.w(L.ms1), r.b(L.ms1), r.w(L.ms2), r.b(L.ms2), r.w(L.head0), r.b(L.head0), B, d->H, d->W, Cf, A,
                         nullptr, stream));
    const float *F_prev = nullptr;
    for (int s = 0; s < S; ++s) {
        const int H = d->H >> s, W = d->W >> s;
        if (s) NET_TRY(conv3(r, L.heads[s], F_prev, Cf, H, W, A, Cf, 0, 1, 0, nullptr, 0));
        l3c_conv_desc dd{};
        dd.in = A;  dd.in_cstride = Cf;  dd.in_coff = 0;
        dd.packed_w = r.w(L.down[s]);  dd.bias = r.b(L.down[s]);
        dd.residual = nullptr;  dd.res_cstride = 0;  dd.res_coff = 0;
        dd.out = eb[0];  dd.out_cstride = Cf;  dd.out_coff = 0;
        dd.B = B;  dd.Hin = H;  dd.Win = W;  dd.Cin = Cf;  dd.Cout = Cf;
        dd.KS = 5;  dd.stride = 2;  dd.dilation = 1;  dd.epilogue = 0;
        NET_TRY(l3c_conv_wino4_stride2(&dd, stream));
        float *F = d->F_enc[s] ? d->F_enc[s] : eb[3];
        NET_TRY(body(r, L.enc_body[s], c.enc_blocks, Cf, H / 2, W / 2, eb[0], eb[1], eb[2], eb[3], F));
        NET_TRY(l3c_to_q_quantize(F, r.w(L.to_q[s]), r.b(L.to_q[s]), r.w(L.levels[s]), B, (int64_t)(H / 2) * (W / 2), Cf, c.C, c.L,
                                  d->sym[s + 1], d->bn_q[s + 1], nullptr, stream));
        F_prev = F;
    }
    // decoders: body buffers in the cat region; F_dec[s] in the caller's buffer, its slot, or (s == 0) the memory of P[0]
    float *fd[L3C_NET_MAX_SCALES];
    for (int s = 0; s < S; ++s)
        fd[s] = d->F_dec[s] ? d->F_dec[s] : p.fd_off[s] >= 0 ? reinterpret_cast<float *>(ws + p.fd_off[s]) : d->P[0];
    for (int s = S - 1; s >= 0; --s) {
        const int H = d->H >> (s + 1), W = d->W >> (s + 1);
        NET_TRY(decoder(r, c, s, d->bn_q[s + 1], s == S - 1 ? nullptr : fd[s + 1], H, W, A, (int64_t)B * H * W * Cf, fd[s]));
    }
    for (int s = 0; s < S; ++s) NET_TRY(prob(r, c, s, fd[s], d->H >> s, d->W >> s, A, d->P[s]));
    return L3C_OK;
}

int64_t l3c_net_get_p_workspace_bytes(const l3c_net_config *cfg, int64_t B, int h, int w) {
    NET_TRY(check_config(cfg, true));
    NET_TRY(check_image(*cfg, B, 2ll * h, 2ll * w));
    int64_t m = 0;
    for (int s = 0; s < cfg->num_scales; ++s) {
        const int64_t b = getp_plan(*cfg, s, B, h, w).bytes;
        m = b > m ? b : m;
    }
    return m;
}

int l3c_net_get_p(const l3c_net_get_p_desc *d, l3c_stream_t stream) {
    L3C_REQUIRE(d, "null descriptor");
    NET_TRY(check_config(d->cfg_host, true));
    const l3c_net_config &c = *d->cfg_host;
    L3C_REQUIRE(d->net >= 0 && d->net < c.num_scales, "net out of range (0 .. num_scales - 1)");
    L3C_REQUIRE(d->packed && d->bn_q && d->P, "null pointer");
    L3C_REQUIRE(aligned16(d->packed) && aligned16(d->bn_q) && aligned16(d->fuse) && aligned16(d->P) && aligned16(d->F) &&
                aligned16(d->workspace), "every pointer must be 16-byte aligned");
    L3C_REQUIRE(c.dec_skip || !d->fuse, "dec_skip == 0: the decoder takes no fused features (fuse must be NULL)");
    NET_TRY(check_image(c, d->B, 2ll * d->h, 2ll * d->w));
    Layout L;
    build_layout(c, L);
    if (d->packed_bytes != L.bytes)
        return NET_FAIL(L3C_ERR_INVALID_ARG, "packed_bytes %lld != l3c_net_packed_bytes %lld (packed for another config?)",
                        (long long)d->packed_bytes, (long long)L.bytes);
    const GetPPlan p = getp_plan(c, d->net, d->B, d->h, d->w);
    L3C_REQUIRE(d->workspace || p.bytes == 0, "null pointer: workspace");
    if (d->workspace_bytes < p.bytes)
        return NET_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)d->workspace_bytes, (long long)p.bytes);

    const Run r{static_cast<const char *>(d->packed), &L, (int)d->B, stream};
    char *ws = static_cast<char *>(d->workspace);
    float *region = reinterpret_cast<float *>(ws);
    float *F = d->F ? d->F : p.f_off >= 0 ? reinterpret_cast<float *>(ws + p.f_off) : d->P;   // F without a caller buffer: in P's memory
    NET_TRY(decoder(r, c, d->net, d->bn_q, d->fuse, d->h, d->w, region, p.body / 4, F));
    return prob(r, c, d->net, F, 2 * d->h, 2 * d->w, region, d->P);
}

int l3c_net_halo_rows(int dec_blocks) {
    L3C_REQUIRE(dec_blocks >= 0 && dec_blocks <= MAX_BLOCKS, "dec_blocks must be 0 .. 64");
    return (int)l3c_plan::region_halo_rows(dec_blocks);
}

int l3c_net_apron_rows(int dec_blocks) {
    L3C_REQUIRE(dec_blocks >= 0 && dec_blocks <= MAX_BLOCKS, "dec_blocks must be 0 .. 64");
    return (int)l3c_plan::region_apron_rows(dec_blocks);
}

int64_t l3c_net_get_p_rows_workspace_bytes(const l3c_net_config *cfg, int64_t B, int h, int w, int c0, int c1) {
    NET_TRY(check_rows(cfg, 0, B, h, w, c0, c1));
    return rows_plan(*cfg, B, h, w, c0, c1).bytes;
}

int l3c_net_get_p_rows(const l3c_net_get_p_rows_desc *d, l3c_stream_t stream) {
    L3C_REQUIRE(d, "null descriptor");
    NET_TRY(check_rows(d->cfg_host, d->net, d->B, d->h, d->w, d->c0, d->c1));
    const l3c_net_config &c = *d->cfg_host;
    L3C_REQUIRE(d->packed && d->bn_q && d->P && d->workspace, "null pointer");
    L3C_REQUIRE(d->fuse, "null pointer: fuse (the windowed step needs the coarser decoder's features)");
    L3C_REQUIRE(aligned16(d->packed) && aligned16(d->bn_q) && aligned16(d->fuse) && aligned16(d->P) && aligned16(d->workspace),
                "every pointer must be 16-byte aligned");
    Layout L;
    build_layout(c, L);
    if (d->packed_bytes != L.bytes)
        return NET_FAIL(L3C_ERR_INVALID_ARG, "packed_bytes %lld != l3c_net_packed_bytes %lld (packed for another config?)",
                        (long long)d->packed_bytes, (long long)L.bytes);
    const RowsPlan p = rows_plan(c, d->B, d->h, d->w, d->c0, d->c1);
    if (d->workspace_bytes < p.bytes)
        return NET_FAIL(L3C_ERR_INVALID_ARG, "workspace_bytes too small: %lld < %lld", (long long)d->workspace_bytes, (long long)p.bytes);

    // ---- everything checked: enqueue
    const Run r{static_cast<const char *>(d->packed), &L, (int)d->B, stream};
    const hipStream_t st = l3c::as_stream(stream);
    char *ws = static_cast<char *>(d->workspace);
    const int64_t B = d->B, h = d->h, w = d->w, W = 2 * w, ha = (p.a1 - p.a0) / 2, rows = d->c1 - d->c0;
    const float *bn = d->bn_q, *fuse = d->fuse;
    if (p.cut) {
        float *g = reinterpret_cast<float *>(ws + p.bn);
        NET_TRY(copy_rows(g, d->bn_q, B * c.C, h, p.a0 / 2, ha, w * 4, st));
        bn = g;
        fuse = d->fuse + (p.a0 / 2) * w * c.Cf;              // one image: the rows are contiguous where they lie
        if (p.fuse >= 0) {
            float *f = reinterpret_cast<float *>(ws + p.fuse);
            NET_TRY(copy_rows(f, d->fuse, B, h, p.a0 / 2, ha, w * c.Cf * 4, st));
            fuse = f;
        }
    }
    float *F = reinterpret_cast<float *>(ws + p.F);
    NET_TRY(decoder(r, c, 0, bn, fuse, (int)ha, (int)w, reinterpret_cast<float *>(ws), p.body / 4, F));
    const float *Fw = F + (d->c0 - p.a0) * W * c.Cf;         // (likewise)
    if (p.Fc >= 0) {
        float *f = reinterpret_cast<float *>(ws + p.Fc);
        NET_TRY(copy_rows(f, F, B, p.a1 - p.a0, d->c0 - p.a0, rows, W * c.Cf * 4, st));
        Fw = f;
    }
    return prob(r, c, 0, Fw, (int)rows, (int)W, reinterpret_cast<float *>(ws), d->P);
}
}
