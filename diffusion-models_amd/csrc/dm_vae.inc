// The first-stage models of the latent-diffusion path (textually included at the end of dm_api.hip).
// Decode replaces VQModel.decode (LD/models/autoencoder.py:113-116) = post_quant_conv (1x1) -> Decoder.forward
// (LD/modules/diffusionmodules/model.py:552-585) and runs once per sample() call.  Encode replaces VQModel.encode
// (autoencoder.py:102-106) = Encoder.forward (model.py:451-476) -> quant_conv (1x1) -> VectorQuantizer, or the posterior
// of AutoencoderKL.  The quantizer is taming-transformers' VectorQuantizer2 (taming/modules/vqvae/quantize.py, a pip
// dependency that is not in the reference tree): nearest codebook row under d = |z|^2 + |e|^2 - 2 z.e, output z + (e - z).
//
// Each network is one list of nodes in execution order (decoder_nodes / encoder_nodes) that the expected-parameter list,
// the weight upload and the forward walk all loop over, as unet_graph.inc does for the U-Net.
namespace dm {

struct VaeRes {
    int cin = 0, cout = 0;
    float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr;
    ConvLayer c1, c2, nin;
    bool has_nin = false;
};
struct VaeAttn {
    int c = 0;
    float *nw = nullptr, *nb = nullptr;
    ConvLayer q, k, v, proj;
};

enum VaeKind { VAE_RES, VAE_ATTN, VAE_NORM, VAE_CONV };  // VAE_NORM: norm_out + swish; VAE_CONV: every plain convolution

struct VaeNode {
    VaeKind kind;
    std::string prefix;  // parameter-name prefix
    int cin, cout;
    int level;  // resolution level of the node's output, the reference's i_level: resolution >> level
    // VAE_CONV: k x k taps; `up`: nearest x2 in front; in_nchw / out_nchw: the network's input / output tensor; every
    // convolution of the networks has a bias (dm_op_vae_conv may leave it out)
    int k = 1, stride = 1, pad = 0, pad_hi = 0;
    bool up = false, in_nchw = false, out_nchw = false, bias = true;
    // the layer, by kind
    VaeRes res;
    VaeAttn attn;
    float *nw = nullptr, *nb = nullptr;
    ConvLayer conv;
};
using VaeTrunk = std::vector<VaeNode>;

static VaeNode& add_node(VaeTrunk& T, VaeKind kind, const std::string& prefix, int cin, int cout, int level) {
    T.push_back(VaeNode{kind, prefix, cin, cout, level});
    return T.back();
}
// a k x k convolution of stride 1 that keeps the size; the caller changes what differs
static VaeNode& add_conv(VaeTrunk& T, const std::string& prefix, int cin, int cout, int k, int level) {
    VaeNode& N = add_node(T, VAE_CONV, prefix, cin, cout, level);
    N.k = k;
    N.pad = k / 2;
    return N;
}
// mid.block_1 -> mid.attn_1 -> mid.block_2 (model.py:398-407 / :520-529)
static void add_mid(VaeTrunk& T, const std::string& p, int c, int level) {
    add_node(T, VAE_RES, p + ".block_1", c, c, level);
    add_node(T, VAE_ATTN, p + ".attn_1", c, c, level);
    add_node(T, VAE_RES, p + ".block_2", c, c, level);
}
static bool attn_at(const int32_t* attn_resolutions, int n, int curr_res) {
    bool attn = false;
    for (int a = 0; a < n; ++a) attn = attn || attn_resolutions[a] == curr_res;
    return attn;
}

// post_quant_conv -> Decoder (model.py:476-585)
static VaeTrunk decoder_nodes(const dm_decoder_cfg& cfg) {
    VaeTrunk T;
    int lvl = cfg.n_levels - 1;
    int block_in = cfg.ch * cfg.ch_mult[lvl];
    int curr_res = cfg.resolution >> lvl;
    add_conv(T, "post_quant_conv", cfg.embed_dim, cfg.z_channels, 1, lvl).in_nchw = true;
    add_conv(T, "decoder.conv_in", cfg.z_channels, block_in, 3, lvl);
    add_mid(T, "decoder.mid", block_in, lvl);
    for (; lvl >= 0; --lvl) {
        const int block_out = cfg.ch * cfg.ch_mult[lvl];
        const bool attn = attn_at(cfg.attn_resolutions, cfg.n_attn_res, curr_res);
        const std::string p = "decoder.up." + std::to_string(lvl);
        for (int b = 0; b < cfg.num_res_blocks + 1; ++b) {
            add_node(T, VAE_RES, p + ".block." + std::to_string(b), block_in, block_out, lvl);
            block_in = block_out;
            if (attn) add_node(T, VAE_ATTN, p + ".attn." + std::to_string(b), block_in, block_in, lvl);
        }
        if (lvl != 0) {
            add_conv(T, p + ".upsample.conv", block_in, block_in, 3, lvl - 1).up = true;
            curr_res *= 2;
        }
    }
    add_node(T, VAE_NORM, "decoder.norm_out", block_in, block_in, 0);
    add_conv(T, "decoder.conv_out", block_in, cfg.out_ch, 3, 0).out_nchw = true;
    return T;
}

// Encoder (model.py:368-476) -> quant_conv
static VaeTrunk encoder_nodes(const dm_encoder_cfg& cfg) {
    VaeTrunk T;
    add_conv(T, "encoder.conv_in", cfg.in_channels, cfg.ch, 3, 0).in_nchw = true;
    int curr_res = cfg.resolution, block_in = cfg.ch;
    const int top = cfg.n_levels - 1;
    for (int lvl = 0; lvl <= top; ++lvl) {
        block_in = cfg.ch * (lvl == 0 ? 1 : cfg.ch_mult[lvl - 1]);
        const int block_out = cfg.ch * cfg.ch_mult[lvl];
        const bool attn = attn_at(cfg.attn_resolutions, cfg.n_attn_res, curr_res);
        const std::string p = "encoder.down." + std::to_string(lvl);
        for (int b = 0; b < cfg.num_res_blocks; ++b) {
            add_node(T, VAE_RES, p + ".block." + std::to_string(b), block_in, block_out, lvl);
            block_in = block_out;
            if (attn) add_node(T, VAE_ATTN, p + ".attn." + std::to_string(b), block_in, block_in, lvl);
        }
        if (lvl != top) {  // Downsample: pad (0,1,0,1) + conv3x3 stride 2 (model.py:89-93)
            VaeNode& D = add_conv(T, p + ".downsample.conv", block_in, block_in, 3, lvl + 1);
            D.stride = 2;
            D.pad = 0;
            D.pad_hi = 1;
            curr_res /= 2;
        }
    }
    add_mid(T, "encoder.mid", block_in, top);
    add_node(T, VAE_NORM, "encoder.norm_out", block_in, block_in, top);
    const int zc = cfg.double_z ? 2 * cfg.z_channels : cfg.z_channels;
    add_conv(T, "encoder.conv_out", block_in, zc, 3, top);
    const int qc = cfg.n_embed == 0 ? 2 * cfg.embed_dim : cfg.embed_dim;  // LD/models/autoencoder.py:356 / :40
    add_conv(T, "quant_conv", zc, qc, 1, top);
    return T;
}

// The one handle behind dm_decoder and dm_encoder
struct VaeHandle {
    struct {
        int n_levels = 0, embed_dim = 0;
        int n_embed = 0;  // rows of the codebook: an encoder that quantises
    } cfg;  // what outlives create of dm_decoder_cfg / dm_encoder_cfg
    int device = 0;
    dm_unet holder;   // parameter table, device buffers and workspace management are shared code
    bool finalized = false;
    VaeTrunk trunk;
    float *codebook = nullptr, *code_sq = nullptr;
    float* bad_index = nullptr;  // one int: raised by embed_code_kernel
    bool kl() const { return cfg.n_embed == 0; }  // AutoencoderKL: quant_conv yields 2 * embed_dim moments, no codebook
    virtual ~VaeHandle() = default;
};

}  // namespace dm

struct dm_decoder : dm::VaeHandle {};
struct dm_encoder : dm::VaeHandle {};

namespace dm {

static void vexpect_res(dm_unet* u, const std::string& p, int cin, int cout) {
    expect(u, p + ".norm1.weight", {cin});
    expect(u, p + ".norm1.bias", {cin});
    expect(u, p + ".conv1.weight", {cout, cin, 3, 3});
    expect(u, p + ".conv1.bias", {cout});
    expect(u, p + ".norm2.weight", {cout});
    expect(u, p + ".norm2.bias", {cout});
    expect(u, p + ".conv2.weight", {cout, cout, 3, 3});
    expect(u, p + ".conv2.bias", {cout});
    if (cin != cout) {
        expect(u, p + ".nin_shortcut.weight", {cout, cin, 1, 1});
        expect(u, p + ".nin_shortcut.bias", {cout});
    }
}
static void vexpect_attn(dm_unet* u, const std::string& p, int c) {
    expect(u, p + ".norm.weight", {c});
    expect(u, p + ".norm.bias", {c});
    for (const char* n : {"q", "k", "v", "proj_out"}) {
        expect(u, p + "." + n + ".weight", {c, c, 1, 1});
        expect(u, p + "." + n + ".bias", {c});
    }
}
static void expect_node(dm_unet* u, const VaeNode& N) {
    switch (N.kind) {
    case VAE_RES: vexpect_res(u, N.prefix, N.cin, N.cout); break;
    case VAE_ATTN: vexpect_attn(u, N.prefix, N.cin); break;
    case VAE_NORM:
        expect(u, N.prefix + ".weight", {N.cin});
        expect(u, N.prefix + ".bias", {N.cin});
        break;
    case VAE_CONV:
        expect(u, N.prefix + ".weight", {N.cout, N.cin, N.k, N.k});
        if (N.bias) expect(u, N.prefix + ".bias", {N.cout});
        break;
    }
}

static int vconv(dm_unet* u, ConvLayer& L, const std::string& p, int cout, int cin, int k, int pad, bool up) {
    return make_conv(u, L, p + ".weight", p + ".bias", cout, cin, 0, k, k, 1, pad, up);
}
static int vbuild_res(dm_unet* u, VaeRes& R, const std::string& p, int cin, int cout) {
    R.cin = cin;
    R.cout = cout;
    R.has_nin = cin != cout;
    if (up1(u, p + ".norm1.weight", &R.n1w) || up1(u, p + ".norm1.bias", &R.n1b) ||
        up1(u, p + ".norm2.weight", &R.n2w) || up1(u, p + ".norm2.bias", &R.n2b))
        return 1;
    if (vconv(u, R.c1, p + ".conv1", cout, cin, 3, 1, false) || vconv(u, R.c2, p + ".conv2", cout, cout, 3, 1, false))
        return 1;
    if (R.has_nin && vconv(u, R.nin, p + ".nin_shortcut", cout, cin, 1, 0, false)) return 1;
    return 0;
}
static int vbuild_attn(dm_unet* u, VaeAttn& A, const std::string& p, int c) {
    A.c = c;
    if (up1(u, p + ".norm.weight", &A.nw) || up1(u, p + ".norm.bias", &A.nb)) return 1;
    return vconv(u, A.q, p + ".q", c, c, 1, 0, false) || vconv(u, A.k, p + ".k", c, c, 1, 0, false) ||
           vconv(u, A.v, p + ".v", c, c, 1, 0, false) || vconv(u, A.proj, p + ".proj_out", c, c, 1, 0, false);
}
static int build_node(dm_unet* u, VaeNode& N) {
    switch (N.kind) {
    case VAE_RES: return vbuild_res(u, N.res, N.prefix, N.cin, N.cout);
    case VAE_ATTN: return vbuild_attn(u, N.attn, N.prefix, N.cin);
    case VAE_NORM: return up1(u, N.prefix + ".weight", &N.nw) || up1(u, N.prefix + ".bias", &N.nb);
    case VAE_CONV:
        return make_conv(u, N.conv, N.prefix + ".weight", N.bias ? N.prefix + ".bias" : "", N.cout, N.cin, 0, N.k, N.k, N.stride,
                         N.pad, N.up, N.pad_hi);
    }
    return 1;
}

// The one place that picks the attention kernel (vrun_attn and dm_op_vae_attention): the MFMA kernel where it applies,
// else one row per wavefront; force_rows runs the row kernel at any shape it can take.
static int launch_vae_attention(const float* q, const float* k, const float* v, float* out, int B, int n, int C,
                                bool force_rows, hipStream_t s) {
    DM_REQUIRE(B > 0 && n > 0 && C > 0, "VAE attention: empty input");
    DM_REQUIRE(B <= 65535, "VAE attention: the batch is the grid's y dimension");
    if (!force_rows && vae_attn_mfma_ok(n, C)) return launch_vae_attn_mfma(q, k, v, out, B, n, C, s);
    return launch_attention_rows(q, k, v, out, B, n, C, s);
}

// ResnetBlock.forward with temb=None (model.py:138-158)
static int vrun_res(Ctx& c, const VaeRes& R, const float* x, int H, int W, float* stats, float** out) {
    const size_t pix = (size_t)c.B * H * W;
    float* a = c.A->alloc(pix * R.cin);
    float* h1 = c.A->alloc(pix * R.cout);
    float* a2 = c.A->alloc(pix * R.cout);
    float* h2 = c.A->alloc(pix * R.cout);
    if (!c.dry() && launch_group_norm(x, R.n1w, R.n1b, a, stats, c.B, H * W, R.cin, 32, 1e-6f, 1, c.s)) return 1;
    if (run_conv(c, R.c1, a, nullptr, H, W, h1, 0, nullptr, nullptr, nullptr)) return 1;
    if (!c.dry() && launch_group_norm(h1, R.n2w, R.n2b, a2, stats, c.B, H * W, R.cout, 32, 1e-6f, 1, c.s)) return 1;
    if (!R.has_nin) {
        if (run_conv(c, R.c2, a2, nullptr, H, W, h2, EPI_RESIDUAL, nullptr, nullptr, x)) return 1;
        *out = h2;
        return 0;
    }
    if (run_conv(c, R.c2, a2, nullptr, H, W, h2, 0, nullptr, nullptr, nullptr)) return 1;
    float* o = c.A->alloc(pix * R.cout);
    if (run_conv(c, R.nin, x, nullptr, H, W, o, EPI_RESIDUAL, nullptr, nullptr, h2)) return 1;
    *out = o;
    return 0;
}

// AttnBlock.forward (model.py:195-219)
static int vrun_attn(Ctx& c, const VaeAttn& At, const float* x, int H, int W, float* stats, float** out) {
    const int n = H * W;
    const size_t e = (size_t)c.B * n * At.c;
    float* hn = c.A->alloc(e);
    float* q = c.A->alloc(e);
    float* k = c.A->alloc(e);
    float* v = c.A->alloc(e);
    float* o = c.A->alloc(e);
    float* y = c.A->alloc(e);
    if (!c.dry() && launch_group_norm(x, At.nw, At.nb, hn, stats, c.B, n, At.c, 32, 1e-6f, 0, c.s)) return 1;
    if (run_conv(c, At.q, hn, nullptr, H, W, q, 0, nullptr, nullptr, nullptr)) return 1;
    if (run_conv(c, At.k, hn, nullptr, H, W, k, 0, nullptr, nullptr, nullptr)) return 1;
    if (run_conv(c, At.v, hn, nullptr, H, W, v, 0, nullptr, nullptr, nullptr)) return 1;
    if (!c.dry()) {
        if (launch_vae_attention(q, k, v, o, c.B, n, At.c, /*force_rows=*/false, c.s)) return 1;
    }
    if (run_conv(c, At.proj, o, nullptr, H, W, y, EPI_RESIDUAL, nullptr, nullptr, x)) return 1;
    *out = y;
    return 0;
}

// One VAE_CONV node on `cur` of *h x *w pixels (run_trunk and dm_op_vae_conv): the output size into *h, *w; the output into
// `out`, or into a buffer of the arena when there is none; *y is where it went.
static int vrun_conv(Ctx& c, const VaeNode& N, const float* cur, int* h, int* w, float* out, float** y) {
    const int hin = N.up ? 2 * *h : *h, win = N.up ? 2 * *w : *w;  // run_conv takes the size behind the nearest x2
    *h = (hin + 2 * N.pad + N.pad_hi - N.k) / N.stride + 1;
    *w = (win + 2 * N.pad + N.pad_hi - N.k) / N.stride + 1;
    *y = out ? out : c.A->alloc((size_t)c.B * *h * *w * N.cout);
    return run_conv(c, N.conv, cur, nullptr, hin, win, *y, 0, nullptr, nullptr, nullptr, N.in_nchw, N.out_nchw);
}

// The trunk on x of h x w pixels.  Every node's output is a buffer of the arena that nothing releases, except that the last
// node writes to `out` when there is one.  *last, *h_out, *w_out (each may be null): the last node's output as pixel rows,
// or `out`, and its size.
static int run_trunk(VaeHandle* d, Arena& A, const float* x, float* out, int B, int h, int w, hipStream_t s,
                     float** last = nullptr, int* h_out = nullptr, int* w_out = nullptr) {
    Ctx c{&d->holder, &A, s, B, nullptr, 0};
    float* stats = A.alloc(group_stats_ws_floats(B, 32));  // (mean, rstd) + per-block partial sums (launch_group_norm)
    const float* cur = x;
    float* y = nullptr;
    for (const VaeNode& N : d->trunk) {
        switch (N.kind) {
        case VAE_RES:
            if (vrun_res(c, N.res, cur, h, w, stats, &y)) return 1;
            break;
        case VAE_ATTN:
            if (vrun_attn(c, N.attn, cur, h, w, stats, &y)) return 1;
            break;
        case VAE_NORM:
            y = A.alloc((size_t)B * h * w * N.cin);
            if (!A.dry && launch_group_norm(cur, N.nw, N.nb, y, stats, B, h * w, N.cin, 32, 1e-6f, 1, s)) return 1;
            break;
        case VAE_CONV:
            if (vrun_conv(c, N, cur, &h, &w, &N == &d->trunk.back() ? out : nullptr, &y)) return 1;
            break;
        }
        cur = y;
    }
    if (last) *last = y;
    if (h_out) *h_out = h;
    if (w_out) *w_out = w;
    return 0;
}

// `body` on a dry Arena to size the workspace, then on the holder's workspace
template <class Body>
static int with_workspace(dm_unet* holder, Body body) {
    Arena dry;
    dry.dry = true;
    if (body(dry)) return 1;
    if (ensure_workspace(holder, dry.off)) return 1;
    Arena A;
    A.base = holder->ws;
    A.cap = holder->ws_cap;
    return body(A);
}

static int encoder_forward_impl(dm_encoder* d, Arena& A, const float* x, float* zq, float* pre_quant, int* indices, int B,
                                int H, int W, hipStream_t s) {
    float* pq;  // the quant_conv output as pixel rows (B * h * w, embed_dim)
    int h, w;
    if (run_trunk(d, A, x, nullptr, B, H, W, s, &pq, &h, &w)) return 1;
    if (A.dry) return 0;
    if (pre_quant && launch_nhwc_to_nchw(pq, pre_quant, B, d->cfg.embed_dim, h * w, s)) return 1;
    if (zq) {
        if (launch_vq_nearest(pq, d->codebook, d->code_sq, zq, indices, (int64_t)B * h * w, d->cfg.embed_dim, d->cfg.n_embed, h * w, s))
            return 1;
    }
    return 0;
}

// AutoencoderKL.encode (+ sample / mode / kl of the posterior): the trunk, then one pass over the moment rows
static int encoder_forward_kl_impl(dm_encoder* d, Arena& A, const float* x, float* moments_nchw, float* z, float* kl,
                                   const float* eps, uint64_t seed, uint64_t draw, uint64_t element_offset, int sample, int B,
                                   int H, int W, hipStream_t s) {
    float* pq;
    int h, w;
    if (run_trunk(d, A, x, nullptr, B, H, W, s, &pq, &h, &w)) return 1;
    float* ws = kl ? A.alloc(kl_posterior_ws_floats(B, d->cfg.embed_dim, h * w)) : nullptr;
    if (A.dry) return 0;
    return launch_kl_posterior(pq, /*rows=*/1, eps, seed, draw, element_offset, sample, z, moments_nchw, kl, ws, B,
                               d->cfg.embed_dim, h * w, s);
}

// |e_j|^2 of every codebook row: fp32, summed in channel order like torch.sum(embedding.weight ** 2, dim=1)
static std::vector<float> code_sq_host(const float* cb, int n_embed, int E) {
    std::vector<float> sq((size_t)n_embed);
    for (int j = 0; j < n_embed; ++j) {
        float s2 = 0.f;
        for (int c = 0; c < E; ++c) s2 += cb[(size_t)j * E + c] * cb[(size_t)j * E + c];
        sq[j] = s2;
    }
    return sq;
}

// what only one of the two cfg types can get wrong
static int check_cfg(const dm_decoder_cfg*) { return 0; }
static int check_cfg(const dm_encoder_cfg* cfg) {
    DM_REQUIRE(cfg->n_embed >= 0 && cfg->embed_dim > 0, "codebook shape");
    DM_REQUIRE(cfg->n_embed > 0 || cfg->double_z != 0, "an encoder without a codebook (n_embed == 0, AutoencoderKL) needs double_z");
    return 0;
}

// A handle that expects the parameters of build(cfg)
template <class Handle, class Cfg>
static int vae_create(const Cfg* cfg, int device, Handle** out, VaeTrunk (*build)(const Cfg&)) {
    DM_REQUIRE(cfg && out, "null argument");
    DM_REQUIRE(cfg->n_levels >= 1 && cfg->n_levels <= DM_MAX_STAGES, "n_levels out of range");
    DM_REQUIRE(cfg->ch % 32 == 0, "GroupNorm(32) needs ch % 32 == 0");
    if (check_cfg(cfg)) return 1;
    int ndev = 0;
    DM_CHECK_HIP(hipGetDeviceCount(&ndev));
    DM_REQUIRE(device >= 0 && device < ndev, "no such HIP device");
    auto d = std::make_unique<Handle>();
    d->device = device;
    d->cfg.n_levels = cfg->n_levels;
    d->cfg.embed_dim = cfg->embed_dim;
    d->holder.device = device;
    init_dummy(d->holder, 4, 32);
    d->trunk = build(*cfg);
    for (const VaeNode& N : d->trunk) expect_node(&d->holder, N);
    *out = d.release();
    return 0;
}

static void vae_destroy(VaeHandle* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->holder.ws) (void)hipFree(d->holder.ws);
    d->holder.ws = nullptr;
    delete d;
}

static int vae_set_param(VaeHandle* d, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    DM_REQUIRE(d, "null handle");
    DM_REQUIRE(!d->finalized, "set_param after finalize");
    return dm_unet_set_param(&d->holder, name, data_host, shape, ndim);
}

static int vae_missing_params(VaeHandle* d) { return d ? dm_unet_missing_params(&d->holder) : -1; }

static int vae_finalize(VaeHandle* d) {
    DM_REQUIRE(d, "null handle");
    DM_REQUIRE(!d->finalized, "already finalized");
    if (vae_missing_params(d) != 0) return 1;
    DM_CHECK_HIP(hipSetDevice(d->device));
    dm_unet* u = &d->holder;
    for (VaeNode& N : d->trunk)
        if (build_node(u, N)) return 1;
    if (d->cfg.n_embed > 0) {
        const HostTensor& cb = P(u, "quantize.embedding.weight");
        const std::vector<float> sq = code_sq_host(cb.data.data(), d->cfg.n_embed, d->cfg.embed_dim);
        const float zero = 0.f;
        if (u->own.upload(cb.data.data(), cb.data.size(), &d->codebook) || u->own.upload(sq.data(), sq.size(), &d->code_sq) ||
            u->own.upload(&zero, 1, &d->bad_index))
            return 1;
    }
    for (auto& kv : u->params) std::vector<float>().swap(kv.second.data);
    d->finalized = true;
    return 0;
}

}  // namespace dm

extern "C" {

int dm_decoder_create(const dm_decoder_cfg* cfg, int device, dm_decoder** out) {
    return vae_create(cfg, device, out, decoder_nodes);
}
void dm_decoder_destroy(dm_decoder* d) { vae_destroy(d); }
int dm_decoder_set_param(dm_decoder* d, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    return vae_set_param(d, name, data_host, shape, ndim);
}
int dm_decoder_missing_params(dm_decoder* d) { return vae_missing_params(d); }
int dm_decoder_finalize(dm_decoder* d) { return vae_finalize(d); }

int dm_decoder_forward(dm_decoder* d, const float* z, float* out, int B, int h, int w, void* stream) {
    DM_REQUIRE(d && z && out, "null argument");
    DM_REQUIRE(d->finalized, "dm_decoder_finalize has not been called");
    DM_REQUIRE(B > 0 && h > 0 && w > 0, "empty input");
    DM_CHECK_HIP(hipSetDevice(d->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_workspace(&d->holder, [&](Arena& A) { return run_trunk(d, A, z, out, B, h, w, s); });
}

int dm_encoder_create(const dm_encoder_cfg* cfg, int device, dm_encoder** out) {
    if (vae_create(cfg, device, out, encoder_nodes)) return 1;
    (*out)->cfg.n_embed = cfg->n_embed;
    if (cfg->n_embed > 0) expect(&(*out)->holder, "quantize.embedding.weight", {cfg->n_embed, cfg->embed_dim});
    return 0;
}
void dm_encoder_destroy(dm_encoder* d) { vae_destroy(d); }
int dm_encoder_set_param(dm_encoder* d, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    return vae_set_param(d, name, data_host, shape, ndim);
}
int dm_encoder_missing_params(dm_encoder* d) { return vae_missing_params(d); }
int dm_encoder_finalize(dm_encoder* d) { return vae_finalize(d); }

int dm_encoder_forward(dm_encoder* d, const float* x, float* zq, float* pre_quant, int32_t* indices, int B, int H, int W,
                       void* stream) {
    DM_REQUIRE(d && x && (zq || pre_quant), "null argument");
    DM_REQUIRE(d->finalized, "dm_encoder_finalize has not been called");
    DM_REQUIRE(!d->kl(), "this handle has no codebook (n_embed == 0): use dm_encoder_forward_kl");
    DM_REQUIRE(B > 0 && H > 0 && W > 0, "empty input");
    const int f = 1 << (d->cfg.n_levels - 1);
    DM_REQUIRE(H % f == 0 && W % f == 0, "image size must be divisible by the encoder's downsampling factor");
    DM_CHECK_HIP(hipSetDevice(d->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_workspace(&d->holder,
                          [&](Arena& A) { return encoder_forward_impl(d, A, x, zq, pre_quant, indices, B, H, W, s); });
}

int dm_encoder_forward_kl(dm_encoder* d, const float* x, float* moments_nchw, float* z, float* kl, const float* eps,
                          uint64_t seed, uint64_t draw, uint64_t element_offset, int sample, int B, int H, int W, void* stream) {
    DM_REQUIRE(d && x && (moments_nchw || z || kl), "null argument");
    DM_REQUIRE(d->finalized, "dm_encoder_finalize has not been called");
    DM_REQUIRE(d->kl(), "this handle quantises (n_embed > 0): use dm_encoder_forward");
    DM_REQUIRE(B > 0 && H > 0 && W > 0, "empty input");
    const int f = 1 << (d->cfg.n_levels - 1);
    DM_REQUIRE(H % f == 0 && W % f == 0, "image size must be divisible by the encoder's downsampling factor");
    if (z && sample && !eps) {  // refused here, before the encoder has run
        DM_REQUIRE((int64_t)d->cfg.embed_dim * (H / f) * (W / f) % 4 == 0,
                   "Philox noise needs embed_dim * h * w % 4 == 0 (one counter serves four elements)");
        DM_REQUIRE(element_offset % 4 == 0, "Philox element offset must be a multiple of 4 (one counter serves 4 elements)");
    }
    DM_CHECK_HIP(hipSetDevice(d->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_workspace(&d->holder, [&](Arena& A) {
        return encoder_forward_kl_impl(d, A, x, moments_nchw, z, kl, eps, seed, draw, element_offset, sample, B, H, W, s);
    });
}

int dm_encoder_quantize(dm_encoder* d, const float* h_nchw, float* zq, int32_t* indices, int B, int h, int w, void* stream) {
    DM_REQUIRE(d && h_nchw && zq, "null argument");
    DM_REQUIRE(d->finalized, "dm_encoder_finalize has not been called");
    DM_REQUIRE(!d->kl(), "this handle has no codebook (n_embed == 0)");
    DM_REQUIRE(B > 0 && h > 0 && w > 0, "empty input");
    DM_CHECK_HIP(hipSetDevice(d->device));
    return launch_vq_nearest(h_nchw, d->codebook, d->code_sq, zq, indices, (int64_t)B * h * w, d->cfg.embed_dim, d->cfg.n_embed,
                             h * w, static_cast<hipStream_t>(stream), /*in_nchw=*/true);
}

// the flag of embed_code_kernel, read after the stream has drained: an index outside the codebook is the caller's error
static int embed_code_verdict(int rc, const int* bad_dev, hipStream_t s) {
    if (rc) return rc;
    int bad = 0;
    DM_CHECK_HIP(hipMemcpyAsync(&bad, bad_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    DM_CHECK_HIP(hipStreamSynchronize(s));
    DM_REQUIRE(bad == 0, "embed_code: an index lies outside [0, n_embed)");
    return 0;
}

int dm_encoder_embed_code(dm_encoder* d, const int64_t* indices, float* out, int B, int h, int w, void* stream) {
    DM_REQUIRE(d && indices && out, "null argument");
    DM_REQUIRE(d->finalized, "dm_encoder_finalize has not been called");
    DM_REQUIRE(!d->kl(), "this handle has no codebook (n_embed == 0)");
    DM_REQUIRE(B > 0 && h > 0 && w > 0, "empty input");
    DM_CHECK_HIP(hipSetDevice(d->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int* bad = reinterpret_cast<int*>(d->bad_index);
    return embed_code_verdict(launch_embed_code(indices, 8, d->codebook, out, bad, (int64_t)B * h * w, d->cfg.embed_dim, d->cfg.n_embed,
                                                h * w, s), bad, s);
}

}  // extern "C"

// =====================================================================================================
// The three kernels groups above on their own (dm_op_*): the same launch functions, workspaces owned by the call.
// =====================================================================================================
namespace dm {

// wait for the stream, release the call's scratch buffers, report an execution error
static int finish_vae_op(int rc, hipStream_t s, void* buf0, void* buf1 = nullptr) {
    hipError_t e = hipStreamSynchronize(s);
    if (buf0) (void)hipFree(buf0);
    if (buf1) (void)hipFree(buf1);
    if (!rc && e != hipSuccess) {
        set_error(std::string("kernel execution failed: ") + hipGetErrorString(e));
        rc = 1;
    }
    return rc;
}

// dm_op_vq_nearest (z as pixel rows) and dm_op_vq_nearest_nchw behind their null checks
static int vq_nearest_op(const float* z, const float* codebook, float* zq_nchw, int32_t* indices, int64_t pixels, int E,
                         int n_embed, int hw, void* stream, bool in_nchw) {
    DM_REQUIRE(pixels > 0 && E > 0 && n_embed > 0 && hw > 0, "empty input");
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<float> cb;
    if (d2h(codebook, (size_t)n_embed * E, cb)) return 1;
    const std::vector<float> sq = code_sq_host(cb.data(), n_embed, E);
    float* e2 = nullptr;
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&e2), sq.size() * sizeof(float)));
    hipError_t e = hipMemcpy(e2, sq.data(), sq.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(e2);
        DM_CHECK_HIP(e);
    }
    int rc = launch_vq_nearest(z, codebook, e2, zq_nchw, indices, pixels, E, n_embed, hw, s, in_nchw);
    return finish_vae_op(rc, s, e2);
}

// One node of the trunk on its own (dm_op_vae_conv, dm_op_vae_resblock, dm_op_vae_attn_block).  `params`: the node's
// parameters as device pointers in the order of expect_node; they go through the host into a handle of their own, which
// build_node packs and uploads as it does for the networks.  `x` -> `out` in the layouts of the trunk.
static int vae_node_op(VaeNode& N, std::initializer_list<const float*> params, const float* x, float* out, int B, int H, int W,
                       void* stream) {
    DM_REQUIRE(x && out, "null argument");
    DM_REQUIRE(B > 0 && H > 0 && W > 0 && N.cin > 0 && N.cout > 0, "empty input");
    hipStream_t s = static_cast<hipStream_t>(stream);
    dm_unet dummy;
    init_dummy(dummy, 4, 32);
    expect_node(&dummy, N);
    DM_REQUIRE(params.size() == dummy.order.size(), "parameter list of another node kind");
    auto p = params.begin();
    for (const std::string& name : dummy.order) {
        DM_REQUIRE(*p, "null argument");
        HostTensor& t = dummy.params[name];
        if (d2h(*p++, t.numel(), t.data)) return 1;
        t.set = true;
    }
    if (build_node(&dummy, N)) return 1;
    return run_op(s, [&](Arena& A) -> int {
        Ctx c{&dummy, &A, s, B, nullptr, 0};
        float* y = nullptr;
        int h = H, w = W;
        if (N.kind == VAE_CONV) return vrun_conv(c, N, x, &h, &w, out, &y);
        float* stats = A.alloc(group_stats_ws_floats(B, 32));
        if (N.kind == VAE_RES ? vrun_res(c, N.res, x, H, W, stats, &y) : vrun_attn(c, N.attn, x, H, W, stats, &y)) return 1;
        if (!A.dry)
            DM_CHECK_HIP(hipMemcpyAsync(out, y, (size_t)B * H * W * N.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    });
}

}  // namespace dm

extern "C" {

int dm_op_vae_conv(const float* in, const float* weight, const float* bias, float* out, int B, int H, int W, int Cin, int Cout,
                   int k, int stride, int pad, int pad_hi, int up, int in_nchw, int out_nchw, void* stream) {
    DM_REQUIRE(weight, "null argument");
    DM_REQUIRE(k > 0 && stride > 0 && pad >= 0 && pad_hi >= 0, "VAE conv: k, stride > 0 and pad, pad_hi >= 0");
    const int hin = up ? 2 * H : H, win = up ? 2 * W : W;
    DM_REQUIRE(hin + 2 * pad + pad_hi >= k && win + 2 * pad + pad_hi >= k, "VAE conv: the kernel is larger than the padded image");
    dm::VaeNode N{dm::VAE_CONV, "op", Cin, Cout, 0};
    N.k = k; N.stride = stride; N.pad = pad; N.pad_hi = pad_hi;
    N.up = up != 0; N.in_nchw = in_nchw != 0; N.out_nchw = out_nchw != 0; N.bias = bias != nullptr;
    if (bias) return dm::vae_node_op(N, {weight, bias}, in, out, B, H, W, stream);
    return dm::vae_node_op(N, {weight}, in, out, B, H, W, stream);
}

int dm_op_vae_resblock(const float* x, const float* norm1_w, const float* norm1_b, const float* conv1_w, const float* conv1_b,
                       const float* norm2_w, const float* norm2_b, const float* conv2_w, const float* conv2_b,
                       const float* nin_w, const float* nin_b, float* out, int B, int H, int W, int cin, int cout,
                       void* stream) {
    DM_REQUIRE((nin_w == nullptr) == (cin == cout) && (nin_b == nullptr) == (cin == cout),
               "nin_shortcut is given exactly when cin != cout");
    dm::VaeNode N{dm::VAE_RES, "op", cin, cout, 0};
    if (cin == cout)
        return dm::vae_node_op(N, {norm1_w, norm1_b, conv1_w, conv1_b, norm2_w, norm2_b, conv2_w, conv2_b}, x, out, B, H, W, stream);
    return dm::vae_node_op(N, {norm1_w, norm1_b, conv1_w, conv1_b, norm2_w, norm2_b, conv2_w, conv2_b, nin_w, nin_b}, x, out, B,
                           H, W, stream);
}

int dm_op_vae_attn_block(const float* x, const float* norm_w, const float* norm_b, const float* q_w, const float* q_b,
                         const float* k_w, const float* k_b, const float* v_w, const float* v_b, const float* proj_w,
                         const float* proj_b, float* out, int B, int H, int W, int C, void* stream) {
    dm::VaeNode N{dm::VAE_ATTN, "op", C, C, 0};
    return dm::vae_node_op(N, {norm_w, norm_b, q_w, q_b, k_w, k_b, v_w, v_b, proj_w, proj_b}, x, out, B, H, W, stream);
}

int dm_op_group_norm(const float* x_nhwc, const float* weight, const float* bias, float* y_nhwc, int B, int HW, int C,
                     int groups, float eps, int swish, void* stream) {
    DM_REQUIRE(x_nhwc && weight && bias && y_nhwc, "null argument");
    DM_REQUIRE(B > 0 && HW > 0 && C > 0 && groups > 0, "empty input");
    DM_REQUIRE(B <= 65535 && C % groups == 0, "GroupNorm: B <= 65535 and C % groups == 0");  // before the workspace is sized
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = nullptr;
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&ws), group_stats_ws_floats(B, groups) * sizeof(float)));
    int rc = launch_group_norm(x_nhwc, weight, bias, y_nhwc, ws, B, HW, C, groups, eps, swish, s);
    return finish_vae_op(rc, s, ws);
}

int dm_op_vae_attention(const float* q, const float* k, const float* v, float* out, int B, int n, int C, int kernel,
                        void* stream) {
    DM_REQUIRE(q && k && v && out, "null argument");
    DM_REQUIRE(kernel == 0 || kernel == 1, "kernel: 0 (as the model dispatches) or 1 (row kernel)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_vae_attention(q, k, v, out, B, n, C, kernel == 1, s);
    return finish_vae_op(rc, s, nullptr);
}

int dm_op_vq_nearest(const float* z_rows, const float* codebook, float* zq_nchw, int32_t* indices, int64_t pixels, int E,
                     int n_embed, int hw, void* stream) {
    DM_REQUIRE(z_rows && codebook && zq_nchw, "null argument");
    return vq_nearest_op(z_rows, codebook, zq_nchw, indices, pixels, E, n_embed, hw, stream, /*in_nchw=*/false);
}

int dm_op_vq_nearest_nchw(const float* z_nchw, const float* codebook, float* zq_nchw, int32_t* indices, int64_t pixels, int E,
                          int n_embed, int hw, void* stream) {
    DM_REQUIRE(z_nchw && codebook && zq_nchw, "null argument");
    return vq_nearest_op(z_nchw, codebook, zq_nchw, indices, pixels, E, n_embed, hw, stream, /*in_nchw=*/true);
}

int dm_op_kl_posterior(const float* moments, int layout, const float* eps, uint64_t seed, uint64_t draw,
                       uint64_t element_offset, int sample, float* z, float* moments_nchw, float* kl, int B, int E, int hw,
                       void* stream) {
    DM_REQUIRE(moments && (z || moments_nchw || kl), "null argument");
    DM_REQUIRE(layout == DM_KL_NCHW || layout == DM_KL_ROWS, "layout: DM_KL_NCHW or DM_KL_ROWS");
    DM_REQUIRE(B > 0 && B <= 65535 && E > 0 && hw > 0, "empty input, or B > 65535");  // before the workspace is sized
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = nullptr;
    if (kl) DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&ws), kl_posterior_ws_floats(B, E, hw) * sizeof(float)));
    int rc = launch_kl_posterior(moments, layout == DM_KL_ROWS, eps, seed, draw, element_offset, sample, z, moments_nchw, kl,
                                 ws, B, E, hw, s);
    return finish_vae_op(rc, s, ws);
}

int dm_op_embed_code(const void* indices, int index_bytes, const float* codebook, float* out_nchw, int64_t pixels, int E,
                     int n_embed, int hw, void* stream) {
    DM_REQUIRE(indices && codebook && out_nchw, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int* bad = nullptr;
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&bad), sizeof(int)));
    int rc = embed_code_verdict(launch_embed_code(indices, index_bytes, codebook, out_nchw, bad, pixels, E, n_embed, hw, s),
                                bad, s);
    return finish_vae_op(rc, s, bad);
}

}  // extern "C"
