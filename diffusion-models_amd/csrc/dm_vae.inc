// VAE decode for the latent-diffusion path (textually included at the end of dm_api.hip).
// Replaces VQModel.decode (LD/models/autoencoder.py:113-116) = post_quant_conv (1x1) ->
// Decoder.forward (LD/modules/diffusionmodules/model.py:552-585).  Runs once per sample() call.
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
struct VaeLevel {
    std::vector<VaeRes> blocks;
    std::vector<VaeAttn> attns;
    bool has_up = false;
    ConvLayer up;
};

// single-head attention over n tokens of C channels (AttnBlock, model.py:203-215): one query row
// per wavefront; keys/values stream from L2.  q,k,v,out: (B, n, C) rows.
__global__ __launch_bounds__(256) void attention_rows_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ v, float* __restrict__ out,
                                                             int n, int C, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int i = blockIdx.x * 4 + wave;
    float* qs = sm + wave * (C + n);
    float* ps = qs + C;
    if (i >= n) return;
    const float* qb = q + ((size_t)b * n + i) * C;
    for (int c = lane; c < C; c += 64) qs[c] = qb[c];
    __builtin_amdgcn_wave_barrier();
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) {
        const float* kr = k + ((size_t)b * n + j) * C;
        float acc = 0.f;
        for (int c = 0; c < C; c += 4) {
            float4 kk = *reinterpret_cast<const float4*>(kr + c);
            acc += qs[c] * kk.x + qs[c + 1] * kk.y + qs[c + 2] * kk.z + qs[c + 3] * kk.w;
        }
        acc *= scale;
        ps[j] = acc;
        mx = fmaxf(mx, acc);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) {
        float e = __expf(ps[j] - mx);
        ps[j] = e;
        sum += e;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    __builtin_amdgcn_wave_barrier();
    const float inv = 1.0f / sum;
    float* ob = out + ((size_t)b * n + i) * C;
    for (int c = lane; c < C; c += 64) {
        float acc = 0.f;
        const float* vb = v + (size_t)b * n * C + c;
        for (int j = 0; j < n; ++j) acc += ps[j] * vb[(size_t)j * C];
        ob[c] = acc * inv;
    }
}

static int launch_attention_rows(const float* q, const float* k, const float* v, float* out, int B, int n, int C,
                                 hipStream_t s) {
    DM_REQUIRE(C % 4 == 0, "VAE attention needs C % 4 == 0");
    size_t lds = 4 * (size_t)(C + n) * sizeof(float);
    DM_REQUIRE(lds <= 160 * 1024, "VAE attention: too many tokens for this kernel");  // n + C <= 10240
    static LdsOptIn lds_flag;
    if (lds_opt_in(lds_flag, reinterpret_cast<const void*>(attention_rows_kernel), 1)) return 1;
    hipLaunchKernelGGL(attention_rows_kernel, dim3((n + 3) / 4, B), dim3(256), lds, s, q, k, v, out, n, C,
                       1.0f / sqrtf((float)C));
    DM_CHECK_HIP(hipGetLastError());
    return 0;
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

}  // namespace dm

struct dm_decoder {
    dm_decoder_cfg cfg{};
    int device = 0;
    dm_unet holder;  // parameter table, device buffers and workspace management are shared code
    bool finalized = false;
    ConvLayer post_quant, conv_in, conv_out;
    VaeRes mid1, mid2;
    VaeAttn mid_attn;
    std::vector<VaeLevel> levels;
    float *now = nullptr, *nob = nullptr;
    int block_in_final = 0;
};

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

static int decoder_forward_impl(dm_decoder* d, Arena& A, const float* z, float* out, int B, int h, int w,
                                hipStream_t s) {
    const dm_decoder_cfg& cfg = d->cfg;
    Ctx c{&d->holder, &A, s, B, nullptr, 0};
    int maxC = cfg.ch * cfg.ch_mult[cfg.n_levels - 1];
    (void)maxC;
    float* stats = A.alloc(group_stats_ws_floats(B, 32));  // (mean, rstd) + per-block partial sums (launch_group_norm)
    float* zq = A.alloc((size_t)B * h * w * cfg.z_channels);
    if (run_conv(c, d->post_quant, z, nullptr, h, w, zq, 0, nullptr, nullptr, nullptr, /*in_nchw=*/true)) return 1;
    float* cur = A.alloc((size_t)B * h * w * d->conv_in.Cout);
    if (run_conv(c, d->conv_in, zq, nullptr, h, w, cur, 0, nullptr, nullptr, nullptr)) return 1;
    float* t;
    if (vrun_res(c, d->mid1, cur, h, w, stats, &t)) return 1; cur = t;
    if (vrun_attn(c, d->mid_attn, cur, h, w, stats, &t)) return 1; cur = t;
    if (vrun_res(c, d->mid2, cur, h, w, stats, &t)) return 1; cur = t;
    for (int lvl = cfg.n_levels - 1; lvl >= 0; --lvl) {
        VaeLevel& L = d->levels[lvl];
        for (size_t b = 0; b < L.blocks.size(); ++b) {
            if (vrun_res(c, L.blocks[b], cur, h, w, stats, &t)) return 1; cur = t;
            if (!L.attns.empty()) { if (vrun_attn(c, L.attns[b], cur, h, w, stats, &t)) return 1; cur = t; }
        }
        if (L.has_up) {
            float* u = A.alloc((size_t)B * 4 * h * w * L.up.Cout);
            if (run_conv(c, L.up, cur, nullptr, 2 * h, 2 * w, u, 0, nullptr, nullptr, nullptr)) return 1;
            cur = u; h *= 2; w *= 2;
        }
    }
    float* a = A.alloc((size_t)B * h * w * d->block_in_final);
    if (!A.dry && launch_group_norm(cur, d->now, d->nob, a, stats, B, h * w, d->block_in_final, 32, 1e-6f, 1, s)) return 1;
    return run_conv(c, d->conv_out, a, nullptr, h, w, out, 0, nullptr, nullptr, nullptr, false, /*out_nchw=*/true);
}

}  // namespace dm

extern "C" {

int dm_decoder_create(const dm_decoder_cfg* cfg, int device, dm_decoder** out) {
    DM_REQUIRE(cfg && out, "null argument");
    DM_REQUIRE(cfg->n_levels >= 1 && cfg->n_levels <= DM_MAX_STAGES, "n_levels out of range");
    DM_REQUIRE(cfg->ch % 32 == 0, "GroupNorm(32) needs ch % 32 == 0");
    int ndev = 0;
    DM_CHECK_HIP(hipGetDeviceCount(&ndev));
    DM_REQUIRE(device >= 0 && device < ndev, "no such HIP device");
    auto d = std::make_unique<dm_decoder>();
    d->cfg = *cfg;
    d->device = device;
    d->holder.device = device;
    init_dummy(d->holder, 4, 32);
    dm_unet* u = &d->holder;
    int block_in = cfg->ch * cfg->ch_mult[cfg->n_levels - 1];
    int curr_res = cfg->resolution >> (cfg->n_levels - 1);
    expect(u, "post_quant_conv.weight", {cfg->z_channels, cfg->embed_dim, 1, 1});
    expect(u, "post_quant_conv.bias", {cfg->z_channels});
    expect(u, "decoder.conv_in.weight", {block_in, cfg->z_channels, 3, 3});
    expect(u, "decoder.conv_in.bias", {block_in});
    vexpect_res(u, "decoder.mid.block_1", block_in, block_in);
    vexpect_attn(u, "decoder.mid.attn_1", block_in);
    vexpect_res(u, "decoder.mid.block_2", block_in, block_in);
    for (int lvl = cfg->n_levels - 1; lvl >= 0; --lvl) {
        int block_out = cfg->ch * cfg->ch_mult[lvl];
        bool attn = false;
        for (int a = 0; a < cfg->n_attn_res; ++a) attn = attn || cfg->attn_resolutions[a] == curr_res;
        std::string p = "decoder.up." + std::to_string(lvl);
        for (int b = 0; b < cfg->num_res_blocks + 1; ++b) {
            vexpect_res(u, p + ".block." + std::to_string(b), block_in, block_out);
            block_in = block_out;
            if (attn) vexpect_attn(u, p + ".attn." + std::to_string(b), block_in);
        }
        if (lvl != 0) {
            expect(u, p + ".upsample.conv.weight", {block_in, block_in, 3, 3});
            expect(u, p + ".upsample.conv.bias", {block_in});
            curr_res *= 2;
        }
    }
    expect(u, "decoder.norm_out.weight", {block_in});
    expect(u, "decoder.norm_out.bias", {block_in});
    expect(u, "decoder.conv_out.weight", {cfg->out_ch, block_in, 3, 3});
    expect(u, "decoder.conv_out.bias", {cfg->out_ch});
    *out = d.release();
    return 0;
}

void dm_decoder_destroy(dm_decoder* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->holder.ws) (void)hipFree(d->holder.ws);
    d->holder.ws = nullptr;
    delete d;
}

int dm_decoder_set_param(dm_decoder* d, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    DM_REQUIRE(d, "null handle");
    DM_REQUIRE(!d->finalized, "set_param after finalize");
    return dm_unet_set_param(&d->holder, name, data_host, shape, ndim);
}

int dm_decoder_missing_params(dm_decoder* d) { return d ? dm_unet_missing_params(&d->holder) : -1; }

int dm_decoder_finalize(dm_decoder* d) {
    DM_REQUIRE(d, "null handle");
    DM_REQUIRE(!d->finalized, "already finalized");
    if (dm_decoder_missing_params(d) != 0) return 1;
    DM_CHECK_HIP(hipSetDevice(d->device));
    const dm_decoder_cfg& cfg = d->cfg;
    dm_unet* u = &d->holder;
    int block_in = cfg.ch * cfg.ch_mult[cfg.n_levels - 1];
    int curr_res = cfg.resolution >> (cfg.n_levels - 1);
    if (vconv(u, d->post_quant, "post_quant_conv", cfg.z_channels, cfg.embed_dim, 1, 0, false)) return 1;
    if (vconv(u, d->conv_in, "decoder.conv_in", block_in, cfg.z_channels, 3, 1, false)) return 1;
    if (vbuild_res(u, d->mid1, "decoder.mid.block_1", block_in, block_in)) return 1;
    if (vbuild_attn(u, d->mid_attn, "decoder.mid.attn_1", block_in)) return 1;
    if (vbuild_res(u, d->mid2, "decoder.mid.block_2", block_in, block_in)) return 1;
    d->levels.resize(cfg.n_levels);
    for (int lvl = cfg.n_levels - 1; lvl >= 0; --lvl) {
        int block_out = cfg.ch * cfg.ch_mult[lvl];
        bool attn = false;
        for (int a = 0; a < cfg.n_attn_res; ++a) attn = attn || cfg.attn_resolutions[a] == curr_res;
        std::string p = "decoder.up." + std::to_string(lvl);
        VaeLevel& L = d->levels[lvl];
        L.blocks.resize(cfg.num_res_blocks + 1);
        if (attn) L.attns.resize(cfg.num_res_blocks + 1);
        for (int b = 0; b < cfg.num_res_blocks + 1; ++b) {
            if (vbuild_res(u, L.blocks[b], p + ".block." + std::to_string(b), block_in, block_out)) return 1;
            block_in = block_out;
            if (attn && vbuild_attn(u, L.attns[b], p + ".attn." + std::to_string(b), block_in)) return 1;
        }
        L.has_up = lvl != 0;
        if (L.has_up) {
            if (vconv(u, L.up, p + ".upsample.conv", block_in, block_in, 3, 1, /*up=*/true)) return 1;
            curr_res *= 2;
        }
    }
    d->block_in_final = block_in;
    if (up1(u, "decoder.norm_out.weight", &d->now) || up1(u, "decoder.norm_out.bias", &d->nob)) return 1;
    if (vconv(u, d->conv_out, "decoder.conv_out", cfg.out_ch, block_in, 3, 1, false)) return 1;
    for (auto& kv : u->params) std::vector<float>().swap(kv.second.data);
    d->finalized = true;
    return 0;
}

int dm_decoder_forward(dm_decoder* d, const float* z, float* out, int B, int h, int w, void* stream) {
    DM_REQUIRE(d && z && out, "null argument");
    DM_REQUIRE(d->finalized, "dm_decoder_finalize has not been called");
    DM_REQUIRE(B > 0 && h > 0 && w > 0, "empty input");
    DM_CHECK_HIP(hipSetDevice(d->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Arena dry;
    dry.dry = true;
    if (decoder_forward_impl(d, dry, z, out, B, h, w, s)) return 1;
    if (ensure_workspace(&d->holder, dry.off)) return 1;
    Arena A;
    A.base = d->holder.ws;
    A.cap = d->holder.ws_cap;
    return decoder_forward_impl(d, A, z, out, B, h, w, s);
}

}  // extern "C"

// =====================================================================================================
// VAE encode for the image-conditional latent path: VQModel.encode (LD/models/autoencoder.py:102-106) =
// Encoder.forward (LD/modules/diffusionmodules/model.py:451-476) -> quant_conv (1x1) -> VectorQuantizer.
// The quantizer is taming-transformers' VectorQuantizer2 (taming/modules/vqvae/quantize.py, a pip dependency that
// is not in the reference tree): nearest codebook row under d = |z|^2 + |e|^2 - 2 z.e, output z + (e - z).
// =====================================================================================================
namespace dm {

// One wavefront per latent pixel: lane l scans codes l, l+64, ...; ties resolve to the lowest index (torch.argmin).
// z: (pixels, E) rows, or (B, E, hw) NCHW when NCHW (the sampler's latents; the same arithmetic in the same order on the
// same values); e: (n_embed, E); e2[j] = sum_c e[j][c]^2; zq_nchw (B, E, hw); idx (pixels) or nullptr.
template <bool NCHW>
__global__ __launch_bounds__(256) void vq_nearest_kernel(const float* __restrict__ z, const float* __restrict__ e,
                                                         const float* __restrict__ e2, float* __restrict__ zq_nchw,
                                                         int* __restrict__ idx, int64_t pixels, int E, int n_embed,
                                                         int hw) {
    const int lane = threadIdx.x & 63;
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= pixels) return;
    const int64_t b = pix / hw, sp = pix - b * hw;
    const float* zr = NCHW ? z + b * E * hw + sp : z + pix * E;
    const int64_t cs = NCHW ? hw : 1;  // distance between two channels of a pixel
    float z2 = 0.f;
    for (int c = 0; c < E; ++c) z2 += zr[c * cs] * zr[c * cs];
    float best = INFINITY;
    int bi = 0x7fffffff;
    for (int j = lane; j < n_embed; j += 64) {
        float dot = 0.f;
        for (int c = 0; c < E; ++c) dot += zr[c * cs] * e[(size_t)j * E + c];
        const float d = z2 + e2[j] - 2.0f * dot;
        if (d < best) {
            best = d;
            bi = j;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m);
        const int oi = __shfl_xor(bi, m);
        if (ob < best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
    }
    for (int c = lane; c < E; c += 64) {
        const float zv = zr[c * cs];
        zq_nchw[(b * E + c) * hw + sp] = zv + (e[(size_t)bi * E + c] - zv);  // z + (z_q - z).detach(), as the reference forms it
    }
    if (idx && lane == 0) idx[pix] = bi;
}

static int launch_vq_nearest(const float* z, const float* e, const float* e2, float* zq_nchw, int* idx, int64_t pixels,
                             int E, int n_embed, int hw, hipStream_t s, bool in_nchw = false) {
    DM_REQUIRE(pixels > 0 && E > 0 && n_embed > 0 && hw > 0, "VQ: empty input");
    DM_REQUIRE(pixels % hw == 0, "VQ: pixels is a whole number of images of hw pixels");
    DM_REQUIRE((pixels + 3) / 4 <= 0x7fffffff, "VQ: too many pixels for one launch");
    const dim3 grid((unsigned)((pixels + 3) / 4));
    if (in_nchw)
        hipLaunchKernelGGL(vq_nearest_kernel<true>, grid, dim3(256), 0, s, z, e, e2, zq_nchw, idx, pixels, E, n_embed, hw);
    else
        hipLaunchKernelGGL(vq_nearest_kernel<false>, grid, dim3(256), 0, s, z, e, e2, zq_nchw, idx, pixels, E, n_embed, hw);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
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

}  // namespace dm

struct dm_encoder {
    dm_encoder_cfg cfg{};
    int device = 0;
    dm_unet holder;
    bool finalized = false;
    ConvLayer conv_in, conv_out, quant_conv;
    VaeRes mid1, mid2;
    VaeAttn mid_attn;
    std::vector<VaeLevel> levels;  // VaeLevel::up holds the level's Downsample conv here
    float *now = nullptr, *nob = nullptr, *codebook = nullptr, *code_sq = nullptr;
    float* bad_index = nullptr;  // one int: raised by embed_code_kernel
    int block_in_final = 0;
    bool kl() const { return cfg.n_embed == 0; }  // AutoencoderKL: quant_conv yields 2 * embed_dim moments, no codebook
};

namespace dm {

// Encoder.forward -> quant_conv: *pq_out = the quant_conv output as pixel rows (B * h * w, quant_conv.Cout) in the arena
static int encoder_trunk(dm_encoder* d, Arena& A, const float* x, int B, int H, int W, hipStream_t s, float** pq_out,
                         int* h_out, int* w_out) {
    const dm_encoder_cfg& cfg = d->cfg;
    Ctx c{&d->holder, &A, s, B, nullptr, 0};
    float* stats = A.alloc(group_stats_ws_floats(B, 32));  // (mean, rstd) + per-block partial sums (launch_group_norm)
    int h = H, w = W;
    float* cur = A.alloc((size_t)B * h * w * cfg.ch);
    if (run_conv(c, d->conv_in, x, nullptr, h, w, cur, 0, nullptr, nullptr, nullptr, /*in_nchw=*/true)) return 1;
    float* t;
    for (int lvl = 0; lvl < cfg.n_levels; ++lvl) {
        VaeLevel& L = d->levels[lvl];
        for (size_t b = 0; b < L.blocks.size(); ++b) {
            if (vrun_res(c, L.blocks[b], cur, h, w, stats, &t)) return 1; cur = t;
            if (!L.attns.empty()) { if (vrun_attn(c, L.attns[b], cur, h, w, stats, &t)) return 1; cur = t; }
        }
        if (L.has_up) {  // Downsample: pad (0,1,0,1) + conv3x3 stride 2 (model.py:89-93)
            const int ho = (h + 1 - 3) / 2 + 1, wo = (w + 1 - 3) / 2 + 1;
            float* dn = A.alloc((size_t)B * ho * wo * L.up.Cout);
            if (run_conv(c, L.up, cur, nullptr, h, w, dn, 0, nullptr, nullptr, nullptr)) return 1;
            cur = dn; h = ho; w = wo;
        }
    }
    if (vrun_res(c, d->mid1, cur, h, w, stats, &t)) return 1; cur = t;
    if (vrun_attn(c, d->mid_attn, cur, h, w, stats, &t)) return 1; cur = t;
    if (vrun_res(c, d->mid2, cur, h, w, stats, &t)) return 1; cur = t;
    float* a = A.alloc((size_t)B * h * w * d->block_in_final);
    if (!A.dry && launch_group_norm(cur, d->now, d->nob, a, stats, B, h * w, d->block_in_final, 32, 1e-6f, 1, s)) return 1;
    float* hz = A.alloc((size_t)B * h * w * d->conv_out.Cout);
    if (run_conv(c, d->conv_out, a, nullptr, h, w, hz, 0, nullptr, nullptr, nullptr)) return 1;
    float* pq = A.alloc((size_t)B * h * w * d->quant_conv.Cout);
    if (run_conv(c, d->quant_conv, hz, nullptr, h, w, pq, 0, nullptr, nullptr, nullptr)) return 1;
    *pq_out = pq;
    *h_out = h;
    *w_out = w;
    return 0;
}

static int encoder_forward_impl(dm_encoder* d, Arena& A, const float* x, float* zq, float* pre_quant, int* indices, int B,
                                int H, int W, hipStream_t s) {
    const dm_encoder_cfg& cfg = d->cfg;
    float* pq;
    int h, w;
    if (encoder_trunk(d, A, x, B, H, W, s, &pq, &h, &w)) return 1;
    if (A.dry) return 0;
    if (pre_quant && launch_nhwc_to_nchw(pq, pre_quant, B, cfg.embed_dim, h * w, s)) return 1;
    if (zq) {
        if (launch_vq_nearest(pq, d->codebook, d->code_sq, zq, indices, (int64_t)B * h * w, cfg.embed_dim, cfg.n_embed,
                              h * w, s))
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
    if (encoder_trunk(d, A, x, B, H, W, s, &pq, &h, &w)) return 1;
    float* ws = kl ? A.alloc(kl_posterior_ws_floats(B, d->cfg.embed_dim, h * w)) : nullptr;
    if (A.dry) return 0;
    return launch_kl_posterior(pq, /*rows=*/1, eps, seed, draw, element_offset, sample, z, moments_nchw, kl, ws, B,
                               d->cfg.embed_dim, h * w, s);
}

}  // namespace dm

extern "C" {

int dm_encoder_create(const dm_encoder_cfg* cfg, int device, dm_encoder** out) {
    DM_REQUIRE(cfg && out, "null argument");
    DM_REQUIRE(cfg->n_levels >= 1 && cfg->n_levels <= DM_MAX_STAGES, "n_levels out of range");
    DM_REQUIRE(cfg->ch % 32 == 0, "GroupNorm(32) needs ch % 32 == 0");
    DM_REQUIRE(cfg->n_embed >= 0 && cfg->embed_dim > 0, "codebook shape");
    DM_REQUIRE(cfg->n_embed > 0 || cfg->double_z != 0, "an encoder without a codebook (n_embed == 0, AutoencoderKL) needs double_z");
    int ndev = 0;
    DM_CHECK_HIP(hipGetDeviceCount(&ndev));
    DM_REQUIRE(device >= 0 && device < ndev, "no such HIP device");
    auto d = std::make_unique<dm_encoder>();
    d->cfg = *cfg;
    d->device = device;
    d->holder.device = device;
    init_dummy(d->holder, 4, 32);
    dm_unet* u = &d->holder;
    expect(u, "encoder.conv_in.weight", {cfg->ch, cfg->in_channels, 3, 3});
    expect(u, "encoder.conv_in.bias", {cfg->ch});
    int curr_res = cfg->resolution, block_in = cfg->ch;
    for (int lvl = 0; lvl < cfg->n_levels; ++lvl) {
        block_in = cfg->ch * (lvl == 0 ? 1 : cfg->ch_mult[lvl - 1]);
        const int block_out = cfg->ch * cfg->ch_mult[lvl];
        bool attn = false;
        for (int a = 0; a < cfg->n_attn_res; ++a) attn = attn || cfg->attn_resolutions[a] == curr_res;
        const std::string p = "encoder.down." + std::to_string(lvl);
        for (int b = 0; b < cfg->num_res_blocks; ++b) {
            vexpect_res(u, p + ".block." + std::to_string(b), block_in, block_out);
            block_in = block_out;
            if (attn) vexpect_attn(u, p + ".attn." + std::to_string(b), block_in);
        }
        if (lvl != cfg->n_levels - 1) {
            expect(u, p + ".downsample.conv.weight", {block_in, block_in, 3, 3});
            expect(u, p + ".downsample.conv.bias", {block_in});
            curr_res /= 2;
        }
    }
    vexpect_res(u, "encoder.mid.block_1", block_in, block_in);
    vexpect_attn(u, "encoder.mid.attn_1", block_in);
    vexpect_res(u, "encoder.mid.block_2", block_in, block_in);
    expect(u, "encoder.norm_out.weight", {block_in});
    expect(u, "encoder.norm_out.bias", {block_in});
    const int zc = cfg->double_z ? 2 * cfg->z_channels : cfg->z_channels;
    expect(u, "encoder.conv_out.weight", {zc, block_in, 3, 3});
    expect(u, "encoder.conv_out.bias", {zc});
    const int qc = cfg->n_embed == 0 ? 2 * cfg->embed_dim : cfg->embed_dim;  // LD/models/autoencoder.py:356 / :40
    expect(u, "quant_conv.weight", {qc, zc, 1, 1});
    expect(u, "quant_conv.bias", {qc});
    if (cfg->n_embed > 0) expect(u, "quantize.embedding.weight", {cfg->n_embed, cfg->embed_dim});
    *out = d.release();
    return 0;
}

void dm_encoder_destroy(dm_encoder* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->holder.ws) (void)hipFree(d->holder.ws);
    d->holder.ws = nullptr;
    delete d;
}

int dm_encoder_set_param(dm_encoder* d, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    DM_REQUIRE(d, "null handle");
    DM_REQUIRE(!d->finalized, "set_param after finalize");
    return dm_unet_set_param(&d->holder, name, data_host, shape, ndim);
}

int dm_encoder_missing_params(dm_encoder* d) { return d ? dm_unet_missing_params(&d->holder) : -1; }

int dm_encoder_finalize(dm_encoder* d) {
    DM_REQUIRE(d, "null handle");
    DM_REQUIRE(!d->finalized, "already finalized");
    if (dm_encoder_missing_params(d) != 0) return 1;
    DM_CHECK_HIP(hipSetDevice(d->device));
    const dm_encoder_cfg& cfg = d->cfg;
    dm_unet* u = &d->holder;
    if (vconv(u, d->conv_in, "encoder.conv_in", cfg.ch, cfg.in_channels, 3, 1, false)) return 1;
    int curr_res = cfg.resolution, block_in = cfg.ch;
    d->levels.resize(cfg.n_levels);
    for (int lvl = 0; lvl < cfg.n_levels; ++lvl) {
        block_in = cfg.ch * (lvl == 0 ? 1 : cfg.ch_mult[lvl - 1]);
        const int block_out = cfg.ch * cfg.ch_mult[lvl];
        bool attn = false;
        for (int a = 0; a < cfg.n_attn_res; ++a) attn = attn || cfg.attn_resolutions[a] == curr_res;
        const std::string p = "encoder.down." + std::to_string(lvl);
        VaeLevel& L = d->levels[lvl];
        L.blocks.resize(cfg.num_res_blocks);
        if (attn) L.attns.resize(cfg.num_res_blocks);
        for (int b = 0; b < cfg.num_res_blocks; ++b) {
            if (vbuild_res(u, L.blocks[b], p + ".block." + std::to_string(b), block_in, block_out)) return 1;
            block_in = block_out;
            if (attn && vbuild_attn(u, L.attns[b], p + ".attn." + std::to_string(b), block_in)) return 1;
        }
        L.has_up = lvl != cfg.n_levels - 1;
        if (L.has_up) {
            const std::string q = p + ".downsample.conv";
            if (make_conv(u, L.up, q + ".weight", q + ".bias", block_in, block_in, 0, 3, 3, /*stride=*/2, /*pad=*/0, false,
                          /*pad_hi=*/1))
                return 1;
            curr_res /= 2;
        }
    }
    if (vbuild_res(u, d->mid1, "encoder.mid.block_1", block_in, block_in)) return 1;
    if (vbuild_attn(u, d->mid_attn, "encoder.mid.attn_1", block_in)) return 1;
    if (vbuild_res(u, d->mid2, "encoder.mid.block_2", block_in, block_in)) return 1;
    d->block_in_final = block_in;
    if (up1(u, "encoder.norm_out.weight", &d->now) || up1(u, "encoder.norm_out.bias", &d->nob)) return 1;
    const int zc = cfg.double_z ? 2 * cfg.z_channels : cfg.z_channels;
    if (vconv(u, d->conv_out, "encoder.conv_out", zc, block_in, 3, 1, false)) return 1;
    if (vconv(u, d->quant_conv, "quant_conv", d->kl() ? 2 * cfg.embed_dim : cfg.embed_dim, zc, 1, 0, false)) return 1;
    if (!d->kl()) {
        const HostTensor& cb = P(u, "quantize.embedding.weight");
        const std::vector<float> sq = code_sq_host(cb.data.data(), cfg.n_embed, cfg.embed_dim);
        const float zero = 0.f;
        if (u->own.upload(cb.data.data(), cb.data.size(), &d->codebook) || u->own.upload(sq.data(), sq.size(), &d->code_sq) ||
            u->own.upload(&zero, 1, &d->bad_index))
            return 1;
    }
    for (auto& kv : u->params) std::vector<float>().swap(kv.second.data);
    d->finalized = true;
    return 0;
}

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
    Arena dry;
    dry.dry = true;
    if (encoder_forward_impl(d, dry, x, zq, pre_quant, indices, B, H, W, s)) return 1;
    if (ensure_workspace(&d->holder, dry.off)) return 1;
    Arena A;
    A.base = d->holder.ws;
    A.cap = d->holder.ws_cap;
    return encoder_forward_impl(d, A, x, zq, pre_quant, indices, B, H, W, s);
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
    Arena dry;
    dry.dry = true;
    if (encoder_forward_kl_impl(d, dry, x, moments_nchw, z, kl, eps, seed, draw, element_offset, sample, B, H, W, s)) return 1;
    if (ensure_workspace(&d->holder, dry.off)) return 1;
    Arena A;
    A.base = d->holder.ws;
    A.cap = d->holder.ws_cap;
    return encoder_forward_kl_impl(d, A, x, moments_nchw, z, kl, eps, seed, draw, element_offset, sample, B, H, W, s);
}

int dm_encoder_quantize(dm_encoder* d, const float* h_nchw, float* zq, int32_t* indices, int B, int h, int w, void* stream) {
    DM_REQUIRE(d && h_nchw && zq, "null argument");
    DM_REQUIRE(d->finalized, "dm_encoder_finalize has not been called");
    DM_REQUIRE(!d->kl(), "this handle has no codebook (n_embed == 0)");
    DM_REQUIRE(B > 0 && h > 0 && w > 0, "empty input");
    DM_CHECK_HIP(hipSetDevice(d->device));
    return launch_vq_nearest(h_nchw, d->codebook, d->code_sq, zq, indices, (int64_t)B * h * w, d->cfg.embed_dim,
                             d->cfg.n_embed, h * w, static_cast<hipStream_t>(stream), /*in_nchw=*/true);
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
    return embed_code_verdict(launch_embed_code(indices, 8, d->codebook, out, bad, (int64_t)B * h * w, d->cfg.embed_dim,
                                                d->cfg.n_embed, h * w, s), bad, s);
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

}  // namespace dm

extern "C" {

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
    int rc = launch_vq_nearest(z_rows, codebook, e2, zq_nchw, indices, pixels, E, n_embed, hw, s);
    return finish_vae_op(rc, s, e2);
}

int dm_op_vq_nearest_nchw(const float* z_nchw, const float* codebook, float* zq_nchw, int32_t* indices, int64_t pixels, int E,
                          int n_embed, int hw, void* stream) {
    DM_REQUIRE(z_nchw && codebook && zq_nchw, "null argument");
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
    int rc = launch_vq_nearest(z_nchw, codebook, e2, zq_nchw, indices, pixels, E, n_embed, hw, s, /*in_nchw=*/true);
    return finish_vae_op(rc, s, e2);
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
