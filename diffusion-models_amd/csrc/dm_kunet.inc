// KarrasUnet, the EDM2 magnitude-preserving U-Net (Karras et al., arXiv 2312.02696, config G; DD/karras_unet.py:374-595), as a
// second body behind the dm_unet handle: creation, the host-side pack, the forward walk and the single-operator entry
// points (dm_op_kunet_*).  Included by dm_api.hip after dm_ops.inc; kernels in karras.hip.
//
// The network has no bias, no learned norm and no constant that is not linear, so the pack folds everything into weights, on
// the host, in double:
//   * forced weight normalisation: every row w / max(||w||, 1e-4) * sqrt(numel) / sqrt(fan_in) (:91-95, :121, :142); numel and
//     fan_in differ for input_block alone, whose row counts the ones channel and whose fan_in does not (:107, :111);
//   * MPSiLU's 1 / 0.596 goes into the convolution (or Linear) that reads the activation;
//   * MPAdd(t): out = a x + b res with a = (1 - t) / den, b = t / den, den = sqrt((1 - t)^2 + t^2).  a goes into the convolution
//     that produces x (block2, to_out), b into res_conv where it is a convolution, else into the pass that writes the residual
//     operand (kunet_pixelnorm, kunet_bilinear_up2, kunet_act): EPI_RESIDUAL is then the whole mp_add;
//   * MPCat(t) of the skip: ca = C (1 - t) / sqrt(Na), cb = C t / sqrt(Nb), C = sqrt((Na + Nb) / ((1 - t)^2 + t^2)).  res_conv
//     reads the raw pair as a two-source convolution whose input-channel groups carry ca and cb; kunet_act multiplies by
//     them in front of the SiLU;
//   * Gain: output_block.1.gain into the output convolution, every to_emb.1.gain into its rows of the concatenated to_emb
//     matrix, whose output rows are laid out as EPI_SCALE_SHIFT reads them (dout scales, then dout zero shifts);
//   * mem_kv: pixel-normed along dh here, it does not depend on the input.
// The convolution kernels are those of the image U-Net, unchanged: block1 runs with EPI_SCALE_SHIFT | EPI_SILU (no norm),
// block2 / to_out with EPI_RESIDUAL.
//
// The same list is restated in torch by tests/karras_oracle.py (fold / forward), which the host tests pin against the
// reference's fp64 outputs.

namespace dm {

static const double kMpSiluGain = 1.0 / 0.596;
static const int kNumMemKv = 4;

struct KBlock {
    std::string prefix;
    bool decoder = false, down = false, up = false, skip = false, attn = false;
    int din = 0, dout = 0;
    int na = 0, nb = 0;  // skip decoders: widths of x and of the skip (na + nb == din)
    int ss_off = 0, heads = 0;
    float res_scale = 0.f, attn_res_scale = 0.f, ca = 1.f, cb = 1.f;
    ConvLayer down_conv, c1, c2, res, qkv, out;
    float* mem_kv = nullptr;  // (2, heads, 4, dh), normalised
    bool res_conv() const { return decoder && din != dout; }
};

// the conditioning head: Fourier features [| labels] -> emb_w -> silu -> ss_w
struct KHead {
    int half = 0, n_labels = 0, emb_dim = 0, ss_total = 0;
    float *fw = nullptr, *emb_w = nullptr, *ss_w = nullptr;
    int in_dim() const { return 2 * half + n_labels; }
};

struct KUnet {
    dm_kunet_cfg cfg{};
    std::vector<KBlock> downs, mids, ups;
    ConvLayer in_conv, out_conv;
    KHead head;
    float* labels = nullptr;  // (labels_cap, num_classes) device rows the head reads (dm_kunet_set_class_labels)
    int labels_cap = 0, labels_B = 0;
};

static int kunet_image_size(const dm_unet* u) { return u->kunet->cfg.image_size; }

void kunet_free(dm_unet* u) {
    if (!u->kunet) return;
    if (u->kunet->labels) (void)hipFree(u->kunet->labels);
    delete u->kunet;
    u->kunet = nullptr;
}

// ---- constants and the host-side folding ------------------------------------------------------------------------------------------
static void mp_add_consts(double t, double* a, double* b) {
    const double den = std::sqrt((1 - t) * (1 - t) + t * t);
    *a = (1 - t) / den;
    *b = t / den;
}
static void mp_cat_consts(double t, int na, int nb, double* ca, double* cb) {
    const double c = std::sqrt((na + nb) / ((1 - t) * (1 - t) + t * t));
    *ca = c * (1 - t) / std::sqrt((double)na);
    *cb = c * t / std::sqrt((double)nb);
}
static int kunet_heads(int dim_out, int dh) { return std::max((dim_out + dh - 1) / dh, 2); }

// normalize_weight(w, 1e-4) / sqrt(fan_in) of a (rows, ...) parameter, times `scale`; fan_in == 0: the row's element count
static std::vector<double> knorm_rows(const HostTensor& t, double scale = 1.0, int fan_in = 0) {
    const size_t rows = (size_t)t.shape[0], per = t.numel() / rows;
    std::vector<double> w(t.numel());
    const double f = std::sqrt((double)per) / std::sqrt((double)(fan_in ? fan_in : (int)per)) * scale;
    for (size_t r = 0; r < rows; ++r) {
        double ss = 0.0;
        for (size_t i = 0; i < per; ++i) ss += (double)t.data[r * per + i] * (double)t.data[r * per + i];
        const double d = std::max(std::sqrt(ss), 1e-4);
        for (size_t i = 0; i < per; ++i) w[r * per + i] = (double)t.data[r * per + i] / d * f;
    }
    return w;
}
static std::vector<float> to_f32(const std::vector<double>& w) { return std::vector<float>(w.begin(), w.end()); }

// a bias-less K x K / stride 1 / same-padding convolution of the handle from folded weights
static int make_kconv(dm_unet* u, ConvLayer& L, const std::vector<double>& w, int Cout, int C0, int C1, int K) {
    L.src = PackSrc();
    const std::vector<float> wf = to_f32(w);
    DM_REQUIRE(wf.size() == (size_t)Cout * (C0 + C1) * K * K, "KarrasUnet: weight size");
    return make_conv(u->own, L, wf.data(), nullptr, Cout, C0, C1, K, K, 1, K / 2, false);
}

// ---- structure ------------------------------------------------------------------------------------------------------------------------
// The module lists in forward order, built as DD/karras_unet.py:461-513 builds them (`ups` is filled by prepending).
static void kunet_structure(KUnet& K) {
    const dm_kunet_cfg& cfg = K.cfg;
    const int dh = cfg.attn_dim_head;
    auto in_attn_res = [&](int res) {
        for (int i = 0; i < cfg.n_attn_res; ++i)
            if (cfg.attn_res[i] == res) return true;
        return false;
    };
    auto block = [&](bool decoder, int din, int dout, bool attn, bool down, bool up, bool skip) {
        KBlock b;
        b.decoder = decoder; b.din = din; b.dout = dout; b.attn = attn; b.down = down; b.up = up; b.skip = skip;
        if (skip) { b.na = din - dout; b.nb = dout; }
        if (attn) b.heads = kunet_heads(dout, dh);
        return b;
    };
    std::vector<KBlock> downs, ups;
    int curr_dim = cfg.dim, curr_res = cfg.image_size;
    ups.insert(ups.begin(), block(true, 2 * cfg.dim, cfg.dim, false, false, false, true));
    for (int i = 0; i < cfg.num_blocks_per_stage; ++i) {
        downs.push_back(block(false, curr_dim, curr_dim, false, false, false, false));
        ups.insert(ups.begin(), block(true, 2 * curr_dim, curr_dim, false, false, false, true));
    }
    for (int d = 0; d < cfg.num_downsamples; ++d) {
        const int dim_out = std::min(cfg.dim_max, 2 * curr_dim);
        const KBlock upsample = block(true, dim_out, curr_dim, in_attn_res(curr_res), false, true, false);
        curr_res /= 2;
        const bool has_attn = in_attn_res(curr_res);
        downs.push_back(block(false, curr_dim, dim_out, has_attn, true, false, false));
        ups.insert(ups.begin(), upsample);
        ups.insert(ups.begin(), block(true, 2 * dim_out, dim_out, has_attn, false, false, true));
        for (int i = 0; i < cfg.num_blocks_per_stage; ++i) {
            downs.push_back(block(false, dim_out, dim_out, has_attn, false, false, false));
            ups.insert(ups.begin(), block(true, 2 * dim_out, dim_out, has_attn, false, false, true));
        }
        curr_dim = dim_out;
    }
    const bool mid_attn = in_attn_res(curr_res);
    K.downs = downs;
    K.ups = ups;
    K.mids = {block(true, curr_dim, curr_dim, mid_attn, false, false, false), block(true, curr_dim, curr_dim, mid_attn, false, false, false)};
    int ss_off = 0;
    auto name = [&](std::vector<KBlock>& v, const char* list) {
        for (size_t i = 0; i < v.size(); ++i) {
            v[i].prefix = idx(list, (int)i);
            v[i].ss_off = ss_off;
            ss_off += 2 * v[i].dout;
        }
    };
    name(K.downs, "downs");
    name(K.mids, "mids");
    name(K.ups, "ups");
    K.head.half = cfg.fourier_dim / 2;
    K.head.n_labels = cfg.num_classes;
    K.head.emb_dim = 4 * cfg.dim;
    K.head.ss_total = ss_off;
}

static void expect_kblock(dm_unet* u, const KBlock& b, int emb_dim, int dh) {
    const std::string& p = b.prefix;
    if (b.down) expect(u, p + ".downsample_conv.weight", {b.dout, b.din, 1, 1});
    expect(u, p + ".to_emb.0.weight", {b.dout, emb_dim});
    expect(u, p + ".to_emb.1.gain", {});
    expect(u, p + ".block1.1.weight", {b.dout, b.down ? b.dout : b.din, 3, 3});
    expect(u, p + ".block2.2.weight", {b.dout, b.dout, 3, 3});
    if (b.res_conv()) expect(u, p + ".res_conv.weight", {b.dout, b.din, 1, 1});
    if (b.attn) {
        expect(u, p + ".attn.mem_kv", {2, b.heads, kNumMemKv, dh});
        expect(u, p + ".attn.to_qkv.weight", {3 * b.heads * dh, b.dout, 1, 1});
        expect(u, p + ".attn.to_out.weight", {b.dout, b.heads * dh, 1, 1});
    }
}

// ---- the pack -------------------------------------------------------------------------------------------------------------------------
static int build_kblock(dm_unet* u, KBlock& b, const dm_kunet_cfg& cfg) {
    return weight_group(u, b.prefix, [&]() -> int {
        const std::string& p = b.prefix;
        const int dh = cfg.attn_dim_head;
        double a, r;
        mp_add_consts(cfg.resnet_mp_add_t, &a, &r);
        b.res_scale = (float)r;
        if (b.down && make_kconv(u, b.down_conv, knorm_rows(P(u, p + ".downsample_conv.weight")), b.dout, b.din, 0, 1)) return 1;
        if (make_kconv(u, b.c1, knorm_rows(P(u, p + ".block1.1.weight"), kMpSiluGain), b.dout, b.down ? b.dout : b.din, 0, 3)) return 1;
        if (make_kconv(u, b.c2, knorm_rows(P(u, p + ".block2.2.weight"), kMpSiluGain * a), b.dout, b.dout, 0, 3)) return 1;
        double ca = 1.0, cb = 1.0;
        if (b.skip) mp_cat_consts(cfg.mp_cat_t, b.na, b.nb, &ca, &cb);
        b.ca = (float)ca;
        b.cb = (float)cb;
        if (b.res_conv()) {
            std::vector<double> w = knorm_rows(P(u, p + ".res_conv.weight"), r);
            if (b.skip)
                for (int o = 0; o < b.dout; ++o)
                    for (int i = 0; i < b.din; ++i) w[(size_t)o * b.din + i] *= i < b.na ? ca : cb;
            if (make_kconv(u, b.res, w, b.dout, b.skip ? b.na : b.din, b.skip ? b.nb : 0, 1)) return 1;
        }
        if (b.attn) {
            double aa, ar;
            mp_add_consts(cfg.attn_res_mp_add_t, &aa, &ar);
            b.attn_res_scale = (float)ar;
            const int hidden = b.heads * dh;
            if (make_kconv(u, b.qkv, knorm_rows(P(u, p + ".attn.to_qkv.weight")), 3 * hidden, b.dout, 0, 1)) return 1;
            if (make_kconv(u, b.out, knorm_rows(P(u, p + ".attn.to_out.weight"), aa), b.dout, hidden, 0, 1)) return 1;
            // PixelNorm(dim = -1) of the memory rows: x / max(||x||, 1e-4) * sqrt(dh)
            const HostTensor& m = P(u, p + ".attn.mem_kv");
            std::vector<float> mn(m.numel());
            for (size_t row = 0; row < m.numel() / dh; ++row) {
                double ss = 0.0;
                for (int i = 0; i < dh; ++i) ss += (double)m.data[row * dh + i] * (double)m.data[row * dh + i];
                const double d = std::max(std::sqrt(ss), 1e-4);
                for (int i = 0; i < dh; ++i) mn[row * dh + i] = (float)((double)m.data[row * dh + i] / d * std::sqrt((double)dh));
            }
            if (u->own.upload(mn.data(), mn.size(), &b.mem_kv)) return 1;
        }
        return 0;
    });
}

// The head's three buffers from host tensors.  blocks: every Encoder / Decoder in ss_off order.
static int build_khead(DeviceOwner& own, KHead& h, const HostTensor& fourier_w, const HostTensor& time_w, const HostTensor* class_w,
                       double mp_add_emb_t, const std::vector<std::pair<const HostTensor*, double>>& to_emb /* weight, gain */) {
    std::vector<double> wt = knorm_rows(time_w);
    const int E = h.emb_dim, F = 2 * h.half, NC = h.n_labels, I = F + NC;
    std::vector<float> emb((size_t)E * I);
    double a = 1.0, r = 0.0;
    std::vector<double> wc;
    if (class_w) {
        mp_add_consts(mp_add_emb_t, &a, &r);
        wc = knorm_rows(*class_w);
    }
    for (int o = 0; o < E; ++o) {
        for (int i = 0; i < F; ++i) emb[(size_t)o * I + i] = (float)(wt[(size_t)o * F + i] * a);
        for (int i = 0; i < NC; ++i) emb[(size_t)o * I + F + i] = (float)(wc[(size_t)o * NC + i] * r);
    }
    std::vector<float> ss((size_t)h.ss_total * E, 0.f);  // per block: dout rows of gain * w / 0.596, then dout zero rows (the shift)
    size_t row = 0;
    for (auto& te : to_emb) {
        const std::vector<double> w = knorm_rows(*te.first, te.second * kMpSiluGain);
        const size_t dout = (size_t)te.first->shape[0];
        for (size_t i = 0; i < dout * E; ++i) ss[row * E + i] = (float)w[i];
        row += 2 * dout;
    }
    DM_REQUIRE(row == (size_t)h.ss_total, "KarrasUnet: to_emb rows");
    return own.upload(fourier_w.data.data(), fourier_w.data.size(), &h.fw) || own.upload(emb.data(), emb.size(), &h.emb_w) ||
           own.upload(ss.data(), ss.size(), &h.ss_w);
}

static int kunet_build_all(dm_unet* u) {
    KUnet& K = *u->kunet;
    const dm_kunet_cfg& cfg = K.cfg;
    u->own.rec = nullptr;  // no device-side re-pack recipes: the handle does not train
    if (weight_group(u, "input_block", [&]() -> int {
            return make_kconv(u, K.in_conv, knorm_rows(P(u, "input_block.weight"), 1.0, cfg.input_channels * 9), cfg.dim,
                              cfg.input_channels + 1, 0, 3);
        }))
        return 1;
    if (weight_group(u, "output_block", [&]() -> int {
            const double gain = P(u, "output_block.1.gain").data[0];
            return make_kconv(u, K.out_conv, knorm_rows(P(u, "output_block.0.weight"), gain), cfg.channels, cfg.dim, 0, 3);
        }))
        return 1;
    std::vector<KBlock*> blocks;
    for (auto* v : {&K.downs, &K.mids, &K.ups})
        for (KBlock& b : *v) blocks.push_back(&b);
    for (KBlock* b : blocks)
        if (build_kblock(u, *b, cfg)) return 1;
    // the head reads parameters of every block: rebuilt when any of them changed
    bool dirty = P(u, "to_time_emb.0.weights").dirty || P(u, "to_time_emb.1.weight").dirty ||
                 (cfg.num_classes > 0 && P(u, "to_class_emb.weight").dirty);
    std::vector<std::pair<const HostTensor*, double>> to_emb;
    for (KBlock* b : blocks) {
        const HostTensor &w = P(u, b->prefix + ".to_emb.0.weight"), &g = P(u, b->prefix + ".to_emb.1.gain");
        dirty = dirty || w.dirty || g.dirty;
        to_emb.emplace_back(&w, (double)g.data[0]);
    }
    if (u->own.refreshing && !dirty) {
        u->own.cursor += 3;
        return 0;
    }
    return build_khead(u->own, K.head, P(u, "to_time_emb.0.weights"), P(u, "to_time_emb.1.weight"),
                       cfg.num_classes > 0 ? &P(u, "to_class_emb.weight") : nullptr, cfg.mp_add_emb_t, to_emb);
}

// ---- the walk -------------------------------------------------------------------------------------------------------------------------
// The head: (Bt, ss_total) scale / shift rows, Bt = 1 when the whole batch shares the time and there are no labels.  *ss stays
// allocated until the walk ends.
static int khead_forward(const KHead& h, Arena& A, const float* tf, int tf_stride, const SamplerState* step_dev, const float* labels,
                         int B, hipStream_t s, float** ss, int* Bt) {
    const int R = *Bt = (step_dev && h.n_labels == 0) ? 1 : B;
    float* e0 = A.alloc((size_t)R * h.in_dim());
    float* emb = A.alloc((size_t)R * h.emb_dim);
    *ss = A.alloc((size_t)R * h.ss_total);
    if (!A.dry) {
        if (launch_kunet_fourier(tf, tf_stride, step_dev, h.fw, labels, h.n_labels, e0, R, h.half, s)) return 1;
        if (launch_linear_rows(e0, h.in_dim(), h.emb_w, nullptr, emb, h.emb_dim, R, h.in_dim(), h.emb_dim, 0, 0, s)) return 1;
        if (launch_linear_rows(emb, h.emb_dim, h.ss_w, nullptr, *ss, h.ss_total, R, h.emb_dim, h.ss_total, 1, 0, s)) return 1;
    }
    A.release(e0);
    A.release(emb);
    return 0;
}

// Attention (:329-369) + its MPAdd: to_qkv, the q / k / v norm, the core with the four memory rows, to_out + b x
static int run_kattn(Ctx& c, const KBlock& b, const float* x, int H, int W, int dh, float** out) {
    const int n = H * W, hidden = b.heads * dh;
    const size_t rows = (size_t)c.B * n;
    float* qkv = c.A->alloc(rows * 3 * hidden);
    float* xs = c.A->alloc(rows * b.dout);
    if (run_conv(c, b.qkv, x, nullptr, H, W, qkv, 0, nullptr, nullptr, nullptr)) return 1;
    if (!c.dry()) {
        if (launch_kunet_act(x, b.dout, 1.f, nullptr, 0, 1.f, nullptr, xs, b.attn_res_scale, (int64_t)rows, c.s)) return 1;
        if (launch_kunet_qkv_norm(qkv, (int64_t)rows, b.heads, dh, c.s)) return 1;
    }
    float* o = c.A->alloc(rows * hidden);
    if (!c.dry() && launch_attention_core(qkv, 3 * hidden, qkv + hidden, qkv + 2 * hidden, 3 * hidden, b.mem_kv,
                                          b.mem_kv + (size_t)b.heads * kNumMemKv * dh, kNumMemKv, o, hidden, c.B, n, n, b.heads, dh,
                                          1.0f / sqrtf((float)dh), c.s))
        return 1;
    c.A->release(qkv);
    float* y = c.A->alloc(rows * b.dout);
    if (run_conv(c, b.out, o, nullptr, H, W, y, EPI_RESIDUAL, nullptr, nullptr, xs)) return 1;
    c.A->release(o);
    c.A->release(xs);
    *out = y;
    return 0;
}

// block1 (with the embedding's scale and the SiLU of block2 in its epilogue), block2 + residual, attention: the tail every
// Encoder and Decoder shares.  act and res are released here.
static int run_kblock_tail(Ctx& c, const KBlock& b, float* act, float* res, int H, int W, int dh, float** out) {
    const size_t n = (size_t)c.B * H * W * b.dout;
    float* h1 = c.A->alloc(n);
    if (run_conv(c, b.c1, act, nullptr, H, W, h1, EPI_SCALE_SHIFT | EPI_SILU, nullptr, c.ss + b.ss_off, nullptr)) return 1;
    c.A->release(act);
    float* y = c.A->alloc(n);
    if (run_conv(c, b.c2, h1, nullptr, H, W, y, EPI_RESIDUAL, nullptr, nullptr, res)) return 1;
    c.A->release(h1);
    c.A->release(res);
    if (b.attn) {
        float* ya = nullptr;
        if (run_kattn(c, b, y, H, W, dh, &ya)) return 1;
        c.A->release(y);
        y = ya;
    }
    *out = y;
    return 0;
}

// Encoder.forward (:219-246).  (H, W): the input's size, updated to the output's.
static int run_kencoder(Ctx& c, const KBlock& b, const float* x, int* H, int* W, int dh, float** out) {
    float* xd = nullptr;
    if (b.down) {
        const int h2 = *H / 2, w2 = *W / 2;
        float* pooled = c.A->alloc((size_t)c.B * h2 * w2 * b.din);
        if (!c.dry() && launch_kunet_avgpool2(x, pooled, c.B, *H, *W, b.din, c.s)) return 1;
        *H = h2;
        *W = w2;
        xd = c.A->alloc((size_t)c.B * h2 * w2 * b.dout);
        if (run_conv(c, b.down_conv, pooled, nullptr, h2, w2, xd, 0, nullptr, nullptr, nullptr)) return 1;
        c.A->release(pooled);
        x = xd;
    }
    const size_t n = (size_t)c.B * *H * *W * b.dout;
    float* res = c.A->alloc(n);
    float* act = c.A->alloc(n);
    if (!c.dry() && launch_kunet_pixelnorm(x, res, act, (int64_t)c.B * *H * *W, b.dout, b.res_scale, c.s)) return 1;
    if (xd) c.A->release(xd);
    return run_kblock_tail(c, b, act, res, *H, *W, dh, out);
}

// Decoder.forward (:301-325); skip: the tensor MPCat concatenates behind x (nullptr for the mids and the upsampling decoders)
static int run_kdecoder(Ctx& c, const KBlock& b, const float* x, const float* skip, int* H, int* W, int dh, float** out) {
    float *act = nullptr, *res = nullptr;
    if (b.up) {
        const int h = *H, w = *W;
        *H = 2 * h;
        *W = 2 * w;
        const size_t n_in = (size_t)c.B * *H * *W * b.din;
        act = c.A->alloc(n_in);
        if (b.res_conv()) {
            float* xup = c.A->alloc(n_in);
            if (!c.dry() && launch_kunet_bilinear_up2(x, xup, act, nullptr, c.B, h, w, b.din, 0.f, c.s)) return 1;
            res = c.A->alloc((size_t)c.B * *H * *W * b.dout);
            if (run_conv(c, b.res, xup, nullptr, *H, *W, res, 0, nullptr, nullptr, nullptr)) return 1;
            c.A->release(xup);
        } else {
            res = c.A->alloc(n_in);
            if (!c.dry() && launch_kunet_bilinear_up2(x, nullptr, act, res, c.B, h, w, b.din, b.res_scale, c.s)) return 1;
        }
    } else {
        const int64_t rows = (int64_t)c.B * *H * *W;
        DM_REQUIRE(b.skip == (skip != nullptr), "KarrasUnet: a skip decoder without its skip");
        act = c.A->alloc((size_t)rows * b.din);
        res = c.A->alloc((size_t)rows * b.dout);
        float* copy = b.res_conv() ? nullptr : res;  // the identity res_conv: res = x * t / den
        if (!c.dry() && launch_kunet_act(x, b.skip ? b.na : b.din, b.ca, skip, b.skip ? b.nb : 0, b.cb, act, copy, b.res_scale, rows, c.s))
            return 1;
        if (b.res_conv() && run_conv(c, b.res, x, skip, *H, *W, res, 0, nullptr, nullptr, nullptr)) return 1;
    }
    return run_kblock_tail(c, b, act, res, *H, *W, dh, out);
}

// KarrasUnet.forward (:521-595).  x_nchw (B, input_channels, H, W), out_nchw (B, channels, H, W); the time is real-valued:
// tf[b], or with step_dev the entry tf[step * tf_stride] of the EDM step table for the whole batch.
static int kunet_forward_impl(dm_unet* u, Arena& A, const float* x_nchw, const SamplerState* step_dev, float* out_nchw, int B,
                              int H, int W, hipStream_t s, const float* tf, int tf_stride) {
    KUnet& K = *u->kunet;
    const dm_kunet_cfg& cfg = K.cfg;
    DM_REQUIRE(tf, "a KarrasUnet handle takes a real-valued time: dm_unet_forward_ft and dm_sample_edm");
    DM_REQUIRE(H == cfg.image_size && W == cfg.image_size, "KarrasUnet: the input must be image_size x image_size");
    DM_REQUIRE(cfg.num_classes == 0 || K.labels_B == B,
               "KarrasUnet with num_classes: dm_kunet_set_class_labels must give the labels of this batch first");
    const int dh = cfg.attn_dim_head;
    float* ss = nullptr;
    int Bt = 0;
    if (khead_forward(K.head, A, tf, tf_stride, step_dev, K.labels, B, s, &ss, &Bt)) return 1;
    Ctx c{u, &A, s, B, A.dry ? reinterpret_cast<const float*>(16) : ss, Bt == 1 ? 0 : K.head.ss_total};

    const int Cin = cfg.input_channels;
    float* xin = A.alloc((size_t)B * H * W * (Cin + 1));
    if (!A.dry && launch_kunet_input(x_nchw, xin, B, Cin, H * W, s)) return 1;
    float* x = A.alloc((size_t)B * H * W * cfg.dim);
    if (run_conv(c, K.in_conv, xin, nullptr, H, W, x, 0, nullptr, nullptr, nullptr)) return 1;
    A.release(xin);

    std::vector<float*> skips{x};
    auto done_with = [&](float* p) {  // an encoder output lives on as a skip until its decoder has read it
        if (std::find(skips.begin(), skips.end(), p) == skips.end()) A.release(p);
    };
    int h = H, w = W;
    for (const KBlock& b : K.downs) {
        float* y = nullptr;
        if (run_kencoder(c, b, x, &h, &w, dh, &y)) return 1;
        skips.push_back(y);
        x = y;
    }
    for (const KBlock& b : K.mids) {
        float* y = nullptr;
        if (run_kdecoder(c, b, x, nullptr, &h, &w, dh, &y)) return 1;
        done_with(x);
        x = y;
    }
    for (const KBlock& b : K.ups) {
        float* sk = nullptr;
        if (b.skip) {
            DM_REQUIRE(!skips.empty(), "KarrasUnet: skip stack underflow");
            sk = skips.back();
            skips.pop_back();
        }
        float* y = nullptr;
        if (run_kdecoder(c, b, x, sk, &h, &w, dh, &y)) return 1;
        done_with(x);
        if (sk && sk != x) A.release(sk);
        x = y;
    }
    DM_REQUIRE(skips.empty() && h == H && w == W, "KarrasUnet: the walk did not return to the input size");
    if (run_conv(c, K.out_conv, x, nullptr, H, W, out_nchw, 0, nullptr, nullptr, nullptr, false, /*out_nchw=*/true)) return 1;
    A.release(x);
    A.release(ss);
    return 0;
}

static int kunet_cfg_ok(const dm_kunet_cfg* cfg) {
    DM_REQUIRE(cfg->image_size > 0 && cfg->dim > 0 && cfg->dim % 4 == 0 && cfg->dim_max >= cfg->dim && cfg->dim_max % 4 == 0,
               "KarrasUnet: image_size, dim and dim_max must be positive, dim and dim_max multiples of 4, dim_max >= dim");
    DM_REQUIRE(cfg->channels > 0 && cfg->input_channels >= cfg->channels, "KarrasUnet: channels");
    DM_REQUIRE(cfg->num_classes >= 0, "KarrasUnet: num_classes (0 = none)");
    DM_REQUIRE(cfg->num_downsamples >= 0 && cfg->num_downsamples < DM_MAX_STAGES, "KarrasUnet: num_downsamples out of range");
    DM_REQUIRE(cfg->image_size % (1 << cfg->num_downsamples) == 0, "KarrasUnet: image_size must be divisible by 2^num_downsamples");
    DM_REQUIRE(cfg->num_blocks_per_stage >= 1, "KarrasUnet: num_blocks_per_stage >= 1");
    DM_REQUIRE(cfg->n_attn_res >= 0 && cfg->n_attn_res <= DM_MAX_STAGES, "KarrasUnet: at most DM_MAX_STAGES attention resolutions");
    DM_REQUIRE(cfg->fourier_dim > 0 && cfg->fourier_dim % 2 == 0, "KarrasUnet: fourier_dim must be positive and even");
    DM_REQUIRE(cfg->attn_dim_head == 32 || cfg->attn_dim_head == 64,
               "attn_dim_head: the HIP attention kernels support head widths 32 and 64");
    for (float t : {cfg->mp_cat_t, cfg->mp_add_emb_t, cfg->attn_res_mp_add_t, cfg->resnet_mp_add_t})
        DM_REQUIRE(t >= 0.f && t <= 1.f, "KarrasUnet: the magnitude-preserving t constants lie in [0, 1]");
    return 0;
}

}  // namespace dm

extern "C" {

int dm_kunet_create(const dm_kunet_cfg* cfg, int device, dm_unet** out) {
    DM_REQUIRE(cfg && out, "null argument");
    if (kunet_cfg_ok(cfg)) return 1;
    int ndev = 0;
    DM_CHECK_HIP(hipGetDeviceCount(&ndev));
    DM_REQUIRE(device >= 0 && device < ndev, "no such HIP device");
    DM_CHECK_HIP(hipSetDevice(device));
    auto u = std::make_unique<dm_unet>();
    u->device = device;
    // what the handle-generic code reads of a dm_unet_cfg: an x -> x network with a random Fourier time embedding
    u->cfg.dim = cfg->dim;
    u->cfg.channels = u->cfg.out_dim = cfg->channels;
    u->cfg.input_channels = cfg->input_channels;
    u->cfg.n_stages = cfg->num_downsamples + 1;
    u->cfg.attn_heads = 2;
    u->cfg.attn_dim_head = cfg->attn_dim_head;
    u->cfg.learned_sinusoidal_dim = cfg->fourier_dim;
    u->init_dim = cfg->dim;
    u->out_dim = cfg->channels;
    u->time_dim = 4 * cfg->dim;
    u->heads = 2;
    u->dh = cfg->attn_dim_head;
    u->kunet = new KUnet();
    KUnet& K = *u->kunet;
    K.cfg = *cfg;
    kunet_structure(K);
    dm_unet* p = u.get();
    const int E = K.head.emb_dim;
    expect(p, "input_block.weight", {cfg->dim, cfg->input_channels + 1, 3, 3});
    expect(p, "output_block.0.weight", {cfg->channels, cfg->dim, 3, 3});
    expect(p, "output_block.1.gain", {});
    expect(p, "to_time_emb.0.weights", {cfg->fourier_dim / 2});
    expect(p, "to_time_emb.1.weight", {E, cfg->fourier_dim});
    if (cfg->num_classes > 0) expect(p, "to_class_emb.weight", {E, cfg->num_classes});
    for (auto* v : {&K.downs, &K.ups, &K.mids})  // registration order of the reference: mids last
        for (const KBlock& b : *v) expect_kblock(p, b, E, cfg->attn_dim_head);
    *out = u.release();
    return 0;
}

int dm_kunet_set_class_labels(dm_unet* u, const float* labels_dev, int B) {
    DM_REQUIRE(u && labels_dev && B > 0, "null argument");
    DM_REQUIRE(u->kunet && u->kunet->cfg.num_classes > 0, "dm_kunet_set_class_labels needs a KarrasUnet handle with num_classes");
    KUnet& K = *u->kunet;
    DM_CHECK_HIP(hipSetDevice(u->device));
    DM_CHECK_HIP(hipDeviceSynchronize());  // the previous call may still read the buffer; the caller's rows may still be written
    if (B > K.labels_cap) {
        u->drop_graph();  // the captured step reads the old buffer
        if (K.labels) (void)hipFree(K.labels);
        K.labels = nullptr;
        K.labels_cap = K.labels_B = 0;
        const int cap = std::max(B, 16);
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&K.labels), (size_t)cap * K.cfg.num_classes * sizeof(float)));
        K.labels_cap = cap;
    }
    DM_CHECK_HIP(hipMemcpy(K.labels, labels_dev, (size_t)B * K.cfg.num_classes * sizeof(float), hipMemcpyDeviceToDevice));
    DM_CHECK_HIP(hipDeviceSynchronize());
    K.labels_B = B;
    return 0;
}

// ---- single operators ---------------------------------------------------------------------------------------------------------------
// Tensors are device pointers.  The row passes take NHWC / row tensors as the library holds them; the convolution blocks take
// NCHW and the reference's parameter layouts, packed per call.

int dm_op_kunet_pixelnorm(const float* x, float* res_out, float* act_out, int64_t rows, int C, float res_scale, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_kunet_pixelnorm(x, res_out, act_out, rows, C, res_scale, s)) return 1;
    DM_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int dm_op_kunet_avgpool2(const float* x, float* y, int B, int H, int W, int C, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_kunet_avgpool2(x, y, B, H, W, C, s)) return 1;
    DM_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int dm_op_kunet_bilinear_up2(const float* x, float* up_out, float* act_out, float* res_out, int B, int H, int W, int C,
                             float res_scale, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_kunet_bilinear_up2(x, up_out, act_out, res_out, B, H, W, C, res_scale, s)) return 1;
    DM_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int dm_op_kunet_act(const float* a, int Ca, float ca, const float* b, int Cb, float cb, float* act_out, float* copy_out,
                    float copy_scale, int64_t rows, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_kunet_act(a, Ca, ca, b, Cb, cb, act_out, copy_out, copy_scale, rows, s)) return 1;
    DM_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

// q / k / v norm + the attention core on a raw to_qkv output (B, n, 3 heads dh) and the raw mem_kv parameter
// (2, heads, 4, dh); out (B, n, heads dh)
int dm_op_kunet_attention(const float* qkv, const float* mem_kv, float* out, int B, int n, int heads, int dh, void* stream) {
    DM_REQUIRE(qkv && mem_kv && out && B > 0 && n > 0 && heads > 0, "null argument");
    DM_REQUIRE(dh == 32 || dh == 64, "dim_head: the attention kernels support 32 and 64");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int hidden = heads * dh;
    return run_op(s, [&](Arena& A) -> int {
        float* q = A.alloc((size_t)B * n * 3 * hidden);
        float* m = A.alloc((size_t)2 * heads * kNumMemKv * dh);
        if (A.dry) return 0;
        DM_CHECK_HIP(hipMemcpyAsync(q, qkv, (size_t)B * n * 3 * hidden * sizeof(float), hipMemcpyDeviceToDevice, s));
        // the memory rows through the same row norm (the handle normalises them at pack time, on the host)
        if (launch_kunet_pixelnorm(mem_kv, m, nullptr, (int64_t)2 * heads * kNumMemKv, dh, 1.0f, s)) return 1;
        if (launch_kunet_qkv_norm(q, (int64_t)B * n, heads, dh, s)) return 1;
        return launch_attention_core(q, 3 * hidden, q + hidden, q + 2 * hidden, 3 * hidden, m, m + (size_t)heads * kNumMemKv * dh,
                                     kNumMemKv, out, hidden, B, n, n, heads, dh, 1.0f / sqrtf((float)dh), s);
    });
}

namespace {
// a parameter of a stand-alone operator's dummy handle from a device pointer
int op_param(dm_unet& u, const std::string& name, const float* dev, std::vector<int64_t> shape) {
    HostTensor t;
    t.shape = std::move(shape);
    if (d2h(dev, t.numel(), t.data)) return 1;
    t.set = true;
    u.params[name] = std::move(t);
    return 0;
}
}  // namespace

// The conditioning head.  time (B); labels (B, num_classes) already times sqrt(num_classes), or NULL with num_classes = 0;
// to_emb_w: the to_emb.0.weight matrices of n_blocks blocks one behind the other ((sum dout, 4 dim) rows), dout_host /
// gain_host their widths and gains; out (B, 2 sum dout): per block dout scales, then dout zeros.
int dm_op_kunet_head(const float* time, const float* labels, const float* fourier_w, const float* time_w, const float* class_w,
                     const float* to_emb_w, const int32_t* dout_host, const float* gain_host, int n_blocks, int fourier_dim,
                     int emb_dim, int num_classes, float mp_add_emb_t, float* out, int B, void* stream) {
    DM_REQUIRE(time && fourier_w && time_w && to_emb_w && dout_host && gain_host && out && B > 0 && n_blocks > 0, "null argument");
    DM_REQUIRE((num_classes > 0) == (labels != nullptr) && (num_classes > 0) == (class_w != nullptr),
               "labels, class_w and num_classes come together");
    hipStream_t s = static_cast<hipStream_t>(stream);
    dm_unet dummy;
    KHead h;
    h.half = fourier_dim / 2;
    h.n_labels = num_classes;
    h.emb_dim = emb_dim;
    if (op_param(dummy, "fw", fourier_w, {fourier_dim / 2}) || op_param(dummy, "tw", time_w, {emb_dim, fourier_dim})) return 1;
    if (class_w && op_param(dummy, "cw", class_w, {emb_dim, num_classes})) return 1;
    std::vector<std::pair<const HostTensor*, double>> to_emb;
    size_t row = 0;
    for (int i = 0; i < n_blocks; ++i) {
        const std::string name = "e" + std::to_string(i);
        if (op_param(dummy, name, to_emb_w + row * emb_dim, {dout_host[i], emb_dim})) return 1;
        row += (size_t)dout_host[i];
        h.ss_total += 2 * dout_host[i];
    }
    for (int i = 0; i < n_blocks; ++i) to_emb.emplace_back(&dummy.params.at("e" + std::to_string(i)), (double)gain_host[i]);
    if (build_khead(dummy.own, h, dummy.params.at("fw"), dummy.params.at("tw"), class_w ? &dummy.params.at("cw") : nullptr,
                    mp_add_emb_t, to_emb))
        return 1;
    return run_op(s, [&](Arena& A) -> int {
        float* ss = nullptr;
        int Bt = 0;
        if (khead_forward(h, A, time, 0, nullptr, labels, B, s, &ss, &Bt)) return 1;
        if (!A.dry) DM_CHECK_HIP(hipMemcpyAsync(out, ss, (size_t)B * h.ss_total * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    });
}

// input_block: x (B, C, H, W) NCHW, weight (dim, C + 1, 3, 3) as stored -> out (B, dim, H, W) NCHW
int dm_op_kunet_input_block(const float* x, const float* weight, float* out, int B, int C, int H, int W, int dim, void* stream) {
    DM_REQUIRE(x && weight && out && B > 0 && C > 0 && dim > 0 && dim % 4 == 0, "null argument, or dim is no multiple of 4");
    hipStream_t s = static_cast<hipStream_t>(stream);
    dm_unet dummy;
    init_dummy(dummy, 2, 32);
    if (op_param(dummy, "w", weight, {dim, C + 1, 3, 3})) return 1;
    ConvLayer L;
    if (make_kconv(&dummy, L, knorm_rows(dummy.params.at("w"), 1.0, C * 9), dim, C + 1, 0, 3)) return 1;
    return run_op(s, [&](Arena& A) -> int {
        Ctx c{&dummy, &A, s, B, nullptr, 0};
        float* xin = A.alloc((size_t)B * H * W * (C + 1));
        float* y = A.alloc((size_t)B * H * W * dim);
        if (!A.dry && launch_kunet_input(x, xin, B, C, H * W, s)) return 1;
        if (run_conv(c, L, xin, nullptr, H, W, y, 0, nullptr, nullptr, nullptr)) return 1;
        return A.dry ? 0 : launch_nhwc_to_nchw(y, out, B, dim, H * W, s);
    });
}

// output_block: x (B, dim, H, W) NCHW, weight (channels, dim, 3, 3) as stored, the gain -> out (B, channels, H, W) NCHW
int dm_op_kunet_output_block(const float* x, const float* weight, float gain, float* out, int B, int dim, int H, int W,
                             int channels, void* stream) {
    DM_REQUIRE(x && weight && out && B > 0 && channels > 0 && dim > 0 && dim % 4 == 0, "null argument, or dim is no multiple of 4");
    hipStream_t s = static_cast<hipStream_t>(stream);
    dm_unet dummy;
    init_dummy(dummy, 2, 32);
    if (op_param(dummy, "w", weight, {channels, dim, 3, 3})) return 1;
    ConvLayer L;
    if (make_kconv(&dummy, L, knorm_rows(dummy.params.at("w"), (double)gain), channels, dim, 0, 3)) return 1;
    return run_op(s, [&](Arena& A) -> int {
        int rc = 0;
        Ctx c{&dummy, &A, s, B, nullptr, 0};
        float* a = to_nhwc(A, x, B, dim, H * W, s, &rc);
        if (rc) return 1;
        return run_conv(c, L, a, nullptr, H, W, out, 0, nullptr, nullptr, nullptr, false, /*out_nchw=*/true);
    });
}

// One Encoder or Decoder.  x (B, din or the width of x in front of the skip, H, W) and skip (B, nb, H, W) NCHW; emb_scale
// (B, dout) = gain * to_emb(emb), what the head produces for the block; the weights as stored.  out: (B, dout, Ho, Wo) NCHW
// with Ho = H / 2 (downsample), 2 H (upsample) or H.
int dm_op_kunet_block(const dm_kunet_block_op* a, void* stream) {
    DM_REQUIRE(a && a->x && a->emb_scale && a->w1 && a->w2 && a->out, "null argument");
    DM_REQUIRE(a->dh == 32 || a->dh == 64, "dim_head: the attention kernels support 32 and 64");
    DM_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->din > 0 && a->dout > 0 && a->din % 4 == 0 && a->dout % 4 == 0,
               "empty tensor, or a width that is no multiple of 4");
    DM_REQUIRE(!(a->down && a->decoder) && !(a->up && !a->decoder) && !(a->skip && (!a->decoder || a->up)), "no such block form");
    DM_REQUIRE(!a->down || (a->H % 2 == 0 && a->W % 2 == 0), "a downsampling Encoder needs even H and W");
    hipStream_t s = static_cast<hipStream_t>(stream);
    dm_unet dummy;
    init_dummy(dummy, 2, a->dh);
    dm_kunet_cfg cfg{};
    cfg.attn_dim_head = a->dh;
    cfg.mp_cat_t = a->mp_cat_t;
    cfg.attn_res_mp_add_t = a->attn_res_mp_add_t;
    cfg.resnet_mp_add_t = a->resnet_mp_add_t;
    KBlock b;
    b.prefix = "b";
    b.decoder = a->decoder != 0; b.down = a->down != 0; b.up = a->up != 0; b.skip = a->skip != 0; b.attn = a->attn != 0;
    b.din = a->din; b.dout = a->dout;
    if (b.skip) {
        DM_REQUIRE(a->skip_x && a->skip_channels > 0 && a->skip_channels < a->din && a->skip_channels % 4 == 0, "skip tensor");
        b.nb = a->skip_channels;
        b.na = a->din - b.nb;
    }
    const int c1_in = b.down ? b.dout : b.din;
    if (b.down && (!a->down_w || op_param(dummy, "b.downsample_conv.weight", a->down_w, {b.dout, b.din, 1, 1}))) return 1;
    if (op_param(dummy, "b.block1.1.weight", a->w1, {b.dout, c1_in, 3, 3}) ||
        op_param(dummy, "b.block2.2.weight", a->w2, {b.dout, b.dout, 3, 3}))
        return 1;
    if (b.res_conv()) {
        DM_REQUIRE(a->res_w, "a Decoder with din != dout has a res_conv");
        if (op_param(dummy, "b.res_conv.weight", a->res_w, {b.dout, b.din, 1, 1})) return 1;
    }
    if (b.attn) {
        DM_REQUIRE(a->mem_kv && a->qkv_w && a->out_w, "attention parameters");
        b.heads = kunet_heads(b.dout, a->dh);
        if (op_param(dummy, "b.attn.mem_kv", a->mem_kv, {2, b.heads, kNumMemKv, a->dh}) ||
            op_param(dummy, "b.attn.to_qkv.weight", a->qkv_w, {3 * b.heads * a->dh, b.dout, 1, 1}) ||
            op_param(dummy, "b.attn.to_out.weight", a->out_w, {b.dout, b.heads * a->dh, 1, 1}))
            return 1;
    }
    if (build_kblock(&dummy, b, cfg)) return 1;
    const int B = a->B, H = a->H, W = a->W, xc = b.skip ? b.na : b.din;
    return run_op(s, [&](Arena& A) -> int {
        int rc = 0;
        float* ss = A.alloc((size_t)B * 2 * b.dout);  // [scale | zero shift] rows
        if (!A.dry) {
            DM_CHECK_HIP(hipMemsetAsync(ss, 0, (size_t)B * 2 * b.dout * sizeof(float), s));
            DM_CHECK_HIP(hipMemcpy2DAsync(ss, 2 * b.dout * sizeof(float), a->emb_scale, b.dout * sizeof(float),
                                          b.dout * sizeof(float), B, hipMemcpyDeviceToDevice, s));
        }
        Ctx c{&dummy, &A, s, B, A.dry ? reinterpret_cast<const float*>(16) : ss, 2 * b.dout};
        float* x = to_nhwc(A, a->x, B, xc, H * W, s, &rc);
        float* sk = b.skip ? to_nhwc(A, a->skip_x, B, b.nb, H * W, s, &rc) : nullptr;
        if (rc) return 1;
        int h = H, w = W;
        float* y = nullptr;
        if (b.decoder ? run_kdecoder(c, b, x, sk, &h, &w, a->dh, &y) : run_kencoder(c, b, x, &h, &w, a->dh, &y)) return 1;
        return A.dry ? 0 : launch_nhwc_to_nchw(y, a->out, B, b.dout, h * w, s);
    });
}

}  // extern "C"
