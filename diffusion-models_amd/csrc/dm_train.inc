// Training step of the denoising U-Net (SURVEY.md 8(f) rank 4): DenoisingDiffusion.forward / p_losses
// (DD/denoising_diffusion.py:805-900) and the backward pass autograd derives from it, as explicit HIP launches.
// Textually included at the end of dm_api.hip.
//
// Forward in "tape" mode: the same convolution / attention kernels as the sampling path, but unfused at the points where
// the backward pass needs an intermediate (the convolution output in front of every RMSNorm, the attention projections),
// and nothing is released.  Backward: every convolution's input gradient is a convolution of dY with the 180-degree
// rotated, Cin<->Cout transposed weights -- the forward kernels (Winograd F(4x4) / F(2x2), 1x1 GEMM, direct) run on them
// unchanged; the weight gradient is wgrad_mfma.hip; norms / activations / attention cores / loss are train_kernels.hip and
// attn_bwd.hip.  What does not sit on the input-gradient chain is not launched where the pass reaches it: the weight
// gradients of all layers run as one grouped launch per mode at the end, the split-K sums, the per-image / per-channel
// reductions behind the norm kernels and the bias column sums as table-driven launches (unet_train_backward).
// No autograd, no torch op, no CPU fallback anywhere on this path.
namespace dm {

template <class F>
static int guarded(F f) {  // nothing throws across the C ABI
    try {
        return f();
    } catch (const std::exception& e) {
        set_error(e.what());
        return 1;
    }
}

// what the backward pass needs of one convolution layer
enum ConvBwdKind {
    CB_3X3,    // 3x3 s1 p1 (fwd.up: on a nearest-x2 source)
    CB_1X1,
    CB_DOWN,   // Downsample (2x2 s2)
    CB_INIT7,  // init_conv: 7x7 over the NCHW image, no input-gradient layer
    CB_FINAL,  // final_conv: thin 1x1 to the NCHW output, no input-gradient layer
};
struct ConvBwd {
    ConvBwdKind kind = CB_3X3;
    ConvLayer d0, d1;  // dY -> d(in0), d(in1): rotated / transposed weights through make_conv
    bool has1 = false;
};

// Modes of the weight-gradient kernels (wgrad_mfma.hip).  The values are kernel arguments and the N of the profile rows
// `wgrad m<N>`: they stay as they are.
enum WgradMode { WG_3X3 = 0, WG_1X1 = 1, WG_DOWN = 2, WG_WINO = 3, WG_MODES = 4 };  // WG_WINO: 3x3 in the Winograd domain
// products per weight element and 2x2 output tile (`taps`) and the input channels of one weight row
static void wgrad_dims(WgradMode mode, const ConvLayer& L, int* taps, int* cin_w) {
    static const int kTaps[WG_MODES] = {9, 1, 4, 16};
    *taps = kTaps[mode];
    *cin_w = mode == WG_DOWN ? L.C0 : L.C0 + L.C1;
}

struct TrainState {
    DeviceOwner own;  // dgrad weights
    std::map<const ConvLayer*, ConvBwd> conv;
    float* grad = nullptr;  // one flat buffer, parameters in state-dict order
    size_t grad_floats = 0;
    std::map<std::string, size_t> off;
    // device-resident training loop: master parameters (same offsets as grad), Adam moments, optional EMA copy
    float *param = nullptr, *adam_m = nullptr, *adam_v = nullptr, *ema = nullptr;
    double* norm_ws = nullptr;  // 1024 partial sums of the gradient norm
    float* clip2 = nullptr;     // (total gradient norm, clip coefficient)
    float* pack_tmp = nullptr;  // rotated / transposed weights of the layer being re-packed
    size_t pack_tmp_floats = 0;
    int adam_step = 0;
    float dropout = 0.f;        // nn.Dropout(p) of every Block in training mode
    uint64_t drop_seed = 0;     // Philox key of the masks
    uint64_t drop_call = 0;     // loss / backward calls since the seed was set: every call draws fresh masks
    std::vector<PackOp> ops;    // recipes of the input-gradient convolutions (the forward ones are on the handle)
    // Lazy re-packing: an optimiser step marks every packed convolution weight stale; a buffer is rebuilt from the master
    // parameters right before the first convolution that reads it (only the layouts the current shapes dispatch to are
    // ever rebuilt).  Small raw copies (biases, gains, mem_kv, the time MLP, the concatenated ResnetBlock.mlp) are redone
    // eagerly by ONE scatter-copy kernel driven by a device table.
    std::unordered_map<const float*, std::pair<int, int>> op_of;  // packed buffer -> (0 forward / 1 backward list, index)
    std::vector<char> stale_f, stale_b;
    // Batched re-packing: the buffers the training step asked for since the recipes were indexed (used_*) are rebuilt right
    // after the optimiser step in two grouped launches (sources that need a rotated / transposed copy first, then the
    // packs); only layouts the grouped kernel does not know stay on the lazy path.
    std::vector<char> used_f, used_b;
    int used_version = 0, jobs_version = -1;  // the job tables are rebuilt when a new buffer joins the used set
    std::vector<PackJob> pk_host[2];
    PackJob* pk_dev[2] = {nullptr, nullptr};
    size_t pk_cap[2] = {0, 0};
    int pk_blocks[2] = {0, 0};
    std::vector<std::pair<int, int>> pk_ops;  // (list, index) of the recipes the job tables cover
    float* big_tmp = nullptr;  // rotated / transposed sources of all batched input-gradient layers
    size_t big_tmp_floats = 0;
    struct CopyEntry {
        long long src_off;  // floats into the flat parameter buffer
        float* dst;
        long long n;
    };
    // Device tables of the grouped weight-gradient launches and of the split-K sums behind them, one set per FLUSH of a
    // backward pass (one flush at the end of the pass; one per gradient bucket when data-parallel bucketing is on)
    struct FlushTables {
        WgradParams* wtab_dev[WG_MODES] = {};
        size_t wtab_cap[WG_MODES] = {};
        std::vector<WgradParams> wtab_host[WG_MODES];
        WgradJob* jobs_dev = nullptr;
        size_t jobs_cap = 0;
        std::vector<WgradJob> jobs_host;
    };
    std::vector<FlushTables> flush;
    // Gradient buckets (data-parallel training): the flat buffer is laid out bucket by bucket in the order the backward pass
    // completes them -- the convolution weights of the stages it leaves first come first, everything that only the end of
    // the pass completes (norm gains, biases, the time / ResnetBlock MLPs, the last stages) is the last bucket -- so that a
    // bucket is ONE contiguous span a collective can take while the pass is still running.
    struct Bucket {
        size_t off = 0, n = 0;     // span of the flat buffers (floats)
        int last_phase = 0;        // the bucket is complete when the backward pass has left this phase
        hipEvent_t ready = nullptr;
    };
    std::vector<Bucket> buckets;
    std::set<std::string> conv_weights;  // parameters whose gradient a flush completes (grouped / deferred weight gradients)
    bool bucketed = false;               // flush (and record `ready`) per bucket instead of once at the end of the pass
    RowgradJob* rjobs_dev = nullptr;  // deferred reductions of one backward pass
    size_t rjobs_cap = 0;
    std::vector<RowgradJob> rjobs_host;
    ColsumJob* cjobs_dev = nullptr;
    size_t cjobs_cap = 0;
    std::vector<ColsumJob> cjobs_host;
    float** mlp_rows = nullptr;  // [2][ss_total]: gradient row pointers of the concatenated ResnetBlock.mlp matrix / bias
    CopyEntry* copy_table = nullptr;
    int n_copies = 0;
    long long max_copy = 0;
    char* ws = nullptr;
    size_t ws_cap = 0;
    // per-image device rows of a loss / backward call, grown together (grow_train_rows) to cap_B images.  A handle is armed
    // for integer or float time, never both: a call writes t_dev or tf_dev, and the coefficient rows at the width its own
    // kernels index them with (DM_TRAIN_COEFS, or DM_EDM_COEFS on the float-time paths)
    float* coef_dev = nullptr;    // [B][up to DM_EDM_COEFS]
    int64_t* t_dev = nullptr;     // [B] integer timesteps
    float* tf_dev = nullptr;      // [B] float times: c_noise(sigma_b), log_snr_b
    int32_t* mask_dev = nullptr;  // [B]: the per-image text mask of a masked call (dm_unet_loss_backward_masked)
    int cap_B = 0;
    float* loss_dev = nullptr;
    // float-time training (dm_unet_train_enable_ft: ElucidatedDiffusion): the U-Net's time is a float per image and the
    // embedding's `weights` take a gradient (exact zeros when frozen: random_fourier_features has requires_grad = False)
    bool ft = false, freqs_frozen = false;
    float* init_w_raw = nullptr;  // ft: init_conv.weight as stored (a raw copy, redone after every optimiser step), which
                                  // launch_conv7_dgrad reads when a call asks for the gradient of the U-Net's input
    std::vector<float> coef_stage;  // the call's coefficient rows at the device width, then its float times
    // workspace bytes per call (measured by a dry run, once): entry, B, H, W, bucketed, the entry's own TrainRun::sel
    std::map<std::array<long long, 9>, size_t> ws_need;
    ~TrainState() {
        for (void* q : {(void*)param, (void*)adam_m, (void*)adam_v, (void*)ema, (void*)norm_ws, (void*)clip2, (void*)pack_tmp,
                        (void*)copy_table, (void*)mlp_rows, (void*)rjobs_dev, (void*)cjobs_dev, (void*)pk_dev[0], (void*)pk_dev[1],
                        (void*)big_tmp})
            if (q) (void)hipFree(q);
        for (FlushTables& f : flush) {
            for (int m = 0; m < WG_MODES; ++m)
                if (f.wtab_dev[m]) (void)hipFree(f.wtab_dev[m]);
            if (f.jobs_dev) (void)hipFree(f.jobs_dev);
        }
        for (Bucket& b : buckets)
            if (b.ready) (void)hipEventDestroy(b.ready);
        if (grad) (void)hipFree(grad);
        if (ws) (void)hipFree(ws);
        if (coef_dev) (void)hipFree(coef_dev);
        if (t_dev) (void)hipFree(t_dev);
        if (mask_dev) (void)hipFree(mask_dev);
        if (loss_dev) (void)hipFree(loss_dev);
        if (tf_dev) (void)hipFree(tf_dev);
    }
};

// (c_n, Cout, K, K) <- rotate 180 degrees and swap the channel roles of rows [c_lo, c_lo + c_n) of an OIHW (Cout, Cin, K, K)
static void rot_transpose(const float* w, int Cout, int Cin, int K, int c_lo, int c_n, std::vector<float>& out) {
    out.resize((size_t)c_n * Cout * K * K);
    for (int c = 0; c < c_n; ++c)
        for (int o = 0; o < Cout; ++o)
            for (int ky = 0; ky < K; ++ky)
                for (int kx = 0; kx < K; ++kx)
                    out[(((size_t)c * Cout + o) * K + ky) * K + kx] =
                        w[(((size_t)o * Cin + c_lo + c) * K + (K - 1 - ky)) * K + (K - 1 - kx)];
}

// the backward half of layer L (built by the named make_conv: it knows its weight)
static int build_conv_bwd(dm_unet* u, TrainState& T, const ConvLayer& L, ConvBwdKind kind) {
    ConvBwd& B = T.conv[&L];
    B.kind = kind;
    const std::string& wname = L.src.wname;
    T.conv_weights.insert(wname);
    const HostTensor& w = P(u, wname);
    if (kind == CB_INIT7 && T.ft) {
        if (T.own.upload(w.data.data(), w.numel(), &T.init_w_raw)) return 1;
        T.own.record_raw(wname, T.init_w_raw, w.numel());
    }
    if (kind == CB_INIT7 || kind == CB_FINAL) return 0;
    std::vector<float> wt;
    const int Cin = L.C0 + L.C1;
    PackSrc src;
    src.wname = wname;
    src.sCout = L.Cout;
    if (kind == CB_DOWN) {
        src.kind = PS_S2D_T;
        src.sCin = L.C0;
        B.d0.src = src;
        // Downsample: out[o] = sum_{c,sub} W[o][c*4 + sub] x[2y+p1][2x+p2][c]; the input gradient in space-to-depth order
        // t[(sub*C + c)] = sum_o W[o][c*4 + sub] dY[o] is a 1x1 convolution Cout -> 4C, then a depth-to-space copy
        const int C = L.C0, Cout = L.Cout;
        wt.resize((size_t)4 * C * Cout);
        for (int sub = 0; sub < 4; ++sub)
            for (int c = 0; c < C; ++c)
                for (int o = 0; o < Cout; ++o) wt[((size_t)sub * C + c) * Cout + o] = w.data[(size_t)o * 4 * C + c * 4 + sub];
        return make_conv(T.own, B.d0, wt.data(), nullptr, 4 * C, Cout, 0, 1, 1, 1, 0, false);
    }
    const int K = kind == CB_3X3 ? 3 : 1;
    src.kind = PS_ROT;
    src.sCin = Cin;
    src.sK = K;
    src.c_lo = 0;
    src.c_n = L.C0;
    B.d0.src = src;
    rot_transpose(w.data.data(), L.Cout, Cin, K, 0, L.C0, wt);
    if (make_conv(T.own, B.d0, wt.data(), nullptr, L.C0, L.Cout, 0, K, K, 1, K / 2, false)) return 1;
    B.has1 = L.C1 > 0;
    if (B.has1) {
        src.c_lo = L.C0;
        src.c_n = L.C1;
        B.d1.src = src;
        rot_transpose(w.data.data(), L.Cout, Cin, K, L.C0, L.C1, wt);
        if (make_conv(T.own, B.d1, wt.data(), nullptr, L.C1, L.Cout, 0, K, K, 1, K / 2, false)) return 1;
    }
    return 0;
}

static int build_resnet_bwd(dm_unet* u, TrainState& T, const ResBlock& R) {
    if (build_conv_bwd(u, T, R.c1, CB_3X3) || build_conv_bwd(u, T, R.c2, CB_3X3)) return 1;
    return R.has_res ? build_conv_bwd(u, T, R.res, CB_1X1) : 0;
}
static int build_attn_bwd(dm_unet* u, TrainState& T, const AttnLayer& A) {
    return build_conv_bwd(u, T, A.qkv, CB_1X1) || build_conv_bwd(u, T, A.out, CB_1X1);
}

// (re)build every dgrad layer from the host copies of the parameters
static int build_train(dm_unet* u) {
    TrainState& T = *u->train;
    T.own.reset();
    T.conv.clear();
    T.ops.clear();
    T.own.rec = &T.ops;
    const int n = u->cfg.n_stages;
    auto stage = [&](const Stage& S, ConvBwdKind resample) -> int {
        return build_resnet_bwd(u, T, S.b1) || build_resnet_bwd(u, T, S.b2) || build_attn_bwd(u, T, S.attn) ||
               build_conv_bwd(u, T, S.resample, resample);
    };
    if (build_conv_bwd(u, T, u->init_conv, CB_INIT7)) return 1;
    for (int i = 0; i < n; ++i)
        if (stage(u->downs[i], i < n - 1 ? CB_DOWN : CB_3X3)) return 1;
    if (build_resnet_bwd(u, T, u->mid1) || build_attn_bwd(u, T, u->mid_attn) || build_resnet_bwd(u, T, u->mid2)) return 1;
    for (int j = 0; j < n; ++j)
        if (stage(u->ups[j], CB_3X3)) return 1;
    if (build_resnet_bwd(u, T, u->final_res)) return 1;
    if (build_conv_bwd(u, T, u->final_conv, CB_FINAL)) return 1;
    if (u->cfg.text_mode == DM_TEXT_CROSS)
        for (const CrossLayer* C : {&u->cross_mid, &u->cross_down, &u->cross_up})
            if (build_conv_bwd(u, T, C->q, CB_1X1) || build_conv_bwd(u, T, C->out, CB_1X1)) return 1;
    // the host has just packed every buffer: nothing is stale, and the buffer -> recipe index is rebuilt on next use
    T.op_of.clear();
    T.n_copies = 0;
    std::fill(T.stale_f.begin(), T.stale_f.end(), 0);
    T.stale_b.clear();
    return 0;
}

// ---- the tape --------------------------------------------------------------------------------------------------------
struct BlockTape {
    const float *x0 = nullptr, *x1 = nullptr;
    float *u = nullptr, *y = nullptr;
    uint64_t drop_stream = 0;  // Philox stream of this block's dropout mask (0: no dropout)
};
struct ResTape {
    BlockTape b1, b2;
    float* out = nullptr;
};
struct AttnTape {
    const float* x = nullptr;
    float *xn = nullptr, *qkv = nullptr, *ctx = nullptr, *kst = nullptr, *o = nullptr, *y0 = nullptr, *y = nullptr;
};
struct CrossTape {
    const float* x = nullptr;
    float *q = nullptr, *k = nullptr, *v = nullptr, *o = nullptr, *y0 = nullptr, *y = nullptr;
};
struct NodeTape {  // what one node of the graph keeps: the member of its kind (a resample convolution keeps only its output)
    ResTape res;
    AttnTape attn;
    CrossTape cross;
};
struct Tape {
    float *e0 = nullptr, *h1pre = nullptr, *h1 = nullptr, *temb = nullptr, *ss = nullptr;
    float* tact = nullptr;  // SiLU(tfinal): the input of every ResnetBlock.mlp Linear
    int e0_dim = 0;         // row width of e0: dim (fixed sinusoid of an integer time) or learned_sinusoidal_dim + 1 (float time)
    // text conditioning: concat variant (text_proj -> cat(t, .) -> text_concat_proj) and the three CrossAttention layers
    float *te0pre = nullptr, *te0 = nullptr, *cat = nullptr;
    const float* tfinal = nullptr;  // what the ResnetBlock.mlp layers see (temb, or the text-concat projection)
    const float* ctx = nullptr;
    int ctx_tokens = 0;
    const int32_t* mask = nullptr;  // per-image caption dropout: rows with mask 0 took the text_emb = None path
    const UnetGraph* graph = nullptr;  // the node list the forward pass ran (unet_graph.inc)
    std::vector<NodeTape> nodes;       // one entry per node
    std::vector<float*> val;           // the tensor of every value id; val[0] is init_conv's output
};

// DM_TRAIN_NO_LANDING_FUSE: every K-split convolution of the training step lands its partial tiles in a pass of its own
static bool train_landing_fuse_off() {
    static const bool off = env_flag("DM_TRAIN_NO_LANDING_FUSE");
    return off;
}

struct TCtx {
    dm_unet* u;
    Arena* A;
    hipStream_t s;
    int B;
    const float* ss;
    int ss_stride;
    int acc = 0;  // 1: parameter gradients are added to what the buffers hold (gradient accumulation, :1164-1176)
    int n_blocks = 0;  // Blocks run so far in this forward: index of the next dropout mask
    std::vector<RowgradJob>* rjobs = nullptr;  // when set: the reductions behind norm_act_bwd / the column sums are collected
    std::vector<ColsumJob>* cjobs = nullptr;
    RowgradJob* rdefer() {
        if (!rjobs) return nullptr;
        rjobs->emplace_back();
        return &rjobs->back();
    }
    ColsumJob* cdefer() {
        if (!cjobs) return nullptr;
        cjobs->emplace_back();
        return &cjobs->back();
    }
    std::function<int(int)> phase_done;  // called when the backward pass leaves a phase (a stage): bucketed flush point
    std::vector<WgradDesc>* wbatch = nullptr;  // when set: MFMA weight gradients are recorded per mode ([3]) and run grouped
    std::vector<WgradJob>* jobs = nullptr;  // when set: the split-K sums of the weight gradients are collected, not launched
    WgradJob* defer() {
        if (!jobs) return nullptr;
        jobs->emplace_back();
        return &jobs->back();
    }
    float drop() const { return u->train ? u->train->dropout : 0.f; }
    bool dry() const { return A->dry; }
    Ctx conv() const { return Ctx{u, A, s, B, ss, ss_stride}; }
    float* grad(const std::string& name) const {
        auto it = u->train->off.find(name);
        if (it == u->train->off.end()) throw std::runtime_error("training: no gradient slot for parameter " + name);
        return u->train->grad + it->second;
    }
};

// Block.forward with the convolution output kept: u = conv(x) + b;  y = dropout(silu(norm(u) * (scale + 1) + shift)) [+ residual]
static int t_block(TCtx& t, const ConvLayer& L, const float* x0, const float* x1, int H, int W, const float* g,
                   const float* scale, const float* residual, BlockTape& bt) {
    const size_t rows = (size_t)t.B * H * W;
    bt.x0 = x0;
    bt.x1 = x1;
    bt.u = t.A->alloc(rows * L.Cout);
    bt.y = t.A->alloc(rows * L.Cout);
    const float p = t.drop();
    const int block_index = t.n_blocks++;
    bt.drop_stream = p > 0.f ? ((t.u->train->drop_call << 16) | (uint64_t)(block_index + 1)) : 0;
    Ctx c = t.conv();
    const bool no_fuse = train_landing_fuse_off();  // A/B: landing pass, then the norm pass
    PlannedConv P;
    if (plan_conv(c, L, x1 != nullptr, H, W, 0, false, false, P)) return 1;
    const int flags = EPI_NORM | EPI_SILU | (scale ? EPI_SCALE_SHIFT : 0);
    if (plan_leaves_partials(P) && !no_fuse) {
        // K-split / multi-tile convolution: ONE landing pass sums the partial tiles, adds the bias, keeps u and writes y
        float* part = nullptr;
        int nsplit = 0;
        if (run_conv_partial(c, L, x0, x1, H, W, &part, &nsplit)) return 1;
        const int rc = t.dry() ? 0
                               : launch_norm_act_drop(part, g, scale, t.ss_stride, H * W, residual, bt.y, t.B, L.Cout, flags, p,
                                                      t.u->train->drop_seed, bt.drop_stream, t.s, nsplit,
                                                      (int64_t)(rows * L.Cout), L.bias, bt.u);
        t.A->release(part);
        return rc;
    }
    if (run_conv(c, L, x0, x1, H, W, bt.u, 0, nullptr, nullptr, nullptr)) return 1;
    if (t.dry()) return 0;
    // one pass: norm, scale-shift, SiLU, the dropout mask (p > 0), then the residual (Block returns dropout(act(x)))
    return launch_norm_act_drop(bt.u, g, scale, t.ss_stride, H * W, residual, bt.y, t.B, L.Cout, flags, p,
                                t.u->train->drop_seed, bt.drop_stream, t.s);
}

static int t_resnet(TCtx& t, const ResBlock& R, const float* x0, const float* x1, int H, int W, ResTape& rt) {
    const float* scale = t.ss + R.ss_off;
    if (t_block(t, R.c1, x0, x1, H, W, R.g1, scale, nullptr, rt.b1)) return 1;
    if (!R.has_res) {  // block2(h) + x
        if (t_block(t, R.c2, rt.b1.y, nullptr, H, W, R.g2, nullptr, x0, rt.b2)) return 1;
        rt.out = rt.b2.y;
        return 0;
    }
    if (t_block(t, R.c2, rt.b1.y, nullptr, H, W, R.g2, nullptr, nullptr, rt.b2)) return 1;
    rt.out = t.A->alloc((size_t)t.B * H * W * R.dout);
    Ctx c = t.conv();
    return run_conv(c, R.res, x0, x1, H, W, rt.out, EPI_RESIDUAL, nullptr, nullptr, rt.b2.y);
}

static int t_attn(TCtx& t, const AttnLayer& At, const float* x, int H, int W, AttnTape& at) {
    dm_unet* u = t.u;
    const int n = H * W, heads = At.heads, hidden = heads * u->dh;
    const size_t rows = (size_t)t.B * n;
    at.x = x;
    at.xn = t.A->alloc(rows * At.dim);
    at.qkv = t.A->alloc(rows * 3 * hidden);
    at.o = t.A->alloc(rows * hidden);
    at.y = t.A->alloc(rows * At.dim);
    Ctx c = t.conv();
    if (attn_qkv(c, At, x, H, W, at.xn, at.qkv)) return 1;
    if (At.full) {
        if (attn_core(c, At, at.qkv, n, at.o, nullptr, nullptr)) return 1;
        return run_conv(c, At.out, at.o, nullptr, H, W, at.y, EPI_RESIDUAL, nullptr, nullptr, x);
    }
    at.ctx = t.A->alloc((size_t)t.B * heads * u->dh * u->dh);
    at.kst = t.A->alloc((size_t)t.B * heads * 2 * u->dh);  // the key statistics the backward pass starts from
    at.y0 = t.A->alloc(rows * At.dim);
    if (attn_core(c, At, at.qkv, n, at.o, at.ctx, at.kst)) return 1;
    if (run_conv(c, At.out, at.o, nullptr, H, W, at.y0, 0, nullptr, nullptr, nullptr)) return 1;
    if (t.dry()) return 0;
    return launch_norm_act(at.y0, 1, 0, nullptr, At.out_g, nullptr, 0, n, x, at.y, (int64_t)rows, At.dim,
                           EPI_NORM | EPI_RESIDUAL, t.s);
}

static int conv_wgrad(TCtx& t, const ConvLayer& L, const float* x0, const float* x1, const float* dy, int Ho, int Wo,
                      bool bias_from_colsum);
static int conv_dgrad(TCtx& t, const ConvLayer& L, const float* dy, int Hin, int Win, const float* add0, const float* add1,
                      float** dx0, float** dx1);

// CrossAttention.forward (DD/denoising_diffusion_text_conditional.py:54-78) in tape mode, general path (m context tokens);
// the result REPLACES x (:173-177): no residual.  mask (per-image caption dropout): the layer is skipped for rows with
// mask 0 (text_emb is None, :173/:183/:194), so those rows of the result are x -- the select of dm_unet_forward_masked
static int t_cross(TCtx& t, const CrossLayer& Cr, const float* x, int H, int W, const float* ctx, int m, CrossTape& ct,
                   const int32_t* mask) {
    const int n = H * W, inner = 4 * t.u->dh, dim = Cr.out.Cout;
    const size_t rows = (size_t)t.B * n;
    ct.x = x;
    ct.q = t.A->alloc(rows * inner);
    ct.k = t.A->alloc((size_t)t.B * m * inner);
    ct.v = t.A->alloc((size_t)t.B * m * inner);
    ct.o = t.A->alloc(rows * inner);
    ct.y0 = t.A->alloc(rows * dim);
    ct.y = t.A->alloc(rows * dim);
    Ctx c = t.conv();
    if (cross_front(c, Cr, x, H, W, ctx, m, ct.q, ct.k, ct.v, ct.o)) return 1;
    if (run_conv(c, Cr.out, ct.o, nullptr, H, W, ct.y0, 0, nullptr, nullptr, nullptr)) return 1;
    if (t.dry()) return 0;
    if (launch_norm_act(ct.y0, 1, 0, nullptr, Cr.g, nullptr, 0, n, nullptr, ct.y, (int64_t)rows, dim, EPI_NORM, t.s)) return 1;
    return mask ? launch_select_rows(ct.y, x, (int64_t)n * dim, mask, t.B, (int64_t)n * dim, t.s) : 0;
}

// mask (per-image caption dropout): rows with mask 0 kept the layer's input, so their gradient bypasses the layer -- the
// layer receives exact zeros for them (every parameter gradient is linear in it) and *dx_out is dy for those rows
static int t_cross_bwd(TCtx& t, const CrossLayer& Cr, const CrossTape& ct, const float* dy_in, int H, int W, const float* ctx, int m,
                       float** dx_out, const int32_t* mask) {
    dm_unet* u = t.u;
    const std::string& p = Cr.prefix;
    const int n = H * W, inner = 4 * u->dh, dim = Cr.out.Cout, E = u->cfg.text_emb_dim;
    const size_t rows = (size_t)t.B * n;
    const int64_t per = (int64_t)n * dim;
    const float* dy = dy_in;
    if (mask) {
        DM_REQUIRE(Cr.q.C0 == dim, "CrossAttention replaces x: its input and output widths are equal");
        float* kept = t.A->alloc(rows * dim);
        if (!t.dry() && launch_route_rows(kept, per, dy_in, per, nullptr, 0, mask, t.B, per, t.s)) return 1;
        dy = kept;
    }
    float* dy0 = t.A->alloc(rows * dim);
    float* ws = t.A->alloc(norm_act_bwd_ws_floats(t.B, n, dim));
    if (!t.dry() && launch_norm_act_bwd(dy, ct.y0, Cr.g, nullptr, 0, n, dy0, ws, t.grad(p + ".to_out.1.g"),
                                        t.grad(p + ".to_out.0.bias"), nullptr, 0, t.B, dim, EPI_NORM, t.acc, t.s, t.rdefer()))
        return 1;
    if (conv_wgrad(t, Cr.out, ct.o, nullptr, dy0, H, W, false)) return 1;
    float *dO = nullptr, *none = nullptr;
    if (conv_dgrad(t, Cr.out, dy0, H, W, nullptr, nullptr, &dO, &none)) return 1;
    float* dq = t.A->alloc(rows * inner);
    float* dk = t.A->alloc((size_t)t.B * m * inner);
    float* dv = t.A->alloc((size_t)t.B * m * inner);
    float* aws = t.A->alloc(attn_bwd_ws_floats(t.B, n, m, 0, 4, u->dh));
    if (!t.dry()) {
        if (launch_cross_attention_core_bwd(ct.q, ct.k, ct.v, dO, dq, dk, dv, aws, t.B, n, m, 4, u->dh, t.s)) return 1;
        if (launch_linear_wgrad(dk, inner, ctx, E, t.grad(p + ".to_k.weight"), t.B * m, E, inner, 0, t.acc, t.s)) return 1;
        if (launch_linear_wgrad(dv, inner, ctx, E, t.grad(p + ".to_v.weight"), t.B * m, E, inner, 0, t.acc, t.s)) return 1;
    }
    if (conv_wgrad(t, Cr.q, ct.x, nullptr, dq, H, W, false)) return 1;
    if (conv_dgrad(t, Cr.q, dq, H, W, nullptr, nullptr, dx_out, &none)) return 1;
    if (mask && !t.dry()) return launch_route_rows(*dx_out, per, *dx_out, per, dy_in, per, mask, t.B, per, t.s);
    return 0;
}

// The conditioning head of the training forward: as cond_forward (dm_api.hip), one row per image, with every activation a
// pass of its own so that the backward head (cond_backward) finds its inputs in the tape.  unet_train_forward and
// dm_unet_cond_forward run this one function.
static int cond_train_forward(dm_unet* u, Arena& A, const int64_t* t_dev, const float* tf_dev, const float* ctx, int ctx_tokens,
                              const int32_t* mask, int B, hipStream_t s, Tape& tp) {
    const dm_unet_cfg& cfg = u->cfg;
    const int td = u->time_dim;
    const bool text_concat = cfg.text_mode == DM_TEXT_CONCAT && ctx != nullptr;
    // tf_dev: a float time per image (ElucidatedDiffusion's c_noise(sigma)) through cat(t, sin(t w 2 pi), cos(t w 2 pi))
    const int fdim = tp.e0_dim = tf_dev ? cfg.learned_sinusoidal_dim + 1 : cfg.dim;
    tp.e0 = A.alloc((size_t)B * fdim);
    tp.h1pre = A.alloc((size_t)B * td);
    tp.h1 = A.alloc((size_t)B * td);
    tp.temb = A.alloc((size_t)B * td);
    tp.ss = A.alloc((size_t)B * u->ss_total);
    if (!A.dry) {
        if (tf_dev) {
            if (launch_sinusoid_ft(tf_dev, 0, nullptr, u->freqs, tp.e0, B, cfg.learned_sinusoidal_dim / 2, s, true)) return 1;
        } else if (launch_sinusoid(t_dev, nullptr, nullptr, u->freqs, tp.e0, B, cfg.dim / 2, s)) {
            return 1;
        }
        if (launch_linear_rows(tp.e0, fdim, u->tw1, u->tb1, tp.h1pre, td, B, fdim, td, 0, 0, s)) return 1;
        if (launch_act_fwd(tp.h1pre, tp.h1, (int64_t)B * td, 2, s)) return 1;
        if (launch_linear_rows(tp.h1, td, u->tw2, u->tb2, tp.temb, td, B, td, td, 0, 0, s)) return 1;
    }
    tp.tfinal = tp.temb;
    if (text_concat) {
        // t = text_concat_proj(cat(t, text_proj(text_emb)))  (DD/denoising_diffusion_text_conditional.py:146-152)
        DM_REQUIRE(ctx_tokens == 1, "text concat conditioning takes one pooled embedding per sample");
        const int E = cfg.text_emb_dim;
        tp.te0pre = A.alloc((size_t)B * td);
        tp.te0 = A.alloc((size_t)B * td);
        tp.cat = A.alloc((size_t)B * 2 * td);
        float* t2 = A.alloc((size_t)B * td);
        if (!A.dry) {
            DM_CHECK_HIP(hipMemcpy2DAsync(tp.cat, 2 * td * sizeof(float), tp.temb, td * sizeof(float), td * sizeof(float), B,
                                          hipMemcpyDeviceToDevice, s));
            if (launch_linear_rows(ctx, E, u->tp_w0, u->tp_b0, tp.te0pre, td, B, E, td, 0, 0, s)) return 1;
            if (launch_act_fwd(tp.te0pre, tp.te0, (int64_t)B * td, 2, s)) return 1;
            if (launch_linear_rows(tp.te0, td, u->tp_w2, u->tp_b2, tp.cat + td, 2 * td, B, td, td, 0, 0, s)) return 1;
            if (launch_linear_rows(tp.cat, 2 * td, u->tc_w, u->tc_b, t2, td, B, 2 * td, td, 0, 0, s)) return 1;
            // per-image caption dropout: rows with mask 0 keep the raw time embedding (text_emb is None, :146)
            if (mask && launch_select_rows(t2, tp.temb, td, mask, B, td, s)) return 1;
        }
        tp.tfinal = t2;
    }
    // all 19 ResnetBlock.mlp (SiLU -> Linear) in one launch; SiLU(t) is formed once here, not once per output row of the
    // [ss_total][time_dim] matrix inside the kernel (98 -> 30 us at B = 64)
    float* tact = tp.tact = A.alloc((size_t)B * td);
    if (!A.dry && (launch_act_fwd(tp.tfinal, tact, (int64_t)B * td, 1, s) ||
                   launch_linear_rows(tact, td, u->ss_w, u->ss_b, tp.ss, u->ss_total, B, td, u->ss_total, 0, 0, s)))
        return 1;
    return 0;
}

// Unet.forward (DD/denoising_diffusion.py:349-390) with per-sample times and everything kept for the backward pass
static int unet_train_forward(dm_unet* u, Arena& A, const float* x_nchw, const int64_t* t_dev, float* out_nchw, int B, int H,
                              int W, hipStream_t s, Tape& tp, const float* ctx = nullptr, int ctx_tokens = 0,
                              const int32_t* mask = nullptr, const float* tf_dev = nullptr) {
    const dm_unet_cfg& cfg = u->cfg;
    const bool text_cross = cfg.text_mode == DM_TEXT_CROSS && ctx != nullptr;
    tp.ctx = ctx;
    tp.ctx_tokens = ctx_tokens;
    tp.mask = ctx ? mask : nullptr;
    TCtx t{u, &A, s, B, nullptr, 0};
    if (cond_train_forward(u, A, t_dev, tf_dev, ctx, ctx_tokens, mask, B, s, tp)) return 1;
    t.ss = A.dry ? reinterpret_cast<const float*>(16) : tp.ss;
    t.ss_stride = u->ss_total;
    Ctx c = t.conv();
    const UnetGraph& G = u->graphs[text_cross ? GRAPH_CROSS : GRAPH_PLAIN];
    tp.graph = &G;
    tp.nodes.assign(G.nodes.size(), NodeTape{});
    tp.val.assign(G.n_values(), nullptr);
    tp.val[0] = A.alloc((size_t)B * H * W * u->init_dim);
    if (run_conv(c, u->init_conv, x_nchw, nullptr, H, W, tp.val[0], 0, nullptr, nullptr, nullptr, /*in_nchw=*/true)) return 1;
    // the node list of the inference walk (unet_graph.inc), with everything kept: nothing is released
    for (size_t k = 0; k < G.nodes.size(); ++k) {
        const UnetNode& N = G.nodes[k];
        NodeTape& nt = tp.nodes[k];
        const float* in0 = tp.val[N.in0];
        const float* in1 = N.in1 >= 0 ? tp.val[N.in1] : nullptr;
        const int hi = H >> N.lin, wi = W >> N.lin, ho = H >> N.lout, wo = W >> N.lout;
        switch (N.kind) {
        case NODE_RESNET:
            if (t_resnet(t, N.res(), in0, in1, hi, wi, nt.res)) return 1;
            tp.val[N.out] = nt.res.out;
            break;
        case NODE_ATTN:
            if (t_attn(t, N.attn(), in0, hi, wi, nt.attn)) return 1;
            tp.val[N.out] = nt.attn.y;
            break;
        case NODE_CROSS:  // the text hooks around the bottleneck (DD/denoising_diffusion_text_conditional.py:173-203)
            if (t_cross(t, N.cross(), in0, hi, wi, ctx, ctx_tokens, nt.cross, mask)) return 1;
            tp.val[N.out] = nt.cross.y;
            break;
        case NODE_CONV:
            tp.val[N.out] = A.alloc((size_t)B * ho * wo * N.conv().Cout);
            if (run_conv(c, N.conv(), in0, nullptr, std::max(hi, ho), std::max(wi, wo), tp.val[N.out], 0, nullptr, nullptr, nullptr)) return 1;
            break;
        }
    }
    return run_conv(c, u->final_conv, tp.val[G.out()], nullptr, H, W, out_nchw, 0, nullptr, nullptr, nullptr, false, /*out_nchw=*/true);
}

// ---- backward pieces ---------------------------------------------------------------------------------------------------
// weight (+ bias, from the column sums of dy) gradient of one convolution, into the gradient slots of the parameters the
// layer was built from; dy = gradient of its output (NHWC unless the layer is the NCHW final_conv)
static int conv_wgrad(TCtx& t, const ConvLayer& L, const float* x0, const float* x1, const float* dy, int Ho, int Wo,
                      bool bias_from_colsum) {
    const ConvBwdKind kind = t.u->train->conv.at(&L).kind;
    const std::string &wname = L.src.wname, &bname = L.src.bname;
    const int Cin = L.C0 + L.C1;
    const int64_t rows = (int64_t)t.B * Ho * Wo;
    if (kind == CB_INIT7 || kind == CB_FINAL) {
        int splits;
        float* ws = t.A->alloc(wgrad_naive_ws_floats(t.B, Ho, L.Cout, Cin, L.KH, L.KW, &splits));
        float* cw = (bias_from_colsum && kind == CB_INIT7) ? t.A->alloc(colsum_ws_floats(rows, L.Cout)) : nullptr;
        if (t.dry()) return 0;
        if (launch_wgrad_naive(x0, kind == CB_INIT7, dy, kind == CB_FINAL, Cin, L.Cout, L.KH, L.KW, L.pad, t.B, Ho, Wo, ws,
                               t.grad(wname), t.acc, t.s, t.defer()))
            return 1;
        if (!bias_from_colsum) return 0;
        if (kind == CB_FINAL) return launch_colsum_nchw(dy, t.B, L.Cout, Ho * Wo, t.grad(bname), t.acc, t.s);
        return launch_colsum(dy, rows, L.Cout, L.Cout, 1, cw, t.grad(bname), t.acc, t.s, t.cdefer());
    }
    // 3x3 on even image sizes: Winograd-domain weight gradient (16 instead of 36 products per 2x2 tile)
    static const bool no_wino = env_flag("DM_WGRAD_NO_WINO") || winograd_off();
    const WgradMode mode = kind == CB_1X1 ? WG_1X1 : kind == CB_DOWN ? WG_DOWN
                           : (!no_wino && Ho % 2 == 0 && Wo % 2 == 0) ? WG_WINO : WG_3X3;
    int T, cin_w;
    wgrad_dims(mode, L, &T, &cin_w);
    if (t.wbatch) {  // runs with every other layer of its mode at the end of the backward pass (unet_train_backward)
        t.wbatch[mode].push_back(WgradDesc{x0, x1, dy, t.dry() ? nullptr : t.grad(wname), L.C0, L.C1, L.Cout, t.B, Ho, Wo,
                                           L.up ? 1 : 0, t.acc});
    } else {
        float* ws = t.A->alloc(wgrad_ws_floats(t.B, Ho, Wo, L.Cout, cin_w, T, nullptr));
        if (!t.dry() && launch_wgrad(x0, L.C0, x1, L.C1, dy, L.Cout, t.B, Ho, Wo, mode, L.up ? 1 : 0, ws, t.grad(wname), t.acc,
                                     t.s, t.defer()))
            return 1;
    }
    if (bias_from_colsum) {
        float* cw = t.A->alloc(colsum_ws_floats(rows, L.Cout));
        if (!t.dry() && launch_colsum(dy, rows, L.Cout, L.Cout, 1, cw, t.grad(bname), t.acc, t.s, t.cdefer())) return 1;
    }
    return 0;
}

// input gradient(s) of one convolution: *dx0 = dgrad0(dy) [+ add0], *dx1 = dgrad1(dy) [+ add1]; (Hin, Win) = input size
static int conv_dgrad(TCtx& t, const ConvLayer& L, const float* dy, int Hin, int Win, const float* add0, const float* add1,
                      float** dx0, float** dx1) {
    const ConvBwd& Bw = t.u->train->conv.at(&L);
    Ctx c{t.u, t.A, t.s, t.B, nullptr, 0};
    if (Bw.kind == CB_DOWN) {  // Downsample: 1x1 to 4C channels at the output size, then depth-to-space
        const int Ho = Hin / 2, Wo = Win / 2;
        float* tmp = t.A->alloc((size_t)t.B * Ho * Wo * 4 * L.C0);
        if (run_conv(c, Bw.d0, dy, nullptr, Ho, Wo, tmp, 0, nullptr, nullptr, nullptr)) return 1;
        *dx0 = t.A->alloc((size_t)t.B * Hin * Win * L.C0);
        if (!t.dry() && launch_depth_to_space(tmp, add0, *dx0, t.B, Ho, Wo, L.C0, t.s)) return 1;
        return 0;
    }
    if (L.up) {  // nearest x2 in front of the conv: input gradient at the upsampled size, then the 2x2 sums
        const int Hu = 2 * Hin, Wu = 2 * Win;
        float* tmp = t.A->alloc((size_t)t.B * Hu * Wu * L.C0);
        if (run_conv(c, Bw.d0, dy, nullptr, Hu, Wu, tmp, 0, nullptr, nullptr, nullptr)) return 1;
        *dx0 = t.A->alloc((size_t)t.B * Hin * Win * L.C0);
        if (!t.dry() && launch_pool2x2_sum(tmp, add0, *dx0, t.B, Hin, Win, L.C0, t.s)) return 1;
        return 0;
    }
    *dx0 = t.A->alloc((size_t)t.B * Hin * Win * L.C0);
    if (run_conv(c, Bw.d0, dy, nullptr, Hin, Win, *dx0, add0 ? EPI_RESIDUAL : 0, nullptr, nullptr, add0)) return 1;
    if (Bw.has1) {
        *dx1 = t.A->alloc((size_t)t.B * Hin * Win * L.C1);
        if (run_conv(c, Bw.d1, dy, nullptr, Hin, Win, *dx1, add1 ? EPI_RESIDUAL : 0, nullptr, nullptr, add1)) return 1;
    }
    return 0;
}

// A gradient tensor handed to norm_act_bwd_kernel: the tensor itself (nsplit == 1) or the K-split partial sums of the
// convolution that produced it, which the kernel adds up on load (no landing pass in between)
struct DyParts {
    const float* p = nullptr;
    int nsplit = 1;
    int64_t stride = 0;
    float* owned = nullptr;  // partial-sum buffer to release once the consumer has been enqueued
};
// input gradient of a single-input, stride-1 convolution for a consumer that can sum partial tiles itself
static int conv_dgrad_parts(TCtx& t, const ConvLayer& L, const float* dy, int H, int W, DyParts* out) {
    const ConvBwd& Bw = t.u->train->conv.at(&L);
    const bool no_fuse = train_landing_fuse_off();
    Ctx c{t.u, t.A, t.s, t.B, nullptr, 0};
    PlannedConv P;
    const bool plain = (Bw.kind == CB_3X3 || Bw.kind == CB_1X1) && !L.up && !Bw.has1 && !no_fuse;
    if (plain && plan_conv(c, Bw.d0, false, H, W, 0, false, false, P)) return 1;
    if (plain && plan_leaves_partials(P)) {
        float* part = nullptr;
        if (run_conv_partial(c, Bw.d0, dy, nullptr, H, W, &part, &out->nsplit)) return 1;
        out->p = out->owned = part;
        out->stride = (int64_t)t.B * H * W * L.C0;
        return 0;
    }
    float *dx = nullptr, *none = nullptr;
    if (conv_dgrad(t, L, dy, H, W, nullptr, nullptr, &dx, &none)) return 1;
    *out = DyParts{dx, 1, 0, nullptr};
    return 0;
}

// Block backward: dy -> du (gradient of the convolution output), parameter gradients of g / bias / weight and, with a
// scale-shift, this block's columns of dss
static int t_block_bwd(TCtx& t, const ConvLayer& L, const BlockTape& bt, const DyParts& dy, int H, int W, const float* g,
                       const float* scale, int ss_off, float* dss, const std::string& p, float** du_out) {
    const size_t rows = (size_t)t.B * H * W;
    float* du = t.A->alloc(rows * L.Cout);
    float* ws = t.A->alloc(norm_act_bwd_ws_floats(t.B, H * W, L.Cout));
    const int flags = EPI_NORM | EPI_SILU | (scale ? EPI_SCALE_SHIFT : 0);
    // the gradient goes through the dropout mask of the forward pass: the kernel recomputes it from its key
    if (!t.dry() && launch_norm_act_bwd(dy.p, bt.u, g, scale, t.ss_stride, H * W, du, ws, t.grad(p + ".norm.g"),
                                        t.grad(p + ".proj.bias"), scale ? dss + ss_off : nullptr, t.u->ss_total, t.B, L.Cout,
                                        flags, t.acc, t.s, t.rdefer(), t.drop(), t.u->train->drop_seed, bt.drop_stream, nullptr,
                                        dy.nsplit, dy.stride))
        return 1;
    if (dy.owned) t.A->release(dy.owned);
    if (conv_wgrad(t, L, bt.x0, bt.x1, du, H, W, false)) return 1;
    *du_out = du;
    return 0;
}

// ResnetBlock backward: dout -> d(x0) [+ extra0], d(x1)
static int t_resnet_bwd(TCtx& t, const ResBlock& R, const ResTape& rt, const float* dout, int H, int W, float* dss,
                        const float* extra0, float** dx0, float** dx1) {
    TrainState& T = *t.u->train;
    const float* scale = t.ss + R.ss_off;
    float *du2 = nullptr, *du1 = nullptr;
    DyParts dh1;
    if (t_block_bwd(t, R.c2, rt.b2, DyParts{dout}, H, W, R.g2, nullptr, 0, nullptr, R.prefix + ".block2", &du2)) return 1;
    if (conv_dgrad_parts(t, R.c2, du2, H, W, &dh1)) return 1;
    if (t_block_bwd(t, R.c1, rt.b1, dh1, H, W, R.g1, scale, R.ss_off, dss, R.prefix + ".block1", &du1)) return 1;
    const size_t n0 = (size_t)t.B * H * W * R.c1.C0;
    *dx1 = nullptr;
    if (!R.has_res) {  // + x: the output gradient flows straight into d(x0)
        const float* add = dout;
        if (extra0) {
            float* sum = t.A->alloc(n0);
            if (!t.dry() && launch_add3(dout, extra0, nullptr, sum, (int64_t)n0, t.s)) return 1;
            add = sum;
        }
        return conv_dgrad(t, R.c1, du1, H, W, add, nullptr, dx0, dx1);
    }
    if (conv_wgrad(t, R.res, rt.b1.x0, rt.b1.x1, dout, H, W, true)) return 1;
    const ConvBwd &Br = T.conv.at(&R.res), &Bc = T.conv.at(&R.c1);
    // d(x) = dgrad_c1(du1) + dgrad_res(dout), per concat half.  Where block1's input gradient leaves K-split partial tiles for a
    // landing pass anyway, res_conv's input gradient stays partial tiles too and that ONE landing sums both (what run_resnet
    // does for block2 + res_conv in the forward pass): two launches per half instead of four.
    const bool no_merge = train_landing_fuse_off();
    Ctx c{t.u, t.A, t.s, t.B, nullptr, 0};
    auto half = [&](const ConvLayer& Lc, const ConvLayer& Lr, int C, float** dx, bool* done) -> int {
        *done = false;
        PlannedConv Pc, Pr;
        if (plan_conv(c, Lc, false, H, W, EPI_RESIDUAL, false, false, Pc) || plan_conv(c, Lr, false, H, W, 0, false, false, Pr)) return 1;
        if (!plan_leaves_partials(Pc) || !conv_families[Pr.kind].partials) return 0;
        ResParts rp{};
        float* rpart = nullptr;
        if (run_conv_partial(c, Lr, dout, nullptr, H, W, &rpart, &rp.nsplit)) return 1;
        rp.part = rpart;
        rp.stride = (int64_t)t.B * H * W * C;
        rp.bias = nullptr;
        *dx = t.A->alloc((size_t)t.B * H * W * C);
        if (run_conv(c, Lc, du1, nullptr, H, W, *dx, 0, nullptr, nullptr, nullptr, false, false, &rp)) return 1;
        t.A->release(rpart);
        *done = true;
        return 0;
    };
    if (!no_merge && !extra0 && Bc.kind == CB_3X3 && Br.kind == CB_1X1 && !R.c1.up && Bc.has1 == Br.has1) {
        bool d0 = false, d1 = !Bc.has1;
        if (half(Bc.d0, Br.d0, R.c1.C0, dx0, &d0)) return 1;
        if (Bc.has1 && d0 && half(Bc.d1, Br.d1, R.c1.C1, dx1, &d1)) return 1;
        if (d0 && d1) return 0;
        if (d0 != d1) {  // (one half planned in-kernel, the other not: finish the other one the plain way)
            DM_REQUIRE(d0 && Bc.has1, "res merge: halves");
            float* r1 = t.A->alloc((size_t)t.B * H * W * R.c1.C1);
            if (run_conv(c, Br.d1, dout, nullptr, H, W, r1, 0, nullptr, nullptr, nullptr)) return 1;
            *dx1 = t.A->alloc((size_t)t.B * H * W * R.c1.C1);
            return run_conv(c, Bc.d1, du1, nullptr, H, W, *dx1, EPI_RESIDUAL, nullptr, nullptr, r1);
        }
    }
    float *r0 = nullptr, *r1 = nullptr;
    if (conv_dgrad(t, R.res, dout, H, W, extra0, nullptr, &r0, &r1)) return 1;
    return conv_dgrad(t, R.c1, du1, H, W, r0, r1, dx0, dx1);
}

// (attn(x) + x) backward: dy -> dx
static int t_attn_bwd(TCtx& t, const AttnLayer& At, const AttnTape& at, const float* dy, int H, int W, float** dx_out,
                      bool add_x = true) {
    dm_unet* u = t.u;
    const std::string& p = At.prefix;
    const int n = H * W, heads = At.heads, hidden = heads * u->dh;
    const size_t rows = (size_t)t.B * n;
    const float* dyo = dy;  // gradient of the to_out convolution's output
    if (!At.full) {
        float* dy0 = t.A->alloc(rows * At.dim);
        float* ws = t.A->alloc(norm_act_bwd_ws_floats(t.B, n, At.dim));
        if (!t.dry() && launch_norm_act_bwd(dy, at.y0, At.out_g, nullptr, 0, n, dy0, ws, t.grad(p + ".to_out.1.g"),
                                            t.grad(At.out.src.bname), nullptr, 0, t.B, At.dim, EPI_NORM, t.acc, t.s, t.rdefer()))
            return 1;
        dyo = dy0;
    }
    if (conv_wgrad(t, At.out, at.o, nullptr, dyo, H, W, At.full)) return 1;
    float *dO = nullptr, *none = nullptr;
    if (conv_dgrad(t, At.out, dyo, H, W, nullptr, nullptr, &dO, &none)) return 1;
    float* dqkv = t.A->alloc(rows * 3 * hidden);
    const size_t nmem = (size_t)2 * heads * u->dh * 4;
    float* dmem = t.A->alloc((size_t)t.B * nmem);
    float* cw = t.A->alloc(colsum_ws_floats(t.B, (int)nmem));
    if (At.full) {
        float* ws = t.A->alloc(attn_bwd_ws_floats(t.B, n, n, 4, heads, u->dh));
        if (!t.dry() && launch_attention_core_bwd(at.qkv, At.mem_kv, dO, dqkv, dmem, ws, t.B, n, heads, u->dh, t.s))
            return 1;
    } else {
        float* ws = t.A->alloc(linattn_bwd_ws_floats(t.B, n, heads, u->dh));
        if (!t.dry() && launch_linear_attention_core_bwd(at.qkv, At.mem_kv, at.ctx, dO, ws, dqkv, dmem, t.B, n, heads,
                                                         u->dh, t.s, at.kst))
            return 1;
    }
    if (!t.dry() && launch_colsum(dmem, t.B, (int)nmem, (int64_t)nmem, 1, cw, t.grad(p + ".mem_kv"), t.acc, t.s, t.cdefer()))
        return 1;
    if (conv_wgrad(t, At.qkv, at.xn, nullptr, dqkv, H, W, false)) return 1;
    DyParts dxn;
    if (conv_dgrad_parts(t, At.qkv, dqkv, H, W, &dxn)) return 1;
    float* dxa = t.A->alloc(rows * At.dim);
    float* ws2 = t.A->alloc(norm_act_bwd_ws_floats(t.B, n, At.dim));
    // (attn(x) + x): the residual branch's gradient dy joins in the kernel's store
    if (!t.dry() && launch_norm_act_bwd(dxn.p, at.x, At.norm_g, nullptr, 0, n, dxa, ws2, t.grad(p + ".norm.g"), nullptr, nullptr,
                                        0, t.B, At.dim, EPI_NORM, t.acc, t.s, t.rdefer(), 0.f, 0, 0, add_x ? dy : nullptr,
                                        dxn.nsplit, dxn.stride))
        return 1;
    if (dxn.owned) t.A->release(dxn.owned);
    *dx_out = dxa;
    return 0;
}

// plain convolution (resample convs, final_conv): weight / bias gradient, input gradient [+ add]
static int t_conv_bwd(TCtx& t, const ConvLayer& L, const float* x, const float* dy, int Hin, int Win, int Ho, int Wo,
                      const float* add, float** dx) {
    if (conv_wgrad(t, L, x, nullptr, dy, Ho, Wo, true)) return 1;
    float* none = nullptr;
    return conv_dgrad(t, L, dy, Hin, Win, add, nullptr, dx, &none);
}

// a table that is a function of the shapes only: uploaded when it differs from the one already on the device
template <class E>
static int upload_table(const std::vector<E>& host, std::vector<E>& cached, E*& dev, size_t& cap, hipStream_t s) {
    const size_t bytes = host.size() * sizeof(E);
    if (host.size() == cached.size() && std::memcmp(host.data(), cached.data(), bytes) == 0) return 0;
    if (host.size() > cap) {
        DM_CHECK_HIP(hipStreamSynchronize(s));
        if (dev) (void)hipFree(dev);
        dev = nullptr;
        cap = 0;
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&dev), bytes));
        cap = host.size();
    }
    DM_CHECK_HIP(hipMemcpyAsync(dev, host.data(), bytes, hipMemcpyHostToDevice, s));
    DM_CHECK_HIP(hipStreamSynchronize(s));  // pageable source
    cached = host;
    return 0;
}

// The per-image / per-channel reductions behind every norm_act_bwd_kernel of a backward pass (dss is complete after them)
// and every bias / mem_kv column sum of it, as collected in TCtx::rjobs / TCtx::cjobs: two launches each.  The tables are
// given their block prefixes (the column sums: partial-pass jobs first) and uploaded here.
static int flush_deferred_reductions(TrainState& T, std::vector<RowgradJob>& rjobs, std::vector<ColsumJob>& cjobs, hipStream_t s) {
    if (!rjobs.empty()) {
        int ib = 0, fb = 0;
        rowgrad_jobs_prefix(rjobs, &ib, &fb);
        if (upload_table(rjobs, T.rjobs_host, T.rjobs_dev, T.rjobs_cap, s)) return 1;
        if (launch_rowgrad_jobs(T.rjobs_dev, (int)rjobs.size(), ib, fb, s)) return 1;
    }
    if (!cjobs.empty()) {
        int pb = 0, fb = 0;
        colsum_jobs_prefix(cjobs, &pb, &fb);
        int n_part = 0;
        for (const ColsumJob& j : cjobs) n_part += j.nb > 0;
        if (upload_table(cjobs, T.cjobs_host, T.cjobs_dev, T.cjobs_cap, s)) return 1;
        if (launch_colsum_jobs(T.cjobs_dev, (int)cjobs.size(), n_part, pb, fb, s)) return 1;
    }
    return 0;
}

// Where a call that differentiates through the U-Net's inputs wants them (float-time handles): dx (B, C, H, W), dt (B)
struct InputGrad {
    float* dx;
    float* dt;
};

// The backward of the conditioning head (cond_train_forward) from dss (B, ss_total), the gradient of the scale / shift rows:
// ResnetBlock.mlp (SiLU -> Linear), all 19 of them through the concatenated matrix, then (text_concat_proj, text_proj,)
// time_mlp, and on a float-time handle the embedding's weights and ig->dt.  unet_train_backward_impl and
// dm_unet_cond_backward run this one function.
static int cond_backward(TCtx& t, const Tape& tp, const float* dss, const InputGrad* ig) {
    dm_unet* u = t.u;
    Arena& A = *t.A;
    hipStream_t s = t.s;
    const int B = t.B;
    const dm_unet_cfg& cfg = u->cfg;
    const int td = u->time_dim;
    const bool text_concat = cfg.text_mode == DM_TEXT_CONCAT && tp.ctx != nullptr;
    float* dtf0 = A.alloc((size_t)B * td);
    float* dtf = A.alloc((size_t)B * td);
    float* dcat = text_concat ? A.alloc((size_t)B * 2 * td) : nullptr;
    float* dte0 = text_concat ? A.alloc((size_t)B * td) : nullptr;
    float* dte0pre = text_concat ? A.alloc((size_t)B * td) : nullptr;
    float* dtc_kept = text_concat && tp.mask ? A.alloc((size_t)B * td) : nullptr;
    float* dh1 = A.alloc((size_t)B * td);
    float* dh1pre = A.alloc((size_t)B * td);
    float* cw = A.alloc(colsum_ws_floats(B, std::max(u->ss_total, 2 * td)));
    float* dgw = A.alloc(linear_dgrad_ws_floats(B, td, u->ss_total));
    const bool ft = u->train->ft;  // the embedding has a parameter: the pass goes on through time_mlp.1 into e0
    float* de0 = ft ? A.alloc((size_t)B * tp.e0_dim) : nullptr;
    if (A.dry) return 0;
    {   // every ResnetBlock.mlp weight / bias gradient in one launch (row table built once)
        TrainState& T = *u->train;
        if (!T.mlp_rows) {
            std::vector<float*> rows(2 * (size_t)u->ss_total);
            for (auto& pr : u->resnets) {
                const ResBlock& R = *pr.second;
                float* gw = t.grad(pr.first + ".mlp.1.weight");
                float* gb = t.grad(pr.first + ".mlp.1.bias");
                for (int o = 0; o < 2 * R.dout; ++o) {
                    rows[R.ss_off + o] = gw + (size_t)o * td;
                    rows[u->ss_total + R.ss_off + o] = gb + o;
                }
            }
            DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.mlp_rows), rows.size() * sizeof(float*)));
            DM_CHECK_HIP(hipMemcpy(T.mlp_rows, rows.data(), rows.size() * sizeof(float*), hipMemcpyHostToDevice));
        }
        if (launch_mlp_rows_wgrad(dss, u->ss_total, tp.tfinal, td, T.mlp_rows, T.mlp_rows + u->ss_total, B, td, u->ss_total,
                                  t.acc, s, tp.tact))
            return 1;
    }
    if (launch_linear_dgrad(dss, u->ss_total, u->ss_w, dtf0, td, B, td, u->ss_total, dgw, s)) return 1;  // d silu(tfinal)
    if (launch_act_bwd(dtf0, tp.tfinal, dtf, (int64_t)B * td, 1, s)) return 1;
    const float* dtemb = dtf;  // gradient of time_mlp's output, rows ldt floats apart
    int ldt = td;
    if (text_concat) {
        const int E = cfg.text_emb_dim;
        const float* dtc = dtf;  // what text_concat_proj's output receives
        if (tp.mask) {
            // per-image caption dropout: rows with mask 0 took the raw time embedding, so their gradient bypasses the text
            // branch -- the branch receives exact zeros for them, and below they take dtf itself as time_mlp's gradient
            if (launch_route_rows(dtc_kept, td, dtf, td, nullptr, 0, tp.mask, B, td, s)) return 1;
            dtc = dtc_kept;
        }
        if (launch_linear_wgrad(dtc, td, tp.cat, 2 * td, t.grad("text_concat_proj.weight"), B, 2 * td, td, 0, t.acc, s)) return 1;
        if (launch_colsum(dtc, B, td, td, 1, cw, t.grad("text_concat_proj.bias"), t.acc, s)) return 1;
        if (launch_linear_dgrad(dtc, td, u->tc_w, dcat, 2 * td, B, 2 * td, td, nullptr, s)) return 1;
        if (tp.mask && launch_route_rows(dcat, 2 * td, dcat, 2 * td, dtf, td, tp.mask, B, td, s)) return 1;  // the left half
        const float* dte = dcat + td;  // right half: text_proj's output
        if (launch_linear_wgrad(dte, 2 * td, tp.te0, td, t.grad("text_proj.2.weight"), B, td, td, 0, t.acc, s)) return 1;
        if (launch_colsum(dte, B, td, 2 * td, 1, cw, t.grad("text_proj.2.bias"), t.acc, s)) return 1;
        if (launch_linear_dgrad(dte, 2 * td, u->tp_w2, dte0, td, B, td, td, nullptr, s)) return 1;
        if (launch_act_bwd(dte0, tp.te0pre, dte0pre, (int64_t)B * td, 2, s)) return 1;
        if (launch_linear_wgrad(dte0pre, td, tp.ctx, E, t.grad("text_proj.0.weight"), B, E, td, 0, t.acc, s)) return 1;
        if (launch_colsum(dte0pre, B, td, td, 1, cw, t.grad("text_proj.0.bias"), t.acc, s)) return 1;
        dtemb = dcat;  // left half
        ldt = 2 * td;
    }
    if (launch_linear_wgrad(dtemb, ldt, tp.h1, td, t.grad("time_mlp.3.weight"), B, td, td, 0, t.acc, s)) return 1;
    if (launch_colsum(dtemb, B, td, ldt, 1, cw, t.grad("time_mlp.3.bias"), t.acc, s)) return 1;
    if (launch_linear_dgrad(dtemb, ldt, u->tw2, dh1, td, B, td, td, nullptr, s)) return 1;
    if (launch_act_bwd(dh1, tp.h1pre, dh1pre, (int64_t)B * td, 2, s)) return 1;
    const int fdim = tp.e0_dim;
    if (launch_linear_wgrad(dh1pre, td, tp.e0, fdim, t.grad("time_mlp.1.weight"), B, fdim, td, 0, t.acc, s)) return 1;
    if (launch_colsum(dh1pre, B, td, td, 1, cw, t.grad("time_mlp.1.bias"), t.acc, s)) return 1;
    if (ft) {
        // fdim = learned_sinusoidal_dim + 1 is odd: launch_linear_dgrad takes its scalar kernel (rows_gemm_nn_ok wants I % 64 == 0)
        if (launch_linear_dgrad(dh1pre, td, u->tw1, de0, fdim, B, fdim, td, nullptr, s)) return 1;
        if (launch_sinusoid_ft_bwd(de0, tp.e0, t.grad("time_mlp.0.weights"), B, cfg.learned_sinusoidal_dim / 2,
                                   !u->train->freqs_frozen, t.acc, s))
            return 1;
        if (ig && launch_sinusoid_ft_tgrad(de0, tp.e0, u->freqs, ig->dt, B, cfg.learned_sinusoidal_dim / 2, s)) return 1;
    }
    return 0;
}

static int unet_train_backward_impl(dm_unet* u, Arena& A, const float* x_nchw, const float* dout_nchw, int B, int H, int W,
                                    hipStream_t s, Tape& tp, int accumulate, std::vector<WgradJob>* jobs,
                                    std::vector<WgradDesc>* wbatch, const std::function<int(int)>& phase_done,
                                    const InputGrad* ig) {
    const dm_unet_cfg& cfg = u->cfg;
    const UnetGraph& G = *tp.graph;
    TCtx t{u, &A, s, B, A.dry ? reinterpret_cast<const float*>(16) : tp.ss, u->ss_total};
    t.acc = accumulate;
    t.jobs = jobs;
    t.wbatch = wbatch;
    t.phase_done = phase_done;
    std::vector<RowgradJob> rjobs;
    std::vector<ColsumJob> cjobs;
    t.rjobs = &rjobs;
    t.cjobs = &cjobs;
    float* dss = A.alloc((size_t)B * u->ss_total);
    // final_conv (NCHW gradient, 64 -> out_dim)
    const int h = H, w = W;
    float* dfr = A.alloc((size_t)B * h * w * u->init_dim);
    {
        const ConvLayer& L = u->final_conv;
        const float* wraw = L.packed[CONV_THIN];
        DM_REQUIRE(wraw != nullptr, "training: final_conv must be the thin pointwise layer (out_dim <= 8)");
        static const bool no_fuse = env_flag("DM_TRAIN_NO_FINAL_FUSE");
        if (!no_fuse && thin_out_bwd_ok(L.Cout, h * w)) {  // dw, db and dx in one pass over the block's output
            float* ws = A.alloc(thin_out_bwd_ws_floats(B, h, w, L.Cout, L.C0));
            if (!A.dry) {
                if (ensure_packed(u, wraw, s)) return 1;
                WgradJob *jw = t.defer(), *jb = nullptr;
                if (jw) {  // (the second emplace_back may move the first)
                    jb = t.defer();
                    jw = jb - 1;
                }
                if (launch_thin_out_bwd(tp.val[G.out()], dout_nchw, wraw, dfr, ws, t.grad(L.src.wname), t.grad(L.src.bname), B, h,
                                        w, L.C0, L.Cout, t.acc, s, jw, jb))
                    return 1;
            }
        } else {
            if (conv_wgrad(t, L, tp.val[G.out()], nullptr, dout_nchw, h, w, true)) return 1;
            if (!A.dry && ensure_packed(u, wraw, s)) return 1;
            if (!A.dry && launch_pointwise_small_dgrad(dout_nchw, wraw, dfr, (int64_t)B * h * w, L.C0, L.Cout, h * w, s))
                return 1;
        }
    }
    // The node list in reverse, with the gradient of every value.  A node finds in grad[in0] what a consumer that ran later in
    // the forward pass has already left there (a skip connection's gradient from the up path, x0's from the last node) and
    // adds it to its own; the kernels have no slot for such a gradient on a second input or in front of an attention layer.
    std::vector<float*> grad(G.n_values(), nullptr);
    grad[G.out()] = dfr;
    for (int k = (int)G.nodes.size() - 1; k >= 0; --k) {
        const UnetNode& N = G.nodes[k];
        const NodeTape& nt = tp.nodes[k];
        const int hi = H >> N.lin, wi = W >> N.lin, ho = H >> N.lout, wo = W >> N.lout;
        float *d0 = nullptr, *d1 = nullptr;
        switch (N.kind) {
        case NODE_RESNET:
            DM_REQUIRE(N.in1 < 0 || !grad[N.in1], "backward: a gradient is already waiting for a ResnetBlock's second input");
            if (t_resnet_bwd(t, N.res(), nt.res, grad[N.out], hi, wi, dss, grad[N.in0], &d0, &d1)) return 1;
            if (N.in1 >= 0) grad[N.in1] = d1;
            break;
        case NODE_ATTN:
        case NODE_CROSS:  // a CrossAttention replaced x, so the gradient reaches its input only through to_q
            DM_REQUIRE(!grad[N.in0], "backward: a gradient is already waiting for an attention layer's input");
            if (N.kind == NODE_ATTN ? t_attn_bwd(t, N.attn(), nt.attn, grad[N.out], hi, wi, &d0)
                                    : t_cross_bwd(t, N.cross(), nt.cross, grad[N.out], hi, wi, tp.ctx, tp.ctx_tokens, &d0, tp.mask))
                return 1;
            break;
        case NODE_CONV:
            if (t_conv_bwd(t, N.conv(), tp.val[N.in0], grad[N.out], hi, wi, ho, wo, grad[N.in0], &d0)) return 1;
            break;
        }
        grad[N.in0] = d0;
        // the walk leaves a phase (grad_phase(): a stage): bucketed flush point
        if ((k == 0 || G.nodes[k - 1].phase != N.phase) && t.phase_done && t.phase_done(N.phase)) return 1;
    }
    float* dcur = grad[0];
    // init_conv: weight / bias gradient; its input is data, so the input gradient runs only for a call that asks for it
    if (conv_wgrad(t, u->init_conv, x_nchw, nullptr, dcur, H, W, true)) return 1;
    if (ig && !A.dry) {
        DM_REQUIRE(u->train->init_w_raw != nullptr, "the input gradient needs a handle armed by dm_unet_train_enable_ft");
        if (launch_conv7_dgrad(dcur, u->train->init_w_raw, ig->dx, B, H, W, u->init_dim, cfg.input_channels, s)) return 1;
    }
    // dss is complete once the deferred reductions have run
    if (!A.dry && flush_deferred_reductions(*u->train, rjobs, cjobs, s)) return 1;
    return cond_backward(t, tp, dss, ig);
}

// The backward pass records the MFMA weight gradients instead of running them: they depend only on tensors that stay alive
// (the tape and the dY buffers; nothing is released), so all layers of one mode (3x3, 1x1, Downsample) run as ONE grouped
// launch at the end -- independent layers fill the chip, where a lone 64 -> 64 layer had to split its pixels 256 ways and
// write 38 MB of partial sums -- followed by ONE launch that sums the remaining split-K partial tiles of every layer.
static int unet_train_backward(dm_unet* u, Arena& A, const float* x_nchw, const float* dout_nchw, int B, int H, int W,
                               hipStream_t s, Tape& tp, int accumulate, const InputGrad* ig = nullptr) {
    std::vector<WgradJob> jobs;
    std::vector<WgradDesc> batch[WG_MODES];
    TrainState& T = *u->train;
    int n_flush = 0;
    // run what has been recorded since the last flush: the grouped weight-gradient launches (one per mode) and the launch
    // that sums their split-K partial tiles -- after it the gradients of every convolution weight recorded so far are final
    auto flush = [&]() -> int {
        const int fi = n_flush++;
        if ((int)T.flush.size() <= fi) T.flush.resize(fi + 1);
        TrainState::FlushTables& F = T.flush[fi];
        for (int mode = 0; mode < WG_MODES; ++mode) {
            if (batch[mode].empty()) continue;
            std::vector<int> splits;
            std::vector<size_t> wsf;
            wgrad_group_plan(batch[mode], mode, splits, wsf);
            std::vector<float*> ws(wsf.size());
            for (size_t k = 0; k < wsf.size(); ++k) ws[k] = A.alloc(wsf[k]);
            if (!A.dry) {
                std::vector<WgradParams> table;
                int total = 0;
                size_t lds = 0;
                if (wgrad_group_fill(batch[mode], mode, splits, ws, table, jobs, &total, &lds)) return 1;
                if (upload_table(table, F.wtab_host[mode], F.wtab_dev[mode], F.wtab_cap[mode], s)) return 1;
                if (launch_wgrad_group(F.wtab_dev[mode], (int)table.size(), total, lds, mode, s)) return 1;
            }
            batch[mode].clear();
        }
        if (!A.dry && !jobs.empty()) {
            int total = 0;
            for (WgradJob& jb : jobs) {
                jb.first_block = total;
                const int rp = wgrad_reduce_pairs(jb.T, jb.oc);
                total += (int)((jb.oc + rp - 1) / rp);
            }
            if (upload_table(jobs, F.jobs_host, F.jobs_dev, F.jobs_cap, s)) return 1;
            if (launch_wgrad_reduce_jobs(F.jobs_dev, (int)jobs.size(), total, s)) return 1;
        }
        jobs.clear();
        return 0;
    };
    std::function<int(int)> phase_done;
    if (T.bucketed)
        phase_done = [&](int phase) -> int {  // data-parallel bucketing: a bucket's last phase has just been left
            for (TrainState::Bucket& bk : T.buckets) {
                if (bk.last_phase != phase || &bk == &T.buckets.back()) continue;
                if (flush()) return 1;
                if (!A.dry) DM_CHECK_HIP(hipEventRecord(bk.ready, s));
            }
            return 0;
        };
    if (unet_train_backward_impl(u, A, x_nchw, dout_nchw, B, H, W, s, tp, accumulate, &jobs, batch, phase_done, ig)) return 1;
    if (flush()) return 1;
    if (!A.dry && T.bucketed && !T.buckets.empty()) DM_CHECK_HIP(hipEventRecord(T.buckets.back().ready, s));
    return 0;
}

// ---- device-side re-packing ----------------------------------------------------------------------------------------
// Re-create one packed buffer from the flat master parameters (T.param) with the device mirror of its host packer.
static int run_pack_op(dm_unet* u, TrainState& T, const PackOp& op, hipStream_t s) {
    auto param = [&](const std::string& name) -> const float* {
        auto it = T.off.find(name);
        if (it == T.off.end()) throw std::runtime_error("device re-pack: unknown parameter " + name);
        return T.param + it->second;
    };
    if (op.kind == PK_RAW_NAME) {
        DM_CHECK_HIP(hipMemcpyAsync(op.dst, param(op.name), op.n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    if (op.kind == PK_RAW_B) {
        DM_CHECK_HIP(hipMemcpyAsync(op.dst, param(op.src.bname), op.n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    // the OIHW tensor the packer reads: the parameter itself, or its rotated / transposed form in T.pack_tmp
    const float* w = param(op.src.wname);
    DM_REQUIRE(op.src.kind != PS_UP1D, "device re-pack: the sequence model's Upsample packing has no device mirror");
    if (op.src.kind == PS_ROT) {
        const size_t n = (size_t)op.src.c_n * op.src.sCout * op.src.sK * op.src.sK;
        DM_REQUIRE(n <= T.pack_tmp_floats, "device re-pack: temporary too small");
        if (launch_rot_transpose(w, T.pack_tmp, op.src.sCout, op.src.sCin, op.src.sK, op.src.c_lo, op.src.c_n, s)) return 1;
        w = T.pack_tmp;
    } else if (op.src.kind == PS_S2D_T) {
        const size_t n = (size_t)4 * op.src.sCin * op.src.sCout;
        DM_REQUIRE(n <= T.pack_tmp_floats, "device re-pack: temporary too small");
        if (launch_s2d_transpose(w, T.pack_tmp, op.src.sCout, op.src.sCin, s)) return 1;
        w = T.pack_tmp;
    }
    if (op.kind == PK_FOLD) {
        // four 2x2 parity convolutions, each packed like a direct convolution; the taps are summed into the second
        // half of the temporary
        const int Cin = op.C0 + op.C1;
        const size_t per = conv_packed_floats(op.Cout, op.C0, op.C1, 2, 2);
        const size_t w2n = (size_t)op.Cout * Cin * 4;
        DM_REQUIRE(op.src.kind == PS_STORED && w2n <= T.pack_tmp_floats, "device re-pack: folded upsample conv");
        for (int q = 0; q < 4; ++q) {
            if (launch_fold_taps(w, T.pack_tmp, op.Cout, Cin, q >> 1, q & 1, s)) return 1;
            if (launch_pack_direct(T.pack_tmp, op.dst + q * per, op.Cout, op.C0, op.C1, 2, 2, s)) return 1;
        }
        return 0;
    }
    const ConvRecipe* R = conv_recipe_of(op.kind);
    DM_REQUIRE(R, "device re-pack: unknown packing kind");
    return R->device_pack(w, op.dst, op.Cout, op.C0, op.C1, op.KH, op.KW, s);
}

static bool is_raw_copy(const PackOp& op) { return op.kind == PK_RAW_NAME || op.kind == PK_RAW_B; }

// (re)build the buffer -> recipe index and the device table of the raw copies; called whenever the recipes change
static int index_pack_ops(dm_unet* u) {
    TrainState& T = *u->train;
    T.op_of.clear();
    T.stale_f.assign(u->pack_ops.size(), 0);
    T.stale_b.assign(T.ops.size(), 0);
    T.used_f.assign(u->pack_ops.size(), 0);
    T.used_b.assign(T.ops.size(), 0);
    T.used_version += 1;
    std::vector<TrainState::CopyEntry> table;
    T.max_copy = 0;
    auto add = [&](const std::vector<PackOp>& ops, int which) {
        for (size_t i = 0; i < ops.size(); ++i) {
            const PackOp& op = ops[i];
            if (is_raw_copy(op)) {
                const std::string& name = op.kind == PK_RAW_NAME ? op.name : op.src.bname;
                auto it = T.off.find(name);
                if (it == T.off.end()) throw std::runtime_error("device re-pack: unknown parameter " + name);
                table.push_back(TrainState::CopyEntry{(long long)it->second, op.dst, (long long)op.n});
                T.max_copy = std::max<long long>(T.max_copy, (long long)op.n);
            } else {
                T.op_of[op.dst] = {which, (int)i};
            }
        }
    };
    add(u->pack_ops, 0);
    add(T.ops, 1);
    if (T.copy_table) (void)hipFree(T.copy_table);
    T.copy_table = nullptr;
    T.n_copies = (int)table.size();
    if (!table.empty()) {
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.copy_table), table.size() * sizeof(TrainState::CopyEntry)));
        DM_CHECK_HIP(hipMemcpy(T.copy_table, table.data(), table.size() * sizeof(TrainState::CopyEntry), hipMemcpyHostToDevice));
    }
    return 0;
}

// the grouped form of run_pack_op for the layouts pack_jobs_kernel knows: level-0 job (rotated / transposed source into
// `tmp`) and level-1 job (the pack); false: the recipe stays on the lazy path
static bool pack_jobs_of(TrainState& T, const PackOp& op, float* tmp, size_t* tmp_floats, std::vector<PackJob>* lv) {
    const ConvFamily* F = nullptr;
    const ConvRecipe* R = conv_recipe_of(op.kind, &F);
    if (!R || F->pj < 0) return false;
    const int kind = F->pj;
    const int Cin = R->s2d ? 4 * op.C0 : op.C0 + op.C1;
    // the grouped kernel walks the packed layout: whole chunks / cout tiles only (what the kernels' dispatch requires anyway)
    if (Cin % F->cin_mult != 0 || op.Cout % F->cout_mult != 0) return false;
    auto it = T.off.find(op.src.wname);
    if (it == T.off.end()) return false;
    const float* w = T.param + it->second;
    *tmp_floats = 0;
    static const bool rot_tmp = env_flag("DM_REPACK_ROT_TMP");  // A/B: materialise the rotated weights first
    int rs = 0, rc = 0;
    if (op.src.kind == PS_ROT && !rot_tmp && !R->s2d && op.src.sK == F->rot_k) {
        rs = op.src.sCin;  // the pack reads the rotated pair in place
        rc = op.src.c_lo;
    } else if (op.src.kind == PS_ROT) {
        const long long n = (long long)op.src.c_n * op.src.sCout * op.src.sK * op.src.sK;
        if (lv) lv[0].push_back(PackJob{w, tmp, n, PJ_ROT, op.src.sCout, op.src.sCin, op.src.sK, op.src.c_lo, 0});
        *tmp_floats = (size_t)n;
        w = tmp;
    } else if (op.src.kind == PS_S2D_T) {
        const long long n = (long long)4 * op.src.sCin * op.src.sCout;
        if (lv) lv[0].push_back(PackJob{w, tmp, n, PJ_S2D_T, op.src.sCout, op.src.sCin, 0, 0, 0});
        *tmp_floats = (size_t)n;
        w = tmp;
    }
    if (!lv) return true;
    if (kind == PJ_COPY)
        lv[1].push_back(PackJob{w, op.dst, (long long)op.n, PJ_COPY, 0, 0, 0, 0, 0});
    else
        lv[1].push_back(PackJob{w, op.dst, (long long)op.Cout * Cin, kind, op.Cout, Cin, R->s2d ? op.C0 : 0, 0, 0, rs, rc});
    return true;
}

// rebuild every used buffer of a known layout in two grouped launches
static int batched_repack(dm_unet* u, hipStream_t s) {
    static const bool off = env_flag("DM_NO_BATCH_REPACK");  // A/B: everything on the lazy path
    TrainState& T = *u->train;
    if (off) return 0;
    if (T.jobs_version != T.used_version) {
        auto each = [&](auto&& fn) {
            for (size_t i = 0; i < u->pack_ops.size(); ++i)
                if (T.used_f[i] && !is_raw_copy(u->pack_ops[i])) fn(u->pack_ops[i], 0, (int)i);
            for (size_t i = 0; i < T.ops.size(); ++i)
                if (T.used_b[i] && !is_raw_copy(T.ops[i])) fn(T.ops[i], 1, (int)i);
        };
        size_t need = 0;
        each([&](const PackOp& op, int, int) {
            size_t n = 0;
            if (pack_jobs_of(T, op, nullptr, &n, nullptr)) need += (n + 63) & ~size_t(63);
        });
        if (need > T.big_tmp_floats) {
            DM_CHECK_HIP(hipStreamSynchronize(s));
            if (T.big_tmp) (void)hipFree(T.big_tmp);
            T.big_tmp = nullptr;
            T.big_tmp_floats = 0;
            DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.big_tmp), need * sizeof(float)));
            T.big_tmp_floats = need;
        }
        std::vector<PackJob> lv[2];
        T.pk_ops.clear();
        size_t at = 0;
        each([&](const PackOp& op, int list, int idx) {
            size_t n = 0;
            if (!pack_jobs_of(T, op, T.big_tmp + at, &n, lv)) return;
            at += (n + 63) & ~size_t(63);
            T.pk_ops.emplace_back(list, idx);
        });
        for (int l = 0; l < 2; ++l) {
            T.pk_blocks[l] = pack_jobs_prefix(lv[l]);
            if (!lv[l].empty() && upload_table(lv[l], T.pk_host[l], T.pk_dev[l], T.pk_cap[l], s)) return 1;
            if (lv[l].empty()) T.pk_host[l].clear();
        }
        T.jobs_version = T.used_version;
    }
    for (int l = 0; l < 2; ++l)
        if (launch_pack_jobs(T.pk_dev[l], (int)T.pk_host[l].size(), T.pk_blocks[l], s)) return 1;
    for (const auto& pr : T.pk_ops) (pr.first == 0 ? T.stale_f : T.stale_b)[pr.second] = 0;
    return 0;
}

// after an optimiser step: raw copies (one kernel) and the packed weights the step has been using (two launches) now, any
// other packed convolution weight when first used
static int device_repack(dm_unet* u, hipStream_t s) {
    TrainState& T = *u->train;
    if (T.op_of.empty() && T.n_copies == 0 && index_pack_ops(u)) return 1;
    if (T.n_copies && launch_scatter_copy(T.param, T.copy_table, T.n_copies, T.max_copy, s)) return 1;
    std::fill(T.stale_f.begin(), T.stale_f.end(), 1);
    std::fill(T.stale_b.begin(), T.stale_b.end(), 1);
    return batched_repack(u, s);
}

// called in front of every convolution of the training step: rebuild its weight buffer if an optimiser step made it stale
static int ensure_packed(dm_unet* u, const float* w, hipStream_t s) {
    TrainState* T = u->train;
    if (!T || !T->param || T->op_of.empty()) return 0;
    auto it = T->op_of.find(w);
    if (it == T->op_of.end()) return 0;
    char& stale = it->second.first == 0 ? T->stale_f[it->second.second] : T->stale_b[it->second.second];
    char& used = it->second.first == 0 ? T->used_f[it->second.second] : T->used_b[it->second.second];
    if (!used) {
        used = 1;
        T->used_version += 1;
    }
    if (!stale) return 0;
    const PackOp& op = it->second.first == 0 ? u->pack_ops[it->second.second] : T->ops[it->second.second];
    if (run_pack_op(u, *T, op, s)) return 1;
    stale = 0;
    return 0;
}

// upload the host parameters into the flat master buffer (first use, and after a host-side refresh)
static int upload_master(dm_unet* u) {
    TrainState& T = *u->train;
    if (!T.param) {
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.param), T.grad_floats * sizeof(float)));
        DM_CHECK_HIP(hipMemset(T.param, 0, T.grad_floats * sizeof(float)));
        size_t tmp = 4;
        for (const std::string& name : u->order) tmp = std::max(tmp, P(u, name).numel());
        T.pack_tmp_floats = tmp;
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.pack_tmp), tmp * sizeof(float)));
    }
    for (const std::string& name : u->order) {
        const HostTensor& t = P(u, name);
        DM_CHECK_HIP(hipMemcpy(T.param + T.off.at(name), t.data.data(), t.numel() * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}

static int upload_master_if_resident(dm_unet* u) { return (u->train && u->train->param) ? upload_master(u) : 0; }

void free_train(dm_unet* u) {
    delete u->train;
    u->train = nullptr;
}

static int ensure_train_ws(TrainState& T, size_t bytes) {
    if (bytes <= T.ws_cap) return 0;
    DM_CHECK_HIP(hipDeviceSynchronize());
    if (T.ws) (void)hipFree(T.ws);
    T.ws = nullptr;
    T.ws_cap = 0;
    void* p = nullptr;
    DM_CHECK_HIP(hipMalloc(&p, bytes));
    T.ws = static_cast<char*>(p);
    T.ws_cap = bytes;
    return 0;
}

// the per-image device rows (coefficients at the widest row, integer and float times, text mask) hold B images
static int grow_train_rows(TrainState& T, int B) {
    if (B <= T.cap_B) return 0;
    DM_CHECK_HIP(hipDeviceSynchronize());
    for (void** q : {(void**)&T.coef_dev, (void**)&T.t_dev, (void**)&T.tf_dev, (void**)&T.mask_dev}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    T.cap_B = 0;
    static_assert(DM_EDM_COEFS >= DM_TRAIN_COEFS, "the rows are sized for the widest entry");
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.coef_dev), (size_t)B * DM_EDM_COEFS * sizeof(float)));
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.t_dev), (size_t)B * sizeof(int64_t)));
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.tf_dev), (size_t)B * sizeof(float)));
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.mask_dev), (size_t)B * sizeof(int32_t)));
    T.cap_B = B;
    return 0;
}

// ---- one loss + backward call -------------------------------------------------------------------------------------------
// What every training entry (DDPM, learned variance, weighted objective, ElucidatedDiffusion, continuous time) hands
// run_train once its own argument checks have passed.  An entry keeps what is its own: those checks and run(arena, tape)
// -- its noise-in pass, tape forward, loss kernel and backward pass, reading T.coef_dev / t_dev / tf_dev / mask_dev.
enum TrainEntry : long long { TRAIN_DDPM, TRAIN_EDM, TRAIN_CT, TRAIN_LV, TRAIN_WO };
namespace {
struct TrainRun {
    TrainEntry entry = TRAIN_DDPM;
    std::array<long long, 4> sel{};  // whatever else selects the entry's allocation sequence (workspace key, below)
    int B = 0, H = 0, W = 0;
    void* stream = nullptr;
    float* loss_out_host = nullptr;  // nullptr: the loss stays on the device (dm_unet_train_scalar)
    const float* coef_host = nullptr;  // B rows of `cstride` floats; on the device a row is `width` floats, zero-extended
    int cstride = 0, width = 0;
    int tf_col = -1;                   // >= 0: this column of every row is also the image's float time (tf_dev)
    const int64_t* t_host = nullptr;   // integer timesteps (t_dev)
    const int32_t* text_mask = nullptr;  // per-image text mask (mask_dev)
};
}  // namespace

// The call itself: device, per-image rows, workspace (sized by a dry run of `run`, once per key: entry, shape, bucketing
// and r.sel), ordering behind the handle's previous call, the uploads, the real run on an arena over the workspace, the
// dropout call counter -- advanced by a call that succeeded, and only by that --, then the handle's done mark and the
// optional loss read-back, which waits for the stream.
static int run_train(dm_unet* u, const TrainRun& r, const std::function<int(Arena&, Tape&)>& run) {
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(r.stream);
    TrainState& T = *u->train;
    const int B = r.B;
    const size_t n_coef = (size_t)B * r.width;
    if (guarded([&]() -> int {
            if (grow_train_rows(T, B)) return 1;
            const std::array<long long, 9> key{r.entry, B, r.H, r.W, T.bucketed ? 1 : 0, r.sel[0], r.sel[1], r.sel[2], r.sel[3]};
            auto known = T.ws_need.find(key);
            if (known == T.ws_need.end()) {
                Arena dry;
                dry.dry = true;
                Tape tp;
                if (run(dry, tp)) return 1;
                known = T.ws_need.emplace(key, dry.off).first;
            }
            if (ensure_train_ws(T, known->second)) return 1;
            if (u->order_after_previous(s)) return 1;  // e.g. an optimiser step enqueued on another stream
            T.coef_stage.assign(n_coef + (r.tf_col >= 0 ? B : 0), 0.f);
            const int ncopy = std::min(r.cstride, r.width);
            for (int b = 0; b < B; ++b) {
                std::memcpy(&T.coef_stage[(size_t)b * r.width], r.coef_host + (size_t)b * r.cstride, ncopy * sizeof(float));
                if (r.tf_col >= 0) T.coef_stage[n_coef + b] = r.coef_host[(size_t)b * r.cstride + r.tf_col];
            }
            DM_CHECK_HIP(hipMemcpyAsync(T.coef_dev, T.coef_stage.data(), n_coef * sizeof(float), hipMemcpyHostToDevice, s));
            if (r.t_host) DM_CHECK_HIP(hipMemcpyAsync(T.t_dev, r.t_host, (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice, s));
            if (r.tf_col >= 0)
                DM_CHECK_HIP(hipMemcpyAsync(T.tf_dev, T.coef_stage.data() + n_coef, (size_t)B * sizeof(float), hipMemcpyHostToDevice, s));
            if (r.text_mask)
                DM_CHECK_HIP(hipMemcpyAsync(T.mask_dev, r.text_mask, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
            Arena A;
            A.base = T.ws;
            A.cap = T.ws_cap;
            Tape tp;
            if (run(A, tp)) return 1;
            T.drop_call += 1;
            DM_REQUIRE(A.off <= T.ws_cap, "training workspace overrun: the dry run and the real run allocated differently");
            return 0;
        }))
        return 1;
    if (u->mark_done(s)) return 1;
    if (!r.loss_out_host) return 0;
    DM_CHECK_HIP(hipMemcpyAsync(r.loss_out_host, T.loss_dev, sizeof(float), hipMemcpyDeviceToHost, s));
    DM_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // namespace dm

extern "C" {

// ft: the handle is armed for float-time training (dm_unet_train_enable_ft) instead of the integer-time p_losses path
static int train_enable_impl(dm_unet* u, bool ft) {
    DM_REQUIRE(!u->cfg.seq1d, "training the sequence model (Unet1D: loss, backward pass, Trainer1D) is not on the HIP path yet: "
                              "a seq1d handle serves dm_unet_forward and the sampling loops");
    DM_REQUIRE(!u->kunet, "training KarrasUnet (forced weight normalisation in the training forward, the backward of its "
                          "operators) is not on the HIP path yet: the handle serves dm_unet_forward_ft and dm_sample_edm");
    DM_CHECK_HIP(hipSetDevice(u->device));
    if (u->train) {
        DM_REQUIRE(u->train->ft == ft, "the handle is already in training mode through the other entry "
                                       "(dm_unet_train_enable / dm_unet_train_enable_ft)");
        return 0;
    }
    u->train = new TrainState();
    TrainState& T = *u->train;
    T.ft = ft;
    if (build_train(u)) {  // also collects T.conv_weights
        free_train(u);
        return 1;
    }
    // Flat layout of the gradients (and of the master parameters, Adam moments, EMA copy): bucket by bucket.  A bucket is
    // closed when the convolution weights of the phases walked so far reach DM_TRAIN_BUCKET_MB (default 25, torch DDP's
    // bucket_cap_mb); the last bucket takes every other parameter too.  Offsets are looked up by name everywhere, so the
    // order is free; it is a function of the configuration only (every rank lays its buffers out alike).
    static const size_t cap_floats = (size_t)env_int("DM_TRAIN_BUCKET_MB", 25) * (1u << 20) / sizeof(float);
    const int last_phase = 2 * u->cfg.n_stages + 2;
    auto padded = [&](const std::string& name) { return (P(u, name).numel() + 3) & ~size_t(3); };
    std::vector<size_t> phase_floats(last_phase + 1, 0);
    for (const std::string& name : u->order)
        if (T.conv_weights.count(name)) phase_floats[grad_phase(u, name)] += padded(name);
    std::vector<int> bucket_of_phase(last_phase + 1, 0);
    {
        int b = 0;
        size_t acc = 0;
        for (int ph = 0; ph <= last_phase; ++ph) {
            bucket_of_phase[ph] = b;
            acc += phase_floats[ph];
            if (acc >= cap_floats && ph < last_phase) {  // close the bucket behind this phase
                T.buckets.emplace_back();
                T.buckets.back().last_phase = ph;
                b += 1;
                acc = 0;
            }
        }
        T.buckets.emplace_back();
        T.buckets.back().last_phase = last_phase;
    }
    const int tail = (int)T.buckets.size() - 1;
    size_t off = 0;
    for (int b = 0; b <= tail; ++b) {
        T.buckets[b].off = off;
        for (const std::string& name : u->order) {
            const int nb = T.conv_weights.count(name) ? bucket_of_phase[grad_phase(u, name)] : tail;
            if (nb != b) continue;
            T.off[name] = off;
            off += padded(name);
        }
        T.buckets[b].n = off - T.buckets[b].off;
        DM_CHECK_HIP(hipEventCreateWithFlags(&T.buckets[b].ready, hipEventDisableTiming));
    }
    T.grad_floats = off;
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.grad), off * sizeof(float)));
    DM_CHECK_HIP(hipMemset(T.grad, 0, off * sizeof(float)));
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.loss_dev), 256));
    return 0;
}

int dm_unet_train_enable(dm_unet* u) {
    DM_REQUIRE(u && u->finalized, "dm_unet_train_enable needs a finalized handle");
    DM_REQUIRE(u->cfg.learned_sinusoidal_dim == 0,
               "the random / learned sinusoidal embedding is forward-only: DenoisingDiffusion (hence p_losses) refuses such a U-Net");
    return train_enable_impl(u, false);
}

/* Data-parallel gradient buckets (torch DDP's bucketed all-reduce, DD/denoising_diffusion.py:971-974 via accelerate): with
 * enable != 0 every later dm_unet_loss_backward runs the weight gradients of a bucket as soon as the backward pass has
 * left the bucket's stages and records an event; dm_unet_train_bucket gives bucket i's span of the flat gradient buffer
 * (floats) and makes `stream` wait for that event, so a collective enqueued on it runs BESIDE the rest of the pass.  Returns
 * the number of buckets (>= 1; the last one is complete only at the end of the pass), -1 on error. */
int dm_unet_train_buckets(dm_unet* u, int enable) {
    if (!u || !u->train) return -1;
    u->train->bucketed = enable != 0;
    return (int)u->train->buckets.size();
}
int dm_unet_train_bucket(dm_unet* u, int i, int64_t* off_out, int64_t* n_out, int wait, void* wait_stream) {
    DM_REQUIRE(u && u->train && off_out && n_out && i >= 0 && i < (int)u->train->buckets.size(), "dm_unet_train_bucket: bad argument");
    TrainState::Bucket& b = u->train->buckets[i];
    *off_out = (int64_t)b.off;
    *n_out = (int64_t)b.n;
    if (wait) {
        DM_REQUIRE(u->train->bucketed, "dm_unet_train_bucket: bucketing is off (dm_unet_train_buckets)");
        DM_CHECK_HIP(hipSetDevice(u->device));
        DM_CHECK_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(wait_stream), b.ready, 0));
    }
    return 0;
}

int64_t dm_unet_grad_floats(dm_unet* u) { return (u && u->train) ? (int64_t)u->train->grad_floats : -1; }

/* the flat gradient buffer itself (device pointer, floats): data-parallel training all-reduces it in place -- ONE collective
 * over RCCL for all 245 gradients -- between the last dm_unet_loss_backward of an iteration and dm_unet_optimizer_step */
int dm_unet_grads_flat(dm_unet* u, float** ptr_out, int64_t* n_out) {
    DM_REQUIRE(u && u->train && ptr_out && n_out, "dm_unet_grads_flat needs a handle in training mode");
    *ptr_out = u->train->grad;
    *n_out = (int64_t)u->train->grad_floats;
    return 0;
}

/* copy the gradient of one parameter (reference layout) to a DEVICE buffer */
int dm_unet_get_grad(dm_unet* u, const char* name, float* out_dev, void* stream) {
    DM_REQUIRE(u && name && out_dev && u->train, "dm_unet_get_grad needs a handle in training mode");
    auto it = u->train->off.find(name);
    if (it == u->train->off.end()) {
        set_error(std::string("unknown parameter: ") + name);
        return 1;
    }
    if (u->order_after_previous(static_cast<hipStream_t>(stream))) return 1;
    DM_CHECK_HIP(hipMemcpyAsync(out_dev, u->train->grad + it->second, P(u, name).numel() * sizeof(float),
                                hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return 0;
}

static int loss_backward_impl(dm_unet* u, const dm_train_args& a, const int32_t* text_mask = nullptr) {
    const float *x_start = a.x_start, *coef_host = a.coef_host, *noise = a.noise, *noise_q = a.noise_q, *cond = a.cond,
                *ctx = a.ctx;
    const int64_t* t_host = a.t_host;
    const int cond_channels = a.cond_channels, ctx_tokens = a.ctx_tokens, self_cond = a.self_cond, objective = a.objective,
              accumulate = a.accumulate, B = a.B, H = a.H, W = a.W;
    const float loss_scale = a.loss_scale;
    float *loss_out_host = a.loss_out_host, *model_out = a.model_out;
    void* stream = a.stream;
    const int terms = a.loss_terms ? a.loss_terms : 1;
    const int cstride = a.coef_stride ? a.coef_stride : 8;
    DM_REQUIRE(u && x_start && t_host && coef_host && noise, "null argument");
    DM_REQUIRE(u->train, "dm_unet_train_enable has not been called");
    DM_REQUIRE(!u->train->ft, "the handle is armed for float-time training (dm_unet_train_enable_ft): an integer timestep would "
                              "truncate c_noise(sigma) -- use dm_unet_loss_backward_edm");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    DM_REQUIRE(u->out_dim != 2 * u->cfg.channels, "the U-Net predicts a learned variance (out_dim == 2 * channels): its loss is "
                                                  "dm_unet_loss_backward_lv");
    DM_REQUIRE(u->out_dim != 2 * u->cfg.channels + 2, "the U-Net predicts noise, x_start and two weight maps (out_dim == 2 * channels + 2): "
                                                      "its loss is dm_unet_loss_backward_wo");
    DM_REQUIRE(B > 0 && objective >= DM_OBJ_PRED_NOISE && objective <= DM_OBJ_PRED_V, "bad argument");
    DM_REQUIRE(terms >= 1 && terms <= 3 && cstride >= 8 && cstride <= DM_TRAIN_COEFS && (!(terms & 2) || cstride == DM_TRAIN_COEFS),
               "loss_terms is 1 (MSE), 2 (KL) or 3 (both); the KL term needs coef rows of 12 floats");
    DM_REQUIRE((cond == nullptr) == (cond_channels == 0) && cond_channels >= 0, "cond and cond_channels come together");
    DM_REQUIRE(self_cond >= 0 && self_cond <= 2 && !(self_cond && cond), "self_cond: 0 off, 1 zeros, 2 predicted x_start; not with cond");
    DM_REQUIRE((ctx == nullptr) == (ctx_tokens == 0) && ctx_tokens >= 0, "ctx and ctx_tokens come together");
    DM_REQUIRE(!ctx || u->cfg.text_mode != DM_TEXT_NONE, "the U-Net was built without text conditioning");
    DM_REQUIRE(!text_mask || ctx, "text_mask needs ctx: without captions there is nothing to drop");
    DM_REQUIRE(u->cfg.input_channels == u->cfg.channels * (self_cond ? 2 : 1) + cond_channels && u->out_dim == u->cfg.channels,
               "training path: U-Net input channels != channels [* 2 with self-conditioning] + cond_channels");
    if (check_hw(u, H, W)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrainState& T = *u->train;
    const int C = u->cfg.channels;
    const int per = C * H * W;
    const size_t n = (size_t)B * per;
    auto run = [&](Arena& A, Tape& tp) -> int {
        if (!A.dry && !accumulate && !ctx && u->cfg.text_mode != DM_TEXT_NONE) {
            // text_emb=None on a text-conditional U-Net (caption dropout): the pass visits no text parameter, and with
            // accumulate == 0 every other gradient is overwritten -- torch leaves these .grad None, here they must not keep
            // the values of an earlier call with captions
            for (const std::string& name : u->order)
                if (name.compare(0, 5, "text_") == 0 || name.compare(0, 10, "cross_attn") == 0)
                    DM_CHECK_HIP(hipMemsetAsync(T.grad + T.off.at(name), 0, P(u, name).numel() * sizeof(float), s));
        }
        const int32_t* mask = text_mask ? T.mask_dev : nullptr;  // the same mask in every forward pass of the call
        float* x = A.alloc(n);
        float* out = A.alloc(n);
        float* dout = A.alloc(n);
        float* part = A.alloc(B);
        float* klpart = A.alloc(B);
        const float* xq = x;  // the q_sample output (before self-conditioning / the condition image join it)
        if (!A.dry && launch_q_sample(x_start, noise_q ? noise_q : noise, T.coef_dev, x, B, per, s)) return 1;
        if (self_cond) {
            // Unet(self_condition=True) sees [x_self_cond | x] (:352-354).  p_losses (:846-855) conditions on zeros or, for
            // half of the iterations, on the x_start a gradient-free forward pass predicts from [0 | x] (unclipped, :849)
            const size_t n2 = (size_t)B * 2 * C * H * W;
            float* xin = A.alloc(n2);
            if (!A.dry) {
                DM_CHECK_HIP(hipMemsetAsync(xin, 0, n2 * sizeof(float), s));
                if (launch_copy_channels(x, xin, B, C, 2 * C, C, H * W, s)) return 1;
            }
            if (self_cond == 2) {
                Tape tp0;
                float* out0 = A.alloc(n);
                float* xs = A.alloc(n);
                TrainState& TT = *u->train;
                const uint64_t call = TT.drop_call;
                TT.drop_call = call | (1ull << 40);  // the gradient-free pass draws its own dropout masks
                const int rc = unet_train_forward(u, A, xin, T.t_dev, out0, B, H, W, s, tp0, ctx, ctx_tokens, mask);
                TT.drop_call = call;
                if (rc) return 1;
                if (!A.dry && (launch_pred_x_start(x, out0, T.coef_dev, xs, B, per, objective, s) ||
                               launch_copy_channels(xs, xin, B, C, 2 * C, 0, H * W, s)))
                    return 1;
            }
            x = xin;
        }
        if (cond) {  // the image-conditional U-Net sees [x | cond] (DD/denoising_diffusion_image_conditional.py:51-55)
            float* xin = A.alloc((size_t)B * (C + cond_channels) * H * W);
            if (!A.dry && (launch_copy_channels(x, xin, B, C, C + cond_channels, 0, H * W, s) ||
                           launch_copy_channels(cond, xin, B, cond_channels, C + cond_channels, C, H * W, s)))
                return 1;
            x = xin;
        }
        if (unet_train_forward(u, A, x, T.t_dev, out, B, H, W, s, tp, ctx, ctx_tokens, mask)) return 1;
        if (!A.dry) {
            if (launch_mse_loss(out, x_start, noise, T.coef_dev, dout, part, T.loss_dev, B, per, objective, loss_scale, s, terms,
                                xq, klpart, a.kl_scale))
                return 1;
            if (model_out) DM_CHECK_HIP(hipMemcpyAsync(model_out, out, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        return unet_train_backward(u, A, x, dout, B, H, W, s, tp, accumulate);
    };
    TrainRun r;
    r.entry = TRAIN_DDPM;
    r.sel = {self_cond, cond_channels, ctx_tokens, (ctx ? 1 : 0) | (model_out ? 2 : 0) | (text_mask ? 4 : 0)};
    r.B = B; r.H = H; r.W = W; r.stream = stream; r.loss_out_host = loss_out_host;
    r.coef_host = coef_host; r.cstride = cstride; r.width = DM_TRAIN_COEFS;
    r.t_host = t_host; r.text_mask = text_mask;
    return run_train(u, r, run);
}

int dm_unet_loss_backward(dm_unet* u, const float* x_start, const int64_t* t_host, const float* coef_host, const float* noise,
                          const float* noise_q, const float* cond, int cond_channels, const float* ctx, int ctx_tokens, int self_cond, int objective,
                          float loss_scale, int accumulate, float* loss_out_host, float* model_out, int B, int H, int W,
                          void* stream) {
    dm_train_args a{};
    a.x_start = x_start; a.t_host = t_host; a.coef_host = coef_host; a.coef_stride = 8; a.noise = noise; a.noise_q = noise_q;
    a.cond = cond; a.cond_channels = cond_channels; a.ctx = ctx; a.ctx_tokens = ctx_tokens; a.self_cond = self_cond;
    a.objective = objective; a.loss_scale = loss_scale; a.accumulate = accumulate; a.loss_out_host = loss_out_host;
    a.model_out = model_out; a.B = B; a.H = H; a.W = W; a.stream = stream; a.loss_terms = 1;
    return loss_backward_impl(u, a);
}

int dm_unet_loss_backward_ex(dm_unet* u, const dm_train_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return loss_backward_impl(u, *a);
}

int dm_unet_loss_backward_masked(dm_unet* u, const dm_train_args* a, const int32_t* text_mask) {
    DM_REQUIRE(u && a && text_mask, "null argument");
    return loss_backward_impl(u, *a, text_mask);
}

/* The scalars of the training loop without a host round trip: which = 0 the loss of the last dm_unet_loss_backward, 1 the
 * total gradient norm of the last dm_unet_optimizer_step (before clipping), copied to a DEVICE float on `stream`.  With
 * loss_out_host / grad_norm_out_host == NULL those calls return as soon as their kernels are enqueued, as the reference's
 * loop does until it calls loss.item() (:1173). */
int dm_unet_train_scalar(dm_unet* u, int which, float* out_dev, void* stream) {
    DM_REQUIRE(u && u->train && out_dev && (which == 0 || which == 1), "dm_unet_train_scalar: bad argument");
    TrainState& T = *u->train;
    DM_REQUIRE(which == 0 || T.clip2, "no optimiser step yet (dm_unet_optimizer_step)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (u->order_after_previous(s)) return 1;
    DM_CHECK_HIP(hipMemcpyAsync(out_dev, which == 0 ? T.loss_dev : T.clip2, sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

/* The optimiser step of Trainer.train (DD/denoising_diffusion.py:1006, :1178-1183): clip_grad_norm_(max_grad_norm), Adam
 * on the device-resident master parameters, then every packed weight buffer is rebuilt on the device. */
static int ensure_adam_state(TrainState& T);
int dm_unet_optimizer_step(dm_unet* u, double lr, double beta1, double beta2, double eps, float max_grad_norm,
                           float* grad_norm_out_host, void* stream) {
    return dm_unet_optimizer_step_ex(u, lr, beta1, beta2, eps, max_grad_norm, 0.0f, grad_norm_out_host, stream);
}

/* The same step when parameters outside the handle share the clip (a trained noise schedule on the host): extra_sq_norm,
 * the squared norm of their gradients, joins the sum before the coefficient is formed; the norm returned is the combined one. */
int dm_unet_optimizer_step_ex(dm_unet* u, double lr, double beta1, double beta2, double eps, float max_grad_norm,
                              float extra_sq_norm, float* grad_norm_out_host, void* stream) {
    DM_REQUIRE(u && u->train, "dm_unet_train_enable has not been called");
    DM_REQUIRE(extra_sq_norm >= 0.0f || extra_sq_norm != extra_sq_norm, "extra_sq_norm is a squared norm");
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrainState& T = *u->train;
    return guarded([&]() -> int {
        if (!T.param && upload_master(u)) return 1;
        if (ensure_adam_state(T)) return 1;
        if (u->order_after_previous(s)) return 1;  // the previous call on this handle may have used another stream
        if (launch_grad_norm(T.grad, (int64_t)T.grad_floats, T.norm_ws, max_grad_norm, T.clip2, s, (double)extra_sq_norm)) return 1;
        T.adam_step += 1;
        if (launch_adam(T.param, T.grad, T.adam_m, T.adam_v, T.norm_ws, (int64_t)T.grad_floats, lr, beta1, beta2, eps,
                        (int)T.adam_step, s))
            return 1;
        if (device_repack(u, s)) return 1;
        u->infer_stale = true;  // the fused inference-only packs (attn16, fused LinearAttention) still hold the old values
        u->drop_graph();
        if (u->mark_done(s)) return 1;
        if (grad_norm_out_host) {
            DM_CHECK_HIP(hipMemcpyAsync(grad_norm_out_host, T.clip2, sizeof(float), hipMemcpyDeviceToHost, s));
            DM_CHECK_HIP(hipStreamSynchronize(s));
        }
        return 0;
    });
}

/* ema.update() of ema_pytorch as Trainer uses it (:1190): copy != 0 copies the online parameters into the EMA buffer,
 * else ema.lerp_(param, 1 - decay) with the weight formed in double.  The decay schedule (update_after_step, update_every,
 * warm-up) is host logic in the Python mirror. */
int dm_unet_ema_update(dm_unet* u, double decay, int copy, void* stream) {
    DM_REQUIRE(u && u->train, "dm_unet_train_enable has not been called");
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrainState& T = *u->train;
    return guarded([&]() -> int {
        if (!T.param && upload_master(u)) return 1;
        const bool fresh = T.ema == nullptr;
        if (fresh) DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.ema), T.grad_floats * sizeof(float)));
        if (u->order_after_previous(s)) return 1;
        if (copy || fresh) {
            DM_CHECK_HIP(hipMemcpyAsync(T.ema, T.param, T.grad_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
            return u->mark_done(s);
        }
        if (launch_lerp(T.ema, T.param, (int64_t)T.grad_floats, decay, s)) return 1;
        return u->mark_done(s);
    });
}

/* read one tensor of the device-resident state (reference layout) into a DEVICE buffer: which = 0 online parameters,
 * 1 EMA parameters, 2 / 3 Adam's exp_avg / exp_avg_sq (torch.optim.Adam's per-parameter state) */
static int ensure_adam_state(TrainState& T) {
    if (T.adam_m) return 0;
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.adam_m), T.grad_floats * sizeof(float)));
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.adam_v), T.grad_floats * sizeof(float)));
    DM_CHECK_HIP(hipMemset(T.adam_m, 0, T.grad_floats * sizeof(float)));
    DM_CHECK_HIP(hipMemset(T.adam_v, 0, T.grad_floats * sizeof(float)));
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.norm_ws), 1024 * sizeof(double)));
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.clip2), 2 * sizeof(float)));
    return 0;
}
int dm_unet_get_param(dm_unet* u, const char* name, int which, float* out_dev, void* stream) {
    DM_REQUIRE(u && name && out_dev && u->train, "dm_unet_get_param needs a handle in training mode");
    DM_REQUIRE(which >= 0 && which <= 3, "dm_unet_get_param: which is 0 (online), 1 (EMA), 2 (exp_avg) or 3 (exp_avg_sq)");
    DM_CHECK_HIP(hipSetDevice(u->device));
    TrainState& T = *u->train;
    return guarded([&]() -> int {
        if (!T.param && upload_master(u)) return 1;
        auto it = T.off.find(name);
        DM_REQUIRE(it != T.off.end(), "unknown parameter");
        const float* src = which == 0 ? T.param : (which == 1 ? T.ema : (which == 2 ? T.adam_m : T.adam_v));
        DM_REQUIRE(src != nullptr, which == 1 ? "no EMA parameters yet (dm_unet_ema_update)"
                                              : "no optimiser state yet (dm_unet_optimizer_step)");
        if (u->order_after_previous(static_cast<hipStream_t>(stream))) return 1;
        DM_CHECK_HIP(hipMemcpyAsync(out_dev, src + it->second, P(u, name).numel() * sizeof(float), hipMemcpyDeviceToDevice,
                                    static_cast<hipStream_t>(stream)));
        return 0;
    });
}

/* restore one tensor of the training state from a DEVICE buffer (resuming from a Trainer checkpoint): which = 1 EMA
 * parameters, 2 / 3 Adam's exp_avg / exp_avg_sq.  The online parameters go through dm_unet_set_param + dm_unet_refresh. */
int dm_unet_set_train_tensor(dm_unet* u, const char* name, int which, const float* src_dev, void* stream) {
    DM_REQUIRE(u && name && src_dev && u->train, "dm_unet_set_train_tensor needs a handle in training mode");
    DM_REQUIRE(which >= 1 && which <= 3, "dm_unet_set_train_tensor: which is 1 (EMA), 2 (exp_avg) or 3 (exp_avg_sq)");
    DM_CHECK_HIP(hipSetDevice(u->device));
    TrainState& T = *u->train;
    return guarded([&]() -> int {
        if (!T.param && upload_master(u)) return 1;
        auto it = T.off.find(name);
        DM_REQUIRE(it != T.off.end(), "unknown parameter");
        if (which == 1 && !T.ema) {
            DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.ema), T.grad_floats * sizeof(float)));
            DM_CHECK_HIP(hipMemcpy(T.ema, T.param, T.grad_floats * sizeof(float), hipMemcpyDeviceToDevice));
        }
        if (which >= 2 && ensure_adam_state(T)) return 1;
        float* dst = which == 1 ? T.ema : (which == 2 ? T.adam_m : T.adam_v);
        if (u->order_after_previous(static_cast<hipStream_t>(stream))) return 1;
        DM_CHECK_HIP(hipMemcpyAsync(dst + it->second, src_dev, P(u, name).numel() * sizeof(float), hipMemcpyDeviceToDevice,
                                    static_cast<hipStream_t>(stream)));
        return u->mark_done(static_cast<hipStream_t>(stream));
    });
}

/* Adam's step counter (the `step` entry of torch.optim.Adam's per-parameter state; one value, all parameters step
 * together): returns it; set_to >= 0 sets it first.  -1 on a handle that is not in training mode. */
long long dm_unet_adam_step(dm_unet* u, long long set_to) {
    if (!u || !u->train) return -1;
    if (set_to >= 0) u->train->adam_step = (int)set_to;
    return u->train->adam_step;
}

/* bring the host copies (and with them the fused inference-only packs and the sampling path) up to date with the
 * device-resident parameters: device -> host, then dm_unet_refresh */
int dm_unet_train_sync(dm_unet* u) {
    DM_REQUIRE(u && u->train, "dm_unet_train_enable has not been called");
    DM_CHECK_HIP(hipSetDevice(u->device));
    TrainState& T = *u->train;
    if (!T.param || !u->infer_stale) return 0;
    DM_CHECK_HIP(hipDeviceSynchronize());
    for (const std::string& name : u->order) {
        HostTensor& t = u->params.at(name);
        DM_CHECK_HIP(hipMemcpy(t.data.data(), T.param + T.off.at(name), t.numel() * sizeof(float), hipMemcpyDeviceToHost));
        t.dirty = true;
    }
    u->infer_stale = false;
    return dm_unet_refresh(u);
}

/* self-check of the device packers: re-pack every buffer from the master parameters on the device and compare it with
 * what the host packer produced; returns the number of buffers that differ (0 = all bit-identical), -1 on error */
int dm_unet_check_device_pack(dm_unet* u) {
    if (!u || !u->train) return -1;
    if (hipSetDevice(u->device) != hipSuccess) return -1;
    TrainState& T = *u->train;
    int bad = 0;
    std::map<int, int> by_kind;
    std::string first;
    try {
        if (!T.param && upload_master(u)) return -1;
        auto check = [&](const PackOp& op) -> int {
            std::vector<float> host(op.n), devp(op.n);
            if (hipMemcpy(host.data(), op.dst, op.n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1;
            if (hipMemset(op.dst, 0xFF, op.n * sizeof(float)) != hipSuccess) return -1;
            if (run_pack_op(u, T, op, nullptr)) return -1;
            if (hipDeviceSynchronize() != hipSuccess) return -1;
            if (hipMemcpy(devp.data(), op.dst, op.n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1;
            if (std::memcmp(host.data(), devp.data(), op.n * sizeof(float)) != 0) {
                ++bad;
                by_kind[op.kind] += 1;
                if (first.empty()) {
                    size_t at = 0;
                    while (at < op.n && std::memcmp(&host[at], &devp[at], 4) == 0) ++at;
                    first = (op.kind == PK_RAW_NAME ? op.name : op.src.wname) + " src kind " + std::to_string(op.src.kind) +
                            " first difference at " + std::to_string(at) + " of " + std::to_string(op.n) + ": host " +
                            std::to_string(host[at]) + " device " + std::to_string(devp[at]);
                }
                (void)hipMemcpy(op.dst, host.data(), op.n * sizeof(float), hipMemcpyHostToDevice);
            }
            return 0;
        };
        // (a buffer no step has used since the last optimiser step is stale by design: rebuilt when first used)
        for (size_t i = 0; i < u->pack_ops.size(); ++i)
            if (!(i < T.stale_f.size() && T.stale_f[i]) && check(u->pack_ops[i])) return -1;
        for (size_t i = 0; i < T.ops.size(); ++i)
            if (!(i < T.stale_b.size() && T.stale_b[i]) && check(T.ops[i])) return -1;
    } catch (const std::exception& e) {
        set_error(e.what());
        return -1;
    }
    // the grouped re-pack (what an optimiser step runs: every buffer a training step has used, two launches) against the
    // buffers just verified
    try {
        if (!bad && !T.used_f.empty()) {
            std::vector<std::pair<const PackOp*, std::vector<float>>> want;
            auto keep = [&](const PackOp& op, bool used) -> int {
                if (!used || is_raw_copy(op)) return 0;
                want.emplace_back(&op, std::vector<float>(op.n));
                if (hipMemcpy(want.back().second.data(), op.dst, op.n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                    return -1;
                return hipMemset(op.dst, 0xFF, op.n * sizeof(float)) != hipSuccess ? -1 : 0;
            };
            for (size_t i = 0; i < u->pack_ops.size(); ++i)
                if (keep(u->pack_ops[i], T.used_f[i])) return -1;
            for (size_t i = 0; i < T.ops.size(); ++i)
                if (keep(T.ops[i], T.used_b[i])) return -1;
            std::fill(T.stale_f.begin(), T.stale_f.end(), 1);
            std::fill(T.stale_b.begin(), T.stale_b.end(), 1);
            if (batched_repack(u, nullptr)) return -1;
            if (hipDeviceSynchronize() != hipSuccess) return -1;
            for (size_t i = 0; i < u->pack_ops.size(); ++i)  // whatever the grouped launch does not cover: the lazy path
                if (T.used_f[i] && T.stale_f[i] && !is_raw_copy(u->pack_ops[i]) && run_pack_op(u, T, u->pack_ops[i], nullptr))
                    return -1;
            for (size_t i = 0; i < T.ops.size(); ++i)
                if (T.used_b[i] && T.stale_b[i] && !is_raw_copy(T.ops[i]) && run_pack_op(u, T, T.ops[i], nullptr)) return -1;
            if (hipDeviceSynchronize() != hipSuccess) return -1;
            std::fill(T.stale_f.begin(), T.stale_f.end(), 0);
            std::fill(T.stale_b.begin(), T.stale_b.end(), 0);
            std::vector<float> got;
            for (auto& w : want) {
                const PackOp& op = *w.first;
                got.resize(op.n);
                if (hipMemcpy(got.data(), op.dst, op.n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1;
                if (std::memcmp(got.data(), w.second.data(), op.n * sizeof(float)) != 0) {
                    ++bad;
                    by_kind[op.kind] += 1;
                    if (first.empty()) first = "grouped re-pack of " + op.src.wname + " (src kind " + std::to_string(op.src.kind) + ")";
                    (void)hipMemcpy(op.dst, w.second.data(), op.n * sizeof(float), hipMemcpyHostToDevice);
                }
            }
        }
    } catch (const std::exception& e) {
        set_error(e.what());
        return -1;
    }
    if (bad) {
        std::string msg = "device packers differ from the host packers:";
        for (auto& kv : by_kind) {
            const ConvFamily* F = nullptr;
            const char* name = conv_recipe_of(kv.first, &F) ? F->name : (kv.first == PK_FOLD ? "folded upsample" : "raw copy");
            msg += std::string(" ") + name + " x" + std::to_string(kv.second);
        }
        set_error(msg + "; " + first);
    }
    return bad;
}

/* nn.Dropout(p) of the Blocks in training mode (Unet(dropout=p), DD/denoising_diffusion.py:111,121; the shipped
 * ddpm_cifar.yaml trains with 0.1).  Masks are Philox4x32-10 draws keyed by (seed, call, block): every loss / backward
 * call after this one uses fresh masks, the backward pass of a call re-creates the masks of its forward. */
int dm_unet_train_dropout(dm_unet* u, float p, uint64_t seed) {
    DM_REQUIRE(u && u->train, "dm_unet_train_enable has not been called");
    DM_REQUIRE(p >= 0.f && p < 1.f, "dropout probability must be in [0, 1)");
    u->train->dropout = p;
    u->train->drop_seed = seed;
    u->train->drop_call = 0;
    return 0;
}
/* the factor (0 or 1 / (1 - p)) the `block_index`-th Block (forward order) of loss / backward call number `call` (0 = the
 * first after dm_unet_train_dropout) applies, for n elements in the kernels' NHWC order (B, H, W, C): parity tests hand
 * these masks to the oracle */
int dm_op_dropout_mask(float* out, int64_t n, float p, uint64_t seed, uint64_t call, int block_index, void* stream) {
    DM_REQUIRE(out && n > 0 && n % 4 == 0, "bad argument");
    return launch_dropout(nullptr, nullptr, out, n, p, seed, (call << 16) | (uint64_t)(block_index + 1),
                          static_cast<hipStream_t>(stream));
}

// Per-call coefficient tables of the stand-alone elementwise ops: one grow-only device buffer per (host thread, device), on
// the device the data lives on (the ops take no handle: the device comes from the data pointer).  The caller synchronises
// the stream before it returns, so the buffer is free again for the thread's next call.  These ops keep this helper
// beside table_op (dm_op_scaffold.inc), which allocates per call on the CURRENT device: they pick the device from the
// data pointer, which a caller with tensors on several devices observes (q_sample and lincomb are product calls of the
// Python classes, not test plumbing only), and dm_op_mse_loss copies its parts to DEVICE pointers.  Nothing is read that
// the call did not write: the table is uploaded whole and the kernel writes every scratch float the entry copies out.
// `extra`: floats of device scratch behind the table (per-sample partial sums, a scalar result)
static int stage_coefs(const void* data_dev, const float* host, size_t n, hipStream_t s, float** out, size_t extra = 0) {
    hipPointerAttribute_t at{};
    DM_CHECK_HIP(hipPointerGetAttributes(&at, data_dev));
    DM_CHECK_HIP(hipSetDevice(at.device));
    thread_local std::map<int, std::pair<float*, size_t>> scratch;
    auto& sc = scratch[at.device];
    if (sc.second < n + extra) {
        if (sc.first) (void)hipFree(sc.first);
        sc = {nullptr, 0};
        const size_t cap = std::max<size_t>(n + extra, 4096);
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&sc.first), cap * sizeof(float)));
        sc.second = cap;
    }
    DM_CHECK_HIP(hipMemcpyAsync(sc.first, host, n * sizeof(float), hipMemcpyHostToDevice, s));
    *out = sc.first;
    return 0;
}
static int finish_op(int rc, hipStream_t s) {
    hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) {
        set_error(std::string("kernel execution failed: ") + hipGetErrorString(e));
        rc = 1;
    }
    return rc;
}

int dm_op_q_sample(const float* x_start, const float* noise, const float* coef_host, float* out, int B, int per_sample,
                   void* stream) {
    DM_REQUIRE(x_start && noise && coef_host && out && B > 0 && per_sample > 0, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* cd = nullptr;
    if (stage_coefs(out, coef_host, (size_t)B * DM_TRAIN_COEFS, s, &cd)) return 1;
    return finish_op(launch_q_sample(x_start, noise, cd, out, B, per_sample, s), s);
}

int dm_op_lincomb(const float* x, const float* y, const float* coef_host, float* out, int B, int64_t per_sample, int mode,
                  int clamp, void* stream) {
    DM_REQUIRE(x && y && coef_host && out && B > 0 && per_sample > 0 && (mode == 0 || mode == 1), "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* cd = nullptr;
    if (stage_coefs(out, coef_host, (size_t)B * 2, s, &cd)) return 1;
    return finish_op(launch_lincomb(x, y, cd, out, B, per_sample, mode, clamp, s), s);
}

int dm_op_mask_mix(const float* a, const float* b, const float* mask, float* out, int64_t n, void* stream) {
    DM_REQUIRE(a && b && mask && out && n > 0, "bad argument");
    return guarded([&]() -> int { return launch_mask_mix(a, b, mask, out, n, static_cast<hipStream_t>(stream)); });
}

int dm_op_offset_noise(float* noise, const float* offset, float strength, int BC, int HW, void* stream) {
    DM_REQUIRE(noise && offset && BC > 0 && HW > 0, "bad argument");
    return guarded([&]() -> int { return launch_offset_noise(noise, offset, strength, BC, HW, static_cast<hipStream_t>(stream)); });
}

int dm_op_cdist(const float* x, const float* y, float* out, int n, int m, int64_t D, void* stream) {
    DM_REQUIRE(x && y && out && n > 0 && m > 0 && D > 0, "bad argument");
    return guarded([&]() -> int { return launch_cdist(x, y, out, n, m, D, static_cast<hipStream_t>(stream)); });
}

int dm_op_gather_rows(const float* src, const int64_t* idx_host, float* dst, int n, int64_t D, void* stream) {
    DM_REQUIRE(src && idx_host && dst && src != dst && n > 0 && D > 0, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int i = 0; i < n; ++i) {
        DM_REQUIRE(idx_host[i] >= 0 && idx_host[i] < n, "gather index out of range");
        DM_CHECK_HIP(hipMemcpyAsync(dst + (size_t)i * D, src + (size_t)idx_host[i] * D, (size_t)D * sizeof(float),
                                    hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

/* The DDPM loss kernel on its own (p_losses :864-897 after the U-Net): the weighted MSE (terms & 1) and / or the hybrid KL
 * term (terms & 2), the gradient with respect to the model output, and the per-sample parts.  The factor of the KL term is
 * kl_weight / (n_pos + 1e-8) in fp32, n_pos = the number of rows with t > 0 (coef[b][3]), as the reference forms
 * kl / (mask.sum() + 1e-8).  The training call does not form it: dm_train_args.kl_scale arrives from the caller, which is
 * hybrid_kl_scale() in diffusion.py.  The two must stay the same fp32 expression;
 * test_mse_loss_kl_factor_is_the_one_training_passes compares them bit for bit. */
static float hybrid_kl_scale(float kl_weight, const float* coef_host, int B) {
    float n_pos = 0.f;
    for (int b = 0; b < B; ++b) n_pos += coef_host[(size_t)b * DM_TRAIN_COEFS + 3];
    return kl_weight / (n_pos + 1e-8f);
}
int dm_op_mse_loss(const float* out, const float* x_start, const float* noise, const float* xq, const float* coef_host,
                   int objective, int terms, float loss_scale, float kl_weight, float* dout, float* loss_out_host,
                   float* part_out, float* klpart_out, int B, int per_sample, void* stream) {
    DM_REQUIRE(out && x_start && noise && coef_host && dout && loss_out_host && B > 0 && per_sample > 0, "bad argument");
    DM_REQUIRE(objective >= 0 && objective <= 2 && terms >= 1 && terms <= 3 && (!(terms & 2) || xq), "mse_loss: objective / terms");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        const size_t nc = (size_t)B * DM_TRAIN_COEFS;
        float* cd = nullptr;
        if (stage_coefs(dout, coef_host, nc, s, &cd, 2 * (size_t)B + 1)) return 1;
        float *part = cd + nc, *klpart = part + B, *loss = klpart + B;
        const float kl_scale = (terms & 2) ? hybrid_kl_scale(kl_weight, coef_host, B) : 0.f;
        int rc = launch_mse_loss(out, x_start, noise, cd, dout, part, loss, B, per_sample, objective, loss_scale, s, terms, xq,
                                 klpart, kl_scale);
        // from here on the stream may hold work on the scratch: every path goes through finish_op, which synchronises
        auto copy = [&](void* dst, const float* src, size_t floats, hipMemcpyKind kind) {
            const hipError_t e = rc ? hipSuccess : hipMemcpyAsync(dst, src, floats * sizeof(float), kind, s);
            if (e != hipSuccess) {
                set_error(std::string("mse_loss: copying a result failed: ") + hipGetErrorString(e));
                rc = 1;
            }
        };
        copy(loss_out_host, loss, 1, hipMemcpyDeviceToHost);
        if (part_out) copy(part_out, part, (size_t)B, hipMemcpyDeviceToDevice);
        if (klpart_out && (terms & 2)) copy(klpart_out, klpart, (size_t)B, hipMemcpyDeviceToDevice);
        return finish_op(rc, s);
    });
}

/* clip_grad_norm_(max_grad_norm) + one torch.optim.Adam step (the `step`-th) on flat device buffers: what
 * dm_unet_optimizer_step runs on the handle's parameters.  norm_coef_out_host (optional): the total gradient norm before
 * clipping and the clip coefficient. */
int dm_op_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                    int step, float max_grad_norm, float* norm_coef_out_host, void* stream) {
    DM_REQUIRE(p && g && m && v && n > 0 && step >= 1, "bad argument");
    DM_REQUIRE((reinterpret_cast<uintptr_t>(g) & 15) == 0, "adam_step: the gradient buffer must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        double* ws = nullptr;  // 1024 partial sums, then (norm, coefficient)
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&ws), 1024 * sizeof(double) + 2 * sizeof(float)));
        float* clip2 = reinterpret_cast<float*>(ws + 1024);
        int rc = launch_grad_norm(g, n, ws, max_grad_norm, clip2, s) ||
                 launch_adam(p, g, m, v, ws, n, lr, beta1, beta2, eps, step, s);
        if (!rc && norm_coef_out_host &&
            hipMemcpyAsync(norm_coef_out_host, clip2, 2 * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess) {
            set_error("adam_step: copying the norm failed");
            rc = 1;
        }
        rc = finish_op(rc, s);
        (void)hipFree(ws);
        return rc;
    });
}

/* ema.lerp_(online, 1 - decay) on flat device buffers (what dm_unet_ema_update runs) */
int dm_op_ema_lerp(float* ema, const float* p, int64_t n, double decay, void* stream) {
    DM_REQUIRE(ema && p && n > 0, "bad argument");
    return guarded([&]() -> int { return launch_lerp(ema, p, n, decay, static_cast<hipStream_t>(stream)); });
}

}  // extern "C"
