// The scaffolding every sampling loop on the C ABI runs on -- handle checks, step-table growth, stream choice, workspace,
// state upload, the eager / captured-graph loop driver -- and the DDPM / DDIM loop behind dm_sample*.  Included by
// dm_api.hip before dm_edm.inc, dm_ct.inc, dm_repaint.inc, dm_learned.inc, dm_weighted.inc, dm_cguide.inc and dm_bpd.inc
// (the bits-per-dim evaluation loop, which calls the pieces itself), whose loops use the same pieces.  A loop keeps what is its own: argument checks, buffer list, prologue, step, graph key and the
// kernel that writes `out`.  dm_repaint.inc .. dm_cguide.inc are the table-driven integer-time loops: table_loop_begin / table_loop_end
// run the pieces for them, and they keep their argument and U-Net checks, their extra buffers, a prologue kernel, their
// step lambdas, their extra key fields and their run_steps call.  The EDM and continuous-time loops (float time, no
// `times`, their own kernel that writes `out`) and sample_impl (the other table pair, guidance buffers) call the pieces
// themselves.

namespace dm {

// ---- handle checks ----------------------------------------------------------------------------------------------------
// karras_ok: the caller runs a KarrasUnet handle too (the float-time forward and the EDM loops); every other loop refuses it
static int handle_ready(dm_unet* u, bool karras_ok = false) {
    DM_REQUIRE(u->finalized, "dm_unet_finalize has not been called");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    DM_REQUIRE(!u->infer_stale, "parameters were updated on the device (dm_unet_optimizer_step): call dm_unet_train_sync "
                                "before sampling from this handle");
    DM_REQUIRE(karras_ok || !u->kunet, "a KarrasUnet handle runs dm_unet_forward_ft and dm_sample_edm only");
    return 0;
}

// the U-Net maps x to x with no text condition; text_msg: the caller's own message for the text half
// the sequence model is pinned for dm_unet_forward and the DDPM / DDIM loop of dm_sample_ex; the other loops refuse its handle
static int image_unet_only(dm_unet* u) {
    DM_REQUIRE(!u->cfg.seq1d, "this loop is not available for the sequence model (seq1d): it samples through dm_sample_ex");
    return 0;
}

static int plain_unet_ok(dm_unet* u, const char* msg, const char* text_msg = nullptr) {
    if (image_unet_only(u)) return 1;
    DM_REQUIRE(u->cfg.text_mode == DM_TEXT_NONE, text_msg ? text_msg : msg);
    DM_REQUIRE(u->out_dim == u->cfg.channels && u->cfg.input_channels == u->cfg.channels, msg);
    return 0;
}

// ---- device step tables -----------------------------------------------------------------------------------------------
enum { TAB_INT = 1, TAB_FLOAT = 2 };  // times_dev + coefs_dev (integer time) / edm_tab_dev (16-float rows)

// Make the tables of `which` hold n rows (and the sampler state exist).  A table that is too small is reallocated at n
// rounded up to `granule` rows, and the captured graph, which reads the old one, is dropped; one that is large enough
// keeps its address, and with it the graph.
static int grow_tables(dm_unet* u, int which, int n, int granule) {
    if (!u->state_dev) DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&u->state_dev), 256));
    const int want = (n + granule - 1) / granule * granule;
    auto grow = [&](int& cap, std::initializer_list<std::pair<void**, size_t>> bufs) -> int {  // (buffer, bytes per row)
        if (n <= cap) return 0;
        DM_CHECK_HIP(hipDeviceSynchronize());
        u->drop_graph();
        for (auto& b : bufs) {
            if (*b.first) (void)hipFree(*b.first);
            *b.first = nullptr;
        }
        cap = 0;
        for (auto& b : bufs) DM_CHECK_HIP(hipMalloc(b.first, (size_t)want * b.second));
        cap = want;
        return 0;
    };
    if ((which & TAB_INT) && grow(u->sampler_cap, {{reinterpret_cast<void**>(&u->times_dev), sizeof(int64_t)},
                                                   {reinterpret_cast<void**>(&u->coefs_dev), DM_COEFS * sizeof(float)}}))
        return 1;
    if ((which & TAB_FLOAT) && grow(u->edm_cap, {{reinterpret_cast<void**>(&u->edm_tab_dev), DM_EDM_COEFS * sizeof(float)}}))
        return 1;
    return 0;
}

// ---- one run of a loop ------------------------------------------------------------------------------------------------
namespace {
struct SamplerRun {
    dm_unet* u = nullptr;
    hipStream_t s = nullptr;  // the stream of the whole call
    bool use_graph = false;
    bool own_stream = false;  // s is the handle's: the caller passed the legacy default stream, which cannot be captured
    SamplerState st_host{};   // lives here until the upload has been waited for
    Arena A;                  // over the handle's workspace, the loop's own buffers allocated ...
    std::vector<Arena::Blk> mark;  // ... allocator state in front of a step
    void rewind() { A.blks = mark; }
};
}  // namespace

// Graph mode on the legacy default stream: the whole call runs on a stream of the handle, ordered after the caller's
// work by a synchronisation here and finished before return (run_finish).
static int run_begin(SamplerRun& r, dm_unet* u, void* stream, int use_graph) {
    r.u = u;
    r.s = static_cast<hipStream_t>(stream);
    r.use_graph = use_graph != 0;
    r.own_stream = r.use_graph && r.s == nullptr;
    if (r.own_stream) {
        if (!u->cap_stream) DM_CHECK_HIP(hipStreamCreateWithFlags(&u->cap_stream, hipStreamNonBlocking));
        DM_CHECK_HIP(hipStreamSynchronize(nullptr));
        r.s = u->cap_stream;
    }
    return 0;
}

// Size the workspace with a dry run of `layout` (the loop's buffers, in front of the forward arena) and one forward, wait
// for the previous call on the handle, then lay the buffers out for real.
static int run_workspace(SamplerRun& r, const std::function<void(Arena&)>& layout, const std::function<int(Arena&)>& dry_forward) {
    Arena dry;
    dry.dry = true;
    layout(dry);
    if (dry_forward(dry)) return 1;
    if (ensure_workspace(r.u, dry.off)) return 1;
    if (r.u->order_after_previous(r.s)) return 1;
    r.A.base = r.u->ws;
    r.A.cap = r.u->ws_cap;
    layout(r.A);
    r.mark = r.A.blks;
    return 0;
}

// Step tables (those that are given) and the sampler state to the device.  The host tables may go away when the call
// returns, so the stream is waited for: here, or with sync == false by the caller after uploads of its own.
static int run_upload(SamplerRun& r, int n_rows, const int64_t* times_host, const float* coefs_host, const float* tab_host,
                      int unnormalize, uint64_t seed, uint64_t elem_off, bool sync = true) {
    dm_unet* u = r.u;
    r.st_host.step = 0;
    r.st_host.n_steps = n_rows;
    r.st_host.unnormalize = unnormalize;
    r.st_host.seed = seed;
    r.st_host.off4 = elem_off / 4;
    if (times_host) DM_CHECK_HIP(hipMemcpyAsync(u->times_dev, times_host, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice, r.s));
    if (coefs_host)
        DM_CHECK_HIP(hipMemcpyAsync(u->coefs_dev, coefs_host, (size_t)n_rows * DM_COEFS * sizeof(float), hipMemcpyHostToDevice, r.s));
    if (tab_host)
        DM_CHECK_HIP(hipMemcpyAsync(u->edm_tab_dev, tab_host, (size_t)n_rows * DM_EDM_COEFS * sizeof(float), hipMemcpyHostToDevice, r.s));
    DM_CHECK_HIP(hipMemcpyAsync(u->state_dev, &r.st_host, sizeof(r.st_host), hipMemcpyHostToDevice, r.s));
    if (sync) DM_CHECK_HIP(hipStreamSynchronize(r.s));
    return 0;
}

// capture fn(s) into an instantiated graph
static int capture_graph(dm_unet* u, hipStream_t s, const std::function<int(hipStream_t)>& fn, hipGraph_t* g_out,
                         hipGraphExec_t* e_out) {
    DM_CHECK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = fn(s);
    hipGraph_t graph = nullptr;
    hipError_t ce = hipStreamEndCapture(s, &graph);
    if (rc || ce != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        if (!rc) set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
        return 1;
    }
    hipGraphExec_t exec = nullptr;
    hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (ie != hipSuccess) {
        (void)hipGraphDestroy(graph);
        set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
        return 1;
    }
    *g_out = graph;
    *e_out = exec;
    u->graph_captures += 1;
    return 0;
}

// The loop: n times `step`, eagerly or as replays of the handle's graph.  The slot is this loop's while `key` (shape,
// kind, every pointer and flag that is a kernel argument of the step) holds; otherwise what it held is dropped and the
// step is captured again.  ElucidatedDiffusion's Heun loop has two steps: `step` where is_full(i), else `last` (graph in
// edm_last_graph); each is captured when the loop first needs it.  With `between` (classifier guidance) every iteration
// is `step`, then between(i) on the host, then `last`: the two halves of one step, a graph slot each; a non-zero
// between(i) ends the loop and nothing more is launched.
static int run_steps(SamplerRun& r, const dm_unet::GraphKey& key, int n, const std::function<int(hipStream_t)>& step,
                     const std::function<int(hipStream_t)>& last = nullptr, const std::function<bool(int)>& is_full = nullptr,
                     const std::function<int(int)>& between = nullptr) {
    dm_unet* u = r.u;
    if (!r.use_graph) {
        for (int i = 0; i < n; ++i) {
            if (between) {
                if (step(r.s) || between(i) || last(r.s)) return 1;
            } else if ((!is_full || is_full(i) ? step : last)(r.s)) {
                return 1;
            }
        }
        return 0;
    }
    if (!(u->gkey == key)) {
        u->drop_graph();
        u->gkey = key;
    }
    auto replay = [&](bool full) -> int {
        hipGraphExec_t* e = full ? &u->gexec : &u->edm_last_gexec;
        if (!*e && capture_graph(u, r.s, full ? step : last, full ? &u->graph : &u->edm_last_graph, e)) {
            u->drop_graph();
            return 1;
        }
        DM_CHECK_HIP(hipGraphLaunch(*e, r.s));
        return 0;
    };
    for (int i = 0; i < n; ++i) {
        if (between) {
            if (replay(true) || between(i) || replay(false)) return 1;
        } else if (replay(!is_full || is_full(i))) {
            return 1;
        }
    }
    return 0;
}

// after the kernel that writes `out`: later calls on the handle wait for this one, and a call on the handle's own stream
// is finished before it returns
static int run_finish(SamplerRun& r) {
    if (r.u->mark_done(r.s)) return 1;
    if (r.own_stream) DM_CHECK_HIP(hipStreamSynchronize(r.s));
    return 0;
}

// ---- the table-driven integer-time loops ------------------------------------------------------------------------------
// What the learned-variance, weighted-objective, classifier-guided and RePaint loops share around their steps: the times
// next to a 16-float step table in edm_tab_dev, a U-Net called as model(x, t), the image in `xbuf` and the last step's
// result in `fin` (the caller's `out` stays out of the captured graph).
namespace {
struct TableLoop {
    SamplerRun r;
    hipStream_t s = nullptr;  // r.s
    int64_t n = 0;            // B * C * H * W
    float *xbuf = nullptr, *fin = nullptr;
    const float* tab = nullptr;  // the uploaded table
    dm_unet::GraphKey key;       // B, H, W, noise, all_steps, ws, times, tab; the loop adds its kind and its own fields
};
}  // namespace

// From the device choice to frame 0: tables grown by `granule` rows, the stream, the workspace ([x | result | `layout`'s
// buffers | forward arena]), the upload of `n_rows` rows and the state, x_T in xbuf and in all_steps.  `a`: the loop's
// argument struct, read by the field names the four share; its checks have run.
template <class Args>
static int table_loop_begin(TableLoop& L, dm_unet* u, const Args& a, int n_rows, int granule, uint64_t elem_off,
                            const std::function<void(Arena&)>& layout) {
    if (image_unet_only(u)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    const int B = a.B, H = a.H, W = a.W;
    L.n = (int64_t)B * u->cfg.channels * H * W;
    if (grow_tables(u, TAB_INT | TAB_FLOAT, n_rows, granule) || run_begin(L.r, u, a.stream, a.use_graph)) return 1;
    L.s = L.r.s;
    auto buffers = [&](Arena& A) {
        L.xbuf = A.alloc(L.n);
        L.fin = A.alloc(L.n);
        layout(A);
    };
    if (run_workspace(L.r, buffers, [&](Arena& dry) {
            return unet_forward_impl(u, dry, nullptr, nullptr, u->times_dev, u->state_dev, nullptr, 0, nullptr, B, H, W, L.s);
        }))
        return 1;
    if (run_upload(L.r, n_rows, a.times_host, nullptr, a.table_host, a.unnormalize ? 1 : 0, a.seed, elem_off)) return 1;
    L.tab = u->edm_tab_dev;
    DM_CHECK_HIP(hipMemcpyAsync(L.xbuf, a.x_T, L.n * sizeof(float), hipMemcpyDeviceToDevice, L.s));  // img = randn(shape)
    if (a.all_steps) DM_CHECK_HIP(hipMemcpyAsync(a.all_steps, a.x_T, L.n * sizeof(float), hipMemcpyDeviceToDevice, L.s));
    L.key.B = B; L.key.H = H; L.key.W = W;
    L.key.noise = a.noise; L.key.all_steps = a.all_steps; L.key.ws = u->ws; L.key.times = u->times_dev; L.key.tab = u->edm_tab_dev;
    return 0;
}

// after run_steps: the result to the caller, and the run is done
static int table_loop_end(TableLoop& L, float* out) {
    DM_CHECK_HIP(hipMemcpyAsync(out, L.fin, L.n * sizeof(float), hipMemcpyDeviceToDevice, L.s));
    return run_finish(L.r);
}

// ---- DDPM / DDIM ------------------------------------------------------------------------------------------------------
// The sampling loop behind dm_sample / dm_sample_cond.  cond (B, cond_channels, H, W) is the image condition of
// DD/denoising_diffusion_image_conditional.py:51-55,156-180: constant over the loop, concatenated behind x in front of
// init_conv at every step.
//
// One denoise step (U-Net forward + update + step counter) touches only handle-owned memory: x, eps, the [x | cond]
// input, the text context and the final image live at fixed offsets of the workspace, and everything that differs
// between two calls of one shape (seed, Philox offset, step tables) is device DATA, not a kernel argument.  The step is
// therefore captured into a hipGraph once per (shape, sampler kind) and the instantiated graph is replayed by every
// later call; it is re-captured only when the shape, an injected-noise / all-steps pointer or the workspace changes.
static int sample_impl(dm_unet* u, int kind, int n_steps, const int64_t* times_host, const float* coefs_host,
                       const float* x_T, const float* noise, uint64_t seed, uint64_t sample_offset, const float* ctx,
                       int ctx_tokens, const float* cond, int cond_channels, float* out, float* all_steps, int B, int H,
                       int W, int unnormalize, int use_graph, void* stream, int objective = DM_OBJ_PRED_NOISE,
                       int self_cond = 0, const CfgParams* guide = nullptr, int ddim_flags = 0,
                       const dm_sample_dyn_args* dyn_args = nullptr) {
    DM_REQUIRE(u && times_host && coefs_host && x_T && out, "null argument");
    if (handle_ready(u)) return 1;
    DM_REQUIRE(kind == DM_SAMPLER_DDPM || kind == DM_SAMPLER_DDIM || kind == DM_SAMPLER_DPMPP, "unknown sampler kind");
    const bool dpmpp = kind == DM_SAMPLER_DPMPP;
    DM_REQUIRE(!(dpmpp && u->cfg.seq1d), "DPM-Solver++ is not pinned for the sequence model (seq1d) yet");
    DM_REQUIRE(n_steps > 0 && B > 0, "empty run");
    DM_REQUIRE(ddim_flags == 0 || kind == DM_SAMPLER_DDIM, "ddim_flags belong to the DDIM loop");
    DM_REQUIRE((ddim_flags & ~(DM_DDIM_NO_CLAMP | DM_DDIM_RAW_NOISE)) == 0, "unknown ddim_flags");
    DM_REQUIRE(u->out_dim == u->cfg.channels, "sampler needs out_dim == channels (DD/denoising_diffusion.py:456)");
    DM_REQUIRE((cond == nullptr) == (cond_channels == 0) && cond_channels >= 0, "cond and cond_channels come together");
    DM_REQUIRE(objective >= DM_OBJ_PRED_NOISE && objective <= DM_OBJ_PRED_V, "unknown objective");
    DM_REQUIRE(!self_cond || cond_channels == 0, "self-conditioning and an image condition are not combined");
    DM_REQUIRE(u->cfg.input_channels == u->cfg.channels * (self_cond ? 2 : 1) + cond_channels,
               "U-Net input channels != channels [* 2 with self-conditioning] + cond_channels");
    DM_REQUIRE((ctx == nullptr) == (ctx_tokens == 0), "ctx and ctx_tokens come together");
    // classifier-free guidance: every step runs the U-Net on [x | x] with the text mask [1.. | 0..] (B conditioned and
    // B null images in one forward) and combines the two halves into the model output the update reads
    const bool guided = guide != nullptr;
    if (guided) {
        DM_REQUIRE(u->cfg.text_mode != DM_TEXT_NONE, "classifier-free guidance (cfg_scale != 1) needs a text-conditional U-Net");
        DM_REQUIRE(ctx != nullptr, "classifier-free guidance needs a text context");
        DM_REQUIRE(!self_cond, "classifier-free guidance is not combined with self-conditioning");
        DM_REQUIRE(cond == nullptr, "classifier-free guidance is not combined with an image condition");
    }
    // dynamic thresholding: one select per step between the model output and the update, which then reads s[b]
    const bool dyn = dyn_args && dyn_args->dyn_threshold != 0;
    if (dyn) {
        DM_REQUIRE(dyn_args->dyn_percentile > 0.0f && dyn_args->dyn_percentile <= 1.0f,
                   "the percentile of dynamic thresholding lies in (0, 1]");
        DM_REQUIRE(!u->cfg.seq1d, "dynamic thresholding is not available for the sequence model (seq1d)");
        DM_REQUIRE(ddim_flags == 0, "dynamic thresholding is not combined with ddim_flags");
    }
    const int Bf = guided ? 2 * B : B;  // batch of the U-Net forward
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    const int C = u->cfg.channels;
    const int64_t n = (int64_t)B * C * H * W;
    // the U-Net input when it is wider than x: [x | cond] (image condition) or [x_start | x] (self-conditioning)
    const int Cin = self_cond ? 2 * C : C + cond_channels;
    const bool wide = Cin != C;
    const int64_t n_in = (int64_t)B * Cin * H * W;
    const int64_t n_ctx = ctx ? (int64_t)B * ctx_tokens * u->cfg.text_emb_dim : 0;
    const uint64_t elem_off = sample_offset * (uint64_t)C * H * W;  // global element index of this shard's first value
    DM_REQUIRE(elem_off % 4 == 0, "sample_offset * C * H * W must be a multiple of 4");

    SamplerRun r;
    if (grow_tables(u, TAB_INT, n_steps, 1) || run_begin(r, u, stream, use_graph)) return 1;
    hipStream_t s = r.s;
    // workspace: [x | eps | [x | cond] | ctx | forward arena]; guided: [x | x copy | eps | 2B model output | ctx | ctx copy |
    // text mask | guidance parameters | forward arena]; with dynamic thresholding s (B) and its parameters in front of
    // the forward arena
    const int64_t n_ws = guided ? 2 * n : n;
    float *xbuf, *eps, *eps2, *xin, *xstart, *ctxbuf, *gpar, *dyn_s, *dpar;
    int32_t* tmask;
    auto layout = [&](Arena& A) {
        xbuf = A.alloc(n_ws);  // guided: [x | x], the U-Net input of both halves
        eps = A.alloc(n);
        eps2 = guided ? A.alloc(2 * n) : nullptr;  // model output of the conditioned and the null half
        xin = wide ? A.alloc(n_in) : nullptr;      // [x | cond] or [x_start | x] per image, what init_conv reads
        // clamped x_0 estimate of the previous step: what self-conditioning feeds back and what DPM-Solver++ (2M)
        // extrapolates from, one buffer for both
        xstart = self_cond || dpmpp ? A.alloc(n) : nullptr;
        ctxbuf = ctx ? A.alloc(guided ? 2 * n_ctx : n_ctx) : nullptr;
        tmask = guided ? reinterpret_cast<int32_t*>(A.alloc(2 * B)) : nullptr;
        gpar = guided ? A.alloc(4) : nullptr;  // CfgParams: device data, so a captured step serves any guidance scale
        dyn_s = dyn ? A.alloc(B) : nullptr;
        dpar = dyn ? A.alloc(4) : nullptr;  // DynParams: device data, so a captured step serves any percentile
    };
    const float* ctx_marker = ctx ? reinterpret_cast<const float*>(16) : nullptr;
    const int32_t* mask_marker = guided ? reinterpret_cast<const int32_t*>(16) : nullptr;
    if (run_workspace(r, layout, [&](Arena& dry) {
            return unet_forward_impl(u, dry, nullptr, nullptr, u->times_dev, u->state_dev, ctx_marker, ctx_tokens, nullptr, Bf, H,
                                     W, s, mask_marker);
        }))
        return 1;
    Arena& A = r.A;
    if (run_upload(r, n_steps, times_host, coefs_host, nullptr, unnormalize, seed, elem_off, /*sync=*/false)) return 1;
    std::vector<int32_t> tmask_host;
    if (guided) {
        tmask_host.assign(2 * B, 0);
        std::fill(tmask_host.begin(), tmask_host.begin() + B, 1);
        DM_CHECK_HIP(hipMemcpyAsync(tmask, tmask_host.data(), 2 * B * sizeof(int32_t), hipMemcpyHostToDevice, s));
        DM_CHECK_HIP(hipMemcpyAsync(gpar, guide, sizeof(CfgParams), hipMemcpyHostToDevice, s));
    }
    const DynParams dyn_host = dyn ? dyn_params((double)dyn_args->dyn_percentile, n / B) : DynParams{};
    if (dyn) DM_CHECK_HIP(hipMemcpyAsync(dpar, &dyn_host, sizeof(DynParams), hipMemcpyHostToDevice, s));
    DM_CHECK_HIP(hipStreamSynchronize(s));  // the host tables and the host state may go away when this function returns
    DM_CHECK_HIP(hipMemcpyAsync(xbuf, x_T, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (ctx) DM_CHECK_HIP(hipMemcpyAsync(ctxbuf, ctx, n_ctx * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (guided) {  // the null half reads the same x and (unused) context rows
        DM_CHECK_HIP(hipMemcpyAsync(xbuf + n, x_T, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        DM_CHECK_HIP(hipMemcpyAsync(ctxbuf + n_ctx, ctx, n_ctx * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if (cond && launch_copy_channels(cond, xin, B, cond_channels, C + cond_channels, C, H * W, s)) return 1;
    if (xstart) DM_CHECK_HIP(hipMemsetAsync(xstart, 0, n * sizeof(float), s));  // x_self_cond = zeros_like(x) (:353)
    if (all_steps) DM_CHECK_HIP(hipMemcpyAsync(all_steps, x_T, n * sizeof(float), hipMemcpyDeviceToDevice, s));

    auto one_step = [&](hipStream_t st) -> int {
        r.rewind();
        if (cond && launch_copy_channels(xbuf, xin, B, C, Cin, 0, H * W, st)) return 1;
        if (self_cond && (launch_copy_channels(xstart, xin, B, C, Cin, 0, H * W, st) ||
                          launch_copy_channels(xbuf, xin, B, C, Cin, C, H * W, st)))
            return 1;
        if (guided) {
            if (unet_forward_impl(u, A, xbuf, nullptr, u->times_dev, u->state_dev, ctxbuf, ctx_tokens, eps2, Bf, H, W, st,
                                  tmask))
                return 1;
            if (launch_cfg_combine(eps2, eps2 + n, eps, B, n / B, gpar, CfgParams{}, st)) return 1;
        } else if (unet_forward_impl(u, A, wide ? xin : xbuf, nullptr, u->times_dev, u->state_dev, ctxbuf, ctx_tokens, eps,
                                     B, H, W, st)) {
            return 1;
        }
        if (dyn && launch_dyn_threshold(objective, xbuf, eps, u->coefs_dev, u->state_dev, reinterpret_cast<const DynParams*>(dpar),
                                        DynParams{}, B, n / B, dyn_s, st))
            return 1;
        // guided: x_{t-1} goes to both halves of the next step's input
        float* const dup = guided ? xbuf + n : nullptr;
        if (dpmpp ? launch_dpmpp_update(xbuf, eps, xstart, u->coefs_dev, u->state_dev, xbuf, all_steps, dup, n, st, objective,
                                        dyn_s, n / B)
                  : launch_sampler_update(kind, xbuf, eps, noise, u->coefs_dev, u->state_dev, n, xbuf, all_steps, nullptr, n, st,
                                          objective, xstart, dup, ddim_flags, dyn_s, n / B))
            return 1;
        return launch_step_advance(u->state_dev, st);
    };
    // profiling leg: park the GPU while the host enqueues, so that event intervals are kernel times (<= 8 steps)
    if (!use_graph && prof::enabled() && n_steps <= 8 && launch_spin(8.0 * n_steps, s)) return 1;
    dm_unet::GraphKey key;
    key.kind = dpmpp ? dm_unet::GK_DPMPP : kind == DM_SAMPLER_DDPM ? dm_unet::GK_DDPM : dm_unet::GK_DDIM;
    key.B = B; key.H = H; key.W = W; key.ctx_tokens = ctx_tokens; key.cond_channels = cond_channels;
    key.objective = objective; key.self_cond = self_cond; key.guided = guided;
    key.ddim_flags = ddim_flags;
    key.dyn = dyn;
    key.noise = noise; key.all_steps = all_steps; key.ws = u->ws; key.times = u->times_dev; key.coefs = u->coefs_dev;
    if (run_steps(r, key, n_steps, one_step)) return 1;
    if (launch_finalize(xbuf, out, n, unnormalize, s)) return 1;  // out = x_0 [ (x + 1) / 2 ]
    return run_finish(r);
}

}  // namespace dm

extern "C" {

int dm_sample(dm_unet* u, int kind, int n_steps, const int64_t* times_host, const float* coefs_host,
              const float* x_T, const float* noise, uint64_t seed, uint64_t sample_offset, const float* ctx,
              int ctx_tokens, float* out, float* all_steps, int B, int H, int W, int unnormalize, int use_graph,
              void* stream) {
    return sample_impl(u, kind, n_steps, times_host, coefs_host, x_T, noise, seed, sample_offset, ctx, ctx_tokens,
                       nullptr, 0, out, all_steps, B, H, W, unnormalize, use_graph, stream);
}

int dm_sample_cond(dm_unet* u, int kind, int n_steps, const int64_t* times_host, const float* coefs_host,
                   const float* x_T, const float* noise, uint64_t seed, uint64_t sample_offset, const float* ctx,
                   int ctx_tokens, const float* cond, int cond_channels, float* out, float* all_steps, int B, int H,
                   int W, int unnormalize, int use_graph, void* stream) {
    DM_REQUIRE(cond && cond_channels > 0, "dm_sample_cond needs a condition image");
    return sample_impl(u, kind, n_steps, times_host, coefs_host, x_T, noise, seed, sample_offset, ctx, ctx_tokens, cond,
                       cond_channels, out, all_steps, B, H, W, unnormalize, use_graph, stream);
}

int dm_sample_ex(dm_unet* u, const dm_sample_args* a) { return dm_sample_ex_dyn(u, a, nullptr); }

int dm_sample_ex_dyn(dm_unet* u, const dm_sample_args* a, const dm_sample_dyn_args* dyn) {
    DM_REQUIRE(u && a, "null argument");
    DM_REQUIRE(a->cfg_remove_parallel == 0 || a->cfg_remove_parallel == 1, "cfg_remove_parallel is 0 or 1");
    const CfgParams g{a->cfg_scale, a->cfg_rescaled_phi, a->cfg_keep_parallel_frac, (float)a->cfg_remove_parallel};
    return sample_impl(u, a->kind, a->n_steps, a->times_host, a->coefs_host, a->x_T, a->noise, a->seed, a->sample_offset,
                       a->ctx, a->ctx_tokens, a->cond, a->cond_channels, a->out, a->all_steps, a->B, a->H, a->W,
                       a->unnormalize, a->use_graph, a->stream, a->objective, a->self_condition, a->cfg ? &g : nullptr,
                       a->ddim_flags, dyn);
}

}  // extern "C"
