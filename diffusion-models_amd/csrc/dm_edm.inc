// ElucidatedDiffusion on the C ABI: the float-time forward, the two sampling loops, the training loss + backward and the
// single-pass entry points (dm_op_edm_*).  Included by dm_api.hip; kernels in edm.hip.

namespace dm {

static int edm_handle_ok(dm_unet* u) {
    DM_REQUIRE(u->finalized, "dm_unet_finalize has not been called");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    DM_REQUIRE(!u->infer_stale, "parameters were updated on the device (dm_unet_optimizer_step): call dm_unet_train_sync "
                                "before sampling from this handle");
    DM_REQUIRE(u->cfg.learned_sinusoidal_dim > 0,
               "a real-valued time needs a learned / random sinusoidal U-Net (ElucidatedDiffusion asserts it)");
    return 0;
}

// capture fn(s) into an instantiated graph
static int edm_capture(dm_unet* u, hipStream_t s, const std::function<int(hipStream_t)>& fn, hipGraph_t* g_out,
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

// The loops of DD/elucidated_diffusion.py:129-224.  Like sample_impl, a step touches handle-owned memory only and reads
// everything that differs between two calls of one shape (step table, step counter, seed, Philox offset) as device data,
// so the step graphs are captured once per shape: one Heun step with its two forwards, and the single-forward step the
// loop ends on (sigma_next == 0); one graph for DPM-Solver++.  Both are linear chains.
static int sample_edm_impl(dm_unet* u, const dm_edm_args* a) {
    DM_REQUIRE(a->kind == DM_EDM_HEUN || a->kind == DM_EDM_DPMPP, "unknown EDM sampler kind");
    DM_REQUIRE(a->table_host && a->x_init && a->out, "null argument");
    DM_REQUIRE(a->n_steps > 0 && a->B > 0, "empty run");
    if (edm_handle_ok(u)) return 1;
    DM_REQUIRE(u->cfg.text_mode == DM_TEXT_NONE, "ElucidatedDiffusion calls net(x, t, self_cond) only: no text-conditional U-Net");
    DM_REQUIRE(u->out_dim == u->cfg.channels && u->cfg.input_channels == u->cfg.channels,
               "ElucidatedDiffusion needs a U-Net with out_dim == input channels == channels (no self-conditioning, no image "
               "condition, no learned variance)");
    const int B = a->B, H = a->H, W = a->W, n_steps = a->n_steps, clamp = a->clamp ? 1 : 0;
    const bool heun = a->kind == DM_EDM_HEUN;
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(a->stream);
    const int C = u->cfg.channels;
    const int64_t per = (int64_t)C * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    const float* noise = a->noise;
    const float* tab_host = a->table_host;

    if (!u->state_dev) DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&u->state_dev), 256));
    if (n_steps > u->edm_cap) {
        DM_CHECK_HIP(hipDeviceSynchronize());
        u->drop_graph();
        if (u->edm_tab_dev) (void)hipFree(u->edm_tab_dev);
        u->edm_tab_dev = nullptr;
        u->edm_cap = 0;
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&u->edm_tab_dev), (size_t)n_steps * DM_EDM_COEFS * sizeof(float)));
        u->edm_cap = n_steps;
    }
    const bool own_stream = a->use_graph && s == nullptr;
    if (own_stream) {
        if (!u->cap_stream) DM_CHECK_HIP(hipStreamCreateWithFlags(&u->cap_stream, hipStreamNonBlocking));
        DM_CHECK_HIP(hipStreamSynchronize(nullptr));
        s = u->cap_stream;
    }
    // workspace: Heun [x | xhat | xin | F | d | forward arena], DPM++ [x | xin | F | d_old | forward arena]
    const int n_bufs = heun ? 5 : 4;
    Arena dry;
    dry.dry = true;
    for (int i = 0; i < n_bufs; ++i) dry.alloc(n);
    const float* tf_marker = reinterpret_cast<const float*>(16);
    if (unet_forward_impl(u, dry, nullptr, nullptr, nullptr, u->state_dev, nullptr, 0, nullptr, B, H, W, s, nullptr, tf_marker,
                          DM_EDM_COEFS))
        return 1;
    if (ensure_workspace(u, dry.off)) return 1;

    if (u->order_after_previous(s)) return 1;
    SamplerState st_host{};
    st_host.step = 0;
    st_host.n_steps = n_steps;
    st_host.seed = a->seed;
    const uint64_t elem_off = a->sample_offset * (uint64_t)per;
    st_host.off4 = elem_off / 4;
    DM_CHECK_HIP(hipMemcpyAsync(u->edm_tab_dev, tab_host, (size_t)n_steps * DM_EDM_COEFS * sizeof(float), hipMemcpyHostToDevice, s));
    DM_CHECK_HIP(hipMemcpyAsync(u->state_dev, &st_host, sizeof(st_host), hipMemcpyHostToDevice, s));
    DM_CHECK_HIP(hipStreamSynchronize(s));  // st_host may go away when this function returns

    Arena A;
    A.base = u->ws;
    A.cap = u->ws_cap;
    float* x = A.alloc(n);
    float* xhat = heun ? A.alloc(n) : nullptr;
    float* xin = A.alloc(n);
    float* F = A.alloc(n);
    float* d = A.alloc(n);  // Heun: d of the Euler step; DPM++: the previous step's denoised image
    const std::vector<Arena::Blk> arena_mark = A.blks;
    const float* tab = u->edm_tab_dev;
    const EdmRows rows{tab, u->state_dev, EDM_ROW_STEP, per};

    if (launch_edm_scale(a->x_init, a->sigma_init, x, n, s)) return 1;  // images = sigmas[0] * randn (:151, :201)
    if (!heun) DM_CHECK_HIP(hipMemsetAsync(d, 0, n * sizeof(float), s));

    auto forward = [&](hipStream_t st, int col) -> int {
        A.blks = arena_mark;
        return unet_forward_impl(u, A, xin, nullptr, nullptr, u->state_dev, nullptr, 0, F, B, H, W, st, nullptr, tab + col,
                                 DM_EDM_COEFS);
    };
    // second == false: the loop's last step, images = images_next of the Euler step (:176)
    auto heun_step = [&](hipStream_t st, bool second) -> int {
        if (launch_edm_churn_in(x, noise, n, rows, xhat, xin, n, st)) return 1;
        if (forward(st, EDM_C_NOISE)) return 1;
        if (launch_edm_euler(xhat, F, rows, clamp, nullptr, d, x, second ? xin : nullptr, n, st)) return 1;
        if (second) {
            if (forward(st, EDM_C_NOISE2)) return 1;
            if (launch_edm_heun(xhat, d, x, F, rows, clamp, x, n, st)) return 1;
        }
        return launch_step_advance(u->state_dev, st);
    };
    auto dpmpp_step = [&](hipStream_t st) -> int {
        if (launch_edm_churn_in(x, nullptr, 0, rows, nullptr, xin, n, st)) return 1;  // churn column is 0: xin = c_in x
        if (forward(st, EDM_C_NOISE)) return 1;
        if (launch_edm_dpmpp(x, F, d, rows, x, n, st)) return 1;
        return launch_step_advance(u->state_dev, st);
    };
    auto is_full = [&](int i) { return heun && tab_host[(size_t)i * DM_EDM_COEFS + EDM_SIGMA2] != 0.0f; };
    auto finish = [&]() -> int {
        if (launch_edm_finalize(x, a->out, n, s)) return 1;
        if (u->mark_done(s)) return 1;
        if (own_stream) DM_CHECK_HIP(hipStreamSynchronize(s));
        return 0;
    };

    if (!a->use_graph) {
        for (int i = 0; i < n_steps; ++i)
            if (heun ? heun_step(s, is_full(i)) : dpmpp_step(s)) return 1;
        return finish();
    }
    dm_unet::GraphKey key;
    // the handle's graph slot is shared with DDPM / DDIM: EDM kinds follow the DM_SAMPLER_* values
    constexpr int kEdmKindBase = 2;
    static_assert(DM_SAMPLER_DDPM < kEdmKindBase && DM_SAMPLER_DDIM < kEdmKindBase && DM_EDM_HEUN >= 0 && DM_EDM_DPMPP >= 0,
                  "EDM graph kinds must not collide with DM_SAMPLER_*");
    key.kind = kEdmKindBase + a->kind;
    key.B = B; key.H = H; key.W = W;
    key.edm_clamp = clamp;
    key.noise = noise; key.ws = u->ws; key.coefs = u->edm_tab_dev;
    if (!(u->gkey == key)) {
        u->drop_graph();
        u->gkey = key;
    }
    for (int i = 0; i < n_steps; ++i) {
        const bool full = heun ? is_full(i) : true;
        hipGraph_t* g = full ? &u->graph : &u->edm_last_graph;
        hipGraphExec_t* e = full ? &u->gexec : &u->edm_last_gexec;
        if (!*e) {
            const std::function<int(hipStream_t)> fn = [&](hipStream_t st) { return heun ? heun_step(st, full) : dpmpp_step(st); };
            if (edm_capture(u, s, fn, g, e)) {
                u->drop_graph();
                return 1;
            }
        }
        DM_CHECK_HIP(hipGraphLaunch(*e, s));
    }
    return finish();
}

// one stand-alone pass: upload `rows` table rows, run fn, wait
static int edm_op(const float* c_host, int rows, void* stream, const std::function<int(const float*, hipStream_t)>& fn) {
    DM_REQUIRE(c_host && rows > 0, "null step table");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* cd = nullptr;
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&cd), (size_t)rows * DM_EDM_COEFS * sizeof(float)));
    hipError_t e = hipMemcpy(cd, c_host, (size_t)rows * DM_EDM_COEFS * sizeof(float), hipMemcpyHostToDevice);
    int rc = 0;
    if (e == hipSuccess) {
        rc = fn(cd, s);
        e = hipStreamSynchronize(s);
    }
    (void)hipFree(cd);
    if (!rc && e != hipSuccess) {
        set_error(std::string("kernel execution failed: ") + hipGetErrorString(e));
        rc = 1;
    }
    return rc;
}
// rows == 1: one row for every image; rows == B: row b for image b
static int edm_rows(const float* tab, int rows, int B, int64_t per, EdmRows* out) {
    DM_REQUIRE(B > 0 && per > 0, "empty tensor");
    DM_REQUIRE(rows == 1 || rows == B, "the step table has one row, or one row per image");
    *out = EdmRows{tab, nullptr, rows == B && B > 1 ? EDM_ROW_IMAGE : EDM_ROW_FIRST, per};
    return 0;
}

// ElucidatedDiffusion.forward (DD/elucidated_diffusion.py:234-264) + backward on a handle armed by dm_unet_train_enable_ft:
// the noise-in pass, the tape forward with c_noise(sigma) as a float time, the weighted loss with its gradient, then the
// backward pass of the p_losses path, which goes on through time_mlp.1 into the embedding's weights.  Workspace, arena and
// stream ordering follow loss_backward_impl.
static int loss_backward_edm_impl(dm_unet* u, const dm_edm_train_args& a) {
    DM_REQUIRE(a.images && a.noise && a.coef_host, "null argument");
    DM_REQUIRE(u->train && u->train->ft, "dm_unet_train_enable_ft has not been called");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    const int cstride = a.coef_stride ? a.coef_stride : DM_EDM_COEFS;
    DM_REQUIRE(a.B > 0 && cstride > EDM_LOSS_W, "coef_host rows hold at least 15 floats (loss_weight is column 14)");
    DM_REQUIRE(u->cfg.text_mode == DM_TEXT_NONE && u->out_dim == u->cfg.channels && u->cfg.input_channels == u->cfg.channels,
               "ElucidatedDiffusion needs a U-Net with out_dim == input channels == channels and no text conditioning");
    const int B = a.B, H = a.H, W = a.W, accumulate = a.accumulate ? 1 : 0;
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(a.stream);
    TrainState& T = *u->train;
    if (B > T.edm_cap_B) {
        DM_CHECK_HIP(hipDeviceSynchronize());
        if (T.edm_coef_dev) (void)hipFree(T.edm_coef_dev);
        if (T.tf_dev) (void)hipFree(T.tf_dev);
        T.edm_coef_dev = nullptr; T.tf_dev = nullptr; T.edm_cap_B = 0;
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.edm_coef_dev), (size_t)B * DM_EDM_COEFS * sizeof(float)));
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.tf_dev), (size_t)B * sizeof(float)));
        T.edm_cap_B = B;
    }
    const int64_t per = (int64_t)u->cfg.channels * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    const EdmRows rows{T.edm_coef_dev, nullptr, B > 1 ? EDM_ROW_IMAGE : EDM_ROW_FIRST, per};
    auto run = [&](Arena& A, Tape& tp) -> int {
        float* x0 = A.alloc(n);
        float* noised = A.alloc(n);
        float* xin = A.alloc(n);
        float* F = A.alloc(n);
        float* dF = A.alloc(n);
        float* part = A.alloc(B);
        if (!A.dry && launch_edm_noise_in(a.images, a.noise, rows, x0, noised, xin, n, s)) return 1;
        if (unet_train_forward(u, A, xin, nullptr, F, B, H, W, s, tp, nullptr, 0, nullptr, T.tf_dev)) return 1;
        if (!A.dry && launch_edm_loss(noised, F, x0, T.edm_coef_dev, dF, a.denoised_out, part, T.loss_dev, B, per, a.loss_scale, s))
            return 1;
        return unet_train_backward(u, A, xin, dF, B, H, W, s, tp, accumulate);
    };
    try {
        // (the fourth entry is self_cond on the integer-time path, never negative there)
        const std::array<long long, 8> key{B, H, W, -1, 0, 0, 0, (a.denoised_out ? 1 : 0) | (T.bucketed ? 2 : 0)};
        auto known = T.ws_need.find(key);
        if (known == T.ws_need.end()) {
            Arena dry;
            dry.dry = true;
            Tape tp;
            if (run(dry, tp)) return 1;
            known = T.ws_need.emplace(key, dry.off).first;
        }
        if (ensure_train_ws(T, known->second)) return 1;
        if (u->order_after_previous(s)) return 1;
        // rows as the kernels index them (DM_EDM_COEFS floats), then the B float times the embedding reads
        T.coef_stage.assign((size_t)B * DM_EDM_COEFS + B, 0.f);
        const int ncopy = cstride < DM_EDM_COEFS ? cstride : DM_EDM_COEFS;
        for (int b = 0; b < B; ++b) {
            std::memcpy(&T.coef_stage[(size_t)b * DM_EDM_COEFS], a.coef_host + (size_t)b * cstride, ncopy * sizeof(float));
            T.coef_stage[(size_t)B * DM_EDM_COEFS + b] = a.coef_host[(size_t)b * cstride + EDM_C_NOISE];
        }
        DM_CHECK_HIP(hipMemcpyAsync(T.edm_coef_dev, T.coef_stage.data(), (size_t)B * DM_EDM_COEFS * sizeof(float),
                                    hipMemcpyHostToDevice, s));
        DM_CHECK_HIP(hipMemcpyAsync(T.tf_dev, T.coef_stage.data() + (size_t)B * DM_EDM_COEFS, (size_t)B * sizeof(float),
                                    hipMemcpyHostToDevice, s));
        Arena A;
        A.base = T.ws;
        A.cap = T.ws_cap;
        Tape tp;
        if (run(A, tp)) return 1;
        T.drop_call += 1;
        DM_REQUIRE(A.off <= T.ws_cap, "training workspace overrun: the dry run and the real run allocated differently");
    } catch (const std::exception& e) {
        set_error(e.what());
        return 1;
    }
    if (u->mark_done(s)) return 1;
    if (!a.loss_out_host) return 0;  // asynchronous form: the loss stays on the device (dm_unet_train_scalar)
    DM_CHECK_HIP(hipMemcpyAsync(a.loss_out_host, T.loss_dev, sizeof(float), hipMemcpyDeviceToHost, s));
    DM_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // namespace dm

extern "C" {

int dm_unet_forward_ft(dm_unet* u, const float* x, const float* time, const float* ctx, int ctx_tokens, float* out, int B,
                       int H, int W, void* stream) {
    DM_REQUIRE(u && x && time && out, "null argument");
    if (edm_handle_ok(u)) return 1;
    DM_REQUIRE(B > 0, "empty batch");
    DM_REQUIRE((ctx == nullptr) == (ctx_tokens == 0), "ctx and ctx_tokens come together");
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Arena dry;
    dry.dry = true;
    if (unet_forward_impl(u, dry, x, nullptr, nullptr, nullptr, ctx, ctx_tokens, out, B, H, W, s, nullptr, time, 0)) return 1;
    if (ensure_workspace(u, dry.off)) return 1;
    Arena A;
    A.base = u->ws;
    A.cap = u->ws_cap;
    if (u->order_after_previous(s)) return 1;
    if (unet_forward_impl(u, A, x, nullptr, nullptr, nullptr, ctx, ctx_tokens, out, B, H, W, s, nullptr, time, 0)) return 1;
    return u->mark_done(s);
}

int dm_sample_edm(dm_unet* u, const dm_edm_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return sample_edm_impl(u, a);
}

int dm_op_edm_churn_in(const float* x, const float* eps, const float* c_host, int rows, uint64_t seed, uint64_t draw,
                       uint64_t element_offset, float* xhat, float* xin, int B, int64_t per, void* stream) {
    DM_REQUIRE(x && xin, "null argument");
    DM_REQUIRE(element_offset % 4 == 0, "Philox element offset must be a multiple of 4 (one counter serves 4 elements)");
    DM_REQUIRE(eps || draw >= 1, "Philox draw 0 is the initial noise: a step's draw is its index + 1");
    // the kernel draws `step + 1`: a state with step = draw - 1 selects the draw; the table row is 0 or the image's
    SamplerState st_host{};
    st_host.step = eps ? 0 : (int)(draw - 1);
    st_host.n_steps = st_host.step + 1;
    st_host.seed = seed;
    st_host.off4 = element_offset / 4;
    SamplerState* st_dev = nullptr;
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&st_dev), sizeof(SamplerState)));
    hipError_t e = hipMemcpy(st_dev, &st_host, sizeof(st_host), hipMemcpyHostToDevice);
    int rc = 1;
    if (e == hipSuccess) {
        rc = edm_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
            EdmRows r;
            if (edm_rows(cd, rows, B, per, &r)) return 1;
            r.st = st_dev;
            return launch_edm_churn_in(x, eps, 0, r, xhat, xin, (int64_t)B * per, s);
        });
    } else {
        set_error(std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    (void)hipFree(st_dev);
    return rc;
}

int dm_op_edm_euler(const float* xhat, const float* F, const float* c_host, int rows, int clamp, float* D_out, float* d_out,
                    float* xnext, float* xin_next, int B, int64_t per, void* stream) {
    DM_REQUIRE(xhat && F, "null argument");
    return edm_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        EdmRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_edm_euler(xhat, F, r, clamp ? 1 : 0, D_out, d_out, xnext, xin_next, (int64_t)B * per, s);
    });
}

int dm_op_edm_heun(const float* xhat, const float* d, const float* xnext, const float* F2, const float* c_host, int rows,
                   int clamp, float* out, int B, int64_t per, void* stream) {
    DM_REQUIRE(xhat && d && xnext && F2 && out, "null argument");
    return edm_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        EdmRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_edm_heun(xhat, d, xnext, F2, r, clamp ? 1 : 0, out, (int64_t)B * per, s);
    });
}

int dm_op_edm_dpmpp(const float* x, const float* F, float* d_old, const float* c_host, int rows, float* out, int B,
                    int64_t per, void* stream) {
    DM_REQUIRE(x && F && d_old && out, "null argument");
    return edm_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        EdmRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_edm_dpmpp(x, F, d_old, r, out, (int64_t)B * per, s);
    });
}

int dm_op_edm_finalize(const float* x, float* out, int64_t n, void* stream) {
    DM_REQUIRE(x && out, "null argument");
    return launch_edm_finalize(x, out, n, static_cast<hipStream_t>(stream));
}

int dm_unet_train_enable_ft(dm_unet* u, int time_weights_frozen) {
    DM_REQUIRE(u && u->finalized, "dm_unet_train_enable_ft needs a finalized handle");
    DM_REQUIRE(u->cfg.learned_sinusoidal_dim > 0,
               "float-time training is for the learned / random sinusoidal U-Net ElucidatedDiffusion asserts: every other U-Net "
               "trains through dm_unet_train_enable");
    DM_REQUIRE(u->cfg.text_mode == DM_TEXT_NONE && u->out_dim == u->cfg.channels && u->cfg.input_channels == u->cfg.channels,
               "ElucidatedDiffusion needs a U-Net with out_dim == input channels == channels and no text conditioning");
    if (train_enable_impl(u, true)) return 1;
    // the handle's configuration does not say which of the two embeddings it holds: the caller does, at the one call that arms it
    u->train->freqs_frozen = time_weights_frozen != 0;
    return 0;
}

int dm_unet_loss_backward_edm(dm_unet* u, const dm_edm_train_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return loss_backward_edm_impl(u, *a);
}

int dm_op_edm_noise_in(const float* images, const float* eps, const float* c_host, int rows, float* x0, float* noised,
                       float* xin, int B, int64_t per, void* stream) {
    DM_REQUIRE(images && eps && x0 && noised && xin, "null argument");
    return edm_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        EdmRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_edm_noise_in(images, eps, r, x0, noised, xin, (int64_t)B * per, s);
    });
}

int dm_op_edm_loss(const float* noised, const float* F, const float* x0, const float* c_host, float loss_scale, float* dF,
                   float* D_out, float* loss_out_host, int B, int64_t per, void* stream) {
    DM_REQUIRE(noised && F && x0 && dF && loss_out_host && B > 0, "null argument");
    float* scratch = nullptr;  // [B] per-image partials, then the loss
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&scratch), ((size_t)B + 1) * sizeof(float)));
    int rc = edm_op(c_host, B, stream, [&](const float* cd, hipStream_t s) {
        return launch_edm_loss(noised, F, x0, cd, dF, D_out, scratch, scratch + B, B, per, loss_scale, s);
    });
    if (!rc && hipMemcpy(loss_out_host, scratch + B, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("dm_op_edm_loss: reading the loss back failed");
        rc = 1;
    }
    (void)hipFree(scratch);
    return rc;
}

int dm_op_sinusoid_ft_bwd(const float* de0, const float* e0, float* dw, int B, int half, int learned, int accumulate,
                          void* stream) {
    DM_REQUIRE(de0 && e0 && dw && B > 0 && half > 0, "bad argument");
    return launch_sinusoid_ft_bwd(de0, e0, dw, B, half, learned != 0, accumulate, static_cast<hipStream_t>(stream));
}

}  // extern "C"
