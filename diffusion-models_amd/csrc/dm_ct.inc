// Continuous-time Gaussian diffusion on the C ABI: the sampling loop, the training loss + backward and the single-pass
// entry points (dm_op_ct_*).  Included by dm_api.hip after dm_edm.inc (whose handle checks, capture helper and row helper
// it shares); kernels in ct.hip.

namespace dm {

static_assert(DM_CT_COEFS == CT_NCOLS && DM_CT_COEFS == DM_EDM_COEFS,
              "the continuous-time table shares the handle's EDM table buffers: the row widths must agree");
static_assert(DM_CT_PRED_NOISE == CT_PRED_NOISE && DM_CT_PRED_V == CT_PRED_V, "objective ids of the header and ct.h");

static int ct_unet_ok(dm_unet* u) {
    DM_REQUIRE(u->cfg.text_mode == DM_TEXT_NONE,
               "continuous-time diffusion calls model(x, log_snr) only: no text-conditional U-Net");
    DM_REQUIRE(u->out_dim == u->cfg.channels && u->cfg.input_channels == u->cfg.channels,
               "continuous-time diffusion needs a U-Net with out_dim == input channels == channels (no self-conditioning, no "
               "image condition, no learned variance)");
    return 0;
}

// p_sample_loop of DD/continuous_time_gaussian_diffusion.py:199-213 (and the v class, :115-129).  One step -- the forward
// at log_snr(t_i), ct_step, the step counter -- is one linear chain that reads everything that differs between two calls
// of one shape (table, step counter, seed, Philox offset) as device data, so it is captured once per shape.
static int sample_ct_impl(dm_unet* u, const dm_ct_args* a) {
    DM_REQUIRE(a->objective == DM_CT_PRED_NOISE || a->objective == DM_CT_PRED_V, "unknown continuous-time objective");
    DM_REQUIRE(a->table_host && a->x_init && a->out, "null argument");
    DM_REQUIRE(a->n_steps > 0 && a->B > 0, "empty run");
    if (edm_handle_ok(u)) return 1;
    if (ct_unet_ok(u)) return 1;
    const int B = a->B, H = a->H, W = a->W, n_steps = a->n_steps, clip = a->clip ? 1 : 0, objective = a->objective;
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(a->stream);
    const int C = u->cfg.channels;
    const int64_t per = (int64_t)C * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    const float* noise = a->noise;
    const float* tab_host = a->table_host;
    // the noise tensor has n_steps - 1 rows: the step that would read row n_steps - 1 must be the one that adds none
    DM_REQUIRE(!noise || tab_host[(size_t)(n_steps - 1) * DM_CT_COEFS + CT_SQRT_VAR] == 0.0f,
               "with a noise tensor the last table row must have c[6] == 0 (time_next == 0 adds no noise)");

    if (!u->state_dev) DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&u->state_dev), 256));
    if (n_steps > u->edm_cap) {
        DM_CHECK_HIP(hipDeviceSynchronize());
        u->drop_graph();
        if (u->edm_tab_dev) (void)hipFree(u->edm_tab_dev);
        u->edm_tab_dev = nullptr;
        u->edm_cap = 0;
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&u->edm_tab_dev), (size_t)n_steps * DM_CT_COEFS * sizeof(float)));
        u->edm_cap = n_steps;
    }
    const bool own_stream = a->use_graph && s == nullptr;
    if (own_stream) {
        if (!u->cap_stream) DM_CHECK_HIP(hipStreamCreateWithFlags(&u->cap_stream, hipStreamNonBlocking));
        DM_CHECK_HIP(hipStreamSynchronize(nullptr));
        s = u->cap_stream;
    }
    // workspace: [x | F | forward arena]
    Arena dry;
    dry.dry = true;
    for (int i = 0; i < 2; ++i) dry.alloc(n);
    const float* tf_marker = reinterpret_cast<const float*>(16);
    if (unet_forward_impl(u, dry, nullptr, nullptr, nullptr, u->state_dev, nullptr, 0, nullptr, B, H, W, s, nullptr, tf_marker,
                          DM_CT_COEFS))
        return 1;
    if (ensure_workspace(u, dry.off)) return 1;

    if (u->order_after_previous(s)) return 1;
    SamplerState st_host{};
    st_host.step = 0;
    st_host.n_steps = n_steps;
    st_host.seed = a->seed;
    const uint64_t elem_off = a->sample_offset * (uint64_t)per;
    st_host.off4 = elem_off / 4;
    DM_CHECK_HIP(hipMemcpyAsync(u->edm_tab_dev, tab_host, (size_t)n_steps * DM_CT_COEFS * sizeof(float), hipMemcpyHostToDevice, s));
    DM_CHECK_HIP(hipMemcpyAsync(u->state_dev, &st_host, sizeof(st_host), hipMemcpyHostToDevice, s));
    DM_CHECK_HIP(hipStreamSynchronize(s));  // st_host may go away when this function returns

    Arena A;
    A.base = u->ws;
    A.cap = u->ws_cap;
    float* x = A.alloc(n);
    float* F = A.alloc(n);
    const std::vector<Arena::Blk> arena_mark = A.blks;
    const float* tab = u->edm_tab_dev;
    const EdmRows rows{tab, u->state_dev, EDM_ROW_STEP, per};

    DM_CHECK_HIP(hipMemcpyAsync(x, a->x_init, n * sizeof(float), hipMemcpyDeviceToDevice, s));  // img = randn(shape)

    auto step = [&](hipStream_t st) -> int {
        A.blks = arena_mark;
        if (unet_forward_impl(u, A, x, nullptr, nullptr, u->state_dev, nullptr, 0, F, B, H, W, st, nullptr, tab + CT_LOG_SNR,
                              DM_CT_COEFS))
            return 1;
        if (launch_ct_step(x, F, noise, n, rows, objective, clip, x, nullptr, n, st)) return 1;
        return launch_step_advance(u->state_dev, st);
    };
    auto finish = [&]() -> int {
        if (launch_edm_finalize(x, a->out, n, s)) return 1;
        if (u->mark_done(s)) return 1;
        if (own_stream) DM_CHECK_HIP(hipStreamSynchronize(s));
        return 0;
    };

    if (!a->use_graph) {
        for (int i = 0; i < n_steps; ++i)
            if (step(s)) return 1;
        return finish();
    }
    dm_unet::GraphKey key;
    // the handle's graph slot is shared with DDPM / DDIM (DM_SAMPLER_*) and EDM (2 + DM_EDM_*)
    constexpr int kCtKind = 4;
    static_assert(DM_SAMPLER_DDPM < kCtKind && DM_SAMPLER_DDIM < kCtKind && 2 + DM_EDM_HEUN < kCtKind && 2 + DM_EDM_DPMPP < kCtKind,
                  "the continuous-time graph kind must not collide with DM_SAMPLER_* or the EDM kinds");
    key.kind = kCtKind;
    key.B = B; key.H = H; key.W = W;
    key.objective = objective;
    key.edm_clamp = clip;
    key.noise = noise; key.ws = u->ws; key.coefs = u->edm_tab_dev;
    if (!(u->gkey == key)) {
        u->drop_graph();
        u->gkey = key;
    }
    if (!u->gexec) {
        const std::function<int(hipStream_t)> fn = step;
        if (edm_capture(u, s, fn, &u->graph, &u->gexec)) {
            u->drop_graph();
            return 1;
        }
    }
    for (int i = 0; i < n_steps; ++i) DM_CHECK_HIP(hipGraphLaunch(u->gexec, s));
    return finish();
}

// p_losses of both classes (+ forward's normalisation) and the backward pass on a handle armed by dm_unet_train_enable_ft:
// q_sample with the target, the tape forward with log_snr_b as the float time, the weighted loss with its gradient, then
// the backward pass, which goes on through time_mlp.1 into the embedding's weights.  Workspace, arena and stream ordering
// follow loss_backward_edm_impl; the per-image rows and times use its device buffers (the row widths agree).
static int loss_backward_ct_impl(dm_unet* u, const dm_ct_train_args& a) {
    DM_REQUIRE(a.images && a.noise && a.coef_host, "null argument");
    DM_REQUIRE(a.objective == DM_CT_PRED_NOISE || a.objective == DM_CT_PRED_V, "unknown continuous-time objective");
    DM_REQUIRE(u->train && u->train->ft, "dm_unet_train_enable_ft has not been called");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    const int cstride = a.coef_stride ? a.coef_stride : DM_CT_COEFS;
    DM_REQUIRE(a.B > 0 && cstride > CT_LOSS_W, "coef_host rows hold at least 10 floats (the loss weight is column 9)");
    if (ct_unet_ok(u)) return 1;
    const int B = a.B, H = a.H, W = a.W, accumulate = a.accumulate ? 1 : 0, objective = a.objective;
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(a.stream);
    TrainState& T = *u->train;
    if (B > T.edm_cap_B) {
        DM_CHECK_HIP(hipDeviceSynchronize());
        if (T.edm_coef_dev) (void)hipFree(T.edm_coef_dev);
        if (T.tf_dev) (void)hipFree(T.tf_dev);
        T.edm_coef_dev = nullptr; T.tf_dev = nullptr; T.edm_cap_B = 0;
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.edm_coef_dev), (size_t)B * DM_CT_COEFS * sizeof(float)));
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.tf_dev), (size_t)B * sizeof(float)));
        T.edm_cap_B = B;
    }
    const int64_t per = (int64_t)u->cfg.channels * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    const EdmRows rows{T.edm_coef_dev, nullptr, B > 1 ? EDM_ROW_IMAGE : EDM_ROW_FIRST, per};
    auto run = [&](Arena& A, Tape& tp) -> int {
        float* x = A.alloc(n);
        float* target = A.alloc(n);
        float* F = A.alloc(n);
        float* dF = A.alloc(n);
        float* part = A.alloc(B);
        if (!A.dry && launch_ct_noise_in(a.images, a.noise, rows, objective, a.normalize, x, target, n, s)) return 1;
        if (unet_train_forward(u, A, x, nullptr, F, B, H, W, s, tp, nullptr, 0, nullptr, T.tf_dev)) return 1;
        if (!A.dry && launch_ct_loss(F, target, T.edm_coef_dev, dF, part, T.loss_dev, B, per, a.loss_scale, s)) return 1;
        return unet_train_backward(u, A, x, dF, B, H, W, s, tp, accumulate);
    };
    try {
        // (the fourth entry is self_cond on the integer-time path, never negative there, and -1 on the EDM path)
        const std::array<long long, 8> key{B, H, W, -2, 0, 0, 0, T.bucketed ? 2 : 0};
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
        // rows as the kernels index them (DM_CT_COEFS floats), then the B float times the embedding reads
        T.coef_stage.assign((size_t)B * DM_CT_COEFS + B, 0.f);
        const int ncopy = cstride < DM_CT_COEFS ? cstride : DM_CT_COEFS;
        for (int b = 0; b < B; ++b) {
            std::memcpy(&T.coef_stage[(size_t)b * DM_CT_COEFS], a.coef_host + (size_t)b * cstride, ncopy * sizeof(float));
            T.coef_stage[(size_t)B * DM_CT_COEFS + b] = a.coef_host[(size_t)b * cstride + CT_LOG_SNR];
        }
        DM_CHECK_HIP(hipMemcpyAsync(T.edm_coef_dev, T.coef_stage.data(), (size_t)B * DM_CT_COEFS * sizeof(float),
                                    hipMemcpyHostToDevice, s));
        DM_CHECK_HIP(hipMemcpyAsync(T.tf_dev, T.coef_stage.data() + (size_t)B * DM_CT_COEFS, (size_t)B * sizeof(float),
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

int dm_sample_ct(dm_unet* u, const dm_ct_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return sample_ct_impl(u, a);
}

int dm_unet_loss_backward_ct(dm_unet* u, const dm_ct_train_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return loss_backward_ct_impl(u, *a);
}

int dm_op_ct_step(const float* x, const float* F, const float* eps, const float* c_host, int rows, int objective, int clip,
                  uint64_t seed, uint64_t draw, uint64_t element_offset, float* out, float* x_start_out, int B, int64_t per,
                  void* stream) {
    DM_REQUIRE(x && F && out, "null argument");
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
            return launch_ct_step(x, F, eps, 0, r, objective, clip ? 1 : 0, out, x_start_out, (int64_t)B * per, s);
        });
    } else {
        set_error(std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    (void)hipFree(st_dev);
    return rc;
}

int dm_op_ct_noise_in(const float* images, const float* eps, const float* c_host, int rows, int objective, int normalize,
                      float* x, float* target, int B, int64_t per, void* stream) {
    DM_REQUIRE(images && eps && x && target, "null argument");
    return edm_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        EdmRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_ct_noise_in(images, eps, r, objective, normalize, x, target, (int64_t)B * per, s);
    });
}

int dm_op_ct_loss(const float* F, const float* target, const float* c_host, float loss_scale, float* dF, float* loss_out_host,
                  int B, int64_t per, void* stream) {
    DM_REQUIRE(F && target && dF && loss_out_host && B > 0, "null argument");
    float* scratch = nullptr;  // [B] per-image partials, then the loss
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&scratch), ((size_t)B + 1) * sizeof(float)));
    int rc = edm_op(c_host, B, stream, [&](const float* cd, hipStream_t s) {
        return launch_ct_loss(F, target, cd, dF, scratch, scratch + B, B, per, loss_scale, s);
    });
    if (!rc && hipMemcpy(loss_out_host, scratch + B, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("dm_op_ct_loss: reading the loss back failed");
        rc = 1;
    }
    (void)hipFree(scratch);
    return rc;
}

}  // extern "C"
