// Continuous-time Gaussian diffusion on the C ABI: the sampling loop, the training loss + backward and the single-pass
// entry points (dm_op_ct_*).  Included by dm_api.hip after dm_sampler.inc (the loop scaffolding) and dm_edm.inc (the
// float-time handle check, the float-time training driver, the row and state helpers of the dm_op_* passes); kernels in
// ct.hip.

namespace dm {

static_assert(DM_CT_COEFS == CT_NCOLS && DM_CT_COEFS == DM_EDM_COEFS,
              "the continuous-time table shares the handle's EDM table buffers: the row widths must agree");
static_assert(DM_CT_PRED_NOISE == CT_PRED_NOISE && DM_CT_PRED_V == CT_PRED_V, "objective ids of the header and ct.h");

static int ct_unet_ok(dm_unet* u) {
    return plain_unet_ok(u,
                         "continuous-time diffusion needs a U-Net with out_dim == input channels == channels (no self-conditioning, no "
                         "image condition, no learned variance)",
                         "continuous-time diffusion calls model(x, log_snr) only: no text-conditional U-Net");
}

// The two loops of the continuous-time classes as one argument list: dm_ct_args, or dm_ct_dpmpp_args with dpmpp set
// (then nothing is drawn: noise, seed and sample_offset stay 0).
struct CtLoop {
    int objective, clip, n_steps;
    const float* table_host;
    const float* x_init;
    const float* noise;
    uint64_t seed, sample_offset;
    float* out;
    float* x_out;  // DPM-Solver++ only (optional): the final iterate in front of the finalize pass
    int B, H, W, use_graph;
    void* stream;
    bool dpmpp;
};

// p_sample_loop of DD/continuous_time_gaussian_diffusion.py:199-213 (and the v class, :115-129).  One step -- the forward
// at log_snr(t_i), ct_step, the step counter -- is one linear chain that reads everything that differs between two calls
// of one shape (table, step counter, seed, Philox offset) as device data, so it is captured once per shape.
// dpmpp: the DPM-Solver++ (2M) loop on a ct_dpmpp_table instead -- the same chain with ct_dpmpp_step in the place of ct_step
// and one more buffer, the previous step's x_start, which the first row (g == 0) leaves unread.  N, order and node spacing
// are table data, so its graph (a kind of its own) serves them all.
static int sample_ct_impl(dm_unet* u, const CtLoop* a) {
    DM_REQUIRE(a->objective == DM_CT_PRED_NOISE || a->objective == DM_CT_PRED_V, "unknown continuous-time objective");
    DM_REQUIRE(a->table_host && a->x_init && a->out, "null argument");
    DM_REQUIRE(a->n_steps > 0 && a->B > 0, "empty run");
    if (edm_handle_ok(u)) return 1;
    if (ct_unet_ok(u)) return 1;
    const int B = a->B, H = a->H, W = a->W, n_steps = a->n_steps, clip = a->clip ? 1 : 0, objective = a->objective;
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    const int C = u->cfg.channels;
    const int64_t per = (int64_t)C * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    const bool dpmpp = a->dpmpp;
    const float* noise = a->noise;
    const float* tab_host = a->table_host;
    // the noise tensor has n_steps - 1 rows: the step that would read row n_steps - 1 must be the one that adds none
    DM_REQUIRE(!noise || tab_host[(size_t)(n_steps - 1) * DM_CT_COEFS + CT_SQRT_VAR] == 0.0f,
               "with a noise tensor the last table row must have c[6] == 0 (time_next == 0 adds no noise)");
    DM_REQUIRE(!dpmpp || tab_host[CT_DPM_G] == 0.0f,
               "the first DPM-Solver++ row must have c[12] == 0: there is no earlier x_start to extrapolate from");

    SamplerRun r;
    if (grow_tables(u, TAB_FLOAT, n_steps, 1) || run_begin(r, u, a->stream, a->use_graph)) return 1;
    hipStream_t s = r.s;
    // workspace: [x | F | forward arena], DPM-Solver++ [x | F | hist | forward arena]
    float *x, *F, *hist;
    auto layout = [&](Arena& A) {
        x = A.alloc(n);
        F = A.alloc(n);
        hist = dpmpp ? A.alloc(n) : nullptr;
    };
    const float* tf_marker = reinterpret_cast<const float*>(16);
    if (run_workspace(r, layout, [&](Arena& dry) {
            return unet_forward_impl(u, dry, nullptr, nullptr, nullptr, u->state_dev, nullptr, 0, nullptr, B, H, W, s, nullptr,
                                     tf_marker, DM_CT_COEFS);
        }))
        return 1;
    if (run_upload(r, n_steps, nullptr, nullptr, tab_host, 0, a->seed, a->sample_offset * (uint64_t)per)) return 1;
    const float* tab = u->edm_tab_dev;
    const StepRows rows{tab, u->state_dev, STEP_ROW_STEP, per};

    DM_CHECK_HIP(hipMemcpyAsync(x, a->x_init, n * sizeof(float), hipMemcpyDeviceToDevice, s));  // img = randn(shape)

    auto step = [&](hipStream_t st) -> int {
        r.rewind();
        if (unet_forward_impl(u, r.A, x, nullptr, nullptr, u->state_dev, nullptr, 0, F, B, H, W, st, nullptr, tab + CT_LOG_SNR,
                              DM_CT_COEFS))
            return 1;
        if (dpmpp ? launch_ct_dpmpp_step(x, F, hist, rows, objective, clip, x, n, st)
                  : launch_ct_step(x, F, noise, n, rows, objective, clip, x, nullptr, n, st))
            return 1;
        return launch_step_advance(u->state_dev, st);
    };
    dm_unet::GraphKey key;
    key.kind = dpmpp ? dm_unet::GK_CT_DPMPP : dm_unet::GK_CT;
    key.B = B; key.H = H; key.W = W;
    key.objective = objective;
    key.ct_clip = clip;
    key.noise = noise; key.ws = u->ws; key.tab = u->edm_tab_dev;
    if (run_steps(r, key, n_steps, step)) return 1;
    if (a->x_out) DM_CHECK_HIP(hipMemcpyAsync(a->x_out, x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (launch_edm_finalize(x, a->out, n, s)) return 1;
    return run_finish(r);
}

// p_losses of both classes (+ forward's normalisation) and the backward pass: q_sample with the target, the tape forward
// with log_snr_b as the float time, the weighted loss with its gradient, the backward pass (an entry of run_train).
// ig (dm_unet_loss_backward_ct_ig): the same call, and behind it the gradient with respect to the U-Net's two inputs and
// the per-image sums a trained schedule needs; only then does the arena hold dX, dt and the (B, 4) rows.
struct CtInputGradOut {
    float* sched_out_host;
    float* dx_out;
    float* dtime_out;
};

static int loss_backward_ct_impl(dm_unet* u, const dm_ct_train_args& a, const CtInputGradOut* ig = nullptr) {
    DM_REQUIRE(a.images && a.noise && a.coef_host, "null argument");
    DM_REQUIRE(a.objective == DM_CT_PRED_NOISE || a.objective == DM_CT_PRED_V, "unknown continuous-time objective");
    DM_REQUIRE(u->train && u->train->ft, "dm_unet_train_enable_ft has not been called");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    const int cstride = a.coef_stride ? a.coef_stride : DM_CT_COEFS;
    DM_REQUIRE(a.B > 0 && cstride > CT_LOSS_W, "coef_host rows hold at least 10 floats (the loss weight is column 9)");
    if (ct_unet_ok(u)) return 1;
    const int B = a.B, H = a.H, W = a.W, accumulate = a.accumulate ? 1 : 0, objective = a.objective;
    if (check_hw(u, H, W)) return 1;
    hipStream_t s = static_cast<hipStream_t>(a.stream);
    TrainState& T = *u->train;
    const int64_t per = (int64_t)u->cfg.channels * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    float* sched = nullptr;  // (B, 4) rows [ga, gs, dt, l] in the handle's workspace
    auto run = [&](Arena& A, Tape& tp) -> int {
        const StepRows rows{T.coef_dev, nullptr, B > 1 ? STEP_ROW_IMAGE : STEP_ROW_FIRST, per};
        float* x = A.alloc(n);
        float* target = A.alloc(n);
        float* F = A.alloc(n);
        float* dF = A.alloc(n);
        float* part = A.alloc(B);
        InputGrad g{nullptr, nullptr};
        if (ig) {
            g.dx = A.alloc(n);
            g.dt = A.alloc(B);
            sched = A.alloc((size_t)B * 4);
        }
        if (!A.dry && launch_ct_noise_in(a.images, a.noise, rows, objective, a.normalize, x, target, n, s)) return 1;
        if (unet_train_forward(u, A, x, nullptr, F, B, H, W, s, tp, nullptr, 0, nullptr, T.tf_dev)) return 1;
        if (!A.dry && launch_ct_loss(F, target, T.coef_dev, dF, part, T.loss_dev, B, per, a.loss_scale, s)) return 1;
        if (unet_train_backward(u, A, x, dF, B, H, W, s, tp, accumulate, ig ? &g : nullptr)) return 1;
        if (!ig || A.dry) return 0;
        if (launch_ct_sched_reduce(g.dx, a.images, a.noise, F, target, g.dt, a.normalize, sched, B, per, s)) return 1;
        if (ig->dx_out) DM_CHECK_HIP(hipMemcpyAsync(ig->dx_out, g.dx, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (ig->dtime_out) DM_CHECK_HIP(hipMemcpyAsync(ig->dtime_out, g.dt, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    };
    TrainRun r;
    r.entry = TRAIN_CT;
    r.B = B; r.H = H; r.W = W; r.stream = a.stream; r.loss_out_host = a.loss_out_host;
    r.coef_host = a.coef_host; r.cstride = cstride; r.width = DM_CT_COEFS; r.tf_col = CT_LOG_SNR;
    r.sel[0] = ig ? 1 : 0;  // the two forms allocate differently
    if (run_train(u, r, run)) return 1;
    if (!ig || !ig->sched_out_host) return 0;
    // the workspace stays the handle's: the rows are read back behind the call's own kernels, then the stream is waited for
    DM_CHECK_HIP(hipMemcpyAsync(ig->sched_out_host, sched, (size_t)B * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
    DM_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // namespace dm

extern "C" {

int dm_sample_ct(dm_unet* u, const dm_ct_args* a) {
    DM_REQUIRE(u && a, "null argument");
    const CtLoop l{a->objective, a->clip, a->n_steps, a->table_host, a->x_init, a->noise, a->seed, a->sample_offset, a->out,
                   nullptr, a->B, a->H, a->W, a->use_graph, a->stream, false};
    return sample_ct_impl(u, &l);
}

int dm_sample_ct_dpmpp(dm_unet* u, const dm_ct_dpmpp_args* a) {
    DM_REQUIRE(u && a, "null argument");
    const CtLoop l{a->objective, a->clip, a->n_steps, a->table_host, a->x_init, nullptr, 0, 0, a->out,
                   a->x_out, a->B, a->H, a->W, a->use_graph, a->stream, true};
    return sample_ct_impl(u, &l);
}

int dm_unet_loss_backward_ct(dm_unet* u, const dm_ct_train_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return loss_backward_ct_impl(u, *a);
}

int dm_unet_loss_backward_ct_ig(dm_unet* u, const dm_ct_train_ig_args* a) {
    DM_REQUIRE(u && a, "null argument");
    const dm_ct_train_args base{a->images, a->noise, a->coef_host, a->coef_stride, a->objective, a->loss_scale, a->accumulate,
                                a->B, a->H, a->W, a->normalize, a->loss_out_host, a->stream};
    const CtInputGradOut ig{a->sched_out_host, a->dx_out, a->dtime_out};
    return loss_backward_ct_impl(u, base, &ig);
}

int dm_op_ct_sched_reduce(const float* dx, const float* images, const float* eps, const float* F, const float* target,
                          const float* dt, int normalize, float* out, int B, int64_t per, void* stream) {
    DM_REQUIRE(dx && images && eps && F && target && out, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_ct_sched_reduce(dx, images, eps, F, target, dt, normalize, out, B, per, s)) return 1;
    DM_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int dm_op_sinusoid_ft_tgrad(const float* de0, const float* e0, const float* freqs, float* dt, int B, int half, void* stream) {
    DM_REQUIRE(de0 && e0 && freqs && dt && B > 0 && half > 0, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_sinusoid_ft_tgrad(de0, e0, freqs, dt, B, half, s)) return 1;
    DM_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int dm_op_conv7_dgrad(const float* dy_nchw, const float* weight, float* dx, int B, int H, int W, int Cout, int C, void* stream) {
    DM_REQUIRE(dy_nchw && weight && dx, "null argument");
    DM_REQUIRE(B > 0 && H > 0 && W > 0 && Cout > 0 && C >= 1 && C <= 8, "conv7_dgrad: 1..8 input channels");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_op(s, [&](Arena& A) -> int {
        int e = 0;
        float* g = to_nhwc(A, dy_nchw, B, Cout, H * W, s, &e);
        if (e) return 1;
        return A.dry ? 0 : launch_conv7_dgrad(g, weight, dx, B, H, W, Cout, C, s);
    });
}

int dm_op_ct_step(const float* x, const float* F, const float* eps, const float* c_host, int rows, int objective, int clip,
                  uint64_t seed, uint64_t draw, uint64_t element_offset, float* out, float* x_start_out, int B, int64_t per,
                  void* stream) {
    DM_REQUIRE(x && F && out, "null argument");
    DM_REQUIRE(element_offset % 4 == 0, "Philox element offset must be a multiple of 4 (one counter serves 4 elements)");
    DM_REQUIRE(eps || draw >= 1, "Philox draw 0 is the initial noise: a step's draw is its index + 1");
    return state_op(draw_state(eps != nullptr, seed, draw, element_offset), c_host, rows, stream,
                    [&](const SamplerState* st, const float* cd, hipStream_t s) {
                        StepRows r;
                        if (edm_rows(cd, rows, B, per, &r)) return 1;
                        r.st = st;
                        return launch_ct_step(x, F, eps, 0, r, objective, clip ? 1 : 0, out, x_start_out, (int64_t)B * per, s);
                    });
}

int dm_op_ct_dpmpp_step(const float* x, const float* F, float* hist, const float* c_host, int rows, int objective, int clip,
                        float* out, int B, int64_t per, void* stream) {
    DM_REQUIRE(x && F && hist && out, "null argument");
    return table_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        StepRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_ct_dpmpp_step(x, F, hist, r, objective, clip ? 1 : 0, out, (int64_t)B * per, s);
    });
}

int dm_op_ct_noise_in(const float* images, const float* eps, const float* c_host, int rows, int objective, int normalize,
                      float* x, float* target, int B, int64_t per, void* stream) {
    DM_REQUIRE(images && eps && x && target, "null argument");
    return table_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        StepRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_ct_noise_in(images, eps, r, objective, normalize, x, target, (int64_t)B * per, s);
    });
}

int dm_op_ct_loss(const float* F, const float* target, const float* c_host, float loss_scale, float* dF, float* loss_out_host,
                  int B, int64_t per, void* stream) {
    DM_REQUIRE(F && target && dF && loss_out_host && B > 0, "null argument");
    // scratch: [B] per-image partials, then the loss
    return table_op(c_host, B, stream, [&](float* cd, hipStream_t s) {
        float* part = cd + (size_t)B * DM_CT_COEFS;
        return launch_ct_loss(F, target, cd, dF, part, part + B, B, per, loss_scale, s);
    }, DM_CT_COEFS, (size_t)B + 1, {{loss_out_host, (size_t)B, 1}});
}

}  // extern "C"
