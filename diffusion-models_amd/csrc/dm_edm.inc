// ElucidatedDiffusion on the C ABI: the float-time forward, the two sampling loops, the EDM loss + backward (an entry of
// run_train, dm_train.inc) and the single-pass entry points (dm_op_edm_*).  Included by dm_api.hip after dm_sampler.inc,
// whose loop scaffolding it runs on; kernels in edm.hip.

namespace dm {

static int edm_handle_ok(dm_unet* u, bool karras_ok = false) {
    if (handle_ready(u, karras_ok)) return 1;
    DM_REQUIRE(u->cfg.learned_sinusoidal_dim > 0,
               "a real-valued time needs a learned / random sinusoidal U-Net (ElucidatedDiffusion asserts it)");
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
    if (edm_handle_ok(u, /*karras_ok=*/true)) return 1;
    if (plain_unet_ok(u,
                      "ElucidatedDiffusion needs a U-Net with out_dim == input channels == channels (no self-conditioning, no image "
                      "condition, no learned variance)",
                      "ElucidatedDiffusion calls net(x, t, self_cond) only: no text-conditional U-Net"))
        return 1;
    const int B = a->B, H = a->H, W = a->W, n_steps = a->n_steps, clamp = a->clamp ? 1 : 0;
    const bool heun = a->kind == DM_EDM_HEUN;
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    const int C = u->cfg.channels;
    const int64_t per = (int64_t)C * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    const float* noise = a->noise;
    const float* tab_host = a->table_host;

    SamplerRun r;
    if (grow_tables(u, TAB_FLOAT, n_steps, 1) || run_begin(r, u, a->stream, a->use_graph)) return 1;
    hipStream_t s = r.s;
    // workspace: Heun [x | xhat | xin | F | d | forward arena], DPM++ [x | xin | F | d_old | forward arena]
    float *x, *xhat, *xin, *F, *d;
    auto layout = [&](Arena& A) {
        x = A.alloc(n);
        xhat = heun ? A.alloc(n) : nullptr;
        xin = A.alloc(n);
        F = A.alloc(n);
        d = A.alloc(n);  // Heun: d of the Euler step; DPM++: the previous step's denoised image
    };
    const float* tf_marker = reinterpret_cast<const float*>(16);
    if (run_workspace(r, layout, [&](Arena& dry) {
            return unet_forward_impl(u, dry, nullptr, nullptr, nullptr, u->state_dev, nullptr, 0, nullptr, B, H, W, s, nullptr,
                                     tf_marker, DM_EDM_COEFS);
        }))
        return 1;
    if (run_upload(r, n_steps, nullptr, nullptr, tab_host, 0, a->seed, a->sample_offset * (uint64_t)per)) return 1;
    const float* tab = u->edm_tab_dev;
    const StepRows rows{tab, u->state_dev, STEP_ROW_STEP, per};

    if (launch_edm_scale(a->x_init, a->sigma_init, x, n, s)) return 1;  // images = sigmas[0] * randn (:151, :201)
    if (!heun) DM_CHECK_HIP(hipMemsetAsync(d, 0, n * sizeof(float), s));

    auto forward = [&](hipStream_t st, int col) -> int {
        r.rewind();
        return unet_forward_impl(u, r.A, xin, nullptr, nullptr, u->state_dev, nullptr, 0, F, B, H, W, st, nullptr, tab + col,
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
    dm_unet::GraphKey key;
    key.kind = heun ? dm_unet::GK_EDM_HEUN : dm_unet::GK_EDM_DPMPP;
    key.B = B; key.H = H; key.W = W;
    key.edm_clamp = clamp;
    key.noise = noise; key.ws = u->ws; key.tab = u->edm_tab_dev;
    if (heun) {
        if (run_steps(r, key, n_steps, [&](hipStream_t st) { return heun_step(st, true); },
                      [&](hipStream_t st) { return heun_step(st, false); },
                      [&](int i) { return tab_host[(size_t)i * DM_EDM_COEFS + EDM_SIGMA2] != 0.0f; }))
            return 1;
    } else if (run_steps(r, key, n_steps, dpmpp_step)) {
        return 1;
    }
    if (launch_edm_finalize(x, a->out, n, s)) return 1;
    return run_finish(r);
}

static const char* const kEdmTrainUnet =
    "ElucidatedDiffusion needs a U-Net with out_dim == input channels == channels and no text conditioning";

// ElucidatedDiffusion.forward (DD/elucidated_diffusion.py:234-264) + backward: the noise-in pass, the tape forward with
// c_noise(sigma) as the float time, the weighted loss with its gradient, the backward pass.
static int loss_backward_edm_impl(dm_unet* u, const dm_edm_train_args& a) {
    DM_REQUIRE(a.images && a.noise && a.coef_host, "null argument");
    DM_REQUIRE(u->train && u->train->ft, "dm_unet_train_enable_ft has not been called");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    const int cstride = a.coef_stride ? a.coef_stride : DM_EDM_COEFS;
    DM_REQUIRE(a.B > 0 && cstride > EDM_LOSS_W, "coef_host rows hold at least 15 floats (loss_weight is column 14)");
    if (plain_unet_ok(u, kEdmTrainUnet)) return 1;
    const int B = a.B, H = a.H, W = a.W, accumulate = a.accumulate ? 1 : 0;
    if (check_hw(u, H, W)) return 1;
    hipStream_t s = static_cast<hipStream_t>(a.stream);
    TrainState& T = *u->train;
    const int64_t per = (int64_t)u->cfg.channels * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    auto run = [&](Arena& A, Tape& tp) -> int {
        const StepRows rows{T.coef_dev, nullptr, B > 1 ? STEP_ROW_IMAGE : STEP_ROW_FIRST, per};
        float* x0 = A.alloc(n);
        float* noised = A.alloc(n);
        float* xin = A.alloc(n);
        float* F = A.alloc(n);
        float* dF = A.alloc(n);
        float* part = A.alloc(B);
        if (!A.dry && launch_edm_noise_in(a.images, a.noise, rows, x0, noised, xin, n, s)) return 1;
        if (unet_train_forward(u, A, xin, nullptr, F, B, H, W, s, tp, nullptr, 0, nullptr, T.tf_dev)) return 1;
        if (!A.dry && launch_edm_loss(noised, F, x0, T.coef_dev, dF, a.denoised_out, part, T.loss_dev, B, per, a.loss_scale, s))
            return 1;
        return unet_train_backward(u, A, xin, dF, B, H, W, s, tp, accumulate);
    };
    TrainRun r;
    r.entry = TRAIN_EDM;
    r.sel = {a.denoised_out ? 1 : 0};
    r.B = B; r.H = H; r.W = W; r.stream = a.stream; r.loss_out_host = a.loss_out_host;
    r.coef_host = a.coef_host; r.cstride = cstride; r.width = DM_EDM_COEFS; r.tf_col = EDM_C_NOISE;
    return run_train(u, r, run);
}

}  // namespace dm

extern "C" {

int dm_unet_forward_ft(dm_unet* u, const float* x, const float* time, const float* ctx, int ctx_tokens, float* out, int B,
                       int H, int W, void* stream) {
    DM_REQUIRE(u && x && time && out, "null argument");
    if (edm_handle_ok(u, /*karras_ok=*/true)) return 1;
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
    return state_op(draw_state(eps != nullptr, seed, draw, element_offset), c_host, rows, stream,
                    [&](const SamplerState* st, const float* cd, hipStream_t s) {
                        StepRows r;
                        if (edm_rows(cd, rows, B, per, &r)) return 1;
                        r.st = st;
                        return launch_edm_churn_in(x, eps, 0, r, xhat, xin, (int64_t)B * per, s);
                    });
}

int dm_op_edm_euler(const float* xhat, const float* F, const float* c_host, int rows, int clamp, float* D_out, float* d_out,
                    float* xnext, float* xin_next, int B, int64_t per, void* stream) {
    DM_REQUIRE(xhat && F, "null argument");
    return table_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        StepRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_edm_euler(xhat, F, r, clamp ? 1 : 0, D_out, d_out, xnext, xin_next, (int64_t)B * per, s);
    });
}

int dm_op_edm_heun(const float* xhat, const float* d, const float* xnext, const float* F2, const float* c_host, int rows,
                   int clamp, float* out, int B, int64_t per, void* stream) {
    DM_REQUIRE(xhat && d && xnext && F2 && out, "null argument");
    return table_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        StepRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_edm_heun(xhat, d, xnext, F2, r, clamp ? 1 : 0, out, (int64_t)B * per, s);
    });
}

int dm_op_edm_dpmpp(const float* x, const float* F, float* d_old, const float* c_host, int rows, float* out, int B,
                    int64_t per, void* stream) {
    DM_REQUIRE(x && F && d_old && out, "null argument");
    return table_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        StepRows r;
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
    if (plain_unet_ok(u, kEdmTrainUnet)) return 1;
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
    return table_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) {
        StepRows r;
        if (edm_rows(cd, rows, B, per, &r)) return 1;
        return launch_edm_noise_in(images, eps, r, x0, noised, xin, (int64_t)B * per, s);
    });
}

int dm_op_edm_loss(const float* noised, const float* F, const float* x0, const float* c_host, float loss_scale, float* dF,
                   float* D_out, float* loss_out_host, int B, int64_t per, void* stream) {
    DM_REQUIRE(noised && F && x0 && dF && loss_out_host && B > 0, "null argument");
    // scratch: [B] per-image partials, then the loss
    return table_op(c_host, B, stream, [&](float* cd, hipStream_t s) {
        float* part = cd + (size_t)B * DM_EDM_COEFS;
        return launch_edm_loss(noised, F, x0, cd, dF, D_out, part, part + B, B, per, loss_scale, s);
    }, DM_EDM_COEFS, (size_t)B + 1, {{loss_out_host, (size_t)B, 1}});
}

int dm_op_sinusoid_ft_bwd(const float* de0, const float* e0, float* dw, int B, int half, int learned, int accumulate,
                          void* stream) {
    DM_REQUIRE(de0 && e0 && dw && B > 0 && half > 0, "bad argument");
    return launch_sinusoid_ft_bwd(de0, e0, dw, B, half, learned != 0, accumulate, static_cast<hipStream_t>(stream));
}

}  // extern "C"
