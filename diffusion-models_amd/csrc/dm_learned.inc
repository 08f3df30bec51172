// LearnedGaussianDiffusion on the C ABI: the sampling loop, the hybrid loss + backward and the single-pass entry points
// (dm_op_lv_*).  Included by dm_api.hip after dm_train.inc (the tape forward / backward), dm_sampler.inc (the loop
// scaffolding); kernels in learned.hip.

namespace dm {

static_assert(DM_LV_COEFS == LV_NCOLS && DM_LV_COEFS == DM_EDM_COEFS,
              "the learned-variance step table lives in the handle's EDM table buffer: the row widths must agree");
static_assert(DM_LV_TRAIN_COEFS == LVT_NCOLS && DM_LV_TRAIN_COEFS == DM_TRAIN_COEFS,
              "q_sample_kernel reads columns 0, 1 of the learned-variance training rows at its own row width");

static int lv_unet_ok(dm_unet* u) {
    DM_REQUIRE(u->cfg.text_mode == DM_TEXT_NONE, "LearnedGaussianDiffusion calls model(x, t) only: no text-conditional U-Net");
    DM_REQUIRE(u->cfg.learned_sinusoidal_dim == 0, "LearnedGaussianDiffusion calls model(x, t) with an integer time");
    DM_REQUIRE(u->out_dim == 2 * u->cfg.channels && u->cfg.input_channels == u->cfg.channels,
               "LearnedGaussianDiffusion needs a U-Net with out_dim == 2 * channels == 2 * input channels "
               "(DD/learned_gaussian_diffusion.py:70-71: learned_variance=True, no self-conditioning)");
    return 0;
}

// p_sample_loop of the base class (DD/denoising_diffusion.py:647-664) with the subclass's p_mean_variance.  One step -- the
// forward into the 2n buffer, lv_step_kernel, the step counter -- is one linear chain that reads everything that differs
// between two calls of one shape (tables, step counter and count, seed, Philox offset, unnormalise) as device data: it is
// captured once per shape.
static int sample_lv_impl(dm_unet* u, const dm_lv_args* a) {
    DM_REQUIRE(a->times_host && a->table_host && a->x_T && a->out, "null argument");
    DM_REQUIRE(a->n_steps > 0 && a->B > 0, "empty run");
    if (handle_ready(u)) return 1;
    if (lv_unet_ok(u)) return 1;
    const int B = a->B, H = a->H, W = a->W, n_steps = a->n_steps;
    if (check_hw(u, H, W)) return 1;
    const int64_t per = (int64_t)u->cfg.channels * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    const float* noise = a->noise;
    float* all_steps = a->all_steps;

    // workspace: [x | result | model output (2n) | forward arena]
    TableLoop L;
    float* eps2;
    if (table_loop_begin(L, u, *a, n_steps, 1, a->sample_offset * (uint64_t)per, [&](Arena& A) { eps2 = A.alloc(2 * n); }))
        return 1;
    auto step = [&](hipStream_t st) -> int {
        L.r.rewind();
        if (unet_forward_impl(u, L.r.A, L.xbuf, nullptr, u->times_dev, u->state_dev, nullptr, 0, eps2, B, H, W, st)) return 1;
        if (launch_lv_step(L.xbuf, eps2, noise, n, L.tab, u->state_dev, STEP_ROW_STEP, per, L.xbuf, all_steps, L.fin, nullptr, nullptr,
                           nullptr, n, st))
            return 1;
        return launch_step_advance(u->state_dev, st);
    };
    L.key.kind = dm_unet::GK_LV;
    if (run_steps(L.r, L.key, n_steps, step)) return 1;
    return table_loop_end(L, a->out);
}

// p_losses (DD/learned_gaussian_diffusion.py:113-146) and the backward pass, an entry of run_train: q_sample, the tape
// forward into a 2n buffer, the loss with its gradient, the backward pass.
static int loss_backward_lv_impl(dm_unet* u, const dm_lv_train_args& a) {
    DM_REQUIRE(a.x_start && a.t_host && a.coef_host && a.noise, "null argument");
    DM_REQUIRE(u->train, "dm_unet_train_enable has not been called");
    DM_REQUIRE(!u->train->ft, "the handle is armed for float-time training (dm_unet_train_enable_ft)");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    const int cstride = a.coef_stride ? a.coef_stride : DM_LV_TRAIN_COEFS;
    DM_REQUIRE(a.B > 0 && cstride > LVT_T0 && cstride <= DM_LV_TRAIN_COEFS, "coef_host rows hold 10 to 12 floats (the t == 0 flag is column 9)");
    if (lv_unet_ok(u)) return 1;
    const int B = a.B, H = a.H, W = a.W, accumulate = a.accumulate ? 1 : 0;
    if (check_hw(u, H, W)) return 1;
    hipStream_t s = static_cast<hipStream_t>(a.stream);
    TrainState& T = *u->train;
    const int64_t per = (int64_t)u->cfg.channels * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0 && per < (int64_t(1) << 30), "C * H * W must be a multiple of 4");
    auto run = [&](Arena& A, Tape& tp) -> int {
        float* x = A.alloc(n);
        float* out = A.alloc(2 * n);
        float* dout = A.alloc(2 * n);
        float* part = A.alloc(3 * (size_t)B);  // [loss | mse | vb] per image
        if (!A.dry && launch_q_sample(a.x_start, a.noise, T.coef_dev, x, B, (int)per, s)) return 1;
        if (unet_train_forward(u, A, x, T.t_dev, out, B, H, W, s, tp, nullptr, 0, nullptr)) return 1;
        if (!A.dry) {
            if (launch_lv_loss(out, a.x_start, a.noise, x, T.coef_dev, a.vb_loss_weight, a.clip_denoised, dout, part, part + B,
                               part + 2 * B, T.loss_dev, B, per, a.loss_scale, s))
                return 1;
            if (a.model_out) DM_CHECK_HIP(hipMemcpyAsync(a.model_out, out, 2 * n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        return unet_train_backward(u, A, x, dout, B, H, W, s, tp, accumulate);
    };
    TrainRun r;
    r.entry = TRAIN_LV;
    r.sel = {a.model_out ? 1 : 0};
    r.B = B; r.H = H; r.W = W; r.stream = a.stream; r.loss_out_host = a.loss_out_host;
    r.coef_host = a.coef_host; r.cstride = cstride; r.width = DM_LV_TRAIN_COEFS;
    r.t_host = a.t_host;
    return run_train(u, r, run);
}

}  // namespace dm

extern "C" {

int dm_sample_lv(dm_unet* u, const dm_lv_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return sample_lv_impl(u, a);
}

int dm_unet_loss_backward_lv(dm_unet* u, const dm_lv_train_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return loss_backward_lv_impl(u, *a);
}

int dm_op_lv_step(const float* x, const float* model_out, const float* z, const float* c_host, uint64_t seed, uint64_t draw,
                  uint64_t element_offset, float* out, float* mean_out, float* logvar_out, float* x_start_out, int B,
                  int64_t per, void* stream) {
    DM_REQUIRE(x && model_out && c_host && out, "null argument");
    DM_REQUIRE(B > 0 && per > 0, "empty tensor");
    if (draw_args_ok(z, draw, element_offset)) return 1;
    return state_op(draw_state(z != nullptr, seed, draw, element_offset), c_host, 1, stream,
                    [&](const SamplerState* st, const float* cd, hipStream_t s) {
                        return launch_lv_step(x, model_out, z, 0, cd, st, STEP_ROW_FIRST, per, out, nullptr, nullptr, mean_out,
                                              logvar_out, x_start_out, (int64_t)B * per, s);
                    });
}

int dm_op_lv_loss(const float* model_out, const float* x_start, const float* noise, const float* x_t, const float* c_host,
                  float vb_loss_weight, int clip_denoised, float loss_scale, float* dout, float* loss_out_host,
                  float* mse_part_out_host, float* vb_part_out_host, int B, int64_t per, void* stream) {
    DM_REQUIRE(model_out && x_start && noise && x_t && c_host && dout && loss_out_host && B > 0, "null argument");
    // scratch: [3 B per-image parts: loss | mse | vb] [the loss]
    const size_t nb = (size_t)B;
    return table_op(c_host, B, stream, [&](float* cd, hipStream_t s) {
        float* part = cd + nb * LVT_NCOLS;
        return launch_lv_loss(model_out, x_start, noise, x_t, cd, vb_loss_weight, clip_denoised, dout, part, part + B,
                              part + 2 * B, part + 3 * nb, B, per, loss_scale, s);
    }, LVT_NCOLS, 3 * nb + 1, {{loss_out_host, 3 * nb, 1}, {mse_part_out_host, nb, nb}, {vb_part_out_host, 2 * nb, nb}});
}

}  // extern "C"
