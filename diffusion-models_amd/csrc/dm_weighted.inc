// WeightedObjectiveGaussianDiffusion on the C ABI: the sampling loop, the three-term loss + backward and the single-pass
// entry points (dm_op_wo_*).  Included by dm_api.hip after dm_train.inc (the tape forward / backward), dm_sampler.inc (the
// loop scaffolding); kernels in weighted.hip.

namespace dm {

static_assert(DM_WO_COEFS == WO_NCOLS && DM_WO_COEFS == DM_EDM_COEFS,
              "the weighted-objective step table lives in the handle's EDM table buffer: the row widths must agree");
static_assert(DM_WO_TRAIN_COEFS == WOT_NCOLS && DM_WO_TRAIN_COEFS == DM_TRAIN_COEFS,
              "q_sample_kernel reads columns 0, 1 of the weighted-objective training rows at its own row width");

static int wo_unet_ok(dm_unet* u) {
    DM_REQUIRE(u->cfg.text_mode == DM_TEXT_NONE, "WeightedObjectiveGaussianDiffusion calls model(x, t) only: no text-conditional U-Net");
    DM_REQUIRE(u->cfg.learned_sinusoidal_dim == 0, "WeightedObjectiveGaussianDiffusion calls model(x, t) with an integer time");
    DM_REQUIRE(u->out_dim == 2 * u->cfg.channels + 2 && u->cfg.input_channels == u->cfg.channels,
               "WeightedObjectiveGaussianDiffusion needs a U-Net with out_dim == 2 * channels + 2 and input channels == channels "
               "(DD/weighted_objective_gaussian_diffusion.py:25-26: noise, x_start and two weight maps; no self-conditioning)");
    DM_REQUIRE(u->out_dim <= 8, "WeightedObjectiveGaussianDiffusion: out_dim == 2 * channels + 2 must be at most 8 (channels <= 3): "
                                "the thin-output final_conv kernels stop at 8 outputs");
    return 0;
}

// p_sample_loop of the base class (DD/denoising_diffusion.py:647-664) over the subclass's p_mean_variance.  One step -- the
// forward into the (2C + 2) / C * n buffer, wo_step_kernel, the step counter -- is one linear chain that reads everything
// that differs between two calls of one shape (tables, step counter and count, seed, Philox offset, unnormalise) as device
// data: it is captured once per shape.
static int sample_wo_impl(dm_unet* u, const dm_wo_args* a) {
    DM_REQUIRE(a->times_host && a->table_host && a->x_T && a->out, "null argument");
    DM_REQUIRE(a->n_steps > 0 && a->B > 0, "empty run");
    if (handle_ready(u)) return 1;
    if (wo_unet_ok(u)) return 1;
    const int B = a->B, H = a->H, W = a->W, n_steps = a->n_steps;
    if (check_hw(u, H, W)) return 1;
    const int C = u->cfg.channels;
    const int64_t HW = (int64_t)H * W, per = C * HW, n = (int64_t)B * per, n_out = (int64_t)B * u->out_dim * HW;
    DM_REQUIRE(HW % 4 == 0, "H * W must be a multiple of 4");
    const float* noise = a->noise;
    float* all_steps = a->all_steps;

    // workspace: [x | result | model output ((2C + 2) / C * n) | forward arena]
    TableLoop L;
    float* mo;
    if (table_loop_begin(L, u, *a, n_steps, 1, a->sample_offset * (uint64_t)per, [&](Arena& A) { mo = A.alloc(n_out); }))
        return 1;
    auto step = [&](hipStream_t st) -> int {
        L.r.rewind();
        if (unet_forward_impl(u, L.r.A, L.xbuf, nullptr, u->times_dev, u->state_dev, nullptr, 0, mo, B, H, W, st)) return 1;
        if (launch_wo_step(L.xbuf, mo, noise, n, L.tab, u->state_dev, STEP_ROW_STEP, B, C, HW, 1, L.xbuf, all_steps, L.fin, nullptr,
                           nullptr, st))
            return 1;
        return launch_step_advance(u->state_dev, st);
    };
    L.key.kind = dm_unet::GK_WO;
    if (run_steps(L.r, L.key, n_steps, step)) return 1;
    return table_loop_end(L, a->out);
}

// p_losses (DD/weighted_objective_gaussian_diffusion.py:51-74) and the backward pass, an entry of run_train: q_sample, the
// tape forward into a (B, 2C + 2, H, W) buffer, the loss with its gradient, the backward pass.
static int loss_backward_wo_impl(dm_unet* u, const dm_wo_train_args& a) {
    DM_REQUIRE(a.x_start && a.t_host && a.coef_host && a.noise, "null argument");
    DM_REQUIRE(u->train, "dm_unet_train_enable has not been called");
    DM_REQUIRE(!u->train->ft, "the handle is armed for float-time training (dm_unet_train_enable_ft)");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    const int cstride = a.coef_stride ? a.coef_stride : DM_WO_TRAIN_COEFS;
    DM_REQUIRE(a.B > 0 && cstride > WOT_RECIPM1 && cstride <= DM_WO_TRAIN_COEFS, "coef_host rows hold 4 to 12 floats");
    if (wo_unet_ok(u)) return 1;
    const int B = a.B, H = a.H, W = a.W, accumulate = a.accumulate ? 1 : 0;
    if (check_hw(u, H, W)) return 1;
    hipStream_t s = static_cast<hipStream_t>(a.stream);
    TrainState& T = *u->train;
    const int C = u->cfg.channels;
    const int64_t HW = (int64_t)H * W, per = C * HW, n = (int64_t)B * per, n_out = (int64_t)B * u->out_dim * HW;
    DM_REQUIRE(HW % 4 == 0 && (int64_t)u->out_dim * HW < (int64_t(1) << 30), "H * W must be a multiple of 4");
    auto run = [&](Arena& A, Tape& tp) -> int {
        float* x = A.alloc(n);
        float* out = A.alloc(n_out);
        float* dout = A.alloc(n_out);
        float* part = A.alloc(4 * (size_t)B);  // [loss | weighted | x_start | noise] per image
        if (!A.dry && launch_q_sample(a.x_start, a.noise, T.coef_dev, x, B, (int)per, s)) return 1;
        if (unet_train_forward(u, A, x, T.t_dev, out, B, H, W, s, tp, nullptr, 0, nullptr)) return 1;
        if (!A.dry) {
            if (launch_wo_loss(out, a.x_start, a.noise, x, T.coef_dev, a.pred_noise_loss_weight, a.pred_x_start_loss_weight, dout,
                               part, part + B, part + 2 * B, part + 3 * B, T.loss_dev, B, C, HW, a.loss_scale, s))
                return 1;
            if (a.model_out) DM_CHECK_HIP(hipMemcpyAsync(a.model_out, out, n_out * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        return unet_train_backward(u, A, x, dout, B, H, W, s, tp, accumulate);
    };
    TrainRun r;
    r.entry = TRAIN_WO;
    r.sel = {a.model_out ? 1 : 0};
    r.B = B; r.H = H; r.W = W; r.stream = a.stream; r.loss_out_host = a.loss_out_host;
    r.coef_host = a.coef_host; r.cstride = cstride; r.width = DM_WO_TRAIN_COEFS;
    r.t_host = a.t_host;
    return run_train(u, r, run);
}

}  // namespace dm

extern "C" {

int dm_sample_wo(dm_unet* u, const dm_wo_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return sample_wo_impl(u, a);
}

int dm_unet_loss_backward_wo(dm_unet* u, const dm_wo_train_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return loss_backward_wo_impl(u, *a);
}

int dm_op_wo_step(const float* x, const float* model_out, const float* z, const float* c_host, int clip_denoised, uint64_t seed,
                  uint64_t draw, uint64_t element_offset, float* out, float* mean_out, float* x_start_out, int B, int C,
                  int64_t HW, void* stream) {
    DM_REQUIRE(x && model_out && c_host && out, "null argument");
    DM_REQUIRE(B > 0 && C > 0 && HW > 0, "empty tensor");
    if (draw_args_ok(z, draw, element_offset)) return 1;
    return state_op(draw_state(z != nullptr, seed, draw, element_offset), c_host, 1, stream,
                    [&](const SamplerState* st, const float* cd, hipStream_t s) {
                        return launch_wo_step(x, model_out, z, 0, cd, st, STEP_ROW_FIRST, B, C, HW, clip_denoised, out, nullptr,
                                              nullptr, mean_out, x_start_out, s);
                    });
}

int dm_op_wo_loss(const float* model_out, const float* x_start, const float* noise, const float* x_t, const float* c_host,
                  float pred_noise_loss_weight, float pred_x_start_loss_weight, float loss_scale, float* dout,
                  float* loss_out_host, float* weighted_part_out_host, float* x_start_part_out_host,
                  float* noise_part_out_host, int B, int C, int64_t HW, void* stream) {
    DM_REQUIRE(model_out && x_start && noise && x_t && c_host && dout && loss_out_host && B > 0, "null argument");
    // scratch: [4 B per-image parts: loss | weighted | x_start | noise] [the loss]
    const size_t nb = (size_t)B;
    return table_op(c_host, B, stream, [&](float* cd, hipStream_t s) {
        float* part = cd + nb * WOT_NCOLS;
        return launch_wo_loss(model_out, x_start, noise, x_t, cd, pred_noise_loss_weight, pred_x_start_loss_weight, dout, part,
                              part + B, part + 2 * B, part + 3 * B, part + 4 * nb, B, C, HW, loss_scale, s);
    }, WOT_NCOLS, 4 * nb + 1, {{loss_out_host, 4 * nb, 1}, {weighted_part_out_host, nb, nb},
                               {x_start_part_out_host, 2 * nb, nb}, {noise_part_out_host, 3 * nb, nb}});
}

}  // extern "C"
