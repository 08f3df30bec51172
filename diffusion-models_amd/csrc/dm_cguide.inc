// Classifier-guided DDPM sampling on the C ABI: the loop whose step leaves the GPU for the caller's cond_fn, and the
// single-pass entry points (dm_op_cg_*).  Included by dm_api.hip after dm_sampler.inc (the loop scaffolding) and
// dm_edm.inc (the state helper of the dm_op_* passes); kernels in cguide.hip.

namespace dm {

static_assert(DM_CG_COEFS == CG_NCOLS && DM_CG_COEFS == DM_EDM_COEFS,
              "the classifier-guidance step table lives in the handle's EDM table buffer: the row widths must agree");

// p_sample_loop of DD/guided_diffusion.py:586-603 with cond_fn and guidance_kwargs given.  A step is two linear chains
// with the host in between:
//   front  self-conditioning copies, U-Net forward, cg_mean_kernel -> a->mean (and the x_start of the next step's input)
//   host   hipStreamSynchronize(run's stream); cond_cb(user, i, t_i): the caller reads a->mean, writes a->grad and returns
//          only when a->grad is complete (its own stream is synchronised)
//   back   cg_finish_kernel (a->mean, a->grad -> x), the step counter
// Each half touches handle-owned memory and the caller's mean / grad only, and reads everything that differs between two
// calls of one shape (tables, step counter and count, seed, Philox offset, unnormalise) as device data: the halves are
// captured once each, into the handle's two graph slots.
static int sample_cg_impl(dm_unet* u, const dm_cguide_args* a) {
    DM_REQUIRE(a->times_host && a->table_host && a->x_T && a->out, "null argument");
    DM_REQUIRE(a->mean && a->grad && a->cond_cb, "classifier guidance needs the mean and grad tensors and the callback");
    DM_REQUIRE(a->mean != a->grad, "mean and grad are two tensors");
    DM_REQUIRE(a->n_steps > 0 && a->B > 0, "empty run");
    DM_REQUIRE(a->objective >= DM_OBJ_PRED_NOISE && a->objective <= DM_OBJ_PRED_V, "unknown objective");
    if (handle_ready(u)) return 1;
    const int self_cond = a->self_condition ? 1 : 0;
    DM_REQUIRE(u->cfg.text_mode == DM_TEXT_NONE,
               "classifier guidance calls model(x, t, x_self_cond) only: no text-conditional U-Net");
    DM_REQUIRE(u->cfg.learned_sinusoidal_dim == 0, "classifier guidance calls the model with an integer time");
    DM_REQUIRE(u->out_dim == u->cfg.channels, "classifier guidance needs out_dim == channels (DD/guided_diffusion.py:397)");
    DM_REQUIRE(u->cfg.input_channels == u->cfg.channels * (self_cond ? 2 : 1),
               "classifier guidance takes no image condition: U-Net input channels != channels [* 2 with self-conditioning]");
    const int B = a->B, H = a->H, W = a->W, n_steps = a->n_steps, objective = a->objective;
    if (check_hw(u, H, W)) return 1;
    const int C = u->cfg.channels;
    const int64_t per = (int64_t)C * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    const float* noise = a->noise;
    float* all_steps = a->all_steps;
    float *mean = a->mean, *grad = a->grad;

    // workspace: [x | result | model output | [x_start | x] | x_start | forward arena]
    TableLoop L;
    float *eps, *xin, *xstart;
    auto layout = [&](Arena& A) {
        eps = A.alloc(n);
        xin = self_cond ? A.alloc(2 * n) : nullptr;  // [x_start | x] per image, what init_conv reads
        xstart = self_cond ? A.alloc(n) : nullptr;   // the unguided clamped x_0 estimate of the previous step
    };
    if (table_loop_begin(L, u, *a, n_steps, 1, a->sample_offset * (uint64_t)per, layout)) return 1;
    hipStream_t s = L.s;
    float* const xbuf = L.xbuf;
    if (self_cond) DM_CHECK_HIP(hipMemsetAsync(xstart, 0, n * sizeof(float), s));  // x_self_cond = None reads as zeros

    auto front = [&](hipStream_t st) -> int {
        L.r.rewind();
        if (self_cond && (launch_copy_channels(xstart, xin, B, C, 2 * C, 0, H * W, st) ||
                          launch_copy_channels(xbuf, xin, B, C, 2 * C, C, H * W, st)))
            return 1;
        if (unet_forward_impl(u, L.r.A, self_cond ? xin : xbuf, nullptr, u->times_dev, u->state_dev, nullptr, 0, eps, B, H, W, st))
            return 1;
        return launch_cg_mean(xbuf, eps, L.tab, u->state_dev, STEP_ROW_STEP, per, objective, mean, xstart, n, st);
    };
    auto host = [&](int i) -> int {
        DM_CHECK_HIP(hipStreamSynchronize(s));  // the mean is complete before cond_fn reads it
        const int rc = a->cond_cb(a->user, i, a->times_host[i]);
        DM_REQUIRE(rc == 0, "dm_sample_classifier_guided: cond_cb returned " + std::to_string(rc) + " at step " +
                                std::to_string(i) + " (t = " + std::to_string((long long)a->times_host[i]) +
                                "): the loop ends here");
        return 0;
    };
    auto back = [&](hipStream_t st) -> int {
        if (launch_cg_finish(mean, grad, noise, n, L.tab, u->state_dev, STEP_ROW_STEP, per, xbuf, all_steps, L.fin, nullptr, n, st))
            return 1;
        return launch_step_advance(u->state_dev, st);
    };
    L.key.kind = dm_unet::GK_CG;
    L.key.objective = objective; L.key.self_cond = self_cond;
    L.key.cg_mean = mean; L.key.cg_grad = grad;
    if (run_steps(L.r, L.key, n_steps, front, back, nullptr, host)) return 1;
    return table_loop_end(L, a->out);
}

}  // namespace dm

extern "C" {

int dm_sample_classifier_guided(dm_unet* u, const dm_cguide_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return sample_cg_impl(u, a);
}

int dm_op_cg_mean(const float* x, const float* model_out, const float* c_host, int objective, float* mean, float* x_start_out,
                  int B, int64_t per, void* stream) {
    DM_REQUIRE(x && model_out && c_host && mean, "null argument");
    DM_REQUIRE(B > 0 && per > 0, "empty tensor");
    return table_op(c_host, 1, stream, [&](const float* cd, hipStream_t s) {
        return launch_cg_mean(x, model_out, cd, nullptr, STEP_ROW_FIRST, per, objective, mean, x_start_out, (int64_t)B * per, s);
    });
}

int dm_op_cg_finish(const float* mean, const float* grad, const float* z, const float* c_host, uint64_t seed, uint64_t draw,
                    uint64_t element_offset, float* out, float* guided_out, int B, int64_t per, void* stream) {
    DM_REQUIRE(mean && grad && c_host && out, "null argument");
    DM_REQUIRE(B > 0 && per > 0, "empty tensor");
    if (draw_args_ok(z, draw, element_offset)) return 1;
    return state_op(draw_state(z != nullptr, seed, draw, element_offset), c_host, 1, stream,
                    [&](const SamplerState* st, const float* cd, hipStream_t s) {
                        return launch_cg_finish(mean, grad, z, 0, cd, st, STEP_ROW_FIRST, per, out, nullptr, nullptr, guided_out,
                                                (int64_t)B * per, s);
                    });
}

}  // extern "C"
