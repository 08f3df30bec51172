// Bits-per-dim evaluation on the C ABI: the variational-bound loop (dm_eval_bpd) and its kernels on their own
// (dm_op_bpd_*).  Included by dm_api.hip after dm_sampler.inc (the loop scaffolding) and dm_learned.inc (lv_unet_ok);
// kernels in bpd.hip.

namespace dm {

static_assert(DM_BPD_COEFS == BPD_NCOLS && DM_BPD_COEFS == DM_EDM_COEFS,
              "the bits-per-dim step table lives in the handle's EDM table buffer: the row widths must agree");
static_assert(DM_BPD_CHUNK == BPD_CHUNK, "bpd.h and dm_hip.h disagree");
static_assert(sizeof(dm_bpd_args) == 136, "dm_bpd_args is bound field by field (_lib.py: BpdArgs)");

// Improved DDPM's calc_bpd_loop: for every row of the table x_t = q_sample(x0, t, z), the model, the three per-image
// means.  One step -- bpd_step_in_kernel, [the channel copy of an image condition,] the forward, bpd_terms_kernel, the
// finishing pass that also advances the step counter -- is one linear chain that touches handle-owned memory only and
// reads everything that differs between two calls of one shape (times, table, step counter and count, seed, Philox
// offset) as device data: it is captured once per shape and serves any `times`.
static int eval_bpd_impl(dm_unet* u, const dm_bpd_args* a) {
    DM_REQUIRE(a->times_host && a->table_host && a->x0 && a->terms_out, "null argument");
    DM_REQUIRE(a->n_steps > 0 && a->B > 0, "empty run");
    if (handle_ready(u) || image_unet_only(u)) return 1;
    const bool learned = a->learned != 0;
    const int B = a->B, H = a->H, W = a->W, n_steps = a->n_steps, ctx_tokens = a->ctx_tokens, cond_channels = a->cond_channels;
    DM_REQUIRE(a->objective >= DM_OBJ_PRED_NOISE && a->objective <= DM_OBJ_PRED_V, "unknown objective");
    DM_REQUIRE((a->cond == nullptr) == (cond_channels == 0) && cond_channels >= 0, "cond and cond_channels come together");
    DM_REQUIRE((a->ctx == nullptr) == (ctx_tokens == 0) && ctx_tokens >= 0, "ctx and ctx_tokens come together");
    if (learned) {
        DM_REQUIRE(!a->ctx && !a->cond && a->objective == DM_OBJ_PRED_NOISE,
                   "LearnedGaussianDiffusion calls model(x, t) only and reads the first half of its output as noise");
        if (lv_unet_ok(u)) return 1;
    } else {
        DM_REQUIRE(u->out_dim == u->cfg.channels, "bits per dim with a fixed variance needs out_dim == channels");
        DM_REQUIRE(u->cfg.input_channels == u->cfg.channels + cond_channels,
                   "U-Net input channels != channels + cond_channels (self-conditioning has no bits-per-dim loop)");
    }
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    const int C = u->cfg.channels, Cin = C + cond_channels;
    const int64_t per = (int64_t)C * H * W, n = (int64_t)B * per;
    DM_REQUIRE(per % 4 == 0, "C * H * W must be a multiple of 4");
    const int64_t n_out = learned ? 2 * n : n, n_in = (int64_t)B * Cin * H * W;
    const int64_t n_ctx = a->ctx ? (int64_t)B * ctx_tokens * u->cfg.text_emb_dim : 0;
    const float* noise = a->noise;

    SamplerRun r;
    if (grow_tables(u, TAB_INT | TAB_FLOAT, n_steps, 1) || run_begin(r, u, a->stream, a->use_graph)) return 1;
    hipStream_t s = r.s;
    // workspace: [x0 copy | x_t | model output (n or 2n) | result rows | partial sums | ticket | [x | cond] | ctx | forward arena].
    // The result rows are sized by the table's capacity, not by this call's step count: the offsets behind them, which a
    // captured step holds, then move only when the tables grow, and that drops the graph anyway.
    float *x0, *xt, *mo, *rows, *part, *xin, *ctxbuf;
    unsigned* ticket;
    auto layout = [&](Arena& A) {
        x0 = A.alloc(n);
        xt = A.alloc(n);
        mo = A.alloc(n_out);
        rows = A.alloc((size_t)3 * B * u->edm_cap);
        part = A.alloc(bpd_part_floats(B, per));
        ticket = reinterpret_cast<unsigned*>(A.alloc(1));  // the finishing pass counts its workgroups here
        xin = cond_channels ? A.alloc(n_in) : nullptr;
        ctxbuf = a->ctx ? A.alloc(n_ctx) : nullptr;
    };
    const float* ctx_marker = a->ctx ? reinterpret_cast<const float*>(16) : nullptr;
    if (run_workspace(r, layout, [&](Arena& dry) {
            return unet_forward_impl(u, dry, nullptr, nullptr, u->times_dev, u->state_dev, ctx_marker, ctx_tokens, nullptr, B, H, W, s);
        }))
        return 1;
    if (run_upload(r, n_steps, a->times_host, nullptr, a->table_host, 0, a->seed, a->sample_offset * (uint64_t)per)) return 1;
    DM_CHECK_HIP(hipMemcpyAsync(x0, a->x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    DM_CHECK_HIP(hipMemsetAsync(ticket, 0, sizeof(unsigned), s));
    if (a->ctx) DM_CHECK_HIP(hipMemcpyAsync(ctxbuf, a->ctx, n_ctx * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (a->cond && launch_copy_channels(a->cond, xin, B, cond_channels, Cin, C, H * W, s)) return 1;
    if (a->prior_out && launch_bpd_prior(x0, a->prior_sqrt_ac, a->prior_logvar, a->prior_out, B, per, s)) return 1;

    auto step = [&](hipStream_t st) -> int {
        r.rewind();
        if (launch_bpd_step_in(x0, noise, n, u->edm_tab_dev, u->state_dev, STEP_ROW_STEP, xt, n, st)) return 1;
        if (xin && launch_copy_channels(xt, xin, B, C, Cin, 0, H * W, st)) return 1;
        if (unet_forward_impl(u, r.A, xin ? xin : xt, nullptr, u->times_dev, u->state_dev, ctxbuf, ctx_tokens, mo, B, H, W, st))
            return 1;
        return launch_bpd_terms(mo, x0, xt, noise, n, u->edm_tab_dev, u->state_dev, learned, a->objective, a->clip_denoised, part,
                                rows, ticket, B, per, st);
    };
    // profiling leg: park the GPU while the host enqueues, so that event intervals are kernel times (<= 8 steps)
    if (!a->use_graph && prof::enabled() && n_steps <= 8 && launch_spin(8.0 * n_steps, s)) return 1;
    dm_unet::GraphKey key;
    key.kind = dm_unet::GK_BPD;
    key.B = B; key.H = H; key.W = W; key.ctx_tokens = ctx_tokens; key.cond_channels = cond_channels;
    key.objective = a->objective;
    key.bpd_flags = (learned ? 1 : 0) | (a->clip_denoised ? 2 : 0);
    key.noise = noise; key.ws = u->ws; key.times = u->times_dev; key.tab = u->edm_tab_dev;
    if (run_steps(r, key, n_steps, step)) return 1;
    DM_CHECK_HIP(hipMemcpyAsync(a->terms_out, rows, (size_t)3 * B * n_steps * sizeof(float), hipMemcpyDeviceToDevice, s));
    return run_finish(r);
}

}  // namespace dm

extern "C" {

int dm_eval_bpd(dm_unet* u, const dm_bpd_args* a) {
    DM_REQUIRE(u && a, "null argument");
    DM_REQUIRE(a->sample_offset < (uint64_t(1) << 40), "sample_offset out of range");
    return eval_bpd_impl(u, a);
}

int dm_op_bpd_step_in(const float* x0, const float* z, const float* c_host, uint64_t seed, uint64_t draw, uint64_t element_offset,
                      float* x_t, int B, int64_t per, void* stream) {
    DM_REQUIRE(x0 && c_host && x_t, "null argument");
    DM_REQUIRE(B > 0 && per > 0, "empty tensor");
    if (draw_args_ok(z, draw, element_offset)) return 1;
    return state_op(draw_state(z != nullptr, seed, draw, element_offset), c_host, 1, stream,
                    [&](const SamplerState* st, const float* cd, hipStream_t s) {
                        return launch_bpd_step_in(x0, z, 0, cd, st, STEP_ROW_FIRST, x_t, (int64_t)B * per, s);
                    });
}

int dm_op_bpd_terms(const float* model_out, const float* x0, const float* x_t, const float* z, const float* c_host, int learned,
                    int objective, int clip_denoised, float* terms_out_host, int B, int64_t per, void* stream) {
    DM_REQUIRE(model_out && x0 && x_t && z && c_host && terms_out_host, "null argument");
    DM_REQUIRE(B > 0 && B <= 65535 && per > 0 && per % 4 == 0, "B images (1 .. 65535) of C*H*W values, a multiple of 4");
    // scratch behind the one table row (64 bytes: the doubles stay aligned): [partial sums | 3 B results]
    const size_t n_part = bpd_part_floats(B, per), nb = (size_t)3 * B;
    return table_op(c_host, 1, stream, [&](float* cd, hipStream_t s) {
        float* part = cd + BPD_NCOLS;
        return launch_bpd_terms(model_out, x0, x_t, z, 0, cd, nullptr, learned, objective, clip_denoised, part, part + n_part, nullptr, B, per, s);
    }, BPD_NCOLS, n_part + nb, {{terms_out_host, n_part, nb}});
}

int dm_op_bpd_prior(const float* x0, float sqrt_ac, float logvar, float* prior, int B, int64_t per, void* stream) {
    DM_REQUIRE(x0 && prior, "null argument");
    return launch_bpd_prior(x0, sqrt_ac, logvar, prior, B, per, static_cast<hipStream_t>(stream));
}

}  // extern "C"
