// RePaint inpainting on the C ABI: the flattened sampling loop and the single-row entry point (dm_op_repaint_step).
// Included by dm_api.hip after dm_sampler.inc (the loop scaffolding) and dm_edm.inc (the state helper of the dm_op_*
// passes); kernel in repaint.hip.

namespace dm {

static_assert(DM_REPAINT_COEFS == RP_NCOLS && DM_REPAINT_COEFS == DM_EDM_COEFS,
              "the RePaint table lives in the handle's EDM table buffer: the row widths must agree");
static_assert(DM_REPAINT_AUTO == RP_AUTO && DM_REPAINT_BLEND == RP_BLEND && DM_REPAINT_STEP == RP_STEP &&
                  DM_REPAINT_STEP_NEXT == RP_STEP_NEXT && DM_REPAINT_LAST == RP_LAST,
              "mode ids of the header and repaint.h");

// a row of the table must not send the kernel outside all_steps
static int repaint_table_ok(const float* tab, int n_rows, int n_frames, bool frames) {
    for (int r = 0; r < n_rows; ++r) {
        const float slot = tab[(size_t)r * RP_NCOLS + RP_SLOT];
        DM_REQUIRE(slot == (float)(int)slot && slot >= -1.0f, "table column 13 is a frame index or -1");
        DM_REQUIRE(!frames || slot < (float)n_frames, "table column 13 names a frame beyond n_frames");
    }
    return 0;
}

// p_sample_loop of DD/repaint.py:644-681 with a mask, unrolled by the host into n_rows rows (one U-Net evaluation each).
// One row -- the forward at the row's time, repaint_step_kernel, the row counter -- is one linear chain that reads
// everything that differs between two calls of one shape (tables, row counter and count, seed, Philox offset, unnormalise,
// gt and mask through workspace copies) as device data: it is captured once per shape and replayed n_rows times.
static int sample_repaint_impl(dm_unet* u, const dm_repaint_args* a) {
    DM_REQUIRE(a->times_host && a->table_host && a->x_T && a->gt && a->mask && a->out, "null argument");
    DM_REQUIRE(a->n_rows > 0 && a->B > 0, "empty run");
    DM_REQUIRE(a->objective >= DM_OBJ_PRED_NOISE && a->objective <= DM_OBJ_PRED_V, "unknown objective");
    if (handle_ready(u)) return 1;
    const char* const time_msg = "RePaint calls model(x, t) with an integer time: no text-conditional or float-time U-Net";
    DM_REQUIRE(u->cfg.learned_sinusoidal_dim == 0, time_msg);
    if (plain_unet_ok(u, "RePaint needs a U-Net with out_dim == input channels == channels (no self-conditioning, no image condition)",
                      time_msg))
        return 1;
    const int B = a->B, H = a->H, W = a->W, n_rows = a->n_rows, objective = a->objective;
    const int C = u->cfg.channels, Cm = a->mask_channels, HW = H * W;
    DM_REQUIRE(Cm == 1 || Cm == C, "the mask has 1 or C channels");
    DM_REQUIRE(!a->all_steps || a->n_frames > 0, "all_steps comes with its frame count");
    if (check_hw(u, H, W)) return 1;
    if (repaint_table_ok(a->table_host, n_rows, a->n_frames, a->all_steps != nullptr)) return 1;
    const int64_t per = (int64_t)C * HW, n = (int64_t)B * per, n_mask = (int64_t)B * Cm * HW;
    const uint64_t elem_off = a->sample_offset * (uint64_t)per;
    DM_REQUIRE(elem_off % 4 == 0, "sample_offset * C * H * W must be a multiple of 4");

    // The default loop has about 3000 rows against the 1000 steps of a DDPM run.  The buffers grow in units of 4096 rows,
    // so that a change of the resampling settings keeps their addresses, and with them the captured graph.
    // workspace: [x | result | eps | gt | mask | forward arena]
    TableLoop L;
    float *eps, *gt, *mask;
    auto layout = [&](Arena& A) {
        eps = A.alloc(n);
        gt = A.alloc(n);
        mask = A.alloc(n_mask);
    };
    if (table_loop_begin(L, u, *a, n_rows, 4096, elem_off, layout)) return 1;
    hipStream_t s = L.s;
    float* const xbuf = L.xbuf;
    const float* tab = L.tab;
    RepaintNoise z;
    if (a->noise) z = RepaintNoise{a->noise, a->noise + n, a->noise + 2 * n, 3 * n};
    float* all_steps = a->all_steps;

    DM_CHECK_HIP(hipMemcpyAsync(gt, a->gt, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    DM_CHECK_HIP(hipMemcpyAsync(mask, a->mask, n_mask * sizeof(float), hipMemcpyDeviceToDevice, s));
    // prologue: the blend in front of row 0's model call
    if (launch_repaint_step(RP_BLEND, objective, xbuf, nullptr, z, tab, 0, u->state_dev, gt, mask, Cm, per, HW, xbuf, nullptr,
                            nullptr, nullptr, n, s))
        return 1;

    auto row = [&](hipStream_t st) -> int {
        L.r.rewind();
        if (unet_forward_impl(u, L.r.A, xbuf, nullptr, u->times_dev, u->state_dev, nullptr, 0, eps, B, H, W, st)) return 1;
        if (launch_repaint_step(RP_AUTO, objective, xbuf, eps, z, tab, 0, u->state_dev, gt, mask, Cm, per, HW, xbuf, all_steps,
                                L.fin, nullptr, n, st))
            return 1;
        return launch_step_advance(u->state_dev, st);
    };
    L.key.kind = dm_unet::GK_REPAINT;
    L.key.objective = objective;
    L.key.mask_channels = Cm;
    if (run_steps(L.r, L.key, n_rows, row)) return 1;
    return table_loop_end(L, a->out);
}

}  // namespace dm

extern "C" {

int dm_sample_repaint(dm_unet* u, const dm_repaint_args* a) {
    DM_REQUIRE(u && a, "null argument");
    return sample_repaint_impl(u, a);
}

int dm_op_repaint_step(int mode, int objective, const float* x, const float* eps, const float* gt, const float* mask,
                       int mask_channels, const float* z_jump, const float* z_known, const float* z_step, const float* c_host,
                       int unnormalize, uint64_t seed, uint64_t row, uint64_t element_offset, float* out, float* x_start_out,
                       int B, int C, int HW, void* stream) {
    DM_REQUIRE(x && c_host && out, "null argument");
    DM_REQUIRE(mode >= DM_REPAINT_BLEND && mode <= DM_REPAINT_LAST, "dm_op_repaint_step runs one of the four explicit modes");
    DM_REQUIRE(B > 0 && C > 0 && HW > 0, "empty tensor");
    DM_REQUIRE(element_offset % 4 == 0, "Philox element offset must be a multiple of 4 (one counter serves 4 elements)");
    DM_REQUIRE(row < (uint64_t(1) << 30), "row index out of range");
    // which draws the launch reads: with injected noise those tensors must be there (the others are never touched)
    const int n_tab = mode == DM_REPAINT_STEP_NEXT ? 2 : 1;  // STEP_NEXT also reads the next row
    const float* cb = c_host + (size_t)(n_tab - 1) * RP_NCOLS;
    const bool need_step = mode != DM_REPAINT_BLEND && c_host[5] != 0.0f;
    const bool need_known = mode == DM_REPAINT_BLEND || mode == DM_REPAINT_STEP_NEXT;
    const bool need_jump = mode == DM_REPAINT_STEP_NEXT && cb[RP_JUMP] != 0.0f;
    RepaintNoise z;
    if (z_jump || z_known || z_step) {
        DM_REQUIRE((!need_step || z_step) && (!need_known || z_known) && (!need_jump || z_jump),
                   "with injected noise every draw the row reads must be given");
        const float* any = z_step ? z_step : (z_known ? z_known : z_jump);
        z = RepaintNoise{z_jump ? z_jump : any, z_known ? z_known : any, z_step ? z_step : any, 0};
    }
    const int64_t per = (int64_t)C * HW;
    SamplerState st_host{};
    st_host.step = (int)row;
    st_host.n_steps = (int)row + 1;
    st_host.unnormalize = unnormalize ? 1 : 0;
    st_host.seed = seed;
    st_host.off4 = element_offset / 4;
    return state_op(st_host, c_host, n_tab, stream, [&](const SamplerState* st, const float* cd, hipStream_t s) {
        return launch_repaint_step(mode, objective, x, eps, z, cd, (int)row, st, gt, mask, mask_channels, per, HW, out, nullptr,
                                   nullptr, x_start_out, (int64_t)B * per, s);
    });
}

}  // extern "C"
