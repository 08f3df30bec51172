// Classifier-guided DDPM sampling (Sohl-Dickstein et al. 2015 / Dhariwal & Nichol 2021, as DD/guided_diffusion.py:553-584
// has it): launchers of cguide.hip, the two halves of a reverse step around the host's cond_fn.
#pragma once

#include "dm_common.h"

namespace dm {

// Columns of one row of the step table (DM_CG_COEFS floats, include/dm_hip.h).  Columns 0..7 are the DDPM row of dm_sample
// as it is, so ddpm_coefs / ddpm_x_start (step_device.h) read the row unchanged.
enum CgCol : int {
    CG_SIGMA = 4,      // exp(0.5 posterior_log_variance_clipped[t])
    CG_NOISE = 5,      // 1 when t > 0, else 0: the step adds noise
    CG_VARIANCE = 8,   // posterior_variance[t], unclipped: 0 at t == 0
    CG_NCOLS = 16,
};

// Front half of a step, p_mean_variance (:543-551) behind the model call.  Row st->step of `tab` (CG_NCOLS floats) with
// row_mode STEP_ROW_STEP, row 0 with STEP_ROW_FIRST (step_device.h); n = B * per, per % 4 == 0, 16-byte pointers:
//   x_start = clamp(x_0 by `objective` from x and model_out, -1, 1);  mean = c[2] x_start + c[3] x
// mean is what cond_fn sees; x_start_out (optional) is the unguided clamped estimate.
int launch_cg_mean(const float* x, const float* model_out, const float* tab, const SamplerState* st, int row_mode, int64_t per,
                   int objective, float* mean, float* x_start_out, int64_t n, hipStream_t s);

// Back half, condition_mean (:553-569) and the draw of p_sample (:582-583):
//   m = mean + c[8] grad;   r = m + c[4] z,  z = row `step` of noise (stride noise_step_stride), or the Philox draw
//   step + 1 under st->seed when noise == nullptr; a row with c[5] == 0 reads and draws nothing (z = 0).
// out = r (out may be mean or grad); all_steps (optional) frame step + 1 = r; final_out (optional) on step n_steps - 1 =
// st->unnormalize ? (r + 1) / 2 : r;  guided_out (optional) = m.
int launch_cg_finish(const float* mean, const float* grad, const float* noise, int64_t noise_step_stride, const float* tab,
                     const SamplerState* st, int row_mode, int64_t per, float* out, float* all_steps, float* final_out,
                     float* guided_out, int64_t n, hipStream_t s);

}  // namespace dm
