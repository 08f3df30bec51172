// Weighted-objective Gaussian diffusion (DD/weighted_objective_gaussian_diffusion.py): launchers of weighted.hip and the
// column layout of their tables.  The U-Net predicts 2C + 2 maps per image: the noise (C), x_start (C) and two weight maps
// whose softmax over the pair blends the two x_start estimates pixel by pixel.
#pragma once

#include "dm_common.h"

namespace dm {

// Columns of one row of the step table (DM_WO_COEFS floats, include/dm_hip.h): what `extract` gathers at the step's time.
// The columns sit where the learned-variance step table has them (learned.h), so the handle's table buffer serves unchanged.
enum WoCol : int {
    WO_RECIP = 0,    // sqrt_recip_alphas_cumprod[t]
    WO_RECIPM1 = 1,  // sqrt_recipm1_alphas_cumprod[t]
    WO_COEF1 = 2,    // posterior_mean_coef1[t]
    WO_COEF2 = 3,    // posterior_mean_coef2[t]
    WO_LOGVAR = 4,   // posterior_log_variance_clipped[t]
    WO_NOISE = 5,    // 1 when t > 0, else 0: the step adds noise
    WO_NCOLS = 16,
};
// Columns of one per-image training row (DM_WO_TRAIN_COEFS floats).  Columns 0, 1 sit where q_sample_kernel reads them,
// 2, 3 where the learned-variance training rows have them.
enum WoTrainCol : int {
    WOT_SQRT_AC = 0,     // sqrt_alphas_cumprod[t_b]
    WOT_SQRT_1M_AC = 1,  // sqrt_one_minus_alphas_cumprod[t_b]
    WOT_RECIP = 2,       // sqrt_recip_alphas_cumprod[t_b]
    WOT_RECIPM1 = 3,     // sqrt_recipm1_alphas_cumprod[t_b]
    WOT_NCOLS = 12,
};

// One reverse step, p_mean_variance (:33-49) + the base class's p_sample, on the (B, 2C + 2, H, W) model output `mo`
// (image b: C noise maps, C x_start maps, the weight maps w0, w1; image stride (2C + 2) HW).  Row st->step of `tab`
// (WO_NCOLS floats) with row_mode STEP_ROW_STEP, row 0 with STEP_ROW_FIRST (step_device.h); HW % 4 == 0, 16-byte pointers:
//   s0 = sigmoid(w0 - w1), s1 = 1 - s0                                     (softmax over the pair, once per pixel)
//   x_start = s0 (c[0] x - c[1] eps) + s1 px   [clamped to [-1, 1] when clip != 0];   mean = c[2] x_start + c[3] x
//   r = mean + exp(0.5 c[4]) * z,  z = row `step` of noise (stride noise_step_stride), or the Philox draw step + 1 under
//   st->seed when noise == nullptr (counter of element b per + c HW + p); a row with c[5] == 0 reads and draws nothing.
// out = r (out may be x); all_steps (optional) frame step + 1 = r; final_out (optional) on step n_steps - 1 =
// st->unnormalize ? (r + 1) / 2 : r.  mean_out / x_start_out (optional) are p_mean_variance's mean and weighted x_start.
int launch_wo_step(const float* x, const float* mo, const float* noise, int64_t noise_step_stride, const float* tab,
                   const SamplerState* st, int row_mode, int B, int C, int64_t HW, int clip, float* out, float* all_steps,
                   float* final_out, float* mean_out, float* x_start_out, hipStream_t s);

// p_losses (:51-74) behind the model call, one workgroup per image.  mo, dout (B, 2C + 2, H, W); x_start, noise, x_t (the
// q_sample output) (B, C, H, W); tab: B device rows of WOT_NCOLS floats.  With N = B C HW, xs = c[2] x_t - c[3] pn,
// xc = clamp(xs, -2, 2), wx = s0 xc + s1 px:
//   w_part[b] = mean_b((x_start - wx)^2)   x_part[b] = mean_b((x_start - px)^2)   n_part[b] = mean_b((noise - pn)^2)
//   part[b] = w_part[b] + w_x x_part[b] + w_n n_part[b];   *loss = loss_scale * mean_b(part[b])
//   d pn = loss_scale 2 / N [w_n (pn - noise) - (wx - x_start) s0 c[3] (-2 <= xs <= 2)]
//   d px = loss_scale 2 / N [w_x (px - x_start) + (wx - x_start) s1]
//   d w0 = loss_scale 2 / N sum_c (wx - x_start) (xc - px) s0 s1;   d w1 = -d w0
int launch_wo_loss(const float* mo, const float* x_start, const float* noise, const float* x_t, const float* tab,
                   float noise_w, float x_start_w, float* dout, float* part, float* w_part, float* x_part, float* n_part,
                   float* loss, int B, int C, int64_t HW, float loss_scale, hipStream_t s);

}  // namespace dm
