// Continuous-time Gaussian diffusion (log-SNR time; noise and v objectives): launchers of ct.hip.
// Reference: DD/continuous_time_gaussian_diffusion.py:155-251, DD/v_param_continuous_time_gaussian_diffusion.py:72-162.
#pragma once

#include "edm.h"

namespace dm {

// Columns of one table row (DM_CT_COEFS floats, include/dm_hip.h).  Every value is a 0-dim (sampling) or per-image
// (training) fp32 tensor expression of the reference, computed by the host; the kernels only multiply, add, divide, clamp.
enum CtCol : int {
    CT_LOG_SNR = 0,     // log_snr(time): the U-Net's float time
    CT_ALPHA = 1,       // sqrt(sigmoid(log_snr))
    CT_SIGMA = 2,       // sqrt(sigmoid(-log_snr))
    CT_ALPHA_NEXT = 3,  // sqrt(sigmoid(log_snr_next))
    CT_C = 4,           // -expm1(log_snr - log_snr_next)
    CT_ONE_M_C = 5,     // 1 - c
    CT_SQRT_VAR = 6,    // sqrt(sigmoid(-log_snr_next) * c); 0 on the step with time_next == 0 (it adds no noise)
    CT_AN_OVER_A = 7,   // alpha_next / alpha   (noise objective without clipping)
    CT_C_SIGMA = 8,     // c * sigma            (noise objective without clipping)
    CT_LOSS_W = 9,      // training rows only: 1, or clamp(snr, min = gamma) / snr (min-SNR weighting)
    // DPM-Solver++ rows only (ct_dpmpp_table: columns 0..2 as above, 3..9 zero); h = (log_snr_next - log_snr) / 2
    CT_DPM_CX = 10,     // sigma_next / sigma
    CT_DPM_CD = 11,     // -alpha_next * expm1(-h)
    CT_DPM_G = 12,      // h / (2 h_last); 0 at order 1 and on the first row
    CT_NCOLS = 16,
};
enum CtObjective : int { CT_PRED_NOISE = 0, CT_PRED_V = 1 };

// Rows are selected by a StepRows (step_device.h: step / image / first); n = B * per, per % 4 == 0, 16-byte pointers.
// One reverse step, p_mean_variance + p_sample of both classes:
//   v:               x_start = alpha x - sigma F [clamped];        mean = alpha_next (x (1 - c) / alpha + c x_start)
//   noise, clip:     x_start = (x - sigma F) / alpha, clamped;     the same mean
//   noise, no clip:  mean = (alpha_next / alpha) (x - (c sigma) F)   (x_start_out must be nullptr)
//   out = mean + sqrt_var * eps;  eps: row `step` of noise (stride noise_step_stride), or the Philox draw step + 1 under
//   st->seed when noise == nullptr; a row with sqrt_var == 0 reads and draws nothing.  out may be x.
int launch_ct_step(const float* x, const float* F, const float* noise, int64_t noise_step_stride, StepRows r, int objective,
                   int clip, float* out, float* x_start_out, int64_t n, hipStream_t s);
// One DPM-Solver++ (2M, data prediction; arXiv 2211.01095, Algorithm 2) step on a row with columns CT_DPM_*:
//   x_start as in launch_ct_step (v: alpha x - sigma F; noise: (x - sigma F) / alpha), clamped when clip
//   D = x_start + g (x_start - hist)   (g == 0: hist is not read, whatever it holds);   out = c_x x + c_D D
// hist receives x_start.  out may be x; hist aliases neither.  A thread touches its own 4 elements only.
int launch_ct_dpmpp_step(const float* x, const float* F, float* hist, StepRows r, int objective, int clip, float* out,
                         int64_t n, hipStream_t s);
// q_sample + regression target: x0 = 2 img - 1 (normalize != 0) or img; x = x0 alpha_b + eps sigma_b;
// target = eps (noise) or alpha_b eps - sigma_b x0 (v)
int launch_ct_noise_in(const float* img, const float* eps, StepRows r, int objective, int normalize, float* x, float* target,
                       int64_t n, hipStream_t s);
// *loss = loss_scale * mean_b(w_b * mean((F - target)^2)); dF = loss_scale * w_b * 2 (F - target) / (B * per).
// tab: B device rows (w_b = column CT_LOSS_W); part: B floats of workspace
int launch_ct_loss(const float* F, const float* target, const float* tab, float* dF, float* part, float* loss, int B,
                   int64_t per, float loss_scale, hipStream_t s);
// Per image, for a trained schedule: out[b] = [sum dX x0, sum dX eps, dt[b] (0 when dt == nullptr), mean((F - target)^2)];
// x0 = 2 img - 1 (normalize != 0) or img.  out: B rows of 4 device floats
int launch_ct_sched_reduce(const float* dx, const float* img, const float* eps, const float* F, const float* target,
                           const float* dt, int normalize, float* out, int B, int64_t per, hipStream_t s);

}  // namespace dm
