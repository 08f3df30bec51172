// Learned-variance Gaussian diffusion (Improved DDPM, arXiv 2102.09672, as DD/learned_gaussian_diffusion.py has it):
// launchers of learned.hip and the per-element arithmetic of the variational-bound term, which host code can call too.
#pragma once

#include "dm_common.h"

namespace dm {

// Columns of one row of the step table (DM_LV_COEFS floats, include/dm_hip.h): what `extract` gathers at the step's time.
// Columns 0..3 and 5 sit where ddpm_step_table has them, so ddpm_coefs / ddpm_x_start (step_device.h) read the row as it is.
enum LvCol : int {
    LV_RECIP = 0,     // sqrt_recip_alphas_cumprod[t]
    LV_RECIPM1 = 1,   // sqrt_recipm1_alphas_cumprod[t]
    LV_COEF1 = 2,     // posterior_mean_coef1[t]
    LV_COEF2 = 3,     // posterior_mean_coef2[t]
    LV_MIN_LOG = 4,   // posterior_log_variance_clipped[t]
    LV_NOISE = 5,     // 1 when t > 0, else 0: the step adds noise
    LV_MAX_LOG = 6,   // log(betas)[t]
    LV_NCOLS = 16,
};
// Columns of one per-image training row (DM_LV_TRAIN_COEFS floats).  Columns 0, 1 sit where q_sample_kernel reads them.
enum LvTrainCol : int {
    LVT_SQRT_AC = 0,     // sqrt_alphas_cumprod[t_b]
    LVT_SQRT_1M_AC = 1,  // sqrt_one_minus_alphas_cumprod[t_b]
    LVT_RECIP = 2,       // sqrt_recip_alphas_cumprod[t_b]
    LVT_RECIPM1 = 3,     // sqrt_recipm1_alphas_cumprod[t_b]
    LVT_COEF1 = 4,       // posterior_mean_coef1[t_b]
    LVT_COEF2 = 5,       // posterior_mean_coef2[t_b]
    LVT_MIN_LOG = 6,     // posterior_log_variance_clipped[t_b], as p_mean_variance's min_log (:97)
    LVT_TRUE_LOG = 7,    // posterior_log_variance_clipped[t_b], as q_posterior's true log variance (:123)
    LVT_MAX_LOG = 8,     // log(betas)[t_b]
    LVT_T0 = 9,          // 1 when t_b == 0 (the image's vb term is the decoder NLL), else 0 (the KL)
    LVT_NCOLS = 12,
};

#pragma clang fp contract(off)
// model_log_variance of p_mean_variance (:99-101) from the variance half v of the model output
__host__ __device__ inline float lv_logvar(float v, float min_log, float max_log) {
    const float frac = (v + 1.0f) * 0.5f;  // unnormalize_to_zero_to_one
    return frac * max_log + (1.0f - frac) * min_log;
}

// approx_standard_normal_cdf (:31-32) and its derivative as autograd forms it: 0.5 (1 - tanh^2) d(inner)
__host__ __device__ inline float lv_cdf(float x, float* dcdf) {
    const float k = 0.7978845608028654f;  // sqrt(2 / pi)
    const float th = tanhf(k * (x + 0.044715f * (x * x * x)));
    *dcdf = 0.5f * ((1.0f - th * th) * (k * (1.0f + (3.0f * 0.044715f) * (x * x))));
    return 0.5f * (1.0f + th);
}

// One element of the variational-bound term of p_losses (:123-138) in nats, BEFORE meanflat and the 1 / ln 2:
//   t0 == false: normal_kl(true_mean, true_logvar, model_mean, logvar)                                   (:25-29)
//   t0 == true:  -discretized_gaussian_log_likelihood(x_start, means = model_mean, log_scales = 0.5 logvar)  (:34-53)
// *dlv = d term / d logvar (the mean is detached, :128).  The NLL's derivative goes through inv_stdv = exp(-0.5 logvar)
// in both CDF arguments (d arg / d logvar = -0.5 arg) and is 0 where log's clamp at 1e-15 is active.
__host__ __device__ inline float lv_vb_term(bool t0, float x_start, float true_mean, float true_logvar, float model_mean,
                                            float logvar, float* dlv) {
    if (!t0) {
        const float d = true_mean - model_mean;
        const float e1 = expf(true_logvar - logvar), e2 = expf(-logvar);
        *dlv = 0.5f * ((1.0f - e1) - (d * d) * e2);
        return 0.5f * ((((-1.0f + logvar) - true_logvar) + e1) + (d * d) * e2);
    }
    const float eps = 1e-15f;
    const float centered = x_start - model_mean;
    const float inv_stdv = expf(-(0.5f * logvar));
    const float bin = 0.00392156862745098f;  // 1. / 255.
    const float plus_in = inv_stdv * (centered + bin), min_in = inv_stdv * (centered - bin);
    float dplus, dmin;
    const float cdf_plus = lv_cdf(plus_in, &dplus), cdf_min = lv_cdf(min_in, &dmin);
    dplus = dplus * (-0.5f * plus_in);  // d cdf_plus / d logvar
    dmin = dmin * (-0.5f * min_in);
    float arg, darg;
    if (x_start < -0.999f) {
        arg = cdf_plus;
        darg = dplus;
    } else if (x_start > 0.999f) {
        arg = 1.0f - cdf_min;
        darg = -dmin;
    } else {
        arg = cdf_plus - cdf_min;
        darg = dplus - dmin;
    }
    *dlv = arg >= eps ? -(darg / arg) : 0.0f;  // clamp(min = eps) passes the gradient where arg >= eps
    return -logf(fmaxf(arg, eps));
}
#pragma clang fp contract(fast)

// One reverse step, p_mean_variance (:93-111) + p_sample, on the (B, 2C, H, W) model output `eps2` (noise half, variance
// half).  Row st->step of `tab` (LV_NCOLS floats) with row_mode STEP_ROW_STEP, row 0 with STEP_ROW_FIRST (step_device.h);
// n = B * per, per % 4 == 0, 16-byte pointers:
//   logvar = lv_logvar(v, c[4], c[6]);  x_start = clamp(c[0] x - c[1] eps, -1, 1);  mean = c[2] x_start + c[3] x
//   r = mean + exp(0.5 logvar) * z,  z = row `step` of noise (stride noise_step_stride), or the Philox draw step + 1 under
//   st->seed when noise == nullptr; a row with c[5] == 0 reads and draws nothing (z = 0).
// out = r (out may be x); all_steps (optional) frame step + 1 = r; final_out (optional) on step n_steps - 1 =
// st->unnormalize ? (r + 1) / 2 : r.  mean_out / logvar_out / x_start_out (optional) are p_mean_variance's values.
int launch_lv_step(const float* x, const float* eps2, const float* noise, int64_t noise_step_stride, const float* tab,
                   const SamplerState* st, int row_mode, int64_t per, float* out, float* all_steps, float* final_out, float* mean_out,
                   float* logvar_out, float* x_start_out, int64_t n, hipStream_t s);

// p_losses (:113-146) behind the model call, one workgroup per image.  out2 (B, 2C, H, W); x_start, noise, x_t (the
// q_sample output) (B, C, H, W); tab: B device rows of LVT_NCOLS floats.
//   mse_part[b] = mean((pred - noise)^2);  vb_part[b] = meanflat(vb term) / ln 2;  part[b] = mse_part[b] + w vb_part[b]
//   *loss = loss_scale * mean_b(part[b])
//   dout noise half    = loss_scale * 2 (pred - noise) / (B per)
//   dout variance half = loss_scale * w / (ln 2 B per) * d term / d logvar * 0.5 (max_log - min_log)
// clip: x_start of the model mean is clamped to [-1, 1] (the mean is detached: values change, gradients do not).
int launch_lv_loss(const float* out2, const float* x_start, const float* noise, const float* x_t, const float* tab,
                   float vb_loss_weight, int clip, float* dout, float* part, float* mse_part, float* vb_part, float* loss,
                   int B, int64_t per, float loss_scale, hipStream_t s);

}  // namespace dm
