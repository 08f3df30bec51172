// ElucidatedDiffusion (Karras et al. "EDM") sampling and training: launchers of edm.hip.
// Reference: DD/elucidated_diffusion.py:76-110 (preconditioning), :129-187 (Heun), :189-224 (DPM-Solver++(2M)).
#pragma once

#include "step_device.h"

namespace dm {

// Columns of one row of the step table (DM_EDM_COEFS floats, include/dm_hip.h).  Every value is computed by the host
// the way the reference computes it; the kernels only multiply, add and divide.
enum EdmCol : int {
    EDM_CHURN = 0,     // sqrt(sigma_hat^2 - sigma^2), 0 when gamma == 0
    EDM_S_NOISE = 1,
    EDM_C_IN = 2,      // preconditioning at sigma_hat (Heun) / sigma (DPM++)
    EDM_C_NOISE = 3,
    EDM_C_SKIP = 4,
    EDM_C_OUT = 5,
    EDM_SIGMA = 6,     // sigma_hat
    EDM_DT = 7,        // sigma_next - sigma_hat
    EDM_C_IN2 = 8,     // preconditioning at sigma_next (Heun); DPM++: a = sigma_fn(t_next) / sigma_fn(t)
    EDM_C_NOISE2 = 9,  //                                      DPM++: b = expm1(-h)
    EDM_C_SKIP2 = 10,  //                                      DPM++: g (gamma of the multistep blend)
    EDM_C_OUT2 = 11,   //                                      DPM++: 1 - g
    EDM_SIGMA2 = 12,   // sigma_next
    EDM_HALF_DT = 13,  // 0.5 * (sigma_next - sigma_hat)
    EDM_LOSS_W = 14,   // training rows only: loss_weight(sigma) (:228-229)
    EDM_NCOLS = 16,
};
enum : int { EDM_A = EDM_C_IN2, EDM_B = EDM_C_NOISE2, EDM_G = EDM_C_SKIP2, EDM_OMG = EDM_C_OUT2 };

// Rows are selected by a StepRows (step_device.h: step / image / first; STEP_ROW_IMAGE is preconditioned_network_forward
// on a (B,) sigma); n = B * per, per % 4 == 0, 16-byte pointers.
// e[r] = [t | sin(t w 2 pi) | cos(t w 2 pi)] (learned) or [sin(t f) | cos(t f)] for a REAL-valued time.
// st == nullptr: row r reads t[r]; else one row (R == 1) reads t[st->step * t_stride]
int launch_sinusoid_ft(const float* t, int t_stride, const SamplerState* st, const float* freqs, float* e, int R, int half,
                       hipStream_t s, bool learned);
// xhat = x + churn * (S_noise * eps), xin = c_in * xhat.  eps: row `step` of noise (stride noise_step_stride), or the
// Philox draw step + 1 under st->seed when noise == nullptr; not read at all when churn == 0.  xhat may be nullptr.
int launch_edm_churn_in(const float* x, const float* noise, int64_t noise_step_stride, StepRows r, float* xhat, float* xin,
                        int64_t n, hipStream_t s);
// D = c_skip xhat + c_out F [clamped]; d = (xhat - D) / sigma_hat; xnext = xhat + dt d; xin2 = c_in' xnext.
// Every output may be nullptr.
int launch_edm_euler(const float* xhat, const float* F, StepRows r, int clamp, float* D_out, float* d_out, float* xnext,
                     float* xin2, int64_t n, hipStream_t s);
// D' = c_skip' xnext + c_out' F2 [clamped]; d' = (xnext - D') / sigma_next; out = xhat + half_dt (d + d').  out may be xnext.
int launch_edm_heun(const float* xhat, const float* d, const float* xnext, const float* F2, StepRows r, int clamp, float* out,
                    int64_t n, hipStream_t s);
// D = c_skip x + c_out F; out = a x - b ((1 - g) D + g d_old); d_old = D.  out may be x.
int launch_edm_dpmpp(const float* x, const float* F, float* d_old, StepRows r, float* out, int64_t n, hipStream_t s);
// out = (clamp(x, -1, 1) + 1) / 2
int launch_edm_finalize(const float* x, float* out, int64_t n, hipStream_t s);
// out = scale * x
int launch_edm_scale(const float* x, float scale, float* out, int64_t n, hipStream_t s);

// Training rows (one per image, STEP_ROW_IMAGE): c_in, c_noise, c_skip, c_out, sigma in their sampling columns, EDM_LOSS_W.
// x0 = 2 img - 1; noised = x0 + sigma eps; xin = c_in noised
int launch_edm_noise_in(const float* img, const float* eps, StepRows r, float* x0, float* noised, float* xin, int64_t n,
                        hipStream_t s);
// D = c_skip noised + c_out F; *loss = loss_scale * mean_b(loss_weight_b * mean((D - x0)^2)); dF = d(loss) / dF.
// tab: B device rows; part: B floats of workspace; D_out may be nullptr.
int launch_edm_loss(const float* noised, const float* F, const float* x0, const float* tab, float* dF, float* D_out, float* part,
                    float* loss, int B, int64_t per, float loss_scale, hipStream_t s);
// dW[k] (+)= sum_b 2 pi t_b (de_sin[b][k] cos[b][k] - de_cos[b][k] sin[b][k]) from the taped e0 = [t | sin | cos] rows of
// width 2 half + 1; learned == false writes zeros (random_fourier_features)
int launch_sinusoid_ft_bwd(const float* de0, const float* e0, float* dw, int B, int half, bool learned, int accumulate,
                           hipStream_t s);
// The same embedding's gradient with respect to its float time, from the same taped rows (frozen weights pass it on too):
// dt[b] = de0[b][0] + 2 pi sum_k w_k (de_sin[b][k] cos[b][k] - de_cos[b][k] sin[b][k]), k ascending, summed in double
int launch_sinusoid_ft_tgrad(const float* de0, const float* e0, const float* freqs, float* dt, int B, int half, hipStream_t s);

}  // namespace dm
