// Bits-per-dim evaluation (Improved DDPM, arXiv 2102.09672: calc_bpd_loop / _vb_terms_bpd / _prior_bpd): launchers of
// bpd.hip.  The loop is in dm_bpd.inc; the per-element arithmetic is that of learned.h (lv_logvar, lv_vb_term) and
// step_device.h (ddpm_x_start).
#pragma once

#include "dm_common.h"

namespace dm {

// Columns of one row of the step table (DM_BPD_COEFS floats, include/dm_hip.h): what `extract` gathers at the step's time.
// Columns 0..4, 6 and 7 sit where ddpm_step_table has them, so ddpm_coefs / ddpm_x_start (step_device.h) read the row as
// it is; 6 and 7 are q_sample's pair as well.
enum BpdCol : int {
    BPD_RECIP = 0,       // sqrt_recip_alphas_cumprod[t]
    BPD_RECIPM1 = 1,     // sqrt_recipm1_alphas_cumprod[t]
    BPD_COEF1 = 2,       // posterior_mean_coef1[t]
    BPD_COEF2 = 3,       // posterior_mean_coef2[t]
    BPD_POST_LOG = 4,    // posterior_log_variance_clipped[t]: the true log variance, the fixed model's, the learned one's min_log
    BPD_T0 = 5,          // 1 when t == 0 (the term is the decoder NLL), else 0 (the KL)
    BPD_SQRT_AC = 6,     // sqrt_alphas_cumprod[t]
    BPD_SQRT_1M_AC = 7,  // sqrt_one_minus_alphas_cumprod[t]
    BPD_MAX_LOG = 8,     // log(betas)[t]: the learned variance's max_log
    BPD_NCOLS = 16,
};
// elements of an image one workgroup of the term kernel sums: 256 threads x one dwordx4 (fixed, so that
// a partial sum, and with it a result, is the same for every batch and shard)
constexpr int BPD_CHUNK = 1024;
inline int bpd_chunks(int64_t per) { return (int)((per + BPD_CHUNK - 1) / BPD_CHUNK); }
// floats of scratch behind the term kernel: 3 * chunks * B doubles
inline size_t bpd_part_floats(int B, int64_t per) { return (size_t)6 * bpd_chunks(per) * B; }

// x_t = c[6] x0 + c[7] z (q_sample) with the row of st->step (STEP_ROW_STEP) or row 0 (STEP_ROW_FIRST, step_device.h); z = row `step` of noise (stride
// noise_step_stride), or the Philox draw step + 1 under st->seed when noise == nullptr.  n % 4 == 0, 16-byte pointers.
int launch_bpd_step_in(const float* x0, const float* noise, int64_t noise_step_stride, const float* tab, const SamplerState* st,
                       int row_mode, float* x_t, int64_t n, hipStream_t s);

// The three per-image means of one step from the model output (B, C | 2C with `learned`, H, W), x0, x_t and the same z:
//   rows[step][b] = [vb in bits, mean((pred_x_start - x0)^2), mean((eps(x_t, pred_x_start) - z)^2)]
// part: bpd_part_floats(B, per) floats, 8-byte aligned.  The second launch sums the partial sums in chunk order, writes the
// row and, with a state, advances st->step; `ticket` (one zeroed unsigned, null without a state) counts its workgroups.
// per % 4 == 0, 16-byte pointers, B <= 65535.
int launch_bpd_terms(const float* model_out, const float* x0, const float* x_t, const float* noise, int64_t noise_step_stride,
                     const float* tab, SamplerState* st, int learned, int objective, int clip, float* part, float* rows,
                     unsigned* ticket, int B, int64_t per, hipStream_t s);

// prior[b] = meanflat(normal_kl(sqrt_ac x0, logvar, 0, 0)) / ln 2, one workgroup per image, formed in double
int launch_bpd_prior(const float* x0, float sqrt_ac, float logvar, float* prior, int B, int64_t per, hipStream_t s);

}  // namespace dm
