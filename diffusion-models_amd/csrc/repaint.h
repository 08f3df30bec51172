// RePaint inpainting (arXiv 2201.09865 as DD/repaint.py:614-681 has it): launcher of repaint.hip.
#pragma once

#include "dm_common.h"

namespace dm {

// Columns of one row of the flattened loop (DM_REPAINT_COEFS floats, include/dm_hip.h); one row is one U-Net evaluation.
// Every value is a 0-dim fp32 tensor expression of the reference, computed by the host.
enum RepaintCol : int {
    RP_DDPM = 0,      // 0..7: the row of ddpm_step_table at the row's time (what sampler_update_kernel reads)
    RP_KNOWN_GT = 8,  // sqrt(alphas_cumprod[t]): weight of the normalised ground truth in the known region
    RP_KNOWN_Z = 9,   // sqrt(1 - alphas_cumprod[t]): weight of the known region's fresh noise
    RP_JUMP_X = 10,   // sqrt(1 - betas[resample_jump]) on a row that opens a resample iteration, else 1
    RP_JUMP_Z = 11,   // sqrt(betas[resample_jump]) on such a row, else 0
    RP_JUMP = 12,     // 1 on such a row, else 0: the forward jump is applied (and its noise drawn) in front of the row
    RP_SLOT = 13,     // frame of all_steps the row's result goes to, or -1
    RP_NCOLS = 16,
};
// What one launch does; AUTO resolves to LAST on row n_steps - 1 of the device state and to STEP_NEXT on every other row
enum RepaintMode : int { RP_AUTO = 0, RP_BLEND = 1, RP_STEP = 2, RP_STEP_NEXT = 3, RP_LAST = 4 };

// Philox draw ids of row r (draw 0 is x_T): the jump in front of the row, the row's known-region noise, its step noise
__host__ __device__ inline uint64_t repaint_draw_jump(uint64_t r) { return 3 * r + 1; }
__host__ __device__ inline uint64_t repaint_draw_known(uint64_t r) { return 3 * r + 2; }
__host__ __device__ inline uint64_t repaint_draw_step(uint64_t r) { return 3 * r + 3; }

struct RepaintNoise {
    // injected N(0,1) tensors of the row tab_base, each n floats; row k's are k * stride floats further on.
    // All nullptr: the Philox draws above under st->seed.
    const float* jump = nullptr;
    const float* known = nullptr;
    const float* step = nullptr;
    int64_t stride = 0;
};

// With r = st->step and c = tab + (r - tab_base) * RP_NCOLS, g = 2 gt - 1:
//   BLEND      out = mask (c[8] g + c[9] z_known(r)) + (1 - mask) x                            (eps is not read)
//   STEP       out = pred = the DDPM update of sampler_update_kernel (kind 0) with c[0..7] and z_step(r)
//   STEP_NEXT  pred as STEP; all_steps[c[13]] = pred; then with the NEXT row's c':
//              v = c'[12] ? c'[10] pred + c'[11] z_jump(r + 1) : pred;  out = mask (c'[8] g + c'[9] z_known(r + 1)) + (1 - mask) v
//   LAST       pred as STEP; v = mask g + (1 - mask) pred; all_steps[c[13]] = v;
//              final_out (out when it is nullptr) = st->unnormalize ? (v + 1) / 2 : v
// mask is (B, Cm, HW) with Cm == 1 (broadcast over the C = per / HW channels) or Cm == C; out may be x.  STEP needs neither
// gt nor mask.  all_steps, final_out and xstart_out (the clamped x_start of the update) are optional.
int launch_repaint_step(int mode, int objective, const float* x, const float* eps, RepaintNoise z, const float* tab,
                        int tab_base, const SamplerState* st, const float* gt, const float* mask, int Cm, int64_t per, int HW,
                        float* out, float* all_steps, float* final_out, float* xstart_out, int64_t n, hipStream_t s);

}  // namespace dm
