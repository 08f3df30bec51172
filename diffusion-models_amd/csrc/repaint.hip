// RePaint inpainting kernel (gfx950): one launch per row of the flattened loop of DD/repaint.py:614-681.
//
// A row is one U-Net evaluation.  What the reference does around it -- the known-region blend in front of the model call
// (:619-628), the DDPM update behind it (:630-636), the forward jump that opens a resample iteration (:672-674) and the
// ground-truth paste at t == 0 (:638-640) -- is elementwise, so the update of row r and the jump and blend in front of row
// r + 1 are one pass over the image: a masked row costs the launches of a plain DDPM step and adds the reads of gt and mask.
// Bandwidth-bound like sampler_update_kernel, whose update it shares (ddpm_update, step_device.h); 4 elements per thread
// share one Philox counter.  Contraction is off so the expression trees round like the reference's tensor ops.
#include "repaint.h"
#include "step_device.h"

namespace dm {

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void repaint_step_kernel(int mode, int objective, const float* x,
                                                           const float* __restrict__ eps, RepaintNoise zin,
                                                           const float* __restrict__ tab, int tab_base,
                                                           const SamplerState* __restrict__ st,
                                                           const float* __restrict__ gt, const float* __restrict__ mask,
                                                           int Cm, int64_t per, int HW, float* out,
                                                           float* __restrict__ all_steps, float* __restrict__ final_out,
                                                           float* __restrict__ xstart_out, int64_t n) {
    // everything that changes between two calls of one shape comes from the device-side state and tables, so one captured
    // graph serves every row of every call
    const int row = st->step;
    const uint64_t seed = st->seed, off4 = st->off4;
    if (mode == RP_AUTO) mode = row == st->n_steps - 1 ? RP_LAST : RP_STEP_NEXT;
    const bool do_step = mode != RP_BLEND;
    const bool do_blend = mode == RP_BLEND || mode == RP_STEP_NEXT;
    const int brow = mode == RP_BLEND ? row : row + 1;  // the row whose model call the blend prepares
    const float* c = tab + (size_t)(row - tab_base) * RP_NCOLS;
    const float* cb = tab + (size_t)(do_blend ? brow - tab_base : row - tab_base) * RP_NCOLS;
    const DdpmCoefs dc = ddpm_coefs(c);
    const bool step_noise = do_step && c[5] != 0.0f;
    const int slot = (int)c[RP_SLOT];
    const float kg = cb[RP_KNOWN_GT], kz = cb[RP_KNOWN_Z], jx = cb[RP_JUMP_X], jz = cb[RP_JUMP_Z];
    const bool do_jump = mode == RP_STEP_NEXT && cb[RP_JUMP] != 0.0f;
    const bool philox = zin.known == nullptr && zin.step == nullptr && zin.jump == nullptr;

    const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i4 * 4 >= n) return;
    float zs[4] = {0.f, 0.f, 0.f, 0.f}, zj[4] = {0.f, 0.f, 0.f, 0.f}, zk[4] = {0.f, 0.f, 0.f, 0.f};
    if (philox) {
        if (step_noise && dc.c4 != 0.0f) philox_normal4(seed, repaint_draw_step((uint64_t)row), off4 + (uint64_t)i4, zs);
        if (do_jump) philox_normal4(seed, repaint_draw_jump((uint64_t)brow), off4 + (uint64_t)i4, zj);
        if (do_blend) philox_normal4(seed, repaint_draw_known((uint64_t)brow), off4 + (uint64_t)i4, zk);
    } else {
        // a row's tensors are addressed only where the row reads them: on the last row there is no row + 1
        const float* ps = step_noise ? zin.step + (size_t)(row - tab_base) * zin.stride : nullptr;
        const float* pj = do_jump ? zin.jump + (size_t)(brow - tab_base) * zin.stride : nullptr;
        const float* pk = do_blend ? zin.known + (size_t)(brow - tab_base) * zin.stride : nullptr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = i4 * 4 + j;
            if (i >= n) break;
            if (ps) zs[j] = ps[i];
            if (pj) zj[j] = pj[i];
            if (pk) zk[j] = pk[i];
        }
    }
    // the mask is (B, Cm, HW): the element's own value, or its pixel's in the image's single plane.  The thread's four
    // elements are consecutive, so one division finds the first one's image and pixel and the others follow by counting.
    int64_t mi[4] = {i4 * 4, i4 * 4 + 1, i4 * 4 + 2, i4 * 4 + 3};
    if (Cm == 1 && mode != RP_STEP) {
        const int64_t b = (i4 * 4) / per;
        uint32_t rem = (uint32_t)(i4 * 4 - b * per), p = rem % (uint32_t)HW;  // per < 2^31 (launch_repaint_step)
        int64_t base = b * HW;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mi[j] = base + p;
            if (++p == (uint32_t)HW) p = 0;
            if (++rem == (uint32_t)per) {
                rem = 0;
                base += HW;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = i4 * 4 + j;
        if (i >= n) break;
        float v = x[i];
        if (do_step) {
            // :630-636: model_predictions :546-568 / :591-593, q_posterior :570-574, noise = 0. at t == 0
            const float x0 = ddpm_x_start(dc, objective, v, eps[i]);
            if (xstart_out) xstart_out[i] = x0;
            v = ddpm_update(dc, x0, v, step_noise, zs[j]);
        }
        if (mode == RP_STEP) {
            out[i] = v;
            continue;
        }
        const float m = mask[mi[j]];
        const float g = gt[i] * 2.0f - 1.0f;  // normalize_to_neg_one_to_one, whatever auto_normalize is :621
        if (mode == RP_LAST) {
            v = (m * g) + ((1.0f - m) * v);  // :638-640
            if (all_steps && slot >= 0) all_steps[(size_t)slot * n + i] = v;
            (final_out ? final_out : out)[i] = st->unnormalize ? (v + 1.0f) * 0.5f : v;  // unnormalize :680
            continue;
        }
        if (mode == RP_STEP_NEXT && all_steps && slot >= 0) all_steps[(size_t)slot * n + i] = v;  // p_sample's return value
        if (do_jump) v = jx * v + jz * zj[j];                                                  // :673-674
        const float weighed_gt = kg * g + kz * zk[j];                                          // :622-627
        out[i] = (m * weighed_gt) + ((1.0f - m) * v);                                          // :628
    }
}

#pragma clang fp contract(fast)

int launch_repaint_step(int mode, int objective, const float* x, const float* eps, RepaintNoise z, const float* tab,
                        int tab_base, const SamplerState* st, const float* gt, const float* mask, int Cm, int64_t per, int HW,
                        float* out, float* all_steps, float* final_out, float* xstart_out, int64_t n, hipStream_t s) {
    DM_REQUIRE(mode >= RP_AUTO && mode <= RP_LAST, "repaint_step: unknown mode");
    DM_REQUIRE(objective >= 0 && objective <= 2, "repaint_step: unknown objective");
    DM_REQUIRE(x && tab && st && out && n > 0, "repaint_step: null tensor");
    DM_REQUIRE(eps || mode == RP_BLEND, "repaint_step: every mode but the blend reads the model output");
    DM_REQUIRE(mode == RP_STEP || (gt && mask), "repaint_step: gt and mask are needed by every mode but the plain step");
    DM_REQUIRE(HW > 0 && per > 0 && per % HW == 0 && n % per == 0, "repaint_step: n = B * per, per = C * HW");
    DM_REQUIRE(per < (int64_t(1) << 31), "repaint_step: C * HW must be below 2^31");
    DM_REQUIRE(mode == RP_STEP || Cm == 1 || Cm == per / HW, "repaint_step: the mask has 1 or C channels");
    const bool any = z.jump || z.known || z.step;
    DM_REQUIRE(!any || (z.jump && z.known && z.step), "repaint_step: injected noise comes as jump, known and step together");
    const int64_t n4 = (n + 3) / 4;
    hipLaunchKernelGGL(repaint_step_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, mode, objective, x, eps, z,
                       tab, tab_base, st, gt, mask, Cm, per, HW, out, all_steps, final_out, xstart_out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dm
