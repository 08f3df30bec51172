// Learned-variance Gaussian diffusion kernels (gfx950): the reverse step of DD/learned_gaussian_diffusion.py:93-111 behind
// the base class's p_sample (DD/denoising_diffusion.py:638-645), and the hybrid loss of :113-146 with its gradient.
//
// The U-Net predicts 2C maps per image: the noise and a per-pixel weight v that interpolates between the two extreme
// posterior log-variances.  Both passes are bandwidth-bound: one dwordx4 load per tensor and thread, every schedule scalar
// from the host-built table (learned.h), an fp32 `extract` of the reference.  The step costs what a plain DDPM step costs
// plus one read of the variance half.  Contraction is off so the expression trees round like the reference's tensor ops;
// expf / logf / tanhf are the library functions, not the fast intrinsics.  Row lookup, 16-byte access, noise fetch, block
// reduction and the launch checks are those of step_device.h.
#include "learned.h"
#include "step_device.h"

namespace dm {

#pragma clang fp contract(off)

// out may alias x (each thread reads its 4 values before it writes them)
__global__ __launch_bounds__(256) void lv_step_kernel(const float* x, const float* __restrict__ eps2,
                                                      const float* __restrict__ noise, int64_t noise_step_stride, StepRows r,
                                                      float* out, float* __restrict__ all_steps,
                                                      float* __restrict__ final_out, float* __restrict__ mean_out,
                                                      float* __restrict__ logvar_out, float* __restrict__ x_start_out,
                                                      int64_t n) {
    const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = i4 * 4;
    if (i >= n) return;
    const float* c = step_row<LV_NCOLS>(r, i);
    const DdpmCoefs dc = ddpm_coefs(c);
    const float min_log = c[LV_MIN_LOG], max_log = c[LV_MAX_LOG];
    const bool noisy = c[LV_NOISE] != 0.0f;
    // image b's noise half starts at b * 2 per, its variance half at b * 2 per + per; per % 4 == 0 keeps the 4 elements
    // of a thread in one image
    const int64_t b = i / r.per, j = i - b * r.per;
    const float4 x4 = ld4(x, i), e4 = ld4(eps2, b * 2 * r.per + j), v4 = ld4(eps2, b * 2 * r.per + r.per + j);
    const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy) step_noise4(r, noise, noise_step_stride, i4, z);
    float o[4], mean[4], lv[4], xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lv[k] = lv_logvar(v[k], min_log, max_log);         // :97-101
        xs[k] = ddpm_x_start(dc, 0, xv[k], e[k]);          // :104-107: the first half is noise whatever `objective` says
        mean[k] = dc.c2 * xs[k] + dc.c3 * xv[k];           // q_posterior :109
        const float sd = expf(0.5f * lv[k]);
        o[k] = noisy ? mean[k] + sd * z[k] : mean[k] + sd * 0.0f;  // noise = 0. at t == 0 still meets a NaN / Inf sd
    }
    st4(out, i, make_float4(o[0], o[1], o[2], o[3]));
    if (mean_out) st4(mean_out, i, make_float4(mean[0], mean[1], mean[2], mean[3]));
    if (logvar_out) st4(logvar_out, i, make_float4(lv[0], lv[1], lv[2], lv[3]));
    if (x_start_out) st4(x_start_out, i, make_float4(xs[0], xs[1], xs[2], xs[3]));
    const int step = r.st ? r.st->step : 0;
    if (all_steps) st4(all_steps + (size_t)(step + 1) * n, i, make_float4(o[0], o[1], o[2], o[3]));
    if (final_out && (!r.st || step == r.st->n_steps - 1)) {
        if (r.st && r.st->unnormalize)
            st4(final_out, i, make_float4((o[0] + 1.0f) * 0.5f, (o[1] + 1.0f) * 0.5f, (o[2] + 1.0f) * 0.5f, (o[3] + 1.0f) * 0.5f));
        else
            st4(final_out, i, make_float4(o[0], o[1], o[2], o[3]));
    }
}

// One workgroup per image: the squared error of the noise half and the image's vb term (the branch its t selects), summed
// in double in a fixed order (no float atomics: block_sum256); dout in the same pass.
__global__ __launch_bounds__(256) void lv_loss_kernel(const float* __restrict__ out2, const float* __restrict__ x_start,
                                                      const float* __restrict__ noise, const float* __restrict__ x_t,
                                                      const float* __restrict__ tab, float vb_w, int clip,
                                                      float* __restrict__ dout, float* __restrict__ part,
                                                      float* __restrict__ mse_part, float* __restrict__ vb_part, int per,
                                                      int B, float loss_scale) {
    __shared__ double red[256];
    __shared__ double red2[256];
    const int b = blockIdx.x;
    const float* c = tab + (size_t)b * LVT_NCOLS;
    const float recip = c[LVT_RECIP], recipm1 = c[LVT_RECIPM1], coef1 = c[LVT_COEF1], coef2 = c[LVT_COEF2];
    const float min_log = c[LVT_MIN_LOG], true_log = c[LVT_TRUE_LOG], max_log = c[LVT_MAX_LOG];
    const bool t0 = c[LVT_T0] != 0.0f;
    const float nat = 1.4426950408889634f;  // NAT = 1 / ln 2 (:13)
    const float gscale = loss_scale * 2.0f / ((float)per * (float)B);
    // d loss / d v = loss_scale * w * (1 / B) * NAT * (1 / per) * d term / d logvar * d logvar / d v
    const float vscale = loss_scale * vb_w * nat / ((float)per * (float)B) * (0.5f * (max_log - min_log));
    const int64_t base = (int64_t)b * per, base2 = (int64_t)b * 2 * per;
    double s = 0.0, sv = 0.0;
    for (int i = threadIdx.x * 4; i < per; i += 256 * 4) {
        const float4 p4 = ld4(out2, base2 + i), v4 = ld4(out2, base2 + per + i), n4 = ld4(noise, base + i);
        const float4 a4 = ld4(x_start, base + i), q4 = ld4(x_t, base + i);
        const float p[4] = {p4.x, p4.y, p4.z, p4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w}, nz[4] = {n4.x, n4.y, n4.z, n4.w};
        const float xs[4] = {a4.x, a4.y, a4.z, a4.w}, xt[4] = {q4.x, q4.y, q4.z, q4.w};
        float g[4], gv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = p[k] - nz[k];  // F.mse_loss(pred_noise, noise) :142-144
            s += (double)d * d;
            g[k] = d * gscale;
            const float lv = lv_logvar(v[k], min_log, max_log);
            float x0 = recip * xt[k] - recipm1 * p[k];  // predict_start_from_noise :104
            if (clip) x0 = clamp1(x0);
            const float model_mean = coef1 * x0 + coef2 * xt[k];
            const float true_mean = coef1 * xs[k] + coef2 * xt[k];  // q_posterior :123
            float dlv;
            const float term = lv_vb_term(t0, xs[k], true_mean, true_log, model_mean, lv, &dlv);
            sv += (double)term;
            gv[k] = vscale * dlv;
        }
        st4(dout, base2 + i, make_float4(g[0], g[1], g[2], g[3]));
        st4(dout, base2 + per + i, make_float4(gv[0], gv[1], gv[2], gv[3]));
    }
    s = block_sum256(s, red);
    sv = block_sum256(sv, red2);
    if (threadIdx.x == 0) {
        const float m = (float)(s / per), vb = (float)(sv / per) * nat;  // meanflat(.) * NAT :131, :134
        mse_part[b] = m;
        vb_part[b] = vb;
        part[b] = m + vb * vb_w;
    }
}

#pragma clang fp contract(fast)

int launch_lv_step(const float* x, const float* eps2, const float* noise, int64_t noise_step_stride, const float* tab,
                   const SamplerState* st, int row_mode, int64_t per, float* out, float* all_steps, float* final_out, float* mean_out,
                   float* logvar_out, float* x_start_out, int64_t n, hipStream_t s) {
    DM_REQUIRE(x && eps2 && out, "lv_step: null tensor");
    if (vec4_ok("learned-variance", n, {x, eps2, noise, out, all_steps, final_out, mean_out, logvar_out, x_start_out})) return 1;
    DM_REQUIRE(per > 0 && per % 4 == 0 && n % per == 0, "lv_step: C*H*W must be a multiple of 4 that divides the element count");
    DM_REQUIRE(noise_step_stride % 4 == 0, "noise rows must keep 16-byte alignment");
    DM_REQUIRE(row_mode == STEP_ROW_STEP || row_mode == STEP_ROW_FIRST, "lv_step: the row is the step's, or the first");
    const StepRows r{tab, st, row_mode, per};
    if (rows_ok(r, n, "null step table")) return 1;
    hipLaunchKernelGGL(lv_step_kernel, grid4(n), dim3(256), 0, s, x, eps2, noise, noise_step_stride, r, out, all_steps, final_out,
                       mean_out, logvar_out, x_start_out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_lv_loss(const float* out2, const float* x_start, const float* noise, const float* x_t, const float* tab,
                   float vb_loss_weight, int clip, float* dout, float* part, float* mse_part, float* vb_part, float* loss,
                   int B, int64_t per, float loss_scale, hipStream_t s) {
    DM_REQUIRE(out2 && x_start && noise && x_t && tab && dout && part && mse_part && vb_part && loss && B > 0,
               "lv_loss: null tensor");
    DM_REQUIRE(per > 0 && per % 4 == 0 && per < (int64_t(1) << 30), "lv_loss: C*H*W must be a multiple of 4");
    if (vec4_ok("learned-variance", (int64_t)B * per, {out2, x_start, noise, x_t, dout})) return 1;
    hipLaunchKernelGGL(lv_loss_kernel, dim3(B), dim3(256), 0, s, out2, x_start, noise, x_t, tab, vb_loss_weight, clip ? 1 : 0,
                       dout, part, mse_part, vb_part, (int)per, B, loss_scale);
    DM_CHECK_HIP(hipGetLastError());
    return launch_loss_mean(part, B, loss, loss_scale, s);
}

}  // namespace dm
