// Classifier-guided DDPM sampling kernels (gfx950): the reverse step of DD/guided_diffusion.py:573-584 cut in two around
// the host's cond_fn (:553-569).  cg_mean_kernel leaves the posterior mean where cond_fn reads it; cg_finish_kernel shifts
// it by posterior_variance * gradient and adds the noise.
//
// Both passes are bandwidth-bound: one dwordx4 load per tensor and thread, every schedule scalar from the host-built
// table (cguide.h), no LDS, no atomics.  Together they cost what the plain DDPM update costs plus one write and one read
// of the mean and one read of the gradient.  Contraction is off so the expression trees round like the reference's tensor
// ops: with a zero gradient the pair reproduces sampler_update_kernel's result.  Row lookup, 16-byte access, noise fetch
// and the launch checks are those of step_device.h.
#include "cguide.h"
#include "step_device.h"

namespace dm {

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void cg_mean_kernel(const float* __restrict__ x, const float* __restrict__ model_out,
                                                      StepRows r, int objective, float* __restrict__ mean,
                                                      float* __restrict__ x_start_out, int64_t n) {
    const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = i4 * 4;
    if (i >= n) return;
    const float* c = step_row<CG_NCOLS>(r, i);
    const DdpmCoefs dc = ddpm_coefs(c);
    const float4 x4 = ld4(x, i), e4 = ld4(model_out, i);
    const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w};
    float m[4], xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xs[k] = ddpm_x_start(dc, objective, xv[k], e[k]);  // model_predictions + clamp_ :544-548
        m[k] = dc.c2 * xs[k] + dc.c3 * xv[k];              // q_posterior :513-516
    }
    st4(mean, i, make_float4(m[0], m[1], m[2], m[3]));
    if (x_start_out) st4(x_start_out, i, make_float4(xs[0], xs[1], xs[2], xs[3]));
}

// out may alias mean or grad (each thread reads its 4 values before it writes them)
__global__ __launch_bounds__(256) void cg_finish_kernel(const float* mean, const float* grad, const float* __restrict__ noise,
                                                        int64_t noise_step_stride, StepRows r, float* out,
                                                        float* __restrict__ all_steps, float* __restrict__ final_out,
                                                        float* __restrict__ guided_out, int64_t n) {
    const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = i4 * 4;
    if (i >= n) return;
    const float* c = step_row<CG_NCOLS>(r, i);
    const float sigma = c[CG_SIGMA], var = c[CG_VARIANCE];
    const bool noisy = c[CG_NOISE] != 0.0f;
    const float4 m4 = ld4(mean, i), g4 = ld4(grad, i);
    const float mv[4] = {m4.x, m4.y, m4.z, m4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w};
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy) step_noise4(r, noise, noise_step_stride, i4, z);
    float o[4], m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m[k] = mv[k] + var * g[k];                                    // condition_mean :565-567
        o[k] = noisy ? m[k] + sigma * z[k] : m[k] + sigma * 0.0f;     // noise = 0. at t == 0 still meets a NaN / Inf sigma
    }
    st4(out, i, make_float4(o[0], o[1], o[2], o[3]));
    if (guided_out) st4(guided_out, i, make_float4(m[0], m[1], m[2], m[3]));
    const int step = r.st ? r.st->step : 0;
    if (all_steps) st4(all_steps + (size_t)(step + 1) * n, i, make_float4(o[0], o[1], o[2], o[3]));
    if (final_out && (!r.st || step == r.st->n_steps - 1)) {
        if (r.st && r.st->unnormalize)
            st4(final_out, i, make_float4((o[0] + 1.0f) * 0.5f, (o[1] + 1.0f) * 0.5f, (o[2] + 1.0f) * 0.5f, (o[3] + 1.0f) * 0.5f));
        else
            st4(final_out, i, make_float4(o[0], o[1], o[2], o[3]));
    }
}

#pragma clang fp contract(fast)

int launch_cg_mean(const float* x, const float* model_out, const float* tab, const SamplerState* st, int row_mode, int64_t per,
                   int objective, float* mean, float* x_start_out, int64_t n, hipStream_t s) {
    DM_REQUIRE(x && model_out && mean, "cg_mean: null tensor");
    DM_REQUIRE(objective >= 0 && objective <= 2, "cg_mean: unknown objective");
    if (vec4_ok("classifier-guidance", n, {x, model_out, mean, x_start_out})) return 1;
    DM_REQUIRE(per > 0 && per % 4 == 0 && n % per == 0, "cg_mean: C*H*W must be a multiple of 4 that divides the element count");
    DM_REQUIRE(row_mode == STEP_ROW_STEP || row_mode == STEP_ROW_FIRST, "cg_mean: the row is the step's, or the first");
    DM_REQUIRE(mean != x && mean != model_out && (!x_start_out || (x_start_out != x && x_start_out != model_out && x_start_out != mean)),
               "cg_mean: the outputs do not alias the inputs or each other");
    const StepRows r{tab, st, row_mode, per};
    if (rows_ok(r, n, "null step table")) return 1;
    hipLaunchKernelGGL(cg_mean_kernel, grid4(n), dim3(256), 0, s, x, model_out, r, objective, mean, x_start_out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_cg_finish(const float* mean, const float* grad, const float* noise, int64_t noise_step_stride, const float* tab,
                     const SamplerState* st, int row_mode, int64_t per, float* out, float* all_steps, float* final_out,
                     float* guided_out, int64_t n, hipStream_t s) {
    DM_REQUIRE(mean && grad && out, "cg_finish: null tensor");
    if (vec4_ok("classifier-guidance", n, {mean, grad, noise, out, all_steps, final_out, guided_out})) return 1;
    DM_REQUIRE(per > 0 && per % 4 == 0 && n % per == 0, "cg_finish: C*H*W must be a multiple of 4 that divides the element count");
    DM_REQUIRE(noise_step_stride % 4 == 0, "noise rows must keep 16-byte alignment");
    DM_REQUIRE(row_mode == STEP_ROW_STEP || row_mode == STEP_ROW_FIRST, "cg_finish: the row is the step's, or the first");
    const StepRows r{tab, st, row_mode, per};
    if (rows_ok(r, n, "null step table")) return 1;
    hipLaunchKernelGGL(cg_finish_kernel, grid4(n), dim3(256), 0, s, mean, grad, noise, noise_step_stride, r, out, all_steps,
                       final_out, guided_out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dm
