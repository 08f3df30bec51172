// Continuous-time Gaussian diffusion kernels (gfx950): the reverse step of DD/continuous_time_gaussian_diffusion.py:155-197
// and DD/v_param_continuous_time_gaussian_diffusion.py:72-113, and the training passes of :222-251 / :138-162 (q_sample with
// the regression target, the weighted loss with its gradient).
//
// Like the EDM passes they are bandwidth-bound: one dwordx4 load / store per tensor and thread, no schedule logic -- every
// scalar comes from the host-built table (ct.h), an fp32 tensor expression of the reference.  Contraction is off so the
// expression trees round like the reference's tensor ops.  Row lookup, 16-byte access, noise fetch, block reduction and
// the launch checks are those of step_device.h.
#include "ct.h"

namespace dm {

#pragma clang fp contract(off)

// x_start of one element from the model output by objective (p_mean_variance of both classes), clamped when clip: the one
// formation the ancestral step and the DPM-Solver++ step share
static __device__ __forceinline__ float ct_x_start(int objective, int clip, float alpha, float sigma, float xv, float f) {
    const float xs = objective == CT_PRED_V ? alpha * xv - sigma * f : (xv - sigma * f) / alpha;
    return clip ? clamp1(xs) : xs;
}

// p_mean_variance + p_sample; out may alias x (each thread reads its 4 values before it writes them)
__global__ __launch_bounds__(256) void ct_step_kernel(const float* x, const float* __restrict__ F,
                                                      const float* __restrict__ noise, int64_t noise_step_stride, StepRows r,
                                                      int objective, int clip, float* out, float* __restrict__ x_start_out,
                                                      int64_t n) {
    const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = i4 * 4;
    if (i >= n) return;
    const float* c = step_row<CT_NCOLS>(r, i);
    const float alpha = c[CT_ALPHA], sigma = c[CT_SIGMA], alpha_next = c[CT_ALPHA_NEXT], cc = c[CT_C], omc = c[CT_ONE_M_C];
    const float sqrt_var = c[CT_SQRT_VAR], ratio = c[CT_AN_OVER_A], c_sigma = c[CT_C_SIGMA];
    const float4 x4 = ld4(x, i), f4 = ld4(F, i);
    const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w};
    float xs[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (objective == CT_PRED_NOISE && !clip) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ratio * (xv[j] - c_sigma * f[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xs[j] = ct_x_start(objective, clip, alpha, sigma, xv[j], f[j]);
            o[j] = alpha_next * (xv[j] * omc / alpha + cc * xs[j]);
        }
        if (x_start_out) st4(x_start_out, i, make_float4(xs[0], xs[1], xs[2], xs[3]));
    }
    if (sqrt_var != 0.0f) {
        float z[4];
        step_noise4(r, noise, noise_step_stride, i4, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = o[j] + sqrt_var * z[j];
    }
    st4(out, i, make_float4(o[0], o[1], o[2], o[3]));
}

// One DPM-Solver++ (2M) step (ct.h): hist holds the previous step's x_start and receives this step's; a thread reads and
// writes its own elements only, so out may alias x.  A thread's 4 elements share one row (per % 4 == 0): on a row with
// g == 0 (the first step, order 1) it never loads hist, which may be uninitialised memory there.
__global__ __launch_bounds__(256) void ct_dpmpp_step_kernel(const float* x, const float* __restrict__ F,
                                                            float* __restrict__ hist, StepRows r, int objective, int clip,
                                                            float* out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = step_row<CT_NCOLS>(r, i);
    const float alpha = c[CT_ALPHA], sigma = c[CT_SIGMA], c_x = c[CT_DPM_CX], c_d = c[CT_DPM_CD], g = c[CT_DPM_G];
    const float4 x4 = ld4(x, i), f4 = ld4(F, i);
    const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w};
    float xs[4], D[4], o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) D[j] = xs[j] = ct_x_start(objective, clip, alpha, sigma, xv[j], f[j]);
    if (g != 0.0f) {
        const float4 h4 = ld4(hist, i);
        const float h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) D[j] = xs[j] + g * (xs[j] - h[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = c_x * xv[j] + c_d * D[j];
    st4(hist, i, make_float4(xs[0], xs[1], xs[2], xs[3]));
    st4(out, i, make_float4(o[0], o[1], o[2], o[3]));
}

// normalize_to_neg_one_to_one (forward; normalize == 0: img is x_start already), q_sample and the target of p_losses,
// per-image rows
__global__ __launch_bounds__(256) void ct_noise_in_kernel(const float* __restrict__ img, const float* __restrict__ eps,
                                                          StepRows r, int objective, int normalize,
                                                          float* __restrict__ x, float* __restrict__ target, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = step_row<CT_NCOLS>(r, i);
    const float alpha = c[CT_ALPHA], sigma = c[CT_SIGMA];
    const float4 im4 = ld4(img, i), e4 = ld4(eps, i);
    const float im[4] = {im4.x, im4.y, im4.z, im4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w};
    float xn[4], tg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = normalize ? im[j] * 2.0f - 1.0f : im[j];
        xn[j] = a * alpha + e[j] * sigma;
        tg[j] = objective == CT_PRED_V ? alpha * e[j] - sigma * a : e[j];
    }
    st4(x, i, make_float4(xn[0], xn[1], xn[2], xn[3]));
    st4(target, i, make_float4(tg[0], tg[1], tg[2], tg[3]));
}

// one workgroup per image: part[b] = w_b * mean((F - target)^2), the squares summed in double in a fixed order (no float
// atomics: block_sum256); dF = d(loss) / dF in the same pass
__global__ __launch_bounds__(256) void ct_loss_kernel(const float* __restrict__ F, const float* __restrict__ target,
                                                      const float* __restrict__ tab, float* __restrict__ dF,
                                                      float* __restrict__ part, int per, int B, float loss_scale) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    const float w = tab[(size_t)b * CT_NCOLS + CT_LOSS_W];
    const float gscale = loss_scale * 2.0f * w / ((float)per * (float)B);
    const int64_t base = (int64_t)b * per;
    double s = 0.0;
    for (int i = threadIdx.x * 4; i < per; i += 256 * 4) {
        const float4 f4 = ld4(F, base + i), t4 = ld4(target, base + i);
        const float f[4] = {f4.x, f4.y, f4.z, f4.w}, t[4] = {t4.x, t4.y, t4.z, t4.w};
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = f[j] - t[j];
            s += (double)d * d;
            g[j] = d * gscale;
        }
        st4(dF, base + i, make_float4(g[0], g[1], g[2], g[3]));
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) part[b] = (float)(s / per) * w;
}

// What a schedule that is itself trained needs of one image, one workgroup per image, double sums in a fixed order
// (block_sum256): with x = alpha_b x0 + sigma_b eps,
//   out[b] = [ sum dX x0 | sum dX eps | dt[b] (0 without dt) | mean((F - target)^2) ]
// are dL/d alpha_b, dL/d sigma_b through the noised image, the U-Net's time gradient, and the unweighted per-image loss.
__global__ __launch_bounds__(256) void ct_sched_reduce_kernel(const float* __restrict__ dx, const float* __restrict__ img,
                                                              const float* __restrict__ eps, const float* __restrict__ F,
                                                              const float* __restrict__ target, const float* __restrict__ dt,
                                                              int normalize, float* __restrict__ out, int per) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    const int64_t base = (int64_t)b * per;
    double sa = 0.0, ss = 0.0, sl = 0.0;
    for (int i = threadIdx.x * 4; i < per; i += 256 * 4) {
        const float4 g4 = ld4(dx, base + i), im4 = ld4(img, base + i), e4 = ld4(eps, base + i);
        const float4 f4 = ld4(F, base + i), t4 = ld4(target, base + i);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w}, im[4] = {im4.x, im4.y, im4.z, im4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w};
        const float f[4] = {f4.x, f4.y, f4.z, f4.w}, t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = normalize ? im[j] * 2.0f - 1.0f : im[j];
            const float d = f[j] - t[j];
            sa += (double)g[j] * a;
            ss += (double)g[j] * e[j];
            sl += (double)d * d;
        }
    }
    sa = block_sum256(sa, red);
    __syncthreads();  // every thread has read red[0] before the next sum overwrites it
    ss = block_sum256(ss, red);
    __syncthreads();
    sl = block_sum256(sl, red);
    if (threadIdx.x == 0) {
        float* o = out + (size_t)b * 4;
        o[0] = (float)sa;
        o[1] = (float)ss;
        o[2] = dt ? dt[b] : 0.0f;
        o[3] = (float)(sl / per);
    }
}

#pragma clang fp contract(fast)

int launch_ct_sched_reduce(const float* dx, const float* img, const float* eps, const float* F, const float* target,
                           const float* dt, int normalize, float* out, int B, int64_t per, hipStream_t s) {
    DM_REQUIRE(dx && img && eps && F && target && out && B > 0, "ct_sched_reduce: null tensor");
    DM_REQUIRE(per > 0 && per % 4 == 0 && per < (int64_t(1) << 30), "ct_sched_reduce: C*H*W must be a multiple of 4");
    if (vec4_ok("continuous-time", (int64_t)B * per, {dx, img, eps, F, target})) return 1;
    hipLaunchKernelGGL(ct_sched_reduce_kernel, dim3(B), dim3(256), 0, s, dx, img, eps, F, target, dt, normalize ? 1 : 0, out,
                       (int)per);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_ct_step(const float* x, const float* F, const float* noise, int64_t noise_step_stride, StepRows r, int objective,
                   int clip, float* out, float* x_start_out, int64_t n, hipStream_t s) {
    DM_REQUIRE(x && F && out, "ct_step: null tensor");
    DM_REQUIRE(objective == CT_PRED_NOISE || objective == CT_PRED_V, "ct_step: unknown objective");
    DM_REQUIRE(!(x_start_out && objective == CT_PRED_NOISE && !clip),
               "ct_step: noise prediction without clipping forms no x_start");
    if (vec4_ok("continuous-time", n, {x, F, noise, out, x_start_out})) return 1;
    DM_REQUIRE(noise_step_stride % 4 == 0, "noise rows must keep 16-byte alignment");
    if (rows_ok(r, n, "null coefficient table")) return 1;
    hipLaunchKernelGGL(ct_step_kernel, grid4(n), dim3(256), 0, s, x, F, noise, noise_step_stride, r, objective, clip ? 1 : 0,
                       out, x_start_out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_ct_dpmpp_step(const float* x, const float* F, float* hist, StepRows r, int objective, int clip, float* out,
                         int64_t n, hipStream_t s) {
    DM_REQUIRE(x && F && hist && out, "ct_dpmpp_step: null tensor (the solver needs its history buffer)");
    DM_REQUIRE(objective == CT_PRED_NOISE || objective == CT_PRED_V, "ct_dpmpp_step: unknown objective");
    DM_REQUIRE(hist != x && hist != out && hist != F, "ct_dpmpp_step: the history buffer aliases another tensor");
    if (vec4_ok("continuous-time", n, {x, F, hist, out})) return 1;
    if (rows_ok(r, n, "null coefficient table")) return 1;
    hipLaunchKernelGGL(ct_dpmpp_step_kernel, grid4(n), dim3(256), 0, s, x, F, hist, r, objective, clip ? 1 : 0, out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_ct_noise_in(const float* img, const float* eps, StepRows r, int objective, int normalize, float* x, float* target,
                       int64_t n, hipStream_t s) {
    DM_REQUIRE(img && eps && x && target, "ct_noise_in: null tensor");
    DM_REQUIRE(objective == CT_PRED_NOISE || objective == CT_PRED_V, "ct_noise_in: unknown objective");
    if (vec4_ok("continuous-time", n, {img, eps, x, target})) return 1;
    if (rows_ok(r, n, "null coefficient table")) return 1;
    hipLaunchKernelGGL(ct_noise_in_kernel, grid4(n), dim3(256), 0, s, img, eps, r, objective, normalize ? 1 : 0, x,
                       target, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_ct_loss(const float* F, const float* target, const float* tab, float* dF, float* part, float* loss, int B,
                   int64_t per, float loss_scale, hipStream_t s) {
    DM_REQUIRE(F && target && tab && dF && part && loss && B > 0, "ct_loss: null tensor");
    DM_REQUIRE(per > 0 && per % 4 == 0 && per < (int64_t(1) << 30), "ct_loss: C*H*W must be a multiple of 4");
    if (vec4_ok("continuous-time", (int64_t)B * per, {F, target, dF})) return 1;
    hipLaunchKernelGGL(ct_loss_kernel, dim3(B), dim3(256), 0, s, F, target, tab, dF, part, (int)per, B, loss_scale);
    DM_CHECK_HIP(hipGetLastError());
    return launch_loss_mean(part, B, loss, loss_scale, s);  // losses.mean()
}

}  // namespace dm
