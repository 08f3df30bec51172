// ElucidatedDiffusion kernels (gfx950): the elementwise passes of the Heun and DPM-Solver++(2M) loops of
// DD/elucidated_diffusion.py:129-224, the real-valued time embedding their U-Net reads, and the training passes of :234-264
// (noise-in, weighted loss + its gradient, the backward of the learned embedding).
//
// The passes are bandwidth-bound: each thread moves 16 bytes per tensor (one dwordx4 load / store), reads every input
// once and holds no schedule logic -- every per-step scalar comes from the host-built step table (edm.h), rounded to
// fp32 where the reference rounds it.  Contraction is off so the expression trees round like the reference's tensor ops.
// Row lookup, 16-byte access, noise fetch, block reduction and the launch checks are those of step_device.h.
#include "edm.h"

namespace dm {

#pragma clang fp contract(off)

// RandomOrLearnedSinusoidalPosEmb / SinusoidalPosEmb on a float time (DD/denoising_diffusion.py:77-101)
__global__ void sinusoid_ft_kernel(const float* __restrict__ t, int t_stride, const SamplerState* __restrict__ st,
                                   const float* __restrict__ freqs, float* __restrict__ e, int R, int half, int learned) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * half) return;
    int r = i / half, k = i - r * half;
    const float tv = st ? t[(size_t)st->step * t_stride] : t[r];
    if (learned) {
        const float a = (tv * freqs[k]) * 6.283185307179586f;
        float* row = e + (size_t)r * (2 * half + 1);
        if (k == 0) row[0] = tv;
        row[1 + k] = sinf(a);
        row[1 + half + k] = cosf(a);
        return;
    }
    const float a = tv * freqs[k];
    e[(size_t)r * 2 * half + k] = sinf(a);
    e[(size_t)r * 2 * half + half + k] = cosf(a);
}

// :162-165 and the input scaling of :100
__global__ __launch_bounds__(256) void edm_churn_in_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                           int64_t noise_step_stride, StepRows r, float* __restrict__ xhat,
                                                           float* __restrict__ xin, int64_t n) {
    const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = i4 * 4;
    if (i >= n) return;
    const float* c = step_row<EDM_NCOLS>(r, i);
    const float churn = c[EDM_CHURN], s_noise = c[EDM_S_NOISE], c_in = c[EDM_C_IN];
    float4 xv = ld4(x, i);
    if (churn != 0.0f) {
        float z[4];
        step_noise4(r, noise, noise_step_stride, i4, z);
        xv.x = xv.x + churn * (s_noise * z[0]);
        xv.y = xv.y + churn * (s_noise * z[1]);
        xv.z = xv.z + churn * (s_noise * z[2]);
        xv.w = xv.w + churn * (s_noise * z[3]);
    }
    if (xhat) st4(xhat, i, xv);
    st4(xin, i, make_float4(c_in * xv.x, c_in * xv.y, c_in * xv.z, c_in * xv.w));
}

// :105-108 (preconditioned output), :170-172 (Euler step) and the input scaling of the second forward
__global__ __launch_bounds__(256) void edm_euler_kernel(const float* __restrict__ xhat, const float* __restrict__ F, StepRows r,
                                                        int clamp, float* __restrict__ D_out, float* __restrict__ d_out,
                                                        float* __restrict__ xnext, float* __restrict__ xin2, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = step_row<EDM_NCOLS>(r, i);
    const float c_skip = c[EDM_C_SKIP], c_out = c[EDM_C_OUT], sigma = c[EDM_SIGMA], dt = c[EDM_DT], c_in2 = c[EDM_C_IN2];
    const float4 xh4 = ld4(xhat, i), f4 = ld4(F, i);
    const float xh[4] = {xh4.x, xh4.y, xh4.z, xh4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w};
    float D[4], d[4], xn[4], xi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        D[j] = c_skip * xh[j] + c_out * f[j];
        if (clamp) D[j] = clamp1(D[j]);
        d[j] = (xh[j] - D[j]) / sigma;
        xn[j] = xh[j] + dt * d[j];
        xi[j] = c_in2 * xn[j];
    }
    if (D_out) st4(D_out, i, make_float4(D[0], D[1], D[2], D[3]));
    if (d_out) st4(d_out, i, make_float4(d[0], d[1], d[2], d[3]));
    if (xnext) st4(xnext, i, make_float4(xn[0], xn[1], xn[2], xn[3]));
    if (xin2) st4(xin2, i, make_float4(xi[0], xi[1], xi[2], xi[3]));
}

// :179-181 (second-order correction); out may alias xnext (each thread reads its 4 values before it writes them)
__global__ __launch_bounds__(256) void edm_heun_kernel(const float* __restrict__ xhat, const float* __restrict__ d,
                                                       const float* xnext, const float* __restrict__ F2, StepRows r, int clamp,
                                                       float* out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = step_row<EDM_NCOLS>(r, i);
    const float c_skip = c[EDM_C_SKIP2], c_out = c[EDM_C_OUT2], sigma = c[EDM_SIGMA2], half_dt = c[EDM_HALF_DT];
    const float4 xh4 = ld4(xhat, i), d4 = ld4(d, i), xn4 = ld4(xnext, i), f4 = ld4(F2, i);
    const float xh[4] = {xh4.x, xh4.y, xh4.z, xh4.w}, dv[4] = {d4.x, d4.y, d4.z, d4.w};
    const float xn[4] = {xn4.x, xn4.y, xn4.z, xn4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w};
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float D = c_skip * xn[j] + c_out * f[j];
        if (clamp) D = clamp1(D);
        const float d2 = (xn[j] - D) / sigma;
        o[j] = xh[j] + half_dt * (dv[j] + d2);
    }
    st4(out, i, make_float4(o[0], o[1], o[2], o[3]));
}

// :208-221; out may alias x
__global__ __launch_bounds__(256) void edm_dpmpp_kernel(const float* x, const float* __restrict__ F, float* __restrict__ d_old,
                                                        StepRows r, float* out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = step_row<EDM_NCOLS>(r, i);
    const float c_skip = c[EDM_C_SKIP], c_out = c[EDM_C_OUT], a = c[EDM_A], b = c[EDM_B], g = c[EDM_G], omg = c[EDM_OMG];
    const float4 x4 = ld4(x, i), f4 = ld4(F, i), o4 = ld4(d_old, i);
    const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w}, od[4] = {o4.x, o4.y, o4.z, o4.w};
    float D[4], o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        D[j] = c_skip * xv[j] + c_out * f[j];
        // g == 0 (first step, sigma_next == 0): denoised_d IS denoised in the reference
        const float dd = g != 0.0f ? omg * D[j] + g * od[j] : D[j];
        o[j] = a * xv[j] - b * dd;
    }
    st4(d_old, i, make_float4(D[0], D[1], D[2], D[3]));
    st4(out, i, make_float4(o[0], o[1], o[2], o[3]));
}

// :186-187 / :223-224
__global__ __launch_bounds__(256) void edm_finalize_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float4 v = ld4(x, i);
    st4(out, i, make_float4((clamp1(v.x) + 1.0f) * 0.5f, (clamp1(v.y) + 1.0f) * 0.5f, (clamp1(v.z) + 1.0f) * 0.5f,
                            (clamp1(v.w) + 1.0f) * 0.5f));
}

__global__ __launch_bounds__(256) void edm_scale_kernel(const float* __restrict__ x, float scale, float* __restrict__ out,
                                                        int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float4 v = ld4(x, i);
    st4(out, i, make_float4(scale * v.x, scale * v.y, scale * v.z, scale * v.w));
}

// ---- training (DD/elucidated_diffusion.py:234-264) ----------------------------------------------------------------
// :240 (normalize_to_neg_one_to_one), :247 (noised = images + sigma * noise) and the input scaling of :100, per-image rows
__global__ __launch_bounds__(256) void edm_noise_in_kernel(const float* __restrict__ img, const float* __restrict__ eps,
                                                           StepRows r, float* __restrict__ x0, float* __restrict__ noised,
                                                           float* __restrict__ xin, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = step_row<EDM_NCOLS>(r, i);
    const float sigma = c[EDM_SIGMA], c_in = c[EDM_C_IN];
    const float4 im4 = ld4(img, i), e4 = ld4(eps, i);
    const float im[4] = {im4.x, im4.y, im4.z, im4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w};
    float a[4], nz[4], xi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = im[j] * 2.0f - 1.0f;
        nz[j] = a[j] + sigma * e[j];
        xi[j] = c_in * nz[j];
    }
    st4(x0, i, make_float4(a[0], a[1], a[2], a[3]));
    st4(noised, i, make_float4(nz[0], nz[1], nz[2], nz[3]));
    st4(xin, i, make_float4(xi[0], xi[1], xi[2], xi[3]));
}

// :105 (D = c_skip noised + c_out F) and :259-262: one workgroup per image, part[b] = loss_weight_b * mean((D - x0)^2) with the
// squares summed in double in a fixed order (no float atomics: block_sum256, as mse_loss_kernel);  dF = d(loss) / dF in the same pass:
// loss_scale * loss_weight_b * c_out_b * 2 (D - x0) / (B * per)
__global__ __launch_bounds__(256) void edm_loss_kernel(const float* __restrict__ noised, const float* __restrict__ F,
                                                       const float* __restrict__ x0, const float* __restrict__ tab,
                                                       float* __restrict__ dF, float* __restrict__ D_out,
                                                       float* __restrict__ part, int per, int B, float loss_scale) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    const float* c = tab + (size_t)b * EDM_NCOLS;
    const float c_skip = c[EDM_C_SKIP], c_out = c[EDM_C_OUT], lw = c[EDM_LOSS_W];
    const float gscale = (loss_scale * 2.0f * lw / ((float)per * (float)B)) * c_out;
    const int64_t base = (int64_t)b * per;
    double s = 0.0;
    for (int i = threadIdx.x * 4; i < per; i += 256 * 4) {
        const float4 n4 = ld4(noised, base + i), f4 = ld4(F, base + i), a4 = ld4(x0, base + i);
        const float nz[4] = {n4.x, n4.y, n4.z, n4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w}, a[4] = {a4.x, a4.y, a4.z, a4.w};
        float D[4], g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            D[j] = c_skip * nz[j] + c_out * f[j];
            const float d = D[j] - a[j];
            s += (double)d * d;
            g[j] = d * gscale;
        }
        st4(dF, base + i, make_float4(g[0], g[1], g[2], g[3]));
        if (D_out) st4(D_out, base + i, make_float4(D[0], D[1], D[2], D[3]));
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) part[b] = (float)(s / per) * lw;
}

// Backward of RandomOrLearnedSinusoidalPosEmb (DD/denoising_diffusion.py:96-101) with respect to its `weights`, from the
// taped rows e0[b] = [t_b | sin_b | cos_b] -- no trigonometric function is evaluated again:
//   dW[k] (+)= sum_b (de_sin[b][k] cos[b][k] - de_cos[b][k] sin[b][k]) * 2 pi * t_b,   b in order (one thread per k).
// learned == 0 (random_fourier_features: requires_grad = False): the slot is exact zeros.
__global__ void sinusoid_ft_bwd_kernel(const float* __restrict__ de0, const float* __restrict__ e0, float* __restrict__ dw, int B,
                                       int half, int learned, int accumulate) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= half) return;
    if (!learned) {
        dw[k] = 0.0f;
        return;
    }
    const int wdt = 2 * half + 1;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* e = e0 + (size_t)b * wdt;
        const float* d = de0 + (size_t)b * wdt;
        const float da = d[1 + k] * e[1 + half + k] - d[1 + half + k] * e[1 + k];
        s += (double)((da * 6.283185307179586f) * e[0]);
    }
    dw[k] = accumulate ? dw[k] + (float)s : (float)s;
}

// The same module with respect to its input t (:98-100: freqs = t w 2 pi; cat(t, sin, cos)), from the same taped rows:
//   dt[b] = de0[b][0] + 2 pi sum_k w_k (de_sin[b][k] cos[b][k] - de_cos[b][k] sin[b][k]),   k in order, in double
// (one thread per image).  It does not ask whether `weights` is trainable: a frozen embedding still passes the gradient on.
__global__ void sinusoid_ft_tgrad_kernel(const float* __restrict__ de0, const float* __restrict__ e0,
                                         const float* __restrict__ freqs, float* __restrict__ dt, int B, int half) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int wdt = 2 * half + 1;
    const float* e = e0 + (size_t)b * wdt;
    const float* d = de0 + (size_t)b * wdt;
    double s = 0.0;
    for (int k = 0; k < half; ++k)
        s += (double)freqs[k] * ((double)d[1 + k] * (double)e[1 + half + k] - (double)d[1 + half + k] * (double)e[1 + k]);
    dt[b] = (float)((double)d[0] + 6.283185307179586 * s);
}

#pragma clang fp contract(fast)

int launch_sinusoid_ft(const float* t, int t_stride, const SamplerState* st, const float* freqs, float* e, int R, int half,
                       hipStream_t s, bool learned) {
    const int n = R * half;
    hipLaunchKernelGGL(sinusoid_ft_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t, t_stride, st, freqs, e, R, half,
                       learned ? 1 : 0);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_churn_in(const float* x, const float* noise, int64_t noise_step_stride, StepRows r, float* xhat, float* xin,
                        int64_t n, hipStream_t s) {
    if (vec4_ok("EDM", n, {x, noise, xhat, xin})) return 1;
    DM_REQUIRE(noise_step_stride % 4 == 0, "noise rows must keep 16-byte alignment");
    if (rows_ok(r, n, "null step table")) return 1;
    hipLaunchKernelGGL(edm_churn_in_kernel, grid4(n), dim3(256), 0, s, x, noise, noise_step_stride, r, xhat, xin, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_euler(const float* xhat, const float* F, StepRows r, int clamp, float* D_out, float* d_out, float* xnext,
                     float* xin2, int64_t n, hipStream_t s) {
    if (vec4_ok("EDM", n, {xhat, F, D_out, d_out, xnext, xin2})) return 1;
    if (rows_ok(r, n, "null step table")) return 1;
    hipLaunchKernelGGL(edm_euler_kernel, grid4(n), dim3(256), 0, s, xhat, F, r, clamp, D_out, d_out, xnext, xin2, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_heun(const float* xhat, const float* d, const float* xnext, const float* F2, StepRows r, int clamp, float* out,
                    int64_t n, hipStream_t s) {
    if (vec4_ok("EDM", n, {xhat, d, xnext, F2, out})) return 1;
    if (rows_ok(r, n, "null step table")) return 1;
    hipLaunchKernelGGL(edm_heun_kernel, grid4(n), dim3(256), 0, s, xhat, d, xnext, F2, r, clamp, out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_dpmpp(const float* x, const float* F, float* d_old, StepRows r, float* out, int64_t n, hipStream_t s) {
    if (vec4_ok("EDM", n, {x, F, d_old, out})) return 1;
    if (rows_ok(r, n, "null step table")) return 1;
    hipLaunchKernelGGL(edm_dpmpp_kernel, grid4(n), dim3(256), 0, s, x, F, d_old, r, out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_finalize(const float* x, float* out, int64_t n, hipStream_t s) {
    if (vec4_ok("EDM", n, {x, out})) return 1;
    hipLaunchKernelGGL(edm_finalize_kernel, grid4(n), dim3(256), 0, s, x, out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_scale(const float* x, float scale, float* out, int64_t n, hipStream_t s) {
    if (vec4_ok("EDM", n, {x, out})) return 1;
    hipLaunchKernelGGL(edm_scale_kernel, grid4(n), dim3(256), 0, s, x, scale, out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_noise_in(const float* img, const float* eps, StepRows r, float* x0, float* noised, float* xin, int64_t n,
                        hipStream_t s) {
    DM_REQUIRE(img && eps && x0 && noised && xin, "edm_noise_in: null tensor");
    if (vec4_ok("EDM", n, {img, eps, x0, noised, xin})) return 1;
    if (rows_ok(r, n, "null step table")) return 1;
    hipLaunchKernelGGL(edm_noise_in_kernel, grid4(n), dim3(256), 0, s, img, eps, r, x0, noised, xin, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_loss(const float* noised, const float* F, const float* x0, const float* tab, float* dF, float* D_out, float* part,
                    float* loss, int B, int64_t per, float loss_scale, hipStream_t s) {
    DM_REQUIRE(noised && F && x0 && tab && dF && part && loss && B > 0, "edm_loss: null tensor");
    DM_REQUIRE(per > 0 && per % 4 == 0 && per < (int64_t(1) << 30), "edm_loss: C*H*W must be a multiple of 4");
    if (vec4_ok("EDM", (int64_t)B * per, {noised, F, x0, dF, D_out})) return 1;
    hipLaunchKernelGGL(edm_loss_kernel, dim3(B), dim3(256), 0, s, noised, F, x0, tab, dF, D_out, part, (int)per, B, loss_scale);
    DM_CHECK_HIP(hipGetLastError());
    return launch_loss_mean(part, B, loss, loss_scale, s);  // :264 (losses.mean())
}

int launch_sinusoid_ft_bwd(const float* de0, const float* e0, float* dw, int B, int half, bool learned, int accumulate,
                           hipStream_t s) {
    DM_REQUIRE(de0 && e0 && dw && B > 0 && half > 0, "sinusoid_ft_bwd: bad argument");
    hipLaunchKernelGGL(sinusoid_ft_bwd_kernel, dim3((half + 63) / 64), dim3(64), 0, s, de0, e0, dw, B, half, learned ? 1 : 0,
                       accumulate ? 1 : 0);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_sinusoid_ft_tgrad(const float* de0, const float* e0, const float* freqs, float* dt, int B, int half, hipStream_t s) {
    DM_REQUIRE(de0 && e0 && freqs && dt && B > 0 && half > 0, "sinusoid_ft_tgrad: bad argument");
    hipLaunchKernelGGL(sinusoid_ft_tgrad_kernel, dim3((B + 63) / 64), dim3(64), 0, s, de0, e0, freqs, dt, B, half);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dm
