// Continuous-time Gaussian diffusion kernels (gfx950): the reverse step of DD/continuous_time_gaussian_diffusion.py:155-197
// and DD/v_param_continuous_time_gaussian_diffusion.py:72-113, and the training passes of :222-251 / :138-162 (q_sample with
// the regression target, the weighted loss with its gradient).
//
// Like the EDM passes they are bandwidth-bound: one dwordx4 load / store per tensor and thread, no schedule logic -- every
// scalar comes from the host-built table (ct.h), an fp32 tensor expression of the reference.  Contraction is off so the
// expression trees round like the reference's tensor ops.
#include "ct.h"
#include "philox.h"

#include <initializer_list>

namespace dm {

#pragma clang fp contract(off)

static __device__ __forceinline__ const float* ct_row(const EdmRows& r, int64_t i) {
    const int row = r.mode == EDM_ROW_IMAGE ? (int)(i / r.per) : (r.mode == EDM_ROW_STEP && r.st ? r.st->step : 0);
    return r.tab + (size_t)row * CT_NCOLS;
}
static __device__ __forceinline__ float4 ct_ld4(const float* p, int64_t i) { return *reinterpret_cast<const float4*>(p + i); }
static __device__ __forceinline__ void ct_st4(float* p, int64_t i, float4 v) { *reinterpret_cast<float4*>(p + i) = v; }
static __device__ __forceinline__ float ct_clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

// p_mean_variance + p_sample; out may alias x (each thread reads its 4 values before it writes them)
__global__ __launch_bounds__(256) void ct_step_kernel(const float* x, const float* __restrict__ F,
                                                      const float* __restrict__ noise, int64_t noise_step_stride, EdmRows r,
                                                      int objective, int clip, float* out, float* __restrict__ x_start_out,
                                                      int64_t n) {
    const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = i4 * 4;
    if (i >= n) return;
    const float* c = ct_row(r, i);
    const float alpha = c[CT_ALPHA], sigma = c[CT_SIGMA], alpha_next = c[CT_ALPHA_NEXT], cc = c[CT_C], omc = c[CT_ONE_M_C];
    const float sqrt_var = c[CT_SQRT_VAR], ratio = c[CT_AN_OVER_A], c_sigma = c[CT_C_SIGMA];
    const float4 x4 = ct_ld4(x, i), f4 = ct_ld4(F, i);
    const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w};
    float xs[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (objective == CT_PRED_NOISE && !clip) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ratio * (xv[j] - c_sigma * f[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xs[j] = objective == CT_PRED_V ? alpha * xv[j] - sigma * f[j] : (xv[j] - sigma * f[j]) / alpha;
            if (clip) xs[j] = ct_clamp1(xs[j]);
            o[j] = alpha_next * (xv[j] * omc / alpha + cc * xs[j]);
        }
        if (x_start_out) ct_st4(x_start_out, i, make_float4(xs[0], xs[1], xs[2], xs[3]));
    }
    if (sqrt_var != 0.0f) {
        const int step = r.st ? r.st->step : 0;
        float z[4];
        if (noise) {
            const float4 zv = ct_ld4(noise + (size_t)step * noise_step_stride, i);
            z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
        } else {
            philox_normal4(r.st ? r.st->seed : 0, (uint64_t)step + 1, (r.st ? r.st->off4 : 0) + (uint64_t)i4, z);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = o[j] + sqrt_var * z[j];
    }
    ct_st4(out, i, make_float4(o[0], o[1], o[2], o[3]));
}

// normalize_to_neg_one_to_one (forward; normalize == 0: img is x_start already), q_sample and the target of p_losses,
// per-image rows
__global__ __launch_bounds__(256) void ct_noise_in_kernel(const float* __restrict__ img, const float* __restrict__ eps,
                                                          EdmRows r, int objective, int normalize,
                                                          float* __restrict__ x, float* __restrict__ target, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = ct_row(r, i);
    const float alpha = c[CT_ALPHA], sigma = c[CT_SIGMA];
    const float4 im4 = ct_ld4(img, i), e4 = ct_ld4(eps, i);
    const float im[4] = {im4.x, im4.y, im4.z, im4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w};
    float xn[4], tg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = normalize ? im[j] * 2.0f - 1.0f : im[j];
        xn[j] = a * alpha + e[j] * sigma;
        tg[j] = objective == CT_PRED_V ? alpha * e[j] - sigma * a : e[j];
    }
    ct_st4(x, i, make_float4(xn[0], xn[1], xn[2], xn[3]));
    ct_st4(target, i, make_float4(tg[0], tg[1], tg[2], tg[3]));
}

// one workgroup per image: part[b] = w_b * mean((F - target)^2), the squares summed in double in a fixed order (no float
// atomics, as edm_loss_kernel); dF = d(loss) / dF in the same pass
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
        const float4 f4 = ct_ld4(F, base + i), t4 = ct_ld4(target, base + i);
        const float f[4] = {f4.x, f4.y, f4.z, f4.w}, t[4] = {t4.x, t4.y, t4.z, t4.w};
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = f[j] - t[j];
            s += (double)d * d;
            g[j] = d * gscale;
        }
        ct_st4(dF, base + i, make_float4(g[0], g[1], g[2], g[3]));
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[b] = (float)(red[0] / per) * w;
}
// losses.mean() times loss_scale; image order
__global__ void ct_loss_mean_kernel(const float* __restrict__ part, int B, float* __restrict__ loss, float loss_scale) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += part[b];
    *loss = (float)(s / B) * loss_scale;
}

#pragma clang fp contract(fast)

static bool ct_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
#define CT_VEC_OK(n, ...)                                                                                       \
    do {                                                                                                        \
        DM_REQUIRE((n) > 0 && (n) % 4 == 0, "continuous-time passes move 4 floats per thread: the element count must be a multiple of 4"); \
        for (const void* p_ : std::initializer_list<const void*>{__VA_ARGS__}) DM_REQUIRE(ct_aligned16(p_), "continuous-time passes need 16-byte aligned tensors"); \
    } while (0)
static int ct_rows_ok(const EdmRows& r, int64_t n) {
    DM_REQUIRE(r.tab != nullptr, "null coefficient table");
    DM_REQUIRE(r.mode != EDM_ROW_IMAGE || (r.per > 0 && r.per % 4 == 0 && n % r.per == 0),
               "per-image coefficients need C*H*W to be a multiple of 4 that divides the element count");
    return 0;
}
static dim3 ct_grid4(int64_t n) { return dim3((unsigned)((n / 4 + 255) / 256)); }

int launch_ct_step(const float* x, const float* F, const float* noise, int64_t noise_step_stride, EdmRows r, int objective,
                   int clip, float* out, float* x_start_out, int64_t n, hipStream_t s) {
    DM_REQUIRE(x && F && out, "ct_step: null tensor");
    DM_REQUIRE(objective == CT_PRED_NOISE || objective == CT_PRED_V, "ct_step: unknown objective");
    DM_REQUIRE(!(x_start_out && objective == CT_PRED_NOISE && !clip),
               "ct_step: noise prediction without clipping forms no x_start");
    CT_VEC_OK(n, x, F, noise, out, x_start_out);
    DM_REQUIRE(noise_step_stride % 4 == 0, "noise rows must keep 16-byte alignment");
    if (ct_rows_ok(r, n)) return 1;
    hipLaunchKernelGGL(ct_step_kernel, ct_grid4(n), dim3(256), 0, s, x, F, noise, noise_step_stride, r, objective, clip ? 1 : 0,
                       out, x_start_out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_ct_noise_in(const float* img, const float* eps, EdmRows r, int objective, int normalize, float* x, float* target,
                       int64_t n, hipStream_t s) {
    DM_REQUIRE(img && eps && x && target, "ct_noise_in: null tensor");
    DM_REQUIRE(objective == CT_PRED_NOISE || objective == CT_PRED_V, "ct_noise_in: unknown objective");
    CT_VEC_OK(n, img, eps, x, target);
    if (ct_rows_ok(r, n)) return 1;
    hipLaunchKernelGGL(ct_noise_in_kernel, ct_grid4(n), dim3(256), 0, s, img, eps, r, objective, normalize ? 1 : 0, x,
                       target, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_ct_loss(const float* F, const float* target, const float* tab, float* dF, float* part, float* loss, int B,
                   int64_t per, float loss_scale, hipStream_t s) {
    DM_REQUIRE(F && target && tab && dF && part && loss && B > 0, "ct_loss: null tensor");
    DM_REQUIRE(per > 0 && per % 4 == 0 && per < (int64_t(1) << 30), "ct_loss: C*H*W must be a multiple of 4");
    CT_VEC_OK((int64_t)B * per, F, target, dF);
    hipLaunchKernelGGL(ct_loss_kernel, dim3(B), dim3(256), 0, s, F, target, tab, dF, part, (int)per, B, loss_scale);
    DM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(ct_loss_mean_kernel, dim3(1), dim3(1), 0, s, part, B, loss, loss_scale);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dm
