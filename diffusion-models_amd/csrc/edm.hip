// ElucidatedDiffusion sampling kernels (gfx950): the elementwise passes of the Heun and DPM-Solver++(2M) loops of
// DD/elucidated_diffusion.py:129-224 and the real-valued time embedding their U-Net reads.
//
// The passes are bandwidth-bound: each thread moves 16 bytes per tensor (one dwordx4 load / store), reads every input
// once and holds no schedule logic -- every per-step scalar comes from the host-built step table (edm.h), rounded to
// fp32 where the reference rounds it.  Contraction is off so the expression trees round like the reference's tensor ops.
#include "edm.h"
#include "philox.h"

#include <initializer_list>

namespace dm {

#pragma clang fp contract(off)

__device__ __forceinline__ const float* edm_row(const EdmRows& r, int64_t i) {
    const int row = r.mode == EDM_ROW_IMAGE ? (int)(i / r.per) : (r.mode == EDM_ROW_STEP && r.st ? r.st->step : 0);
    return r.tab + (size_t)row * EDM_NCOLS;
}
__device__ __forceinline__ float4 ld4(const float* p, int64_t i) { return *reinterpret_cast<const float4*>(p + i); }
__device__ __forceinline__ void st4(float* p, int64_t i, float4 v) { *reinterpret_cast<float4*>(p + i) = v; }
__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

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
                                                           int64_t noise_step_stride, EdmRows r, float* __restrict__ xhat,
                                                           float* __restrict__ xin, int64_t n) {
    const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = i4 * 4;
    if (i >= n) return;
    const float* c = edm_row(r, i);
    const float churn = c[EDM_CHURN], s_noise = c[EDM_S_NOISE], c_in = c[EDM_C_IN];
    float4 xv = ld4(x, i);
    if (churn != 0.0f) {
        const int step = r.st ? r.st->step : 0;
        float z[4];
        if (noise) {
            const float4 zv = ld4(noise + (size_t)step * noise_step_stride, i);
            z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
        } else {
            philox_normal4(r.st ? r.st->seed : 0, (uint64_t)step + 1, (r.st ? r.st->off4 : 0) + (uint64_t)i4, z);
        }
        xv.x = xv.x + churn * (s_noise * z[0]);
        xv.y = xv.y + churn * (s_noise * z[1]);
        xv.z = xv.z + churn * (s_noise * z[2]);
        xv.w = xv.w + churn * (s_noise * z[3]);
    }
    if (xhat) st4(xhat, i, xv);
    st4(xin, i, make_float4(c_in * xv.x, c_in * xv.y, c_in * xv.z, c_in * xv.w));
}

// :105-108 (preconditioned output), :170-172 (Euler step) and the input scaling of the second forward
__global__ __launch_bounds__(256) void edm_euler_kernel(const float* __restrict__ xhat, const float* __restrict__ F, EdmRows r,
                                                        int clamp, float* __restrict__ D_out, float* __restrict__ d_out,
                                                        float* __restrict__ xnext, float* __restrict__ xin2, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = edm_row(r, i);
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
                                                       const float* xnext, const float* __restrict__ F2, EdmRows r, int clamp,
                                                       float* out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = edm_row(r, i);
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
                                                        EdmRows r, float* out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = edm_row(r, i);
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

#pragma clang fp contract(fast)

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
#define EDM_VEC_OK(n, ...)                                                                                      \
    do {                                                                                                        \
        DM_REQUIRE((n) > 0 && (n) % 4 == 0, "EDM passes move 4 floats per thread: the element count must be a multiple of 4"); \
        for (const void* p_ : std::initializer_list<const void*>{__VA_ARGS__}) DM_REQUIRE(aligned16(p_), "EDM passes need 16-byte aligned tensors"); \
    } while (0)
static int rows_ok(const EdmRows& r, int64_t n) {
    DM_REQUIRE(r.tab != nullptr, "null step table");
    DM_REQUIRE(r.mode != EDM_ROW_IMAGE || (r.per > 0 && r.per % 4 == 0 && n % r.per == 0),
               "per-image coefficients need C*H*W to be a multiple of 4 that divides the element count");
    return 0;
}
static dim3 grid4(int64_t n) { return dim3((unsigned)((n / 4 + 255) / 256)); }

int launch_sinusoid_ft(const float* t, int t_stride, const SamplerState* st, const float* freqs, float* e, int R, int half,
                       hipStream_t s, bool learned) {
    const int n = R * half;
    hipLaunchKernelGGL(sinusoid_ft_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t, t_stride, st, freqs, e, R, half,
                       learned ? 1 : 0);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_churn_in(const float* x, const float* noise, int64_t noise_step_stride, EdmRows r, float* xhat, float* xin,
                        int64_t n, hipStream_t s) {
    EDM_VEC_OK(n, x, noise, xhat, xin);
    DM_REQUIRE(noise_step_stride % 4 == 0, "noise rows must keep 16-byte alignment");
    if (rows_ok(r, n)) return 1;
    hipLaunchKernelGGL(edm_churn_in_kernel, grid4(n), dim3(256), 0, s, x, noise, noise_step_stride, r, xhat, xin, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_euler(const float* xhat, const float* F, EdmRows r, int clamp, float* D_out, float* d_out, float* xnext,
                     float* xin2, int64_t n, hipStream_t s) {
    EDM_VEC_OK(n, xhat, F, D_out, d_out, xnext, xin2);
    if (rows_ok(r, n)) return 1;
    hipLaunchKernelGGL(edm_euler_kernel, grid4(n), dim3(256), 0, s, xhat, F, r, clamp, D_out, d_out, xnext, xin2, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_heun(const float* xhat, const float* d, const float* xnext, const float* F2, EdmRows r, int clamp, float* out,
                    int64_t n, hipStream_t s) {
    EDM_VEC_OK(n, xhat, d, xnext, F2, out);
    if (rows_ok(r, n)) return 1;
    hipLaunchKernelGGL(edm_heun_kernel, grid4(n), dim3(256), 0, s, xhat, d, xnext, F2, r, clamp, out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_dpmpp(const float* x, const float* F, float* d_old, EdmRows r, float* out, int64_t n, hipStream_t s) {
    EDM_VEC_OK(n, x, F, d_old, out);
    if (rows_ok(r, n)) return 1;
    hipLaunchKernelGGL(edm_dpmpp_kernel, grid4(n), dim3(256), 0, s, x, F, d_old, r, out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_finalize(const float* x, float* out, int64_t n, hipStream_t s) {
    EDM_VEC_OK(n, x, out);
    hipLaunchKernelGGL(edm_finalize_kernel, grid4(n), dim3(256), 0, s, x, out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_edm_scale(const float* x, float scale, float* out, int64_t n, hipStream_t s) {
    EDM_VEC_OK(n, x, out);
    hipLaunchKernelGGL(edm_scale_kernel, grid4(n), dim3(256), 0, s, x, scale, out, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dm
