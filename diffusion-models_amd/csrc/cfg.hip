// Classifier-free guidance (DD/classifier_free_guidance.py:339-369, Unet.forward_with_cond_scale and project :49-60):
// the per-image combine of the conditioned and the null model output, and the row select that gives one batched U-Net
// forward conditioned and null images at once.
#include "dm_common.h"

// the combine follows the reference's rounding: no fused multiply-adds the reference's tensor ops do not make
#pragma clang fp contract(off)

namespace dm {

namespace {

constexpr int CFG_THREADS = 512;
constexpr int CFG_WAVES = CFG_THREADS / 64;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// Sums three doubles over the workgroup.  Every thread gets the same result, summed in a fixed order (lanes by the
// butterfly, then waves 0..CFG_WAVES-1), so an image's result does not depend on the batch around it.
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double (*red)[3]) {
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    c = wave_sum_d(c);
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    __syncthreads();  // `red` may still be read from the previous reduction
    if (lane == 0) {
        red[wave][0] = a;
        red[wave][1] = b;
        red[wave][2] = c;
    }
    __syncthreads();
    a = b = c = 0.0;
#pragma unroll
    for (int w = 0; w < CFG_WAVES; ++w) {
        a += red[w][0];
        b += red[w][1];
        c += red[w][2];
    }
}

// One workgroup per image.  cond / null / out are rows of `per` floats, image b at b * per.  The parameters come from
// `pdev` (4 floats: cond_scale, rescaled_phi, keep_parallel_frac, remove_parallel_component) when it is set -- the
// sampler's step graph reads them there, written before each replay -- else from `p`.
__global__ void __launch_bounds__(CFG_THREADS) cfg_combine_kernel(const float* __restrict__ cond,
                                                                  const float* __restrict__ null_out,
                                                                  float* __restrict__ out, int64_t per,
                                                                  const float* __restrict__ pdev, CfgParams p) {
    __shared__ double red[CFG_WAVES][3];
    if (pdev) p = CfgParams{pdev[0], pdev[1], pdev[2], pdev[3]};
    const float scale_m1 = p.cond_scale - 1.0f;
    const bool remove = p.remove_parallel != 0.0f;
    const int64_t base = (int64_t)blockIdx.x * per;
    const float* c = cond + base;
    const float* nl = null_out + base;
    float* o = out + base;

    // pass 1: <update, cond>, |cond|^2 and sum(cond) in fp64 (project() works in float64, :53-54)
    double s_uc = 0.0, s_cc = 0.0, s_c = 0.0;
    for (int64_t i = threadIdx.x; i < per; i += CFG_THREADS) {
        const float cv = c[i];
        const float up = cv - nl[i];  // update = logits - null_logits, fp32 (:356)
        s_uc += (double)up * (double)cv;
        s_cc += (double)cv * (double)cv;
        s_c += (double)cv;
    }
    block_sum3(s_uc, s_cc, s_c, red);
    // parallel = <update, unit> unit with unit = cond / max(|cond|, 1e-12) (F.normalize)
    const double nrm = fmax(sqrt(s_cc), 1e-12);
    const double coef = s_uc / nrm;

    // pass 2: scaled = logits + update * (cond_scale - 1), with update = orthogonal + parallel * keep when the parallel
    // component is removed (:358-362); sum(scaled) and |scaled|^2 for the rescale
    double s_s = 0.0, s_ss = 0.0, unused = 0.0;
    for (int64_t i = threadIdx.x; i < per; i += CFG_THREADS) {
        const float cv = c[i];
        float up = cv - nl[i];
        if (remove) {
            const double par = coef * ((double)cv / nrm);
            const float par_f = (float)par;
            const float orth_f = (float)((double)up - par);
            up = orth_f + par_f * p.keep_parallel_frac;
        }
        const float sc = cv + up * scale_m1;
        o[i] = sc;
        s_s += (double)sc;
        s_ss += (double)sc * (double)sc;
    }
    if (p.rescaled_phi == 0.0f) return;  // (:364-365); uniform over the workgroup
    block_sum3(s_s, s_ss, unused, red);

    // pass 3: rescaled = scaled * std(logits) / std(scaled), blended by phi (:367-369); unbiased std (correction 1)
    const double n = (double)per;
    const double var_c = fmax((s_cc - s_c * s_c / n) / (n - 1.0), 0.0);
    const double var_s = fmax((s_ss - s_s * s_s / n) / (n - 1.0), 0.0);
    const float ratio = (float)sqrt(var_c) / (float)sqrt(var_s);
    const float phi = p.rescaled_phi, one_m_phi = 1.0f - p.rescaled_phi;
    for (int64_t i = threadIdx.x; i < per; i += CFG_THREADS) {
        const float sc = o[i];
        o[i] = (sc * ratio) * phi + sc * one_m_phi;
    }
}

// y[b][j] = mask[b] ? y[b][j] : x[b * x_ld + j] for j < per
__global__ void select_rows_kernel(float* __restrict__ y, const float* __restrict__ x, int64_t x_ld,
                                   const int32_t* __restrict__ mask, int64_t per, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = i / per, j = i - b * per;
    if (mask[b] == 0) y[i] = x[b * x_ld + j];
}

// Training: the backward of that select (y = mask ? branch(x) : x), four floats per thread.  Row b of `dst` becomes row b
// of `kept` where mask[b] != 0 and row b of `dropped` (zeros when `dropped` is null) elsewhere; rows are 4 * per4 floats long
// and dst_ld / kept_ld / dropped_ld floats apart, all multiples of 4.
//   split: kept = dy, dropped = null                  -> what the text branch receives: exact zeros for the rows that bypassed it
//   merge: dst = kept = the branch's dx, dropped = dy -> the gradient of the select's input, written in place
__global__ void route_rows_kernel(float* dst, int64_t dst_ld, const float* kept, int64_t kept_ld, const float* dropped,
                                  int64_t dropped_ld, const int32_t* __restrict__ mask, int64_t per4, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int64_t b = i / per4, j = 4 * (i - b * per4);
    float4 v{0.f, 0.f, 0.f, 0.f};
    if (mask[b] != 0) {
        if (kept == dst) return;  // in place: the row is already there
        v = *reinterpret_cast<const float4*>(kept + b * kept_ld + j);
    } else if (dropped) {
        v = *reinterpret_cast<const float4*>(dropped + b * dropped_ld + j);
    }
    *reinterpret_cast<float4*>(dst + b * dst_ld + j) = v;
}

}  // namespace

int launch_cfg_combine(const float* cond, const float* null_out, float* out, int B, int64_t per, const float* params_dev,
                       CfgParams p, hipStream_t s) {
    if (B <= 0 || per <= 0) return 0;
    const bool timed = prof::enabled();
    // reads cond and null twice (three times with the rescale), writes out once (twice): 3 passes at most
    if (timed && prof::begin("cfg_combine_kernel", 10.0 * B * per, 4.0 * 7.0 * B * per, s)) return 1;
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(B), dim3(CFG_THREADS), 0, s, cond, null_out, out, per, params_dev, p);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    return 0;
}

int launch_select_rows(float* y, const float* x, int64_t x_ld, const int32_t* mask, int B, int64_t per, hipStream_t s) {
    const int64_t n = (int64_t)B * per;
    if (n == 0) return 0;
    hipLaunchKernelGGL(select_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, y, x, x_ld, mask, per, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_route_rows(float* dst, int64_t dst_ld, const float* kept, int64_t kept_ld, const float* dropped,
                      int64_t dropped_ld, const int32_t* mask, int B, int64_t per, hipStream_t s) {
    DM_REQUIRE(dst && kept && mask && B > 0 && per > 0, "route_rows: null argument");
    DM_REQUIRE(per % 4 == 0 && dst_ld % 4 == 0 && kept_ld % 4 == 0 && dropped_ld % 4 == 0 && dst_ld >= per && kept_ld >= per &&
                   (!dropped || dropped_ld >= per),
               "route_rows: rows are multiples of 4 floats, at least `per` apart");
    const int64_t n4 = (int64_t)B * (per / 4);
    const bool timed = prof::enabled();
    if (timed && prof::begin("route_rows_kernel", 0.0, 4.0 * 2.0 * B * per, s)) return 1;  // at most one read and one write
    hipLaunchKernelGGL(route_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dst, dst_ld, kept, kept_ld,
                       dropped, dropped_ld, mask, per / 4, n4);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    return 0;
}

}  // namespace dm
