// Weighted-objective Gaussian diffusion kernels (gfx950): the reverse step of DD/weighted_objective_gaussian_diffusion.py
// :33-49 behind the base class's p_sample (DD/denoising_diffusion.py:638-645), and the three-term loss of :51-74 with its
// gradient.
//
// The U-Net predicts 2C + 2 maps per image: the noise, x_start and two weight maps.  The softmax over the two weights at a
// pixel blends the x_start derived from the noise with the predicted one.  Both passes are bandwidth-bound: a thread owns 4
// contiguous pixels of one image and walks the C channels, so the two weight maps are read (and their softmax formed) once
// per pixel; one dwordx4 load per tensor, thread and channel; every schedule scalar from the host-built table (weighted.h),
// an fp32 `extract` of the reference.  Contraction is off so the expression trees round like the reference's tensor ops;
// expf is the library function.  Row lookup, 16-byte access, noise fetch, block reduction and the launch checks are those
// of step_device.h.
#include "weighted.h"
#include "step_device.h"

namespace dm {

#pragma clang fp contract(off)

// softmax((w0, w1)) = (sigmoid(w0 - w1), 1 - sigmoid(w0 - w1)), each side formed from exp(-|w0 - w1|) <= 1 so that the
// small one keeps its relative precision
static __device__ __forceinline__ void wo_softmax2(float w0, float w1, float* s0, float* s1) {
    const float d = w0 - w1;
    const float e = expf(-fabsf(d));
    const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
    *s0 = d >= 0.0f ? big : small;
    *s1 = d >= 0.0f ? small : big;
}

// out may alias x (each thread reads its 4 values of a channel before it writes them)
__global__ __launch_bounds__(256) void wo_step_kernel(const float* x, const float* __restrict__ mo,
                                                      const float* __restrict__ noise, int64_t noise_step_stride, StepRows r,
                                                      int C, int64_t HW, int clip, float* out, float* __restrict__ all_steps,
                                                      float* __restrict__ final_out, float* __restrict__ mean_out,
                                                      float* __restrict__ x_start_out, int64_t n_quads, int64_t n) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_quads) return;
    // HW % 4 == 0 keeps the 4 pixels of a thread in one image
    const int64_t pix = q * 4, b = pix / HW, p = pix - b * HW;
    const float* c = step_row<WO_NCOLS>(r, 0);
    const float recip = c[WO_RECIP], recipm1 = c[WO_RECIPM1], coef1 = c[WO_COEF1], coef2 = c[WO_COEF2];
    const float sd = expf(0.5f * c[WO_LOGVAR]);
    const bool noisy = c[WO_NOISE] != 0.0f;
    const float* mb = mo + b * (2 * (int64_t)C + 2) * HW;  // image b of the model output
    const float4 a4 = ld4(mb, 2 * (int64_t)C * HW + p), b4 = ld4(mb, (2 * (int64_t)C + 1) * HW + p);
    const float w0[4] = {a4.x, a4.y, a4.z, a4.w}, w1[4] = {b4.x, b4.y, b4.z, b4.w};
    float s0[4], s1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wo_softmax2(w0[k], w1[k], &s0[k], &s1[k]);  // :37
    const int step = r.st ? r.st->step : 0;
    const bool last = final_out && (!r.st || step == r.st->n_steps - 1);
    const bool unnorm = r.st && r.st->unnormalize;
    for (int ch = 0; ch < C; ++ch) {
        const int64_t i = b * r.per + ch * HW + p;  // element index of (b, ch, p) in a (B, C, H, W) tensor
        const float4 x4 = ld4(x, i), e4 = ld4(mb, ch * HW + p), p4 = ld4(mb, ((int64_t)C + ch) * HW + p);
        const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w}, px[4] = {p4.x, p4.y, p4.z, p4.w};
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (noisy) step_noise4(r, noise, noise_step_stride, i / 4, z);
        float o[4], mean[4], xs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float from_noise = recip * xv[k] - recipm1 * e[k];  // predict_start_from_noise :39
            xs[k] = s0[k] * from_noise + s1[k] * px[k];               // :41-42
            if (clip) xs[k] = clamp1(xs[k]);                          // :44-45
            mean[k] = coef1 * xs[k] + coef2 * xv[k];                  // q_posterior :47
            o[k] = noisy ? mean[k] + sd * z[k] : mean[k] + sd * 0.0f;  // noise = 0. at t == 0 still meets a NaN / Inf sd
        }
        st4(out, i, make_float4(o[0], o[1], o[2], o[3]));
        if (mean_out) st4(mean_out, i, make_float4(mean[0], mean[1], mean[2], mean[3]));
        if (x_start_out) st4(x_start_out, i, make_float4(xs[0], xs[1], xs[2], xs[3]));
        if (all_steps) st4(all_steps + (size_t)(step + 1) * n, i, make_float4(o[0], o[1], o[2], o[3]));
        if (last) {
            if (unnorm)
                st4(final_out, i, make_float4((o[0] + 1.0f) * 0.5f, (o[1] + 1.0f) * 0.5f, (o[2] + 1.0f) * 0.5f, (o[3] + 1.0f) * 0.5f));
            else
                st4(final_out, i, make_float4(o[0], o[1], o[2], o[3]));
        }
    }
}

// One workgroup per image: the three squared errors summed in double in a fixed order (no float atomics: block_sum256);
// dout in the same pass.  A thread's 4 pixels accumulate the weight gradient over the channels in registers.
__global__ __launch_bounds__(256) void wo_loss_kernel(const float* __restrict__ mo, const float* __restrict__ x_start,
                                                      const float* __restrict__ noise, const float* __restrict__ x_t,
                                                      const float* __restrict__ tab, float noise_w, float x_start_w,
                                                      float* __restrict__ dout, float* __restrict__ part,
                                                      float* __restrict__ w_part, float* __restrict__ x_part,
                                                      float* __restrict__ n_part, int C, int64_t HW, int B, float loss_scale) {
    __shared__ double red_w[256];
    __shared__ double red_x[256];
    __shared__ double red_n[256];
    const int b = blockIdx.x;
    const float* c = tab + (size_t)b * WOT_NCOLS;
    const float recip = c[WOT_RECIP], recipm1 = c[WOT_RECIPM1];
    const int64_t per = (int64_t)C * HW;
    const float gscale = loss_scale * 2.0f / ((float)per * (float)B);  // loss_scale * 2 / N
    const int64_t base = (int64_t)b * per, base2 = (int64_t)b * (2 * (int64_t)C + 2) * HW;
    double sw = 0.0, sx = 0.0, sn = 0.0;
    for (int64_t p = (int64_t)threadIdx.x * 4; p < HW; p += 256 * 4) {
        const float4 a4 = ld4(mo, base2 + 2 * (int64_t)C * HW + p), b4 = ld4(mo, base2 + (2 * (int64_t)C + 1) * HW + p);
        const float w0[4] = {a4.x, a4.y, a4.z, a4.w}, w1[4] = {b4.x, b4.y, b4.z, b4.w};
        float s0[4], s1[4], gw[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) wo_softmax2(w0[k], w1[k], &s0[k], &s1[k]);
        for (int ch = 0; ch < C; ++ch) {
            const int64_t i = base + ch * HW + p, in = base2 + ch * HW + p, ix = base2 + ((int64_t)C + ch) * HW + p;
            const float4 n4 = ld4(mo, in), p4 = ld4(mo, ix), z4 = ld4(noise, i), t4 = ld4(x_start, i), q4 = ld4(x_t, i);
            const float pn[4] = {n4.x, n4.y, n4.z, n4.w}, px[4] = {p4.x, p4.y, p4.z, p4.w}, nz[4] = {z4.x, z4.y, z4.z, z4.w};
            const float x0[4] = {t4.x, t4.y, t4.z, t4.w}, xt[4] = {q4.x, q4.y, q4.z, q4.w};
            float gn[4], gx[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xs = recip * xt[k] - recipm1 * pn[k];  // predict_start_from_noise :67
                const bool gate = xs >= -2.0f && xs <= 2.0f;       // torch's clamp passes the gradient on the bounds
                const float xc = fminf(fmaxf(xs, -2.0f), 2.0f);    // :68
                const float wx = s0[k] * xc + s1[k] * px[k];       // :69
                const float dw = wx - x0[k], dx = px[k] - x0[k], dn = pn[k] - nz[k];
                sw += (double)dw * dw;  // :73
                sx += (double)dx * dx;  // :62
                sn += (double)dn * dn;  // :61
                gn[k] = gscale * (noise_w * dn - (gate ? dw * s0[k] * recipm1 : 0.0f));
                gx[k] = gscale * (x_start_w * dx + dw * s1[k]);
                gw[k] += dw * (xc - px[k]) * (s0[k] * s1[k]);
            }
            st4(dout, in, make_float4(gn[0], gn[1], gn[2], gn[3]));
            st4(dout, ix, make_float4(gx[0], gx[1], gx[2], gx[3]));
        }
        const float4 g4 = make_float4(gscale * gw[0], gscale * gw[1], gscale * gw[2], gscale * gw[3]);
        st4(dout, base2 + 2 * (int64_t)C * HW + p, g4);
        st4(dout, base2 + (2 * (int64_t)C + 1) * HW + p, make_float4(-g4.x, -g4.y, -g4.z, -g4.w));
    }
    sw = block_sum256(sw, red_w);
    sx = block_sum256(sx, red_x);
    sn = block_sum256(sn, red_n);
    if (threadIdx.x == 0) {
        const float mw = (float)(sw / per), mx = (float)(sx / per), mn = (float)(sn / per);
        w_part[b] = mw;
        x_part[b] = mx;
        n_part[b] = mn;
        part[b] = (mw + mx * x_start_w) + mn * noise_w;  // :74
    }
}

#pragma clang fp contract(fast)

static int wo_shape_ok(int B, int C, int64_t HW) {
    DM_REQUIRE(B > 0 && C > 0 && HW > 0, "weighted objective: empty tensor");
    DM_REQUIRE(HW % 4 == 0, "weighted-objective passes move 4 pixels of one image per thread: H * W must be a multiple of 4");
    DM_REQUIRE((2 * (int64_t)C + 2) * HW < (int64_t(1) << 30), "weighted objective: (2 C + 2) * H * W must stay below 2^30");
    return 0;
}

int launch_wo_step(const float* x, const float* mo, const float* noise, int64_t noise_step_stride, const float* tab,
                   const SamplerState* st, int row_mode, int B, int C, int64_t HW, int clip, float* out, float* all_steps,
                   float* final_out, float* mean_out, float* x_start_out, hipStream_t s) {
    DM_REQUIRE(x && mo && out, "wo_step: null tensor");
    if (wo_shape_ok(B, C, HW)) return 1;
    const int64_t per = (int64_t)C * HW, n = (int64_t)B * per;
    if (vec4_ok("weighted-objective", n, {x, mo, noise, out, all_steps, final_out, mean_out, x_start_out})) return 1;
    DM_REQUIRE(noise_step_stride % 4 == 0, "noise rows must keep 16-byte alignment");
    DM_REQUIRE(row_mode == STEP_ROW_STEP || row_mode == STEP_ROW_FIRST, "wo_step: the row is the step's, or the first");
    const StepRows r{tab, st, row_mode, per};
    if (rows_ok(r, n, "null step table")) return 1;
    const int64_t n_quads = (int64_t)B * HW / 4;
    hipLaunchKernelGGL(wo_step_kernel, dim3((unsigned)((n_quads + 255) / 256)), dim3(256), 0, s, x, mo, noise, noise_step_stride, r,
                       C, HW, clip ? 1 : 0, out, all_steps, final_out, mean_out, x_start_out, n_quads, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_wo_loss(const float* mo, const float* x_start, const float* noise, const float* x_t, const float* tab,
                   float noise_w, float x_start_w, float* dout, float* part, float* w_part, float* x_part, float* n_part,
                   float* loss, int B, int C, int64_t HW, float loss_scale, hipStream_t s) {
    DM_REQUIRE(mo && x_start && noise && x_t && tab && dout && part && w_part && x_part && n_part && loss, "wo_loss: null tensor");
    if (wo_shape_ok(B, C, HW)) return 1;
    if (vec4_ok("weighted-objective", (int64_t)B * C * HW, {mo, x_start, noise, x_t, dout})) return 1;
    hipLaunchKernelGGL(wo_loss_kernel, dim3(B), dim3(256), 0, s, mo, x_start, noise, x_t, tab, noise_w, x_start_w, dout, part,
                       w_part, x_part, n_part, C, HW, B, loss_scale);
    DM_CHECK_HIP(hipGetLastError());
    return launch_loss_mean(part, B, loss, loss_scale, s);
}

}  // namespace dm
