// Bits-per-dim evaluation kernels (gfx950): one step of Improved DDPM's calc_bpd_loop (arXiv 2102.09672) around the model
// call, written with the reference's functions -- q_sample in front of it; behind it p_mean_variance of the class
// (DD/denoising_diffusion.py:628-636 or DD/learned_gaussian_diffusion.py:93-111), q_posterior, normal_kl or the
// discretised decoder NLL (learned_gaussian_diffusion.py:25-53), and the two squared errors.
//
// Both passes are bandwidth-bound: one dwordx4 load per tensor and thread, every schedule scalar from the host-built
// table (bpd.h), an fp32 `extract` of the reference.  z is never stored: both passes take it from the injected rows or
// draw it again from Philox.  The term kernel sums in double, per thread, then per workgroup in a fixed tree
// (block_sum256), and a fixed-order pass adds the workgroups of an image: no float atomics, and a result depends on its
// own image only.  Contraction is off so the expression trees round like the reference's tensor ops; expf / logf / tanhf
// are the library functions.  Row lookup, 16-byte access, noise fetch and the launch checks are those of step_device.h.
#include "bpd.h"
#include "learned.h"
#include "step_device.h"

namespace dm {

static_assert(BPD_CHUNK == 256 * 4, "the term kernel moves one dwordx4 per thread");

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void bpd_step_in_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                          int64_t noise_step_stride, StepRows r, float* __restrict__ x_t,
                                                          int64_t n) {
    const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = i4 * 4;
    if (i >= n) return;
    const float* c = step_row<BPD_NCOLS>(r, i);
    const float a = c[BPD_SQRT_AC], sg = c[BPD_SQRT_1M_AC];
    const float4 x4 = ld4(x0, i);
    float z[4];
    step_noise4(r, noise, noise_step_stride, i4, z);
    st4(x_t, i, make_float4(a * x4.x + sg * z[0], a * x4.y + sg * z[1], a * x4.z + sg * z[2], a * x4.w + sg * z[3]));  // :813-821
}

// grid (chunks, B): workgroup (k, b) sums elements [k BPD_CHUNK, (k + 1) BPD_CHUNK) of image b
__global__ __launch_bounds__(256) void bpd_terms_kernel(const float* __restrict__ mo, const float* __restrict__ x0,
                                                        const float* __restrict__ xt, const float* __restrict__ noise,
                                                        int64_t noise_step_stride, StepRows r, int learned, int objective,
                                                        int clip, double* __restrict__ part) {
    __shared__ double red0[256];
    __shared__ double red1[256];
    __shared__ double red2[256];
    const int b = blockIdx.y, B = gridDim.y;
    const int64_t per = r.per;
    const int64_t j = (int64_t)blockIdx.x * BPD_CHUNK + (int64_t)threadIdx.x * 4;
    double s_vb = 0.0, s_xs = 0.0, s_eps = 0.0;
    if (j < per) {
        const float* c = step_row<BPD_NCOLS>(r, 0);
        const DdpmCoefs dc = ddpm_coefs(c);
        const float post_log = c[BPD_POST_LOG], max_log = c[BPD_MAX_LOG];
        const bool t0 = c[BPD_T0] != 0.0f;
        const int64_t i = (int64_t)b * per + j;
        // learned variance: image b's prediction half starts at b * 2 per, its variance half at b * 2 per + per
        const int64_t im = learned ? (int64_t)b * 2 * per + j : i;
        const float4 e4 = ld4(mo, im), a4 = ld4(x0, i), q4 = ld4(xt, i);
        const float4 v4 = learned ? ld4(mo, im + per) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float e[4] = {e4.x, e4.y, e4.z, e4.w}, xs0[4] = {a4.x, a4.y, a4.z, a4.w}, x[4] = {q4.x, q4.y, q4.z, q4.w};
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        float z[4];
        step_noise4(r, noise, noise_step_stride, i / 4, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // the learned class reads the first half as noise whatever `objective` says (the caller passes 0)
            const float xs = clip ? ddpm_x_start(dc, objective, x[k], e[k]) : ddpm_x_start_raw(dc, objective, x[k], e[k]);
            const float logvar = learned ? lv_logvar(v[k], post_log, max_log) : post_log;
            const float model_mean = dc.c2 * xs + dc.c3 * x[k];     // q_posterior(x_start = pred, x_t)
            const float true_mean = dc.c2 * xs0[k] + dc.c3 * x[k];  // q_posterior(x_start = x0, x_t)
            float dlv;
            s_vb += (double)lv_vb_term(t0, xs0[k], true_mean, post_log, model_mean, logvar, &dlv);
            const float dx = xs - xs0[k];
            s_xs += (double)dx * dx;
            const float de = (dc.c0 * x[k] - xs) / dc.c1 - z[k];  // predict_noise_from_start :576-580
            s_eps += (double)de * de;
        }
    }
    // the tree of block_sum256 for the three sums at once: a third of the barriers, the same order of additions
    red0[threadIdx.x] = s_vb;
    red1[threadIdx.x] = s_xs;
    red2[threadIdx.x] = s_eps;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) {
            red0[threadIdx.x] += red0[threadIdx.x + m];
            red1[threadIdx.x] += red1[threadIdx.x + m];
            red2[threadIdx.x] += red2[threadIdx.x + m];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)blockIdx.x * B + b) * 3;
        p[0] = red0[0];
        p[1] = red1[0];
        p[2] = red2[0];
    }
}

// One thread per result: rows[step][b][q] = mean over the image of quantity q (chunk order), the first in bits.  Then the
// step counter: every workgroup takes a ticket once its threads have read st->step, and the one that takes the last
// ticket puts the ticket counter back to zero and advances the step (integer atomics only; nothing waits).
__global__ __launch_bounds__(256) void bpd_finish_kernel(const double* __restrict__ part, int chunks, int B, double per,
                                                         SamplerState* st, float* __restrict__ rows, unsigned* ticket) {
    const int step = st ? st->step : 0;
    const float nat = 1.4426950408889634f;  // NAT = 1 / ln 2
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < 3 * B) {
        double s = 0.0;
        for (int k = 0; k < chunks; ++k) s += part[(size_t)k * B * 3 + o];
        const float m = (float)(s / per);  // meanflat
        rows[(size_t)step * B * 3 + o] = o % 3 == 0 ? m * nat : m;
    }
    if (!st) return;
    __syncthreads();  // every thread of the workgroup has read st->step
    if (threadIdx.x == 0 && atomicAdd(ticket, 1u) == gridDim.x - 1) {
        *ticket = 0;
        st->step = step + 1;
    }
}

// One workgroup per image: normal_kl(mean1 = sqrt_ac x0, logvar1, 0, 0) (learned_gaussian_diffusion.py:25-29).  In double:
// with logvar1 = log(1 - alphas_cumprod[T - 1]) next to zero, -1 - logvar1 + exp(logvar1) is what is left of O(1) terms
// after they cancel, and in fp32 one ulp of expf decides the result (3.5e-8 bits at T = 24, linear).  The pass runs once
// per call over fp32 inputs, as the reference's fp64 run sees them.
__global__ __launch_bounds__(256) void bpd_prior_kernel(const float* __restrict__ x0, float sqrt_ac, float logvar,
                                                        float* __restrict__ prior, int64_t per) {
    __shared__ double red[256];
    const int64_t base = (int64_t)blockIdx.x * per;
    const double a = (double)sqrt_ac, lv = (double)logvar;
    const double c = (-1.0 + 0.0 - lv) + exp(lv - 0.0);
    double s = 0.0;
    for (int64_t i = (int64_t)threadIdx.x * 4; i < per; i += 256 * 4) {
        const float4 a4 = ld4(x0, base + i);
        const double m[4] = {a * a4.x, a * a4.y, a * a4.z, a * a4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) s += 0.5 * (c + m[k] * m[k]);
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) prior[blockIdx.x] = (float)(s / (double)per * 1.4426950408889634);
}

#pragma clang fp contract(fast)

int launch_bpd_step_in(const float* x0, const float* noise, int64_t noise_step_stride, const float* tab, const SamplerState* st,
                       int row_mode, float* x_t, int64_t n, hipStream_t s) {
    DM_REQUIRE(x0 && x_t, "bpd_step_in: null tensor");
    DM_REQUIRE(row_mode == STEP_ROW_STEP || row_mode == STEP_ROW_FIRST, "bpd_step_in: the row is the step's, or the first");
    if (vec4_ok("bits-per-dim", n, {x0, noise, x_t})) return 1;
    DM_REQUIRE(noise_step_stride % 4 == 0, "noise rows must keep 16-byte alignment");
    const StepRows r{tab, st, row_mode, 0};
    if (rows_ok(r, n, "null step table")) return 1;
    const bool timed = prof::enabled();
    if (timed && prof::begin("bpd_step_in_kernel", 2.0 * n, 4.0 * (noise ? 3.0 : 2.0) * n, s)) return 1;
    hipLaunchKernelGGL(bpd_step_in_kernel, grid4(n), dim3(256), 0, s, x0, noise, noise_step_stride, r, x_t, n);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    return 0;
}

int launch_bpd_terms(const float* model_out, const float* x0, const float* x_t, const float* noise, int64_t noise_step_stride,
                     const float* tab, SamplerState* st, int learned, int objective, int clip, float* part, float* rows,
                     unsigned* ticket, int B, int64_t per, hipStream_t s) {
    DM_REQUIRE(model_out && x0 && x_t && part && rows, "bpd_terms: null tensor");
    DM_REQUIRE(!st || ticket, "bpd_terms: the step counter needs its ticket counter");
    DM_REQUIRE(B > 0 && B <= 65535, "bpd_terms: the batch is one grid row per image (1 .. 65535)");
    DM_REQUIRE(per > 0 && per % 4 == 0 && per < (int64_t(1) << 40), "bpd_terms: C*H*W must be a multiple of 4");
    DM_REQUIRE(objective >= 0 && objective <= 2, "bpd_terms: unknown objective");
    DM_REQUIRE(!learned || objective == 0, "bpd_terms: the learned-variance class reads the first half as noise");
    if (vec4_ok("bits-per-dim", (int64_t)B * per, {model_out, x0, x_t, noise})) return 1;
    DM_REQUIRE((reinterpret_cast<uintptr_t>(part) & 7) == 0, "bpd_terms: the partial sums are doubles");
    DM_REQUIRE(noise_step_stride % 4 == 0, "noise rows must keep 16-byte alignment");
    const StepRows r{tab, st, STEP_ROW_STEP, per};
    if (rows_ok(r, (int64_t)B * per, "null step table")) return 1;
    const int chunks = bpd_chunks(per);
    double* pd = reinterpret_cast<double*>(part);
    const bool timed = prof::enabled();
    const double n = (double)B * per;
    // reads: the model output (n or 2n), x0, x_t [, z]; some forty flops and three transcendentals per element
    if (timed && prof::begin("bpd_terms_kernel", 40.0 * n, 4.0 * ((learned ? 4.0 : 3.0) + (noise ? 1.0 : 0.0)) * n, s)) return 1;
    hipLaunchKernelGGL(bpd_terms_kernel, dim3(chunks, B), dim3(256), 0, s, model_out, x0, x_t, noise, noise_step_stride, r,
                       learned ? 1 : 0, objective, clip ? 1 : 0, pd);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    if (timed && prof::begin("bpd_finish_kernel", 3.0 * chunks * B, 8.0 * 3.0 * chunks * B, s)) return 1;
    hipLaunchKernelGGL(bpd_finish_kernel, dim3((3 * B + 255) / 256), dim3(256), 0, s, pd, chunks, B, (double)per, st, rows, ticket);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    return 0;
}

int launch_bpd_prior(const float* x0, float sqrt_ac, float logvar, float* prior, int B, int64_t per, hipStream_t s) {
    DM_REQUIRE(x0 && prior && B > 0, "bpd_prior: null tensor");
    DM_REQUIRE(per > 0 && per % 4 == 0, "bpd_prior: C*H*W must be a multiple of 4");
    if (vec4_ok("bits-per-dim", (int64_t)B * per, {x0})) return 1;
    hipLaunchKernelGGL(bpd_prior_kernel, dim3(B), dim3(256), 0, s, x0, sqrt_ac, logvar, prior, per);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dm
