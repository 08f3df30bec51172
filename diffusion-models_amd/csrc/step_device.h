// What the table-driven, bandwidth-bound step and loss passes share (edm.hip, ct.hip, repaint.hip, the sampler part of
// elementwise.hip, the loss part of train_kernels.hip): the table-row selector, the 16-byte load / store, the noise fetch,
// the DDPM update, the 256-thread double reduction, and the host-side checks of a 4-floats-per-thread launch.
// The counterpart of conv_device.h for these passes.  Everything here has internal linkage: a translation unit gets its
// own copy, and no second definition of the same name can be picked silently at link time.
//
// `#pragma clang fp contract(off)` is LEXICAL: it covers the text that follows it, not the functions a kernel under it
// calls.  The step kernels turn contraction off so that their expression trees round like the reference's tensor ops, so
// every function of this header that multiplies and adds sits in the header's own contract(off) region below (closed by
// contract(fast), the state the including files are in at their top).  philox.h is included in front of that region, as
// it is in front of the pragma of every file that draws noise.
#pragma once

#include "dm_common.h"
#include "philox.h"

#include <initializer_list>

namespace dm {

// Which table row an element reads.  STEP_ROW_STEP: row st->step (sampling loops; st == nullptr: row 0); STEP_ROW_IMAGE:
// row b of image b (B rows: a (B,) sigma / time); STEP_ROW_FIRST: row 0 whatever st->step says (a stand-alone pass whose
// state only selects the Philox draw).  n = B * per, per % 4 == 0, 16-byte pointers.
enum StepRowMode : int { STEP_ROW_STEP = 0, STEP_ROW_IMAGE = 1, STEP_ROW_FIRST = 2 };
struct StepRows {
    const float* tab;
    const SamplerState* st;
    int mode;
    int64_t per;
};

template <int NCOLS>
static __device__ __forceinline__ const float* step_row(const StepRows& r, int64_t i) {
    const int row = r.mode == STEP_ROW_IMAGE ? (int)(i / r.per) : (r.mode == STEP_ROW_STEP && r.st ? r.st->step : 0);
    return r.tab + (size_t)row * NCOLS;
}
static __device__ __forceinline__ float4 ld4(const float* p, int64_t i) { return *reinterpret_cast<const float4*>(p + i); }
static __device__ __forceinline__ void st4(float* p, int64_t i, float4 v) { *reinterpret_cast<float4*>(p + i) = v; }
static __device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

// The N(0,1) values of the thread's 4 elements: row `step` of noise (rows `stride` floats apart), or the Philox draw
// step + 1 at off4 + i4 under st->seed when noise == nullptr
static __device__ __forceinline__ void step_noise4(const StepRows& r, const float* __restrict__ noise, int64_t stride,
                                                   int64_t i4, float z[4]) {
    const int step = r.st ? r.st->step : 0;
    if (noise) {
        const float4 zv = ld4(noise + (size_t)step * stride, i4 * 4);
        z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
    } else {
        philox_normal4(r.st ? r.st->seed : 0, (uint64_t)step + 1, (r.st ? r.st->off4 : 0) + (uint64_t)i4, z);
    }
}

// Sum of the 256 threads' values in a fixed tree (no atomics); red: 256 doubles of LDS.  The result is red[0], which
// thread 0 may read after the call.
static __device__ __forceinline__ double block_sum256(double s, double* red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    return red[0];
}

// A row of ddpm_step_table / ddim_step_table (DM_COEFS floats) without c[5], the row's noise flag, which the kernels test
struct DdpmCoefs {
    float c0, c1, c2, c3, c4, c6, c7;
};
static __device__ __forceinline__ DdpmCoefs ddpm_coefs(const float* c) { return {c[0], c[1], c[2], c[3], c[4], c[6], c[7]}; }

#pragma clang fp contract(off)
// x_start from the model output by objective (0 pred_noise, 1 pred_x0, 2 pred_v), as predicted
static __device__ __forceinline__ float ddpm_x_start_raw(const DdpmCoefs& c, int objective, float xv, float ev) {
    float x0;
    if (objective == 0) x0 = c.c0 * xv - c.c1 * ev;  // predict_start_from_noise DD/denoising_diffusion.py:570-574
    else if (objective == 1) x0 = ev;                 // the model predicts x_0 :614-617
    else x0 = c.c6 * xv - c.c7 * ev;                  // predict_start_from_v :588-592
    return x0;
}
// ... and clamped (:633)
static __device__ __forceinline__ float ddpm_x_start(const DdpmCoefs& c, int objective, float xv, float ev) {
    return clamp1(ddpm_x_start_raw(c, objective, xv, ev));
}
// ... and dynamically thresholded (dynthresh.hip): clamp(raw, -s, s) / s with the image's s >= 1.  s == 1 gives the bits
// of ddpm_x_start (a division by one is exact); s = NaN (an image that holds a NaN) gives NaN.
static __device__ __forceinline__ float ddpm_x_start_dyn(const DdpmCoefs& c, int objective, float xv, float ev, float s) {
    return fminf(fmaxf(ddpm_x_start_raw(c, objective, xv, ev), -s), s) / s;
}
// The DDPM update from that x_start: posterior mean (:594-598) plus the noise term (:643-644).  The noise-free row keeps
// `c4 * 0.0f`: noise = 0. at t == 0 still meets a NaN / Inf c4, as in the reference.
static __device__ __forceinline__ float ddpm_update(const DdpmCoefs& c, float x0, float xv, bool noisy, float z) {
    const float mean = c.c2 * x0 + c.c3 * xv;
    return noisy ? mean + c.c4 * z : mean + c.c4 * 0.0f;
}
#pragma clang fp contract(fast)

// ---- host side: the checks of a launch that moves 4 floats per thread ------------------------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// `what` opens the messages ("EDM", "continuous-time"); null pointers are optional tensors and pass
static int vec4_ok(const char* what, int64_t n, std::initializer_list<const void*> ptrs) {
    DM_REQUIRE((n) > 0 && (n) % 4 == 0,
               std::string(what) + " passes move 4 floats per thread: the element count must be a multiple of 4");
    for (const void* p_ : ptrs) DM_REQUIRE(aligned16(p_), std::string(what) + " passes need 16-byte aligned tensors");
    return 0;
}
// null_table: what the pass calls its table ("null step table", "null coefficient table")
static int rows_ok(const StepRows& r, int64_t n, const char* null_table) {
    DM_REQUIRE(r.tab != nullptr, null_table);
    DM_REQUIRE(r.mode != STEP_ROW_IMAGE || (r.per > 0 && r.per % 4 == 0 && n % r.per == 0),
               "per-image coefficients need C*H*W to be a multiple of 4 that divides the element count");
    return 0;
}
static dim3 grid4(int64_t n) { return dim3((unsigned)((n / 4 + 255) / 256)); }

// *loss = loss_scale * mean_b(part[b]), image order (train_kernels.hip): the tail of the EDM and continuous-time losses
int launch_loss_mean(const float* part, int B, float* loss, float loss_scale, hipStream_t s);

}  // namespace dm
