// Dynamic thresholding of x_start (Imagen, arXiv 2205.11487, section 2.3) for the DDPM, DDIM and DPM-Solver++ loops:
//   s_b = max(1, quantile_p(|x_start_raw| over image b)),   x_start = clamp(x_start_raw, -s_b, s_b) / s_b
// This file selects s; the update kernels (elementwise.hip) apply it through ddpm_x_start_dyn (step_device.h).
//
// The quantile is torch.quantile's with linear interpolation: q = v_lo + frac * (v_hi - v_lo) in fp32, v_k the k-th
// smallest value; lo and frac come from the host (dyn_params).  v_lo and v_hi are selected exactly, by a radix select on
// the bit pattern of |v|: a non-negative float orders as its uint32.  The 31 bits below the sign go in four digits, most
// significant first -- the 8 exponent bits, then 8, 8 and 7 bits of the mantissa -- and each pass counts the digit of the
// elements that match the digits chosen so far into an LDS histogram, then picks the bin that holds rank lo.  The image
// is read again from global memory in every pass (it is L2-resident: the U-Net has just written the model output), so its
// size is not bounded by the LDS.  Counting with integer atomics and taking a minimum do not depend on the order the
// threads arrive in: the result is exact and the same in every run.
#include "step_device.h"

namespace dm {

namespace {

constexpr int DT_THREADS = 512;
constexpr uint32_t DT_INF = 0x7f800000u;

// the digit of pass 0..3 as (shift, bits)
__device__ __forceinline__ int dt_shift(int pass) { return pass == 0 ? 23 : pass == 1 ? 15 : pass == 2 ? 7 : 0; }
__device__ __forceinline__ int dt_bits(int pass) { return pass == 3 ? 7 : 8; }

// The bin of `hist` (256 counts) that holds rank k, by wave 0: a lane sums four bins, an inclusive scan over the lanes,
// and the one lane whose range holds k writes sel = {bin, k's rank inside the bin, the bin's count}.
__device__ __forceinline__ void dt_pick(const uint32_t* hist, uint32_t k, uint32_t* sel) {
    const int lane = threadIdx.x;
    if (lane >= 64) return;
    const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
    const uint32_t sum = c0 + c1 + c2 + c3;
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    const uint32_t exc = inc - sum;
    if (k < exc || k >= inc) return;
    uint32_t r = k - exc, cnt = c0;
    int bin = 0;
    if (r >= c0) {
        r -= c0; bin = 1; cnt = c1;
        if (r >= c1) {
            r -= c1; bin = 2; cnt = c2;
            if (r >= c2) { r -= c2; bin = 3; cnt = c3; }
        }
    }
    sel[0] = 4 * lane + bin;
    sel[1] = r;
    sel[2] = cnt;
}

#pragma clang fp contract(off)
// One workgroup per image, as cfg_combine_kernel.  x and model_out are rows of `per` floats, image b at b * per; c is the
// coefficient row of st->step (row 0 without a state).  The parameters come from `pdev` when it is set -- the sampler's
// step graph reads them there -- else from `p`.
__global__ void __launch_bounds__(DT_THREADS) dyn_threshold_kernel(int objective, const float* __restrict__ x,
                                                                   const float* __restrict__ model_out,
                                                                   const float* __restrict__ coefs,
                                                                   const SamplerState* __restrict__ st,
                                                                   const DynParams* __restrict__ pdev, DynParams p,
                                                                   int64_t per, float* __restrict__ s_out) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[3];
    __shared__ uint32_t has_nan, next_key;
    if (pdev) p = *pdev;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    if (p.on == 0) {  // uniform over the grid
        if (tid == 0) s_out[b] = 1.0f;
        return;
    }
    const DdpmCoefs dc = ddpm_coefs(coefs + (size_t)(st ? st->step : 0) * 8);
    const float* xb = x + (int64_t)b * per;
    const float* mb = model_out + (int64_t)b * per;
    auto key_at = [&](int64_t i) -> uint32_t {
        return __float_as_uint(ddpm_x_start_raw(dc, objective, xb[i], mb[i])) & 0x7fffffffu;
    };
    const int64_t lo_arg = p.lo < 0 ? 0 : p.lo;
    const uint32_t lo = (uint32_t)(lo_arg < per ? lo_arg : per - 1);

    uint32_t prefix = 0, k = lo, count = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = dt_shift(pass), top = shift + dt_bits(pass);
        const uint32_t mask = (1u << dt_bits(pass)) - 1u;
        if (tid < 256) hist[tid] = 0;
        if (tid == 0) {
            sel[0] = sel[1] = sel[2] = 0;
            if (pass == 0) has_nan = 0;
        }
        __syncthreads();
        bool nan = false;
        for (int64_t i = tid; i < per; i += DT_THREADS) {
            const uint32_t key = key_at(i);
            nan |= key > DT_INF;
            // pass 0: top == 31 and both sides are 0
            if ((key >> top) == (prefix >> top)) atomicAdd(&hist[(key >> shift) & mask], 1u);
        }
        if (pass == 0 && nan) has_nan = 1;  // every writer stores the same value
        __syncthreads();
        if (pass == 0 && has_nan != 0) {  // torch.quantile: an image that holds a NaN has a NaN quantile
            if (tid == 0) s_out[b] = __uint_as_float(0x7fc00000u);
            return;
        }
        dt_pick(hist, k, sel);
        __syncthreads();
        prefix |= sel[0] << shift;
        k = sel[1];
        count = sel[2];
        __syncthreads();  // sel and hist are cleared by the next pass
    }
    // prefix is v_lo; `lo - k` elements are below it and `count` are equal to it
    const uint32_t le = lo - k + count;
    uint32_t hi_key = prefix;
    if ((int64_t)lo + 1 < per && le == lo + 1) {  // v_hi is the smallest element above v_lo; uniform over the workgroup
        if (tid == 0) next_key = 0xffffffffu;
        __syncthreads();
        uint32_t m = 0xffffffffu;
        for (int64_t i = tid; i < per; i += DT_THREADS) {
            const uint32_t key = key_at(i);
            if (key > prefix) m = min(m, key);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = min(m, (uint32_t)__shfl_xor(m, d));
        if (tid % 64 == 0) atomicMin(&next_key, m);
        __syncthreads();
        hi_key = next_key;
    }
    if (tid == 0) {
        const float v_lo = __uint_as_float(prefix), v_hi = __uint_as_float(hi_key);
        const float q = v_lo + p.frac * (v_hi - v_lo);
        s_out[b] = q <= 1.0f ? 1.0f : q;  // a NaN q (inf - inf) stays
    }
}
#pragma clang fp contract(fast)

}  // namespace

DynParams dyn_params(double percentile, int64_t per) {
    const double pos = percentile * (double)(per - 1);
    const double lo = std::floor(pos);
    return DynParams{1, (int32_t)lo, (float)(pos - lo), 0};
}

int launch_dyn_threshold(int objective, const float* x, const float* model_out, const float* coefs_dev,
                         const SamplerState* state_dev, const DynParams* params_dev, DynParams p, int B, int64_t per,
                         float* s_out, hipStream_t s) {
    DM_REQUIRE(x && model_out && coefs_dev && s_out, "dynamic threshold: null argument");
    DM_REQUIRE(B > 0 && per > 0 && per < (int64_t(1) << 31), "dynamic threshold: B > 0 and 1 <= C*H*W < 2^31");
    DM_REQUIRE(params_dev || p.on == 0 || (p.lo >= 0 && p.lo < per && p.frac >= 0.0f && p.frac <= 1.0f),
               "dynamic threshold: the rank lies in [0, C*H*W) and the weight in [0, 1]");
    const bool timed = prof::enabled();
    // at most five passes over x and the model output; a handful of integer operations per element and pass
    if (timed && prof::begin("dyn_threshold_kernel", 10.0 * 5.0 * B * per, 4.0 * 2.0 * 5.0 * B * per, s)) return 1;
    hipLaunchKernelGGL(dyn_threshold_kernel, dim3(B), dim3(DT_THREADS), 0, s, objective, x, model_out, coefs_dev, state_dev,
                       params_dev, p, per, s_out);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    return 0;
}

}  // namespace dm
