// Kernels of the KL first stage (latent-diffusion/ldm/models/autoencoder.py:339-396) and of the codebook lookups next to
// it: the posterior of DiagonalGaussianDistribution (ldm/modules/distributions/distributions.py:24-62) and
// VectorQuantizer.embed_code followed by the permute of VQModel.decode_code (autoencoder.py:118-121).  gfx950 only.
#include "dm_common.h"
#include "philox.h"

#include <algorithm>

// the reference forms mean + std * eps and mean^2 + var - 1 - logvar with separate tensor ops: no contraction
#pragma clang fp contract(off)

namespace dm {

// ---------------------------------------------------------------------------------------
// Posterior.  moments (B, 2E, hw): channel c < E is the mean, channel E + c the log-variance of latent channel c.
//   rows == 1: pixel rows (B * hw, 2E), as quant_conv leaves them in the encoder's arena;  rows == 0: NCHW.
// A thread owns the quads q, q + gridDim.x * 256, ... of one image: elements 4q .. 4q + 3 of the image's (E, hw) block in
// NCHW order, which is also the Philox counter of dm_randn for that shape.  Every moment is read with its own 4-byte
// load: a row of 2E floats is 16-byte aligned only when 2E % 4 == 0, and a quad crosses a channel when hw % 4 != 0.
// z and eps move 16 bytes per lane where the image block and the pointers allow it (vec), else element by element.
// KL: per-thread double sums, a butterfly over the wavefront, the four wavefronts in order through LDS -> part[b][block];
// kl_finish_kernel adds the blocks of an image in order.  No atomics: the result does not depend on arrival order.
// ---------------------------------------------------------------------------------------
constexpr int KL_MAX_BLOCKS = 64;  // blocks per image (a thread strides over its quads beyond that)

__global__ __launch_bounds__(256) void kl_posterior_kernel(const float* __restrict__ moments, int rows,
                                                           const float* __restrict__ eps, uint64_t seed, uint64_t draw,
                                                           uint64_t off4, int sample, float* __restrict__ z,
                                                           float* __restrict__ moments_nchw, double* __restrict__ part,
                                                           int E, int hw, int vec) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const int64_t n = (int64_t)E * hw;  // latent elements of one image
    const int64_t nq = (n + 3) / 4;
    const float* mb = moments + (size_t)b * 2 * n;
    double acc = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        const int64_t j0 = 4 * q;
        float zn[4] = {0.f, 0.f, 0.f, 0.f};
        if (sample) {
            if (!eps) {
                philox_normal4(seed, draw, off4 + (uint64_t)(((int64_t)b * n + j0) >> 2), zn);  // n % 4 == 0 (launcher)
            } else if (vec) {
                const float4 v = *reinterpret_cast<const float4*>(eps + (size_t)b * n + j0);
                zn[0] = v.x; zn[1] = v.y; zn[2] = v.z; zn[3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j0 + k < n) zn[k] = eps[(size_t)b * n + j0 + k];
            }
        }
        float zo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t j = j0 + k;
            if (j >= n) break;
            const int c = (int)(j / hw);
            const int sp = (int)(j - (int64_t)c * hw);
            const size_t im = rows ? (size_t)sp * 2 * E + c : (size_t)c * hw + sp;        // the mean
            const size_t il = rows ? (size_t)sp * 2 * E + E + c : (size_t)(E + c) * hw + sp;  // the log-variance
            const float mean = mb[im], lraw = mb[il];
            const float lv = fminf(fmaxf(lraw, -30.0f), 20.0f);
            zo[k] = sample ? mean + expf(0.5f * lv) * zn[k] : mean;
            if (moments_nchw) {  // parameters stay raw: the clamp is the distribution's, not the tensor's
                moments_nchw[(size_t)b * 2 * n + (size_t)c * hw + sp] = mean;
                moments_nchw[(size_t)b * 2 * n + (size_t)(E + c) * hw + sp] = lraw;
            }
            if (part) acc += (((double)mean * (double)mean + (double)expf(lv)) - 1.0) - (double)lv;
        }
        if (z) {
            if (vec) {
                *reinterpret_cast<float4*>(z + (size_t)b * n + j0) = make_float4(zo[0], zo[1], zo[2], zo[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j0 + k < n) z[(size_t)b * n + j0 + k] = zo[k];
            }
        }
    }
    if (!part) return;  // uniform over the grid
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void kl_finish_kernel(const double* __restrict__ part, float* __restrict__ kl, int B, int n_blocks) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int k = 0; k < n_blocks; ++k) s += part[(size_t)b * n_blocks + k];
    kl[b] = (float)(0.5 * s);
}

static int kl_blocks(int E, int hw) {
    const int64_t nq = ((int64_t)E * hw + 3) / 4;
    return (int)std::min<int64_t>(KL_MAX_BLOCKS, (nq + 255) / 256);
}
// floats of the KL workspace: one double per (image, block)
size_t kl_posterior_ws_floats(int B, int E, int hw) { return (size_t)B * kl_blocks(E, hw) * 2; }

int launch_kl_posterior(const float* moments, int rows, const float* eps, uint64_t seed, uint64_t draw,
                        uint64_t element_offset, int sample, float* z, float* moments_nchw, float* kl, float* kl_ws, int B,
                        int E, int hw, hipStream_t s) {
    DM_REQUIRE(moments, "KL posterior: null moments");
    DM_REQUIRE(B > 0 && E > 0 && hw > 0, "KL posterior: empty input");
    DM_REQUIRE(B <= 65535, "KL posterior: the batch is the grid's y dimension");
    DM_REQUIRE((int64_t)E * hw <= 0x7fffffff, "KL posterior: one image's latent has more than 2^31 - 1 elements");
    DM_REQUIRE(rows == 0 || rows == 1, "KL posterior layout: 0 (NCHW) or 1 (pixel rows)");
    DM_REQUIRE(!kl || kl_ws, "KL posterior: kl needs its workspace");
    if (!z && !moments_nchw && !kl) return 0;
    const int64_t n = (int64_t)E * hw;
    const bool draws = sample && z;  // the noise feeds z alone
    if (draws && !eps) {
        DM_REQUIRE(n % 4 == 0, "KL posterior: Philox noise needs E * h * w % 4 == 0 (one counter serves four elements)");
        DM_REQUIRE(element_offset % 4 == 0, "Philox element offset must be a multiple of 4 (one counter serves 4 elements)");
    }
    const bool al = (reinterpret_cast<uintptr_t>(z) % 16 == 0) && (!(draws && eps) || reinterpret_cast<uintptr_t>(eps) % 16 == 0);
    const int vec = n % 4 == 0 && al;
    const int nb = kl_blocks(E, hw);
    hipLaunchKernelGGL(kl_posterior_kernel, dim3(nb, B), dim3(256), 0, s, moments, rows, draws ? eps : nullptr, seed, draw,
                       element_offset / 4, draws ? 1 : 0, z, moments_nchw, kl ? reinterpret_cast<double*>(kl_ws) : nullptr, E,
                       hw, vec);
    if (kl) hipLaunchKernelGGL(kl_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s,
                               reinterpret_cast<const double*>(kl_ws), kl, B, nb);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------
// Code gather: out[b][c][sp] = codebook[idx[b * hw + sp]][c].  One thread per output element (the store is coalesced, the
// codebook row comes from L2).  An index outside [0, n_embed) is not used as an address: the element is written as zero
// and *bad is raised, which the host wrapper turns into an error.
// ---------------------------------------------------------------------------------------
template <typename I>
__global__ __launch_bounds__(256) void embed_code_kernel(const I* __restrict__ idx, const float* __restrict__ e,
                                                         float* __restrict__ out, int* __restrict__ bad, int64_t total, int E,
                                                         int n_embed, int hw) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int64_t per = (int64_t)E * hw;
    const int64_t b = o / per, r = o - b * per;
    const int c = (int)(r / hw), sp = (int)(r - (int64_t)c * hw);
    const int64_t i = (int64_t)idx[b * hw + sp];
    float v = 0.f;
    if (i >= 0 && i < n_embed)
        v = e[(size_t)i * E + c];
    else
        *bad = 1;
    out[o] = v;
}

int launch_embed_code(const void* indices, int index_bytes, const float* codebook, float* out_nchw, int* bad, int64_t pixels,
                      int E, int n_embed, int hw, hipStream_t s) {
    DM_REQUIRE(indices && codebook && out_nchw && bad, "embed_code: null argument");
    DM_REQUIRE(index_bytes == 4 || index_bytes == 8, "embed_code: indices are int32 (4) or int64 (8)");
    DM_REQUIRE(pixels > 0 && E > 0 && n_embed > 0 && hw > 0, "embed_code: empty input");
    DM_REQUIRE(pixels % hw == 0, "embed_code: pixels is a whole number of images of hw pixels");
    const int64_t total = pixels * E;
    DM_REQUIRE((total + 255) / 256 <= 0x7fffffff, "embed_code: too many elements for one launch");
    DM_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    const dim3 grid((unsigned)((total + 255) / 256));
    if (index_bytes == 4)
        hipLaunchKernelGGL(embed_code_kernel<int32_t>, grid, dim3(256), 0, s, static_cast<const int32_t*>(indices), codebook,
                           out_nchw, bad, total, E, n_embed, hw);
    else
        hipLaunchKernelGGL(embed_code_kernel<int64_t>, grid, dim3(256), 0, s, static_cast<const int64_t*>(indices), codebook,
                           out_nchw, bad, total, E, n_embed, hw);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dm
