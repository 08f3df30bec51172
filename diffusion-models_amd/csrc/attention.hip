// Attention cores of the denoising U-Net (gfx950).  dim_head is 32 in every reference config
// (DD/denoising_diffusion.py:248,155,200); Unet(attn_dim_head=64) is the usual alternative.  Every core is a template on the
// head width DH and is instantiated at 32 and 64 (one width per model); the 32-wide instantiations are the kernels the
// benchmark model runs.  At 64 the LinearAttention context is 64 x 64 per head: 2 x 2 tiles of the 32x32x2 MFMA product.
//
//   LinearAttention core  DD/denoising_diffusion.py:179-192   (two softmaxes + two DH x DH products/head)
//   Attention core        DD/denoising_diffusion.py:221-226 + DD/attend.py:109-124
//   CrossAttention core   DD/denoising_diffusion_text_conditional.py:68-77 (same kernel, no memory kv)
//
// qkv tensors are NHWC, i.e. one row of 3*heads*DH floats per token: [q(h,d) | k(h,d) | v(h,d)].
#include "dm_common.h"

#include <algorithm>

#include <cstdio>
#include <cstdlib>

namespace dm {

// log2 of a supported head width: row / column of a flattened DH x DH index by shift and mask
template <int DH>
constexpr int log2_dh() {
    static_assert(DH == 32 || DH == 64, "head widths 32 and 64");
    return DH == 32 ? 5 : 6;
}

__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ---------------------------------------------------------------------------------------
// LinearAttention, part 1 on the f32 MFMA: ctx[d][e] = sum_t softmax_t(k)[d][t] * v[e][t] is a (DH x n) x (n x DH)
// product per (image, head), with the tokens as the reduction axis:
//   A[i = d][k = token] = exp(k[token][d] - max_d),  B[k = token][j = e] = v[token][e]
// so a lane loads ONE dword of k and ONE of v per step and 32-row tile (lanes 0-31 / 32-63 read the 128 contiguous bytes of
// two consecutive tokens) and each 32x32 tile of the context accumulates in 16 registers (one tile at DH = 32, 2 x 2 at 64).
// grid (heads, B), NW waves; each wave takes 1 / NW of the tokens, the partial contexts meet in LDS.  The 4 memory tokens
// are two extra steps (NMEM = 4); the sequence model's layers have none (NMEM = 0, mem_kv is not read).
// ---------------------------------------------------------------------------------------
using f32x16_t = __attribute__((ext_vector_type(16))) float;

// NW waves per (image, head): the token loop is a chain of load round trips (8 loads in flight per lane and tile, then the
// MFMAs), so with heads x B workgroups and nothing else to overlap, the kernel's time is one wave's chain; 16 waves on the
// 1024 tokens of a 32x32 stage make that chain 8 rounds instead of 32 (45 -> about 15 us in the B = 64 training step).
template <int NW, int DH, int NMEM = 4>
__global__ __launch_bounds__(64 * NW) void linattn_ctx_mfma_kernel(const float* __restrict__ qkv,
                                                                   const float* __restrict__ mem_kv,
                                                                   float* __restrict__ ctx, float* __restrict__ kstats,
                                                                   int n, int heads) {
    static_assert(NMEM == 0 || NMEM == 4, "memory key / values: 4, or none");
    constexpr int NT = DH / 32;  // 32-wide tiles per side of the context
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, half = lane >> 5;
    const int ld = 3 * heads * DH;
    const float* kb = qkv + (size_t)b * n * ld + heads * DH + h * DH + c;
    const float* vb = qkv + (size_t)b * n * ld + 2 * heads * DH + h * DH + c;
    const float* mk = NMEM > 0 ? mem_kv + (size_t)h * DH * NMEM : nullptr;            // [d][j]
    const float* mv = NMEM > 0 ? mem_kv + (size_t)(heads + h) * DH * NMEM : nullptr;  // [e][j]
    __shared__ float red[NW][DH];
    __shared__ float kmax_s[DH], ksum_s[DH];
    // partial-context slots: at DH = 32, 16 waves fold in two rounds (64 KB of static LDS would not fit with the rest); a
    // 64-wide context is 16 KB, so two slots and NW / 2 - 1 rounds
    constexpr int NP = DH == 32 ? (NW > 8 ? NW / 2 : NW) : 2;
    __shared__ __attribute__((aligned(16))) float part[NP][DH * DH];

    // tokens of this wave: [t0, t1), visited two at a time (one per lane half)
    const int per = ((n + 2 * NW - 1) / (2 * NW)) * 2;  // even number of tokens per wave
    const int t0 = min(n, wave * per), t1 = min(n, t0 + per);

    // pass 1: max over all tokens (incl. memory) of k[.][d]; the lane's columns are c + 32 I
    float m[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I) m[I] = -INFINITY;
    {
        int t = t0;
        for (; t + 16 <= t1; t += 16) {
            float kv[8][NT];
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int I = 0; I < NT; ++I) kv[s][I] = kb[(size_t)(t + 2 * s + half) * ld + 32 * I];
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int I = 0; I < NT; ++I) m[I] = fmaxf(m[I], kv[s][I]);
        }
        for (t += half; t < t1; t += 2)
#pragma unroll
            for (int I = 0; I < NT; ++I) m[I] = fmaxf(m[I], kb[(size_t)t * ld + 32 * I]);
    }
    if (NMEM > 0 && wave == 0) {
#pragma unroll
        for (int I = 0; I < NT; ++I) {
            m[I] = fmaxf(m[I], mk[(32 * I + c) * NMEM + half]);
            m[I] = fmaxf(m[I], mk[(32 * I + c) * NMEM + 2 + half]);
        }
    }
#pragma unroll
    for (int I = 0; I < NT; ++I) {
        m[I] = fmaxf(m[I], __shfl_xor(m[I], 32));
        if (half == 0) red[wave][32 * I + c] = m[I];
    }
    __syncthreads();
    if (tid < DH) {
        float mm = red[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) mm = fmaxf(mm, red[w][tid]);
        kmax_s[tid] = mm;
    }
    __syncthreads();
    float kmax[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I) kmax[I] = kmax_s[32 * I + c];

    // pass 2: exp, row sums, and the outer-product accumulation on the matrix core; acc[I][J] is the (d tile I, e tile J)
    f32x16_t acc[NT][NT];
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J < NT; ++J)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[I][J][e] = 0.f;
    float ksum[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I) ksum[I] = 0.f;
    if (NMEM > 0 && wave == 0) {
#pragma unroll
        for (int j = 0; j < NMEM; j += 2) {
            float a[NT], bv[NT];
#pragma unroll
            for (int I = 0; I < NT; ++I) {
                a[I] = __expf(mk[(32 * I + c) * NMEM + j + half] - kmax[I]);
                bv[I] = mv[(32 * I + c) * NMEM + j + half];
                ksum[I] += a[I];
            }
#pragma unroll
            for (int I = 0; I < NT; ++I)
#pragma unroll
                for (int J = 0; J < NT; ++J) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[I], bv[J], acc[I][J], 0, 0, 0);
        }
    }
    int t = t0;
    for (; t + 8 <= t1; t += 8) {  // 4 steps per iteration: 8 loads in flight per lane and tile
        float kv[4][NT], vv[4][NT];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int I = 0; I < NT; ++I) {
                kv[s][I] = kb[(size_t)(t + 2 * s + half) * ld + 32 * I];
                vv[s][I] = vb[(size_t)(t + 2 * s + half) * ld + 32 * I];
            }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float a[NT];
#pragma unroll
            for (int I = 0; I < NT; ++I) {
                a[I] = __expf(kv[s][I] - kmax[I]);
                ksum[I] += a[I];
            }
#pragma unroll
            for (int I = 0; I < NT; ++I)
#pragma unroll
                for (int J = 0; J < NT; ++J)
                    acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[I], vv[s][J], acc[I][J], 0, 0, 0);
        }
    }
    for (; t < t1; t += 2) {  // tail: a missing token contributes a = 0
        const bool ok = t + half < t1;
        float a[NT], bv[NT];
#pragma unroll
        for (int I = 0; I < NT; ++I) {
            a[I] = ok ? __expf(kb[(size_t)(t + half) * ld + 32 * I] - kmax[I]) : 0.f;
            bv[I] = ok ? vb[(size_t)(t + half) * ld + 32 * I] : 0.f;
            ksum[I] += a[I];
        }
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int J = 0; J < NT; ++J) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[I], bv[J], acc[I][J], 0, 0, 0);
    }
#pragma unroll
    for (int I = 0; I < NT; ++I) ksum[I] += __shfl_xor(ksum[I], 32);
    __syncthreads();  // red is reused
    if (half == 0)
#pragma unroll
        for (int I = 0; I < NT; ++I) red[wave][32 * I + c] = ksum[I];
    // accumulator element e of acc[I][J]: row d = 32 I + (e&3) + 8*(e>>2) + 4*half, column 32 J + lane&31
#define DM_LA_SLOT(I, J, e) ((32 * (I) + ((e) & 3) + 8 * ((e) >> 2) + 4 * half) * DH + 32 * (J) + c)
    if constexpr (DH == 32 && NP < NW) {
        if (wave >= NP) {
#pragma unroll
            for (int e = 0; e < 16; ++e) part[wave - NP][DM_LA_SLOT(0, 0, e)] = acc[0][0][e];
        }
        __syncthreads();
        if (wave < NP) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[0][0][e] += part[wave][DM_LA_SLOT(0, 0, e)];
        }
    } else if constexpr (NP < NW) {  // groups of NP waves fold into waves [0, NP), the last group first
        for (int g = NW / NP - 1; g >= 1; --g) {
            if (wave >= g * NP && wave < (g + 1) * NP) {
#pragma unroll
                for (int I = 0; I < NT; ++I)
#pragma unroll
                    for (int J = 0; J < NT; ++J)
#pragma unroll
                        for (int e = 0; e < 16; ++e) part[wave - g * NP][DM_LA_SLOT(I, J, e)] = acc[I][J][e];
            }
            __syncthreads();
            if (wave < NP) {
#pragma unroll
                for (int I = 0; I < NT; ++I)
#pragma unroll
                    for (int J = 0; J < NT; ++J)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[I][J][e] += part[wave][DM_LA_SLOT(I, J, e)];
            }
            __syncthreads();
        }
    }
    if (wave < NP) {
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int J = 0; J < NT; ++J)
#pragma unroll
                for (int e = 0; e < 16; ++e) part[wave][DM_LA_SLOT(I, J, e)] = acc[I][J][e];
    }
#undef DM_LA_SLOT
    __syncthreads();
    if (tid < DH) {
        float ss = red[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) ss += red[w][tid];
        ksum_s[tid] = ss;
        if (kstats) {  // the training tape keeps the column statistics: the backward pass starts from them
            kstats[(size_t)(b * heads + h) * 2 * DH + tid] = kmax_s[tid];
            kstats[(size_t)(b * heads + h) * 2 * DH + DH + tid] = ss;
        }
    }
    __syncthreads();
    float* cp = ctx + (size_t)(b * heads + h) * DH * DH;
    for (int i = tid; i < DH * DH; i += 64 * NW) {
        const int d = i >> log2_dh<DH>();
        float sum = part[0][i];
#pragma unroll
        for (int w = 1; w < NP; ++w) sum += part[w][i];
        cp[i] = sum / ksum_s[d];
    }
}

// part 2 on the matrix core: out^T[e][token] = sum_d ctx[d][e] q_s[token][d] as 32x32x2 MFMA products with the token rows as the
// B operand (attn_bwd.hip's linattn_bwd_*_mfma_kernel describe the layout): lane (token, half) holds the float4 chunks
// 2 m + half of its token's q row = the columns dset(r) = (r & 3) + 8 (r >> 2) + 4 half, r < DH / 2; the softmax over the DH
// columns is DH / 2 registers plus one exchange with lane ^ 32, the K index runs over d in the same order, and the result
// D[i = e][j = token] of e tile E leaves the lane with out[token][32 E + dset(r)], r < 16: four float4 stores per tile.
// grid (ceil(n / 64), heads, B), one wave = 64 tokens.
template <int DH>
__global__ __launch_bounds__(64) void linattn_out_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ ctx,
                                                              float* __restrict__ out, int n, int heads, float scale) {
    constexpr int NT = DH / 32, NS = DH / 2;  // e tiles; k-steps over d
    const int blk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    const int ld = 3 * heads * DH, hid = heads * DH;
    float a[NT][NS];  // A[i = e = 32 E + l31][k -> d = dset(s)] = ctx[d][e]
    {
        const float* cp = ctx + (size_t)(b * heads + h) * DH * DH + l31;
#pragma unroll
        for (int E = 0; E < NT; ++E)
#pragma unroll
            for (int s = 0; s < NS; ++s) a[E][s] = cp[((s & 3) + 8 * (s >> 2) + 4 * half) * DH + 32 * E];
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int tok = blk * 64 + nt * 32 + l31;
        const bool ok = tok < n;
        const size_t row = (size_t)b * n + (ok ? tok : 0);
        const float4* qp = reinterpret_cast<const float4*>(qkv + row * ld + h * DH);
        float q[NS];
#pragma unroll
        for (int m = 0; m < NS / 4; ++m) {
            const float4 t = qp[2 * m + half];
            q[4 * m] = t.x; q[4 * m + 1] = t.y; q[4 * m + 2] = t.z; q[4 * m + 3] = t.w;
        }
        float mx = q[0];
#pragma unroll
        for (int r = 1; r < NS; ++r) mx = fmaxf(mx, q[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < NS; ++r) {
            q[r] = __expf(q[r] - mx);
            sum += q[r];
        }
        sum += __shfl_xor(sum, 32);
        const float inv = scale / sum;
        f32x16_t acc[NT];
#pragma unroll
        for (int E = 0; E < NT; ++E)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[E][r] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int E = 0; E < NT; ++E) acc[E] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[E][s], q[s] * inv, acc[E], 0, 0, 0);
        if (ok) {
            float4* op = reinterpret_cast<float4*>(out + row * hid + h * DH);
#pragma unroll
            for (int E = 0; E < NT; ++E)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    op[8 * E + 2 * m + half] = make_float4(acc[E][4 * m], acc[E][4 * m + 1], acc[E][4 * m + 2], acc[E][4 * m + 3]);
        }
    }
}

template <int DH>
static int linear_attention_core(const float* qkv, const float* mem_kv, float* ctx_ws, float* out, int B, int n, int heads,
                                 hipStream_t s, float* kstats) {
    // waves per (image, head) by the sequence length alone, so that a sample's result does not depend on its batch
    const int nw = n >= 1024 ? 16 : n >= 256 ? 8 : 4;
    const int nmem = mem_kv ? 4 : 0;
    const bool timed = prof::enabled();
    char name[64];
    if (timed) {
        // (n + 4) tokens x DH x DH multiply-adds per (image, head); k and v read once, the context written once
        if (mem_kv) snprintf(name, sizeof(name), "linattn_ctx_mfma_kernel<%d,%d>", nw, DH);
        else snprintf(name, sizeof(name), "linattn_ctx_mfma_kernel<%d,%d,0>", nw, DH);
        if (prof::begin(name, 2.0 * B * heads * (n + (double)nmem) * DH * DH, 4.0 * B * heads * (2.0 * n * DH + DH * DH), s))
            return 1;
    }
    if (!mem_kv) {
        DM_REQUIRE(n >= 1, "LinearAttention without memory key / values needs a token");
        if (nw == 16)
            hipLaunchKernelGGL((linattn_ctx_mfma_kernel<16, DH, 0>), dim3(heads, B), dim3(1024), 0, s, qkv, nullptr, ctx_ws,
                               kstats, n, heads);
        else if (nw == 8)
            hipLaunchKernelGGL((linattn_ctx_mfma_kernel<8, DH, 0>), dim3(heads, B), dim3(512), 0, s, qkv, nullptr, ctx_ws,
                               kstats, n, heads);
        else
            hipLaunchKernelGGL((linattn_ctx_mfma_kernel<4, DH, 0>), dim3(heads, B), dim3(256), 0, s, qkv, nullptr, ctx_ws,
                               kstats, n, heads);
    } else if (nw == 16)
        hipLaunchKernelGGL((linattn_ctx_mfma_kernel<16, DH>), dim3(heads, B), dim3(1024), 0, s, qkv, mem_kv, ctx_ws, kstats,
                           n, heads);
    else if (nw == 8)
        hipLaunchKernelGGL((linattn_ctx_mfma_kernel<8, DH>), dim3(heads, B), dim3(512), 0, s, qkv, mem_kv, ctx_ws, kstats, n,
                           heads);
    else
        hipLaunchKernelGGL((linattn_ctx_mfma_kernel<4, DH>), dim3(heads, B), dim3(256), 0, s, qkv, mem_kv, ctx_ws, kstats, n,
                           heads);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    DM_REQUIRE(B <= 65535, "LinearAttention: batch");
    if (timed) {
        snprintf(name, sizeof(name), "linattn_out_mfma_kernel<%d>", DH);
        if (prof::begin(name, 2.0 * B * heads * (double)n * DH * DH, 4.0 * B * heads * (2.0 * n * DH + DH * DH), s)) return 1;
    }
    hipLaunchKernelGGL(linattn_out_mfma_kernel<DH>, dim3((n + 63) / 64, heads, B), dim3(64), 0, s, qkv, ctx_ws, out, n, heads,
                       1.0f / sqrtf((float)DH));
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    return 0;
}

int launch_linear_attention_core(const float* qkv, const float* mem_kv, float* ctx_ws, float* out, int B, int n,
                                 int heads, int dh, hipStream_t s, float* kstats) {
    DM_REQUIRE(dh == 32 || dh == 64, "LinearAttention kernels support dim_head 32 and 64");
    DM_REQUIRE(heads >= 1 && heads <= 16, "LinearAttention kernel supports 1..16 heads");
    return dh == 32 ? linear_attention_core<32>(qkv, mem_kv, ctx_ws, out, B, n, heads, s, kstats)
                    : linear_attention_core<64>(qkv, mem_kv, ctx_ws, out, B, n, heads, s, kstats);
}

// ---------------------------------------------------------------------------------------
// softmax(q k^T * scale) v for short sequences; K and V of one (batch, head) live in LDS.
// grid (heads, B), 256 threads (4 waves, one query row per wave at a time).
// ---------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(256) void attention_core_kernel(const float* __restrict__ q, int ldq,
                                                             const float* __restrict__ k,
                                                             const float* __restrict__ v, int ldk,
                                                             const float* __restrict__ mem_k,
                                                             const float* __restrict__ mem_v, int n_mem,
                                                             float* __restrict__ out, int ldo, int nq, int nk,
                                                             float scale) {
    constexpr int LDH = log2_dh<DH>();
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntok = nk + n_mem;
    float* Ks = sm;                      // [ntok][DH+1]
    float* Vs = Ks + ntok * (DH + 1);    // [ntok][DH]
    float* Ps = Vs + ntok * DH;          // [4][ntok]
    float* Qs = Ps + 4 * ntok;           // [4][DH]
    for (int it = tid; it < ntok * DH; it += 256) {
        int t = it >> LDH, c = it & (DH - 1);
        float kv, vvv;
        if (t < n_mem) {
            kv = mem_k[((size_t)h * n_mem + t) * DH + c];
            vvv = mem_v[((size_t)h * n_mem + t) * DH + c];
        } else {
            size_t o = ((size_t)b * nk + (t - n_mem)) * ldk + h * DH + c;
            kv = k[o];
            vvv = v[o];
        }
        Ks[t * (DH + 1) + c] = kv;
        Vs[t * DH + c] = vvv;
    }
    __syncthreads();
    float* pw = Ps + wave * ntok;
    float* qw = Qs + wave * DH;
    // blockIdx.z splits the queries when (heads x batch) alone leaves CUs idle (small batches, 64-token stages)
    for (int i = blockIdx.z * 4 + wave; i < nq; i += 4 * gridDim.z) {
        if (lane < DH) qw[lane] = q[((size_t)b * nq + i) * ldq + h * DH + lane] * scale;
        __builtin_amdgcn_wave_barrier();
        // scores for keys j = lane, lane+64, ...
        float mx = -INFINITY;
        for (int j = lane; j < ntok; j += 64) {
            float sc = 0.f;
#pragma unroll
            for (int c = 0; c < DH; ++c) sc += qw[c] * Ks[j * (DH + 1) + c];
            pw[j] = sc;
            mx = fmaxf(mx, sc);
        }
        mx = wave_max64(mx);
        float sum = 0.f;
        for (int j = lane; j < ntok; j += 64) {
            float pe = __expf(pw[j] - mx);
            pw[j] = pe;
            sum += pe;
        }
        sum = wave_sum64(sum);
        __builtin_amdgcn_wave_barrier();
        if constexpr (DH == 32) {
            // out[d] = sum_j p_j v[j][d]; lane = (half, d): halves split the keys
            const int d = lane & 31, half = lane >> 5;
            float acc = 0.f;
            for (int j = half; j < ntok; j += 2) acc += pw[j] * Vs[j * DH + d];
            acc += __shfl_xor(acc, 32);
            if (lane < DH) out[((size_t)b * nq + i) * ldo + h * DH + d] = acc / sum;
        } else {  // lane = d
            float acc = 0.f;
            for (int j = 0; j < ntok; ++j) acc += pw[j] * Vs[j * DH + lane];
            out[((size_t)b * nq + i) * ldo + h * DH + lane] = acc / sum;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// The same for sequences whose K and V do not fit LDS: one wave per 64 queries (lane = query, its q row and the DH
// accumulators in registers), the keys stream through LDS in tiles of 64 twice (row maximum; then exp, row sum and P V) --
// two passes instead of an online rescale keep the arithmetic that of softmax() followed by the product.
// grid (ceil(nq / 64), heads, B), 64 threads.
template <int DH>
__global__ __launch_bounds__(64) void attention_core_tiled_kernel(const float* __restrict__ q, int ldq,
                                                                  const float* __restrict__ k,
                                                                  const float* __restrict__ v, int ldk,
                                                                  const float* __restrict__ mem_k,
                                                                  const float* __restrict__ mem_v, int n_mem,
                                                                  float* __restrict__ out, int ldo, int nq, int nk,
                                                                  float scale) {
    constexpr int LDH = log2_dh<DH>();
    __shared__ float Ks[64 * (DH + 1)], Vs[64 * (DH + 1)];
    const int h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane, ntok = nk + n_mem;
    const bool ok = i < nq;
    float qr[DH], acc[DH];
#pragma unroll
    for (int c = 0; c < DH; ++c) {
        qr[c] = ok ? q[((size_t)b * nq + i) * ldq + h * DH + c] * scale : 0.f;
        acc[c] = 0.f;
    }
    float mx = -INFINITY, sum = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        for (int j0 = 0; j0 < ntok; j0 += 64) {
            __syncthreads();
            for (int e = lane; e < 64 * DH; e += 64) {
                const int t = j0 + (e >> LDH), c = e & (DH - 1);
                float kv = 0.f, vvv = 0.f;
                if (t < ntok) {
                    if (t < n_mem) {
                        kv = mem_k[((size_t)h * n_mem + t) * DH + c];
                        vvv = mem_v[((size_t)h * n_mem + t) * DH + c];
                    } else {
                        const size_t o = ((size_t)b * nk + (t - n_mem)) * ldk + h * DH + c;
                        kv = k[o];
                        vvv = v[o];
                    }
                }
                Ks[(e >> LDH) * (DH + 1) + c] = kv;
                Vs[(e >> LDH) * (DH + 1) + c] = vvv;
            }
            __syncthreads();
            const int jn = min(64, ntok - j0);
            for (int jj = 0; jj < jn; ++jj) {
                float sc = 0.f;
#pragma unroll
                for (int c = 0; c < DH; ++c) sc += qr[c] * Ks[jj * (DH + 1) + c];
                if (pass == 0) {
                    mx = fmaxf(mx, sc);
                } else {
                    const float pe = __expf(sc - mx);
                    sum += pe;
#pragma unroll
                    for (int c = 0; c < DH; ++c) acc[c] += pe * Vs[jj * (DH + 1) + c];
                }
            }
        }
    }
    if (!ok) return;
    const float inv = 1.0f / sum;
    float* o = out + ((size_t)b * nq + i) * ldo + h * DH;
#pragma unroll
    for (int c = 0; c < DH; c += 4) *reinterpret_cast<float4*>(o + c) = make_float4(acc[c] * inv, acc[c + 1] * inv, acc[c + 2] * inv, acc[c + 3] * inv);
}

template <int DH>
static int attention_core(const float* q, int ldq, const float* k, const float* v, int ldk, const float* mem_k,
                          const float* mem_v, int n_mem, float* out, int ldo, int B, int nq, int nk, int heads, float scale,
                          hipStream_t s) {
    int ntok = nk + n_mem;
    size_t lds = ((size_t)ntok * (DH + 1) + (size_t)ntok * DH + 4 * (size_t)ntok + 4 * DH) * sizeof(float);
    static const bool force_tiled = env_flag("DM_ATTN_TILED");  // tests: the tiled form on short sequences
    // beyond ~320 keys the tiled form is also the faster one (tools/attn_time.py: 512 tokens 1.29 vs 2.79 ms per layer at
    // B=64, equal at 256): the LDS-resident kernel re-stages all K / V of an (image, head) in every query block
    static const int tiled_min = env_int("DM_ATTN_TILED_MIN", 320);
    const bool timed = prof::enabled();
    // q k^T and P v: 2 x (nq x ntok x DH) multiply-adds per (image, head); q, k, v read once, out written once
    const double flops = 4.0 * B * heads * (double)nq * ntok * DH, bytes = 4.0 * B * heads * (2.0 * nq + 2.0 * nk) * DH;
    char name[64];
    if (lds > 160 * 1024 || ntok > tiled_min || force_tiled) {
        DM_REQUIRE(B <= 65535 && heads <= 65535 && ldo % 4 == 0, "attention: batch / row stride");
        if (timed) {
            snprintf(name, sizeof(name), "attention_core_tiled_kernel<%d>", DH);
            if (prof::begin(name, flops, bytes, s)) return 1;
        }
        hipLaunchKernelGGL(attention_core_tiled_kernel<DH>, dim3((nq + 63) / 64, heads, B), dim3(64), 0, s, q, ldq, k, v,
                           ldk, mem_k, mem_v, n_mem, out, ldo, nq, nk, scale);
        DM_CHECK_HIP(hipGetLastError());
        if (timed && prof::end(s)) return 1;
        return 0;
    }
    static LdsOptIn lds_flag;
    if (lds_opt_in(lds_flag, reinterpret_cast<const void*>(attention_core_kernel<DH>), 1)) return 1;
    const int qblocks = std::max(1, std::min((nq + 3) / 4, (512 + heads * B - 1) / (heads * B)));
    if (timed) {
        snprintf(name, sizeof(name), "attention_core_kernel<%d>", DH);
        if (prof::begin(name, flops, bytes, s)) return 1;
    }
    hipLaunchKernelGGL(attention_core_kernel<DH>, dim3(heads, B, qblocks), dim3(256), lds, s, q, ldq, k, v, ldk, mem_k,
                       mem_v, n_mem, out, ldo, nq, nk, scale);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    return 0;
}

int launch_attention_core(const float* q, int ldq, const float* k, const float* v, int ldk, const float* mem_k,
                          const float* mem_v, int n_mem, float* out, int ldo, int B, int nq, int nk, int heads,
                          int dh, float scale, hipStream_t s) {
    DM_REQUIRE(dh == 32 || dh == 64, "attention kernels support dim_head 32 and 64");
    return dh == 32 ? attention_core<32>(q, ldq, k, v, ldk, mem_k, mem_v, n_mem, out, ldo, B, nq, nk, heads, scale, s)
                    : attention_core<64>(q, ldq, k, v, ldk, mem_k, mem_v, n_mem, out, ldo, B, nq, nk, heads, scale, s);
}

}  // namespace dm
