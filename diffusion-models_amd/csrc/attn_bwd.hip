// Backward of the two attention cores for the training step (autograd of DD/denoising_diffusion.py:179-192
// LinearAttention and :221-226 + DD/attend.py:109-124 Attention).  dim_head = 32 or 64, 4 learned memory key/values.
// qkv / dqkv are NHWC token rows [q(h,d) | k(h,d) | v(h,d)]; the cores hold < 2 % of a step's FLOPs, so these are plain
// LDS-tiled VALU kernels with a fixed summation order (no atomics).  Every kernel is a template on the head width DH and is
// instantiated at 32 and 64 (attention.hip); at 64 the 32x32x2 MFMA products of the LinearAttention backward work on 2 x 2
// tiles of the 64 x 64 context.
//
// LinearAttention:  p = softmax_d(q);  qs = p * scale;  ks = softmax_tokens(k_ext);  ctx[d][e] = sum_j ks[d][j] v_ext[e][j];
//                   out[e][i] = sum_d ctx[d][e] qs[d][i]
//   dctx[d][e] = sum_i qs[d][i] dout[e][i]         dqs[d][i] = sum_e ctx[d][e] dout[e][i]
//   dq[d][i]   = scale p[d][i] (dqs[d][i] - sum_d' p[d'][i] dqs[d'][i])
//   dks[d][j]  = sum_e dctx[d][e] v[e][j]          dv[e][j] = sum_d ks[d][j] dctx[d][e]
//   dk[d][j]   = ks[d][j] (dks[d][j] - S[d]),      S[d] = sum_j ks dks = sum_e dctx[d][e] ctx[d][e]
#include "dm_common.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace dm {

constexpr int NMEM = 4;
// log2 of a supported head width: row / column of a flattened DH-wide index by shift and mask
template <int DH>
constexpr int bwd_log2_dh() {
    static_assert(DH == 32 || DH == 64, "head widths 32 and 64");
    return DH == 32 ? 5 : 6;
}
using f32x4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f32x4 make_f32x4(float a, float b, float c, float d) { return f32x4{a, b, c, d}; }

// LDS row stride of a token row: 16-byte aligned, 128-bit accesses of 8 consecutive lanes cover all banks
template <int DH>
constexpr int lstr() { return DH + 4; }

// The LinearAttention backward is three launches: linattn_bwd_q_mfma_kernel (dq, and each 64-token block's share of dctx),
// this kernel, then linattn_bwd_kv_mfma_kernel (dk, dv).
// part 2: grid (heads, B), 256 threads: dctx = sum of the block shares (left in share 0), per d the softmax statistics of
// k over the tokens (the forward pass's kstats) and S[d] -> stats (B, heads, 3, DH), and the gradients of this image's 4
// memory key/value tokens.
template <int DH>
__global__ __launch_bounds__(256) void linattn_bwd_stats_kernel(const float* __restrict__ mem_kv, const float* __restrict__ ctx,
                                                                float* __restrict__ dctx_part, int nblk,
                                                                float* __restrict__ stats, float* __restrict__ dmem_part,
                                                                const float* __restrict__ kstats, int heads) {
    constexpr int LDH = bwd_log2_dh<DH>(), NJ = DH * DH / 256;
    __shared__ float dctx[DH][DH + 1];
    __shared__ float kmax[DH], kinv[DH], S[DH];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* mk = mem_kv + (size_t)h * DH * NMEM;  // [d][j]
    {  // the block shares of dctx, summed in block order; the 4 elements of a thread x 4 shares are in flight together
        float s[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) s[j] = 0.f;
        const float* src = dctx_part + ((size_t)b * nblk * heads + h) * DH * DH + tid;
        const size_t kst = (size_t)heads * DH * DH;
        int k = 0;
        for (; k + 4 <= nblk; k += 4) {
            float v[4][NJ];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int j = 0; j < NJ; ++j) v[kk][j] = src[(k + kk) * kst + 256 * j];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int j = 0; j < NJ; ++j) s[j] += v[kk][j];
        }
        for (; k < nblk; ++k)
#pragma unroll
            for (int j = 0; j < NJ; ++j) s[j] += src[k * kst + 256 * j];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int i = tid + 256 * j;
            dctx[i >> LDH][i & (DH - 1)] = s[j];
            dctx_part[((size_t)b * nblk * heads + h) * DH * DH + i] = s[j];
        }
    }
    __syncthreads();
    if (tid < DH) {
        // kstats: the column max and the column sum over tokens of exp(k - max), as the forward context kernel left them
        const float* ks = kstats + (size_t)(b * heads + h) * 2 * DH;
        const float* cr = ctx + ((size_t)(b * heads + h) * DH + tid) * DH;
        float sd = 0.f;
        for (int e = 0; e < DH; ++e) sd += dctx[tid][e] * cr[e];
        float* st = stats + (size_t)(b * heads + h) * 3 * DH;
        st[tid] = kmax[tid] = ks[tid];
        st[DH + tid] = kinv[tid] = 1.0f / ks[DH + tid];
        st[2 * DH + tid] = S[tid] = sd;
    }
    __syncthreads();
    if (tid < NMEM * DH) {  // memory tokens: thread (t, x) forms dk[d = x][t] and dv[e = x][t]
        const int t = tid >> LDH, x = tid & (DH - 1);
        const float* mv = mem_kv + (size_t)(heads + h) * DH * NMEM;  // [e][j]
        float sk = 0.f, sv = 0.f;
        for (int j = 0; j < DH; ++j) {
            sk += dctx[x][j] * mv[j * NMEM + t];
            sv += __expf(mk[j * NMEM + t] - kmax[j]) * kinv[j] * dctx[j][x];
        }
        float* o = dmem_part + (size_t)b * 2 * heads * DH * NMEM;
        o[((size_t)h * DH + x) * NMEM + t] = __expf(mk[x * NMEM + t] - kmax[x]) * kinv[x] * (sk - S[x]);
        o[((size_t)(heads + h) * DH + x) * NMEM + t] = sv;
    }
}

// ---- parts 1 and 3 on the matrix core (v_mfma_f32_32x32x2_f32), grid (ceil(n / 64), heads, B).  Every product of the
// backward pass is a (tokens x DH) x (DH x DH) GEMM; computed TRANSPOSED -- the DH x DH matrix (ctx, dctx) is the A operand, the
// token rows the B operand -- the result D[i][j = token] of a 32-row tile leaves lane (token, half) with the 16 columns
//     dset(r) = (r & 3) + 8 (r >> 2) + 4 half,   r = 0 .. 15      (four float4 chunks 2 m + half of the token's 32-float row)
// of its token, and with the K index enumerated in the same order (k-step s of half h = column dset(s), s < DH / 2) the B
// operand of the next product is exactly those registers: a lane loads DH / 8 chunks of q / dout / k / v, keeps everything
// row-wise (softmax over the columns, the dot products) in registers plus one exchange with lane ^ 32, and stores them.  At
// DH = 64 tile I of a result holds the columns 32 I + dset(r) = dset(16 I + r): the same registers.  One wave = 64 tokens (two
// 32-token tiles), 64 MFMAs per pass at DH = 32 where a lane-per-token VALU form issued ~2000 FMAs and ~600 LDS broadcasts
// per lane.
using f32x16 = __attribute__((ext_vector_type(16))) float;

template <int DH>
__global__ __launch_bounds__(64) void linattn_bwd_q_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ ctx,
                                                                const float* __restrict__ dout, float* __restrict__ dqkv,
                                                                float* __restrict__ dctx_part, int n, int heads, float scale) {
    constexpr int NT = DH / 32, NS = DH / 2;  // 32-wide tiles per side; registers (k-steps) per row and lane
    __shared__ __attribute__((aligned(16))) float ps[64 * lstr<DH>()];  // scale * p, [token][d]
    __shared__ __attribute__((aligned(16))) float ds[64 * lstr<DH>()];  // dout,      [token][e]
    const int blk = blockIdx.x, nblk = gridDim.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    const int ld = 3 * heads * DH, hid = heads * DH;
    // A operand of dqs^T = ctx . dout^T: ctx[d = 32 I + l31][e = dset(s)]
    float actx[NT][NS];
#pragma unroll
    for (int I = 0; I < NT; ++I) {
        const f32x4* cr = reinterpret_cast<const f32x4*>(ctx + ((size_t)(b * heads + h) * DH + 32 * I + l31) * DH);
#pragma unroll
        for (int m = 0; m < NS / 4; ++m) {
            const f32x4 v = cr[2 * m + half];
#pragma unroll
            for (int i = 0; i < 4; ++i) actx[I][4 * m + i] = v[i];
        }
    }
    float p[2][NS], dv[2][NS];
    bool okt[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int tok = blk * 64 + nt * 32 + l31;
        okt[nt] = tok < n;
        const size_t row = (size_t)b * n + (okt[nt] ? tok : 0);
        const f32x4* qp = reinterpret_cast<const f32x4*>(qkv + row * ld + h * DH);
        const f32x4* dp = reinterpret_cast<const f32x4*>(dout + row * hid + h * DH);
#pragma unroll
        for (int m = 0; m < NS / 4; ++m) {
            const f32x4 a = qp[2 * m + half], c = dp[2 * m + half];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                p[nt][4 * m + i] = a[i];
                dv[nt][4 * m + i] = okt[nt] ? c[i] : 0.f;
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        float m = -INFINITY;
#pragma unroll
        for (int r = 0; r < NS; ++r) m = fmaxf(m, p[nt][r]);
        m = fmaxf(m, __shfl_xor(m, 32));
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < NS; ++r) {
            p[nt][r] = __expf(p[nt][r] - m);
            sum += p[nt][r];
        }
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int r = 0; r < NS; ++r) p[nt][r] *= inv;
        f32x16 acc[NT];
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[I][r] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int I = 0; I < NT; ++I) acc[I] = __builtin_amdgcn_mfma_f32_32x32x2f32(actx[I][s], dv[nt][s], acc[I], 0, 0, 0);
        float dot = 0.f;
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int r = 0; r < 16; ++r) dot += p[nt][16 * I + r] * acc[I][r];
        dot += __shfl_xor(dot, 32);
        const int tok = blk * 64 + nt * 32 + l31;
        if (okt[nt]) {
            f32x4* o = reinterpret_cast<f32x4*>(dqkv + ((size_t)b * n + tok) * ld + h * DH);
#pragma unroll
            for (int I = 0; I < NT; ++I)
#pragma unroll
                for (int m4 = 0; m4 < 4; ++m4) {
                    const float* pp = &p[nt][16 * I + 4 * m4];
                    o[8 * I + 2 * m4 + half] = make_f32x4(scale * pp[0] * (acc[I][4 * m4] - dot),
                                                          scale * pp[1] * (acc[I][4 * m4 + 1] - dot),
                                                          scale * pp[2] * (acc[I][4 * m4 + 2] - dot),
                                                          scale * pp[3] * (acc[I][4 * m4 + 3] - dot));
                }
        }
        const float z = okt[nt] ? scale : 0.f;
        float* pr = ps + (nt * 32 + l31) * lstr<DH>();
        float* dr = ds + (nt * 32 + l31) * lstr<DH>();
#pragma unroll
        for (int m4 = 0; m4 < NS / 4; ++m4) {
            *reinterpret_cast<f32x4*>(pr + 4 * (2 * m4 + half)) =
                make_f32x4(z * p[nt][4 * m4], z * p[nt][4 * m4 + 1], z * p[nt][4 * m4 + 2], z * p[nt][4 * m4 + 3]);
            *reinterpret_cast<f32x4*>(dr + 4 * (2 * m4 + half)) =
                make_f32x4(dv[nt][4 * m4], dv[nt][4 * m4 + 1], dv[nt][4 * m4 + 2], dv[nt][4 * m4 + 3]);
        }
    }
    __syncthreads();
    // dctx share of this block: D[i = d][j = e] = sum over the 64 tokens (k-step s, half -> token 2 s + half) ps[t][d] ds[t][e],
    // tile (I, J) = (d, e) in [32 I, 32 I + 32) x [32 J, 32 J + 32)
    f32x16 acc[NT][NT];
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J < NT; ++J)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[I][J][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        float pa[NT], db[NT];
#pragma unroll
        for (int I = 0; I < NT; ++I) {
            pa[I] = ps[(2 * s + half) * lstr<DH>() + 32 * I + l31];
            db[I] = ds[(2 * s + half) * lstr<DH>() + 32 * I + l31];
        }
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int J = 0; J < NT; ++J) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[I], db[J], acc[I][J], 0, 0, 0);
    }
    float* o = dctx_part + (((size_t)b * nblk + blk) * heads + h) * DH * DH;
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J < NT; ++J)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[(32 * I + (r & 3) + 8 * (r >> 2) + 4 * half) * DH + 32 * J + l31] = acc[I][J][r];
}

template <int DH>
__global__ __launch_bounds__(64) void linattn_bwd_kv_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx_part,
                                                                 int nblk, const float* __restrict__ stats,
                                                                 float* __restrict__ dqkv, int n, int heads) {
    constexpr int NT = DH / 32, NS = DH / 2;
    const int blk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    const int ld = 3 * heads * DH;
    const float* dctx = dctx_part + ((size_t)b * nblk * heads + h) * DH * DH;  // share 0 holds the sum
    // A operands: dv^T = dctx^T . ks^T needs dctx[d = dset(s)][e = 32 J + l31]; dks^T = dctx . v^T needs
    // dctx[d = 32 I + l31][e = dset(s)]
    float a3[NT][NS], a4[NT][NS], kmax[NS], kinv[NS], S[NS];
    {
        const f32x4* st = reinterpret_cast<const f32x4*>(stats + (size_t)(b * heads + h) * 3 * DH);
#pragma unroll
        for (int m = 0; m < NS / 4; ++m) {
            f32x4 v[NT];
#pragma unroll
            for (int I = 0; I < NT; ++I) v[I] = reinterpret_cast<const f32x4*>(dctx + (32 * I + l31) * DH)[2 * m + half];
            const f32x4 s0 = st[2 * m + half], s1 = st[DH / 4 + 2 * m + half], s2 = st[DH / 2 + 2 * m + half];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int I = 0; I < NT; ++I) {
                    a4[I][4 * m + i] = v[I][i];
                    a3[I][4 * m + i] = dctx[(8 * m + 4 * half + i) * DH + 32 * I + l31];
                }
                kmax[4 * m + i] = s0[i];
                kinv[4 * m + i] = s1[i];
                S[4 * m + i] = s2[i];
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int tok = blk * 64 + nt * 32 + l31;
        const bool ok = tok < n;
        const size_t row = (size_t)b * n + (ok ? tok : 0);
        const f32x4* kp = reinterpret_cast<const f32x4*>(qkv + row * ld + heads * DH + h * DH);
        const f32x4* vp = reinterpret_cast<const f32x4*>(qkv + row * ld + 2 * heads * DH + h * DH);
        float ks[NS], vv[NS];
#pragma unroll
        for (int m = 0; m < NS / 4; ++m) {
            const f32x4 a = kp[2 * m + half], c = vp[2 * m + half];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ks[4 * m + i] = __expf(a[i] - kmax[4 * m + i]) * kinv[4 * m + i];
                vv[4 * m + i] = c[i];
            }
        }
        f32x16 dvt[NT], dkt[NT];
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int r = 0; r < 16; ++r) dvt[I][r] = dkt[I][r] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int I = 0; I < NT; ++I) {
                dvt[I] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3[I][s], ks[s], dvt[I], 0, 0, 0);
                dkt[I] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[I][s], vv[s], dkt[I], 0, 0, 0);
            }
        }
        if (ok) {
            f32x4* okp = reinterpret_cast<f32x4*>(dqkv + row * ld + heads * DH + h * DH);
            f32x4* ovp = reinterpret_cast<f32x4*>(dqkv + row * ld + 2 * heads * DH + h * DH);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
#pragma unroll
                for (int I = 0; I < NT; ++I) {
                    const int r = 16 * I + 4 * m;  // register of column 32 I + dset(4 m)
                    ovp[8 * I + 2 * m + half] = make_f32x4(dvt[I][4 * m], dvt[I][4 * m + 1], dvt[I][4 * m + 2], dvt[I][4 * m + 3]);
                    okp[8 * I + 2 * m + half] = make_f32x4(ks[r] * (dkt[I][4 * m] - S[r]), ks[r + 1] * (dkt[I][4 * m + 1] - S[r + 1]),
                                                           ks[r + 2] * (dkt[I][4 * m + 2] - S[r + 2]),
                                                           ks[r + 3] * (dkt[I][4 * m + 3] - S[r + 3]));
                }
            }
        }
    }
}

// block shares of dctx (the sum lands in share 0) + the per-(image, head) statistics
size_t linattn_bwd_ws_floats(int B, int n, int heads, int dh) {
    return (size_t)B * ((n + 63) / 64) * heads * dh * dh + (size_t)B * heads * 3 * dh;
}

template <int DH>
static int linear_attention_core_bwd(const float* qkv, const float* mem_kv, const float* ctx, const float* dout, float* ws,
                                     float* dqkv, float* dmem_part, int B, int n, int heads, hipStream_t s,
                                     const float* kstats) {
    const int nblk = (n + 63) / 64;
    const float scale = 1.0f / sqrtf((float)DH);
    float* stats = ws + (size_t)B * nblk * heads * DH * DH;
    const bool timed = prof::enabled();
    // per (image, head): a (tokens x DH) x (DH x DH) product is n * DH * DH multiply-adds
    const double bh = (double)B * heads, mm = 2.0 * bh * n * DH * DH;
    char name[64];
    if (timed) {  // dqs and the dctx shares; q, dout read, dq and the shares written
        snprintf(name, sizeof(name), "linattn_bwd_q_mfma_kernel<%d>", DH);
        if (prof::begin(name, 2.0 * mm, 4.0 * bh * (3.0 * n * DH + (1.0 + nblk) * DH * DH), s)) return 1;
    }
    hipLaunchKernelGGL(linattn_bwd_q_mfma_kernel<DH>, dim3(nblk, heads, B), dim3(64), 0, s, qkv, ctx, dout, dqkv, ws, n, heads,
                       scale);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    if (timed) {
        snprintf(name, sizeof(name), "linattn_bwd_stats_kernel<%d>", DH);
        if (prof::begin(name, bh * (nblk + 2.0 + 4.0 * NMEM) * DH * DH, 4.0 * bh * (nblk + 2.0) * DH * DH, s)) return 1;
    }
    hipLaunchKernelGGL(linattn_bwd_stats_kernel<DH>, dim3(heads, B), dim3(256), 0, s, mem_kv, ctx, ws, nblk, stats, dmem_part,
                       kstats, heads);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    if (timed) {  // dks and dv; k, v read, dk, dv written
        snprintf(name, sizeof(name), "linattn_bwd_kv_mfma_kernel<%d>", DH);
        if (prof::begin(name, 2.0 * mm, 4.0 * bh * (4.0 * n * DH + DH * DH), s)) return 1;
    }
    hipLaunchKernelGGL(linattn_bwd_kv_mfma_kernel<DH>, dim3(nblk, heads, B), dim3(64), 0, s, qkv, ws, nblk, stats, dqkv, n,
                       heads);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    return 0;
}

// qkv (B, n, 3*heads*dh), ctx (B, heads, dh, dh) as the forward core left it, dout (B, n, heads*dh) -> dqkv (same shape as
// qkv), dmem_part (B, 2, heads, dh, 4) per-image memory key/value gradients (the caller sums over B)
int launch_linear_attention_core_bwd(const float* qkv, const float* mem_kv, const float* ctx, const float* dout, float* ws,
                                     float* dqkv, float* dmem_part, int B, int n, int heads, int dh, hipStream_t s,
                                     const float* kstats) {
    DM_REQUIRE((dh == 32 || dh == 64) && heads >= 1 && heads <= 16, "linear attention backward: dim_head 32 or 64");
    DM_REQUIRE(B <= 65535 && n >= 1, "linear attention backward: batch");
    DM_REQUIRE(kstats, "linear attention backward: the key statistics of the forward context kernel");
    return dh == 32 ? linear_attention_core_bwd<32>(qkv, mem_kv, ctx, dout, ws, dqkv, dmem_part, B, n, heads, s, kstats)
                    : linear_attention_core_bwd<64>(qkv, mem_kv, ctx, dout, ws, dqkv, dmem_part, B, n, heads, s, kstats);
}

// ---------------------------------------------------------------------------------------
// Full attention: P = softmax_j(scale q_i k_j), o_i = sum_j P_ij v_j (keys = n_mem memory rows, then the nk key rows)
//   dP_ij = do_i . v_j;  D_i = do_i . o_i;  dS_ij = P_ij (dP_ij - D_i);  dq_i = scale sum_j dS_ij k_j;
//   dk_j = scale sum_i dS_ij q_i;  dv_j = sum_i P_ij do_i
// grid (heads, B); phase 1: thread = query (row statistics, dq); phase 2: thread = key (dk, dv), fixed order over queries.
// Self-attention (Attention :215-229): q, k, v are column blocks of one qkv tensor and 4 learned memory rows come first;
// cross-attention (DD/denoising_diffusion_text_conditional.py:54-78): k, v are projections of the text context, no memory.
// ---------------------------------------------------------------------------------------
// Phase 1 (thread = query) leaves the row statistics m_i, 1 / l_i, D_i; phase 2 (thread = key) forms the same scores and dP
// again and meets them.  Both must round alike, or P_ij is exp() of a difference that is not the one the statistics were
// taken over and dP_ij - D_i does not cancel where it should (one key: P = 1, dS = 0 exactly).  Left to the compiler the
// query side became an fma chain and the key side packed multiplies and adds, and `sc * scale - m` an fma on one side only.
// So: the dot products are explicit fma chains in d, and the softmax argument is the ROUNDED product minus the maximum.
__device__ __forceinline__ float score_minus(float sc, float scale, float m) {
#pragma clang fp contract(off)
    return sc * scale - m;
}
// The row statistics l_i = sum_j e_ij and D_i = sum_j e_ij dP_ij / l_i are compensated (Kahan) sums.  They were single fp32
// accumulators over all keys, and their rounding does not stay small where dq_i and dk_j cancel: with dS_ij = P_ij (dP_ij - D_i)
// the sum over j of dS_ij is D_i's and l_i's error, and it multiplies whatever the key rows share -- a common offset of k (k + 100
// on every token: the worst dq row was 2.4e-4 of the RMS row norm where the same arithmetic with exact sums gives 3e-5), or
// one key far larger than the others (4.8e-4 against 1.7e-5).  tests/test_hip_attn_cores.py holds both inputs.
__device__ __forceinline__ void kahan_add(float& sum, float& comp, float x) {
#pragma clang fp contract(off)
    const float y = x - comp;
    const float t = sum + y;
    comp = (t - sum) - y;
    sum = t;
}

struct AttnBwdParams {
    const float *q, *k, *v;      // rows of ldq / ldk floats per token, head h at column h * dh
    const float *mem_k, *mem_v;  // (heads, n_mem, dh) or nullptr
    const float* dout;           // (B, nq, heads * dh)
    float *dq, *dk, *dv;         // same strides as q / k / v
    float* dmem_part;            // (B, 2, heads, n_mem, dh) or nullptr
    int ldq, ldk, nq, nk, n_mem, heads;
    float scale;
};

template <int DH>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const AttnBwdParams p) {
    constexpr int LDH = bwd_log2_dh<DH>();
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int nkt = p.nk + p.n_mem, n = p.nq;
    float* Ks = sm;                       // [nkt][DH + 1]
    float* Vs = Ks + nkt * (DH + 1);     // [nkt][DH + 1]
    float* Qs = Vs + nkt * (DH + 1);     // [n][DH + 1]
    float* Ds = Qs + n * (DH + 1);       // [n][DH + 1]  dout
    float* rm = Ds + n * (DH + 1);       // [n] row max
    float* rl = rm + n;                   // [n] 1 / row sum
    float* rD = rl + n;                   // [n] D_i
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int hid = p.heads * DH;
    const float scale = p.scale;
    for (int i = tid; i < nkt * DH; i += 256) {
        const int j = i >> LDH, d = i & (DH - 1);
        float kv, vv;
        if (j < p.n_mem) {
            kv = p.mem_k[((size_t)h * p.n_mem + j) * DH + d];
            vv = p.mem_v[((size_t)h * p.n_mem + j) * DH + d];
        } else {
            const size_t row = ((size_t)b * p.nk + (j - p.n_mem)) * p.ldk + h * DH + d;
            kv = p.k[row];
            vv = p.v[row];
        }
        Ks[j * (DH + 1) + d] = kv;
        Vs[j * (DH + 1) + d] = vv;
    }
    for (int i = tid; i < n * DH; i += 256) {
        const int t = i >> LDH, d = i & (DH - 1);
        Qs[t * (DH + 1) + d] = p.q[((size_t)b * n + t) * p.ldq + h * DH + d];
        Ds[t * (DH + 1) + d] = p.dout[((size_t)b * n + t) * hid + h * DH + d];
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        float q[DH], dov[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            q[d] = Qs[i * (DH + 1) + d];
            dov[d] = Ds[i * (DH + 1) + d];
        }
        float m = -INFINITY, l = 0.f, D = 0.f, lc = 0.f, Dc = 0.f, linv;
        float dq[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) dq[d] = 0.f;
        for (int j = 0; j < nkt; ++j) {
            float sc = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) sc = fmaf(q[d], Ks[j * (DH + 1) + d], sc);
            m = fmaxf(m, sc * scale);
        }
        for (int j = 0; j < nkt; ++j) {
            float sc = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                sc = fmaf(q[d], Ks[j * (DH + 1) + d], sc);
                dp = fmaf(dov[d], Vs[j * (DH + 1) + d], dp);
            }
            const float e = __expf(score_minus(sc, scale, m));
            kahan_add(l, lc, e);
            kahan_add(D, Dc, e * dp);
        }
        linv = 1.0f / l;
        D *= linv;
        for (int j = 0; j < nkt; ++j) {
            float sc = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                sc = fmaf(q[d], Ks[j * (DH + 1) + d], sc);
                dp = fmaf(dov[d], Vs[j * (DH + 1) + d], dp);
            }
            const float dS = __expf(score_minus(sc, scale, m)) * linv * (dp - D);
#pragma unroll
            for (int d = 0; d < DH; ++d) dq[d] += dS * Ks[j * (DH + 1) + d];
        }
        rm[i] = m;
        rl[i] = linv;
        rD[i] = D;
        float* o = p.dq + ((size_t)b * n + i) * p.ldq + h * DH;
#pragma unroll
        for (int d = 0; d < DH; ++d) o[d] = scale * dq[d];
    }
    __syncthreads();
    for (int j = tid; j < nkt; j += 256) {
        float kk[DH], vv[DH], dk[DH], dv[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            kk[d] = Ks[j * (DH + 1) + d];
            vv[d] = Vs[j * (DH + 1) + d];
            dk[d] = 0.f;
            dv[d] = 0.f;
        }
        for (int i = 0; i < n; ++i) {
            float sc = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                sc = fmaf(Qs[i * (DH + 1) + d], kk[d], sc);
                dp = fmaf(Ds[i * (DH + 1) + d], vv[d], dp);
            }
            const float P = __expf(score_minus(sc, scale, rm[i])) * rl[i];
            const float dS = P * (dp - rD[i]);
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                dk[d] += dS * Qs[i * (DH + 1) + d];
                dv[d] += P * Ds[i * (DH + 1) + d];
            }
        }
        if (j < p.n_mem) {
            float* o = p.dmem_part + (size_t)b * 2 * p.heads * p.n_mem * DH;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                o[((size_t)h * p.n_mem + j) * DH + d] = scale * dk[d];
                o[((size_t)(p.heads + h) * p.n_mem + j) * DH + d] = dv[d];
            }
        } else {
            const size_t row = ((size_t)b * p.nk + (j - p.n_mem)) * p.ldk + h * DH;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                p.dk[row + d] = scale * dk[d];
                p.dv[row + d] = dv[d];
            }
        }
    }
}

// ---- short sequences (attn_bwd_cached: nq * (nk + n_mem) <= 4096), every phase spread over the 256 threads: the 16 tokens + 4
// memory rows of the 32x32 U-Net's bottleneck are 16 queries and 20 keys, so "thread = query" leaves 240 threads idle while 16
// of them walk 20 keys x three 32-wide dot products each (22 us at any batch).  Here (1) thread = (query, key) pair forms the
// score and dP, (2) thread = query normalises its row (no dot products left), (3) thread = (query, d) forms dq, (4) thread =
// (key, d) forms dk and dv. Every sum runs over the same index in the same order as attn_bwd_kernel's (d, then keys, then
// queries): identical results.
template <int DH>
__global__ __launch_bounds__(256) void attn_bwd_pairs_kernel(const AttnBwdParams p) {
    constexpr int LDH = bwd_log2_dh<DH>();
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int nkt = p.nk + p.n_mem, n = p.nq;
    float* Ks = sm;                       // [nkt][DH + 1]
    float* Vs = Ks + nkt * (DH + 1);     // [nkt][DH + 1]
    float* Qs = Vs + nkt * (DH + 1);     // [n][DH + 1]
    float* Ds = Qs + n * (DH + 1);       // [n][DH + 1]  dout
    float* Pc = Ds + n * (DH + 1) + 3 * n;  // after attn_bwd_kernel's layout (attn_bwd_lds_bytes' cache term)
    float* Sc = Pc + n * nkt;
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int hid = p.heads * DH;
    const float scale = p.scale;
    for (int i = tid; i < nkt * DH; i += 256) {
        const int j = i >> LDH, d = i & (DH - 1);
        float kv, vv;
        if (j < p.n_mem) {
            kv = p.mem_k[((size_t)h * p.n_mem + j) * DH + d];
            vv = p.mem_v[((size_t)h * p.n_mem + j) * DH + d];
        } else {
            const size_t row = ((size_t)b * p.nk + (j - p.n_mem)) * p.ldk + h * DH + d;
            kv = p.k[row];
            vv = p.v[row];
        }
        Ks[j * (DH + 1) + d] = kv;
        Vs[j * (DH + 1) + d] = vv;
    }
    for (int i = tid; i < n * DH; i += 256) {
        const int t = i >> LDH, d = i & (DH - 1);
        Qs[t * (DH + 1) + d] = p.q[((size_t)b * n + t) * p.ldq + h * DH + d];
        Ds[t * (DH + 1) + d] = p.dout[((size_t)b * n + t) * hid + h * DH + d];
    }
    __syncthreads();
    for (int idx = tid; idx < n * nkt; idx += 256) {  // (1) scores and dP
        const int i = idx / nkt, j = idx - i * nkt;
        float sc = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            sc += Qs[i * (DH + 1) + d] * Ks[j * (DH + 1) + d];
            dp += Ds[i * (DH + 1) + d] * Vs[j * (DH + 1) + d];
        }
        Pc[idx] = sc * scale;
        Sc[idx] = dp;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {  // (2) row softmax, D_i, dS
        float* Pi = Pc + i * nkt;
        float* Si = Sc + i * nkt;
        float m = -INFINITY, l = 0.f, D = 0.f, lc = 0.f, Dc = 0.f;
        for (int j = 0; j < nkt; ++j) m = fmaxf(m, Pi[j]);
        for (int j = 0; j < nkt; ++j) {
            const float e = __expf(Pi[j] - m);
            Pi[j] = e;
            kahan_add(l, lc, e);
            kahan_add(D, Dc, e * Si[j]);
        }
        const float linv = 1.0f / l;
        D *= linv;
        for (int j = 0; j < nkt; ++j) {
            const float P = Pi[j] * linv;
            Si[j] = P * (Si[j] - D);
            Pi[j] = P;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < n * DH; idx += 256) {  // (3) dq
        const int i = idx >> LDH, d = idx & (DH - 1);
        float dq = 0.f;
        for (int j = 0; j < nkt; ++j) dq += Sc[i * nkt + j] * Ks[j * (DH + 1) + d];
        p.dq[((size_t)b * n + i) * p.ldq + h * DH + d] = scale * dq;
    }
    for (int idx = tid; idx < nkt * DH; idx += 256) {  // (4) dk, dv
        const int j = idx >> LDH, d = idx & (DH - 1);
        float dk = 0.f, dv = 0.f;
        for (int i = 0; i < n; ++i) {
            dk += Sc[i * nkt + j] * Qs[i * (DH + 1) + d];
            dv += Pc[i * nkt + j] * Ds[i * (DH + 1) + d];
        }
        if (j < p.n_mem) {
            float* o = p.dmem_part + (size_t)b * 2 * p.heads * p.n_mem * DH;
            o[((size_t)h * p.n_mem + j) * DH + d] = scale * dk;
            o[((size_t)(p.heads + h) * p.n_mem + j) * DH + d] = dv;
        } else {
            const size_t row = ((size_t)b * p.nk + (j - p.n_mem)) * p.ldk + h * DH;
            p.dk[row + d] = scale * dk;
            p.dv[row + d] = dv;
        }
    }
}

// ---- the same gradients for sequences that do not fit LDS: two tiled kernels, one wave per 64 queries / 64 keys.
// attn_bwd_q_tiled_kernel   grid (ceil(nq / 64), heads, B): lane = query; the keys stream through LDS in tiles of 64 three
//     times (row maximum; row sum and D_i; dq) -- the three loops of attn_bwd_kernel's first phase; writes dq and the row
//     statistics (m_i, 1 / l_i, D_i) to stats[b][h][i][3].
// attn_bwd_kv_tiled_kernel  grid (ceil((nk + n_mem) / 64), heads, B): lane = key; the queries (q, dO, statistics) stream
//     through LDS in tiles of 64 in order: dk, dv, memory-row gradients.  Fixed summation order, no atomics.
template <int DH>
__device__ __forceinline__ void attn_load_key(const AttnBwdParams& p, int b, int h, int j, int d, float* kv, float* vv) {
    if (j < p.n_mem) {
        *kv = p.mem_k[((size_t)h * p.n_mem + j) * DH + d];
        *vv = p.mem_v[((size_t)h * p.n_mem + j) * DH + d];
    } else {
        const size_t row = ((size_t)b * p.nk + (j - p.n_mem)) * p.ldk + h * DH + d;
        *kv = p.k[row];
        *vv = p.v[row];
    }
}
template <int DH>
__global__ __launch_bounds__(64) void attn_bwd_q_tiled_kernel(const AttnBwdParams p, float* __restrict__ stats) {
    constexpr int LDH = bwd_log2_dh<DH>(), ATS = DH + 1;
    __shared__ float Ks[64 * ATS], Vs[64 * ATS];
    const int h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane, n = p.nq, nkt = p.nk + p.n_mem;
    const bool ok = i < n;
    const int hid = p.heads * DH;
    const float scale = p.scale;
    float q[DH], dov[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        q[d] = ok ? p.q[((size_t)b * n + i) * p.ldq + h * DH + d] : 0.f;
        dov[d] = ok ? p.dout[((size_t)b * n + i) * hid + h * DH + d] : 0.f;
    }
    float m = -INFINITY, l = 0.f, D = 0.f, lc = 0.f, Dc = 0.f, dq[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) dq[d] = 0.f;
    for (int pass = 0; pass < 3; ++pass) {
        float linv = 0.f;
        if (pass == 2) {
            linv = 1.0f / l;
            D *= linv;
        }
        for (int j0 = 0; j0 < nkt; j0 += 64) {
            __syncthreads();
            for (int e = lane; e < 64 * DH; e += 64) {
                const int jj = e >> LDH, d = e & (DH - 1);
                float kv = 0.f, vv = 0.f;
                if (j0 + jj < nkt) attn_load_key<DH>(p, b, h, j0 + jj, d, &kv, &vv);
                Ks[jj * ATS + d] = kv;
                Vs[jj * ATS + d] = vv;
            }
            __syncthreads();
            const int jn = min(64, nkt - j0);
            for (int jj = 0; jj < jn; ++jj) {
                float sc = 0.f, dp = 0.f;
#pragma unroll
                for (int d = 0; d < DH; ++d) {
                    sc = fmaf(q[d], Ks[jj * ATS + d], sc);
                    dp = fmaf(dov[d], Vs[jj * ATS + d], dp);
                }
                if (pass == 0) {
                    m = fmaxf(m, sc * scale);
                } else if (pass == 1) {
                    const float e = __expf(score_minus(sc, scale, m));
                    kahan_add(l, lc, e);
                    kahan_add(D, Dc, e * dp);
                } else {
                    const float dS = __expf(score_minus(sc, scale, m)) * linv * (dp - D);
#pragma unroll
                    for (int d = 0; d < DH; ++d) dq[d] += dS * Ks[jj * ATS + d];
                }
            }
        }
    }
    if (ok) {
        float* st = stats + (((size_t)b * p.heads + h) * n + i) * 3;
        st[0] = m;
        st[1] = 1.0f / l;
        st[2] = D;
        float* o = p.dq + ((size_t)b * n + i) * p.ldq + h * DH;
#pragma unroll
        for (int d = 0; d < DH; ++d) o[d] = scale * dq[d];
    }
}
template <int DH>
__global__ __launch_bounds__(64) void attn_bwd_kv_tiled_kernel(const AttnBwdParams p, const float* __restrict__ stats) {
    constexpr int LDH = bwd_log2_dh<DH>(), ATS = DH + 1;
    __shared__ float Qs[64 * ATS], Ds[64 * ATS], St[64 * 3];
    const int h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const int j = blockIdx.x * 64 + lane, n = p.nq, nkt = p.nk + p.n_mem;
    const bool ok = j < nkt;
    const int hid = p.heads * DH;
    const float scale = p.scale;
    float kk[DH], vv[DH], dk[DH], dv[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        kk[d] = vv[d] = 0.f;
        if (ok) attn_load_key<DH>(p, b, h, j, d, &kk[d], &vv[d]);
        dk[d] = dv[d] = 0.f;
    }
    for (int i0 = 0; i0 < n; i0 += 64) {
        __syncthreads();
        for (int e = lane; e < 64 * DH; e += 64) {
            const int ii = e >> LDH, d = e & (DH - 1);
            const bool in = i0 + ii < n;
            Qs[ii * ATS + d] = in ? p.q[((size_t)b * n + i0 + ii) * p.ldq + h * DH + d] : 0.f;
            Ds[ii * ATS + d] = in ? p.dout[((size_t)b * n + i0 + ii) * hid + h * DH + d] : 0.f;
        }
        for (int e = lane; e < 64 * 3; e += 64)
            St[e] = i0 + e / 3 < n ? stats[(((size_t)b * p.heads + h) * n + i0) * 3 + e] : 0.f;
        __syncthreads();
        const int in_ = min(64, n - i0);
        for (int ii = 0; ii < in_; ++ii) {
            float sc = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                sc = fmaf(Qs[ii * ATS + d], kk[d], sc);
                dp = fmaf(Ds[ii * ATS + d], vv[d], dp);
            }
            const float P = __expf(score_minus(sc, scale, St[3 * ii])) * St[3 * ii + 1];
            const float dS = P * (dp - St[3 * ii + 2]);
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                dk[d] += dS * Qs[ii * ATS + d];
                dv[d] += P * Ds[ii * ATS + d];
            }
        }
    }
    if (!ok) return;
    if (j < p.n_mem) {
        float* o = p.dmem_part + (size_t)b * 2 * p.heads * p.n_mem * DH;
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            o[((size_t)h * p.n_mem + j) * DH + d] = scale * dk[d];
            o[((size_t)(p.heads + h) * p.n_mem + j) * DH + d] = dv[d];
        }
    } else {
        const size_t row = ((size_t)b * p.nk + (j - p.n_mem)) * p.ldk + h * DH;
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            p.dk[row + d] = scale * dk[d];
            p.dv[row + d] = dv[d];
        }
    }
}

static bool attn_bwd_cached(int nq, int nk, int n_mem) {
    static const bool off = env_flag("DM_ATTN_BWD_NO_CACHE");  // A/B, and the tests' other path
    return !off && (size_t)nq * (nk + n_mem) <= 4096;
}
static size_t attn_bwd_lds_bytes(int nq, int nk, int n_mem, int dh) {
    const size_t cache = attn_bwd_cached(nq, nk, n_mem) ? (size_t)2 * nq * (nk + n_mem) : 0;
    return ((size_t)(2 * (nk + n_mem) + 2 * nq) * (dh + 1) + 3 * nq + cache) * sizeof(float);
}
static bool attn_bwd_tiled(int nq, int nk, int n_mem, int dh) {
    static const bool force = env_flag("DM_ATTN_BWD_TILED");  // tests: the tiled form on small shapes too
    return force || attn_bwd_lds_bytes(nq, nk, n_mem, dh) > 160 * 1024;
}
// floats of statistics workspace the tiled form needs (0 when the LDS-resident kernel takes the shape)
size_t attn_bwd_ws_floats(int B, int nq, int nk, int n_mem, int heads, int dh) {
    return attn_bwd_tiled(nq, nk, n_mem, dh) ? (size_t)B * heads * nq * 3 : 0;
}

template <int DH>
static int launch_attn_bwd(const AttnBwdParams& p, int B, float* ws, hipStream_t s) {
    const size_t lds = attn_bwd_lds_bytes(p.nq, p.nk, p.n_mem, DH);
    const bool timed = prof::enabled();
    // scores, dP, dq, dk, dv: 5 x (nq x nkt x DH) multiply-adds per (image, head) (the query / key phases each form the first
    // two); q, k, v, dout read and dq, dk, dv written once
    const double bh = (double)B * p.heads, nkt = p.nk + p.n_mem;
    const double mm = 2.0 * bh * p.nq * nkt * DH, bytes = 4.0 * bh * (3.0 * p.nq + 4.0 * p.nk) * DH;
    char name[64];
    if (attn_bwd_tiled(p.nq, p.nk, p.n_mem, DH)) {
        DM_REQUIRE(ws != nullptr, "attention backward: the tiled form needs its statistics workspace (attn_bwd_ws_floats)");
        DM_REQUIRE(B <= 65535 && p.heads <= 65535, "attention backward: batch");
        if (timed) {
            snprintf(name, sizeof(name), "attn_bwd_q_tiled_kernel<%d>", DH);
            if (prof::begin(name, 3.0 * mm, 0.5 * bytes, s)) return 1;
        }
        hipLaunchKernelGGL(attn_bwd_q_tiled_kernel<DH>, dim3((p.nq + 63) / 64, p.heads, B), dim3(64), 0, s, p, ws);
        DM_CHECK_HIP(hipGetLastError());
        if (timed && prof::end(s)) return 1;
        if (timed) {
            snprintf(name, sizeof(name), "attn_bwd_kv_tiled_kernel<%d>", DH);
            if (prof::begin(name, 4.0 * mm, 0.5 * bytes, s)) return 1;
        }
        hipLaunchKernelGGL(attn_bwd_kv_tiled_kernel<DH>, dim3((p.nk + p.n_mem + 63) / 64, p.heads, B), dim3(64), 0, s, p, ws);
        DM_CHECK_HIP(hipGetLastError());
        if (timed && prof::end(s)) return 1;
        return 0;
    }
    if (attn_bwd_cached(p.nq, p.nk, p.n_mem)) {
        static LdsOptIn flagp;
        if (lds_opt_in(flagp, reinterpret_cast<const void*>(attn_bwd_pairs_kernel<DH>), 1)) return 1;
        if (timed) {
            snprintf(name, sizeof(name), "attn_bwd_pairs_kernel<%d>", DH);
            if (prof::begin(name, 5.0 * mm, bytes, s)) return 1;
        }
        hipLaunchKernelGGL(attn_bwd_pairs_kernel<DH>, dim3(p.heads, B), dim3(256), lds, s, p);
        DM_CHECK_HIP(hipGetLastError());
        if (timed && prof::end(s)) return 1;
        return 0;
    }
    static LdsOptIn flag;
    if (lds_opt_in(flag, reinterpret_cast<const void*>(attn_bwd_kernel<DH>), 1)) return 1;
    if (timed) {
        snprintf(name, sizeof(name), "attn_bwd_kernel<%d>", DH);
        if (prof::begin(name, 7.0 * mm, bytes, s)) return 1;
    }
    hipLaunchKernelGGL(attn_bwd_kernel<DH>, dim3(p.heads, B), dim3(256), lds, s, p);
    DM_CHECK_HIP(hipGetLastError());
    if (timed && prof::end(s)) return 1;
    return 0;
}

// qkv (B, n, 3*heads*dh), dout (B, n, heads*dh) -> dqkv, dmem_part (B, 2, heads, 4, dh)
int launch_attention_core_bwd(const float* qkv, const float* mem_kv, const float* dout, float* dqkv, float* dmem_part, float* ws,
                              int B, int n, int heads, int dh, hipStream_t s) {
    DM_REQUIRE(dh == 32 || dh == 64, "attention backward: dim_head 32 or 64");
    const int hid = heads * dh;
    AttnBwdParams p{};
    p.q = qkv; p.k = qkv + hid; p.v = qkv + 2 * hid;
    p.mem_k = mem_kv; p.mem_v = mem_kv + (size_t)heads * NMEM * dh;
    p.dout = dout;
    p.dq = dqkv; p.dk = dqkv + hid; p.dv = dqkv + 2 * hid;
    p.dmem_part = dmem_part;
    p.ldq = p.ldk = 3 * hid; p.nq = p.nk = n; p.n_mem = NMEM; p.heads = heads;
    p.scale = 1.0f / sqrtf((float)dh);
    return dh == 32 ? launch_attn_bwd<32>(p, B, ws, s) : launch_attn_bwd<64>(p, B, ws, s);
}

// CrossAttention core: q (B, nq, heads*dh), k / v (B, m, heads*dh) projections of the context -> dq, dk, dv (same shapes)
int launch_cross_attention_core_bwd(const float* q, const float* k, const float* v, const float* dout, float* dq, float* dk,
                                    float* dv, float* ws, int B, int nq, int m, int heads, int dh, hipStream_t s) {
    DM_REQUIRE(dh == 32 || dh == 64, "attention backward: dim_head 32 or 64");
    AttnBwdParams p{};
    p.q = q; p.k = k; p.v = v;
    p.dout = dout;
    p.dq = dq; p.dk = dk; p.dv = dv;
    p.ldq = p.ldk = heads * dh; p.nq = nq; p.nk = m; p.n_mem = 0; p.heads = heads;
    p.scale = 1.0f / sqrtf((float)dh);
    return dh == 32 ? launch_attn_bwd<32>(p, B, ws, s) : launch_attn_bwd<64>(p, B, ws, s);
}

}  // namespace dm
