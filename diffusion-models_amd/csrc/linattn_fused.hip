// Fused LinearAttention for gfx950 (DD/denoising_diffusion.py:150-192, called as `attn(x) + x` at :360/:383).
//
// The unfused path (RMSNorm kernel -> to_qkv 1x1 conv -> context kernel -> out kernel -> to_out conv) moves the
// (B, n, 384) qkv tensor through HBM twice and the (B, n, 128) attention output once more: ~1.5 GB per layer at
// 32x32 / batch 256 for ~27 GFLOP of work.  Here the whole layer is two kernels that read x twice and write y once:
//
//   1. linattn_ctx_fused_kernel   (token block, image): k, v = W_k x^, W_v x^ on the MFMA, exp, and the per-head
//      32x32 context  ctx[d][e] += sum_t exp(k[d][t] - bound[d]) v[e][t]  plus the softmax denominators, written
//      as per-block partial sums.  x^ = RMSNorm(x) has unit length before the gain, and the gain g*sqrt(C) is folded
//      into the weights on the host, so |k[d][t]| <= ||W'_k[d]||_2 =: bound[d] (Cauchy-Schwarz).  softmax is
//      invariant to the shift, so the bound replaces the running maximum: no max pass over the tokens, and partial
//      sums of different token blocks simply add.  (Layers whose bound exceeds 40 -- exp(-2*bound) must stay a
//      normal float -- keep the unfused path.)
//   (a tiny kernel sums the block partials, divides by the denominators and folds the context into to_out:
//    z = W_out (ctx^T q) = (W_out ctx^T) q =: M q with M (C x 32) per image and head, packed in lane order)
//   1'. linattn_ctx_image_kernel  (image): the form of kernel 1 for batches that fill the chip (la_image_form).  One
//      workgroup walks all tokens of its image through a double-buffered LDS window, so there are no partial sums and
//      no reduce launch: it finishes the image itself and writes M.  It also folds W_v into the context the way W_out
//      is folded on the output side: ctx = W'_v P with P[d][c] = sum_t a[d][t] rn_t x[t][c], so the token loop forms
//      k and P only (C/2 + C/2 MFMAs per 32-token tile instead of C/2 + C/2 + 16) and W'_v is applied once per image.
//   2. linattn_out_fused_kernel  (token block, image): q = W_q x^, softmax over dim_head, z = M q + b,
//      RMSNorm(z) * g, + x, one store.
//   2'. linattn_out_headsum_kernel  (run of token windows, image): the form of kernel 2 from B = 32 on
//      (la_out_headsum_form).  The waves exchange the softmaxed q through LDS and the sum over heads runs as one MFMA
//      chain per output column tile; the operands stay in registers over a run of windows.
//
// MFMA bookkeeping (v_mfma_f32_32x32x2_f32, wave = head): the accumulator of one product is used DIRECTLY as an
// operand of the next one, without any data movement: accumulator register e of lane (l, half) is element
// (row (e&3) + 8(e>>2) + 4*half, column l).  Taking MFMA step e of the next product to reduce over exactly that
// row pair (one row from each lane half) makes acc[e] the B operand (or, for the transposed products of kernel 1,
// the A operand) of step e.  The remaining operands (projection weights, context, W_out) are packed on the host in
// lane order and sit in registers.
#include "conv_device.h"

#include <cmath>
#include <type_traits>
#include <vector>

namespace dm {

static constexpr int LA_DH = 32;
static constexpr int LA_HEADS = 4;
static constexpr int LA_HID = LA_DH * LA_HEADS;
static constexpr int LA_CTX = LA_DH * LA_DH + LA_DH;  // partial context + partial denominators per (image, block, head)
static constexpr int LA_TOK1 = 128;                   // tokens per workgroup, kernel 1 (C = 128; 256 for C = 64)
__host__ __device__ constexpr int la_tok1(int C) { return C <= 64 ? 256 : LA_TOK1; }
static constexpr int LA_TOK2 = 64;                    // tokens per workgroup, kernel 2
static constexpr int LA_TOKI = 128;                   // tokens per LDS window, per-image form of kernel 1

__host__ __device__ static inline int la_row_of(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

bool linattn_fused_eligible(int C, int heads, int dh) {
    static const bool off = env_flag("DM_NO_FUSED_LINATTN");
    return !off && heads == LA_HEADS && dh == LA_DH && (C == 64 || C == 128);
}

// Host-side packing.  w_qkv is (3*128, C) with rows [q | k | v] x (head, d); norm_g (C); w_out (C, 128);
// mem_kv (2, heads, 32, 4).  Returns false when a softmax bound is too large for the shift trick.
bool linattn_fused_pack(const float* w_qkv, const float* norm_g, const float* w_out, const float* mem_kv, int C,
                        std::vector<float>& wq, std::vector<float>& wk, std::vector<float>& wv, std::vector<float>& wo,
                        std::vector<float>& kbound) {
    const int G = C / 8;
    const float sq = std::sqrt((float)C);
    auto pack_proj = [&](int which, std::vector<float>& dst) {
        // [head][g][lane = half*32 + l][4]: W'[head*32 + l][8g + 4*half + s],  W' = W * g * sqrt(C) per input channel
        dst.assign((size_t)LA_HEADS * G * 64 * 4, 0.f);
        for (int h = 0; h < LA_HEADS; ++h)
            for (int g = 0; g < G; ++g)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s) {
                        const int l = lane & 31, half = lane >> 5;
                        const int row = which * LA_HID + h * LA_DH + l, c = 8 * g + 4 * half + s;
                        dst[(((size_t)h * G + g) * 64 + lane) * 4 + s] = w_qkv[(size_t)row * C + c] * (norm_g[c] * sq);
                    }
    };
    pack_proj(0, wq);
    pack_proj(1, wk);
    pack_proj(2, wv);
    wo.clear();  // to_out is folded with the per-image context on the device (linattn_ctx_reduce_kernel)
    (void)w_out;
    kbound.assign(LA_HID, 0.f);
    bool ok = true;
    for (int h = 0; h < LA_HEADS; ++h)
        for (int d = 0; d < LA_DH; ++d) {
            double ss = 0;
            for (int c = 0; c < C; ++c) {
                const double v = (double)w_qkv[(size_t)(LA_HID + h * LA_DH + d) * C + c] * norm_g[c] * sq;
                ss += v * v;
            }
            float bnd = (float)(std::sqrt(ss) * 1.0001);
            for (int j = 0; j < 4; ++j) bnd = std::fmax(bnd, mem_kv[((size_t)h * LA_DH + d) * 4 + j]);
            kbound[h * LA_DH + d] = bnd;
            if (!(bnd < 40.f)) ok = false;
        }
    return ok;
}

size_t linattn_fused_ws_floats(int B, int n) {
    const int nblk = (n + LA_TOK1 - 1) / LA_TOK1;  // upper bound over C
    // per-block partial contexts, then M = W_out ctx^T per (image, head) packed as the A operand of kernel 2 (C <= 128)
    return (size_t)B * nblk * LA_HEADS * LA_CTX + (size_t)B * LA_HEADS * 128 * LA_DH;
}

// x rows [t0, t0 + TOK) of image b -> LDS (zero rows past the image), rn[t] = 1 / max(||x_t||, 1e-12)
template <int C, int TOK>
__device__ __forceinline__ void la_stage_rows(const float* __restrict__ xb, int nt, float* xs, float* rn) {
    constexpr int XS = C + 4, Q = C / 4;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < TOK * Q / 256; ++i) {
        const int it = tid + 256 * i;
        const int row = it / Q, q = it - row * Q;
        f32x4 v = make_f32x4(0.f, 0.f, 0.f, 0.f);
        if (row < nt) v = *reinterpret_cast<const f32x4*>(xb + (size_t)row * C + 4 * q);
        *reinterpret_cast<f32x4*>(xs + row * XS + 4 * q) = v;
    }
    __syncthreads();
    if (tid < TOK) {
        float ss = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(xs + tid * XS + 4 * q);
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        rn[tid] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    }
}

template <int C, int TOK>
__global__ __launch_bounds__(256) void linattn_ctx_fused_kernel(const float* __restrict__ x, const LinAttnFused w,
                                                                float* __restrict__ ws, int n, int nblk) {
    constexpr int G = C / 8, XS = C + 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;
    float* rn = smem + TOK * XS;
    const int blk = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, h = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int t0 = blk * TOK;
    const int nt = min(TOK, n - t0);

    f32x4 wk[G], wv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        wk[g] = *reinterpret_cast<const f32x4*>(w.wk + (((size_t)h * G + g) * 64 + lane) * 4);
        wv[g] = *reinterpret_cast<const f32x4*>(w.wv + (((size_t)h * G + g) * 64 + lane) * 4);
    }
    const float kb = w.kbound[h * LA_DH + l31];
    la_stage_rows<C, TOK>(x + ((size_t)b * n + t0) * C, nt, xs, rn);
    __syncthreads();

    f32x16 cacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) cacc[e] = 0.f;
    float ksum = 0.f;
    if (blk == 0) {
        // the 4 learned memory tokens (mem_kv, :159/:182-183): two MFMA steps, token j + half per lane half
        const float* mk = w.mem_kv + (size_t)h * LA_DH * 4;               // [d][j]
        const float* mv = w.mem_kv + (size_t)(LA_HEADS + h) * LA_DH * 4;  // [e][j]
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            const float a = __expf(mk[l31 * 4 + j + lh] - kb);
            ksum += a;
            cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, mv[l31 * 4 + j + lh], cacc, 0, 0, 0);
        }
    }
    for (int st = 0; st < TOK / 32; ++st) {
        if (st * 32 >= nt) break;
        // k^T, v^T (tokens x d) = x (tokens x C) W'^T: A = x row of token l31 from LDS, B = weights in registers
        f32x16 kacc, vacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            kacc[e] = 0.f;
            vacc[e] = 0.f;
        }
        const float* xr = xs + (st * 32 + l31) * XS + 4 * lh;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(xr + 8 * g);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                kacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], wk[g][s], kacc, 0, 0, 0);
                vacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], wv[g][s], vacc, 0, 0, 0);
            }
        }
        // register e holds token st*32 + row_of(e, lh), channel d = l31 (k) / e = l31 (v): exactly the operands of
        // step e of  ctx[d][e] += sum_t a[d][t] v[t][e]
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const f32x4 r4 = *reinterpret_cast<const f32x4*>(rn + st * 32 + 8 * m + 4 * lh);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 4 * m + i;
                const bool valid = st * 32 + 8 * m + 4 * lh + i < nt;
                const float a = valid ? __expf(kacc[e] * r4[i] - kb) : 0.f;
                ksum += a;
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, vacc[e] * r4[i], cacc, 0, 0, 0);
            }
        }
    }
    float* cp = ws + (((size_t)b * nblk + blk) * LA_HEADS + h) * LA_CTX;
#pragma unroll
    for (int e = 0; e < 16; ++e) cp[la_row_of(e, lh) * LA_DH + l31] = cacc[e];
    ksum += __shfl_xor(ksum, 32);
    if (lh == 0) cp[LA_DH * LA_DH + l31] = ksum;
}

// Sum the per-block partial contexts in block order, divide by the softmax denominator (k.softmax(dim=-1), :186), and
// fold the result into to_out: out = ctx^T q (:189) followed by z = W_out[:, head] out (:191) is z = M q with
// M[c][d] = sum_e W_out[c][head*32 + e] ctx[d][e].  M is stored in the lane order kernel 2 consumes as an MFMA A
// operand: [image][head][mt][e>>2][lane][e&3] = M[32*mt + l][row_of(e, half)].
template <int C>
__global__ __launch_bounds__(256) void linattn_ctx_reduce_kernel(const float* __restrict__ ws,
                                                                 const float* __restrict__ w_out,
                                                                 float* __restrict__ mz, int nblk) {
    constexpr int MT = C / 32;
    __shared__ float cs[LA_DH][LA_DH + 1];  // normalised context [d][e]
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, e4 = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int d = 8 * e4 + 4 * lh + i;  // every (d, e = l31) once
        float c = 0.f, k = 0.f;
        // the partial sums of the token blocks are independent loads: keep 8 of them in flight (at 64x64 there are 16-32
        // blocks per image and only heads x images workgroups, so this loop is a latency chain otherwise)
#pragma unroll 8
        for (int kb = 0; kb < nblk; ++kb) {
            const float* cp = ws + (((size_t)b * nblk + kb) * LA_HEADS + h) * LA_CTX;
            c += cp[d * LA_DH + l31];
            k += cp[LA_DH * LA_DH + d];
        }
        cs[d][l31] = c / k;
    }
    __syncthreads();
    // M^T (d x c) = ctx (d x e) W_out[:, head]^T (e x c) on the MFMA, one 32-channel column tile per wave: the
    // accumulator layout (row d on the registers, column c on the lanes) IS the packed layout
    const int mt = e4;
    if (mt < MT) {
        const float* wr = w_out + (size_t)(32 * mt + l31) * LA_HID + h * LA_DH;  // W_out[c][head*32 .. +32)
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int st = 0; st < 16; ++st)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cs[l31][2 * st + lh], wr[2 * st + lh], acc, 0, 0, 0);
        float* op = mz + ((((size_t)b * LA_HEADS + h) * MT + mt) * 4) * 64 * 4 + lane * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<f32x4*>(op + q * 64 * 4) = make_f32x4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
    }
}

// ---------------------------------------------------------------------------------------
// The per-image form of kernel 1: one workgroup of 8 waves walks ALL tokens of its image, wave = (head, token half).
// ---------------------------------------------------------------------------------------
// x rows [t0, t0 + TOK) of one image -> registers of a workgroup of NT threads.  Rows past the image read the image's
// last row (always in bounds) and are zeroed, so the LDS window never holds anything but finite numbers.
template <int C, int TOK = LA_TOKI, int NT = 512>
__device__ __forceinline__ void la_image_load(const float* __restrict__ xb, int t0, int n,
                                              f32x4 (&pre)[TOK * (C / 4) / NT]) {
    constexpr int Q = C / 4;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < TOK * Q / NT; ++i) {
        const int it = tid + NT * i;
        const int row = it / Q, q = it - row * Q;
        const int t = t0 + row;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xb + (size_t)min(t, n - 1) * C + 4 * q);
        pre[i] = t < n ? v : make_f32x4(0.f, 0.f, 0.f, 0.f);
    }
}

// Sums over the Q consecutive lanes that hold one row, in every one of them, for N independent values.  The same pairs
// in the same order as the __shfl_xor butterfly, so the same bits, but on the DPP path (one v_add_f32_dpp per step, no
// LDS round trip): xor 1 and xor 2 are quad permutes, and once a group of 4 (8) lanes agrees, the mirrored lane of the
// 8 (16) holds what lane ^ 4 (lane ^ 8) holds.  Only the step across 16-lane rows goes through ds_bpermute.  The steps
// are the outer loop so that the N chains fill each other's DPP wait states.
template <int CTRL, int N>
__device__ __forceinline__ void la_dpp_add(float (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
        v[i] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[i]), CTRL, 0xF, 0xF, false));
}
template <int Q, int N>
__device__ __forceinline__ void la_row_sums(float (&v)[N]) {
    static_assert(Q == 16 || Q == 32, "a row is 16 or 32 lanes");
    la_dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
    la_dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
    la_dpp_add<0x141>(v);  // row_half_mirror
    la_dpp_add<0x140>(v);  // row_mirror
    if (Q == 32) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], 16);
    }
}

// registers -> LDS window, rn[t] = 1 / max(||x_t||, 1e-12) (the Q lanes that hold one row are consecutive); with SS
// (kernel 2, head-sum form) rn[t] = ||x_t||^2 and the reader takes the root, once per tile instead of once per store
template <int C, int TOK = LA_TOKI, int NT = 512, bool SS = false>
__device__ __forceinline__ void la_image_store(const f32x4 (&pre)[TOK * (C / 4) / NT], float* xs, float* rn) {
    constexpr int XS = C + 4, Q = C / 4, N = TOK * Q / NT;
    const int tid = threadIdx.x;
    if (SS) {
        float ss[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int it = tid + NT * i;
            const int row = it / Q, q = it - row * Q;
            const f32x4 v = pre[i];
            *reinterpret_cast<f32x4*>(xs + row * XS + 4 * q) = v;
            ss[i] = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        la_row_sums<Q>(ss);
        if (tid % Q == 0) {
#pragma unroll
            for (int i = 0; i < N; ++i) rn[(tid + NT * i) / Q] = ss[i];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int it = tid + NT * i;
        const int row = it / Q, q = it - row * Q;
        const f32x4 v = pre[i];
        *reinterpret_cast<f32x4*>(xs + row * XS + 4 * q) = v;
        float ss = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
#pragma unroll
        for (int o = 1; o < Q; o <<= 1) ss += __shfl_xor(ss, o);
        if (q == 0) rn[row] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    }
}

// ctx[d][e] = sum_t a[d][t] v[e][t] is linear in v = W'_v (rn_t x_t), so the token loop accumulates
//   P^T[c][d] = sum_t x[t][c] (a[d][t] rn_t)                      (C/32 column tiles of 32 x 32 per head)
// and W'_v is applied once per image: ctx^T = W'_v P^T.  A tile costs C/2 MFMAs for k and C/2 for P^T instead of
// C/2 + C/2 + 16, and no v is ever formed.  Operands: step e of P^T takes A = x[token row_of(e, half)][32 ct + l31]
// (one ds_read_b32: each lane half reads 32 consecutive floats of one row, conflict-free) and B = a rn from k's
// accumulator register e; P^T's accumulator register e (row c = 32 ct + row_of(e, half), column d) is the B operand of
// step (ct, e) of ctx^T = W'_v P^T, whose A operand W'_v[head*32 + l31][8 g + 4 half + s], g = 4 ct + (e >> 2), s = e & 3,
// is the projection packing as it stands; and ctx^T's accumulator register e (ctx[d = l31][e = row_of(e, half)]) is the
// A operand of step e of M^T = ctx W_out[:, head]^T, which leaves M in the order kernel 2 reads.
//
// Token blocks of LA_TOKI rows go through two LDS windows: the rows of block i+1 are loaded into registers before the
// products of block i and written to the other window after them, one barrier per block.  Inside a block wave
// (head, half) takes the 32-token tiles half and half + 2.  The two halves are added through LDS in a fixed order, then
// the half-0 wave of each head adds the memory tokens, divides by the denominators and writes M: the summation order
// of an image depends on n alone, never on B or on where the image sits in the batch.
template <int C>
__global__ __launch_bounds__(512) void linattn_ctx_image_kernel(const float* __restrict__ x, const LinAttnFused w,
                                                                float* __restrict__ mz, int n) {
    constexpr int G = C / 8, XS = C + 4, CT = C / 32, TB = LA_TOKI, NP = TB * (C / 4) / 512;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* rnb = smem + 2 * TB * XS;  // [2][TB]
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int h = wid & 3, th = wid >> 2;  // the two halves of a head share a SIMD
    const int l31 = lane & 31, lh = lane >> 5;
    const float* xb = x + (size_t)b * n * C;
    const int nb = (n + TB - 1) / TB;

    f32x4 wk[G];
#pragma unroll
    for (int g = 0; g < G; ++g) wk[g] = *reinterpret_cast<const f32x4*>(w.wk + (((size_t)h * G + g) * 64 + lane) * 4);
    const float kb = w.kbound[h * LA_DH + l31];

    f32x4 pre[NP];
    la_image_load<C>(xb, 0, n, pre);
    la_image_store<C>(pre, smem, rnb);
    __syncthreads();

    f32x16 pacc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) pacc[ct][e] = 0.f;
    float ksum = 0.f;
    for (int blk = 0; blk < nb; ++blk) {
        const bool more = blk + 1 < nb;
        if (more) la_image_load<C>(xb, (blk + 1) * TB, n, pre);
        const float* xs = smem + (blk & 1) * TB * XS;
        const float* rn = rnb + (blk & 1) * TB;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int tb = 32 * (th + 2 * j);  // first row of the tile inside the window
            const int nt = n - blk * TB - tb;  // valid tokens from there on
            if (nt <= 0) break;
            // k^T (tokens x d) = x (tokens x C) W'_k^T: A = x row of token l31 from LDS, B = weights in registers
            f32x16 kacc;
#pragma unroll
            for (int e = 0; e < 16; ++e) kacc[e] = 0.f;
            const float* xr = xs + (tb + l31) * XS + 4 * lh;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(xr + 8 * g);
#pragma unroll
                for (int s = 0; s < 4; ++s) kacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], wk[g][s], kacc, 0, 0, 0);
            }
            const float* xc = xs + (tb + 4 * lh) * XS + l31;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x4 r4 = *reinterpret_cast<const f32x4*>(rn + tb + 8 * m + 4 * lh);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = 4 * m + i;
                    const bool valid = 8 * m + 4 * lh + i < nt;
                    const float a = valid ? __expf(kacc[e] * r4[i] - kb) : 0.f;
                    ksum += a;
                    const float ar = a * r4[i];
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct)
                        pacc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[(8 * m + i) * XS + 32 * ct], ar, pacc[ct], 0, 0, 0);
                }
            }
        }
        if (more) la_image_store<C>(pre, smem + ((blk + 1) & 1) * TB * XS, rnb + ((blk + 1) & 1) * TB);
        __syncthreads();  // the next window is written; this one may be rewritten after the next block's products
    }

    // token half 1 -> LDS (the windows are free behind the loop's last barrier), [head][ct][e][lane]
    float* cps = smem + (size_t)h * CT * 16 * 64 + lane;
    float* cks = smem + LA_HEADS * CT * 16 * 64 + h * 64 + lane;
    if (th == 1) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int e = 0; e < 16; ++e) cps[(ct * 16 + e) * 64] = pacc[ct][e];
        *cks = ksum;
    }
    __syncthreads();
    if (th == 1) return;

    ksum += *cks;
    f32x16 tacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) tacc[e] = 0.f;
    {
        // the 4 learned memory tokens (mem_kv, :159/:182-183), once per image: token j + half per lane half
        const float* mk = w.mem_kv + (size_t)h * LA_DH * 4;               // [d][j]
        const float* mv = w.mem_kv + (size_t)(LA_HEADS + h) * LA_DH * 4;  // [e][j]
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            const float a = __expf(mk[l31 * 4 + j + lh] - kb);
            ksum += a;
            tacc = __builtin_amdgcn_mfma_f32_32x32x2f32(mv[l31 * 4 + j + lh], a, tacc, 0, 0, 0);
        }
    }
    // ctx^T (e x d) += W'_v (e x C) P^T (C x d)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w.wv + (((size_t)h * G + 4 * ct + q) * 64 + lane) * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 4 * q + i;
                tacc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[i], pacc[ct][e] + cps[(ct * 16 + e) * 64], tacc, 0, 0, 0);
            }
        }
    // softmax denominator of column d = l31 (k.softmax(dim=-1), :186)
    ksum += __shfl_xor(ksum, 32);
#pragma unroll
    for (int e = 0; e < 16; ++e) tacc[e] = tacc[e] / ksum;
    // M^T (d x c) = ctx (d x e) W_out[:, head]^T (e x c), stored as linattn_ctx_reduce_kernel stores it
#pragma unroll
    for (int mt = 0; mt < CT; ++mt) {
        const float* wr = w.wo_raw + (size_t)(32 * mt + l31) * LA_HID + h * LA_DH + 4 * lh;
        f32x16 macc;
#pragma unroll
        for (int e = 0; e < 16; ++e) macc[e] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 wo = *reinterpret_cast<const f32x4*>(wr + 8 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) macc = __builtin_amdgcn_mfma_f32_32x32x2f32(tacc[4 * q + i], wo[i], macc, 0, 0, 0);
        }
        float* op = mz + ((((size_t)b * LA_HEADS + h) * CT + mt) * 4) * 64 * 4 + lane * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<f32x4*>(op + q * 64 * 4) =
                make_f32x4(macc[4 * q], macc[4 * q + 1], macc[4 * q + 2], macc[4 * q + 3]);
    }
}

template <int C>
__global__ __launch_bounds__(256) void linattn_out_fused_kernel(const float* __restrict__ x, const LinAttnFused w,
                                                                const float* __restrict__ mz, float* __restrict__ y,
                                                                int n, int add_x, float scale) {
    constexpr int G = C / 8, XS = C + 4, TOK = LA_TOK2, MT = C / 32, Q = C / 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;                  // [TOK][XS]
    float* rn = smem + TOK * XS;       // [TOK]
    float* zb = rn + TOK;              // [heads][32][XS]
    const int blk = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, h = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int t0 = blk * TOK;
    const int nt = min(TOK, n - t0);

    f32x4 wq[G];
#pragma unroll
    for (int g = 0; g < G; ++g) wq[g] = *reinterpret_cast<const f32x4*>(w.wq + (((size_t)h * G + g) * 64 + lane) * 4);
    // M of this image / head: the A operand of z = M q, loaded once
    f32x4 mreg[MT][4];
    {
        const float* mzp = mz + ((size_t)b * LA_HEADS + h) * MT * 4 * 64 * 4 + lane * 4;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) mreg[mt][e4] = *reinterpret_cast<const f32x4*>(mzp + (mt * 4 + e4) * 64 * 4);
    }
    la_stage_rows<C, TOK>(x + ((size_t)b * n + t0) * C, nt, xs, rn);
    __syncthreads();

    for (int st = 0; st < TOK / 32; ++st) {
        if (st * 32 >= nt) break;
        // q (d x tokens) = W'_q (d x C) x^T: A = weights in registers, B = x row of token l31 from LDS
        f32x16 qacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) qacc[e] = 0.f;
        const float* xr = xs + (st * 32 + l31) * XS + 4 * lh;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(xr + 8 * g);
#pragma unroll
            for (int s = 0; s < 4; ++s) qacc = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[g][s], a[s], qacc, 0, 0, 0);
        }
        // softmax over d (:185) for token l31: 16 values here, 16 in the other lane half; then * scale (:188)
        const float r = rn[st * 32 + l31];
        float m = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            qacc[e] *= r;
            m = fmaxf(m, qacc[e]);
        }
        m = fmaxf(m, __shfl_xor(m, 32));
        float ssum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            qacc[e] = __expf(qacc[e] - m);
            ssum += qacc[e];
        }
        ssum += __shfl_xor(ssum, 32);
        const float inv = scale / ssum;
        // this head's share of z (C x tokens) = M q: the B operand of step e is q's accumulator register e
#pragma unroll
        for (int e = 0; e < 16; ++e) qacc[e] *= inv;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            f32x16 zacc;
#pragma unroll
            for (int e = 0; e < 16; ++e) zacc[e] = 0.f;
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    zacc = __builtin_amdgcn_mfma_f32_32x32x2f32(mreg[mt][e4][i], qacc[4 * e4 + i], zacc, 0, 0, 0);
            }
            // register e = channel 32*mt + row_of(e, lh) of token l31: four consecutive channels per b128 store
            float* zr = zb + (h * 32 + l31) * XS + 32 * mt + 4 * lh;
#pragma unroll
            for (int m4 = 0; m4 < 4; ++m4)
                *reinterpret_cast<f32x4*>(zr + 8 * m4) =
                    make_f32x4(zacc[4 * m4], zacc[4 * m4 + 1], zacc[4 * m4 + 2], zacc[4 * m4 + 3]);
        }
        __syncthreads();
        // sum over heads, + bias, RMSNorm over channels (to_out[1], :170), + x, store
#pragma unroll
        for (int i = 0; i < 32 * Q / 256; ++i) {
            const int it = tid + 256 * i;
            const int tok = it / Q, q4 = it - tok * Q;
            f32x4 z = *reinterpret_cast<const f32x4*>(w.bias + 4 * q4);
#pragma unroll
            for (int hh = 0; hh < LA_HEADS; ++hh) z += *reinterpret_cast<const f32x4*>(zb + (hh * 32 + tok) * XS + 4 * q4);
            float ss = z.x * z.x + z.y * z.y + z.z * z.z + z.w * z.w;
#pragma unroll
            for (int o = 1; o < Q; o <<= 1) ss += __shfl_xor(ss, o);  // the Q lanes of a token are consecutive
            z = z * fast_rsq(fmaxf(ss, 1e-24f)) * *reinterpret_cast<const f32x4*>(w.og + 4 * q4);
            if (add_x) z += *reinterpret_cast<const f32x4*>(xs + (st * 32 + tok) * XS + 4 * q4);
            if (st * 32 + tok < nt)
                *reinterpret_cast<f32x4*>(y + ((size_t)b * n + t0 + st * 32 + tok) * C + 4 * q4) = z;
        }
        __syncthreads();  // zb is rewritten by the next token tile
    }
}

// ---------------------------------------------------------------------------------------
// The head-sum form of kernel 2: z = sum_h M_h p_h is ONE product with K = heads * 32, so the sum over heads runs on
// the MFMA instead of through four C x 32 LDS buffers and the vector ALUs.
// ---------------------------------------------------------------------------------------
// A workgroup walks a run of token windows of one image (LA_OUTW floats of x per window: 64 tokens at C = 64, 32 at
// C = 128) with every operand resident in registers: W'_q of its head, M of its output column tile for all four heads,
// bias and gain.  Per window:
//   A. wave h forms q_h = W'_q x^ and the softmax over d for each 32-token tile, as the other form does, and stores
//      p_h to LDS as [head][tile][e >> 2][lane][e & 3]: 4 KB per head and tile, b128 stores and loads with the lanes
//      contiguous (conflict-free without padding).                                                       -- barrier --
//   B. wave w owns an output column tile instead of a head: mt = w at C = 128, (mt, tile) = (w & 1, w >> 1) at C = 64.
//      It accumulates sum_h M_h[mt] p_h, 4 heads x 16 MFMAs into one accumulator that starts from the bias; step
//      (h, e) takes the M register the other form takes and as B operand exactly the value lane (token, half) of wave
//      h held in accumulator register e.  The MFMA count per token is unchanged.  The tile ends as channel rows on the
//      registers and the token on the lane: the sum of squares over the tile's 32 channels (16 FMAs and one
//      shfl_xor 32) goes to ssb[mt][token], and z to ONE [tokens][C + 4] buffer.  (At C = 64 that buffer lies over p behind one more barrier, which keeps
//      the workgroup under 80 KB.)                                                                       -- barrier --
//   C. all threads: RMSNorm over the channels with the column tiles' sums added in tile order, gain, + x, and the
//      coalesced 16-byte row stores of the other form.
// The rows of the next window are loaded into registers before A and written to the other LDS window after C, one
// barrier per window, as linattn_ctx_image_kernel does.  Every token is computed for itself (there is no sum over
// tokens in this kernel), in an order that is fixed by the code: the result of an image depends neither on the batch
// nor on the run length nor on where the image sits.
// Beside f32-input MFMAs every other instruction of a SIMD's waves costs issue time instead of filling gaps (DESIGN
// section 6), so the loop is also kept short: the window holds ||x_t||^2 and root and reciprocal are taken once per
// tile, the window store's row sums run on DPP, the softmax maximum is formed from the raw products, and whole
// windows take paths without row clamps or masks.
static constexpr int LA_OUTW = 4096;  // floats of x per LDS window of the head-sum form

template <int C>
__global__ __launch_bounds__(256, 2) void linattn_out_headsum_kernel(const float* __restrict__ x, const LinAttnFused w,
                                                                     const float* __restrict__ mz,
                                                                     float* __restrict__ y, int n, int run, int add_x,
                                                                     float scale) {
    constexpr int G = C / 8, XS = C + 4, MT = C / 32, Q = C / 4, TW = LA_OUTW / C, TILES = TW / 32, NP = TW * Q / 256;
    constexpr int PB = LA_HEADS * TILES * 16 * 64;  // floats of p per window
    constexpr bool ZALIAS = C == 64;
    static_assert(!ZALIAS || TW * XS <= PB, "z does not fit over p");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* rnb = smem + 2 * TW * XS;                // [2][TW]
    float* pb = rnb + 2 * TW;                       // [heads][TILES][4][64][4]
    float* zb = ZALIAS ? pb : pb + PB;              // [TW][XS]
    float* ssb = (ZALIAS ? pb + PB : zb + TW * XS);  // [MT][TW]
    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int mt = ZALIAS ? (wv & 1) : wv, zt = ZALIAS ? (wv >> 1) : 0;  // phase B: column tile, token tile
    const float* xb = x + (size_t)b * n * C;
    const int nw = (n + TW - 1) / TW;
    const int w0 = blockIdx.x * run, w1 = min(nw, w0 + run);

    // resident operands, issued before anything waits
    f32x4 wq[G];
#pragma unroll
    for (int g = 0; g < G; ++g) wq[g] = *reinterpret_cast<const f32x4*>(w.wq + (((size_t)wv * G + g) * 64 + lane) * 4);
    f32x4 mreg[LA_HEADS][4];
#pragma unroll
    for (int hh = 0; hh < LA_HEADS; ++hh)
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4)
            mreg[hh][e4] = *reinterpret_cast<const f32x4*>(
                mz + ((((size_t)b * LA_HEADS + hh) * MT + mt) * 4 + e4) * 64 * 4 + lane * 4);
    f32x16 bias;  // in the accumulator's order: the chain of phase B starts from it
#pragma unroll
    for (int m4 = 0; m4 < 4; ++m4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(w.bias + 32 * mt + 8 * m4 + 4 * lh);
#pragma unroll
        for (int i = 0; i < 4; ++i) bias[4 * m4 + i] = v[i];
    }
    const int q4 = tid & (Q - 1);  // 256 is a multiple of Q: a thread keeps its channel quad in phase C
    const f32x4 og = *reinterpret_cast<const f32x4*>(w.og + 4 * q4);

    f32x4 pre[NP];
    la_image_load<C, TW, 256>(xb, w0 * TW, n, pre);
    la_image_store<C, TW, 256, true>(pre, smem, rnb);
    __syncthreads();

    for (int wi = w0; wi < w1; ++wi) {
        const bool more = wi + 1 < w1;
        if (more) {
            if ((wi + 2) * TW <= n) {  // a whole window: nothing to clamp or to zero
                const float* xw = xb + ((size_t)(wi + 1) * TW + tid / Q) * C + 4 * q4;
#pragma unroll
                for (int i = 0; i < NP; ++i) pre[i] = *reinterpret_cast<const f32x4*>(xw + (size_t)i * (256 / Q) * C);
            } else {
                la_image_load<C, TW, 256>(xb, (wi + 1) * TW, n, pre);
            }
        }
        const int buf = (wi - w0) & 1;
        const float* xs = smem + buf * TW * XS;
        const float* rn = rnb + buf * TW;
        const int t0 = wi * TW;
        const int nt = min(TW, n - t0);

        // A. q (d x tokens) = W'_q (d x C) x^T: A = weights in registers, B = x row of token l31 from LDS
#pragma unroll
        for (int st = 0; st < TILES; ++st) {
            if (st * 32 >= nt) break;
            f32x16 qacc;
#pragma unroll
            for (int e = 0; e < 16; ++e) qacc[e] = 0.f;
            const float* xr = xs + (st * 32 + l31) * XS + 4 * lh;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(xr + 8 * g);
#pragma unroll
                for (int s = 0; s < 4; ++s) qacc = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[g][s], a[s], qacc, 0, 0, 0);
            }
            // softmax over d (:185) for token l31: 16 values here, 16 in the other lane half; then * scale (:188)
            const float r = 1.0f / fmaxf(sqrtf(rn[st * 32 + l31]), 1e-12f);  // the window holds ||x_t||^2
            float m = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) m = fmaxf(m, qacc[e]);
            m = fmaxf(m, __shfl_xor(m, 32));
            m *= r;  // = max_e fl(q_e r): r > 0 and rounding is monotonic, so the 16 products need not be formed for it
            float ssum = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                qacc[e] = __expf(qacc[e] * r - m);
                ssum += qacc[e];
            }
            ssum += __shfl_xor(ssum, 32);
            const float inv = scale / ssum;
            float* pw = pb + (size_t)(wv * TILES + st) * 16 * 64 + lane * 4;
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4)
                *reinterpret_cast<f32x4*>(pw + e4 * 64 * 4) = make_f32x4(qacc[4 * e4] * inv, qacc[4 * e4 + 1] * inv,
                                                                          qacc[4 * e4 + 2] * inv, qacc[4 * e4 + 3] * inv);
        }
        __syncthreads();

        // B. z tile (32 channels x 32 tokens) = sum over heads and d of M p; token tiles past the image are skipped
        const bool live = zt * 32 < nt;
        f32x16 zacc;
        float ss = 0.f;
        if (live) {
            zacc = bias;
#pragma unroll
            for (int hh = 0; hh < LA_HEADS; ++hh) {
                const float* pr = pb + (size_t)(hh * TILES + zt) * 16 * 64 + lane * 4;
#pragma unroll
                for (int e4 = 0; e4 < 4; ++e4) {
                    const f32x4 p = *reinterpret_cast<const f32x4*>(pr + e4 * 64 * 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        zacc = __builtin_amdgcn_mfma_f32_32x32x2f32(mreg[hh][e4][i], p[i], zacc, 0, 0, 0);
                }
            }
            // register e = channel 32*mt + row_of(e, lh) of token zt*32 + l31
#pragma unroll
            for (int e = 0; e < 16; ++e) ss = fmaf(zacc[e], zacc[e], ss);
            ss += __shfl_xor(ss, 32);
        }
        if (ZALIAS) __syncthreads();  // every wave has read p before z is written over it
        if (live) {
            float* zr = zb + (zt * 32 + l31) * XS + 32 * mt + 4 * lh;
#pragma unroll
            for (int m4 = 0; m4 < 4; ++m4)
                *reinterpret_cast<f32x4*>(zr + 8 * m4) =
                    make_f32x4(zacc[4 * m4], zacc[4 * m4 + 1], zacc[4 * m4 + 2], zacc[4 * m4 + 3]);
            if (lh == 0) ssb[mt * TW + zt * 32 + l31] = ss;
        }
        __syncthreads();

        // C. RMSNorm over channels (to_out[1], :170), + x, store
        auto rows_out = [&](auto whole) {
            float* yw = y + ((size_t)b * n + t0 + tid / Q) * C + 4 * q4;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int tok = tid / Q + i * (256 / Q);
                if (whole.value || tok < nt) {
                    f32x4 z = *reinterpret_cast<const f32x4*>(zb + tok * XS + 4 * q4);
                    float sq = ssb[tok];
#pragma unroll
                    for (int m = 1; m < MT; ++m) sq += ssb[m * TW + tok];
                    z = z * fast_rsq(fmaxf(sq, 1e-24f)) * og;
                    if (add_x) z += *reinterpret_cast<const f32x4*>(xs + tok * XS + 4 * q4);
                    *reinterpret_cast<f32x4*>(yw + (size_t)i * (256 / Q) * C) = z;
                }
            }
        };
        if (nt == TW) rows_out(std::true_type{});  // a whole window: no row is masked
        else rows_out(std::false_type{});
        if (more) la_image_store<C, TW, 256, true>(pre, smem + (buf ^ 1) * TW * XS, rnb + (buf ^ 1) * TW);
        __syncthreads();  // the next window is written; p, z and this window may be rewritten
    }
}

template <int C, int TOK1>
static int launch_ctx(const LinAttnFused& w, const float* x, float* ws, int B, int n, int nblk, hipStream_t s) {
    const size_t lds1 = (size_t)(TOK1 * (C + 4) + TOK1) * 4;
    static LdsOptIn lds_flag;
    if (lds_opt_in(lds_flag, reinterpret_cast<const void*>(linattn_ctx_fused_kernel<C, TOK1>), 1)) return 1;
    hipLaunchKernelGGL((linattn_ctx_fused_kernel<C, TOK1>), dim3(nblk, B), dim3(256), lds1, s, x, w, ws, n, nblk);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

// Which form of kernel 1 a layer takes.  The per-image form runs B workgroups of 8 waves, so it needs a batch that
// fills the chip's 256 CUs; below that the (token block, image) grid of the blocked kernel plus the reduce launch win.
// Context pass per launch in us on MI355X, blocked kernel + reduce | per-image kernel, event-timed through
// tools/linattn_ctx_time.py (profiles/linattn_image_dispatch_table.json, two runs of each; the second run is within 0.7 us):
//
//   (C, tokens)   B = 32         B = 64         B = 128        B = 256
//   (64, 1024)    16.6 | 80.2    29.5 | 80.4    57.0 | 82.6    106.3 | 86.7
//   (64, 256)     14.4 | 23.2    15.1 | 23.6    17.9 | 24.6     32.5 | 27.1
//   (128, 256)    26.5 | 45.3    27.5 | 45.9    31.8 | 48.0     56.9 | 51.4
//   (128, 64)     13.7 | 19.8    14.8 | 20.2    17.5 | 21.6     24.1 | 23.9
//
// It wins at B = 256 wherever an image has more than one 32-token tile per wave; at (128, 64) the two forms tie (one
// tile per wave, nothing to pipeline, and the C = 128 fold is the larger one), so that shape keeps the blocked kernel.
// Batches between 128 and 256 and C = 64 maps of 64 tokens or fewer are not measured; the rule takes the per-image form
// only from the batch at which it was seen to win.
static bool la_image_form(int B, int n, int C) { return B >= 256 && (C == 64 || n > 64); }

template <int C>
static int launch_ctx_image(const LinAttnFused& w, const float* x, float* mz, int B, int n, hipStream_t s) {
    const size_t lds = (size_t)(2 * LA_TOKI * (C + 4) + 2 * LA_TOKI) * 4;
    static LdsOptIn lds_flag;
    if (lds_opt_in(lds_flag, reinterpret_cast<const void*>(linattn_ctx_image_kernel<C>), 1)) return 1;
    hipLaunchKernelGGL(linattn_ctx_image_kernel<C>, dim3(B), dim3(512), lds, s, x, w, mz, n);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

// Which form of kernel 2 a layer takes.  Output kernel per launch in us on MI355X, linattn_out_fused_kernel |
// linattn_out_headsum_kernel, event-timed through tools/linattn_out_time.py (profiles/linattn_out_dispatch_table.json,
// two runs of each; the second run is within 0.3 us, or 4 % where the launch is longer than 90 us):
//
//   (C, tokens)   B = 8          B = 32         B = 64         B = 128        B = 256
//   (64, 1024)     7.0 |  5.7    14.5 | 12.8    27.4 | 25.0    51.4 | 45.4    98.9 | 85.3
//   (64, 256)      6.6 |  5.2     7.2 |  5.4     8.5 |  6.8    15.3 | 13.3    28.6 | 25.4
//   (128, 256)    13.6 |  5.1    14.8 |  7.3    17.2 | 14.2    36.0 | 25.6    72.4 | 44.2
//   (128, 64)     12.5 |  4.9    12.6 |  5.3    13.1 |  5.6    13.7 |  7.3    16.9 | 14.0
//   (64, 4096)    14.2 | 12.6    49.1 | 45.6    96.1 | 85.2   195.6 |167.8   401.4 |342.8
//
// The head-sum form wins at every shape and batch that was measured.  It is taken from B = 32 on, not from 8: batches
// below 8 are not measured, and a sampler's shards must equal the unsharded batch bit for bit
// (tests/test_hip_configs.py compares a batch of 8 with its shards of 4, 3 and 2), so the two forms, which sum the heads
// in different orders, may not change inside that range.  Batches between the measured ones run the same grid rule.
static constexpr int LA_OUT_WGS = 512;  // two resident workgroups on each of the chip's 256 CUs
static bool la_out_headsum_form(int B, int n, int C) {
#ifdef DM_LA_OUT_FORM  // the two builds behind the table (tools/linattn_out_time.py): every layer on one form
    return DM_LA_OUT_FORM;
#else
    return B >= 32;
#endif
}

// Runs of windows: as few workgroups as still give every CU two (the operands are loaded once per workgroup), cut
// into equal runs so that the grid is one scheduling round where the batch allows it.
template <int C>
static int launch_out_headsum(const LinAttnFused& w, const float* x, const float* mz, float* y, int B, int n, bool add_x,
                              hipStream_t s) {
    constexpr int TW = LA_OUTW / C, TILES = TW / 32;
    constexpr bool ZALIAS = C == 64;
    const size_t lds = (size_t)(2 * TW * (C + 4) + 2 * TW + LA_HEADS * TILES * 16 * 64 + (ZALIAS ? 0 : TW * (C + 4)) +
                                (C / 32) * TW) * 4;
    static LdsOptIn lds_flag;
    if (lds_opt_in(lds_flag, reinterpret_cast<const void*>(linattn_out_headsum_kernel<C>), 1)) return 1;
    const int nw = (n + TW - 1) / TW;
    const int per_image = std::min(nw, std::max(1, (LA_OUT_WGS + B - 1) / B));
    const int run = (nw + per_image - 1) / per_image;
    hipLaunchKernelGGL(linattn_out_headsum_kernel<C>, dim3((nw + run - 1) / run, B), dim3(256), lds, s, x, w, mz, y, n,
                       run, add_x ? 1 : 0, 1.0f / sqrtf((float)LA_DH));
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

template <int C>
static int launch_c(const LinAttnFused& w, const float* x, float* ws, float* y, int B, int n, bool add_x, hipStream_t s) {
    const bool image = la_image_form(B, n, C);
    // 256-token blocks halve the partial-context traffic, but only when they still fill the chip
    const bool big = la_tok1(C) == 256 && (size_t)B * ((n + 255) / 256) >= 512;
    const int tok1 = big ? 256 : LA_TOK1;
    const int nblk = image ? 0 : (n + tok1 - 1) / tok1;
    const size_t lds2 = (size_t)(LA_TOK2 * (C + 4) + LA_TOK2 + LA_HEADS * 32 * (C + 4)) * 4;
    static LdsOptIn lds_flag;
    if (lds_opt_in(lds_flag, reinterpret_cast<const void*>(linattn_out_fused_kernel<C>), 1)) return 1;
    const bool timed = prof::enabled();
    const double tokens = (double)B * n;
    float* ctxn = ws + (size_t)B * nblk * LA_HEADS * LA_CTX;  // M = W_out ctx^T, lane-packed
    if (image) {
        // k and P^T per token, then per image W'_v P^T and W_out ctx^T; one read of x
        if (timed && prof::begin("linattn_ctx_image_kernel",
                                 2.0 * tokens * (2.0 * LA_HID * C) + (double)B * 2.0 * (2.0 * LA_HID * LA_DH * C),
                                 4.0 * tokens * C, s))
            return 1;
        if (launch_ctx_image<C>(w, x, ctxn, B, n, s)) return 1;
        if (timed && prof::end(s)) return 1;
    } else {
        if (timed && prof::begin("linattn_ctx_fused_kernel", 2.0 * tokens * (2.0 * LA_HID * C + LA_HID * LA_DH),
                                 4.0 * tokens * C, s))
            return 1;
        if (big ? launch_ctx<C, (C <= 64 ? 256 : LA_TOK1)>(w, x, ws, B, n, nblk, s)
                : launch_ctx<C, LA_TOK1>(w, x, ws, B, n, nblk, s))
            return 1;
        if (timed && prof::end(s)) return 1;
        if (timed && prof::begin("linattn_ctx_reduce_kernel", (double)B * 2.0 * LA_HID * LA_DH * C,
                                 4.0 * B * ((double)nblk * LA_HEADS * LA_CTX + LA_HID * C + LA_HID * C), s))
            return 1;
        hipLaunchKernelGGL(linattn_ctx_reduce_kernel<C>, dim3(LA_HEADS, B), dim3(256), 0, s, ws, w.wo_raw, ctxn, nblk);
        DM_CHECK_HIP(hipGetLastError());
        if (timed && prof::end(s)) return 1;
    }
    const bool headsum = la_out_headsum_form(B, n, C);
    if (timed && prof::begin(headsum ? "linattn_out_headsum_kernel" : "linattn_out_fused_kernel",
                             2.0 * tokens * (2.0 * LA_HID * C + LA_HID * LA_DH), 8.0 * tokens * C, s))
        return 1;
    if (headsum) {
        if (launch_out_headsum<C>(w, x, ctxn, y, B, n, add_x, s)) return 1;
    } else {
        hipLaunchKernelGGL(linattn_out_fused_kernel<C>, dim3((n + LA_TOK2 - 1) / LA_TOK2, B), dim3(256), lds2, s, x, w,
                           ctxn, y, n, add_x ? 1 : 0, 1.0f / sqrtf((float)LA_DH));
        DM_CHECK_HIP(hipGetLastError());
    }
    if (timed && prof::end(s)) return 1;
    return 0;
}

int launch_linattn_fused(const LinAttnFused& w, const float* x, float* ws, float* y, int B, int n, bool add_x,
                         hipStream_t s) {
    DM_REQUIRE(w.C == 64 || w.C == 128, "fused LinearAttention: C must be 64 or 128");
    if (w.C == 64) return launch_c<64>(w, x, ws, y, B, n, add_x, s);
    return launch_c<128>(w, x, ws, y, B, n, add_x, s);
}

}  // namespace dm
