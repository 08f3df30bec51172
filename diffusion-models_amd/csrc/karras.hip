// KarrasUnet kernels (gfx950): the elementwise and row passes of the EDM2 magnitude-preserving U-Net (Karras et al.,
// arXiv 2312.02696, config G; DD/karras_unet.py) that are not convolutions or the attention core -- the pixel norm, the two
// resamplers, the scaled-SiLU passes around the skip concatenation, the q/k/v normalisation, the Fourier features of the
// conditioning head and the input tensor with its ones channel.  fp32, NHWC, every channel count a multiple of 4: a thread
// moves 16 bytes per tensor.  The passes are bandwidth-bound; each reads its input once and writes every tensor its
// consumers need (the activation of block1, the scaled residual of MPAdd) in the same pass.  The magnitude-preserving
// constants arrive as kernel arguments, formed on the host in double (dm_kunet.inc).
#include "dm_common.h"

#include <cmath>

namespace dm {

#pragma clang fp contract(off)

namespace {

// expf, not __expf: the passes are bandwidth-bound, and the operator tests hold them to 4 x the rounding of the fp32 restatement
__device__ __forceinline__ float ksilu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float4 ksilu4(float4 v) { return make_float4(ksilu(v.x), ksilu(v.y), ksilu(v.z), ksilu(v.w)); }
__device__ __forceinline__ float4 kscale4(float4 v, float c) { return make_float4(v.x * c, v.y * c, v.z * c, v.w * c); }
__device__ __forceinline__ float4 kld4(const float* p, int64_t i) { return *reinterpret_cast<const float4*>(p + i); }
__device__ __forceinline__ void kst4(float* p, int64_t i, float4 v) { *reinterpret_cast<float4*>(p + i) = v; }

struct Timed {  // one profile row around a launch (never while a graph is captured: prof::enabled() is off then)
    hipStream_t s;
    bool on;
    Timed(const char* name, double bytes, hipStream_t st) : s(st), on(prof::enabled()) {
        if (on) on = prof::begin(name, 0.0, bytes, s) == 0;
    }
    int done() {
        DM_CHECK_HIP(hipGetLastError());
        return on ? prof::end(s) : 0;
    }
};

int blocks_of(int64_t threads, unsigned* out) {
    const int64_t b = (threads + 255) / 256;
    DM_REQUIRE(threads > 0 && b < (int64_t(1) << 31), "karras: empty or oversized launch");
    *out = (unsigned)b;
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// PixelNorm (DD/karras_unet.py:77-86): y = x / max(||x||_2, 1e-4) * sqrt(C) over the C channels of a row.
// A row takes LANES lanes of a wavefront (64 / LANES rows per wavefront), each holding NV float4 of it in registers; the sum of
// squares is a butterfly over those lanes.  Writes y * res_scale (the residual operand of MPAdd, or with res_scale = 1 the
// normalised q / k / v, in place) and silu(y) (what block1's convolution reads), each optional.
// ---------------------------------------------------------------------------------------
template <int LANES, int NV>
__global__ __launch_bounds__(256) void kunet_pixelnorm_kernel(const float* x, float* res_out, float* __restrict__ act_out,
                                                              int64_t rows, int C, float res_scale, float sqrt_c) {
    constexpr int RPW = 64 / LANES;
    const int lane = threadIdx.x & 63, sub = lane / LANES, li = lane % LANES;
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + sub;
    const bool ok = row < rows;
    const int64_t base = (ok ? row : rows - 1) * C;  // every lane stays in the butterfly
    const int nv4 = C >> 2;
    float4 v[NV];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = li + LANES * i;
        v[i] = j < nv4 ? kld4(x, base + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
    }
#pragma unroll
    for (int m = LANES / 2; m >= 1; m >>= 1) ss += __shfl_xor(ss, m);
    if (!ok) return;
    const float d = fmaxf(sqrtf(ss), 1e-4f);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = li + LANES * i;
        if (j >= nv4) continue;
        const float4 y = make_float4(v[i].x / d * sqrt_c, v[i].y / d * sqrt_c, v[i].z / d * sqrt_c, v[i].w / d * sqrt_c);
        if (res_out) kst4(res_out, base + 4 * j, kscale4(y, res_scale));
        if (act_out) kst4(act_out, base + 4 * j, ksilu4(y));
    }
}

static int pixelnorm_launch(const char* name, const float* x, float* res_out, float* act_out, int64_t rows, int C, float res_scale,
                            hipStream_t s) {
    DM_REQUIRE(x && (res_out || act_out) && rows > 0, "kunet_pixelnorm: null argument");
    DM_REQUIRE(C > 0 && C % 4 == 0 && C <= 4096, "kunet_pixelnorm: the channel count must be a multiple of 4, at most 4096");
    const float sqrt_c = (float)std::sqrt((double)C);
    const int outs = (res_out ? 1 : 0) + (act_out ? 1 : 0);
    Timed t(name, 4.0 * rows * C * (1 + outs), s);
    const int nv4 = C / 4;
#define DM_KPN(L_, NV_)                                                                                                     \
    {                                                                                                                        \
        const int64_t rpb = 4 * (64 / L_);                                                                                   \
        unsigned nb;                                                                                                         \
        DM_REQUIRE((rows + rpb - 1) / rpb < (int64_t(1) << 31), "kunet_pixelnorm: too many rows");                           \
        nb = (unsigned)((rows + rpb - 1) / rpb);                                                                             \
        hipLaunchKernelGGL((kunet_pixelnorm_kernel<L_, NV_>), dim3(nb), dim3(256), 0, s, x, res_out, act_out, rows, C,        \
                           res_scale, sqrt_c);                                                                               \
        return t.done();                                                                                                     \
    }
    if (nv4 <= 8) DM_KPN(8, 1)
    if (nv4 <= 16) DM_KPN(16, 1)
    if (nv4 <= 32) DM_KPN(32, 1)
    if (nv4 <= 64) DM_KPN(64, 1)
    if (nv4 <= 128) DM_KPN(64, 2)
    if (nv4 <= 256) DM_KPN(64, 4)
    if (nv4 <= 512) DM_KPN(64, 8)
    DM_KPN(64, 16)
#undef DM_KPN
}

int launch_kunet_pixelnorm(const float* x, float* res_out, float* act_out, int64_t rows, int C, float res_scale, hipStream_t s) {
    return pixelnorm_launch("kunet_pixelnorm", x, res_out, act_out, rows, C, res_scale, s);
}

// q, k and v of every head normalised along dh, in place: the (rows, 3 heads dh) to_qkv output is (rows 3 heads, dh)
int launch_kunet_qkv_norm(float* qkv, int64_t rows, int heads, int dh, hipStream_t s) {
    DM_REQUIRE(dh == 32 || dh == 64, "kunet_qkv_norm: head widths 32 and 64");
    return pixelnorm_launch("kunet_qkv_norm", qkv, qkv, nullptr, rows * 3 * heads, dh, 1.0f, s);
}

// ---------------------------------------------------------------------------------------
// F.interpolate(x, (h / 2, w / 2), mode = 'bilinear') == the 2x2 mean (DD/karras_unet.py:224-226)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kunet_avgpool2_kernel(const float* __restrict__ x, float* __restrict__ y, int Ho, int Wo,
                                                             int C4, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho);
    const int64_t b = p / Ho;
    const int64_t W = 2 * (int64_t)Wo, C = 4 * (int64_t)C4;
    const int64_t at = ((b * 2 * Ho + 2 * oy) * W + 2 * ox) * C + 4 * c;
    const float4 a = kld4(x, at), bq = kld4(x, at + C), cq = kld4(x, at + W * C), dq = kld4(x, at + W * C + C);
    kst4(y, i * 4, make_float4((a.x + bq.x + cq.x + dq.x) * 0.25f, (a.y + bq.y + cq.y + dq.y) * 0.25f,
                               (a.z + bq.z + cq.z + dq.z) * 0.25f, (a.w + bq.w + cq.w + dq.w) * 0.25f));
}

int launch_kunet_avgpool2(const float* x, float* y, int B, int H, int W, int C, hipStream_t s) {
    DM_REQUIRE(x && y && B > 0 && C > 0 && C % 4 == 0, "kunet_avgpool2: null argument or a channel count that is no multiple of 4");
    DM_REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "kunet_avgpool2: even H and W");
    const int64_t n4 = (int64_t)B * (H / 2) * (W / 2) * (C / 4);
    unsigned nb;
    if (blocks_of(n4, &nb)) return 1;
    Timed t("kunet_avgpool2", 4.0 * B * H * W * C * 1.25, s);
    hipLaunchKernelGGL(kunet_avgpool2_kernel, dim3(nb), dim3(256), 0, s, x, y, H / 2, W / 2, C / 4, n4);
    return t.done();
}

// ---------------------------------------------------------------------------------------
// F.interpolate(x, (2h, 2w), mode = 'bilinear') (DD/karras_unet.py:306-308): separable, output 2i = 0.25 x[i-1] + 0.75 x[i],
// output 2i+1 = 0.75 x[i] + 0.25 x[i+1], indices clamped to the edge.  Writes x_up (for a convolutional res_conv), silu(x_up)
// (for block1) and x_up * res_scale (the identity res_conv's operand of MPAdd), each optional.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kunet_bilinear_up2_kernel(const float* __restrict__ x, float* __restrict__ up_out,
                                                                 float* __restrict__ act_out, float* __restrict__ res_out, int H,
                                                                 int W, int C4, int64_t n4, float res_scale) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int ox = (int)(p % (2 * W));
    p /= 2 * W;
    const int oy = (int)(p % (2 * H));
    const int64_t b = p / (2 * H);
    // the far tap (weight 0.25) lies before the source pixel for an even output index, behind it for an odd one
    const int iy = oy >> 1, ix = ox >> 1;
    const int fy = (oy & 1) ? min(iy + 1, H - 1) : max(iy - 1, 0);
    const int fx = (ox & 1) ? min(ix + 1, W - 1) : max(ix - 1, 0);
    const int64_t C = 4 * (int64_t)C4, img = b * H * W;
    const float4 nn = kld4(x, ((img + (int64_t)iy * W + ix) * C) + 4 * c), nf = kld4(x, ((img + (int64_t)iy * W + fx) * C) + 4 * c);
    const float4 fn = kld4(x, ((img + (int64_t)fy * W + ix) * C) + 4 * c), ff = kld4(x, ((img + (int64_t)fy * W + fx) * C) + 4 * c);
    auto mix = [](float a, float bq) { return 0.75f * a + 0.25f * bq; };  // a: the near tap
    const float4 u = make_float4(mix(mix(nn.x, nf.x), mix(fn.x, ff.x)), mix(mix(nn.y, nf.y), mix(fn.y, ff.y)),
                                 mix(mix(nn.z, nf.z), mix(fn.z, ff.z)), mix(mix(nn.w, nf.w), mix(fn.w, ff.w)));
    if (up_out) kst4(up_out, i * 4, u);
    if (act_out) kst4(act_out, i * 4, ksilu4(u));
    if (res_out) kst4(res_out, i * 4, kscale4(u, res_scale));
}

int launch_kunet_bilinear_up2(const float* x, float* up_out, float* act_out, float* res_out, int B, int H, int W, int C,
                              float res_scale, hipStream_t s) {
    DM_REQUIRE(x && (up_out || act_out || res_out), "kunet_bilinear_up2: null argument");
    DM_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "kunet_bilinear_up2: a channel count that is a multiple of 4");
    const int64_t n4 = (int64_t)B * 2 * H * 2 * W * (C / 4);
    unsigned nb;
    if (blocks_of(n4, &nb)) return 1;
    const int outs = (up_out ? 1 : 0) + (act_out ? 1 : 0) + (res_out ? 1 : 0);
    Timed t("kunet_bilinear_up2", 4.0 * B * H * W * C * (1 + 4.0 * outs), s);
    hipLaunchKernelGGL(kunet_bilinear_up2_kernel, dim3(nb), dim3(256), 0, s, x, up_out, act_out, res_out, H, W, C / 4, n4, res_scale);
    return t.done();
}

// ---------------------------------------------------------------------------------------
// MPSiLU in front of block1 of a Decoder (its 1 / 0.596 lives in the convolution's weights): act = silu(ca a), or with a
// second source the concatenation cat(silu(ca a), silu(cb b)) of MPCat's two halves (DD/karras_unet.py:41-56); optionally the
// scaled copy a * copy_scale, the residual operand of MPAdd where res_conv is the identity (and in front of an attention layer).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kunet_act_kernel(const float* __restrict__ a, int Ca4, float ca, const float* __restrict__ b,
                                                        int Cb4, float cb, float* __restrict__ act_out, float* __restrict__ copy_out,
                                                        float copy_scale, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int Ct4 = Ca4 + Cb4;
    const int c = (int)(i % Ct4);
    const int64_t row = i / Ct4;
    if (c < Ca4) {
        const float4 v = kld4(a, (row * Ca4 + c) * 4);
        if (act_out) kst4(act_out, i * 4, ksilu4(kscale4(v, ca)));
        if (copy_out) kst4(copy_out, (row * Ca4 + c) * 4, kscale4(v, copy_scale));
    } else {
        const float4 v = kld4(b, (row * Cb4 + (c - Ca4)) * 4);
        kst4(act_out, i * 4, ksilu4(kscale4(v, cb)));
    }
}

int launch_kunet_act(const float* a, int Ca, float ca, const float* b, int Cb, float cb, float* act_out, float* copy_out,
                     float copy_scale, int64_t rows, hipStream_t s) {
    DM_REQUIRE(a && (act_out || copy_out) && rows > 0, "kunet_act: null argument");
    DM_REQUIRE(Ca > 0 && Ca % 4 == 0 && (b ? (Cb > 0 && Cb % 4 == 0 && act_out != nullptr) : Cb == 0),
               "kunet_act: channel counts that are multiples of 4; a second source needs the activation output");
    const int64_t n4 = rows * ((Ca + Cb) / 4);
    unsigned nb;
    if (blocks_of(n4, &nb)) return 1;
    Timed t("kunet_act", 4.0 * rows * ((Ca + Cb) * (act_out ? 2.0 : 1.0) + (copy_out ? Ca : 0)), s);
    hipLaunchKernelGGL(kunet_act_kernel, dim3(nb), dim3(256), 0, s, a, Ca / 4, ca, b, Cb / 4, cb, act_out, copy_out, copy_scale, n4);
    return t.done();
}

// ---------------------------------------------------------------------------------------
// The input rows of the conditioning head: sqrt(2) [sin, cos](2 pi t w) (MPFourierEmbedding, DD/karras_unet.py:147-157) and,
// behind them, the row's class labels (already times sqrt(num_classes)).  t: one value per row, or with `st` entry
// t[st->step * t_stride] of the EDM step table for every row.
// ---------------------------------------------------------------------------------------
__global__ void kunet_fourier_kernel(const float* __restrict__ t, int t_stride, const SamplerState* __restrict__ st,
                                     const float* __restrict__ w, const float* __restrict__ labels, int n_labels,
                                     float* __restrict__ e, int R, int half) {
    const int width = 2 * half + n_labels, per = half + n_labels;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * per) return;
    const int r = i / per, k = i - r * per;
    float* row = e + (size_t)r * width;
    if (k >= half) {
        row[half + k] = labels[(size_t)r * n_labels + (k - half)];
        return;
    }
    const float tv = st ? t[(size_t)st->step * t_stride] : t[r];
    const float f = (tv * w[k]) * 6.283185307179586f;
    row[k] = sinf(f) * 1.4142135623730951f;
    row[half + k] = cosf(f) * 1.4142135623730951f;
}

int launch_kunet_fourier(const float* t, int t_stride, const SamplerState* st, const float* w, const float* labels, int n_labels,
                         float* e, int R, int half, hipStream_t s) {
    DM_REQUIRE(t && w && e && R > 0 && half > 0 && n_labels >= 0 && (labels || n_labels == 0), "kunet_fourier: bad argument");
    const int n = R * (half + n_labels);
    Timed tm("kunet_fourier", 4.0 * R * (2 * half + 2 * n_labels), s);
    hipLaunchKernelGGL(kunet_fourier_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t, t_stride, st, w, labels, n_labels, e, R, half);
    return tm.done();
}

// ---------------------------------------------------------------------------------------
// The tensor input_block reads: the NCHW image as NHWC with a channel of ones in front (Conv2d(concat_ones_to_input = True),
// DD/karras_unet.py:123-124).  The convolution's zero padding then reaches the ones channel too, which is what tells it from
// a bias.  One thread per pixel: the reads of a channel are contiguous across a wavefront.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kunet_input_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int HW,
                                                          int64_t pixels) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const int64_t b = p / HW, sp = p - b * HW;
    float* row = y + p * (C + 1);
    row[0] = 1.0f;
    for (int c = 0; c < C; ++c) row[1 + c] = x[(b * C + c) * HW + sp];
}

int launch_kunet_input(const float* x_nchw, float* y, int B, int C, int HW, hipStream_t s) {
    DM_REQUIRE(x_nchw && y && B > 0 && C > 0 && HW > 0, "kunet_input: bad argument");
    const int64_t pixels = (int64_t)B * HW;
    unsigned nb;
    if (blocks_of(pixels, &nb)) return 1;
    Timed t("kunet_input", 4.0 * pixels * (2 * C + 1), s);
    hipLaunchKernelGGL(kunet_input_kernel, dim3(nb), dim3(256), 0, s, x_nchw, y, C, HW, pixels);
    return t.done();
}

}  // namespace dm
