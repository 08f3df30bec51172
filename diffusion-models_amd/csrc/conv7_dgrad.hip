// Input gradient of the 7x7 / pad 3 first convolution (gfx950): dX (NCHW, 1..8 channels) from dY (NHWC, Cout channels)
// and the (Cout, C, 7, 7) weight as the parameter stores it.  The mirror image of init7_mfma_kernel: K = 49 Cout is long,
// the output is 1..8 channels thin.
//
//   dX[b][c][y][x] = sum_o sum_ky sum_kx dY[b][y + 3 - ky][x + 3 - kx][o] * W[o][c][ky][kx]      (rows / columns outside
//                                                                                                  the image are zero)
//
// fp32 VALU, no matrix core: with N = C <= 8 a 16x16x4 f32 MFMA would run on an operand that is at least half padding, and
// the whole layer is 2 * 49 * Cout * C flops per pixel -- about 1 / 1000 of the training step it belongs to.  One workgroup
// of 256 threads owns a 32 x 8 pixel tile of one image, one thread one pixel with all C accumulators.  The output channels
// o are walked 16 at a time: the chunk's dY halo (38 x 14 pixels) is staged in LDS as [o][row][col], so that the 32 lanes
// of a half-wave read 32 consecutive dwords (conflict-free ds_read_b32 at any pitch), and the chunk's weights as
// [o][tap][c padded to CP], which every lane reads at the same address (a broadcast ds_read_b128 per four channels).  The
// "rotation" of an input-gradient convolution is the index y + 3 - ky above: the kernel reads the parameter itself, so there
// is no second packed copy that an optimiser step could leave stale.
//
// Accumulation order is fixed -- o ascending, then ky, kx -- in one thread per output value: no atomics, no split K, no
// scratch; an image's result does not depend on the batch it is in.
#include "dm_common.h"

namespace dm {

namespace {
constexpr int C7_TW = 32, C7_TH = 8;              // output tile
constexpr int C7_HW = C7_TW + 6, C7_HH = C7_TH + 6;  // dY halo tile
constexpr int C7_OC = 16;                         // output channels per chunk
constexpr int C7_HALO = C7_HW * C7_HH;            // 532 dwords per channel
}  // namespace

template <int CP>
__global__ __launch_bounds__(256) void conv7_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                          float* __restrict__ dx, int H, int W, int Cout, int C, int tiles_x) {
    __shared__ float s_dy[C7_OC * C7_HALO];
    __shared__ __attribute__((aligned(16))) float s_w[C7_OC * 49 * CP];
    const int tid = threadIdx.x;
    const int tx = tid & (C7_TW - 1), ty = tid >> 5;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0 = tile_x * C7_TW, y0 = tile_y * C7_TH;
    const int b = blockIdx.y;
    const float* dyb = dy + (size_t)b * H * W * Cout;

    float acc[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) acc[c] = 0.f;

    for (int ob = 0; ob < Cout; ob += C7_OC) {
        __syncthreads();  // the previous chunk has been consumed
        // dY halo: element e = pixel * 16 + o, o fastest (64 contiguous bytes of a pixel's channels per 16 lanes)
        for (int e = tid; e < C7_HALO * C7_OC; e += 256) {
            const int o = e & (C7_OC - 1), p = e >> 4;
            const int r = p / C7_HW, q = p - r * C7_HW;
            const int yy = y0 - 3 + r, xx = x0 - 3 + q;
            float v = 0.f;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W && ob + o < Cout) v = dyb[((size_t)yy * W + xx) * Cout + ob + o];
            s_dy[o * C7_HALO + p] = v;
        }
        // weights: s_w[(o * 49 + tap) * CP + c] = W[ob + o][c][tap], zero for the padding channels and a ragged last chunk
        for (int e = tid; e < C7_OC * 49 * CP; e += 256) {
            const int c = e % CP, ot = e / CP;
            const int o = ot / 49, tap = ot - o * 49;
            s_w[e] = (c < C && ob + o < Cout) ? w[((size_t)(ob + o) * C + c) * 49 + tap] : 0.f;
        }
        __syncthreads();
        for (int o = 0; o < C7_OC; ++o) {
            const float* dyo = s_dy + o * C7_HALO + (ty + 6) * C7_HW + tx + 6;
            const float* wo = s_w + o * 49 * CP;
#pragma unroll
            for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const float g = dyo[-ky * C7_HW - kx];
                    const float4* w4 = reinterpret_cast<const float4*>(wo + (ky * 7 + kx) * CP);
#pragma unroll
                    for (int c4 = 0; c4 < CP / 4; ++c4) {
                        const float4 wv = w4[c4];
                        acc[4 * c4 + 0] = fmaf(g, wv.x, acc[4 * c4 + 0]);
                        acc[4 * c4 + 1] = fmaf(g, wv.y, acc[4 * c4 + 1]);
                        acc[4 * c4 + 2] = fmaf(g, wv.z, acc[4 * c4 + 2]);
                        acc[4 * c4 + 3] = fmaf(g, wv.w, acc[4 * c4 + 3]);
                    }
                }
            }
        }
    }
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
#pragma unroll
    for (int c = 0; c < CP; ++c)
        if (c < C) dx[(((size_t)b * C + c) * H + y) * W + x] = acc[c];
}

int launch_conv7_dgrad(const float* dy_nhwc, const float* w_oihw, float* dx_nchw, int B, int H, int W, int Cout, int C,
                       hipStream_t s) {
    DM_REQUIRE(dy_nhwc && w_oihw && dx_nchw, "conv7_dgrad: null tensor");
    DM_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && Cout > 0 && C >= 1 && C <= 8,
               "conv7_dgrad: 1..8 input channels, a batch of at most 65535");
    const int tiles_x = (W + C7_TW - 1) / C7_TW, tiles_y = (H + C7_TH - 1) / C7_TH;
    DM_REQUIRE((int64_t)tiles_x * tiles_y < (int64_t(1) << 31), "conv7_dgrad: image too large");
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)B);
    if (C <= 4)
        hipLaunchKernelGGL(conv7_dgrad_kernel<4>, grid, dim3(256), 0, s, dy_nhwc, w_oihw, dx_nchw, H, W, Cout, C, tiles_x);
    else
        hipLaunchKernelGGL(conv7_dgrad_kernel<8>, grid, dim3(256), 0, s, dy_nhwc, w_oihw, dx_nchw, H, W, Cout, C, tiles_x);
    DM_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dm
