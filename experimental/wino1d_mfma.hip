// Winograd F(4,3) for sequences on the f32 MFMA (gfx950): Conv1d(K = 3, stride 1, padding 1) over (B, L, C) rows, the
// K = 3 convolutions of Unet1D (DD/denoising_diffusion_1d.py:122).  1.5 multiplies per output instead of 3.
//
//   Y = A^T [ (G g) . (B^T d) ]     Lavin & Gray (arXiv 1509.09308) at the points 0, +-1, +-2, inf: the 1D factors of the
//                                   F(4x4, 3x3) family (wino4_mfma.hip); d = 6 positions, Y = 4 outputs
// A tile is 4 consecutive outputs of one sequence (L % 4 == 0, so no tile spans two sequences) and reads positions
// 4j - 1 .. 4j + 4 of ITS sequence: what lies outside [0, L) is zero, never the neighbouring sequence's row.
// Tiles are the MFMA rows, output channels the columns, input channels the reduction, one accumulator set per
// transform point.  Both transforms are lane-local: the lane that owns (tile, 4 cin) reads its six float4 and forms the six
// transformed values, and the six accumulators of a (tile, cout) pair sit in one lane (element e of every point).
//
// Workgroup: 4 waves = 2 (tile halves) x 2 (cout halves), 64 tiles x 64 couts; a wave holds 6 x 16 accumulators.
// K runs over chunks of 8 input channels (source 0, then source 1: the skip concatenation), four 32x32x2 steps per chunk
// and point with k index h <-> cin 4 h + s of the chunk.  grid (tile groups, Cout / 64, K splits).
// Epilogue: bias and residual in the kernel when K is not split; everything else (RMSNorm, scale-shift, SiLU) lands through
// launch_norm_act on the partial sums (ConvParams::partial), as for every family that leaves partials.
//
// NOT part of libdm_hip.so: measured against the direct family on every K = 3 layer of Unet1D(64, (1,2,4,8)) at (B, L) =
// (64, 128) and (16, 1024) and 1.5x .. 2.4x slower at each (profiles/seq1d_wino1d_vs_direct.jsonl), so it was
// taken out.  The wiring it was measured with: this file in csrc/ and in the Makefile's SRCS; the declarations of
// wino1d_eligible / _packed_floats / _pack_weights / _plan / _shape_ok / _launch in dm_common.h; a CONV_WINO1D row
// {"F(4,3) 1D", {}, -1, 8, 64, 0, 8, wino1d_launch, true} in conv_family.inc; a pack_wino1d() helper behind make_conv_k,
// make_upsample1d and the dm_op_conv1d layer (wino1d_pack_weights into ConvLayer::packed[CONV_WINO1D] where eligible); and in
// plan_conv, for a layer no other family has taken, with Hin == 1, Wo % 4 == 0 and wino1d_shape_ok: take(CONV_WINO1D),
// geo = wino1d_plan, in_kernel = (splits == 1 and the epilogue is at most the residual).  tests/conv1d_restate.py (wino1d)
// is its fp32 restatement.  To win it needs the window and the weights staged through LDS with the next chunk in flight.
#include "../diffusion-models_amd/csrc/dm_common.h"

#include <algorithm>
#include <cstdio>
#include <vector>

namespace dm {

using f32x16_t = __attribute__((ext_vector_type(16))) float;

enum { W1CK = 8, W1PTS = 6 };

bool wino1d_off() {
    static const bool off = env_flag("DM_NO_WINO1D") || winograd_off();
    return off;
}

bool wino1d_eligible(int Cout, int C0, int C1, int KH, int KW, int stride, int pad_w) {
    return !wino1d_off() && KH == 1 && KW == 3 && stride == 1 && pad_w == 1 && C0 > 0 && C0 % W1CK == 0 && C1 % W1CK == 0 &&
           Cout % 64 == 0;
}

size_t wino1d_packed_floats(int Cout, int C0, int C1) { return (size_t)W1PTS * (C0 + C1) * Cout; }

// (Cout, C0 + C1, 3) -> U = G g in float64, rounded once, in kernel layout [chunk of 8 cin][point 6][s 4][h 2][Cout] with
// cin = 8 chunk + 4 h + s
void wino1d_pack_weights(const float* w, float* packed, int Cout, int C0, int C1) {
    static const double G[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    const int Cin = C0 + C1;
    for (int c = 0; c < Cin; ++c) {
        const int chunk = c / W1CK, h = (c % W1CK) / 4, s = c % 4;
        for (int o = 0; o < Cout; ++o) {
            const float* g = w + ((size_t)o * Cin + c) * 3;
            for (int xi = 0; xi < W1PTS; ++xi) {
                const double u = G[xi][0] * g[0] + G[xi][1] * g[1] + G[xi][2] * g[2];
                packed[((((size_t)chunk * W1PTS + xi) * 4 + s) * 2 + h) * Cout + o] = (float)u;
            }
        }
    }
}

__global__ __launch_bounds__(256) void wino1d_mfma_kernel(ConvParams p, int n_tiles, int tiles_per_seq) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * 64 + (wave & 1) * 32;  // first tile of the wave
    const int n0 = blockIdx.y * 64 + (wave >> 1) * 32;  // first cout of the wave
    const int L = p.Wo, Cout = p.Cout;
    const int split = blockIdx.z;
    const int c_lo = split * p.geo.chunks_per_split, c_hi = min(p.n_chunks, c_lo + p.geo.chunks_per_split);

    // the lane's tile as an A row: sequence b, first output position 4 j
    const int t = m0 + r;
    const bool t_ok = t < n_tiles;
    const int b = t_ok ? t / tiles_per_seq : 0, j = t_ok ? t - b * tiles_per_seq : 0;
    bool ok[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int pos = 4 * j - 1 + q;
        ok[q] = t_ok && pos >= 0 && pos < L;
    }
    const size_t row0 = (size_t)b * L + 4 * j - 1;  // row of window position 0 (only dereferenced where ok)

    f32x16_t acc[W1PTS];
#pragma unroll
    for (int xi = 0; xi < W1PTS; ++xi)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[xi][e] = 0.f;

    for (int ch = c_lo; ch < c_hi; ++ch) {
        const bool src1 = ch >= p.chunks0;
        const float* src = src1 ? p.in1 : p.in0;
        const int C = src1 ? p.C1 : p.C0;
        const int c0 = (src1 ? ch - p.chunks0 : ch) * W1CK + 4 * h;
        float4 d[6];
#pragma unroll
        for (int q = 0; q < 6; ++q)
            d[q] = ok[q] ? *reinterpret_cast<const float4*>(src + (row0 + q) * C + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float* wp = p.w + (size_t)ch * W1PTS * 8 * Cout + (size_t)h * Cout + n0 + r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float x[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) x[q] = s == 0 ? d[q].x : s == 1 ? d[q].y : s == 2 ? d[q].z : d[q].w;
            // B^T d
            float v[W1PTS];
            v[0] = 4.f * x[0] - 5.f * x[2] + x[4];
            v[1] = (x[4] + x[3]) - 4.f * (x[1] + x[2]);
            v[2] = (x[4] - x[3]) + 4.f * (x[1] - x[2]);
            v[3] = (x[4] - x[2]) + 2.f * (x[3] - x[1]);
            v[4] = (x[4] - x[2]) - 2.f * (x[3] - x[1]);
            v[5] = 4.f * x[1] - 5.f * x[3] + x[5];
#pragma unroll
            for (int xi = 0; xi < W1PTS; ++xi) {
                const float u = wp[(size_t)(xi * 4 + s) * 2 * Cout];
                acc[xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[xi], u, acc[xi], 0, 0, 0);
            }
        }
    }

    // A^T: element e of every point is (tile row (e & 3) + 8 (e >> 2) + 4 h, cout n0 + r)
    const bool in_kernel = !p.partial;
    const float bias = in_kernel && (p.epi & EPI_BIAS) ? p.bias[n0 + r] : 0.f;
    float* out = p.out + (p.partial ? (size_t)split * p.B * L * Cout : 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int te = m0 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (te >= n_tiles) continue;
        const float a0 = acc[0][e], a1 = acc[1][e], a2 = acc[2][e], a3 = acc[3][e], a4 = acc[4][e], a5 = acc[5][e];
        const float s12 = a1 + a2, d12 = a1 - a2, s34 = a3 + a4, d34 = a3 - a4;
        float y[4] = {a0 + s12 + s34, d12 + 2.f * d34, s12 + 4.f * s34, d12 + 8.f * d34 + a5};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const size_t o = ((size_t)te * 4 + m) * Cout + n0 + r;  // tiles are consecutive groups of 4 rows of (B L, Cout)
            float val = y[m] + bias;
            if (in_kernel && (p.epi & EPI_RESIDUAL)) val += p.residual[o];
            out[o] = val;
        }
    }
}

// Where the family takes a layer: thresholds from the per-layer timing against the direct family
bool wino1d_shape_ok(int B, int L, int Cout, int C0, int C1) {
    static const int min_cin = env_int("DM_WINO1D_MIN_CIN", 256);
    static const int min_rows = env_int("DM_WINO1D_MIN_ROWS", 1024);
    (void)Cout;
    return C0 + C1 >= min_cin && (int64_t)B * L >= min_rows;
}

// K splits so that small grids still fill the device; every split owns at least one chunk
ConvGeom wino1d_plan(int B, int L, int Cout, int C0, int C1, bool allow_split) {
    static const int target_wgs = env_int("DM_WINO1D_TARGET_WGS", 256);
    ConvGeom g{};
    const int n_chunks = (C0 + C1) / W1CK;
    const int wgs = ((B * (L / 4) + 63) / 64) * (Cout / 64);
    int splits = 1;
    if (allow_split && wgs < target_wgs) splits = std::min(std::min(8, std::max(1, n_chunks / 4)), (target_wgs + wgs - 1) / wgs);
    g.chunks_per_split = (n_chunks + splits - 1) / splits;
    g.splits = (n_chunks + g.chunks_per_split - 1) / g.chunks_per_split;
    g.fused_norm = 0;  // RMSNorm lands through launch_norm_act
    g.CK = W1CK;
    return g;
}

int wino1d_launch(const ConvParams& p, hipStream_t s) {
    const int L = p.Wo;
    DM_REQUIRE(p.KH == 1 && p.KW == 3 && p.stride == 1 && p.pad_w == 1 && p.Ho == 1 && p.Hin == 1 && p.Win == L,
               "wino1d: Conv1d(3, stride 1, padding 1) over one-row images");
    DM_REQUIRE(L % 4 == 0 && p.Cout % 64 == 0 && p.C0 % W1CK == 0 && p.C1 % W1CK == 0 && p.C0 > 0, "wino1d: L % 4, Cout % 64, C % 8");
    DM_REQUIRE(!p.in_nchw && !p.out_nchw && !p.up && !p.fold && !p.s2d, "wino1d: NHWC, no resampling");
    DM_REQUIRE(p.chunks0 == p.C0 / W1CK && p.n_chunks == (p.C0 + p.C1) / W1CK, "wino1d: chunk counts");
    DM_REQUIRE(p.C1 == 0 || p.in1, "wino1d: second source");
    DM_REQUIRE(p.geo.splits >= 1 && p.geo.chunks_per_split >= 1 && p.geo.splits <= 65535, "wino1d: K splits");
    DM_REQUIRE(p.partial || (p.geo.splits == 1 && (p.epi & ~(EPI_BIAS | EPI_RESIDUAL)) == 0),
               "wino1d: the kernel applies bias and residual only, and only without a K split");
    DM_REQUIRE((size_t)p.B * L * p.Cout < ((size_t)1 << 31) && (size_t)p.B * L * (p.C0 + p.C1) < ((size_t)1 << 33), "wino1d: tensor size");
    const int tiles_per_seq = L / 4, n_tiles = p.B * tiles_per_seq;
    const dim3 grid((n_tiles + 63) / 64, p.Cout / 64, p.geo.splits);
    if (prof::enabled()) {
        char name[64];
        if (prof::detail())
            snprintf(name, sizeof(name), "wino1d 1x3 s1 %d+%d->%d @1x%d e%d k%d", p.C0, p.C1, p.Cout, L, p.epi, p.geo.splits);
        else
            snprintf(name, sizeof(name), "wino1d_mfma_kernel");
        const double cin = p.C0 + p.C1, pix = (double)p.B * L;
        if (prof::begin(name, 2.0 * 3.0 * cin * p.Cout * pix, 4.0 * (cin * pix + p.Cout * pix * p.geo.splits + 6.0 * cin * p.Cout), s))
            return 1;
    }
    hipLaunchKernelGGL(wino1d_mfma_kernel, grid, dim3(256), 0, s, p, n_tiles, tiles_per_seq);
    DM_CHECK_HIP(hipGetLastError());
    if (prof::enabled() && prof::end(s)) return 1;
    return 0;
}

}  // namespace dm
