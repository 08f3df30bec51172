// Single-operator entry points (textually included at the end of dm_api.hip).
// Test plumbing around the same launch helpers the U-Net forward uses: weights arrive as DEVICE
// pointers in the reference layout, are packed on the host per call, and every call synchronises.
namespace dm {

static int d2h(const float* dev, size_t n, std::vector<float>& out) {
    out.resize(n);
    if (n) DM_CHECK_HIP(hipMemcpy(out.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

template <class F>
static int run_op(hipStream_t s, F body) {
    Arena dry;
    dry.dry = true;
    if (body(dry)) return 1;
    void* buf = nullptr;
    DM_CHECK_HIP(hipMalloc(&buf, dry.off + 256));
    Arena A;
    A.base = static_cast<char*>(buf);
    A.cap = dry.off + 256;
    // Every float of the workspace starts as a NaN: a kernel that reads a partial-sum slot, a ragged tile or a masked row
    // nobody wrote shows up in the result instead of reading the zeros of fresh device memory.
    hipError_t e = hipMemsetAsync(buf, 0xFF, A.cap, s);
    int rc = 0;
    if (e == hipSuccess) {
        rc = body(A);
        e = hipStreamSynchronize(s);
    }
    (void)hipFree(buf);
    if (!rc && e != hipSuccess) {
        set_error(std::string("kernel execution failed: ") + hipGetErrorString(e));
        rc = 1;
    }
    return rc;
}

static float* to_nhwc(Arena& A, const float* nchw, int B, int C, int HW, hipStream_t s, int* rc) {
    float* t = A.alloc((size_t)B * C * HW);
    if (!A.dry && launch_nchw_to_nhwc(nchw, t, B, C, HW, s)) *rc = 1;
    return t;
}

static void init_dummy(dm_unet& u, int heads, int dh) {
    u.heads = heads;
    u.dh = dh;
    u.cfg.attn_heads = heads;
    u.cfg.attn_dim_head = dh;
}

}  // namespace dm

extern "C" {

int dm_op_conv2d(const float* in0, int C0, const float* in1, int C1, const float* weight, const float* bias,
                 const float* residual, float* out, int B, int H, int W, int Cout, int ksize, int pad, int up2,
                 void* stream) {
    DM_REQUIRE(in0 && weight && out, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<float> wh, bh;
    if (d2h(weight, (size_t)Cout * (C0 + C1) * ksize * ksize, wh)) return 1;
    if (bias && d2h(bias, Cout, bh)) return 1;
    dm_unet dummy;
    init_dummy(dummy, 4, 32);
    ConvLayer L;
    if (make_conv(dummy.own, L, wh.data(), bias ? bh.data() : nullptr, Cout, C0, in1 ? C1 : 0, ksize, ksize, 1, pad,
                  up2 != 0)) return 1;
    const int Hin = up2 ? 2 * H : H, Win = up2 ? 2 * W : W;
    const int Ho = Hin + 2 * pad - ksize + 1, Wo = Win + 2 * pad - ksize + 1;
    return run_op(s, [&](Arena& A) -> int {
        int rc = 0;
        Ctx c{&dummy, &A, s, B, nullptr, 0};
        if (L.packed[CONV_INIT7] && !in1 && !residual && !up2) {
            // the U-Net's first conv reads the NCHW image directly (unet_forward_impl): same call here
            float* o = A.alloc((size_t)B * Ho * Wo * Cout);
            if (run_conv(c, L, in0, nullptr, Hin, Win, o, 0, nullptr, nullptr, nullptr, /*in_nchw=*/true)) return 1;
            if (!A.dry && launch_nhwc_to_nchw(o, out, B, Cout, Ho * Wo, s)) return 1;
            return 0;
        }
        float* a0 = to_nhwc(A, in0, B, C0, H * W, s, &rc);
        float* a1 = in1 ? to_nhwc(A, in1, B, C1, H * W, s, &rc) : nullptr;
        float* r = residual ? to_nhwc(A, residual, B, Cout, Ho * Wo, s, &rc) : nullptr;
        float* o = A.alloc((size_t)B * Ho * Wo * Cout);
        if (rc) return 1;
        if (run_conv(c, L, a0, a1, Hin, Win, o, residual ? EPI_RESIDUAL : 0, nullptr, nullptr, r)) return 1;
        if (!A.dry && launch_nhwc_to_nchw(o, out, B, Cout, Ho * Wo, s)) return 1;
        return 0;
    });
}

int dm_op_downsample(const float* in, int C, const float* weight, const float* bias, float* out, int B, int H,
                     int W, int Cout, void* stream) {
    DM_REQUIRE(in && weight && out, "null argument");
    DM_REQUIRE(H % 2 == 0 && W % 2 == 0, "downsample needs even H, W");
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<float> wh, bh;
    if (d2h(weight, (size_t)Cout * 4 * C, wh)) return 1;
    if (bias && d2h(bias, Cout, bh)) return 1;
    dm_unet dummy;
    init_dummy(dummy, 4, 32);
    ConvLayer L;
    if (make_conv(dummy.own, L, wh.data(), bias ? bh.data() : nullptr, Cout, C, 0, 2, 2, 2, 0, false)) return 1;
    return run_op(s, [&](Arena& A) -> int {
        int rc = 0;
        Ctx c{&dummy, &A, s, B, nullptr, 0};
        float* a0 = to_nhwc(A, in, B, C, H * W, s, &rc);
        float* o = A.alloc((size_t)B * (H / 2) * (W / 2) * Cout);
        if (rc) return 1;
        if (run_conv(c, L, a0, nullptr, H, W, o, 0, nullptr, nullptr, nullptr)) return 1;
        if (!A.dry && launch_nhwc_to_nchw(o, out, B, Cout, (H / 2) * (W / 2), s)) return 1;
        return 0;
    });
}

int dm_op_rmsnorm(const float* x, const float* g, float* out, int B, int C, int H, int W, void* stream) {
    DM_REQUIRE(x && g && out, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_op(s, [&](Arena& A) -> int {
        int rc = 0;
        float* a = to_nhwc(A, x, B, C, H * W, s, &rc);
        float* o = A.alloc((size_t)B * C * H * W);
        if (rc) return 1;
        if (A.dry) return 0;
        if (launch_norm_act(a, 1, 0, nullptr, g, nullptr, 0, H * W, nullptr, o, (int64_t)B * H * W, C, EPI_NORM, s))
            return 1;
        return launch_nhwc_to_nchw(o, out, B, C, H * W, s);
    });
}

int dm_op_block(const float* x, int Cin, const float* weight, const float* bias, const float* g, const float* scale,
                const float* shift, float* out, int B, int H, int W, int Cout, void* stream) {
    DM_REQUIRE(x && weight && bias && g && out, "null argument");
    DM_REQUIRE((scale == nullptr) == (shift == nullptr), "scale and shift come together");
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<float> wh, bh;
    if (d2h(weight, (size_t)Cout * Cin * 9, wh) || d2h(bias, Cout, bh)) return 1;
    dm_unet dummy;
    init_dummy(dummy, 4, 32);
    ConvLayer L;
    if (make_conv(dummy.own, L, wh.data(), bh.data(), Cout, Cin, 0, 3, 3, 1, 1, false)) return 1;
    return run_op(s, [&](Arena& A) -> int {
        int rc = 0;
        Ctx c{&dummy, &A, s, B, nullptr, 0};
        float* a = to_nhwc(A, x, B, Cin, H * W, s, &rc);
        float* ss = nullptr;
        if (scale) {
            ss = A.alloc((size_t)B * 2 * Cout);
            if (!A.dry) {
                DM_CHECK_HIP(hipMemcpy2DAsync(ss, 2 * Cout * sizeof(float), scale, Cout * sizeof(float),
                                              Cout * sizeof(float), B, hipMemcpyDeviceToDevice, s));
                DM_CHECK_HIP(hipMemcpy2DAsync(ss + Cout, 2 * Cout * sizeof(float), shift, Cout * sizeof(float),
                                              Cout * sizeof(float), B, hipMemcpyDeviceToDevice, s));
            }
            c.ss_stride = 2 * Cout;
        }
        float* o = A.alloc((size_t)B * H * W * Cout);
        if (rc) return 1;
        const float* sc = scale ? (A.dry ? reinterpret_cast<const float*>(16) : ss) : nullptr;
        if (run_block(c, L, a, nullptr, H, W, g, sc, nullptr, o)) return 1;
        if (!A.dry && launch_nhwc_to_nchw(o, out, B, Cout, H * W, s)) return 1;
        return 0;
    });
}

static int attn_op(bool full, const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv,
                   const float* w_out, const float* b_out, const float* out_g, float* out, int B, int C, int H,
                   int W, int heads, int dim_head, void* stream) {
    DM_REQUIRE(x && norm_g && w_qkv && w_out && b_out && out, "null argument");  // mem_kv == NULL: no memory key / values
    DM_REQUIRE(dim_head == 32 || dim_head == 64, "dim_head: the attention kernels support 32 and 64");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int hidden = heads * dim_head;
    std::vector<float> wq, wo, bo;
    if (d2h(w_qkv, (size_t)3 * hidden * C, wq) || d2h(w_out, (size_t)C * hidden, wo) || d2h(b_out, C, bo)) return 1;
    dm_unet dummy;
    init_dummy(dummy, heads, dim_head);
    AttnLayer At;
    At.full = full;
    At.dim = C;
    At.heads = heads;
    At.norm_g = const_cast<float*>(norm_g);
    At.mem_kv = const_cast<float*>(mem_kv);
    At.out_g = const_cast<float*>(out_g);
    if (make_conv(dummy.own, At.qkv, wq.data(), nullptr, 3 * hidden, C, 0, 1, 1, 1, 0, false)) return 1;
    if (make_conv(dummy.own, At.out, wo.data(), bo.data(), C, hidden, 0, 1, 1, 1, 0, false)) return 1;
    if (!full && mem_kv) {
        // the layer as the U-Net builds it: the fused kernels where they are eligible
        std::vector<float> ng, mk, og;
        if (d2h(norm_g, C, ng) || d2h(mem_kv, (size_t)2 * hidden * 4, mk) || d2h(out_g, C, og)) return 1;
        if (fuse_linattn(dummy.own, At, wq.data(), ng.data(), wo.data(), mk.data(), og.data(), C, heads, dim_head))
            return 1;
    }
    return run_op(s, [&](Arena& A) -> int {
        int rc = 0;
        Ctx c{&dummy, &A, s, B, nullptr, 0};
        float* a = to_nhwc(A, x, B, C, H * W, s, &rc);
        if (rc) return 1;
        float* y = nullptr;
        if (run_attn(c, At, a, H, W, &y, /*add_x=*/false)) return 1;
        if (!A.dry && launch_nhwc_to_nchw(y, out, B, C, H * W, s)) return 1;
        return 0;
    });
}

int dm_op_linear_attention(const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv,
                           const float* w_out, const float* b_out, const float* out_g, float* out, int B, int C,
                           int H, int W, int heads, int dim_head, void* stream) {
    DM_REQUIRE(out_g, "null argument");
    return attn_op(false, x, norm_g, mem_kv, w_qkv, w_out, b_out, out_g, out, B, C, H, W, heads, dim_head, stream);
}

int dm_op_attention(const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv,
                    const float* w_out, const float* b_out, float* out, int B, int C, int H, int W, int heads,
                    int dim_head, void* stream) {
    return attn_op(true, x, norm_g, mem_kv, w_qkv, w_out, b_out, nullptr, out, B, C, H, W, heads, dim_head, stream);
}

int dm_profile_enable(int on) {
    prof::g_on = on != 0;
    prof::g_detail = on == 2;  // 2: one row per layer shape instead of per kernel instance
    if (on) {
        // calibrate the bracket overhead (see prof::g_overhead_ms): median of 33 empty-kernel brackets behind a parked GPU
        constexpr int N = 33;
        hipEvent_t e0[N], e1[N];
        for (int i = 0; i < N; ++i) {
            DM_CHECK_HIP(hipEventCreate(&e0[i]));
            DM_CHECK_HIP(hipEventCreate(&e1[i]));
        }
        if (launch_spin(2.0, nullptr)) return 1;
        for (int i = 0; i < N; ++i) {
            DM_CHECK_HIP(hipEventRecord(e0[i], nullptr));
            if (launch_spin(0.0, nullptr)) return 1;
            DM_CHECK_HIP(hipEventRecord(e1[i], nullptr));
        }
        DM_CHECK_HIP(hipDeviceSynchronize());
        std::vector<float> ms(N);
        for (int i = 0; i < N; ++i) {
            DM_CHECK_HIP(hipEventElapsedTime(&ms[i], e0[i], e1[i]));
            (void)hipEventDestroy(e0[i]);
            (void)hipEventDestroy(e1[i]);
        }
        std::sort(ms.begin(), ms.end());
        prof::g_overhead_ms = ms[N / 2];
    }
    return 0;
}

int dm_profile_read(dm_profile_row* rows, int max_rows, int* n_rows) {
    DM_REQUIRE(rows && n_rows && max_rows > 0, "bad argument");
    DM_CHECK_HIP(hipDeviceSynchronize());
    std::map<std::string, dm_profile_row> agg;
    for (auto& r : prof::g_recs) {
        float ms = 0.f;
        DM_CHECK_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
        dm_profile_row& a = agg[r.kernel];
        if (a.launches == 0) {
            std::memset(&a, 0, sizeof(a));
            std::snprintf(a.kernel, sizeof(a.kernel), "%s", r.kernel.c_str());
        }
        a.launches += 1;
        a.total_ms += std::max(0.0, (double)ms - prof::g_overhead_ms);
        a.total_flops += r.flops;
        a.total_bytes += r.bytes;
        prof::g_pool.push_back(r.e0);
        prof::g_pool.push_back(r.e1);
    }
    prof::g_recs.clear();
    int n = 0;
    for (auto& kv : agg) {
        if (n >= max_rows) break;
        rows[n++] = kv.second;
    }
    *n_rows = n;
    return 0;
}

int dm_op_sampler_update(int kind, int objective, const float* x, const float* eps, const float* noise,
                         const float* c_host, float* out, float* x_start, int64_t n, void* stream) {
    DM_REQUIRE(x && eps && c_host && out, "null argument");
    DM_REQUIRE(objective >= DM_OBJ_PRED_NOISE && objective <= DM_OBJ_PRED_V, "unknown objective");
    return table_op(c_host, 1, stream, [&](const float* cd, hipStream_t s) {
        return launch_sampler_update(kind, x, eps, noise, cd, nullptr, 0, out, nullptr, nullptr, n, s, objective, x_start);
    }, DM_COEFS);
}

int dm_op_sampler_update_ex(int kind, int objective, int ddim_flags, const float* x, const float* eps, const float* noise,
                            const float* c_host, float* out, float* x_start, int64_t n, void* stream) {
    DM_REQUIRE(x && eps && c_host && out, "null argument");
    DM_REQUIRE(objective >= DM_OBJ_PRED_NOISE && objective <= DM_OBJ_PRED_V, "unknown objective");
    return table_op(c_host, 1, stream, [&](const float* cd, hipStream_t s) {
        return launch_sampler_update(kind, x, eps, noise, cd, nullptr, 0, out, nullptr, nullptr, n, s, objective, x_start,
                                     nullptr, ddim_flags);
    }, DM_COEFS);
}

// a layer of the sequence model from device weights (Cout, Cin, K): 1 x K over the (B, 1, L, C) view, or the Upsample packing
static int op_conv1d_layer(dm_unet& dummy, ConvLayer& L, const float* weight, const float* bias, int Cout, int C0, int C1, int K,
                           int stride, int pad, int up2) {
    std::vector<float> wh, bh;
    if (d2h(weight, (size_t)Cout * (C0 + C1) * K, wh)) return 1;
    if (bias && d2h(bias, Cout, bh)) return 1;
    if (up2) {
        DM_REQUIRE(K == 3 && stride == 1 && pad == 1 && C1 == 0, "Upsample of the sequence model is nearest x2 + Conv1d(3, padding 1)");
        return make_upsample1d(dummy.own, L, wh.data(), bias ? bh.data() : nullptr, Cout, C0);
    }
    if (make_conv(dummy.own, L, wh.data(), bias ? bh.data() : nullptr, Cout, C0, C1, 1, K, stride, 0, false)) return 1;
    L.pad_w = pad;
    return 0;
}

int dm_op_conv1d(const float* in0, int C0, const float* in1, int C1, const float* weight, const float* bias,
                 const float* residual, float* out, int B, int L, int Cout, int K, int stride, int pad, int up2,
                 void* stream) {
    DM_REQUIRE(in0 && weight && out, "null argument");
    DM_REQUIRE(B > 0 && L > 0 && Cout > 0 && C0 > 0 && K >= 1 && (stride == 1 || stride == 2) && pad >= 0 && L + 2 * pad >= K,
               "bad convolution shape");
    DM_REQUIRE(!up2 || !residual, "the Upsample layer has no residual");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!in1) C1 = 0;
    dm_unet dummy;
    init_dummy(dummy, 4, 32);
    ConvLayer Lc;
    if (op_conv1d_layer(dummy, Lc, weight, bias, Cout, C0, C1, K, stride, pad, up2)) return 1;
    const int Lo = up2 ? 2 * L : (L + 2 * pad - K) / stride + 1;
    return run_op(s, [&](Arena& A) -> int {
        int rc = 0;
        Ctx c{&dummy, &A, s, B, nullptr, 0};
        float* o = A.alloc((size_t)B * Lo * Cout);
        if (C1 == 0 && C0 <= 8 && !residual && !up2 && stride == 1) {
            // init_conv reads the (B, C, L) tensor as it is (unet_forward_impl): same call here
            if (run_conv(c, Lc, in0, nullptr, 1, L, o, 0, nullptr, nullptr, nullptr, /*in_nchw=*/true)) return 1;
            if (!A.dry && launch_nhwc_to_nchw(o, out, B, Cout, Lo, s)) return 1;
            return 0;
        }
        float* a0 = to_nhwc(A, in0, B, C0, L, s, &rc);
        float* a1 = C1 ? to_nhwc(A, in1, B, C1, L, s, &rc) : nullptr;
        float* r = residual ? to_nhwc(A, residual, B, Cout, Lo, s, &rc) : nullptr;
        if (rc) return 1;
        // the Upsample layer's (B, L, 2 Cout) result is the (B, 2L, Cout) tensor
        if (run_conv(c, Lc, a0, a1, 1, L, o, residual ? EPI_RESIDUAL : 0, nullptr, nullptr, r)) return 1;
        if (!A.dry && launch_nhwc_to_nchw(o, out, B, Cout, Lo, s)) return 1;
        return 0;
    });
}

int dm_op_block1d(const float* x0, int C0, const float* x1, int C1, const float* weight, const float* bias, const float* g,
                  const float* scale, const float* shift, const float* residual, float* out, int B, int L, int Cout,
                  void* stream) {
    DM_REQUIRE(x0 && weight && bias && g && out, "null argument");
    DM_REQUIRE((scale == nullptr) == (shift == nullptr), "scale and shift come together");
    DM_REQUIRE(B > 0 && L > 0 && Cout > 0 && C0 > 0, "bad block shape");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!x1) C1 = 0;
    dm_unet dummy;
    init_dummy(dummy, 4, 32);
    ConvLayer Lc;
    if (op_conv1d_layer(dummy, Lc, weight, bias, Cout, C0, C1, 3, 1, 1, 0)) return 1;
    return run_op(s, [&](Arena& A) -> int {
        int rc = 0;
        Ctx c{&dummy, &A, s, B, nullptr, 0};
        float* a0 = to_nhwc(A, x0, B, C0, L, s, &rc);
        float* a1 = C1 ? to_nhwc(A, x1, B, C1, L, s, &rc) : nullptr;
        float* r = residual ? to_nhwc(A, residual, B, Cout, L, s, &rc) : nullptr;
        float* ss = nullptr;
        if (scale) {
            ss = A.alloc((size_t)B * 2 * Cout);
            if (!A.dry) {
                DM_CHECK_HIP(hipMemcpy2DAsync(ss, 2 * Cout * sizeof(float), scale, Cout * sizeof(float),
                                              Cout * sizeof(float), B, hipMemcpyDeviceToDevice, s));
                DM_CHECK_HIP(hipMemcpy2DAsync(ss + Cout, 2 * Cout * sizeof(float), shift, Cout * sizeof(float),
                                              Cout * sizeof(float), B, hipMemcpyDeviceToDevice, s));
            }
            c.ss_stride = 2 * Cout;
        }
        float* o = A.alloc((size_t)B * L * Cout);
        if (rc) return 1;
        const float* sc = scale ? (A.dry ? reinterpret_cast<const float*>(16) : ss) : nullptr;
        const float* rr = residual ? (A.dry ? reinterpret_cast<const float*>(16) : r) : nullptr;
        if (run_block(c, Lc, a0, a1, 1, L, g, sc, rr, o)) return 1;
        if (!A.dry && launch_nhwc_to_nchw(o, out, B, Cout, L, s)) return 1;
        return 0;
    });
}

int dm_op_dpmpp_update(int objective, const float* x, const float* model_out, float* x0_hist, const float* coef_host,
                       float* out, int64_t n, void* stream) {
    DM_REQUIRE(x && model_out && x0_hist && coef_host && out, "null argument");
    DM_REQUIRE(n > 0, "empty tensor");
    DM_REQUIRE(objective >= DM_OBJ_PRED_NOISE && objective <= DM_OBJ_PRED_V, "unknown objective");
    return table_op(coef_host, 1, stream, [&](const float* cd, hipStream_t s) {
        return launch_dpmpp_update(x, model_out, x0_hist, cd, nullptr, out, nullptr, nullptr, n, s, objective);
    }, DM_COEFS);
}

int dm_op_dyn_threshold(int objective, const float* x, const float* model_out, const float* c_host, int B, int64_t per,
                        double percentile, float* s_out, void* stream) {
    DM_REQUIRE(x && model_out && c_host && s_out, "null argument");
    DM_REQUIRE(B > 0 && per > 0, "empty tensor");
    DM_REQUIRE(objective >= DM_OBJ_PRED_NOISE && objective <= DM_OBJ_PRED_V, "unknown objective");
    DM_REQUIRE(percentile > 0.0 && percentile <= 1.0, "the percentile of dynamic thresholding lies in (0, 1]");
    return table_op(c_host, 1, stream, [&](const float* cd, hipStream_t s) {
        return launch_dyn_threshold(objective, x, model_out, cd, nullptr, nullptr, dyn_params(percentile, per), B, per, s_out, s);
    }, DM_COEFS);
}

int dm_op_sampler_update_dyn(int kind, int objective, const float* x, const float* eps, const float* noise,
                             const float* c_host, const float* s, int B, int64_t per, float* out, float* x_start,
                             void* stream) {
    DM_REQUIRE(x && eps && c_host && s && out, "null argument");
    DM_REQUIRE(B > 0 && per > 0, "empty tensor");
    DM_REQUIRE(kind == DM_SAMPLER_DDPM || kind == DM_SAMPLER_DDIM, "the update of the DDPM or the DDIM loop");
    DM_REQUIRE(objective >= DM_OBJ_PRED_NOISE && objective <= DM_OBJ_PRED_V, "unknown objective");
    const int64_t n = (int64_t)B * per;
    return table_op(c_host, 1, stream, [&](const float* cd, hipStream_t st) {
        return launch_sampler_update(kind, x, eps, noise, cd, nullptr, 0, out, nullptr, nullptr, n, st, objective, x_start,
                                     nullptr, 0, s, per);
    }, DM_COEFS);
}

int dm_op_dpmpp_update_dyn(int objective, const float* x, const float* model_out, float* x0_hist, const float* coef_host,
                           const float* s, int B, int64_t per, float* out, void* stream) {
    DM_REQUIRE(x && model_out && x0_hist && coef_host && s && out, "null argument");
    DM_REQUIRE(B > 0 && per > 0, "empty tensor");
    DM_REQUIRE(objective >= DM_OBJ_PRED_NOISE && objective <= DM_OBJ_PRED_V, "unknown objective");
    const int64_t n = (int64_t)B * per;
    return table_op(coef_host, 1, stream, [&](const float* cd, hipStream_t st) {
        return launch_dpmpp_update(x, model_out, x0_hist, cd, nullptr, out, nullptr, nullptr, n, st, objective, s, per);
    }, DM_COEFS);
}

int dm_op_cfg_combine(const float* cond, const float* null_out, float* out, int B, int64_t per_sample, float cond_scale,
                      float rescaled_phi, int remove_parallel_component, float keep_parallel_frac, void* stream) {
    DM_REQUIRE(cond && null_out && out, "null argument");
    DM_REQUIRE(B > 0 && per_sample > 1, "dm_op_cfg_combine needs B > 0 and more than one value per sample");
    DM_REQUIRE(out != cond && out != null_out, "dm_op_cfg_combine does not run in place");
    DM_REQUIRE(remove_parallel_component == 0 || remove_parallel_component == 1, "remove_parallel_component is 0 or 1");
    const CfgParams p{cond_scale, rescaled_phi, keep_parallel_frac, (float)remove_parallel_component};
    return launch_cfg_combine(cond, null_out, out, B, per_sample, nullptr, p, static_cast<hipStream_t>(stream));
}

}  // extern "C"
