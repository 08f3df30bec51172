// Single-operator backward entry points (dm_op_*_bwd): the pieces of the training step exposed one at a time so that
// parity tests can check each against the reference module's autograd at shapes the U-Net does not produce (odd sizes,
// two-source inputs, upsampled sources, any channel count that is a multiple of 4).  Same plumbing as dm_ops.inc: weights
// arrive as DEVICE pointers in the reference layout, are packed on the host per call, every call synchronises.
// The conditioning head (dm_unet_cond_forward / dm_unet_cond_backward, on a real handle) and the deferred reduction tables
// (dm_op_deferred_reduce) are not restated here: these entry points call the functions the walks call.
// Textually included after dm_train.inc.
namespace dm {

// a throw-away handle with host parameters `names` and a gradient slot for each
struct OpTrain {
    dm_unet u;
    OpTrain(int heads, int dh) {
        init_dummy(u, heads, dh);
        u.train = new TrainState();
    }
    ~OpTrain() { free_train(&u); }
    int param(const std::string& name, const float* dev, std::vector<int64_t> shape) {
        HostTensor t;
        t.shape = std::move(shape);
        if (dev && d2h(dev, t.numel(), t.data)) return 1;
        if (!dev) t.data.assign(t.numel(), 0.f);
        t.set = true;
        u.params[name] = std::move(t);
        u.order.push_back(name);
        return 0;
    }
    int alloc_grads(bool poison = false) {  // poison: NaN instead of 0 (operators that overwrite every slot they return)
        TrainState& T = *u.train;
        size_t off = 0;
        for (const std::string& n : u.order) {
            T.off[n] = off;
            off += (u.params.at(n).numel() + 3) & ~size_t(3);
        }
        T.grad_floats = off;
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&T.grad), std::max<size_t>(off, 4) * sizeof(float)));
        DM_CHECK_HIP(hipMemset(T.grad, poison ? 0xFF : 0, std::max<size_t>(off, 4) * sizeof(float)));
        return 0;
    }
    int out(const std::string& name, float* dst, hipStream_t s) {  // gradient slot -> caller's device buffer
        if (!dst) return 0;
        DM_CHECK_HIP(hipMemcpyAsync(dst, u.train->grad + u.train->off.at(name), u.params.at(name).numel() * sizeof(float),
                                    hipMemcpyDeviceToDevice, s));
        return 0;
    }
};

static int from_nhwc(Arena& A, const float* nhwc, float* nchw, int B, int C, int HW, hipStream_t s) {
    if (A.dry || !nchw || !nhwc) return 0;
    return launch_nhwc_to_nchw(nhwc, nchw, B, C, HW, s);
}

// one CrossAttention layer "c" on a throw-away handle, packed by build_cross_body as the text-conditional U-Net packs its
// three; train: gradient slots and the input-gradient layers of to_q / to_out as build_train makes them
static int cross_op_layer(OpTrain& op, CrossLayer& Cr, const float* w_q, const float* w_k, const float* w_v, const float* w_out,
                          const float* b_out, const float* out_g, int C, int E, int dim_head, bool train) {
    const int inner = 4 * dim_head;
    op.u.cfg.text_emb_dim = E;  // run_cross / t_cross take the context width from the handle
    if (op.param("c.to_q.weight", w_q, {inner, C}) || op.param("c.to_k.weight", w_k, {inner, E}) ||
        op.param("c.to_v.weight", w_v, {inner, E}) || op.param("c.to_out.0.weight", w_out, {C, inner}) ||
        op.param("c.to_out.0.bias", b_out, {C}) || op.param("c.to_out.1.g", out_g, {1, C}))
        return 1;
    if (build_cross_body(&op.u, Cr, "c", C)) return 1;
    if (!train) return 0;
    if (op.alloc_grads()) return 1;
    return build_conv_bwd(&op.u, *op.u.train, Cr.q, CB_1X1) || build_conv_bwd(&op.u, *op.u.train, Cr.out, CB_1X1);
}

static bool cross_op_args_ok(int B, int C, int H, int W, int m, int E, int dim_head) {
    return B > 0 && C > 0 && H > 0 && W > 0 && m > 0 && E > 0 && (dim_head == 32 || dim_head == 64);
}

// what dm_unet_cond_forward / dm_unet_cond_backward ask of the handle and the conditioning arguments
static int cond_args_ok(dm_unet* u, const float* ctx, const int32_t* text_mask, int B) {
    DM_REQUIRE(u->finalized, "dm_unet_finalize has not been called");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    DM_REQUIRE(B > 0, "empty batch");
    DM_REQUIRE(!ctx || u->cfg.text_mode != DM_TEXT_NONE, "the U-Net was built without text conditioning");
    DM_REQUIRE(!text_mask || ctx, "a text mask needs a text-conditional U-Net and a pooled caption");
    return 0;
}
static int copy_out(float* dst, const float* src, size_t n, hipStream_t s) {
    if (dst && src) DM_CHECK_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // namespace dm

extern "C" {

int dm_op_conv2d_bwd(const float* in0, int C0, const float* in1, int C1, const float* weight, const float* dy, float* d_in0,
                     float* d_in1, float* d_weight, float* d_bias, int B, int H, int W, int Cout, int ksize, int pad, int up2,
                     void* stream) {
    DM_REQUIRE(in0 && weight && dy, "null argument");
    DM_REQUIRE((ksize == 3 && pad == 1) || (ksize == 1 && pad == 0), "conv2d_bwd: 3x3 / pad 1 or 1x1");
    DM_REQUIRE(!up2 || ksize == 3, "conv2d_bwd: up2 goes with the 3x3 convolution");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        OpTrain op(4, 32);
        const int C1e = in1 ? C1 : 0;
        if (op.param("w", weight, {Cout, C0 + C1e, ksize, ksize}) || op.param("b", nullptr, {Cout}) || op.alloc_grads(true)) return 1;
        ConvLayer L;  // packed without its bias (no forward runs here); "b" is only the slot of the bias gradient
        L.src.wname = "w";
        L.src.bname = "b";
        if (make_conv(op.u.own, L, op.u.params["w"].data.data(), nullptr, Cout, C0, C1e, ksize, ksize, 1, pad, up2 != 0)) return 1;
        if (build_conv_bwd(&op.u, *op.u.train, L, ksize == 3 ? CB_3X3 : CB_1X1)) return 1;
        const int Ho = up2 ? 2 * H : H, Wo = up2 ? 2 * W : W;
        int rc = run_op(s, [&](Arena& A) -> int {
            int e = 0;
            TCtx t{&op.u, &A, s, B, nullptr, 0};
            float* a0 = to_nhwc(A, in0, B, C0, H * W, s, &e);
            float* a1 = in1 ? to_nhwc(A, in1, B, C1, H * W, s, &e) : nullptr;
            float* g = to_nhwc(A, dy, B, Cout, Ho * Wo, s, &e);
            if (e) return 1;
            if (conv_wgrad(t, L, a0, a1, g, Ho, Wo, true)) return 1;
            float *dx0 = nullptr, *dx1 = nullptr;
            if (conv_dgrad(t, L, g, H, W, nullptr, nullptr, &dx0, &dx1)) return 1;
            if (from_nhwc(A, dx0, d_in0, B, C0, H * W, s)) return 1;
            if (in1 && from_nhwc(A, dx1, d_in1, B, C1, H * W, s)) return 1;
            if (!A.dry && (op.out("w", d_weight, s) || op.out("b", d_bias, s))) return 1;
            return 0;
        });
        return rc;
    });
}

int dm_op_downsample_bwd(const float* in, int C, const float* weight, const float* dy, float* d_in, float* d_weight,
                         float* d_bias, int B, int H, int W, int Cout, void* stream) {
    DM_REQUIRE(in && weight && dy, "null argument");
    DM_REQUIRE(H % 2 == 0 && W % 2 == 0, "downsample needs even H, W");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        OpTrain op(4, 32);
        if (op.param("w", weight, {Cout, 4 * C, 1, 1}) || op.param("b", nullptr, {Cout}) || op.alloc_grads(true)) return 1;
        ConvLayer L;  // (as in dm_op_conv2d_bwd)
        L.src.wname = "w";
        L.src.bname = "b";
        if (make_conv(op.u.own, L, op.u.params["w"].data.data(), nullptr, Cout, C, 0, 2, 2, 2, 0, false)) return 1;
        if (build_conv_bwd(&op.u, *op.u.train, L, CB_DOWN)) return 1;
        return run_op(s, [&](Arena& A) -> int {
            int e = 0;
            TCtx t{&op.u, &A, s, B, nullptr, 0};
            float* a0 = to_nhwc(A, in, B, C, H * W, s, &e);
            float* g = to_nhwc(A, dy, B, Cout, (H / 2) * (W / 2), s, &e);
            if (e) return 1;
            float* dx = nullptr;
            if (t_conv_bwd(t, L, a0, g, H, W, H / 2, W / 2, nullptr, &dx)) return 1;
            if (from_nhwc(A, dx, d_in, B, C, H * W, s)) return 1;
            if (!A.dry && (op.out("w", d_weight, s) || op.out("b", d_bias, s))) return 1;
            return 0;
        });
    });
}

int dm_op_block_bwd(const float* x, int Cin, const float* weight, const float* bias, const float* g, const float* scale,
                    const float* shift, const float* dy, float* dx, float* d_weight, float* d_bias, float* d_g,
                    float* d_scale, float* d_shift, int B, int H, int W, int Cout, void* stream) {
    DM_REQUIRE(x && weight && bias && g && dy, "null argument");
    DM_REQUIRE((scale == nullptr) == (shift == nullptr), "scale and shift come together");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        OpTrain op(4, 32);
        if (op.param("blk.proj.weight", weight, {Cout, Cin, 3, 3}) || op.param("blk.proj.bias", bias, {Cout}) ||
            op.param("blk.norm.g", g, {1, Cout, 1, 1}) || op.alloc_grads(true))
            return 1;
        ConvLayer L;
        if (make_conv(&op.u, L, "blk.proj.weight", "blk.proj.bias", Cout, Cin, 0, 3, 3, 1, 1, false)) return 1;
        if (build_conv_bwd(&op.u, *op.u.train, L, CB_3X3)) return 1;
        op.u.ss_total = 2 * Cout;
        return run_op(s, [&](Arena& A) -> int {
            int e = 0;
            TCtx t{&op.u, &A, s, B, nullptr, 0};
            float* a = to_nhwc(A, x, B, Cin, H * W, s, &e);
            float* gy = to_nhwc(A, dy, B, Cout, H * W, s, &e);
            float* ss = nullptr;
            float* dss = A.alloc((size_t)B * 2 * Cout);
            if (scale) {
                ss = A.alloc((size_t)B * 2 * Cout);
                if (!A.dry) {
                    DM_CHECK_HIP(hipMemcpy2DAsync(ss, 2 * Cout * sizeof(float), scale, Cout * sizeof(float),
                                                  Cout * sizeof(float), B, hipMemcpyDeviceToDevice, s));
                    DM_CHECK_HIP(hipMemcpy2DAsync(ss + Cout, 2 * Cout * sizeof(float), shift, Cout * sizeof(float),
                                                  Cout * sizeof(float), B, hipMemcpyDeviceToDevice, s));
                }
                t.ss_stride = 2 * Cout;
                t.ss = A.dry ? reinterpret_cast<const float*>(16) : ss;
            }
            if (e) return 1;
            BlockTape bt;
            if (t_block(t, L, a, nullptr, H, W, g, scale ? t.ss : nullptr, nullptr, bt)) return 1;
            float* du = nullptr;
            if (t_block_bwd(t, L, bt, DyParts{gy}, H, W, g, scale ? t.ss : nullptr, 0, dss, "blk", &du)) return 1;
            float *d0 = nullptr, *none = nullptr;
            if (conv_dgrad(t, L, du, H, W, nullptr, nullptr, &d0, &none)) return 1;
            if (from_nhwc(A, d0, dx, B, Cin, H * W, s)) return 1;
            if (A.dry) return 0;
            if (op.out("blk.proj.weight", d_weight, s) || op.out("blk.proj.bias", d_bias, s) || op.out("blk.norm.g", d_g, s))
                return 1;
            if (scale && d_scale)
                DM_CHECK_HIP(hipMemcpy2DAsync(d_scale, Cout * sizeof(float), dss, 2 * Cout * sizeof(float), Cout * sizeof(float),
                                              B, hipMemcpyDeviceToDevice, s));
            if (scale && d_shift)
                DM_CHECK_HIP(hipMemcpy2DAsync(d_shift, Cout * sizeof(float), dss + Cout, 2 * Cout * sizeof(float),
                                              Cout * sizeof(float), B, hipMemcpyDeviceToDevice, s));
            return 0;
        });
    });
}

/* nn.Linear backward (time_mlp :280-285, ResnetBlock.mlp :127-130 without the SiLU): dx = dy W, dW (+)= dy^T x,
 * db (+)= column sums of dy; x (R, I), weight (O, I), dy (R, O), all row-major device pointers.  Goes through the
 * launchers of the training step (the MFMA GEMMs of small_gemm.hip where the shapes allow, else the VALU kernels) in
 * their contiguous form only (ldx = I, ldy = O, one weight block, immediate column sum); the strided, row-pointer-table
 * and shared forms the step uses are reached by dm_unet_cond_backward, its deferred reductions by dm_op_deferred_reduce. */
int dm_op_linear_bwd(const float* x, const float* weight, const float* dy, float* dx, float* d_weight, float* d_bias, int R,
                     int I, int O, int accumulate, void* stream) {
    DM_REQUIRE(x && weight && dy && R > 0 && I > 0 && O > 0, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_op(s, [&](Arena& A) -> int {
        float* ws = A.alloc(std::max<size_t>(linear_dgrad_ws_floats(R, I, O), 4));
        float* cw = A.alloc(colsum_ws_floats(R, O));
        if (A.dry) return 0;
        if (dx && launch_linear_dgrad(dy, O, weight, dx, I, R, I, O, ws, s)) return 1;
        if (d_weight && launch_linear_wgrad(dy, O, x, I, d_weight, R, I, O, 0, accumulate, s)) return 1;
        if (d_bias && launch_colsum(dy, R, O, O, 1, cw, d_bias, accumulate, s)) return 1;
        return 0;
    });
}

int dm_op_rmsnorm_bwd(const float* x, const float* g, const float* dy, float* dx, float* dg, int B, int C, int H, int W,
                      void* stream) {
    DM_REQUIRE(x && g && dy && dx, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_op(s, [&](Arena& A) -> int {
        int e = 0;
        float* a = to_nhwc(A, x, B, C, H * W, s, &e);
        float* gy = to_nhwc(A, dy, B, C, H * W, s, &e);
        float* d = A.alloc((size_t)B * C * H * W);
        float* ws = A.alloc(norm_act_bwd_ws_floats(B, H * W, C));
        float* gg = A.alloc(C);
        if (e) return 1;
        if (A.dry) return 0;
        if (launch_norm_act_bwd(gy, a, g, nullptr, 0, H * W, d, ws, gg, nullptr, nullptr, 0, B, C, EPI_NORM, 0, s)) return 1;
        if (dg) DM_CHECK_HIP(hipMemcpyAsync(dg, gg, C * sizeof(float), hipMemcpyDeviceToDevice, s));
        return launch_nhwc_to_nchw(d, dx, B, C, H * W, s);
    });
}

static int attn_bwd_op(bool full, const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv,
                       const float* w_out, const float* b_out, const float* out_g, const float* dy, float* dx,
                       float* d_norm_g, float* d_mem_kv, float* d_w_qkv, float* d_w_out, float* d_b_out, float* d_out_g,
                       int B, int C, int H, int W, int heads, int dim_head, void* stream) {
    DM_REQUIRE(x && norm_g && mem_kv && w_qkv && w_out && b_out && dy && dx, "null argument");
    DM_REQUIRE(dim_head == 32 || dim_head == 64, "dim_head: the attention kernels support 32 and 64");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        const int hidden = heads * dim_head;
        OpTrain op(heads, dim_head);
        const std::string wo = full ? "a.to_out.weight" : "a.to_out.0.weight", bo = full ? "a.to_out.bias" : "a.to_out.0.bias";
        if (op.param("a.norm.g", norm_g, {1, C, 1, 1}) ||
            op.param("a.mem_kv", mem_kv, full ? std::vector<int64_t>{2, heads, 4, dim_head} : std::vector<int64_t>{2, heads, dim_head, 4}) ||
            op.param("a.to_qkv.weight", w_qkv, {3 * hidden, C, 1, 1}) || op.param(wo, w_out, {C, hidden, 1, 1}) ||
            op.param(bo, b_out, {C}) || (!full && op.param("a.to_out.1.g", out_g, {1, C, 1, 1})) || op.alloc_grads())
            return 1;
        AttnLayer At;
        At.prefix = "a";
        At.full = full;
        At.dim = C;
        At.heads = heads;
        At.norm_g = const_cast<float*>(norm_g);
        At.mem_kv = const_cast<float*>(mem_kv);
        At.out_g = const_cast<float*>(out_g);
        if (make_conv(&op.u, At.qkv, "a.to_qkv.weight", "", 3 * hidden, C, 0, 1, 1, 1, 0, false)) return 1;
        if (make_conv(&op.u, At.out, wo, bo, C, hidden, 0, 1, 1, 1, 0, false)) return 1;
        if (build_attn_bwd(&op.u, *op.u.train, At)) return 1;
        return run_op(s, [&](Arena& A) -> int {
            int e = 0;
            TCtx t{&op.u, &A, s, B, nullptr, 0};
            float* a = to_nhwc(A, x, B, C, H * W, s, &e);
            float* gy = to_nhwc(A, dy, B, C, H * W, s, &e);
            if (e) return 1;
            AttnTape at;
            if (t_attn(t, At, a, H, W, at)) return 1;
            float* d = nullptr;
            if (t_attn_bwd(t, At, at, gy, H, W, &d, /*add_x=*/false)) return 1;  // the module alone, no "+ x"
            if (from_nhwc(A, d, dx, B, C, H * W, s)) return 1;
            if (A.dry) return 0;
            if (op.out("a.norm.g", d_norm_g, s) || op.out("a.mem_kv", d_mem_kv, s) || op.out("a.to_qkv.weight", d_w_qkv, s) ||
                op.out(wo, d_w_out, s) || op.out(bo, d_b_out, s) || (!full && op.out("a.to_out.1.g", d_out_g, s)))
                return 1;
            return 0;
        });
    });
}

int dm_op_linear_attention_bwd(const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv,
                               const float* w_out, const float* b_out, const float* out_g, const float* dy, float* dx,
                               float* d_norm_g, float* d_mem_kv, float* d_w_qkv, float* d_w_out, float* d_b_out,
                               float* d_out_g, int B, int C, int H, int W, int heads, int dim_head, void* stream) {
    DM_REQUIRE(out_g, "null argument");
    return attn_bwd_op(false, x, norm_g, mem_kv, w_qkv, w_out, b_out, out_g, dy, dx, d_norm_g, d_mem_kv, d_w_qkv, d_w_out,
                       d_b_out, d_out_g, B, C, H, W, heads, dim_head, stream);
}

int dm_op_attention_bwd(const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv, const float* w_out,
                        const float* b_out, const float* dy, float* dx, float* d_norm_g, float* d_mem_kv, float* d_w_qkv,
                        float* d_w_out, float* d_b_out, int B, int C, int H, int W, int heads, int dim_head, void* stream) {
    return attn_bwd_op(true, x, norm_g, mem_kv, w_qkv, w_out, b_out, nullptr, dy, dx, d_norm_g, d_mem_kv, d_w_qkv, d_w_out,
                       d_b_out, nullptr, B, C, H, W, heads, dim_head, stream);
}

/* The two attention cores of the training step on their own: the forward core as t_attn launches it (LinearAttention: with
 * the key statistics), then the backward core and the column sum over the images as t_attn_bwd does.  qkv, dout, out and
 * dqkv are token rows, the layout the kernels take, and every output the caller passes is written by the kernels
 * themselves (no copy in between): a stray row or an unwritten column shows in the caller's buffer.  An output that is
 * NULL lives in the NaN-filled arena instead. */
int dm_op_linear_attention_core_bwd(const float* qkv, const float* mem_kv, const float* dout, float* out, float* ctx,
                                    float* kstats, float* dqkv, float* dmem_part, float* d_mem_kv, int B, int n, int heads,
                                    int dim_head, void* stream) {
    DM_REQUIRE(qkv && mem_kv && dout, "null argument");
    DM_REQUIRE(dim_head == 32 || dim_head == 64, "dim_head: the attention kernels support 32 and 64");
    DM_REQUIRE(B > 0 && n > 0 && heads >= 1 && heads <= 16, "linear_attention_core_bwd: positive sizes, 1..16 heads");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_op(s, [&](Arena& A) -> int {
        const size_t rows = (size_t)B * n, hidden = (size_t)heads * dim_head, nmem = 2 * hidden * 4;
        float* o = out ? out : A.alloc(rows * hidden);
        float* cx = ctx ? ctx : A.alloc((size_t)B * hidden * dim_head);
        float* kst = kstats ? kstats : A.alloc((size_t)B * 2 * hidden);
        float* dq = dqkv ? dqkv : A.alloc(rows * 3 * hidden);
        float* dmem = dmem_part ? dmem_part : A.alloc((size_t)B * nmem);
        float* dm_sum = d_mem_kv ? d_mem_kv : A.alloc(nmem);
        float* cw = A.alloc(colsum_ws_floats(B, (int)nmem));
        float* ws = A.alloc(linattn_bwd_ws_floats(B, n, heads, dim_head));
        if (A.dry) return 0;
        if (launch_linear_attention_core(qkv, mem_kv, cx, o, B, n, heads, dim_head, s, kst)) return 1;
        if (launch_linear_attention_core_bwd(qkv, mem_kv, cx, dout, ws, dq, dmem, B, n, heads, dim_head, s, kst)) return 1;
        return launch_colsum(dmem, B, (int)nmem, (int64_t)nmem, 1, cw, dm_sum, 0, s);
    });
}

int dm_op_attention_core_bwd(const float* qkv, const float* mem_kv, const float* dout, float* out, float* dqkv,
                             float* dmem_part, float* d_mem_kv, int B, int n, int heads, int dim_head, void* stream) {
    DM_REQUIRE(qkv && mem_kv && dout, "null argument");
    DM_REQUIRE(dim_head == 32 || dim_head == 64, "dim_head: the attention kernels support 32 and 64");
    DM_REQUIRE(B > 0 && n > 0 && heads >= 1, "attention_core_bwd: positive sizes");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_op(s, [&](Arena& A) -> int {
        const size_t rows = (size_t)B * n, hidden = (size_t)heads * dim_head, nmem = 2 * hidden * 4;
        float* o = out ? out : A.alloc(rows * hidden);
        float* dq = dqkv ? dqkv : A.alloc(rows * 3 * hidden);
        float* dmem = dmem_part ? dmem_part : A.alloc((size_t)B * nmem);
        float* dm_sum = d_mem_kv ? d_mem_kv : A.alloc(nmem);
        float* cw = A.alloc(colsum_ws_floats(B, (int)nmem));
        float* ws = A.alloc(attn_bwd_ws_floats(B, n, n, 4, heads, dim_head));
        if (A.dry) return 0;
        const int hid = (int)hidden;
        if (launch_attention_core(qkv, 3 * hid, qkv + hid, qkv + 2 * hid, 3 * hid, mem_kv, mem_kv + hidden * 4, 4, o, hid, B, n, n,
                                  heads, dim_head, 1.0f / sqrtf((float)dim_head), s))
            return 1;
        if (launch_attention_core_bwd(qkv, mem_kv, dout, dq, dmem, ws, B, n, heads, dim_head, s)) return 1;
        return launch_colsum(dmem, B, (int)nmem, (int64_t)nmem, 1, cw, dm_sum, 0, s);
    });
}

/* CrossAttention (DD/denoising_diffusion_text_conditional.py:54-78) as the text-conditional U-Net runs it: the forward is
 * run_cross (one-token algebra included), the backward t_cross then t_cross_bwd (always the general path; y_out is its
 * forward result).  The forward sits here, next to its backward, because both build the layer on an OpTrain handle. */
int dm_op_cross_attention(const float* x, const float* ctx, const float* w_q, const float* w_k, const float* w_v,
                          const float* w_out, const float* b_out, const float* out_g, const int32_t* text_mask, float* out,
                          int B, int C, int H, int W, int m, int E, int dim_head, void* stream) {
    DM_REQUIRE(x && ctx && w_q && w_k && w_v && w_out && b_out && out_g && out, "null argument");
    DM_REQUIRE(cross_op_args_ok(B, C, H, W, m, E, dim_head), "cross_attention: positive sizes, dim_head 32 or 64");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        OpTrain op(4, dim_head);
        CrossLayer Cr;
        if (cross_op_layer(op, Cr, w_q, w_k, w_v, w_out, b_out, out_g, C, E, dim_head, false)) return 1;
        return run_op(s, [&](Arena& A) -> int {
            int e = 0;
            Ctx c{&op.u, &A, s, B, nullptr, 0};
            float* a = to_nhwc(A, x, B, C, H * W, s, &e);
            if (e) return 1;
            float* y = nullptr;
            if (run_cross(c, Cr, a, H, W, ctx, m, &y, text_mask)) return 1;
            return from_nhwc(A, y, out, B, C, H * W, s);
        });
    });
}

int dm_op_cross_attention_bwd(const float* x, const float* ctx, const float* w_q, const float* w_k, const float* w_v,
                              const float* w_out, const float* b_out, const float* out_g, const int32_t* text_mask,
                              const float* dy, float* y_out, float* dx, float* d_w_q, float* d_w_k, float* d_w_v,
                              float* d_w_out, float* d_b_out, float* d_out_g, int B, int C, int H, int W, int m, int E,
                              int dim_head, void* stream) {
    DM_REQUIRE(x && ctx && w_q && w_k && w_v && w_out && b_out && out_g && dy && dx, "null argument");
    DM_REQUIRE(cross_op_args_ok(B, C, H, W, m, E, dim_head), "cross_attention_bwd: positive sizes, dim_head 32 or 64");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        OpTrain op(4, dim_head);
        CrossLayer Cr;
        if (cross_op_layer(op, Cr, w_q, w_k, w_v, w_out, b_out, out_g, C, E, dim_head, true)) return 1;
        return run_op(s, [&](Arena& A) -> int {
            int e = 0;
            TCtx t{&op.u, &A, s, B, nullptr, 0};
            float* a = to_nhwc(A, x, B, C, H * W, s, &e);
            float* gy = to_nhwc(A, dy, B, C, H * W, s, &e);
            if (e) return 1;
            CrossTape ct;
            if (t_cross(t, Cr, a, H, W, ctx, m, ct, text_mask)) return 1;
            if (from_nhwc(A, ct.y, y_out, B, C, H * W, s)) return 1;
            float* d = nullptr;
            if (t_cross_bwd(t, Cr, ct, gy, H, W, ctx, m, &d, text_mask)) return 1;
            if (from_nhwc(A, d, dx, B, C, H * W, s)) return 1;
            if (A.dry) return 0;
            if (op.out("c.to_q.weight", d_w_q, s) || op.out("c.to_k.weight", d_w_k, s) || op.out("c.to_v.weight", d_w_v, s) ||
                op.out("c.to_out.0.weight", d_w_out, s) || op.out("c.to_out.0.bias", d_b_out, s) ||
                op.out("c.to_out.1.g", d_out_g, s))
                return 1;
            return 0;
        });
    });
}

/* The conditioning head on its own, on a finalized handle: the function the chosen walk itself runs (cond_forward of the
 * inference walk, cond_train_forward of the training forward), in a NaN-filled workspace, then a copy of every
 * intermediate the caller asked for. */
int dm_unet_cond_forward(dm_unet* u, int walk, int time_kind, const void* time, const float* ctx, const int32_t* text_mask,
                         const dm_cond_bufs* out, int B, void* stream) {
    DM_REQUIRE(u && time && out, "null argument");
    DM_REQUIRE(!u->kunet, "dm_unet_cond_forward: the conditioning head of the image U-Net; a KarrasUnet handle has its own");
    DM_REQUIRE(walk == DM_COND_WALK_INFER || walk == DM_COND_WALK_TRAIN, "walk: DM_COND_WALK_INFER or DM_COND_WALK_TRAIN");
    DM_REQUIRE(time_kind >= DM_COND_TIME_INT && time_kind <= DM_COND_TIME_FLOAT_SHARED, "unknown time kind");
    if (cond_args_ok(u, ctx, text_mask, B)) return 1;
    const bool is_float = time_kind == DM_COND_TIME_FLOAT || time_kind == DM_COND_TIME_FLOAT_SHARED;
    const bool shared = time_kind == DM_COND_TIME_INT_SHARED || time_kind == DM_COND_TIME_FLOAT_SHARED;
    const int lsd = u->cfg.learned_sinusoidal_dim;
    DM_REQUIRE(!is_float || lsd > 0, "a real-valued time needs a learned / random sinusoidal U-Net");
    const bool train = walk == DM_COND_WALK_TRAIN;
    DM_REQUIRE(!train || !shared, "the training forward has one time per image");
    DM_REQUIRE(!train || is_float == (lsd > 0), "the training forward embeds an integer time with the fixed sinusoid and a "
                                                "real-valued time with the learned / random one");
    DM_REQUIRE(train || !(out->h1pre || out->te0pre || out->tact),
               "h1pre, te0pre and tact exist in the training forward only: the inference walk fuses the activations");
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t* ti = is_float ? nullptr : static_cast<const int64_t*>(time);
    const float* tf = is_float ? static_cast<const float*>(time) : nullptr;
    const int td = u->time_dim, ctx_tokens = ctx ? 1 : 0;
    const bool text_concat = u->cfg.text_mode == DM_TEXT_CONCAT && ctx != nullptr;
    SamplerState* st_dev = nullptr;  // the shared time is entry `step` = 0 of a sampler's table
    if (shared) {
        const SamplerState st{};
        DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&st_dev), sizeof(SamplerState)));
        if (hipMemcpy(st_dev, &st, sizeof(st), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(st_dev);
            set_error("hipMemcpy of the sampler state failed");
            return 1;
        }
    }
    const int rc = guarded([&]() -> int {
        return run_op(s, [&](Arena& A) -> int {
            if (train) {
                Tape tp;
                if (cond_train_forward(u, A, ti, tf, ctx, ctx_tokens, text_mask, B, s, tp)) return 1;
                if (A.dry) return 0;
                const size_t n = (size_t)B * td;
                return copy_out(out->e0, tp.e0, (size_t)B * tp.e0_dim, s) || copy_out(out->h1pre, tp.h1pre, n, s) ||
                       copy_out(out->h1, tp.h1, n, s) || copy_out(out->temb, tp.temb, n, s) ||
                       copy_out(out->te0pre, tp.te0pre, n, s) || copy_out(out->te0, tp.te0, n, s) ||
                       copy_out(out->cat, tp.cat, 2 * n, s) || copy_out(out->tfinal, tp.tfinal, n, s) ||
                       copy_out(out->tact, tp.tact, n, s) || copy_out(out->ss, tp.ss, (size_t)B * u->ss_total, s);
            }
            CondHead h;
            if (cond_forward(u, A, shared ? nullptr : ti, shared ? ti : nullptr, st_dev, ctx, ctx_tokens, B, s, text_mask, tf,
                             shared ? 1 : 0, h))
                return 1;
            if (A.dry) return 0;
            const size_t n = (size_t)B * td, nt = (size_t)h.Rt * td;
            return copy_out(out->e0, h.e0, (size_t)h.Rt * h.fdim, s) || copy_out(out->h1, h.e1, nt, s) ||
                   copy_out(out->temb, h.temb, nt, s) || copy_out(out->te0, h.tf0, n, s) || copy_out(out->cat, h.cat, 2 * n, s) ||
                   copy_out(out->tfinal, h.tfinal, text_concat ? n : nt, s) ||
                   copy_out(out->ss, h.ss, (size_t)h.Bt * u->ss_total, s);
        });
    });
    if (st_dev) (void)hipFree(st_dev);
    return rc;
}

/* The backward of the conditioning head on its own, on an armed handle: cond_backward, the function the backward walk ends
 * with, on the caller's tape and dss, in a NaN-filled workspace. */
int dm_unet_cond_backward(dm_unet* u, const dm_cond_bufs* tape, const float* ctx, const int32_t* text_mask, const float* dss,
                          float* dt, int B, int accumulate, void* stream) {
    DM_REQUIRE(u && tape && dss, "null argument");
    if (cond_args_ok(u, ctx, text_mask, B)) return 1;
    DM_REQUIRE(u->train, "dm_unet_train_enable / dm_unet_train_enable_ft has not been called");
    const bool text_concat = u->cfg.text_mode == DM_TEXT_CONCAT && ctx != nullptr;
    DM_REQUIRE(tape->e0 && tape->h1pre && tape->h1 && tape->tfinal && tape->tact, "the tape of a training forward: e0, h1pre, h1, "
                                                                                "tfinal and tact");
    DM_REQUIRE(!text_concat || (tape->te0pre && tape->te0 && tape->cat), "text concat: the tape holds te0pre, te0 and cat too");
    DM_REQUIRE(!dt || u->train->ft, "dt needs a handle armed by dm_unet_train_enable_ft");
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        if (u->order_after_previous(s)) return 1;
        Tape tp;
        tp.e0 = tape->e0; tp.h1pre = tape->h1pre; tp.h1 = tape->h1; tp.temb = tape->temb; tp.ss = tape->ss;
        tp.tact = tape->tact; tp.te0pre = tape->te0pre; tp.te0 = tape->te0; tp.cat = tape->cat; tp.tfinal = tape->tfinal;
        tp.e0_dim = u->train->ft ? u->cfg.learned_sinusoidal_dim + 1 : u->cfg.dim;
        tp.ctx = ctx;
        tp.ctx_tokens = ctx ? 1 : 0;
        tp.mask = ctx ? text_mask : nullptr;
        const InputGrad ig{nullptr, dt};
        if (run_op(s, [&](Arena& A) -> int {
                TCtx t{u, &A, s, B, nullptr, 0};
                t.acc = accumulate;
                return cond_backward(t, tp, dss, dt ? &ig : nullptr);
            }))
            return 1;
        return u->mark_done(s);
    });
}

/* The deferred reductions of a backward pass on their own: every layer is launched as the walk launches it -- with
 * deferred != 0 into the two job tables (TCtx::rdefer / TCtx::cdefer), which flush_deferred_reductions then runs, the
 * function the walk calls; with deferred == 0 through the immediate kernels.  Outputs are written by the kernels
 * themselves into the caller's buffers; the workspaces live in a NaN-filled arena. */
int dm_op_deferred_reduce(const dm_reduce_layer* layers, int n_layers, int B, int deferred, int accumulate, void* stream) {
    DM_REQUIRE(layers && n_layers > 0 && B > 0, "bad argument");
    for (int i = 0; i < n_layers; ++i) {
        const dm_reduce_layer& L = layers[i];
        if (L.kind == DM_REDUCE_NORM_BWD) {
            DM_REQUIRE(L.dy && L.u && L.g && L.du && L.dg, "norm backward: dy, u, g, du and dg");
            DM_REQUIRE(L.C % 4 == 0 && L.C >= 4 && L.C <= 1024, "norm backward: C must be a multiple of 4, at most 1024");
            DM_REQUIRE(L.rows > 0, "norm backward: rows is the pixels per image");
            DM_REQUIRE((L.ss == nullptr) == (L.dss == nullptr), "norm backward: ss and dss come together");
            DM_REQUIRE(!L.ss || (L.ss_stride >= 2 * L.C && L.ss_stride % 4 == 0 && L.dss_stride >= 2 * L.C),
                       "norm backward: a (scale | shift) row is 2 C floats, rows a multiple of 4 apart");
        } else {
            DM_REQUIRE(L.kind == DM_REDUCE_COLSUM, "unknown layer kind");
            DM_REQUIRE(L.x && L.out && L.rows > 0 && L.C > 0 && L.row_stride > 0 && L.col_stride > 0, "column sum: x, out, sizes");
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return guarded([&]() -> int {
        OpTrain op(4, 32);
        std::vector<RowgradJob> rjobs;
        std::vector<ColsumJob> cjobs;
        return run_op(s, [&](Arena& A) -> int {
            TCtx t{&op.u, &A, s, B, nullptr, 0};
            t.acc = accumulate;
            rjobs.clear();
            cjobs.clear();
            if (deferred) {
                t.rjobs = &rjobs;
                t.cjobs = &cjobs;
            }
            for (int i = 0; i < n_layers; ++i) {
                const dm_reduce_layer& L = layers[i];
                if (L.kind == DM_REDUCE_NORM_BWD) {
                    float* ws = A.alloc(norm_act_bwd_ws_floats(B, (int)L.rows, L.C));
                    const int flags = EPI_NORM | (L.silu ? EPI_SILU : 0) | (L.ss ? EPI_SCALE_SHIFT : 0);
                    if (!A.dry && launch_norm_act_bwd(L.dy, L.u, L.g, L.ss, L.ss_stride, (int)L.rows, L.du, ws, L.dg, L.dbias, L.dss,
                                                      L.dss_stride, B, L.C, flags, t.acc, s, t.rdefer()))
                        return 1;
                } else {
                    float* ws = A.alloc(colsum_ws_floats(L.rows, L.C));
                    if (!A.dry && launch_colsum(L.x, L.rows, L.C, L.row_stride, L.col_stride, ws, L.out, t.acc, s, t.cdefer()))
                        return 1;
                }
            }
            if (A.dry || !deferred) return 0;
            return flush_deferred_reductions(*op.u.train, rjobs, cjobs, s);
        });
    });
}

}  // extern "C"
