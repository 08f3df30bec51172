// The convolution kernel families.  Textually included by dm_api.hip (namespace dm).
//
// ONE row per family says everything the host code outside plan_conv has to know about it: which packed layout(s) its
// kernel reads and when a layer gets one (make_conv), the device mirror of each packer (run_pack_op), how the grouped
// re-pack covers the layout (pack_jobs_of), the width of its K chunks, its launcher (launch_planned) and whether it can
// leave K-split partial sums for a landing pass.  A new family is its kernel file, a row here and a clause in plan_conv.
// The kernel files' packers differ a little in their signatures; the adapters below bring them to one.

enum ConvKind { CONV_DIRECT, CONV_WINO, CONV_WINO4, CONV_UPWINO, CONV_PW, CONV_INIT7, CONV_THIN, CONV_KINDS };

// nearest x2 + 3x3 runs as four 2x2 parity convolutions on the source grid (ConvParams::fold): make_conv packs those
// (PK_FOLD) in place of the direct layout
static bool conv_folds(int KH, int KW, int stride, int pad, bool up) { return up && KH == 3 && KW == 3 && stride == 1 && pad == 1; }

// one packed layout: the buffer of a layer that is `eligible` holds `floats` floats, written by `pack` on the host and by
// `device_pack` from the master parameters; all read the OIHW (Cout, C0 + C1, KH, KW) weight
struct ConvRecipe {
    int pk;  // PackKind of the recorded PackOp
    bool (*eligible)(int Cout, int C0, int C1, int KH, int KW, int stride, int pad, bool up);
    size_t (*floats)(int Cout, int C0, int C1, int KH, int KW);
    void (*pack)(const float* oihw, float* packed, int Cout, int C0, int C1, int KH, int KW);
    int (*device_pack)(const float* oihw, float* packed, int Cout, int C0, int C1, int KH, int KW, hipStream_t s);
    bool s2d;  // a (Cout, C0, 2, 2) Downsample weight read as a 1x1 convolution over 4 C0 channels
};

struct ConvFamily {
    const char* name;
    ConvRecipe recipe[2];  // in upload order; a family with one layout leaves the second empty (eligible == nullptr)
    int pj;                // PackJobKind of the grouped re-pack, -1: lazy path only
    int cin_mult, cout_mult;  // ... which walks whole K chunks / cout tiles: the multiples it requires
    int rot_k;             // ... and reads the rotated rows of a (., ., rot_k, rot_k) input-gradient source in place (0: never)
    int k_chunk;           // input channels per K chunk of the packed layout (0: conv_ck_for, or none)
    int (*launch)(const ConvParams& p, hipStream_t s);
    bool partials;         // the kernel can write K-split partial sums (ConvParams::partial)
};

// adapters: the kernel files' host packers take (Cout, C0, C1), their device mirrors (Cout, Cin)
template <size_t (*F)(int, int, int)>
static size_t floats_of(int Cout, int C0, int C1, int, int) { return F(Cout, C0, C1); }
template <void (*F)(const float*, float*, int, int, int)>
static void pack_of(const float* w, float* d, int Cout, int C0, int C1, int, int) { F(w, d, Cout, C0, C1); }
template <int (*F)(const float*, float*, int, int, hipStream_t)>
static int device_pack_of(const float* w, float* d, int Cout, int C0, int C1, int, int, hipStream_t s) { return F(w, d, Cout, C0 + C1, s); }

static int launch_thin(const ConvParams& p, hipStream_t s) {
    return launch_pointwise_small(p.in0, p.w, p.bias, p.out, (int64_t)p.B * p.Ho * p.Wo, p.C0, p.Cout, p.Ho * p.Wo, s);
}
static int device_copy_thin(const float* w, float* dst, int Cout, int C0, int, int, int, hipStream_t s) {
    DM_CHECK_HIP(hipMemcpyAsync(dst, w, (size_t)Cout * C0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

static const ConvFamily conv_families[CONV_KINDS] = {
    {"direct",
     {{PK_DIRECT, [](int, int, int, int KH, int KW, int stride, int pad, bool up) { return !conv_folds(KH, KW, stride, pad, up); },
       conv_packed_floats, conv_pack_weights, launch_pack_direct, false}},
     -1, 1, 1, 0, 0, conv_launch, true},
    {"F(2x2)",
     {{PK_WINO, wino_eligible, floats_of<wino_packed_floats>, pack_of<wino_pack_weights>, device_pack_of<launch_pack_wino>, false}},
     PJ_WINO, 8, 1, 3, 8, wino_launch, true},
    {"F(4x4)",
     {{PK_WINO4, wino4_eligible, floats_of<wino4_packed_floats>, pack_of<wino4_pack_weights>, device_pack_of<launch_pack_wino4>, false}},
     PJ_WINO4, 8, 64, 3, 8, wino4_launch, true},
    {"upsample-Winograd",
     {{PK_UPWINO, upwino_eligible, floats_of<upwino_packed_floats>, pack_of<upwino_pack_weights>, device_pack_of<launch_pack_upwino>, false}},
     PJ_UPWINO, 8, 64, 3, 8, upwino_launch, true},
    {"1x1 GEMM",
     {{PK_PW, pw_eligible, floats_of<pw_packed_floats>, pack_of<pw_pack_weights>,
       [](const float* w, float* d, int Cout, int C0, int C1, int, int, hipStream_t s) { return launch_pack_pw(w, d, Cout, C0 + C1, 0, s); },
       false},
      {PK_PW_S2D, pw_s2d_eligible, [](int Cout, int C0, int, int, int) { return (size_t)4 * C0 * Cout; },
       [](const float* w, float* d, int Cout, int C0, int, int, int) { pw_pack_weights_s2d(w, d, Cout, C0); },
       [](const float* w, float* d, int Cout, int C0, int, int, int, hipStream_t s) { return launch_pack_pw(w, d, Cout, 4 * C0, C0, s); },
       true}},
     PJ_PW, 16, 16, 1, 16, pw_launch, true},
    {"7x7 first conv",
     {{PK_INIT7, init7_eligible, [](int, int C0, int, int, int) { return init7_packed_floats(C0); },
       [](const float* w, float* d, int, int C0, int, int, int) { init7_pack_weights(w, d, C0); },
       [](const float* w, float* d, int, int C0, int, int, int, hipStream_t s) { return launch_pack_init7(w, d, C0, s); }, false}},
     -1, 1, 1, 0, 0, init7_launch, false},
    // a 1x1 convolution to a handful of output channels (final_conv): the (Cout, C0) weight as stored, one pixel per thread
    {"thin pointwise",
     {{PK_RAW_W,
       [](int Cout, int C0, int C1, int KH, int KW, int stride, int pad, bool up) {
           return KH == 1 && KW == 1 && stride == 1 && pad == 0 && !up && Cout <= 8 && C1 == 0 && C0 % 4 == 0;
       },
       [](int Cout, int C0, int, int, int) { return (size_t)Cout * C0; },
       [](const float* w, float* d, int Cout, int C0, int, int, int) { std::memcpy(d, w, (size_t)Cout * C0 * sizeof(float)); },
       device_copy_thin, false}},
     PJ_COPY, 1, 1, 0, 0, launch_thin, false},
};

// the recipe (and its family) behind a recorded PackOp; nullptr for the raw copies and the folded upsample layout
static const ConvRecipe* conv_recipe_of(int pk, const ConvFamily** family = nullptr) {
    for (const ConvFamily& F : conv_families)
        for (const ConvRecipe& R : F.recipe)
            if (R.eligible && R.pk == pk) {
                if (family) *family = &F;
                return &R;
            }
    return nullptr;
}
