// The scaffold of the stand-alone single-pass entry points (dm_op_*) that read a host table: upload, run, wait, free.
// Included by dm_api.hip in front of dm_ops.inc; the step, loss and noise-in operators of every sampler and objective
// run on it.

namespace dm {

// `n` floats of the scratch behind the table rows, from float `off` of it, to a host pointer once the stream has drained
struct OpReadback {
    float* host;
    size_t off, n;
};

// One stand-alone pass: upload `rows` table rows of `width` floats with `scratch` floats of device memory behind them
// (per-image partial sums, a scalar result), run fn(table, stream), wait for the stream, copy `back` out, free.
static int table_op(const float* c_host, int rows, void* stream, const std::function<int(float*, hipStream_t)>& fn,
                    int width = DM_EDM_COEFS, size_t scratch = 0, std::initializer_list<OpReadback> back = {}) {
    DM_REQUIRE(c_host && rows > 0, "null step table");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n_tab = (size_t)rows * width;
    float* cd = nullptr;
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&cd), (n_tab + scratch) * sizeof(float)));
    hipError_t e = hipMemcpy(cd, c_host, n_tab * sizeof(float), hipMemcpyHostToDevice);
    int rc = 0;
    if (e == hipSuccess) {
        rc = fn(cd, s);
        e = hipStreamSynchronize(s);
    }
    for (const OpReadback& b : back)
        if (!rc && e == hipSuccess && b.host)
            e = hipMemcpy(b.host, cd + n_tab + b.off, b.n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(cd);
    if (!rc && e != hipSuccess) {
        set_error(std::string("kernel execution failed: ") + hipGetErrorString(e));
        rc = 1;
    }
    return rc;
}
// rows == 1: one row for every image; rows == B: row b for image b
static int edm_rows(const float* tab, int rows, int B, int64_t per, StepRows* out) {
    DM_REQUIRE(B > 0 && per > 0, "empty tensor");
    DM_REQUIRE(rows == 1 || rows == B, "the step table has one row, or one row per image");
    *out = StepRows{tab, nullptr, rows == B && B > 1 ? STEP_ROW_IMAGE : STEP_ROW_FIRST, per};
    return 0;
}

// One SamplerState for a stand-alone pass next to its table rows (table_op): upload, run fn, wait, free.
static int state_op(const SamplerState& st_host, const float* c_host, int rows, void* stream,
                    const std::function<int(const SamplerState*, const float*, hipStream_t)>& fn) {
    SamplerState* st_dev = nullptr;
    DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&st_dev), sizeof(SamplerState)));
    hipError_t e = hipMemcpy(st_dev, &st_host, sizeof(st_host), hipMemcpyHostToDevice);
    int rc = 1;
    if (e == hipSuccess) rc = table_op(c_host, rows, stream, [&](const float* cd, hipStream_t s) { return fn(st_dev, cd, s); });
    else set_error(std::string("hipMemcpy: ") + hipGetErrorString(e));
    (void)hipFree(st_dev);
    return rc;
}
// The kernels draw `step + 1`: a state with step = draw - 1 selects the draw (with injected noise: none).
static SamplerState draw_state(bool injected, uint64_t seed, uint64_t draw, uint64_t element_offset) {
    SamplerState st{};
    st.step = injected ? 0 : (int)(draw - 1);
    st.n_steps = st.step + 1;
    st.seed = seed;
    st.off4 = element_offset / 4;
    return st;
}
// what a step pass of the integer-time classes asks of the arguments draw_state reads
static int draw_args_ok(const float* z, uint64_t draw, uint64_t element_offset) {
    DM_REQUIRE(element_offset % 4 == 0, "Philox element offset must be a multiple of 4 (one counter serves 4 elements)");
    DM_REQUIRE(z || draw >= 1, "Philox draw 0 is the initial noise: a step's draw is its index + 1");
    DM_REQUIRE(draw < (uint64_t(1) << 30), "draw index out of range");
    return 0;
}

}  // namespace dm
