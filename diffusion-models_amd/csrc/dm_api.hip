// C ABI of libdm_hip.so (include/dm_hip.h): U-Net handle, forward, samplers, single operators.
// Host orchestration only -- every FLOP runs in the kernels of conv_mfma.hip / attention.hip /
// elementwise.hip.  No allocation, copy or synchronisation happens inside the per-step launch
// sequence, so one denoise step can be captured into a hipGraph and replayed.
#include "../../include/dm_hip.h"
#include "dm_common.h"
#include "edm.h"
#include "ct.h"
#include "repaint.h"
#include "learned.h"
#include "weighted.h"
#include "cguide.h"
#include "bpd.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

namespace dm {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

// ---------------------------------------------------------------------------------------
// per-kernel event timing (bench.py roofline leg)
// ---------------------------------------------------------------------------------------
namespace prof {
struct Rec {
    std::string kernel;
    double flops, bytes;
    hipEvent_t e0, e1;
};
static bool g_on = false;
static bool g_detail = false;
// Interval of (event, EMPTY kernel, event): dispatch latency plus the two event packets, ~9 us on MI355X.  It is
// measured when profiling is switched on and subtracted from every bracketed launch, so that a row's time is the
// kernel's execution time -- what rocprofv3 --kernel-trace reports -- and not execution + dispatch.
static double g_overhead_ms = 0.0;
static std::vector<Rec> g_recs;
static std::vector<hipEvent_t> g_pool;

bool enabled() { return g_on; }
bool detail() { return g_detail; }

static int get_event(hipEvent_t* e) {
    if (!g_pool.empty()) {
        *e = g_pool.back();
        g_pool.pop_back();
        return 0;
    }
    DM_CHECK_HIP(hipEventCreate(e));
    return 0;
}

int begin(const char* kernel, double flops, double bytes, hipStream_t s) {
    Rec r{kernel, flops, bytes, nullptr, nullptr};
    if (get_event(&r.e0) || get_event(&r.e1)) return 1;
    DM_CHECK_HIP(hipEventRecord(r.e0, s));
    g_recs.push_back(r);
    return 0;
}

int end(hipStream_t s) {
    DM_REQUIRE(!g_recs.empty(), "prof::end without begin");
    DM_CHECK_HIP(hipEventRecord(g_recs.back().e1, s));
    return 0;
}
}  // namespace prof

// ---------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------
struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool set = false;
    bool dirty = false;  // changed by dm_unet_update_param since the device copy was packed
    size_t numel() const {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        return n;
    }
};

// Recipe of one packed weight buffer (recorded while the host packs it): which parameter it comes from and which packer
// made it, so that the training loop can re-pack it on the DEVICE from the flat master parameters (pack_kernels.hip).
enum PackSrcKind {
    PS_STORED,  // the parameter as stored
    PS_ROT,     // rotated / transposed rows [c_lo, c_lo + c_n) of a (sCout, sCin, sK, sK) parameter (input-gradient convolution)
    PS_S2D_T,   // Downsample input-gradient transpose of a (sCout, 4 sCin) parameter
    PS_UP1D,    // the sequence model's Upsample packing of a (sCout, sCin, 3) parameter: the layer holds 2 sCout rows
                // (make_upsample1d).  No device re-pack mirrors it yet: a sequence handle does not train.
};
struct PackSrc {
    PackSrcKind kind = PS_STORED;
    std::string wname, bname;
    int sCout = 0, sCin = 0, sK = 0, c_lo = 0, c_n = 0;
};
enum PackKind { PK_RAW_W, PK_RAW_B, PK_RAW_NAME, PK_DIRECT, PK_FOLD, PK_WINO, PK_WINO4, PK_UPWINO, PK_PW, PK_PW_S2D, PK_INIT7 };
struct PackOp {
    int kind;
    float* dst;
    size_t n;          // floats of dst written by this op
    int Cout, C0, C1, KH, KW;
    PackSrc src;
    std::string name;  // PK_RAW_NAME: the parameter copied to dst
};

// Owner of every repacked weight buffer of a handle.  The first build allocates one buffer per upload; a REFRESH
// (dm_unet_refresh: new values for parameters of the same shapes) replays the same upload sequence into the same
// buffers, so every device pointer -- and with them a captured step graph -- stays valid.
struct DeviceOwner {
    std::vector<void*> ptrs;
    std::vector<size_t> sizes;
    bool refreshing = false;
    size_t cursor = 0;
    std::vector<PackOp>* rec = nullptr;  // when set, make_conv / up1 append the recipe of every buffer they upload
    void record(int kind, float* dst, size_t n, int Cout, int C0, int C1, int KH, int KW, const PackSrc& src) {
        if (rec && !refreshing) rec->push_back(PackOp{kind, dst, n, Cout, C0, C1, KH, KW, src, std::string()});
    }
    void record_raw(const std::string& name, float* dst, size_t n) {
        if (rec && !refreshing) rec->push_back(PackOp{PK_RAW_NAME, dst, n, 0, 0, 0, 0, 0, PackSrc(), name});
    }
    ~DeviceOwner() { reset(); }
    DeviceOwner() = default;
    DeviceOwner(const DeviceOwner&) = delete;  // owns device memory
    DeviceOwner& operator=(const DeviceOwner&) = delete;
    void reset() {  // free every buffer (the input-gradient layers are rebuilt from scratch on a refresh)
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
        sizes.clear();
        cursor = 0;
    }
    int upload(const float* host, size_t n, float** out) {
        if (refreshing) {
            DM_REQUIRE(cursor < ptrs.size() && sizes[cursor] == n, "refresh: the upload sequence differs from the first build");
            void* p = ptrs[cursor++];
            if (n) DM_CHECK_HIP(hipMemcpy(p, host, n * sizeof(float), hipMemcpyHostToDevice));
            *out = static_cast<float*>(p);
            return 0;
        }
        void* p = nullptr;
        DM_CHECK_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(float)));
        ptrs.push_back(p);
        sizes.push_back(n);
        if (n) DM_CHECK_HIP(hipMemcpy(p, host, n * sizeof(float), hipMemcpyHostToDevice));
        *out = static_cast<float*>(p);
        return 0;
    }
};

// Workspace allocator over one device buffer.  Activations are released as soon as their last consumer has been
// ENQUEUED (the launch stream is in order, and so is a captured step graph), so a denoise step works in a few hundred
// megabytes that it keeps re-using instead of a fresh line of HBM per tensor: at the benchmark batch the blocks a
// layer reads were written a few launches earlier and are still in the 256 MB Infinity Cache.
// `dry` replays the same allocation sequence on fake addresses to measure the capacity (`peak`) a run needs; the
// sequence, hence every pointer, is a function of the shapes only -- which is what makes the step capturable.
struct Arena {
    char* base = nullptr;
    size_t cap = 0;
    bool dry = false;
    size_t off = 0;  // capacity required so far (high-water mark)
    struct Blk {
        size_t off, size;
        bool free;
    };
    std::vector<Blk> blks;  // sorted by offset, adjacent, covering [0, end of the last block)
    int n_free = 0;         // free blocks in `blks`: the tape forward of the training step releases almost nothing, and a
                            // best-fit scan over its ~1000 live blocks per allocation was a millisecond of host time per call
    char* origin() const { return dry ? reinterpret_cast<char*>(uintptr_t(1) << 44) : base; }
    float* alloc(size_t nfloats) {
        const size_t bytes = std::max<size_t>((nfloats * sizeof(float) + 255) & ~size_t(255), 256);
        int best = -1;
        if (n_free > 0)
            for (size_t i = 0; i < blks.size(); ++i)  // best fit
                if (blks[i].free && blks[i].size >= bytes && (best < 0 || blks[i].size < blks[best].size)) best = (int)i;
        size_t at;
        if (best >= 0) {
            Blk& b = blks[best];
            at = b.off;
            if (b.size > bytes) {
                const Blk rest{b.off + bytes, b.size - bytes, true};
                b.size = bytes;
                b.free = false;
                blks.insert(blks.begin() + best + 1, rest);  // one free block became a used one and a free rest
            } else {
                b.free = false;
                n_free -= 1;
            }
        } else if (!blks.empty() && blks.back().free) {  // grow the free tail
            at = blks.back().off;
            blks.back().size = bytes;
            blks.back().free = false;
            n_free -= 1;
        } else {
            at = blks.empty() ? 0 : blks.back().off + blks.back().size;
            blks.push_back(Blk{at, bytes, false});
        }
        off = std::max(off, blks.back().off + blks.back().size);
        return reinterpret_cast<float*>(origin() + at);
    }
    void release(const void* p) {
        if (!p) return;
        const size_t at = (size_t)(static_cast<const char*>(p) - origin());
        // blocks are sorted by offset: binary search for the one that starts at `at`
        size_t lo = 0, hi = blks.size();
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (blks[mid].off < at) lo = mid + 1;
            else hi = mid;
        }
        for (size_t i = lo; i < blks.size() && blks[i].off == at; ++i) {
            if (blks[i].free) continue;
            blks[i].free = true;
            n_free += 1;
            if (i + 1 < blks.size() && blks[i + 1].free) {
                blks[i].size += blks[i + 1].size;
                blks.erase(blks.begin() + i + 1);
                n_free -= 1;
            }
            if (i > 0 && blks[i - 1].free) {
                blks[i - 1].size += blks[i].size;
                blks.erase(blks.begin() + i);
                n_free -= 1;
            }
            return;
        }
    }
};

#include "conv_family.inc"

struct ConvLayer {
    int C0 = 0, C1 = 0, Cout = 0, KH = 1, KW = 1, stride = 1, pad = 0;
    int pad_w = -1;     // zero columns left / right when they differ from `pad` rows (1x7 / 7x1 convs of InceptionV3); -1: pad
    int pad_hi = 0;     // extra zero rows / columns at the bottom / right only (VAE Encoder Downsample, model.py:89-93)
    bool up = false;    // nearest x2 in front of the conv (Upsample, DD/denoising_diffusion.py:48-52)
    bool fold = false;  // ... executed as four 2x2 parity convs on the source grid (ConvParams::fold)
    int fold_w_stride = 0;
    float* packed[CONV_KINDS] = {};  // the weights in the layout of every family the layer is eligible for (conv_family.inc)
    float* bias = nullptr;
    PackSrc src;  // the parameters the layer is packed from: weight and bias name (empty: anonymous weights of a single
                  // operator); an input-gradient layer also says which rotated / transposed part of the weight it holds
};

struct ResBlock {
    std::string prefix;  // parameter-name prefix of the block (as for AttnLayer and CrossLayer: set where the layer is built)
    ConvLayer c1, c2, res;
    bool has_res = false;
    float *g1 = nullptr, *g2 = nullptr;
    int ss_off = 0, dout = 0;
};

struct AttnLayer {
    std::string prefix;
    bool full = false;
    int dim = 0, heads = 0;  // heads: attn_heads of the layer's stage (cast_tuple(attn_heads, num_stages), :294)
    int dh = 0;              // head width when it is not the handle's (the sequence model's stages: 32 whatever mid_attn has)
    float *norm_g = nullptr, *mem_kv = nullptr, *out_g = nullptr;  // mem_kv == nullptr: no memory key / values (Unet1D)
    ConvLayer qkv, out;
    bool has_fused = false;  // LinearAttention as two fused kernels (linattn_fused.hip)
    bool has16 = false;      // full attention over 16 tokens as one kernel (attn16_fused.hip)
    Attn16 a16{};
    LinAttnFused fused{};
};

struct CrossLayer {
    std::string prefix;
    ConvLayer q, out;
    float *wk = nullptr, *wv = nullptr, *g = nullptr;
    float* wo_raw = nullptr;  // to_out.0.weight as stored (dim, inner): the one-context-token path runs it per image
};

struct Stage {
    ResBlock b1, b2;
    AttnLayer attn;
    ConvLayer resample;
};

struct TrainState;  // dm_train.inc
struct UnetGraph;   // unet_graph.inc
struct KUnet;       // dm_kunet.inc

}  // namespace dm

using namespace dm;

static_assert(DDIM_NO_CLAMP == DM_DDIM_NO_CLAMP && DDIM_RAW_NOISE == DM_DDIM_RAW_NOISE, "dm_common.h and dm_hip.h disagree");

struct dm_unet {
    dm_unet_cfg cfg{};
    int device = 0;
    int init_dim = 0, out_dim = 0, time_dim = 0, heads = 0, dh = 0;
    std::vector<int> dims;
    std::map<std::string, HostTensor> params;  // expected entries, filled by set_param
    std::vector<std::string> order;
    bool finalized = false;
    bool poisoned = false;  // a refresh failed half-way: device weights are a mix of old and new values
    dm::TrainState* train = nullptr;  // dm_unet_train_enable: gradient buffers, dgrad weights, training workspace
    dm::KUnet* kunet = nullptr;       // dm_kunet_create: the handle is a KarrasUnet (dm_kunet.inc); the image / sequence
                                      // layers below stay empty, `params`, `own`, the workspace and the graph slot serve both
    std::vector<dm::PackOp> pack_ops;  // recipe of every buffer the convolutions / norms read (device-side re-packing)
    bool infer_stale = false;          // device-side optimiser steps since the fused inference-only packs were built
    DeviceOwner own;
    // layers
    ConvLayer init_conv, final_conv;
    std::vector<Stage> downs, ups;
    ResBlock mid1, mid2, final_res;
    AttnLayer mid_attn;
    CrossLayer cross_down, cross_mid, cross_up;
    std::vector<dm::UnetGraph> graphs;  // the order the layers run in, per form of the network (unet_graph.inc)
    float *freqs = nullptr, *tw1 = nullptr, *tb1 = nullptr, *tw2 = nullptr, *tb2 = nullptr;
    float *ss_w = nullptr, *ss_b = nullptr;
    int ss_total = 0;
    float *tp_w0 = nullptr, *tp_b0 = nullptr, *tp_w2 = nullptr, *tp_b2 = nullptr, *tc_w = nullptr, *tc_b = nullptr;
    // workspace
    char* ws = nullptr;
    size_t ws_cap = 0;
    // sampler state (device)
    SamplerState* state_dev = nullptr;
    int64_t* times_dev = nullptr;
    float* coefs_dev = nullptr;
    int sampler_cap = 0;
    // weight groups: parameter-name prefix -> [first upload, count) in `own` (dm_unet_refresh skips clean groups)
    std::map<std::string, std::pair<size_t, size_t>> groups;
    std::vector<std::pair<std::string, ResBlock*>> resnets;  // in ss_off order
    // the instantiated graph of one denoise step, reused while the key (shape, kind, every captured pointer) holds.  The
    // slot serves every sampling loop of the handle (dm_sampler.inc: run_steps); the kind says whose graph it holds.
    enum GraphKind { GK_NONE = -1, GK_DDPM, GK_DDIM, GK_EDM_HEUN, GK_EDM_DPMPP, GK_CT, GK_REPAINT, GK_LV, GK_CG, GK_WO, GK_DPMPP,
                     GK_CT_DPMPP, GK_BPD };
    struct GraphKey {
        int kind = GK_NONE, B = 0, H = 0, W = 0, ctx_tokens = 0, cond_channels = 0, objective = 0, self_cond = 0, guided = 0;
        int ddim_flags = 0;     // DM_DDIM_*: kernel arguments of the captured DDIM update
        int dyn = 0;            // dynamic thresholding: one more kernel in the captured step (the percentile is device data)
        int edm_clamp = 0;      // ElucidatedDiffusion: the clamp flag, a kernel argument of the captured Heun step
        int ct_clip = 0;        // continuous time: the clip flag of the captured ct_step
        int mask_channels = 0;  // RePaint: 1 or C
        int bpd_flags = 0;      // bits per dim: learned variance (1), clip_denoised (2), kernel arguments of the captured term pass
        const void *noise = nullptr, *all_steps = nullptr, *ws = nullptr, *times = nullptr, *coefs = nullptr;
        const void* tab = nullptr;  // the 16-float-row table (edm_tab_dev) of the EDM, continuous-time and RePaint steps
        const void *cg_mean = nullptr, *cg_grad = nullptr;  // classifier guidance: the caller's tensors the two halves touch
        bool operator==(const GraphKey& o) const {
            return kind == o.kind && B == o.B && H == o.H && W == o.W && ctx_tokens == o.ctx_tokens &&
                   cond_channels == o.cond_channels && objective == o.objective && self_cond == o.self_cond &&
                   guided == o.guided && ddim_flags == o.ddim_flags && dyn == o.dyn && edm_clamp == o.edm_clamp && ct_clip == o.ct_clip && mask_channels == o.mask_channels && bpd_flags == o.bpd_flags &&
                   noise == o.noise && all_steps == o.all_steps && ws == o.ws && times == o.times && coefs == o.coefs &&
                   tab == o.tab && cg_mean == o.cg_mean && cg_grad == o.cg_grad;
        }
    } gkey;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    // Workspace, sampler state and the cached graph are shared by every call on the handle: a call waits for the previous
    // call's last kernel (recorded here) before it touches them, so two calls on DIFFERENT streams are still ordered.
    hipEvent_t done_ev = nullptr;
    bool done_recorded = false;
    int order_after_previous(hipStream_t s) {
        if (!done_ev) DM_CHECK_HIP(hipEventCreateWithFlags(&done_ev, hipEventDisableTiming));
        if (done_recorded) DM_CHECK_HIP(hipStreamWaitEvent(s, done_ev, 0));
        return 0;
    }
    int mark_done(hipStream_t s) {
        DM_CHECK_HIP(hipEventRecord(done_ev, s));
        done_recorded = true;
        return 0;
    }
    // ElucidatedDiffusion (dm_edm.inc): device step table (continuous time and RePaint keep theirs in it too) and the graph
    // of the last Heun step (sigma_next == 0: one forward); the graph of a full step is `graph` / `gexec` above
    float* edm_tab_dev = nullptr;
    int edm_cap = 0;
    hipGraph_t edm_last_graph = nullptr;
    hipGraphExec_t edm_last_gexec = nullptr;
    hipStream_t cap_stream = nullptr;  // capture / replay stream when the caller passes the legacy default stream
    int graph_captures = 0;            // diagnostics (dm_unet_graph_captures)
    void drop_graph() {
        if (gexec) (void)hipGraphExecDestroy(gexec);
        if (graph) (void)hipGraphDestroy(graph);
        if (edm_last_gexec) (void)hipGraphExecDestroy(edm_last_gexec);
        if (edm_last_graph) (void)hipGraphDestroy(edm_last_graph);
        edm_last_gexec = nullptr;
        edm_last_graph = nullptr;
        gexec = nullptr;
        graph = nullptr;
        gkey = GraphKey{};
    }
};

namespace dm {

void free_train(dm_unet* u);  // dm_train.inc
void kunet_free(dm_unet* u);  // dm_kunet.inc
static int kunet_build_all(dm_unet* u);
static int kunet_forward_impl(dm_unet* u, Arena& A, const float* x_nchw, const SamplerState* step_dev, float* out_nchw, int B,
                              int H, int W, hipStream_t s, const float* tf, int tf_stride);
static int ensure_packed(dm_unet* u, const float* w, hipStream_t s);
static int build_train(dm_unet* u);
static int upload_master_if_resident(dm_unet* u);

static void expect(dm_unet* u, const std::string& name, std::vector<int64_t> shape) {
    HostTensor t;
    t.shape = std::move(shape);
    u->params[name] = std::move(t);
    u->order.push_back(name);
}

static void expect_resnet(dm_unet* u, const std::string& p, int din, int dout) {
    int td = u->time_dim;
    expect(u, p + ".mlp.1.weight", {2 * dout, td});
    expect(u, p + ".mlp.1.bias", {2 * dout});
    expect(u, p + ".block1.proj.weight", {dout, din, 3, 3});
    expect(u, p + ".block1.proj.bias", {dout});
    expect(u, p + ".block1.norm.g", {1, dout, 1, 1});
    expect(u, p + ".block2.proj.weight", {dout, dout, 3, 3});
    expect(u, p + ".block2.proj.bias", {dout});
    expect(u, p + ".block2.norm.g", {1, dout, 1, 1});
    if (din != dout) {
        expect(u, p + ".res_conv.weight", {dout, din, 1, 1});
        expect(u, p + ".res_conv.bias", {dout});
    }
}

// attn_heads of stage i (Unet(attn_heads = (..)), :294: cast_tuple over the stages; mid_attn takes the last stage's, :324)
static int stage_heads(const dm_unet_cfg& cfg, int i) { return cfg.attn_heads_stage[i] > 0 ? cfg.attn_heads_stage[i] : cfg.attn_heads; }

// the output projection of an attention layer: Attention.to_out is a convolution, LinearAttention.to_out is
// Sequential(convolution, RMSNorm)
static std::string attn_out_param(const std::string& p, bool full) { return p + (full ? ".to_out" : ".to_out.0"); }

static void expect_attn(dm_unet* u, const std::string& p, int dim, bool full, int heads) {
    int hidden = heads * u->dh;
    const std::string out = attn_out_param(p, full);
    expect(u, p + ".mem_kv", full ? std::vector<int64_t>{2, heads, 4, u->dh} : std::vector<int64_t>{2, heads, u->dh, 4});
    expect(u, p + ".norm.g", {1, dim, 1, 1});
    expect(u, p + ".to_qkv.weight", {3 * hidden, dim, 1, 1});
    expect(u, out + ".weight", {dim, hidden, 1, 1});
    expect(u, out + ".bias", {dim});
    if (!full) expect(u, p + ".to_out.1.g", {1, dim, 1, 1});
}

static void expect_cross(dm_unet* u, const std::string& p, int dim) {
    int inner = 4 * u->dh;
    int ctx = u->cfg.text_emb_dim;
    expect(u, p + ".to_q.weight", {inner, dim});
    expect(u, p + ".to_k.weight", {inner, ctx});
    expect(u, p + ".to_v.weight", {inner, ctx});
    expect(u, p + ".to_out.0.weight", {dim, inner});
    expect(u, p + ".to_out.0.bias", {dim});
    expect(u, p + ".to_out.1.g", {1, dim});
}

static std::string idx(const std::string& a, int i) { return a + "." + std::to_string(i); }

// ---- Unet1D (DD/denoising_diffusion_1d.py:219-308): the same tree over nn.Conv1d, so rank-3 weights (Cout, Cin, K) and
// gains (1, C, 1), no mem_kv, and every attention wrapped as Residual(PreNorm(dim, fn)): body `.fn.fn`, pre-norm `.fn.norm`
enum { SEQ1D_STAGE_HEADS = 4, SEQ1D_STAGE_DH = 32 };  // LinearAttention(dim) of the stages takes its defaults (:165, :285, :300)
static void expect_resnet1d(dm_unet* u, const std::string& p, int din, int dout) {
    int td = u->time_dim;
    expect(u, p + ".mlp.1.weight", {2 * dout, td});
    expect(u, p + ".mlp.1.bias", {2 * dout});
    expect(u, p + ".block1.proj.weight", {dout, din, 3});
    expect(u, p + ".block1.proj.bias", {dout});
    expect(u, p + ".block1.norm.g", {1, dout, 1});
    expect(u, p + ".block2.proj.weight", {dout, dout, 3});
    expect(u, p + ".block2.proj.bias", {dout});
    expect(u, p + ".block2.norm.g", {1, dout, 1});
    if (din != dout) {
        expect(u, p + ".res_conv.weight", {dout, din, 1});
        expect(u, p + ".res_conv.bias", {dout});
    }
}
static void expect_attn1d(dm_unet* u, const std::string& p, int dim, bool full, int heads, int dh) {
    const int hidden = heads * dh;
    const std::string body = p + ".fn.fn", out = attn_out_param(body, full);
    expect(u, body + ".to_qkv.weight", {3 * hidden, dim, 1});
    expect(u, out + ".weight", {dim, hidden, 1});
    expect(u, out + ".bias", {dim});
    if (!full) expect(u, body + ".to_out.1.g", {1, dim, 1});
    expect(u, p + ".fn.norm.g", {1, dim, 1});
}
// the resample layer of stage q: Downsample is a plain Conv1d(4, 2, 1) (:62-63), Upsample is Sequential(nn.Upsample, Conv1d)
static std::string resample_param1d(const std::string& q, bool up, bool last_stage, const char* leaf) {
    return q + (up && !last_stage ? ".3.1." : ".3.") + leaf;
}
static void expect_unet1d(dm_unet* u) {
    const dm_unet_cfg& cfg = u->cfg;
    const int n = cfg.n_stages, td = u->time_dim;
    expect(u, "init_conv.weight", {u->init_dim, cfg.input_channels, 7});
    expect(u, "init_conv.bias", {u->init_dim});
    if (cfg.learned_sinusoidal_dim > 0) expect(u, "time_mlp.0.weights", {cfg.learned_sinusoidal_dim / 2});
    expect(u, "time_mlp.1.weight", {td, cfg.learned_sinusoidal_dim > 0 ? cfg.learned_sinusoidal_dim + 1 : cfg.dim});
    expect(u, "time_mlp.1.bias", {td});
    expect(u, "time_mlp.3.weight", {td, td});
    expect(u, "time_mlp.3.bias", {td});
    for (int i = 0; i < n; ++i) {
        const int din = u->dims[i], dout = u->dims[i + 1];
        const std::string q = idx("downs", i);
        const bool last = i == n - 1;
        expect_resnet1d(u, q + ".0", din, din);
        expect_resnet1d(u, q + ".1", din, din);
        expect_attn1d(u, q + ".2", din, false, SEQ1D_STAGE_HEADS, SEQ1D_STAGE_DH);
        expect(u, resample_param1d(q, false, last, "weight"), {dout, din, last ? 3 : 4});
        expect(u, resample_param1d(q, false, last, "bias"), {dout});
    }
    for (int j = 0; j < n; ++j) {
        const int din = u->dims[n - 1 - j], dout = u->dims[n - j];
        const std::string q = idx("ups", j);
        expect_resnet1d(u, q + ".0", dout + din, dout);
        expect_resnet1d(u, q + ".1", dout + din, dout);
        expect_attn1d(u, q + ".2", dout, false, SEQ1D_STAGE_HEADS, SEQ1D_STAGE_DH);
        expect(u, resample_param1d(q, true, j == n - 1, "weight"), {din, dout, 3});
        expect(u, resample_param1d(q, true, j == n - 1, "bias"), {din});
    }
    const int mid = u->dims.back();
    expect_resnet1d(u, "mid_block1", mid, mid);
    expect_attn1d(u, "mid_attn", mid, true, cfg.attn_heads, cfg.attn_dim_head);
    expect_resnet1d(u, "mid_block2", mid, mid);
    expect_resnet1d(u, "final_res_block", 2 * u->init_dim, u->init_dim);
    expect(u, "final_conv.weight", {u->out_dim, u->init_dim, 1});
    expect(u, "final_conv.bias", {u->out_dim});
}

#include "unet_graph.inc"

// ---- weight upload ----------------------------------------------------------------------
// Pack an OIHW weight into the layout of every kernel family the layer is eligible for (conv_family.inc) and upload those
// and the bias.  The recorded recipes take their source from L.src, which the caller has set (default: anonymous).
static int make_conv(DeviceOwner& own, ConvLayer& L, const float* oihw, const float* bias, int Cout, int C0, int C1, int KH,
                     int KW, int stride, int pad, bool up, int pad_hi = 0) {
    L.C0 = C0; L.C1 = C1; L.Cout = Cout; L.KH = KH; L.KW = KW; L.stride = stride; L.pad = pad; L.up = up;
    L.pad_hi = pad_hi;
    L.fold = conv_folds(KH, KW, stride, pad, up);
    std::fill(L.packed, L.packed + CONV_KINDS, nullptr);
    if (L.fold) {
        // nearest x2 then conv3x3 == one 2x2 conv per output parity with summed taps:
        //   parity 0 along an axis: source offsets {-1, 0} <- taps {0}, {1,2};  parity 1: {0, +1} <- taps {0,1}, {2}
        const int Cin = C0 + C1;
        const size_t per = conv_packed_floats(Cout, C0, C1, 2, 2);
        std::vector<float> packed(4 * per);
        std::vector<float> w2((size_t)Cout * Cin * 4);
        auto taps = [](int parity, int a, int* lo, int* hi) {
            if (parity == 0) { *lo = a == 0 ? 0 : 1; *hi = a == 0 ? 0 : 2; }
            else             { *lo = a == 0 ? 0 : 2; *hi = a == 0 ? 1 : 2; }
        };
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                for (size_t oc = 0; oc < (size_t)Cout * Cin; ++oc)
                    for (int a = 0; a < 2; ++a)
                        for (int b = 0; b < 2; ++b) {
                            int y0, y1, x0, x1;
                            taps(py, a, &y0, &y1);
                            taps(px, b, &x0, &x1);
                            float sacc = 0.f;
                            for (int dy = y0; dy <= y1; ++dy)
                                for (int dx = x0; dx <= x1; ++dx) sacc += oihw[oc * 9 + dy * 3 + dx];
                            w2[oc * 4 + a * 2 + b] = sacc;
                        }
                conv_pack_weights(w2.data(), packed.data() + (size_t)(py * 2 + px) * per, Cout, C0, C1, 2, 2);
            }
        L.fold_w_stride = (int)per;
        if (own.upload(packed.data(), packed.size(), &L.packed[CONV_DIRECT])) return 1;
        own.record(PK_FOLD, L.packed[CONV_DIRECT], packed.size(), Cout, C0, C1, KH, KW, L.src);
    }
    for (int k = 0; k < CONV_KINDS; ++k)
        for (const ConvRecipe& R : conv_families[k].recipe) {
            if (!R.eligible || !R.eligible(Cout, C0, C1, KH, KW, stride, pad, up)) continue;
            std::vector<float> wp(R.floats(Cout, C0, C1, KH, KW));
            R.pack(oihw, wp.data(), Cout, C0, C1, KH, KW);
            if (own.upload(wp.data(), wp.size(), &L.packed[k])) return 1;
            own.record(R.pk, L.packed[k], wp.size(), Cout, C0, C1, KH, KW, L.src);
        }
    L.bias = nullptr;
    if (bias) {
        if (own.upload(bias, Cout, &L.bias)) return 1;
        own.record(PK_RAW_B, L.bias, Cout, Cout, C0, C1, KH, KW, L.src);
    }
    return 0;
}

static const HostTensor& P(dm_unet* u, const std::string& n) { return u->params.at(n); }

static int up1(dm_unet* u, const std::string& n, float** out) {
    const HostTensor& t = P(u, n);
    if (u->own.upload(t.data.data(), t.data.size(), out)) return 1;
    u->own.record_raw(n, *out, t.data.size());
    return 0;
}
// a layer of the handle from its parameters; the layer keeps their names (bname empty: no bias) for the device-side
// re-packing recipes and for the backward pass
static int make_conv(dm_unet* u, ConvLayer& L, const std::string& wname, const std::string& bname, int Cout, int C0, int C1,
                     int KH, int KW, int stride, int pad, bool up, int pad_hi = 0) {
    L.src = PackSrc();
    L.src.wname = wname;
    L.src.bname = bname;
    return make_conv(u->own, L, P(u, wname).data.data(), bname.empty() ? nullptr : P(u, bname).data.data(), Cout, C0, C1, KH,
                     KW, stride, pad, up, pad_hi);
}
// A K-tap convolution of the handle: K x K with `pad` rows and columns, or in the sequence model 1 x K over the (B, 1, L, C)
// view of a (B, L, C) tensor with `pad` columns.
static int make_conv_k(dm_unet* u, ConvLayer& L, const std::string& wname, const std::string& bname, int Cout, int C0, int C1,
                       int K, int stride, int pad) {
    if (!u->cfg.seq1d) return make_conv(u, L, wname, bname, Cout, C0, C1, K, K, stride, pad, false);
    if (make_conv(u, L, wname, bname, Cout, C0, C1, 1, K, stride, 0, false)) return 1;
    L.pad_w = pad;
    return 0;
}
// Upsample of the sequence model, nearest x2 then Conv1d(K = 3, padding 1) (DD/denoising_diffusion_1d.py:56-60), as ONE K = 3
// convolution on the source grid with 2 Cout output channels: output 2i reads x[i-1], x[i], x[i] and output 2i + 1 reads
// x[i], x[i], x[i+1], so rows [0, Cout) hold the taps {w0, w1 + w2, 0} and rows [Cout, 2 Cout) hold {0, w0 + w1, w2}, the
// bias twice.  The (B, L, 2 Cout) result is the (B, 2L, Cout) tensor in memory.  w (Cout, Cin, 3) -> w2 (2 Cout, Cin, 3).
static void upsample1d_pack(const float* w, const float* bias, int Cout, int Cin, std::vector<float>& w2, std::vector<float>& b2) {
    w2.assign((size_t)2 * Cout * Cin * 3, 0.f);
    b2.assign((size_t)2 * Cout, 0.f);
    for (size_t oc = 0; oc < (size_t)Cout * Cin; ++oc) {
        const float *t = w + oc * 3;
        float* even = w2.data() + oc * 3;
        float* odd = w2.data() + ((size_t)Cout * Cin + oc) * 3;
        even[0] = t[0]; even[1] = t[1] + t[2]; even[2] = 0.f;
        odd[0] = 0.f; odd[1] = t[0] + t[1]; odd[2] = t[2];
    }
    for (int o = 0; o < Cout; ++o) b2[o] = b2[Cout + o] = bias ? bias[o] : 0.f;
}
static int make_upsample1d(DeviceOwner& own, ConvLayer& L, const float* w, const float* bias, int Cout, int Cin) {
    std::vector<float> w2, b2;
    upsample1d_pack(w, bias, Cout, Cin, w2, b2);
    if (make_conv(own, L, w2.data(), bias ? b2.data() : nullptr, 2 * Cout, Cin, 0, 1, 3, 1, 0, false)) return 1;
    L.pad_w = 1;
    return 0;
}
// the parameters of the resample layer of stage q: Sequential(Rearrange / Upsample, conv) in every stage but the last,
// where it is a plain 3x3 convolution
static std::string resample_param(const std::string& q, bool last_stage, const char* leaf) {
    return q + (last_stage ? ".3." : ".3.1.") + leaf;
}

// One weight group = everything packed from the parameters under one name prefix.  First build: run `build` and
// record which uploads it made.  Refresh: re-run it into the same buffers if any of its parameters changed, else skip.
static bool prefix_dirty(dm_unet* u, const std::string& prefix) {
    for (auto it = u->params.lower_bound(prefix); it != u->params.end(); ++it) {
        const std::string& k = it->first;
        if (k.compare(0, prefix.size(), prefix) != 0) break;
        if ((k.size() == prefix.size() || k[prefix.size()] == '.') && it->second.dirty) return true;
    }
    return false;
}
template <class F>
static int weight_group(dm_unet* u, const std::string& prefix, F build) {
    DeviceOwner& own = u->own;
    if (own.refreshing) {
        auto it = u->groups.find(prefix);
        DM_REQUIRE(it != u->groups.end(), "refresh: unknown weight group");
        DM_REQUIRE(own.cursor == it->second.first, "refresh: weight groups out of order");
        if (!prefix_dirty(u, prefix)) {
            own.cursor += it->second.second;
            return 0;
        }
        if (build()) return 1;
        DM_REQUIRE(own.cursor == it->second.first + it->second.second, "refresh: upload count differs from the first build");
        return 0;
    }
    const size_t start = own.ptrs.size();
    if (build()) return 1;
    u->groups[prefix] = {start, own.ptrs.size() - start};
    return 0;
}

static int build_resnet(dm_unet* u, ResBlock& R, const std::string& p, int C0, int C1, int dout, int& ss_off) {
    // the mlp (SiLU -> Linear) of every ResnetBlock is one row block of the concatenated [ss_total][time_dim] matrix
    // assembled by build_scale_shift
    R.prefix = p;
    R.dout = dout;
    R.ss_off = ss_off;
    ss_off += 2 * dout;
    if (!u->own.refreshing) u->resnets.emplace_back(p, &R);
    return weight_group(u, p, [&]() -> int {
        if (make_conv_k(u, R.c1, p + ".block1.proj.weight", p + ".block1.proj.bias", dout, C0, C1, 3, 1, 1)) return 1;
        if (make_conv_k(u, R.c2, p + ".block2.proj.weight", p + ".block2.proj.bias", dout, dout, 0, 3, 1, 1)) return 1;
        if (up1(u, p + ".block1.norm.g", &R.g1) || up1(u, p + ".block2.norm.g", &R.g2)) return 1;
        R.has_res = C0 + C1 != dout;
        return R.has_res ? make_conv_k(u, R.res, p + ".res_conv.weight", p + ".res_conv.bias", dout, C0, C1, 1, 1, 0) : 0;
    });
}

static int build_scale_shift(dm_unet* u) {
    bool dirty = false;
    for (auto& pr : u->resnets) dirty = dirty || P(u, pr.first + ".mlp.1.weight").dirty || P(u, pr.first + ".mlp.1.bias").dirty;
    if (u->own.refreshing && !dirty) {
        u->own.cursor += 2;
        return 0;
    }
    std::vector<float> ssw, ssb;
    for (auto& pr : u->resnets) {
        const HostTensor& mw = P(u, pr.first + ".mlp.1.weight");
        const HostTensor& mb = P(u, pr.first + ".mlp.1.bias");
        ssw.insert(ssw.end(), mw.data.begin(), mw.data.end());
        ssb.insert(ssb.end(), mb.data.begin(), mb.data.end());
    }
    if (u->own.upload(ssw.data(), ssw.size(), &u->ss_w) || u->own.upload(ssb.data(), ssb.size(), &u->ss_b)) return 1;
    size_t ow = 0, ob = 0;  // recipe: every ResnetBlock.mlp is a row block of the concatenated matrix
    for (auto& pr : u->resnets) {
        const HostTensor& mw = P(u, pr.first + ".mlp.1.weight");
        const HostTensor& mb = P(u, pr.first + ".mlp.1.bias");
        u->own.record_raw(pr.first + ".mlp.1.weight", u->ss_w + ow, mw.data.size());
        u->own.record_raw(pr.first + ".mlp.1.bias", u->ss_b + ob, mb.data.size());
        ow += mw.data.size();
        ob += mb.data.size();
    }
    return 0;
}

// The fused form of a LinearAttention layer (linattn_fused.hip) from host copies of its weights.  A.out.bias and A.mem_kv
// are already on the device.  has_fused stays false when the layer is not eligible or a softmax bound is too large for
// the shift trick: such a layer keeps the unfused chain.
static int fuse_linattn(DeviceOwner& own, AttnLayer& A, const float* w_qkv, const float* norm_g, const float* w_out,
                        const float* mem_kv, const float* out_g, int dim, int heads, int dh) {
    A.has_fused = false;
    if (!linattn_fused_eligible(dim, heads, dh)) return 0;
    std::vector<float> wq, wk, wv, wo, kb;
    if (!linattn_fused_pack(w_qkv, norm_g, w_out, mem_kv, dim, wq, wk, wv, wo, kb)) return 0;
    std::vector<float> ogs(out_g, out_g + dim);
    for (float& v : ogs) v *= std::sqrt((float)dim);
    float *dq, *dk, *dv, *dwo, *dkb, *dog;
    if (own.upload(wq.data(), wq.size(), &dq) || own.upload(wk.data(), wk.size(), &dk) ||
        own.upload(wv.data(), wv.size(), &dv) || own.upload(w_out, (size_t)dim * heads * dh, &dwo) ||
        own.upload(kb.data(), kb.size(), &dkb) || own.upload(ogs.data(), ogs.size(), &dog))
        return 1;
    A.fused = LinAttnFused{dim, dq, dk, dv, dwo, A.out.bias, dog, dkb, A.mem_kv};
    A.has_fused = true;
    return 0;
}

static int build_attn_body(dm_unet* u, AttnLayer& A, const std::string& p, int dim, bool full, int heads) {
    A.prefix = p;
    A.full = full;
    A.dim = dim;
    A.heads = heads;
    int hidden = heads * u->dh;
    if (up1(u, p + ".norm.g", &A.norm_g) || up1(u, p + ".mem_kv", &A.mem_kv)) return 1;
    const std::string out = attn_out_param(p, full);
    if (make_conv(u, A.qkv, p + ".to_qkv.weight", "", 3 * hidden, dim, 0, 1, 1, 1, 0, false)) return 1;
    if (make_conv(u, A.out, out + ".weight", out + ".bias", dim, hidden, 0, 1, 1, 1, 0, false)) return 1;
    if (full) {
        A.has16 = false;
        if (attn16_eligible(dim, heads, u->dh)) {
            std::vector<float> wp, wo;
            attn16_pack(P(u, p + ".to_qkv.weight").data.data(), P(u, p + ".norm.g").data.data(),
                        P(u, out + ".weight").data.data(), dim, wp, wo);
            float *dwp, *dwo;
            if (u->own.upload(wp.data(), wp.size(), &dwp) || u->own.upload(wo.data(), wo.size(), &dwo)) return 1;
            A.a16 = Attn16{dim, dwp, dwo, A.out.bias, A.mem_kv};
            A.has16 = true;
        }
    } else {
        if (up1(u, p + ".to_out.1.g", &A.out_g)) return 1;
        if (fuse_linattn(u->own, A, P(u, p + ".to_qkv.weight").data.data(), P(u, p + ".norm.g").data.data(),
                         P(u, out + ".weight").data.data(), P(u, p + ".mem_kv").data.data(),
                         P(u, p + ".to_out.1.g").data.data(), dim, heads, u->dh))
            return 1;
    }
    return 0;
}

// An attention layer of the sequence model: no memory key / values, so the fused kernels (which bake the memory rows in) do
// not apply and the layer runs as pre-norm, to_qkv, core, to_out.
static int build_attn1d(dm_unet* u, AttnLayer& A, const std::string& p, int dim, bool full, int heads, int dh) {
    return weight_group(u, p, [&]() -> int {
        const std::string body = p + ".fn.fn", out = attn_out_param(body, full);
        A.prefix = p;
        A.full = full;
        A.dim = dim;
        A.heads = heads;
        A.dh = dh;
        A.mem_kv = nullptr;
        A.has_fused = A.has16 = false;
        if (up1(u, p + ".fn.norm.g", &A.norm_g)) return 1;
        if (make_conv_k(u, A.qkv, body + ".to_qkv.weight", "", 3 * heads * dh, dim, 0, 1, 1, 0)) return 1;
        if (make_conv_k(u, A.out, out + ".weight", out + ".bias", dim, heads * dh, 0, 1, 1, 0)) return 1;
        return full ? 0 : up1(u, body + ".to_out.1.g", &A.out_g);
    });
}

static int build_attn(dm_unet* u, AttnLayer& A, const std::string& p, int dim, bool full, int heads) {
    return weight_group(u, p, [&]() -> int { return build_attn_body(u, A, p, dim, full, heads); });
}

static int build_cross_body(dm_unet* u, CrossLayer& C, const std::string& p, int dim) {
    int inner = 4 * u->dh;
    C.prefix = p;
    // nn.Linear weights [out, in] are 1x1 conv weights (out, in, 1, 1)
    if (make_conv(u, C.q, p + ".to_q.weight", "", inner, dim, 0, 1, 1, 1, 0, false)) return 1;
    if (make_conv(u, C.out, p + ".to_out.0.weight", p + ".to_out.0.bias", dim, inner, 0, 1, 1, 1, 0, false)) return 1;
    if (up1(u, p + ".to_k.weight", &C.wk) || up1(u, p + ".to_v.weight", &C.wv) || up1(u, p + ".to_out.1.g", &C.g) ||
        up1(u, p + ".to_out.0.weight", &C.wo_raw))
        return 1;
    return 0;
}

static int build_cross(dm_unet* u, CrossLayer& C, const std::string& p, int dim) {
    return weight_group(u, p, [&]() -> int { return build_cross_body(u, C, p, dim); });
}

// Pack every parameter into its kernel layout and upload it: the first build (dm_unet_finalize) and, with
// own.refreshing set, the in-place refresh of changed parameters (dm_unet_refresh).
static int build_all(dm_unet* u) {
    if (u->kunet) return kunet_build_all(u);
    const dm_unet_cfg& cfg = u->cfg;
    const int n = cfg.n_stages;
    // sinusoid frequencies, fp32 as the reference computes them (DD/denoising_diffusion.py:79-81)
    if (cfg.learned_sinusoidal_dim > 0) {
        // RandomOrLearnedSinusoidalPosEmb (:86-101): the frequencies are the parameter time_mlp.0.weights
        if (weight_group(u, "time_mlp.0", [&]() -> int { return up1(u, "time_mlp.0.weights", &u->freqs); })) return 1;
    } else if (weight_group(u, "#freqs", [&]() -> int {
            int half = cfg.dim / 2;
            double k = std::log((double)cfg.sinusoidal_theta) / (half - 1);
            float kf = (float)(-k);
            std::vector<float> f(half);
            for (int i = 0; i < half; ++i) f[i] = std::exp((float)i * kf);
            return u->own.upload(f.data(), f.size(), &u->freqs);
        }))
        return 1;
    if (weight_group(u, "time_mlp", [&]() -> int {
            return up1(u, "time_mlp.1.weight", &u->tw1) || up1(u, "time_mlp.1.bias", &u->tb1) ||
                   up1(u, "time_mlp.3.weight", &u->tw2) || up1(u, "time_mlp.3.bias", &u->tb2);
        }))
        return 1;
    if (weight_group(u, "init_conv", [&]() -> int {
            return make_conv_k(u, u->init_conv, "init_conv.weight", "init_conv.bias", u->init_dim, cfg.input_channels, 0, 7, 1, 3);
        }))
        return 1;
    int ss_off = 0;
    u->downs.resize(n);
    u->ups.resize(n);
    for (int i = 0; i < n; ++i) {
        int din = u->dims[i], dout = u->dims[i + 1];
        std::string q = idx("downs", i);
        Stage& S = u->downs[i];
        if (build_resnet(u, S.b1, q + ".0", din, 0, din, ss_off)) return 1;
        if (build_resnet(u, S.b2, q + ".1", din, 0, din, ss_off)) return 1;
        if (cfg.seq1d ? build_attn1d(u, S.attn, q + ".2", din, false, SEQ1D_STAGE_HEADS, SEQ1D_STAGE_DH)
                      : build_attn(u, S.attn, q + ".2", din, cfg.full_attn[i] != 0, stage_heads(cfg, i)))
            return 1;
        if (weight_group(u, q + ".3", [&]() -> int {
                const bool last = i == n - 1;
                if (cfg.seq1d)  // Conv1d(4, 2, 1), or in the last stage Conv1d(3, padding 1) (:286)
                    return make_conv_k(u, S.resample, resample_param1d(q, false, last, "weight"),
                                       resample_param1d(q, false, last, "bias"), dout, din, 0, last ? 3 : 4, last ? 1 : 2, 1);
                const std::string w = resample_param(q, last, "weight"), b = resample_param(q, last, "bias");
                if (last) return make_conv(u, S.resample, w, b, dout, din, 0, 3, 3, 1, 1, false);
                // pixel-unshuffle + 1x1  ==  2x2 stride-2 conv: W'[o][c][p1][p2] = W[o][c*4 + p1*2 + p2]
                return make_conv(u, S.resample, w, b, dout, din, 0, 2, 2, 2, 0, false);
            }))
            return 1;
    }
    int mid = u->dims.back();
    if (build_resnet(u, u->mid1, "mid_block1", mid, 0, mid, ss_off)) return 1;
    if (cfg.seq1d ? build_attn1d(u, u->mid_attn, "mid_attn", mid, true, cfg.attn_heads, cfg.attn_dim_head)
                  : build_attn(u, u->mid_attn, "mid_attn", mid, true, stage_heads(cfg, n - 1)))
        return 1;
    if (build_resnet(u, u->mid2, "mid_block2", mid, 0, mid, ss_off)) return 1;
    for (int j = 0; j < n; ++j) {
        int din = u->dims[n - 1 - j], dout = u->dims[n - j];
        std::string q = idx("ups", j);
        Stage& S = u->ups[j];
        if (build_resnet(u, S.b1, q + ".0", dout, din, dout, ss_off)) return 1;
        if (build_resnet(u, S.b2, q + ".1", dout, din, dout, ss_off)) return 1;
        if (cfg.seq1d ? build_attn1d(u, S.attn, q + ".2", dout, false, SEQ1D_STAGE_HEADS, SEQ1D_STAGE_DH)
                      : build_attn(u, S.attn, q + ".2", dout, cfg.full_attn[n - 1 - j] != 0, stage_heads(cfg, n - 1 - j)))
            return 1;
        if (weight_group(u, q + ".3", [&]() -> int {
                const bool last = j == n - 1;
                if (cfg.seq1d) {
                    const std::string w = resample_param1d(q, true, last, "weight"), b = resample_param1d(q, true, last, "bias");
                    if (last) return make_conv_k(u, S.resample, w, b, din, dout, 0, 3, 1, 1);
                    S.resample.src = PackSrc();
                    S.resample.src.kind = PS_UP1D;
                    S.resample.src.wname = w;
                    S.resample.src.bname = b;
                    S.resample.src.sCout = din; S.resample.src.sCin = dout; S.resample.src.sK = 3;
                    return make_upsample1d(u->own, S.resample, P(u, w).data.data(), P(u, b).data.data(), din, dout);
                }
                return make_conv(u, S.resample, resample_param(q, last, "weight"), resample_param(q, last, "bias"), din, dout, 0,
                                 3, 3, 1, 1, /*up=*/!last);
            }))
            return 1;
    }
    if (build_resnet(u, u->final_res, "final_res_block", u->init_dim, u->init_dim, u->init_dim, ss_off)) return 1;
    if (weight_group(u, "final_conv", [&]() -> int {
            return make_conv_k(u, u->final_conv, "final_conv.weight", "final_conv.bias", u->out_dim, u->init_dim, 0, 1, 1, 0);
        }))
        return 1;
    u->ss_total = ss_off;
    if (build_scale_shift(u)) return 1;
    if (cfg.text_mode == DM_TEXT_CONCAT) {
        if (weight_group(u, "text_proj", [&]() -> int {
                return up1(u, "text_proj.0.weight", &u->tp_w0) || up1(u, "text_proj.0.bias", &u->tp_b0) ||
                       up1(u, "text_proj.2.weight", &u->tp_w2) || up1(u, "text_proj.2.bias", &u->tp_b2);
            }) ||
            weight_group(u, "text_concat_proj", [&]() -> int {
                return up1(u, "text_concat_proj.weight", &u->tc_w) || up1(u, "text_concat_proj.bias", &u->tc_b);
            }))
            return 1;
    } else if (cfg.text_mode == DM_TEXT_CROSS) {
        if (build_cross(u, u->cross_mid, "cross_attn", mid) || build_cross(u, u->cross_down, "cross_attn_down", mid) ||
            build_cross(u, u->cross_up, "cross_attn_up", mid))
            return 1;
    }
    if (!u->own.refreshing) build_unet_graphs(u);
    return 0;
}

// ---- launches ---------------------------------------------------------------------------
struct Ctx {
    dm_unet* u;
    Arena* A;
    hipStream_t s;
    int B;
    const float* ss;   // [Bt][ss_total]
    int ss_stride;     // 0 when one row serves the whole batch
    bool dry() const { return A->dry; }
};

// residual operand of a landing pass given as the K-split partial sums of another convolution (+ its bias)
struct ResParts {
    const float* part;
    int nsplit;
    int64_t stride;
    const float* bias;
};

struct PlannedConv {
    ConvParams p;      // everything but the tensor pointers
    int out_h, out_w;  // dims of the output tensor
    ConvKind kind;     // the kernel family (conv_family.inc)
    bool in_kernel;    // the epilogue runs inside the conv kernel (else: partial sums + landing kernel)
};
// the convolution leaves K-split / multi-tile partial sums that a landing pass (its own or a consumer's) has to sum
static bool plan_leaves_partials(const PlannedConv& P) { return !P.in_kernel && conv_families[P.kind].partials; }

// Which kernel and tiling a convolution takes; a function of the layer, the batch and the image size only.
static int plan_conv(const Ctx& c, const ConvLayer& L, bool has_in1, int Hin, int Win, int epi, bool in_nchw, bool out_nchw,
                     PlannedConv& P) {
    ConvParams& p = P.p;
    p = ConvParams{};
    p.C0 = L.C0; p.C1 = L.C1;
    const int CK = conv_ck_for(L.C0, L.C1);
    p.chunks0 = (L.C0 + CK - 1) / CK;
    p.n_chunks = p.chunks0 + (L.C1 ? (L.C1 + CK - 1) / CK : 0);
    p.in_nchw = in_nchw ? 1 : 0;
    p.bias = L.bias;
    p.Cout = L.Cout; p.stride = L.stride; p.pad = L.pad;
    const int padw = L.pad_w >= 0 ? L.pad_w : L.pad;
    p.pad_w = padw;
    p.B = c.B;
    p.out_nchw = out_nchw ? 1 : 0;
    p.ss_stride = c.ss_stride;
    const bool want_norm = (epi & EPI_NORM) != 0;
    // the family takes the layer: its packed weights and, where the layout has K chunks of its own width, their counts
    auto take = [&](ConvKind kind) {
        P.kind = kind;
        p.w = L.packed[kind];
        if (const int kc = conv_families[kind].k_chunk) {
            p.chunks0 = L.C0 / kc;
            p.n_chunks = (L.C0 + L.C1) / kc;
        }
    };
    take(CONV_DIRECT);
    const bool upwino = L.up && L.packed[CONV_UPWINO] && !in_nchw && !out_nchw && !has_in1 && Hin % 2 == 0 && Win % 2 == 0 &&
                        upwino_shape_ok(c.B, Hin / 2, Win / 2, L.Cout, L.C0, L.C1);
    if (upwino) {
        // (Hin, Win) is the upsampled size the caller sees; the kernel works on the source grid (upwino_mfma.hip)
        p.fold = 0; p.fold_w_stride = 0; p.up = 1;
        p.KH = 3; p.KW = 3;
        p.Hin = Hin / 2; p.Win = Win / 2;
        p.Ho = Hin; p.Wo = Win;
        P.out_h = Hin; P.out_w = Win;
        take(CONV_UPWINO);
        p.geo = upwino_plan(c.B, p.Hin, p.Win, L.Cout, L.C0, L.C1, true);
    } else if (L.fold) {
        // (Hin, Win) is the upsampled size the caller sees; the four parity convs run on the source grid
        DM_REQUIRE(!out_nchw && !in_nchw, "folded upsample conv is NHWC");
        p.fold = 1; p.fold_w_stride = L.fold_w_stride; p.up = 0;
        p.KH = 2; p.KW = 2; p.pad_w = 1;
        p.Hin = Hin / 2; p.Win = Win / 2;
        p.Ho = p.Hin; p.Wo = p.Win;
        P.out_h = Hin; P.out_w = Win;
        p.geo = conv_plan(c.B, p.Ho, p.Wo, L.Cout, 2, 2, 1, L.C0, L.C1, want_norm, true, 4);
    } else if (L.KH == 2 && L.KW == 2 && L.stride == 2 && L.pad == 0 && !L.up && L.C1 == 0 && L.C0 % 16 == 0 &&
               !in_nchw && Hin % 2 == 0 && Win % 2 == 0) {
        // Downsample: space-to-depth, then a 1x1 convolution over 4*C0 channels (ConvParams::s2d)
        p.fold = 0; p.fold_w_stride = 0; p.up = 0; p.s2d = 1;
        p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0; p.pad_w = 0;
        p.Ho = Hin / 2; p.Wo = Win / 2;
        p.Hin = p.Ho; p.Win = p.Wo;
        p.chunks0 = p.n_chunks = 4 * (L.C0 / 16);
        P.out_h = p.Ho; P.out_w = p.Wo;
        if (L.packed[CONV_PW] && !out_nchw && pw_shape_ok(c.B, p.Ho, p.Wo, L.Cout, 4 * L.C0, 0)) {
            // the 1x1 GEMM kernel in space-to-depth mode (pw_mfma.hip): the K chunks run over (cin chunk, tap) as above
            P.kind = CONV_PW;
            p.w = L.packed[CONV_PW];
            p.geo = pw_plan(c.B, p.Ho, p.Wo, L.Cout, 4 * L.C0, 0, true);
            P.in_kernel = p.geo.splits == 1 && (!want_norm || p.geo.fused_norm);
            return 0;
        }
        p.geo = conv_plan(c.B, p.Ho, p.Wo, L.Cout, 1, 1, 1, 4 * L.C0, 0, want_norm && !out_nchw, !out_nchw);
    } else {
        p.fold = 0; p.fold_w_stride = 0; p.up = L.up ? 1 : 0;
        p.KH = L.KH; p.KW = L.KW;
        p.Hin = Hin; p.Win = Win;
        // the kernel zero-fills every window pixel outside the image, so bottom / right padding is only an output size
        p.Ho = (Hin + 2 * L.pad + L.pad_hi - L.KH) / L.stride + 1;
        p.Wo = (Win + 2 * padw + L.pad_hi - L.KW) / L.stride + 1;
        P.out_h = p.Ho; P.out_w = p.Wo;
        p.geo = conv_plan(c.B, p.Ho, p.Wo, L.Cout, L.KH, L.KW, L.stride, L.C0, L.C1, want_norm && !out_nchw,
                          !out_nchw);
    }
    const bool direct = P.kind == CONV_DIRECT;  // no family has taken the layer yet
    if (direct && L.packed[CONV_INIT7] && in_nchw && !out_nchw && !has_in1 && epi == 0 && L.pad_hi == 0 && padw == L.pad &&
        (size_t)c.B * p.Ho * p.Wo < (1u << 24)) {
        take(CONV_INIT7);
        P.in_kernel = true;
        return 0;
    }
    if (L.packed[CONV_THIN] && out_nchw && !in_nchw && !has_in1 && epi == 0) {
        // a handful of output channels (final_conv): one pixel per thread instead of a 64-column MFMA tile
        take(CONV_THIN);
        P.in_kernel = true;
        return 0;
    }
    // 3x3 / stride 1 convolutions run as Winograd F(4x4,3x3) on power-of-two images, else as F(2x2,3x3), when the layer
    // has transformed weights
    const bool wino4 = direct && L.packed[CONV_WINO4] && !L.fold && !in_nchw && !out_nchw && padw == L.pad &&
                       wino4_shape_ok(c.B, p.Ho, p.Wo, L.Cout, L.C0, L.C1);
    const bool wino = direct && !wino4 && L.packed[CONV_WINO] && !L.fold && !in_nchw && !out_nchw && padw == L.pad &&
                      wino_shape_ok(c.B, p.Ho, p.Wo, L.Cout, L.C0, L.C1);
    const bool pw = direct && L.packed[CONV_PW] && !L.fold && !p.s2d && !in_nchw && !out_nchw && L.pad_hi == 0 && padw == 0 &&
                    pw_shape_ok(c.B, p.Ho, p.Wo, L.Cout, L.C0, L.C1);
    if (pw) {
        take(CONV_PW);
        p.geo = pw_plan(c.B, p.Ho, p.Wo, L.Cout, L.C0, L.C1, true);
    } else if (wino4) {
        take(CONV_WINO4);
        p.geo = wino4_plan(c.B, p.Ho, p.Wo, L.Cout, L.C0, L.C1, true);
    } else if (wino) {
        take(CONV_WINO);
        p.geo = wino_plan(c.B, p.Ho, p.Wo, L.Cout, L.C0, L.C1, true, want_norm);
    }
    P.in_kernel = p.geo.splits == 1 && (!want_norm || p.geo.fused_norm);
    return 0;
}

static int launch_planned(const PlannedConv& P, const ConvParams& q, hipStream_t s, dm_unet* u = nullptr) {
    if (u && u->train && ensure_packed(u, q.w, s)) return 1;  // training loop: weights re-packed on the device when stale
    return conv_families[P.kind].launch(q, s);
}

static int run_conv(Ctx& c, const ConvLayer& L, const float* in0, const float* in1, int Hin, int Win, float* out,
                    int epi, const float* g, const float* scale, const float* residual, bool in_nchw = false,
                    bool out_nchw = false, const ResParts* res_parts = nullptr) {
    // One convolution with its epilogue (epi = EPI_* requested by the caller; bias is implied by the layer).
    // The plan decides whether the epilogue runs inside the conv kernel (one workgroup owns all couts of a
    // pixel and K is not split) or in norm_act_kernel on the raw / K-split partial sums.  res_parts: the residual
    // is the sum of another convolution's partial tiles (only on the landing path; the caller asks plan_conv first).
    PlannedConv P;
    if (plan_conv(c, L, in1 != nullptr, Hin, Win, epi, in_nchw, out_nchw, P)) return 1;
    ConvParams& p = P.p;
    p.in0 = in0; p.in1 = in1;
    p.residual = residual; p.g = g; p.scale = scale;
    const int full_epi = epi | (L.bias ? EPI_BIAS : 0);
    if (P.in_kernel) {
        DM_REQUIRE(!res_parts, "residual partial sums need the landing pass");
        if (c.dry()) return 0;
        p.out = out; p.partial = 0; p.epi = full_epi;
        return launch_planned(P, p, c.s, c.u);
    }
    DM_REQUIRE(!out_nchw, "split / unfused epilogue writes NHWC");
    const size_t M = (size_t)c.B * P.out_h * P.out_w;
    float* part = c.A->alloc((size_t)p.geo.splits * M * L.Cout);
    if (c.dry()) {
        c.A->release(part);
        return 0;
    }
    p.out = part; p.partial = 1; p.epi = 0;
    if (launch_planned(P, p, c.s, c.u)) return 1;
    const ResParts res = res_parts ? *res_parts : ResParts{residual, 1, 0, nullptr};  // a plain tensor is one "split"
    const int rc = launch_norm_act(part, p.geo.splits, (int64_t)(M * L.Cout), L.bias, g, scale, c.ss_stride, P.out_h * P.out_w,
                                   res.part, out, (int64_t)M, L.Cout, full_epi | (res_parts ? EPI_RESIDUAL : 0), c.s, res.nsplit,
                                   res.stride, res.bias);
    c.A->release(part);
    return rc;
}

// The raw K-split partial sums of a convolution (no bias, no epilogue) for a consumer that lands them itself:
// *part = [nsplit][B*Ho*Wo][Cout], allocated here, released by the caller.
static int run_conv_partial(Ctx& c, const ConvLayer& L, const float* in0, const float* in1, int Hin, int Win, float** part,
                            int* nsplit) {
    PlannedConv P;
    if (plan_conv(c, L, in1 != nullptr, Hin, Win, 0, false, false, P)) return 1;
    DM_REQUIRE(conv_families[P.kind].partials, "partial sums of a layer whose kernel writes none");
    ConvParams& p = P.p;
    p.in0 = in0; p.in1 = in1;
    const size_t M = (size_t)c.B * P.out_h * P.out_w;
    *part = c.A->alloc((size_t)p.geo.splits * M * L.Cout);
    *nsplit = p.geo.splits;
    if (c.dry()) return 0;
    p.out = *part; p.partial = 1; p.epi = 0;
    return launch_planned(P, p, c.s, c.u);
}

// Block.forward: conv3x3 -> RMSNorm -> (scale+1, shift) -> SiLU [-> + residual]
static int run_block(Ctx& c, const ConvLayer& L, const float* in0, const float* in1, int H, int W, const float* g,
                     const float* scale, const float* residual, float* out, const ResParts* res_parts = nullptr) {
    int flags = EPI_NORM | EPI_SILU | (scale ? EPI_SCALE_SHIFT : 0) | (residual ? EPI_RESIDUAL : 0);
    return run_conv(c, L, in0, in1, H, W, out, flags, g, scale, residual, false, false, res_parts);
}

// ResnetBlock.forward (DD/denoising_diffusion.py:136-148); x = cat(x0, x1)
static int run_resnet(Ctx& c, const ResBlock& R, const float* x0, const float* x1, int H, int W, float** out) {
    size_t n = (size_t)c.B * H * W * R.dout;
    const float* scale = c.ss ? c.ss + R.ss_off : nullptr;
    // block2(h1) + res_conv(x).  When both convolutions leave partial sums for a landing pass anyway (several cout
    // tiles under one RMSNorm, or K splits), one landing serves both: it finishes block2 and adds the res_conv partials.
    static const bool merge = !env_flag("DM_NO_RES_MERGE");
    PlannedConv P2, Pr;
    bool merged = false;
    if (R.has_res) {
        if (plan_conv(c, R.c2, false, H, W, EPI_NORM | EPI_SILU, false, false, P2)) return 1;
        if (plan_conv(c, R.res, x1 != nullptr, H, W, EPI_RESIDUAL, false, false, Pr)) return 1;
        merged = merge && plan_leaves_partials(P2) && plan_leaves_partials(Pr);
    }
    ResParts rp{};
    float* rpart = nullptr;
    if (merged) {
        if (run_conv_partial(c, R.res, x0, x1, H, W, &rpart, &rp.nsplit)) return 1;
        rp.part = rpart;
        rp.stride = (int64_t)n;
        rp.bias = R.res.bias;
    }
    float* h1 = c.A->alloc(n);
    float* h2 = c.A->alloc(n);
    if (run_block(c, R.c1, x0, x1, H, W, R.g1, scale, nullptr, h1)) return 1;
    if (!R.has_res) {
        if (run_block(c, R.c2, h1, nullptr, H, W, R.g2, nullptr, x0, h2)) return 1;
        c.A->release(h1);
        *out = h2;
        return 0;
    }
    if (merged) {
        if (run_block(c, R.c2, h1, nullptr, H, W, R.g2, nullptr, nullptr, h2, &rp)) return 1;
        c.A->release(rpart);
        c.A->release(h1);
        *out = h2;
        return 0;
    }
    if (run_block(c, R.c2, h1, nullptr, H, W, R.g2, nullptr, nullptr, h2)) return 1;
    c.A->release(h1);
    float* o = c.A->alloc(n);
    if (run_conv(c, R.res, x0, x1, H, W, o, EPI_RESIDUAL, nullptr, nullptr, h2)) return 1;
    c.A->release(h2);
    *out = o;
    return 0;
}

// The front of an unfused attention layer, shared by the inference form (run_attn) and the tape form (t_attn), into the
// caller's buffers: pre-norm -> to_qkv, then the attention core.  Two calls, because a LinearAttention caller allocates the
// core's buffers between them.  ctxws / kst: LinearAttention only; kst (the key statistics) only for the tape.
static int attn_qkv(Ctx& c, const AttnLayer& At, const float* x, int H, int W, float* xn, float* qkv) {
    const int n = H * W;
    if (!c.dry() && launch_norm_act(x, 1, 0, nullptr, At.norm_g, nullptr, 0, n, nullptr, xn, (int64_t)c.B * n, At.dim, EPI_NORM, c.s))
        return 1;
    return run_conv(c, At.qkv, xn, nullptr, H, W, qkv, 0, nullptr, nullptr, nullptr);
}
static int attn_dh(const dm_unet* u, const AttnLayer& At) { return At.dh ? At.dh : u->dh; }
static int attn_core(Ctx& c, const AttnLayer& At, const float* qkv, int n, float* o, float* ctxws, float* kst) {
    if (c.dry()) return 0;
    const int heads = At.heads, dh = attn_dh(c.u, At), hidden = heads * dh;
    if (!At.full) return launch_linear_attention_core(qkv, At.mem_kv, ctxws, o, c.B, n, heads, dh, c.s, kst);
    const float* mk = At.mem_kv;
    const float* mv = At.mem_kv ? At.mem_kv + (size_t)heads * 4 * dh : nullptr;
    return launch_attention_core(qkv, 3 * hidden, qkv + hidden, qkv + 2 * hidden, 3 * hidden, mk, mv, At.mem_kv ? 4 : 0, o, hidden,
                                 c.B, n, n, heads, dh, 1.0f / sqrtf((float)dh), c.s);
}

// attn(x) + x  (LinearAttention DD/denoising_diffusion.py:173-193, Attention :215-229)
static int run_attn(Ctx& c, const AttnLayer& At, const float* x, int H, int W, float** out, bool add_x = true) {
    const int res_flag = add_x ? EPI_RESIDUAL : 0;
    const float* xres = add_x ? x : nullptr;
    dm_unet* u = c.u;
    const int n = H * W, heads = At.heads, dh = attn_dh(u, At), hidden = heads * dh;
    const size_t rows = (size_t)c.B * n;
    if (!At.full && At.has_fused) {
        float* ws = c.A->alloc(linattn_fused_ws_floats(c.B, n));
        float* yf = c.A->alloc(rows * At.dim);
        if (!c.dry() && launch_linattn_fused(At.fused, x, ws, yf, c.B, n, add_x, c.s)) return 1;
        c.A->release(ws);
        *out = yf;
        return 0;
    }
    if (At.full && At.has16 && n == 16) {
        float* yf = c.A->alloc(rows * At.dim);
        if (!c.dry() && launch_attn16_fused(At.a16, x, yf, c.B, add_x, c.s)) return 1;
        *out = yf;
        return 0;
    }
    float* xn = c.A->alloc(rows * At.dim);
    float* qkv = c.A->alloc(rows * 3 * hidden);
    float* o = c.A->alloc(rows * hidden);
    float* y = c.A->alloc(rows * At.dim);
    if (attn_qkv(c, At, x, H, W, xn, qkv)) return 1;
    if (At.full) {
        if (attn_core(c, At, qkv, n, o, nullptr, nullptr)) return 1;
        if (run_conv(c, At.out, o, nullptr, H, W, y, res_flag, nullptr, nullptr, xres)) return 1;
    } else {
        float* ctxws = c.A->alloc((size_t)c.B * heads * dh * dh);
        if (attn_core(c, At, qkv, n, o, ctxws, nullptr)) return 1;
        if (run_conv(c, At.out, o, nullptr, H, W, y, EPI_NORM | res_flag, At.out_g, nullptr, xres)) return 1;
        c.A->release(ctxws);
    }
    c.A->release(xn);
    c.A->release(qkv);
    c.A->release(o);
    *out = y;
    return 0;
}

// DM_NO_CROSS1: the general CrossAttention path for one context token too (and no dead-bottleneck shortcut)
static bool cross1_off() {
    static const bool off = env_flag("DM_NO_CROSS1");
    return off;
}

// The front of the general CrossAttention path (m context tokens), shared by run_cross and the tape form t_cross, into the
// caller's buffers: to_q over the pixels, to_k / to_v over the context rows, the attention core
static int cross_front(Ctx& c, const CrossLayer& Cr, const float* x, int H, int W, const float* ctx, int m, float* q, float* k,
                       float* v, float* o) {
    const int n = H * W, dh = c.u->dh, inner = 4 * dh, E = c.u->cfg.text_emb_dim;
    if (run_conv(c, Cr.q, x, nullptr, H, W, q, 0, nullptr, nullptr, nullptr)) return 1;
    if (c.dry()) return 0;
    if (launch_linear_rows(ctx, E, Cr.wk, nullptr, k, inner, c.B * m, E, inner, 0, 0, c.s)) return 1;
    if (launch_linear_rows(ctx, E, Cr.wv, nullptr, v, inner, c.B * m, E, inner, 0, 0, c.s)) return 1;
    return launch_attention_core(q, inner, k, v, inner, nullptr, nullptr, 0, o, inner, c.B, n, m, 4, dh, 1.0f / sqrtf((float)dh), c.s);
}

// CrossAttention.forward (DD/denoising_diffusion_text_conditional.py:54-78); the result REPLACES x (:173-177)
static int run_cross(Ctx& c, const CrossLayer& Cr, const float* x, int H, int W, const float* ctx, int m,
                     float** out, const int32_t* tmask = nullptr) {
    // tmask (classifier-free guidance's batched forward): the layers are skipped for images with tmask == 0
    // (DD/denoising_diffusion_text_conditional.py:173,183,194 when text_emb is None), so those rows keep x
    auto keep_null_rows = [&](float* y) -> int {
        if (!tmask || c.dry()) return 0;
        return launch_select_rows(y, x, (int64_t)H * W * Cr.out.Cout, tmask, c.B, (int64_t)H * W * Cr.out.Cout, c.s);
    };
    dm_unet* u = c.u;
    const int n = H * W, inner = 4 * u->dh, dim = Cr.out.Cout, E = u->cfg.text_emb_dim;
    const size_t rows = (size_t)c.B * n;
    if (m == 1 && !cross1_off()) {
        // One context token (what every sampler of the reference passes: (B, 512) -> (B, 1, 512), :57-58): the softmax
        // over a single key is exactly 1.0, so every query's output is v and the q / k projections drop out.  The layer
        // is z_b = RMSNorm1D(to_out(to_v(ctx_b))) spread over the pixels of image b -- three row-per-image launches and
        // one broadcast instead of two 1x1 convolutions over every pixel and an attention core.
        float* v = c.A->alloc((size_t)c.B * inner);
        float* yb = c.A->alloc((size_t)c.B * dim);
        float* zb = c.A->alloc((size_t)c.B * dim);
        float* y = c.A->alloc(rows * dim);
        if (!c.dry()) {
            if (launch_linear_rows(ctx, E, Cr.wv, nullptr, v, inner, c.B, E, inner, 0, 0, c.s)) return 1;
            if (launch_linear_rows(v, inner, Cr.wo_raw, Cr.out.bias, yb, dim, c.B, inner, dim, 0, 0, c.s)) return 1;
            if (launch_norm_act(yb, 1, 0, nullptr, Cr.g, nullptr, 0, 1, nullptr, zb, (int64_t)c.B, dim, EPI_NORM, c.s))
                return 1;
            if (launch_broadcast_rows(zb, y, (int)rows, dim, dim, c.s, n)) return 1;
        }
        if (keep_null_rows(y)) return 1;
        c.A->release(v);
        c.A->release(yb);
        c.A->release(zb);
        *out = y;
        return 0;
    }
    float* q = c.A->alloc(rows * inner);
    float* k = c.A->alloc((size_t)c.B * m * inner);
    float* v = c.A->alloc((size_t)c.B * m * inner);
    float* o = c.A->alloc(rows * inner);
    float* y = c.A->alloc(rows * dim);
    if (cross_front(c, Cr, x, H, W, ctx, m, q, k, v, o)) return 1;
    if (run_conv(c, Cr.out, o, nullptr, H, W, y, EPI_NORM, Cr.g, nullptr, nullptr)) return 1;
    if (keep_null_rows(y)) return 1;
    c.A->release(q);
    c.A->release(k);
    c.A->release(v);
    c.A->release(o);
    *out = y;
    return 0;
}

// The conditioning head of the inference walk: time -> (sinusoid -> time_mlp) -> [text concat] -> the [Bt][ss_total] scale /
// shift rows of every ResnetBlock (DD/denoising_diffusion.py:349-361; DD/denoising_diffusion_text_conditional.py:146-152).
// What it allocates stays allocated until cond_release.  unet_forward_impl and dm_unet_cond_forward run this one function.
struct CondHead {
    int Rt = 0, Bt = 0, fdim = 0;  // rows of the sinusoid / time_mlp, rows of ss, width of e0
    float *e0 = nullptr, *e1 = nullptr, *temb = nullptr, *ss = nullptr;
    float *cat = nullptr, *tf0 = nullptr, *t2 = nullptr;  // text concat only
    const float* tfinal = nullptr;                        // what the ResnetBlock.mlp layers see: temb or t2
};
static int cond_forward(dm_unet* u, Arena& A, const int64_t* t_dev, const int64_t* step_times, const SamplerState* step_dev,
                        const float* ctx, int ctx_tokens, int B, hipStream_t s, const int32_t* tmask, const float* tf,
                        int tf_stride, CondHead& h) {
    const dm_unet_cfg& cfg = u->cfg;
    const int td = u->time_dim;
    const bool text_concat = cfg.text_mode == DM_TEXT_CONCAT && ctx != nullptr;
    // the time embedding is one row when the whole batch shares t (samplers), else one row per sample
    const bool shared_t = step_times || (tf && step_dev);
    const int Bt = h.Bt = (shared_t && !text_concat) ? 1 : B;
    const int Rt = h.Rt = shared_t ? 1 : B;  // rows of the sinusoid / time_mlp
    const int lsd = cfg.learned_sinusoidal_dim;  // > 0: cat(t, sin(t w 2 pi), cos(t w 2 pi)) of width lsd + 1 (:96-101)
    const int fdim = h.fdim = lsd > 0 ? lsd + 1 : cfg.dim;
    float* e0 = h.e0 = A.alloc((size_t)Rt * fdim);
    float* e1 = h.e1 = A.alloc((size_t)Rt * td);
    float* temb = h.temb = A.alloc((size_t)B * td);
    float* ss = h.ss = A.alloc((size_t)Bt * u->ss_total);
    if (!A.dry) {
        if (tf) {
            if (launch_sinusoid_ft(tf, tf_stride, step_dev, u->freqs, e0, Rt, (lsd > 0 ? lsd : cfg.dim) / 2, s, lsd > 0)) return 1;
        } else if (launch_sinusoid(t_dev, step_times, step_dev, u->freqs, e0, Rt, (lsd > 0 ? lsd : cfg.dim) / 2, s, lsd > 0)) {
            return 1;
        }
        if (launch_linear_rows(e0, fdim, u->tw1, u->tb1, e1, td, Rt, fdim, td, 0, 2, s)) return 1;
        if (launch_linear_rows(e1, td, u->tw2, u->tb2, temb, td, Rt, td, td, 0, 0, s)) return 1;
    }
    h.tfinal = temb;
    if (text_concat) {
        // t = text_concat_proj(cat(t, text_proj(text_emb)))  (:146-152); ctx is (B, 1, E) or (B, E)
        DM_REQUIRE(ctx_tokens == 1, "text concat conditioning takes one pooled embedding per sample");
        float* cat = h.cat = A.alloc((size_t)B * 2 * td);
        float* tf0 = h.tf0 = A.alloc((size_t)B * td);
        float* t2 = h.t2 = A.alloc((size_t)B * td);
        if (!A.dry) {
            // left half: the time embedding of every row (one broadcast launch when the batch shares t)
            if (Rt == 1) {
                if (launch_broadcast_rows(temb, cat, B, td, 2 * td, s)) return 1;
            } else {
                DM_CHECK_HIP(hipMemcpy2DAsync(cat, 2 * td * sizeof(float), temb, td * sizeof(float),
                                              td * sizeof(float), B, hipMemcpyDeviceToDevice, s));
            }
            if (launch_linear_rows(ctx, cfg.text_emb_dim, u->tp_w0, u->tp_b0, tf0, td, B, cfg.text_emb_dim, td, 0, 2, s))
                return 1;
            if (launch_linear_rows(tf0, td, u->tp_w2, u->tp_b2, cat + td, 2 * td, B, td, td, 0, 0, s)) return 1;
            if (launch_linear_rows(cat, 2 * td, u->tc_w, u->tc_b, t2, td, B, 2 * td, td, 0, 0, s)) return 1;
            // null rows: the raw time embedding (:146-152 skipped when text_emb is None)
            if (tmask && launch_select_rows(t2, temb, Rt == 1 ? 0 : td, tmask, B, td, s)) return 1;
        }
        h.tfinal = t2;
    }
    if (!A.dry) {
        // every ResnetBlock.mlp (SiLU -> Linear) in one launch
        if (launch_linear_rows(h.tfinal, td, u->ss_w, u->ss_b, ss, u->ss_total, Bt, td, u->ss_total, 1, 0, s)) return 1;
    }
    return 0;
}
// everything of the head but ss, which the ResnetBlocks read until the walk ends
static void cond_release(Arena& A, const CondHead& h) {
    if (h.cat) A.release(h.cat);
    if (h.tf0) A.release(h.tf0);
    if (h.t2) A.release(h.t2);
    A.release(h.e0);
    A.release(h.e1);
    A.release(h.temb);
}

// Unet.forward (DD/denoising_diffusion.py:349-390; text hooks DD/denoising_diffusion_text_conditional.py:131-214)
static int unet_forward_impl(dm_unet* u, Arena& A, const float* x_nchw, const int64_t* t_dev,
                             const int64_t* step_times, const SamplerState* step_dev, const float* ctx, int ctx_tokens,
                             float* out_nchw, int B, int H, int W, hipStream_t s, const int32_t* tmask = nullptr,
                             const float* tf = nullptr, int tf_stride = 0) {
    // tf: a REAL-valued time instead of t_dev / step_times (ElucidatedDiffusion's c_noise(sigma)): one value per image, or
    // with step_dev the value tf[step * tf_stride] of the EDM step table for the whole batch
    // tmask: per-image text mask (device int32, B entries, or nullptr = every image as `ctx` says).  Image b is
    // conditioned iff tmask[b] != 0; the others take the model's null path (text_emb = None).  Every row of ctx is
    // read, the masked-out ones included, and their values do not reach the output.
    const dm_unet_cfg& cfg = u->cfg;
    DM_REQUIRE(!tmask || (ctx && cfg.text_mode != DM_TEXT_NONE), "a text mask needs a text-conditional U-Net and a context");
    if (u->kunet) {
        DM_REQUIRE(!ctx, "KarrasUnet has no text condition");
        return kunet_forward_impl(u, A, x_nchw, step_dev, out_nchw, B, H, W, s, tf, tf_stride);
    }
    Ctx c{u, &A, s, B, nullptr, 0};
    const bool text_cross = cfg.text_mode == DM_TEXT_CROSS && ctx != nullptr;
    // one context token: the three CrossAttention layers ignore their image input (run_cross), which makes everything
    // between the last skip connection and the last of them dead code (DM_NO_CROSS1 computes it anyway)
    // (not with a text mask: the null rows need the bottleneck)
    const bool dead_bottleneck = text_cross && ctx_tokens == 1 && !cross1_off() && !tmask;
    CondHead h;
    if (cond_forward(u, A, t_dev, step_times, step_dev, ctx, ctx_tokens, B, s, tmask, tf, tf_stride, h)) return 1;
    float* ss = h.ss;
    c.ss = A.dry ? reinterpret_cast<const float*>(16) : ss;  // non-null marker in dry mode
    c.ss_stride = h.Bt == 1 ? 0 : u->ss_total;

    float* x = A.alloc((size_t)B * H * W * u->init_dim);
    if (run_conv(c, u->init_conv, x_nchw, nullptr, H, W, x, 0, nullptr, nullptr, nullptr, /*in_nchw=*/true)) return 1;
    cond_release(A, h);
    // the layers between init_conv and final_conv, in the order of the node list (unet_graph.inc).  A tensor is released
    // behind the node that reads it last -- Unet.forward's `r = x.clone()` (value 0) behind the last node.
    const UnetGraph& G = u->graphs[dead_bottleneck ? GRAPH_CROSS1 : text_cross ? GRAPH_CROSS : GRAPH_PLAIN];
    std::vector<float*> val(G.n_values(), nullptr);
    val[0] = x;
    for (size_t k = 0; k < G.nodes.size(); ++k) {
        const UnetNode& N = G.nodes[k];
        const float* in0 = N.in0 >= 0 ? val[N.in0] : nullptr;
        const float* in1 = N.in1 >= 0 ? val[N.in1] : nullptr;
        // a sequence is a one-row image at every level
        const int hi = cfg.seq1d ? 1 : H >> N.lin, wi = W >> N.lin, ho = cfg.seq1d ? 1 : H >> N.lout, wo = W >> N.lout;
        switch (N.kind) {
        case NODE_RESNET:
            if (run_resnet(c, N.res(), in0, in1, hi, wi, &val[N.out])) return 1;
            break;
        case NODE_ATTN:
            if (run_attn(c, N.attn(), in0, hi, wi, &val[N.out])) return 1;
            break;
        case NODE_CROSS:
            if (run_cross(c, N.cross(), in0, hi, wi, ctx, ctx_tokens, &val[N.out], tmask)) return 1;
            break;
        case NODE_CONV:
            if (cfg.seq1d) {
                // the Upsample layer runs on the source grid with 2 Cout channels (make_upsample1d): (B, wi, 2 Cout) is
                // (B, wo, Cout); the other resample layers compute their own output length
                val[N.out] = A.alloc((size_t)B * (wo > wi ? wi : wo) * N.conv().Cout);
                if (run_conv(c, N.conv(), in0, nullptr, 1, wi, val[N.out], 0, nullptr, nullptr, nullptr)) return 1;
                break;
            }
            val[N.out] = A.alloc((size_t)B * ho * wo * N.conv().Cout);
            // an Upsample conv sees the (virtually) upsampled tensor: it is given the output size
            if (run_conv(c, N.conv(), in0, nullptr, std::max(hi, ho), std::max(wi, wo), val[N.out], 0, nullptr, nullptr, nullptr)) return 1;
            break;
        }
        for (int v : {N.in0, N.in1})
            if (v >= 0 && G.last_use[v] == (int)k) A.release(val[v]);
    }
    float* fr = val[G.out()];
    if (run_conv(c, u->final_conv, fr, nullptr, H, W, out_nchw, 0, nullptr, nullptr, nullptr, false, /*out_nchw=*/true))
        return 1;
    A.release(fr);
    A.release(ss);
    return 0;
}

static int ensure_workspace(dm_unet* u, size_t bytes) {
    if (bytes <= u->ws_cap) return 0;
    DM_CHECK_HIP(hipDeviceSynchronize());
    u->drop_graph();  // the captured step points into the old arena
    if (u->ws) (void)hipFree(u->ws);
    u->ws = nullptr;
    u->ws_cap = 0;
    void* p = nullptr;
    DM_CHECK_HIP(hipMalloc(&p, bytes));
    u->ws = static_cast<char*>(p);
    u->ws_cap = bytes;
    return 0;
}

static int kunet_image_size(const dm_unet* u);  // dm_kunet.inc
static int check_hw(dm_unet* u, int H, int W) {
    int f = 1 << (u->cfg.n_stages - 1);
    if (u->kunet) {  // KarrasUnet.forward asserts the square image_size it was built for (the attention layers are placed by it)
        DM_REQUIRE(H == W && H == kunet_image_size(u), "KarrasUnet: the input must be image_size x image_size");
        return 0;
    }
    if (u->cfg.seq1d) {
        DM_REQUIRE(H == 1, "a sequence model takes (B, C, L) as H = 1, W = L");
        if (W <= 0 || W % f) {
            set_error("your sequence length (" + std::to_string(W) + ") needs to be divisible by " + std::to_string(f) +
                      ", given the unet");
            return 1;
        }
        return 0;
    }
    if (H % f || W % f) {
        set_error("your input dimensions (" + std::to_string(H) + ", " + std::to_string(W) +
                  ") need to be divisible by " + std::to_string(f) + ", given the unet");
        return 1;
    }
    return 0;
}

}  // namespace dm

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

const char* dm_last_error(void) { return g_err.c_str(); }
int dm_abi_version(void) { return 9; }

int dm_unet_create(const dm_unet_cfg* cfg, int device, dm_unet** out) {
    DM_REQUIRE(cfg && out, "null argument");
    DM_REQUIRE(cfg->n_stages >= 1 && cfg->n_stages <= DM_MAX_STAGES, "n_stages out of range");
    DM_REQUIRE(cfg->dim > 0 && cfg->dim % 2 == 0, "dim must be positive and even");
    DM_REQUIRE(cfg->attn_dim_head == 32 || cfg->attn_dim_head == 64,
               "attn_dim_head: the HIP attention kernels support head widths 32 and 64");
    DM_REQUIRE(cfg->attn_heads >= 1 && cfg->attn_heads <= 16, "attn_heads out of range");
    for (int i = 0; i < cfg->n_stages; ++i)
        DM_REQUIRE(cfg->attn_heads_stage[i] >= 0 && cfg->attn_heads_stage[i] <= 16, "attn_heads of a stage out of range");
    int ndev = 0;
    DM_CHECK_HIP(hipGetDeviceCount(&ndev));
    DM_REQUIRE(device >= 0 && device < ndev, "no such HIP device");
    DM_CHECK_HIP(hipSetDevice(device));
    auto u = std::make_unique<dm_unet>();
    u->cfg = *cfg;
    u->device = device;
    u->init_dim = cfg->init_dim ? cfg->init_dim : cfg->dim;
    u->out_dim = cfg->out_dim ? cfg->out_dim : cfg->channels;
    u->time_dim = cfg->dim * 4;
    u->heads = cfg->attn_heads;
    u->dh = cfg->attn_dim_head;
    u->dims.push_back(u->init_dim);
    for (int i = 0; i < cfg->n_stages; ++i) u->dims.push_back(cfg->dim * cfg->dim_mults[i]);
    dm_unet* p = u.get();
    const int n = cfg->n_stages, td = u->time_dim;
    if (cfg->seq1d) {
        DM_REQUIRE(cfg->text_mode == DM_TEXT_NONE, "the sequence model (seq1d) has no text condition");
        expect_unet1d(p);
        *out = u.release();
        return 0;
    }
    expect(p, "init_conv.weight", {u->init_dim, cfg->input_channels, 7, 7});
    expect(p, "init_conv.bias", {u->init_dim});
    if (cfg->learned_sinusoidal_dim > 0) expect(p, "time_mlp.0.weights", {cfg->learned_sinusoidal_dim / 2});
    expect(p, "time_mlp.1.weight", {td, cfg->learned_sinusoidal_dim > 0 ? cfg->learned_sinusoidal_dim + 1 : cfg->dim});
    expect(p, "time_mlp.1.bias", {td});
    expect(p, "time_mlp.3.weight", {td, td});
    expect(p, "time_mlp.3.bias", {td});
    for (int i = 0; i < n; ++i) {
        int din = u->dims[i], dout = u->dims[i + 1];
        std::string q = idx("downs", i);
        expect_resnet(p, q + ".0", din, din);
        expect_resnet(p, q + ".1", din, din);
        expect_attn(p, q + ".2", din, cfg->full_attn[i] != 0, stage_heads(*cfg, i));
        const bool last = i == n - 1;
        expect(p, resample_param(q, last, "weight"), last ? std::vector<int64_t>{dout, din, 3, 3} : std::vector<int64_t>{dout, din * 4, 1, 1});
        expect(p, resample_param(q, last, "bias"), {dout});
    }
    for (int j = 0; j < n; ++j) {
        int din = u->dims[n - 1 - j], dout = u->dims[n - j];
        std::string q = idx("ups", j);
        expect_resnet(p, q + ".0", dout + din, dout);
        expect_resnet(p, q + ".1", dout + din, dout);
        expect_attn(p, q + ".2", dout, cfg->full_attn[n - 1 - j] != 0, stage_heads(*cfg, n - 1 - j));
        expect(p, resample_param(q, j == n - 1, "weight"), {din, dout, 3, 3});
        expect(p, resample_param(q, j == n - 1, "bias"), {din});
    }
    int mid = u->dims.back();
    expect_resnet(p, "mid_block1", mid, mid);
    expect_attn(p, "mid_attn", mid, true, stage_heads(*cfg, n - 1));
    expect_resnet(p, "mid_block2", mid, mid);
    expect_resnet(p, "final_res_block", 2 * u->init_dim, u->init_dim);
    expect(p, "final_conv.weight", {u->out_dim, u->init_dim, 1, 1});
    expect(p, "final_conv.bias", {u->out_dim});
    if (cfg->text_mode == DM_TEXT_CONCAT) {
        expect(p, "text_proj.0.weight", {td, cfg->text_emb_dim});
        expect(p, "text_proj.0.bias", {td});
        expect(p, "text_proj.2.weight", {td, td});
        expect(p, "text_proj.2.bias", {td});
        expect(p, "text_concat_proj.weight", {td, 2 * td});
        expect(p, "text_concat_proj.bias", {td});
    } else if (cfg->text_mode == DM_TEXT_CROSS) {
        expect_cross(p, "cross_attn", mid);
        expect_cross(p, "cross_attn_down", mid);
        expect_cross(p, "cross_attn_up", mid);
    }
    *out = u.release();
    return 0;
}

void dm_unet_destroy(dm_unet* u) {
    if (!u) return;
    (void)hipSetDevice(u->device);
    if (u->train) free_train(u);
    kunet_free(u);
    u->drop_graph();
    if (u->cap_stream) (void)hipStreamDestroy(u->cap_stream);
    if (u->done_ev) (void)hipEventDestroy(u->done_ev);
    if (u->ws) (void)hipFree(u->ws);
    if (u->state_dev) (void)hipFree(u->state_dev);
    if (u->times_dev) (void)hipFree(u->times_dev);
    if (u->coefs_dev) (void)hipFree(u->coefs_dev);
    if (u->edm_tab_dev) (void)hipFree(u->edm_tab_dev);
    delete u;
}

int dm_unet_set_param(dm_unet* u, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    DM_REQUIRE(u && name && data_host && shape, "null argument");
    DM_REQUIRE(!u->finalized, "set_param after finalize");
    auto it = u->params.find(name);
    if (it == u->params.end()) {
        set_error(std::string("unexpected parameter: ") + name);
        return 1;
    }
    HostTensor& t = it->second;
    bool ok = (int)t.shape.size() == ndim;
    for (int i = 0; ok && i < ndim; ++i) ok = t.shape[i] == shape[i];
    if (!ok) {
        set_error(std::string("shape mismatch for ") + name);
        return 1;
    }
    t.data.assign(data_host, data_host + t.numel());
    t.set = true;
    return 0;
}

int dm_unet_missing_params(dm_unet* u) {
    if (!u) return -1;
    int missing = 0;
    std::string first;
    for (auto& kv : u->params)
        if (!kv.second.set) {
            if (!missing) first = kv.first;
            ++missing;
        }
    if (missing) set_error("missing parameter: " + first);
    return missing;
}

/* read back the handle's host copy of one parameter (what dm_unet_set_param / dm_unet_update_param stored; after
 * dm_unet_train_sync: the trained values) */
int dm_unet_get_param_host(dm_unet* u, const char* name, float* out_host, int64_t n) {
    DM_REQUIRE(u && name && out_host, "null argument");
    auto it = u->params.find(name);
    if (it == u->params.end() || !it->second.set) {
        set_error(std::string("unknown or unset parameter: ") + name);
        return 1;
    }
    DM_REQUIRE((int64_t)it->second.numel() == n, "dm_unet_get_param_host: element count mismatch");
    std::memcpy(out_host, it->second.data.data(), (size_t)n * sizeof(float));
    return 0;
}

int dm_unet_finalize(dm_unet* u) {
    DM_REQUIRE(u, "null handle");
    DM_REQUIRE(!u->finalized, "already finalized");
    if (dm_unet_missing_params(u) != 0) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    u->own.rec = &u->pack_ops;
    if (build_all(u)) return 1;
    // the host copies stay: dm_unet_update_param / dm_unet_refresh re-pack from them
    u->finalized = true;
    return 0;
}

int dm_unet_update_param(dm_unet* u, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    DM_REQUIRE(u && name && data_host && shape, "null argument");
    DM_REQUIRE(u->finalized, "dm_unet_update_param before dm_unet_finalize (use dm_unet_set_param)");
    // the device-resident parameters have moved on (dm_unet_optimizer_step): bring the host copies up to date first, so
    // that "unchanged" below compares with the current values and a partial update does not resurrect stale ones
    if (u->infer_stale && dm_unet_train_sync(u)) return 1;
    auto it = u->params.find(name);
    if (it == u->params.end()) {
        set_error(std::string("unexpected parameter: ") + name);
        return 1;
    }
    HostTensor& t = it->second;
    bool ok = (int)t.shape.size() == ndim;
    for (int i = 0; ok && i < ndim; ++i) ok = t.shape[i] == shape[i];
    if (!ok) {
        set_error(std::string("shape mismatch for ") + name);
        return 1;
    }
    if (std::memcmp(t.data.data(), data_host, t.numel() * sizeof(float)) == 0) return 0;  // unchanged
    t.data.assign(data_host, data_host + t.numel());
    t.dirty = true;
    return 0;
}

int dm_unet_refresh(dm_unet* u) {
    DM_REQUIRE(u, "null handle");
    DM_REQUIRE(u->finalized, "dm_unet_refresh before dm_unet_finalize");
    bool any = u->poisoned;
    for (auto& kv : u->params) any = any || kv.second.dirty;
    if (!any) return 0;
    DM_CHECK_HIP(hipSetDevice(u->device));
    DM_CHECK_HIP(hipDeviceSynchronize());  // no kernel may be reading the buffers that are rewritten
    u->own.refreshing = true;
    u->own.cursor = 0;
    int rc = build_all(u);
    if (!rc && u->own.cursor != u->own.ptrs.size()) {
        set_error("refresh: not every weight buffer was visited");
        rc = 1;
    }
    u->own.refreshing = false;
    if (rc) {
        // Some buffers hold new values, some old ones.  The dirty flags stay set so that a retry re-packs everything that
        // changed, the cached step graph is dropped, and the handle refuses to run until a refresh has succeeded.
        u->drop_graph();
        u->poisoned = true;
        return rc;
    }
    // the input-gradient convolutions are packed from the same parameters; a device-resident master copy follows the host
    if (u->train && (build_train(u) || upload_master_if_resident(u))) {
        u->poisoned = true;
        return 1;
    }
    u->poisoned = false;
    for (auto& kv : u->params) kv.second.dirty = false;
    return 0;
}

int dm_unet_graph_captures(dm_unet* u) { return u ? u->graph_captures : -1; }
int64_t dm_unet_workspace_bytes(dm_unet* u) { return u ? (int64_t)u->ws_cap : -1; }

int dm_unet_forward(dm_unet* u, const float* x, const int64_t* time, const float* ctx, int ctx_tokens, float* out,
                    int B, int H, int W, void* stream) {
    DM_REQUIRE(u && x && time && out, "null argument");
    DM_REQUIRE(u->finalized, "dm_unet_finalize has not been called");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    DM_REQUIRE(!u->infer_stale, "parameters were updated on the device (dm_unet_optimizer_step): call dm_unet_train_sync "
                                "before sampling from this handle");
    DM_REQUIRE(!u->kunet, "a KarrasUnet handle takes a real-valued time: dm_unet_forward_ft and dm_sample_edm");
    DM_REQUIRE(B > 0, "empty batch");
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Arena dry;
    dry.dry = true;
    if (unet_forward_impl(u, dry, x, time, nullptr, nullptr, ctx, ctx_tokens, out, B, H, W, s)) return 1;
    if (ensure_workspace(u, dry.off)) return 1;
    Arena A;
    A.base = u->ws;
    A.cap = u->ws_cap;
    if (u->order_after_previous(s)) return 1;
    if (unet_forward_impl(u, A, x, time, nullptr, nullptr, ctx, ctx_tokens, out, B, H, W, s)) return 1;
    return u->mark_done(s);
}

int dm_unet_forward_masked(dm_unet* u, const float* x, const int64_t* time, const float* ctx, int ctx_tokens,
                           const int32_t* text_mask, float* out, int B, int H, int W, void* stream) {
    DM_REQUIRE(u && x && time && ctx && text_mask && out, "null argument");
    DM_REQUIRE(u->cfg.text_mode != DM_TEXT_NONE, "dm_unet_forward_masked needs a text-conditional U-Net");
    DM_REQUIRE(u->finalized, "dm_unet_finalize has not been called");
    DM_REQUIRE(!u->poisoned, "the last dm_unet_refresh failed: refresh again before running the model");
    DM_REQUIRE(!u->infer_stale, "parameters were updated on the device (dm_unet_optimizer_step): call dm_unet_train_sync "
                                "before sampling from this handle");
    DM_REQUIRE(B > 0 && ctx_tokens > 0, "empty batch or context");
    if (check_hw(u, H, W)) return 1;
    DM_CHECK_HIP(hipSetDevice(u->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Arena dry;
    dry.dry = true;
    if (unet_forward_impl(u, dry, x, time, nullptr, nullptr, ctx, ctx_tokens, out, B, H, W, s, text_mask)) return 1;
    if (ensure_workspace(u, dry.off)) return 1;
    Arena A;
    A.base = u->ws;
    A.cap = u->ws_cap;
    if (u->order_after_previous(s)) return 1;
    if (unet_forward_impl(u, A, x, time, nullptr, nullptr, ctx, ctx_tokens, out, B, H, W, s, text_mask)) return 1;
    return u->mark_done(s);
}

int dm_randn(float* out, int64_t n, uint64_t seed, uint64_t draw, uint64_t element_offset, void* stream) {
    DM_REQUIRE(out && n >= 0, "bad argument");
    return launch_randn(out, n, seed, draw, element_offset, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// single-operator entry points (dm_op_*) and the VAE decoder share the helpers above
#include "dm_op_scaffold.inc"
#include "dm_ops.inc"
#include "dm_kunet.inc"
#include "dm_vae.inc"
#include "dm_consumer.inc"
#include "dm_train.inc"
#include "dm_train_ops.inc"
#include "dm_sampler.inc"
#include "dm_edm.inc"
#include "dm_ct.inc"
#include "dm_repaint.inc"
#include "dm_learned.inc"
#include "dm_weighted.inc"
#include "dm_cguide.inc"
#include "dm_bpd.inc"
