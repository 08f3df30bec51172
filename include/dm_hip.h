/*
 * dm_hip.h -- C ABI of the MI355X-native sampling path (libdm_hip.so).
 *
 * The reference (lbarseghyan/diffusion-models) has no FFI or plugin interface: its
 * boundary is a Python method surface on nn.Module subclasses.  Each entry point
 * below names the reference method it stands behind (paths relative to the
 * reference checkout; DD = denoising-diffusion-pytorch/denoising_diffusion,
 * LD = latent-diffusion/ldm).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from dm_last_error() (thread-local).  Nothing throws across the ABI.
 *   - `const float*` tensor arguments are DEVICE pointers, contiguous fp32, NCHW at
 *     this boundary (the reference's layout), unless the name says `_host`.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - a handle is bound to one device and is not thread-safe.
 *   - PyTorch (or any caller) owns inputs and outputs; the library owns only its
 *     repacked weights and a workspace that grows outside graph capture.
 */
#ifndef DM_HIP_H
#define DM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM_MAX_STAGES 8

/* text_mode */
#define DM_TEXT_NONE 0
#define DM_TEXT_CONCAT 1 /* DD/denoising_diffusion_text_conditional.py:108-115,146-152 */
#define DM_TEXT_CROSS 2  /* DD/denoising_diffusion_text_conditional.py:120-125,173-198 */

/* Constructor arguments of the reference Unet that fix shapes
 * (DD/denoising_diffusion.py:234-252; text variant
 * DD/denoising_diffusion_text_conditional.py:97). */
typedef struct dm_unet_cfg {
    int32_t dim;
    int32_t init_dim;       /* 0 = dim */
    int32_t out_dim;        /* 0 = channels */
    int32_t channels;       /* image / latent channels the model predicts */
    int32_t input_channels; /* channels init_conv sees (self-cond / image-cond widen it) */
    int32_t n_stages;
    int32_t dim_mults[DM_MAX_STAGES];
    int32_t full_attn[DM_MAX_STAGES];
    int32_t attn_heads;
    int32_t attn_dim_head;
    int32_t text_mode;
    int32_t text_emb_dim;
    float sinusoidal_theta;
    int32_t learned_sinusoidal_dim; /* 0: SinusoidalPosEmb(dim, theta); > 0: RandomOrLearnedSinusoidalPosEmb of that
                                       dimension (DD/denoising_diffusion.py:86-101, parameter time_mlp.0.weights) --
                                       dm_unet_forward only: DenoisingDiffusion refuses such a U-Net (:456-457) */
    int32_t attn_heads_stage[DM_MAX_STAGES]; /* Unet(attn_heads = (h0, h1, ..)): heads of stage i's attention (:294, :310,
                                                :327; mid_attn takes the last stage's, :324); 0 = attn_heads */
    int32_t seq1d; /* 0: the image U-Net above.  != 0: Unet1D (DD/denoising_diffusion_1d.py:219-349), the model of sequences
                      (B, C, L): every entry that takes H, W is called with H = 1, W = L; the parameters have the 1D
                      module's names and rank-3 shapes (conv weights (Cout, Cin, K), gains (1, C, 1), no mem_kv, the
                      attention bodies under `.fn.fn`); every stage's attention is LinearAttention(heads 4, dim_head 32)
                      and mid_attn is Attention(attn_heads, attn_dim_head) (:285, :291, :300), so full_attn and
                      attn_heads_stage are ignored; text_mode must be DM_TEXT_NONE; inference and sampling only
                      (dm_unet_train_enable* refuse the handle) */
} dm_unet_cfg;

typedef struct dm_unet dm_unet;

const char* dm_last_error(void);
/* ABI version of this header; bump on any signature change. */
int dm_abi_version(void);

/* ---- U-Net (replaces DD/denoising_diffusion.py:233-390 `Unet`) -------------------- */

int dm_unet_create(const dm_unet_cfg* cfg, int device, dm_unet** out);
void dm_unet_destroy(dm_unet* u);

/* One call per state_dict() entry of the reference Unet (names without the
 * `model.` prefix, e.g. "downs.0.0.block1.proj.weight"); data is a HOST pointer
 * to contiguous fp32 in the reference's own layout (OIHW conv weights, [out,in]
 * linear weights).  Shapes are checked against the configuration. */
int dm_unet_set_param(dm_unet* u, const char* name, const float* data_host, const int64_t* shape, int ndim);
/* number of parameters still missing (0 = complete) */
int dm_unet_missing_params(dm_unet* u);
/* read back the handle's host copy of one parameter (n = its element count): `Unet.state_dict()` / `.parameters()` of a
 * handle that is not in training mode (a training handle reads its device-resident state: dm_unet_get_param) */
int dm_unet_get_param_host(dm_unet* u, const char* name, float* out_host, int64_t n);
/* repack weights into kernel layouts and upload; must follow the last set_param */
int dm_unet_finalize(dm_unet* u);

/* In-place weight refresh for the caller of record: Trainer.train samples from `self.ema.ema_model` after every EMA
 * update (DD/denoising_diffusion.py:1190,1198,1216), i.e. the same architecture with new values each time.
 * dm_unet_update_param replaces the host copy of one parameter of a FINALIZED handle (same name / shape rules as
 * dm_unet_set_param; unchanged values are detected and cost nothing); dm_unet_refresh then re-packs the layers whose
 * parameters changed into the SAME device buffers (no reallocation: workspace, captured step graph and every device
 * pointer stay valid).  The call synchronises the device. */
int dm_unet_update_param(dm_unet* u, const char* name, const float* data_host, const int64_t* shape, int ndim);
int dm_unet_refresh(dm_unet* u);
/* how many times a denoise-step graph has been captured on this handle (diagnostics / tests: one per shape) */
int dm_unet_graph_captures(dm_unet* u);
/* bytes of the activation workspace the handle currently owns (grown by the largest call so far; activations are
 * released to it as soon as their last consumer is enqueued, so a B=256 step works in a few hundred MB) */
int64_t dm_unet_workspace_bytes(dm_unet* u);

/* Unet.forward(x, time, x_self_cond=None) DD/denoising_diffusion.py:349-390 and the
 * text variant forward(x, time, text_emb) DD/denoising_diffusion_text_conditional.py:131-214.
 *   x      (B, input_channels, H, W)   time (B,) int64 device   ctx (B, ctx_tokens, text_emb_dim) or NULL
 *   out    (B, out_dim, H, W)
 * H and W must be divisible by 2^(n_stages-1) (assert at :350). */
int dm_unet_forward(dm_unet* u, const float* x, const int64_t* time, const float* ctx, int ctx_tokens,
                    float* out, int B, int H, int W, void* stream);

/* The text-conditional forward with a per-image text mask: image i is conditioned on ctx row i iff text_mask[i] != 0,
 * and takes the null path of forward(x, time, text_emb=None) otherwise (DD/denoising_diffusion_text_conditional.py:
 * 146-152 concat, :173/:183/:194 cross).  One batch holds both kinds, so classifier-free guidance runs its conditioned
 * and null predictions as one forward (DD/classifier_free_guidance.py:350-354).
 *   text_mask  (B,) int32 device   ctx (B, ctx_tokens, text_emb_dim), every row initialised (the masked-out rows are
 *              read, their values do not reach the output)
 * Needs a handle with text_mode != DM_TEXT_NONE. */
int dm_unet_forward_masked(dm_unet* u, const float* x, const int64_t* time, const float* ctx, int ctx_tokens,
                           const int32_t* text_mask, float* out, int B, int H, int W, void* stream);

/* ---- samplers (replace DenoisingDiffusion.p_sample_loop / ddim_sample,
 *      DD/denoising_diffusion.py:647-664 and :666-708) ------------------------------------
 *
 * The per-step scalar coefficients are computed by the HOST exactly as the reference
 * computes them (fp32 tensor arithmetic on the schedule buffers) and passed in:
 *   DDPM step i (t = times[i]):   c[0]=sqrt_recip_alphas_cumprod[t]  c[1]=sqrt_recipm1_alphas_cumprod[t]
 *                                 c[2]=posterior_mean_coef1[t]       c[3]=posterior_mean_coef2[t]
 *                                 c[4]=exp(0.5*posterior_log_variance_clipped[t])   c[5]= (t>0) ? 1 : 0
 *   DDIM step i (t, t_next):      c[0], c[1] as above  c[2]=sqrt(alpha_next)  c[3]=c  c[4]=sigma
 *                                 c[5]= (t_next<0) ? 0 : 1   (0: img = x_start, :686-689)
 *   DPM-Solver++ step i (t, t_next) on the DDIM time grid (arXiv 2211.01095, Algorithm 2; not in the reference), with
 *   alpha = sqrt(alphas_cumprod), sigma = sqrt(1 - alphas_cumprod), lambda = log(alpha / sigma), h = lambda_next - lambda_t,
 *   every term in float64 and rounded to fp32 once:
 *                                 c[0], c[1], c[6], c[7] as for DDIM  c[2]=sigma_next/sigma_t  c[3]=-alpha_next*expm1(-h)
 *                                 c[4]=h/(2 h_last) at order 2 (0 at order 1, at the first and at the last step)
 *                                 c[5]= (t_next<0) ? 0 : 1   (0: img = x_start, as DDIM)
 *     x_next = c[2] x + c[3] (x0 + c[4] (x0 - x0_prev)),  x0 the clamped x_start of the step; no noise after x_T
 * coefs_host has n_steps rows of DM_COEFS floats.
 *
 *   x_T        (B,C,H,W) start noise (draw #0 of the reference)
 *   noise      NULL -> device Philox noise from `seed`; else (n_steps, B,C,H,W) injected noise,
 *              row i used by step i (rows of steps that take no noise are ignored)
 *   sample_offset  index of this call's first sample in the GLOBAL batch (0 for an unsharded call).  Philox
 *              counters are the global element index, (sample_offset*C*H*W + e) / 4, so a batch sharded over ranks
 *               draws exactly the noise the unsharded batch draws: cat(shards) == whole, bit for bit.
 *              Generate x_T with dm_randn(..., draw 0, element_offset = sample_offset*C*H*W) for the same property.
 *   out        (B,C,H,W); (x+1)/2 applied when unnormalize != 0 (:663,:707)
 *   all_steps  NULL, or (n_steps+1, B,C,H,W) receiving x_T and every iterate
 *              (return_all_timesteps; the caller permutes to (B, n_steps+1, ...))
 *   use_graph  replay one denoise step as a hipGraph n_steps times.  The instantiated graph is cached on the handle
 *              and reused by later calls of the same (kind, B, H, W, ctx_tokens, cond_channels); seed, offset, step
 *              tables, x_T, ctx and cond are device data or copied into handle-owned buffers, not captured arguments.
 */
#define DM_COEFS 8
#define DM_SAMPLER_DDPM 0
#define DM_SAMPLER_DDIM 1
#define DM_SAMPLER_DPMPP 2
/* The DDIM loop of DenoisingDiffusion1D (DD/denoising_diffusion_1d.py:562-596) calls model_predictions(img, t, self_cond,
 * clip_x_start = clip_denoised) without rederive_pred_noise, unlike the image class (DD/denoising_diffusion.py:684):
 *   DM_DDIM_NO_CLAMP   x_start is not clamped to [-1, 1] (clip_denoised = False)
 *   DM_DDIM_RAW_NOISE  under DM_OBJ_PRED_NOISE the update's pred_noise is the U-Net output itself, not re-derived from the
 *                      (clamped) x_start; the other objectives derive it from x_start either way (:515-524) */
#define DM_DDIM_NO_CLAMP 1
#define DM_DDIM_RAW_NOISE 2
/* what the U-Net output means (`objective` of DenoisingDiffusion.__init__, DD/denoising_diffusion.py:443; branches of
 * model_predictions :607-624).  pred_v reads c[6]=sqrt_alphas_cumprod[t], c[7]=sqrt_one_minus_alphas_cumprod[t]
 * (predict_start_from_v :588-592) from the step table. */
#define DM_OBJ_PRED_NOISE 0
#define DM_OBJ_PRED_X0 1
#define DM_OBJ_PRED_V 2

int dm_sample(dm_unet* u, int kind, int n_steps, const int64_t* times_host, const float* coefs_host,
              const float* x_T, const float* noise, uint64_t seed, uint64_t sample_offset, const float* ctx,
              int ctx_tokens, float* out, float* all_steps, int B, int H, int W, int unnormalize, int use_graph,
              void* stream);

/* The same loop for the image-conditional variant (replaces ImageConditionalDenoisingDiffusion.p_sample_loop /
 * ddim_sample, DD/denoising_diffusion_image_conditional.py:156-224; its Unet.forward concatenates `cond` behind x in
 * front of init_conv, :51-55).  cond is (B, cond_channels, H, W) fp32 on the device, constant over the loop; the
 * handle must have input_channels == channels + cond_channels. */
int dm_sample_cond(dm_unet* u, int kind, int n_steps, const int64_t* times_host, const float* coefs_host,
                   const float* x_T, const float* noise, uint64_t seed, uint64_t sample_offset, const float* ctx,
                   int ctx_tokens, const float* cond, int cond_channels, float* out, float* all_steps, int B, int H,
                   int W, int unnormalize, int use_graph, void* stream);

/* The general form of the two calls above: every option of the loop in one struct (zero-initialise it; unused fields
 * stay 0 / NULL).  objective: DM_OBJ_*.  self_condition != 0: the handle was built with input_channels == 2*channels and
 * every step feeds the U-Net [x_start of the previous step | x] (zeros at the first step), as p_sample_loop / ddim_sample
 * do when model.self_condition is set (DD/denoising_diffusion.py:352-354,:657,:683); not combined with cond. */
typedef struct dm_sample_args {
    int32_t kind;           /* DM_SAMPLER_* */
    int32_t objective;      /* DM_OBJ_* */
    int32_t self_condition;
    int32_t n_steps;
    const int64_t* times_host;
    const float* coefs_host;
    const float* x_T;
    const float* noise;
    uint64_t seed;
    uint64_t sample_offset;
    const float* ctx;
    int32_t ctx_tokens;
    int32_t cond_channels;
    const float* cond;
    float* out;
    float* all_steps;
    int32_t B, H, W;
    int32_t unnormalize;
    int32_t use_graph;
    int32_t ddim_flags; /* DM_DDIM_*; 0 (the zero-initialised struct): the image classes' loop.  kind DM_SAMPLER_DDIM only */
    void* stream;
    /* classifier-free guidance (Unet.forward_with_cond_scale, DD/classifier_free_guidance.py:339-369); cfg == 0 (the
     * zero-initialised struct): no guidance, the other cfg_* fields are ignored.  cfg != 0: every step runs the U-Net
     * once on 2B images, B conditioned on ctx and B null ones, and the update reads the guided output
     *   scaled = cond + update * (cfg_scale - 1),  update = cond - null, its component parallel to cond removed (per
     *   image, in fp64) and cfg_keep_parallel_frac of it added back when cfg_remove_parallel == 1;
     *   rescaled_phi != 0: out = phi * scaled * std(cond) / std(scaled) + (1 - phi) * scaled (unbiased std per image).
     * Needs a text-conditional handle and ctx; not combined with self_condition or cond.  The four values are device
     * data of the captured step graph: a new cfg_scale reuses the graph of the same shape. */
    int32_t cfg;
    float cfg_scale;
    float cfg_rescaled_phi;
    float cfg_keep_parallel_frac;
    int32_t cfg_remove_parallel;
    int32_t cfg_reserved_;
} dm_sample_args;
int dm_sample_ex(dm_unet* u, const dm_sample_args* args);

/* Dynamic thresholding of x_start (Imagen, arXiv 2205.11487, section 2.3) in the loop of dm_sample_ex, every kind:
 *   s_b = max(1, quantile(|x_start_raw| over (C, H, W) of image b, dyn_percentile)),
 *   x_start = clamp(x_start_raw, -s_b, s_b) / s_b   in place of clamp(x_start_raw, -1, 1),
 * with torch.quantile's linear interpolation; where the quantile is <= 1 the step is bit-for-bit the static clamp.
 * x_start is what the update, DDIM's re-derived pred_noise, the DPM-Solver++ history and the self-conditioning feedback
 * read.  One more kernel per step (an exact radix select, one workgroup per image) between the U-Net and the update.
 * dyn_threshold == 0 (the zero-initialised struct, or dyn == NULL): dm_sample_ex as it is.  dyn_threshold != 0 needs
 * dyn_percentile in (0, 1]; refused on a seq1d handle and with ddim_flags != 0.  The rank and the interpolation weight
 * are device data of the captured step graph: a new percentile reuses the graph of the same shape.
 * These fields ride in a struct of their own behind dm_sample_args, whose layout stays as it is. */
typedef struct dm_sample_dyn_args {
    int32_t dyn_threshold;
    float dyn_percentile;
} dm_sample_dyn_args;
int dm_sample_ex_dyn(dm_unet* u, const dm_sample_args* args, const dm_sample_dyn_args* dyn);

/* N(0,1) noise from the library's Philox4x32-10 stream (what dm_sample uses when noise == NULL);
 * element e of the tensor of draw `draw` uses counter ((element_offset + e)/4, draw) under key `seed`
 * (element_offset % 4 == 0; draw 0 = x_T, draw i+1 = the noise of loop step i). */
int dm_randn(float* out, int64_t n, uint64_t seed, uint64_t draw, uint64_t element_offset, void* stream);

/* ---- VAE decode (replaces VQModel.decode, LD/models/autoencoder.py:113-116 ->
 *      Decoder.forward LD/modules/diffusionmodules/model.py:552-585) ----------------------- */
typedef struct dm_decoder_cfg {
    int32_t ch;
    int32_t out_ch;
    int32_t n_levels;
    int32_t ch_mult[DM_MAX_STAGES];
    int32_t num_res_blocks;
    int32_t n_attn_res;
    int32_t attn_resolutions[DM_MAX_STAGES];
    int32_t resolution;
    int32_t z_channels;
    int32_t embed_dim;
} dm_decoder_cfg;

typedef struct dm_decoder dm_decoder;
int dm_decoder_create(const dm_decoder_cfg* cfg, int device, dm_decoder** out);
void dm_decoder_destroy(dm_decoder* d);
int dm_decoder_set_param(dm_decoder* d, const char* name, const float* data_host, const int64_t* shape, int ndim);
int dm_decoder_missing_params(dm_decoder* d);
int dm_decoder_finalize(dm_decoder* d);
/* z (B, embed_dim, h, w) -> out (B, out_ch, h*2^(n_levels-1), w*2^(n_levels-1)) */
int dm_decoder_forward(dm_decoder* d, const float* z, float* out, int B, int h, int w, void* stream);

/* ---- VAE encode (replaces VQModel.encode, LD/models/autoencoder.py:102-106 -> Encoder.forward
 *      LD/modules/diffusionmodules/model.py:451-476 -> quant_conv -> VectorQuantizer2 of taming-transformers):
 *      the condition image of ImageConditionalLatentDiffusion (LD/models/latent_diffusion_image_conditional.py:55-66)
 * Parameter names: VQModel.state_dict() entries "encoder.*", "quant_conv.*", "quantize.embedding.weight". ---- */
typedef struct dm_encoder_cfg {
    int32_t ch;
    int32_t in_channels;
    int32_t n_levels;
    int32_t ch_mult[DM_MAX_STAGES];
    int32_t num_res_blocks;
    int32_t n_attn_res;
    int32_t attn_resolutions[DM_MAX_STAGES];
    int32_t resolution;
    int32_t z_channels;
    int32_t embed_dim;
    int32_t n_embed;
    int32_t double_z;
} dm_encoder_cfg;
typedef struct dm_encoder dm_encoder;
int dm_encoder_create(const dm_encoder_cfg* cfg, int device, dm_encoder** out);
void dm_encoder_destroy(dm_encoder* e);
int dm_encoder_set_param(dm_encoder* e, const char* name, const float* data_host, const int64_t* shape, int ndim);
int dm_encoder_missing_params(dm_encoder* e);
int dm_encoder_finalize(dm_encoder* e);
/* x (B, in_channels, H, W) device fp32 -> zq (B, embed_dim, H/f, W/f) = z + (nearest code - z); optional outputs:
 * pre_quant (same shape, the quant_conv output = VQModel.encode_to_prequant) and indices (B*h*w int32 code ids).
 * zq may be NULL when only pre_quant is wanted. */
int dm_encoder_forward(dm_encoder* e, const float* x, float* zq, float* pre_quant, int32_t* indices, int B, int H, int W,
                       void* stream);
/* The KL first stage (AutoencoderKL, LD/models/autoencoder.py:339-396) on the same handle type: a cfg with n_embed == 0 has
 * no codebook.  It needs double_z != 0, takes "quant_conv.weight" as (2 * embed_dim, 2 * z_channels, 1, 1) (:356) and no
 * "quantize.embedding.weight"; dm_encoder_forward, dm_encoder_quantize and dm_encoder_embed_code refuse such a handle, and
 * dm_encoder_forward_kl refuses one with a codebook.
 * x (B, in_channels, H, W) -> Encoder -> quant_conv -> the posterior of DiagonalGaussianDistribution
 * (LD/modules/distributions/distributions.py:24-62), in one call on the handle's workspace: no host synchronisation, and no
 * allocation after the first call of a shape.  Outputs, each optional (NULL: not written), at least one:
 *   moments_nchw (B, 2 * embed_dim, h, w)  the quant_conv output, log-variance unclamped (`parameters`)
 *   z            (B, embed_dim, h, w)      sample != 0: mean + exp(0.5 * clamp(logvar, -30, 20)) * eps;  0: the mean (mode)
 *   kl           (B)                       0.5 * sum(mean^2 + exp(logvar) - 1 - logvar) over (embed_dim, h, w), logvar clamped
 * eps (B, embed_dim, h, w) injects the noise; eps == NULL draws it from the library's Philox stream, element e of z using
 * counter ((element_offset + e) / 4, draw) under key seed, i.e. the values of dm_randn for that shape (needs
 * embed_dim * h * w % 4 == 0 and element_offset % 4 == 0).  kl is a fixed-order sum: two calls give the same bits. */
int dm_encoder_forward_kl(dm_encoder* e, const float* x, float* moments_nchw, float* z, float* kl, const float* eps,
                          uint64_t seed, uint64_t draw, uint64_t element_offset, int sample, int B, int H, int W, void* stream);
/* VectorQuantizer on a pre-quantisation latent held in NCHW (VQModelInterface.decode, autoencoder.py:329-336): h_nchw
 * (B, embed_dim, h, w) -> zq (same shape) = h + (nearest code - h) and indices (B*h*w, may be NULL), the search of
 * dm_encoder_forward on the handle's device codebook. */
int dm_encoder_quantize(dm_encoder* e, const float* h_nchw, float* zq, int32_t* indices, int B, int h, int w, void* stream);
/* quantize.embed_code + the "b h w c -> b c h w" permute of VQModel.decode_code (autoencoder.py:118-121): indices (B*h*w)
 * int64 -> out (B, embed_dim, h, w).  Synchronises the stream: an index outside [0, n_embed) is an error (it is never used as
 * an address). */
int dm_encoder_embed_code(dm_encoder* e, const int64_t* indices, float* out, int B, int h, int w, void* stream);

/* ---- single operators (the kernels behind the calls above, exposed so that parity tests
 *      can check each one against the reference module it replaces) -------------------------
 * All tensors NCHW fp32 device pointers; weights in the reference layout, DEVICE pointers. */

/* nn.Conv2d forward (stride 1) with optional fused extras used by the U-Net:
 *   in = cat(in0, in1) along C (in1 may be NULL);  up2: nearest x2 before the conv
 *   (DD/denoising_diffusion.py:48-52);  residual (B,Cout,Ho,Wo) added to the result or NULL. */
int dm_op_conv2d(const float* in0, int C0, const float* in1, int C1, const float* weight, const float* bias,
                 const float* residual, float* out, int B, int H, int W, int Cout, int ksize, int pad, int up2,
                 void* stream);
/* Downsample: pixel-unshuffle(2) + conv1x1 (DD/denoising_diffusion.py:54-58); weight (Cout, 4*C, 1, 1) */
int dm_op_downsample(const float* in, int C, const float* weight, const float* bias, float* out, int B, int H,
                     int W, int Cout, void* stream);
/* RMSNorm.forward (DD/denoising_diffusion.py:66-67) */
int dm_op_rmsnorm(const float* x, const float* g, float* out, int B, int C, int H, int W, void* stream);
/* Block.forward (DD/denoising_diffusion.py:113-122); scale/shift (B,Cout) or NULL */
int dm_op_block(const float* x, int Cin, const float* weight, const float* bias, const float* g,
                const float* scale, const float* shift, float* out, int B, int H, int W, int Cout, void* stream);
/* LinearAttention.forward (DD/denoising_diffusion.py:173-193); mem_kv == NULL: the layer without memory key / values of the
 * sequence model (DD/denoising_diffusion_1d.py:164-215), here and in dm_op_attention */
int dm_op_linear_attention(const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv,
                           const float* w_out, const float* b_out, const float* out_g, float* out, int B, int C,
                           int H, int W, int heads, int dim_head, void* stream);
/* Attention.forward (DD/denoising_diffusion.py:215-229, DD/attend.py:109-124) */
int dm_op_attention(const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv,
                    const float* w_out, const float* b_out, float* out, int B, int C, int H, int W, int heads,
                    int dim_head, void* stream);
/* one DDPM / DDIM update on (n) elements given eps = model output (meaning per `objective`, DM_OBJ_*); c = DM_COEFS
 * floats (host); x_start (optional) receives the clamped x_0 estimate of the step (pred_x_start of model_predictions) */
int dm_op_sampler_update(int kind, int objective, const float* x, const float* eps, const float* noise,
                         const float* c_host, float* out, float* x_start, int64_t n, void* stream);
/* the same update with ddim_flags (DM_DDIM_*; kind DM_SAMPLER_DDIM only): 0 is dm_op_sampler_update */
int dm_op_sampler_update_ex(int kind, int objective, int ddim_flags, const float* x, const float* eps, const float* noise,
                            const float* c_host, float* out, float* x_start, int64_t n, void* stream);
/* nn.Conv1d forward on (B, C, L) tensors through the layer forms of Unet1D (DD/denoising_diffusion_1d.py):
 *   in = cat(in0, in1) along C (in1 may be NULL);  weight (Cout, C0 + C1, K);  stride 1 or 2;  residual (B, Cout, Lo) or NULL
 *   up2: Upsample = nearest x2 + Conv1d(K = 3, padding 1) (:56-60), executed as one K = 3 convolution with 2 Cout output
 *        channels on the source grid (even outputs: taps {w0, w1 + w2, 0}; odd outputs: {0, w0 + w1, w2}); out (B, Cout, 2L)
 *   Lo = (L + 2 pad - K) / stride + 1 */
int dm_op_conv1d(const float* in0, int C0, const float* in1, int C1, const float* weight, const float* bias,
                 const float* residual, float* out, int B, int L, int Cout, int K, int stride, int pad, int up2,
                 void* stream);
/* Block.forward of the sequence model (DD/denoising_diffusion_1d.py:127-136) with an optional residual added behind the
 * SiLU (ResnetBlock's `h + x`); x = cat(x0, x1); scale/shift (B, Cout) or NULL; residual (B, Cout, L) or NULL */
int dm_op_block1d(const float* x0, int C0, const float* x1, int C1, const float* weight, const float* bias, const float* g,
                  const float* scale, const float* shift, const float* residual, float* out, int B, int L, int Cout,
                  void* stream);
/* one DPM-Solver++ update (DM_SAMPLER_DPMPP) on (n) elements: coef_host is one row of DM_COEFS floats (host), x0_hist
 * (device) holds the previous step's clamped x_0 estimate and receives this step's; with c[4] == 0 it is not read */
int dm_op_dpmpp_update(int objective, const float* x, const float* model_out, float* x0_hist, const float* coef_host,
                       float* out, int64_t n, void* stream);
/* Dynamic thresholding on its own (dm_sample_ex_dyn).  s_out[b] = max(1, quantile(|x_start_raw|, percentile)) of image b
 * for B images of `per` values; x_start_raw from x and model_out by `objective` with c_host, one row of DM_COEFS floats. */
int dm_op_dyn_threshold(int objective, const float* x, const float* model_out, const float* c_host, int B, int64_t per,
                        double percentile, float* s_out, void* stream);
/* dm_op_sampler_update / dm_op_dpmpp_update on B images of `per` values with x_start thresholded by s (B floats, device) */
int dm_op_sampler_update_dyn(int kind, int objective, const float* x, const float* eps, const float* noise,
                             const float* c_host, const float* s, int B, int64_t per, float* out, float* x_start,
                             void* stream);
int dm_op_dpmpp_update_dyn(int objective, const float* x, const float* model_out, float* x0_hist, const float* coef_host,
                           const float* s, int B, int64_t per, float* out, void* stream);
/* The guidance combine of dm_sample_args.cfg on its own: out[b] = guided(cond[b], null_out[b]) for B rows of
 * per_sample floats (DD/classifier_free_guidance.py:355-369 with project :49-60).  Device pointers, out distinct from
 * both inputs. */
int dm_op_cfg_combine(const float* cond, const float* null_out, float* out, int B, int64_t per_sample, float cond_scale,
                      float rescaled_phi, int remove_parallel_component, float keep_parallel_frac, void* stream);
/* The VAE's non-convolution kernels on their own, in the kernels' own layouts (pixel rows, NHWC), through the same
 * launch functions as the decoder / encoder forward.  Workspaces are allocated inside the call; every call synchronises.
 * GroupNorm(groups, eps) with affine weight / bias (C), then x * sigmoid(x) when swish != 0
 * (LD/modules/diffusionmodules/model.py:50-56).  x, y: (B, HW, C). */
int dm_op_group_norm(const float* x_nhwc, const float* weight, const float* bias, float* y_nhwc, int B, int HW, int C,
                     int groups, float eps, int swish, void* stream);
/* The core of AttnBlock (model.py:203-215): out[b][i] = softmax_j(q[b][i] . k[b][j] * C^-1/2) v[b][j]; q, k, v, out
 * (B, n, C) rows.  kernel 0: the kernel the model dispatches for (n, C); 1: the one-row-per-wavefront kernel. */
int dm_op_vae_attention(const float* q, const float* k, const float* v, float* out, int B, int n, int C, int kernel,
                        void* stream);
/* One node of the first-stage trunk on its own, through the code the decoder / encoder forward runs for it.  Parameters are
 * DEVICE pointers in the reference layout (OIHW weights), packed per call; the operator workspace starts as NaNs; every
 * call synchronises.
 * A plain convolution node (k x k, stride, `pad` on every side and `pad_hi` more rows / columns of zeros below and right,
 * `up`: nearest x2 in front; H, W: the size in front of it).  in (B, Cin, H, W) when in_nchw, else pixel rows (B * H * W,
 * Cin); out (B, Cout, Ho, Wo) when out_nchw, else pixel rows; Ho = (H' + 2 pad + pad_hi - k) / stride + 1 with H' = 2 H
 * behind `up`.  bias may be NULL. */
int dm_op_vae_conv(const float* in, const float* weight, const float* bias, float* out, int B, int H, int W, int Cin, int Cout,
                   int k, int stride, int pad, int pad_hi, int up, int in_nchw, int out_nchw, void* stream);
/* ResnetBlock with temb = None (model.py:138-158) on pixel rows x (B * H * W, cin) -> out (B * H * W, cout); nin_w, nin_b
 * (the 1x1 nin_shortcut) are NULL exactly when cin == cout. */
int dm_op_vae_resblock(const float* x, const float* norm1_w, const float* norm1_b, const float* conv1_w, const float* conv1_b,
                       const float* norm2_w, const float* norm2_b, const float* conv2_w, const float* conv2_b,
                       const float* nin_w, const float* nin_b, float* out, int B, int H, int W, int cin, int cout,
                       void* stream);
/* AttnBlock (model.py:195-219) on pixel rows x, out (B * H * W, C); the weights of q, k, v, proj_out are (C, C, 1, 1). */
int dm_op_vae_attn_block(const float* x, const float* norm_w, const float* norm_b, const float* q_w, const float* q_b,
                         const float* k_w, const float* k_b, const float* v_w, const float* v_b, const float* proj_w,
                         const float* proj_b, float* out, int B, int H, int W, int C, void* stream);
/* The codebook search of VQModel.encode: z_rows (pixels, E), codebook (n_embed, E) -> zq_nchw (pixels / hw, E, hw) =
 * z + (nearest code - z) and indices (pixels, may be NULL); ties go to the lower index. */
int dm_op_vq_nearest(const float* z_rows, const float* codebook, float* zq_nchw, int32_t* indices, int64_t pixels, int E,
                     int n_embed, int hw, void* stream);
/* The same search on a latent in NCHW, z_nchw (pixels / hw, E, hw): the kernel behind dm_encoder_quantize. */
int dm_op_vq_nearest_nchw(const float* z_nchw, const float* codebook, float* zq_nchw, int32_t* indices, int64_t pixels, int E,
                          int n_embed, int hw, void* stream);
/* The posterior kernel of dm_encoder_forward_kl on its own.  moments (B, 2E, hw) in NCHW (layout DM_KL_NCHW) or as pixel rows
 * (B * hw, 2E) (DM_KL_ROWS); eps, seed, draw, element_offset, sample and the three optional outputs as there (Philox noise
 * needs E * hw % 4 == 0, injected noise has no such restriction). */
#define DM_KL_NCHW 0
#define DM_KL_ROWS 1
int dm_op_kl_posterior(const float* moments, int layout, const float* eps, uint64_t seed, uint64_t draw,
                       uint64_t element_offset, int sample, float* z, float* moments_nchw, float* kl, int B, int E, int hw,
                       void* stream);
/* The code gather of dm_encoder_embed_code on its own: indices (pixels) of index_bytes 4 (int32) or 8 (int64), codebook
 * (n_embed, E) -> out_nchw (pixels / hw, E, hw).  An index outside [0, n_embed) is an error. */
int dm_op_embed_code(const void* indices, int index_bytes, const float* codebook, float* out_nchw, int64_t pixels, int E,
                     int n_embed, int hw, void* stream);

/* ---- sample consumer: the InceptionV3 feature extractor behind the reference's FID and
 *      Inception-score evaluators (DD/fid_evaluation.py:41-51 -> pytorch_fid.inception.InceptionV3;
 *      DD/inception_score_evaluation.py:70-92 -> torchvision.models.inception_v3).  The layer graph is host code
 *      (diffusion-models_amd/inception.py); these are its operators.  Activations are NHWC fp32 DEVICE pointers.
 *      Both libraries and their pretrained weights are absent here: parity unpinned, checked against the oracle's
 *      restatement of the published architectures. -------------------------------------------------------------- */
typedef struct dm_conv dm_conv;
/* nn.Conv2d(Cin, Cout, (KH, KW), stride, (pad_h, pad_w)) with an optional ReLU; weight_host OIHW, bias_host or NULL
 * (BasicConv2d = conv + BatchNorm(eval) + ReLU is passed with the BatchNorm folded into weight and bias) */
int dm_conv_create(const float* weight_host, const float* bias_host, int Cout, int Cin, int KH, int KW, int stride,
                   int pad_h, int pad_w, int relu, int device, dm_conv** out);
void dm_conv_destroy(dm_conv* c);
/* in: (B, H, W, Cin) NHWC, or (B, Cin, H, W) when in_nchw != 0; out: (B, Ho, Wo, Cout) NHWC.  All dm_conv handles of a
 * device share one scratch workspace (K-split partial sums): their calls must be ordered on one stream. */
int dm_conv_forward(dm_conv* c, const float* in, int in_nchw, int B, int H, int W, float* out_nhwc, void* stream);
/* F.max_pool2d / F.avg_pool2d on NHWC: mode 0 max, 1 avg with count_include_pad=True, 2 avg with count_include_pad=False */
int dm_op_pool2d(const float* in, float* out, int B, int H, int W, int C, int k, int stride, int pad, int mode,
                 void* stream);
/* F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=False) of an NCHW batch, written NHWC, then
 * scale[c] * v + shift[c] (scale / shift: C floats on the device) */
int dm_op_resize_bilinear(const float* in_nchw, float* out_nhwc, int B, int C, int H, int W, int Ho, int Wo,
                          const float* scale_dev, const float* shift_dev, void* stream);
/* torch.cat along channels, one source at a time: dst[row][c_off + c] = src[row][c] */
int dm_op_copy_channels_nhwc(const float* src, int Cs, float* dst, int Cd, int c_off, int64_t rows, void* stream);
/* adaptive_avg_pool2d(x, (1, 1)) on NHWC: out (B, C) */
int dm_op_global_avgpool(const float* in_nhwc, float* out, int B, int HW, int C, void* stream);
/* nn.Linear: y (R, O) = x (R, I) W^T + b; weight (O, I) and bias on the device */
int dm_op_linear(const float* x, const float* weight, const float* bias, float* y, int R, int I, int O, void* stream);

/* ---- training step: DenoisingDiffusion.forward / p_losses, DD/denoising_diffusion.py:805-900, and
 *      the backward pass of the same U-Net (what `accelerator.backward(loss)` computes in Trainer.train, :1162-1176).
 *      Unconditional U-Net (no text / image condition, no self-conditioning), dropout 0, loss_weight from the caller.
 *      Gradients are kept on the handle in the reference's parameter layouts (state_dict() shapes). ------------------- */

/* allocate the gradient buffers and pack the input-gradient convolutions (the forward kernels run on 180-degree rotated,
 * Cin<->Cout transposed weights); dm_unet_refresh re-packs them together with the forward weights afterwards */
int dm_unet_train_enable(dm_unet* u);
/* total floats of the flat gradient buffer (parameters in state-dict order, each padded to a multiple of 4), or -1 */
int64_t dm_unet_grad_floats(dm_unet* u);
/* the flat gradient buffer itself (device pointer, dm_unet_grad_floats floats): data-parallel training (accelerate / DDP in
 * the reference's Trainer) all-reduces it in place -- ONE collective for all gradients -- before dm_unet_optimizer_step */
int dm_unet_grads_flat(dm_unet* u, float** ptr_out, int64_t* n_out);
/* Gradient buckets for data-parallel training -- what torch DDP's 25 MB buckets are to the reference's Trainer under accelerate
 * (DD/denoising_diffusion.py:971-974, :1175): the flat buffer is laid out bucket by bucket in the order the backward pass
 * completes them (convolution weights of the stages it leaves first; the last bucket holds the last stages and every
 * parameter only the end of the pass completes), DM_TRAIN_BUCKET_MB (default 25) per bucket.
 *   dm_unet_train_buckets(u, enable): returns the number of buckets; with enable != 0 every later dm_unet_loss_backward runs a
 *     bucket's weight gradients as soon as the pass has left the bucket's stages, and records an event.
 *   dm_unet_train_bucket(u, i, &off, &n, wait, stream): bucket i's span of the flat buffer in floats; with wait != 0 `stream`
 *     is made to wait for the bucket's event of the last pass, so that a collective enqueued on it runs beside the rest of
 *     the pass (the caller joins the streams before dm_unet_optimizer_step). */
int dm_unet_train_buckets(dm_unet* u, int enable);
int dm_unet_train_bucket(dm_unet* u, int i, int64_t* off_out, int64_t* n_out, int wait, void* wait_stream);
/* copy the gradient of one parameter (names as in dm_unet_set_param) into a DEVICE buffer of the parameter's size */
int dm_unet_get_grad(dm_unet* u, const char* name, float* out_dev, void* stream);
/* One p_losses call (:823-889) + backward:
 *   x = q_sample(x_start, t, noise) (:813-821);  out = Unet(x, t);  target per `objective` (DM_OBJ_*, :864-872);
 *   loss = loss_scale * mean_b( loss_weight[t_b] * mean((out - target)^2) ) (:874-878, :889);  every parameter gradient.
 * x_start, noise: (B, C, H, W) device, x_start already normalised to [-1, 1];  t_host: (B) timesteps;
 * coef_host: (B, 8) = sqrt_alphas_cumprod[t_b], sqrt_one_minus_alphas_cumprod[t_b], loss_weight[t_b], 0,
 * sqrt_recip_alphas_cumprod[t_b], sqrt_recipm1_alphas_cumprod[t_b], 0, 0 -- the values `extract` gathers (:394-397).
 * self_cond (Unet(self_condition=True), :846-855): 0 off; 1 the U-Net sees [0 | x]; 2 it sees [x_start | x] with x_start
 * predicted (unclipped, without gradient) by a first forward pass on [0 | x] -- the caller flips the reference's coin.  loss_scale = 1 / gradient_accumulate_every and accumulate != 0 adds the gradients to
 * what the buffers hold (the micro-batch loop of Trainer.train, :1164-1176).  loss_out_host receives the scalar loss;
 * model_out (optional, device) the U-Net output.  cond (optional): the condition image (B, cond_channels, H, W) of the
 * image-conditional variant, concatenated behind x in front of init_conv (DD/denoising_diffusion_image_conditional.py:51-55,
 * p_losses :251-311).  ctx (optional): the text embeddings (B, ctx_tokens, text_emb_dim) of the text-conditional variant
 * (DD/denoising_diffusion_text_conditional.py:131-214, p_losses :476-542), concat or cross-attention per the handle's
 * text_mode.  noise_q (optional): the noise q_sample mixes in when it is not `noise` itself -- with immiscible=True the
 * reference's q_sample re-assigns the noise rows inside (:815-817) while p_losses keeps the unpermuted tensor as the
 * target (:865).  The call synchronises the stream unless loss_out_host is NULL (then see dm_unet_train_scalar). */
int dm_unet_loss_backward(dm_unet* u, const float* x_start, const int64_t* t_host, const float* coef_host,
                          const float* noise, const float* noise_q, const float* cond, int cond_channels, const float* ctx,
                          int ctx_tokens,
                          int self_cond, int objective, float loss_scale, int accumulate, float* loss_out_host,
                          float* model_out, int B, int H, int W, void* stream);
/* The same call with its arguments in one struct, plus the hybrid (KL) term of p_losses (:880-897):
 *   loss_terms: 1 the weighted MSE (what dm_unet_loss_backward computes), 2 the KL term alone, 3 both in one pass.  The
 *     reference evaluates the KL term through p_mean_variance, i.e. a SECOND forward pass of the U-Net with gradients: without
 *     dropout that pass repeats the first one bit for bit and loss_terms = 3 is the same loss and gradient; with dropout the
 *     second pass draws new masks -- the caller then runs loss_terms = 1 followed by loss_terms = 2 with accumulate = 1.
 *   coef_stride: floats per row of coef_host, 8 (rows as above) or 12: [3] = 1 if t_b > 0 else 0 (the reference's mask),
 *     [8] posterior_mean_coef1[t_b], [9] posterior_mean_coef2[t_b], [10] posterior_variance[t_b],
 *     [11] posterior_log_variance_clipped[t_b] -- required by the KL term.
 *   kl_scale = 0.001 / (mask.sum() + 1e-8), formed by the caller in fp32 as the reference does (:893-895).
 * The KL term divides by posterior_variance[t], which is 0 at t = 0, before the mask multiplies (inf * 0): a batch holding a
 * t = 0 sample has a NaN loss and NaN gradients in the reference and here. */
typedef struct dm_train_args {
    const float* x_start;
    const int64_t* t_host;
    const float* coef_host;
    int coef_stride;
    const float* noise;
    const float* noise_q;
    const float* cond;
    int cond_channels;
    const float* ctx;
    int ctx_tokens;
    int self_cond;
    int objective;
    float loss_scale;
    int accumulate;
    float* loss_out_host;
    float* model_out;
    int B, H, W;
    void* stream;
    int loss_terms;
    float kl_scale;
} dm_train_args;
int dm_unet_loss_backward_ex(dm_unet* u, const dm_train_args* a);
/* The same call with a per-image text mask (per-image caption dropout, what DD/classifier_free_guidance.py does with
 * cond_drop_prob / prob_mask_like, :41-47, :376-392).  text_mask: B HOST int32 values, copied to the device as t_host is.
 * Image b keeps its caption iff text_mask[b] != 0; the others are trained as if text_emb were None.  The mask holds in
 * every forward pass of the call: the gradient-free self-conditioning pass and the KL term's pass see the same one.  It
 * needs a->ctx; masked-out rows of ctx are read (they must be initialised), their values reach neither the loss nor any
 * gradient.  dm_train_args is unchanged, so dm_unet_loss_backward_ex issues the launches it always did. */
int dm_unet_loss_backward_masked(dm_unet* u, const dm_train_args* a, const int32_t* text_mask);
/* The rest of one Trainer.train iteration (:1178-1190) on device-resident state: the master parameters, the Adam moments and
 * the EMA copy live in flat device buffers in the reference layouts; after the update every packed weight buffer the
 * kernels read is rebuilt on the device (pack_kernels.hip, bit-identical to the host packers).
 *   dm_unet_optimizer_step: clip_grad_norm_(max_grad_norm; <= 0: off), Adam(lr, (beta1, beta2), eps) step; the total
 *                           gradient norm (before clipping) goes to grad_norm_out_host when given.
 *                           lr, the betas and eps are doubles, as torch's Python floats are; the step is evaluated in
 *                           double on the fp32 state and m, v, p are rounded to float once each.  A NaN
 *                           gradient makes the norm, the coefficient and with max_grad_norm > 0 every parameter NaN.
 *   dm_unet_ema_update:     copy != 0: ema <- online;  else ema.lerp_(online, 1 - decay), the weight formed in double
 *   dm_unet_get_param:      one tensor of the online parameters (which = 0), the EMA copy (1) or Adam's exp_avg (2) /
 *                           exp_avg_sq (3) into a device buffer -- what Trainer.save (:1100-1113) writes as 'model' / 'ema' /
 *                           'opt'
 *   dm_unet_set_train_tensor: the inverse for which = 1, 2, 3 (Trainer.load, :1115-1133; the online parameters go through
 *                           dm_unet_set_param + dm_unet_refresh);  dm_unet_adam_step: torch.optim.Adam's `step` counter,
 *                           returned (set first when set_to >= 0; -1: not a training handle)
 *   dm_unet_train_sync:     device -> host copies + dm_unet_refresh, after which the handle samples with the trained weights
 *                           (the sampling entry points refuse to run on stale fused packs until then)
 *   dm_unet_check_device_pack: self-check, number of packed buffers whose device packer differs from the host packer */
int dm_unet_optimizer_step(dm_unet* u, double lr, double beta1, double beta2, double eps, float max_grad_norm,
                           float* grad_norm_out_host, void* stream);
/* The same step when parameters OUTSIDE the handle share the clip (the six host parameters of a learned noise schedule):
 * extra_sq_norm, the squared L2 norm of their gradients, is added to the handle's squared gradient norm before the clip
 * coefficient min(1, max_grad_norm / (norm + 1e-6)) is formed; *grad_norm_out_host is the combined norm, from which the caller
 * forms the same coefficient for its own parameters.  extra_sq_norm == 0 is dm_unet_optimizer_step. */
int dm_unet_optimizer_step_ex(dm_unet* u, double lr, double beta1, double beta2, double eps, float max_grad_norm,
                              float extra_sq_norm, float* grad_norm_out_host, void* stream);
/* The loop's scalars without a host round trip (the reference's loss is a device tensor until Trainer calls loss.item(),
 * DD/denoising_diffusion.py:1173): with loss_out_host == NULL dm_unet_loss_backward, and with grad_norm_out_host == NULL
 * dm_unet_optimizer_step, return as soon as their kernels are enqueued; dm_unet_train_scalar copies the loss of the last
 * loss / backward call (which = 0) or the total gradient norm of the last optimiser step (which = 1) to a DEVICE float. */
int dm_unet_train_scalar(dm_unet* u, int which, float* out_dev, void* stream);
int dm_unet_ema_update(dm_unet* u, double decay, int copy, void* stream);
int dm_unet_get_param(dm_unet* u, const char* name, int which, float* out_dev, void* stream);
int dm_unet_set_train_tensor(dm_unet* u, const char* name, int which, const float* src_dev, void* stream);
long long dm_unet_adam_step(dm_unet* u, long long set_to);
int dm_unet_train_sync(dm_unet* u);
int dm_unet_check_device_pack(dm_unet* u);
/* nn.Dropout(p) of the Blocks in training mode (Unet(dropout = p), :111,121; the shipped ddpm_cifar.yaml trains with 0.1).
 * Masks are Philox4x32-10 draws keyed by (seed, call, block index): every dm_unet_loss_backward call after this one draws
 * fresh masks; the backward pass re-creates the masks of its forward from the key.  The VALUES differ from torch's
 * generator, the semantics (Bernoulli(1 - p) keep, scale 1 / (1 - p), after the activation, before the residual add) do not.
 * dm_op_dropout_mask writes the factor (0 or 1 / (1 - p)) the block_index-th Block (forward order) of call number `call`
 * applies, n elements in (B, H, W, C) order -- parity tests hand these masks to the oracle. */
int dm_unet_train_dropout(dm_unet* u, float p, uint64_t seed);
int dm_op_dropout_mask(float* out, int64_t n, float p, uint64_t seed, uint64_t call, int block_index, void* stream);
/* q_sample (:813-821) on its own: out = coef[b][0] * x_start + coef[b][1] * noise, coef_host (B, 12): rows as in dm_train_args */
int dm_op_q_sample(const float* x_start, const float* noise, const float* coef_host, float* out, int B, int per_sample,
                   void* stream);
/* The elementwise helpers of DenoisingDiffusion as callable methods -- predict_start_from_noise, predict_noise_from_start,
 * predict_v, predict_start_from_v, the posterior mean of q_posterior (DD/denoising_diffusion.py:570-601), and through them
 * model_predictions (:603-626) / p_mean_variance (:628-636) with per-sample timesteps: coef_host (B, 2) = the two values
 * `extract` gathers;  mode 0: out = c0 * x + c1 * y;  mode 1: out = (c0 * x - y) / c1;  clamp != 0: to [-1, 1] afterwards.
 * dm_op_mask_mix: out = a * mask + b * (1 - mask), the guide step of ddim_sample_guided (:754); all (n) device floats. */
int dm_op_lincomb(const float* x, const float* y, const float* coef_host, float* out, int B, int64_t per_sample, int mode,
                  int clamp, void* stream);
int dm_op_mask_mix(const float* a, const float* b, const float* mask, float* out, int64_t n, void* stream);
/* offset noise (:830-834): noise[b][c][:] += strength * offset[b][c]  (noise (B, C, H, W) in place, offset (B, C)) */
int dm_op_offset_noise(float* noise, const float* offset, float strength, int BC, int HW, void* stream);
/* immiscible diffusion's noise assignment (:805-817): out[i][j] = || x[i] - y[j] ||_2 over D floats (torch.cdist of the
 * flattened batches; the caller runs scipy's linear_sum_assignment on it, as the reference does, on the host) and the row
 * gather dst[i] = src[idx[i]] (idx: n host indices) */
int dm_op_cdist(const float* x, const float* y, float* out, int n, int m, int64_t D, void* stream);
int dm_op_gather_rows(const float* src, const int64_t* idx_host, float* dst, int n, int64_t D, void* stream);
/* The loss kernel of dm_unet_loss_backward on its own: out (the model output), x_start, noise, xq (the q_sample output, needed
 * with terms & 2) and dout (B, per_sample) device floats; coef_host (B, 12) rows as in dm_train_args; objective 0 / 1 / 2;
 * terms as loss_terms there; kl_weight: the reference's 0.001 -- the KL factor is kl_weight / (n_pos + 1e-8) in fp32 with
 * n_pos the number of rows whose [3] is 1.  *loss_out_host = loss_scale * (mean_b part[b] + factor * sum_b klpart[b]);
 * part_out / klpart_out (optional, B device floats): loss_weight[t_b] * mean((out - target)^2) and mean(kl) * [t_b > 0]. */
int dm_op_mse_loss(const float* out, const float* x_start, const float* noise, const float* xq, const float* coef_host,
                   int objective, int terms, float loss_scale, float kl_weight, float* dout, float* loss_out_host,
                   float* part_out, float* klpart_out, int B, int per_sample, void* stream);
/* What dm_unet_optimizer_step / dm_unet_ema_update run, on flat device buffers of n floats (g 16-byte aligned):
 * clip_grad_norm_(max_grad_norm; <= 0: off) + the step-th torch.optim.Adam step, p / m / v updated in place,
 * norm_coef_out_host (optional) = {total norm before clipping, clip coefficient};  ema.lerp_(p, 1 - decay) in place. */
int dm_op_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                    int step, float max_grad_norm, float* norm_coef_out_host, void* stream);
int dm_op_ema_lerp(float* ema, const float* p, int64_t n, double decay, void* stream);

/* Backward of the single operators above (what autograd computes for the reference module), for parity tests of each
 * piece of the training step.  All tensors NCHW fp32 device pointers; gradient outputs have the shape of the tensor they
 * differentiate; optional outputs may be NULL. */
/* nn.Conv2d backward: 3x3 / pad 1 (up2: the conv ran on the nearest-x2 upsampled cat(in0, in1)) or 1x1; dy (B,Cout,Ho,Wo) */
int dm_op_conv2d_bwd(const float* in0, int C0, const float* in1, int C1, const float* weight, const float* dy, float* d_in0,
                     float* d_in1, float* d_weight, float* d_bias, int B, int H, int W, int Cout, int ksize, int pad, int up2,
                     void* stream);
/* Downsample backward (DD/denoising_diffusion.py:54-58) */
int dm_op_downsample_bwd(const float* in, int C, const float* weight, const float* dy, float* d_in, float* d_weight,
                         float* d_bias, int B, int H, int W, int Cout, void* stream);
/* Block backward (:113-122); d_scale / d_shift (B, Cout) */
int dm_op_block_bwd(const float* x, int Cin, const float* weight, const float* bias, const float* g, const float* scale,
                    const float* shift, const float* dy, float* dx, float* d_weight, float* d_bias, float* d_g,
                    float* d_scale, float* d_shift, int B, int H, int W, int Cout, void* stream);
/* RMSNorm backward (:66-67) */
/* nn.Linear backward on its own (time_mlp, ResnetBlock.mlp; DD/denoising_diffusion.py:127-130, :280-285): dx (R, I) = dy W,
 * d_weight (O, I) (+)= dy^T x, d_bias (O) (+)= column sums of dy; any of the three outputs may be NULL */
int dm_op_linear_bwd(const float* x, const float* weight, const float* dy, float* dx, float* d_weight, float* d_bias, int R,
                     int I, int O, int accumulate, void* stream);
int dm_op_rmsnorm_bwd(const float* x, const float* g, const float* dy, float* dx, float* dg, int B, int C, int H, int W,
                      void* stream);
/* LinearAttention / Attention backward (:173-193, :215-229) */
int dm_op_linear_attention_bwd(const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv,
                               const float* w_out, const float* b_out, const float* out_g, const float* dy, float* dx,
                               float* d_norm_g, float* d_mem_kv, float* d_w_qkv, float* d_w_out, float* d_b_out,
                               float* d_out_g, int B, int C, int H, int W, int heads, int dim_head, void* stream);
int dm_op_attention_bwd(const float* x, const float* norm_g, const float* mem_kv, const float* w_qkv, const float* w_out,
                        const float* b_out, const float* dy, float* dx, float* d_norm_g, float* d_mem_kv, float* d_w_qkv,
                        float* d_w_out, float* d_b_out, int B, int C, int H, int W, int heads, int dim_head, void* stream);
/* The attention cores of the training step alone (no norm, no projection): the forward core as the training forward runs
 * it, the backward core, and the sum of the per-image memory-token gradients.  Token rows, not NCHW:
 * qkv, dqkv (B, n, 3*heads*dim_head) = [q(h,d) | k(h,d) | v(h,d)] per token;  dout, out (B, n, heads*dim_head).
 * LinearAttention: mem_kv, d_mem_kv (2, heads, dim_head, 4); ctx (B, heads, dim_head, dim_head); kstats (B, heads, 2, dim_head)
 * = per column of k the maximum over the n + 4 tokens and the sum of exp(k - max); dmem_part (B, 2, heads, dim_head, 4).
 * Attention: mem_kv, d_mem_kv (2, heads, 4, dim_head); dmem_part (B, 2, heads, 4, dim_head).
 * Every output is optional (NULL) and is written by the kernels directly, without a copy. */
int dm_op_linear_attention_core_bwd(const float* qkv, const float* mem_kv, const float* dout, float* out, float* ctx,
                                    float* kstats, float* dqkv, float* dmem_part, float* d_mem_kv, int B, int n, int heads,
                                    int dim_head, void* stream);
int dm_op_attention_core_bwd(const float* qkv, const float* mem_kv, const float* dout, float* out, float* dqkv,
                             float* dmem_part, float* d_mem_kv, int B, int n, int heads, int dim_head, void* stream);
/* CrossAttention of the text-conditional U-Net (DD/denoising_diffusion_text_conditional.py:54-78), forward and backward,
 * through the code the models run (4 heads, as there).  x, dy, out, y_out, dx (B, C, H, W); ctx (B, m, E); weights in the
 * reference layout: w_q (4*dim_head, C), w_k / w_v (4*dim_head, E), w_out (C, 4*dim_head), b_out (C), out_g (C).
 * text_mask: B device int32 or NULL; image b with text_mask[b] == 0 skips the layer (out = x, dx = dy, no contribution to
 * any parameter gradient).  The forward takes the one-token algebra at m == 1; the backward call always runs the general
 * path and returns that path's forward result in y_out (optional).  There is no gradient for ctx. */
int dm_op_cross_attention(const float* x, const float* ctx, const float* w_q, const float* w_k, const float* w_v,
                          const float* w_out, const float* b_out, const float* out_g, const int32_t* text_mask, float* out,
                          int B, int C, int H, int W, int m, int E, int dim_head, void* stream);
int dm_op_cross_attention_bwd(const float* x, const float* ctx, const float* w_q, const float* w_k, const float* w_v,
                              const float* w_out, const float* b_out, const float* out_g, const int32_t* text_mask,
                              const float* dy, float* y_out, float* dx, float* d_w_q, float* d_w_k, float* d_w_v,
                              float* d_w_out, float* d_b_out, float* d_out_g, int B, int C, int H, int W, int m, int E,
                              int dim_head, void* stream);

/* The conditioning head of the U-Net on its own: time [+ pooled caption] -> the (B, ss_total) scale / shift rows every
 * ResnetBlock reads (Unet.forward, DD/denoising_diffusion.py:349-361; DD/denoising_diffusion_text_conditional.py:146-152),
 * through the very functions the walks call, in a NaN-filled workspace.  Row-major device buffers, every one optional
 * (NULL = not wanted); td = 4 * dim, fdim = dim or learned_sinusoidal_dim + 1:
 *   e0 (R, fdim) the sinusoidal embedding; h1pre (R, td) time_mlp.1's output; h1 (R, td) = GELU(h1pre); temb (R, td) time_mlp's
 *   output; te0pre (B, td) text_proj.0's output; te0 (B, td) = GELU(te0pre); cat (B, 2 td) = [temb | text_proj(caption)];
 *   tfinal what the ResnetBlock.mlp layers see -- temb (R, td) or, with a caption, text_concat_proj(cat) (B, td), rows with
 *   text_mask 0 holding temb; tact = SiLU(tfinal); ss (Bs, ss_total).
 * R = Bs = B with one time per image.  A shared time (the samplers) gives R = 1, and Bs = 1 unless there is a caption.
 * h1pre, te0pre and tact exist in the training forward only (the inference walk fuses the activations): they must be NULL
 * for DM_COND_WALK_INFER. */
typedef struct dm_cond_bufs {
    float *e0, *h1pre, *h1, *temb, *te0pre, *te0, *cat, *tfinal, *tact, *ss;
} dm_cond_bufs;
#define DM_COND_WALK_INFER 0 /* the head of dm_unet_forward / the samplers */
#define DM_COND_WALK_TRAIN 1 /* the head of the training forward: fills the tape dm_unet_cond_backward reads */
#define DM_COND_TIME_INT 0          /* time: B device int64 */
#define DM_COND_TIME_FLOAT 1        /* time: B device floats (needs learned_sinusoidal_dim > 0) */
#define DM_COND_TIME_INT_SHARED 2   /* time: one device int64 for the whole batch (inference walk only) */
#define DM_COND_TIME_FLOAT_SHARED 3 /* time: one device float for the whole batch (inference walk only) */
/* ctx: (B, text_emb_dim) pooled caption or NULL; text_mask: B device int32 or NULL (needs ctx).  The training walk embeds an
 * integer time with the fixed sinusoid and a float time with the learned / random one, as the training step does. */
int dm_unet_cond_forward(dm_unet* u, int walk, int time_kind, const void* time, const float* ctx, const int32_t* text_mask,
                         const dm_cond_bufs* out, int B, void* stream);
/* Its backward on a handle armed by dm_unet_train_enable / dm_unet_train_enable_ft: `tape` holds the outputs of a
 * DM_COND_WALK_TRAIN forward (e0, h1pre, h1, tfinal, tact; with a caption te0pre, te0, cat too), dss (B, ss_total) is the
 * gradient of ss.  Parameter gradients go to the handle's slots ((+)= with accumulate; dm_unet_get_grad reads them):
 * every *.mlp.1.{weight,bias}, time_mlp.{1,3}.*, text_proj.*, text_concat_proj.*, time_mlp.0.weights (float-time handles).
 * dt (B, optional): the gradient of a float time. */
int dm_unet_cond_backward(dm_unet* u, const dm_cond_bufs* tape, const float* ctx, const int32_t* text_mask, const float* dss,
                          float* dt, int B, int accumulate, void* stream);

/* The reductions a training backward pass defers to its end, on their own.  Every layer is launched as the pass launches
 * it: with deferred != 0 it is recorded in the pass's two job tables, which are then run by the function the pass calls
 * (four launches for all layers); with deferred == 0 each layer runs its immediate kernels.  One B for all layers.
 *   DM_REDUCE_NORM_BWD: the backward of y = [SiLU](RMSNorm(u) * g [* (scale + 1) + shift]); dy, u, du (B * rows, C) token rows
 *     (rows = pixels per image), g, dg, dbias (C) (dbias = column sums of du, optional), ss / dss (B rows, ss_stride /
 *     dss_stride floats apart, (scale | shift) in the first 2 C columns; both or neither).  C % 4 == 0, C <= 1024.
 *   DM_REDUCE_COLSUM: out[c] = sum_r x[r * row_stride + c * col_stride], c < C.
 * dg, dbias and out are (+)= with accumulate; the kernels write into the caller's buffers directly. */
#define DM_REDUCE_NORM_BWD 0
#define DM_REDUCE_COLSUM 1
typedef struct dm_reduce_layer {
    int32_t kind, C, silu, ss_stride, dss_stride, reserved;
    int64_t rows, row_stride, col_stride;
    const float *dy, *u, *g, *ss, *x;
    float *du, *dg, *dbias, *dss, *out;
} dm_reduce_layer;
int dm_op_deferred_reduce(const dm_reduce_layer* layers, int n_layers, int B, int deferred, int accumulate, void* stream);

/* ---- measurement (bench.py's roofline leg; not part of the reference surface) -------------
 * While enabled, every convolution / fused-attention launch is bracketed by two HIP events recorded on
 * the stream the kernel is launched on.  Do not combine with use_graph.  dm_profile_enable(1) first
 * measures the interval of an EMPTY-kernel bracket (dispatch + event packets); dm_profile_read
 * synchronises the device, subtracts that interval from every bracket (total_ms is kernel execution
 * time), aggregates the recorded launches per kernel instance, and clears the records.
 * total_flops / total_bytes are ALGORITHMIC (2*k*k*Cin*Cout*pixels; input + output + weights
 * each moved once), see DESIGN.md. */
typedef struct dm_profile_row {
    char kernel[64];
    int64_t launches;
    double total_ms;
    double total_flops;
    double total_bytes;
} dm_profile_row;
int dm_profile_enable(int on);
int dm_profile_read(dm_profile_row* rows, int max_rows, int* n_rows);

/* ---- ElucidatedDiffusion (DD/elucidated_diffusion.py; Karras et al. "EDM"): sampling, then training ----------------
 * Unet.forward with a REAL-valued time, one float per image (c_noise(sigma) = 0.25 ln sigma): the handle must have
 * learned_sinusoidal_dim > 0, the only U-Net ElucidatedDiffusion accepts (:42).  dm_unet_forward keeps its int64 time. */
int dm_unet_forward_ft(dm_unet* u, const float* x, const float* time, const float* ctx, int ctx_tokens, float* out, int B,
                       int H, int W, void* stream);

/* ElucidatedDiffusion.sample (Heun, :129-187) and .sample_using_dpmpp (DPM-Solver++(2M), :189-224).  As for dm_sample,
 * the HOST computes every per-step scalar exactly as the reference does -- the preconditioning terms in fp32 tensor
 * arithmetic, sigma_hat / sqrt(sigma_hat^2 - sigma^2) / sigma_next - sigma_hat as doubles rounded to fp32 once -- and passes
 * n_steps rows of DM_EDM_COEFS floats:
 *   Heun step i:   c[0]=sqrt(sigma_hat^2 - sigma^2) (0 when gamma == 0)   c[1]=S_noise
 *                  c[2..5]=c_in, c_noise, c_skip, c_out at sigma_hat       c[6]=sigma_hat   c[7]=sigma_next - sigma_hat
 *                  c[8..11]=c_in, c_noise, c_skip, c_out at sigma_next     c[12]=sigma_next c[13]=0.5*(sigma_next - sigma_hat)
 *                  c[12] == 0 marks the step that runs one forward only (the reference's last step, :176)
 *   DPM++ step i:  c[2..5] at sigma_i   c[8]=sigma_fn(t_next)/sigma_fn(t)   c[9]=expm1(-h)   c[10]=gamma   c[11]=1 - gamma
 *                  (gamma = 0 at the first step and when sigma_next == 0: denoised_d = denoised, :212-213)
 *   unused entries are 0.
 *   x_init     (B,C,H,W) N(0,1) noise, draw 0 of the reference; the loop starts from sigma_init * x_init (:151, :201)
 *   noise      Heun only.  NULL -> device Philox noise (draw i + 1 at step i); else (n_steps, B,C,H,W), row i read by step
 *              i.  A step whose c[0] == 0 reads neither.  sample_offset as in dm_sample.
 *   clamp      Heun: clamp every denoised image to [-1, 1] (:107-108); DPM-Solver++ never clamps per step.
 *   out        (clamp(x, -1, 1) + 1) / 2   (:186-187, :223-224)
 *   use_graph  a Heun step (two forwards) and the final single-forward step are captured as one hipGraph each, a DPM++
 *              step as one; cached on the handle per (kind, B, H, W, clamp, noise pointer) like dm_sample's graph. */
#define DM_EDM_COEFS 16
#define DM_EDM_HEUN 0
#define DM_EDM_DPMPP 1
typedef struct dm_edm_args {
    int32_t kind;       /* DM_EDM_* */
    int32_t n_steps;
    const float* table_host;
    const float* x_init;
    const float* noise;
    uint64_t seed;
    uint64_t sample_offset;
    float* out;
    float sigma_init;
    int32_t clamp;
    int32_t B, H, W;
    int32_t use_graph;
    void* stream;
} dm_edm_args;
int dm_sample_edm(dm_unet* u, const dm_edm_args* args);

/* The elementwise passes of the two loops on their own (tests).  c_host: `rows` table rows in the layout above, rows == 1
 * (every image) or rows == B (row b for image b: preconditioned_network_forward on a (B,) sigma).  Tensors are B * per
 * floats, per % 4 == 0, 16-byte aligned.  The table-driven ones wait for the result.
 *   churn_in:  xhat = x + c[0] * (c[1] * eps); xin = c[2] * xhat.  eps NULL: Philox draw `draw` (>= 1) under `seed`.
 *              xhat may be NULL.
 *   euler:     D = c[4] xhat + c[5] F [clamped]; d = (xhat - D) / c[6]; xnext = xhat + c[7] d; xin_next = c[8] xnext.
 *              Each of the four outputs may be NULL.
 *   heun:      D' = c[10] xnext + c[11] F2 [clamped]; d' = (xnext - D') / c[12]; out = xhat + c[13] (d + d').
 *   dpmpp:     D = c[4] x + c[5] F; out = c[8] x - c[9] (c[11] D + c[10] d_old)  (D itself when c[10] == 0); d_old = D.
 *   finalize:  out = (clamp(x, -1, 1) + 1) / 2 on n floats. */
int dm_op_edm_churn_in(const float* x, const float* eps, const float* c_host, int rows, uint64_t seed, uint64_t draw,
                       uint64_t element_offset, float* xhat, float* xin, int B, int64_t per, void* stream);
int dm_op_edm_euler(const float* xhat, const float* F, const float* c_host, int rows, int clamp, float* D_out, float* d_out,
                    float* xnext, float* xin_next, int B, int64_t per, void* stream);
int dm_op_edm_heun(const float* xhat, const float* d, const float* xnext, const float* F2, const float* c_host, int rows,
                   int clamp, float* out, int B, int64_t per, void* stream);
int dm_op_edm_dpmpp(const float* x, const float* F, float* d_old, const float* c_host, int rows, float* out, int B,
                    int64_t per, void* stream);
int dm_op_edm_finalize(const float* x, float* out, int64_t n, void* stream);

/* ---- ElucidatedDiffusion training (DD/elucidated_diffusion.py:228-264) ------------------------------------------------
 * dm_unet_train_enable_ft arms a learned / random sinusoidal U-Net (learned_sinusoidal_dim > 0, no text conditioning,
 * out_dim == channels) for training with a REAL-valued time: the same gradient buffers, optimiser state and buckets as
 * dm_unet_train_enable, which keeps refusing such a U-Net -- what it arms is the integer-time p_losses path, and an int64
 * time would truncate c_noise(sigma).  A handle armed this way is refused by dm_unet_loss_backward*; every other training
 * entry (dm_unet_optimizer_step, dm_unet_ema_update, dm_unet_get_grad, dm_unet_train_sync, dm_unet_grads_flat, the buckets,
 * dm_unet_train_scalar) works on it unchanged.  The embedding's parameter time_mlp.0.weights takes a gradient; with
 * time_weights_frozen != 0 that gradient is exact zeros instead (random_fourier_features: the reference builds the
 * parameter with requires_grad = False -- the handle's configuration does not say which embedding it holds, so the call
 * that arms it does), and Adam leaves the parameter bit for bit where it is.  A repeated call updates the flag. */
int dm_unet_train_enable_ft(dm_unet* u, int time_weights_frozen);

/* One ElucidatedDiffusion.forward (:234-264) + backward:
 *   x0 = 2 images - 1;  noised = x0 + sigma_b noise;  F = Unet(c_in_b noised, c_noise_b);  D = c_skip_b noised + c_out_b F;
 *   loss = loss_scale * mean_b( loss_weight_b * mean((D - x0)^2) );  every parameter gradient.
 * images (in [0, 1]) and noise: (B, C, H, W) device.  coef_host: B rows of coef_stride floats (0: DM_EDM_COEFS) in the
 * layout of the step table above -- c[2..5] = c_in, c_noise, c_skip, c_out at sigma_b, c[6] = sigma_b -- plus
 * c[14] = loss_weight(sigma_b); the host computes them in fp32 tensor arithmetic as the reference does.  loss_scale,
 * accumulate, loss_out_host (NULL: the call only enqueues, see dm_unet_train_scalar) as in dm_unet_loss_backward;
 * denoised_out (optional, device): D. */
typedef struct dm_edm_train_args {
    const float* images;
    const float* noise;
    const float* coef_host;
    int32_t coef_stride;
    float loss_scale;
    int32_t accumulate;
    int32_t B, H, W;
    float* loss_out_host;
    float* denoised_out;
    void* stream;
} dm_edm_train_args;
int dm_unet_loss_backward_edm(dm_unet* u, const dm_edm_train_args* args);

/* The three training passes on their own (tests); tensors as for the sampling passes above.
 *   noise_in:        x0 = 2 images - 1; noised = x0 + c[6] eps; xin = c[2] noised.  rows == 1 or rows == B.
 *   loss:            c_host holds B rows.  D = c[4] noised + c[5] F;  *loss_out_host = loss_scale * mean_b(c[14] mean((D - x0)^2));
 *                    dF = loss_scale * c[14] * c[5] * 2 (D - x0) / (B * per);  D_out (optional) = D.
 *   sinusoid_ft_bwd: e0, de0: (B, 2 half + 1) rows [t | sin | cos] of the float-time embedding and their gradient;
 *                    dw[k] (+)= sum_b 2 pi t_b (de_sin[b][k] cos[b][k] - de_cos[b][k] sin[b][k]), k < half, from the taped
 *                    values; learned == 0 writes zeros.  Enqueues only. */
int dm_op_edm_noise_in(const float* images, const float* eps, const float* c_host, int rows, float* x0, float* noised,
                       float* xin, int B, int64_t per, void* stream);
int dm_op_edm_loss(const float* noised, const float* F, const float* x0, const float* c_host, float loss_scale, float* dF,
                   float* D_out, float* loss_out_host, int B, int64_t per, void* stream);
int dm_op_sinusoid_ft_bwd(const float* de0, const float* e0, float* dw, int B, int half, int learned, int accumulate,
                          void* stream);

/* ---- Continuous-time Gaussian diffusion (DD/continuous_time_gaussian_diffusion.py: noise prediction;
 * DD/v_param_continuous_time_gaussian_diffusion.py: v prediction) -- the U-Net's time is log_snr(t), a float, so the handle
 * must have learned_sinusoidal_dim > 0 (both classes assert it), no text conditioning and out_dim == channels.
 *
 * Sampling (p_sample_loop of both classes).  The HOST evaluates every per-step scalar as the reference's own 0-dim fp32
 * tensor expression and passes n_steps rows of DM_CT_COEFS floats; step i runs Unet(x, c[0]) and one elementwise pass:
 *   c[0]=log_snr(t_i)                  c[1]=alpha=sqrt(sigmoid(c[0]))          c[2]=sigma=sqrt(sigmoid(-c[0]))
 *   c[3]=alpha_next                    c[4]=c=-expm1(log_snr - log_snr_next)   c[5]=1 - c
 *   c[6]=sqrt(sigmoid(-log_snr_next) * c), 0 on the step with time_next == 0 (p_sample returns the mean there)
 *   c[7]=alpha_next / alpha            c[8]=c * sigma                          (noise prediction without clipping)
 *   c[9]=loss weight (training rows only); unused entries are 0.
 *   objective  DM_CT_PRED_NOISE / DM_CT_PRED_V;   clip: clamp x_start to [-1, 1] (clip_sample_denoised)
 *     v:               x_start = c[1] x - c[2] F [clamped];       mean = c[3] (x c[5] / c[1] + c[4] x_start)
 *     noise, clip:     x_start = (x - c[2] F) / c[1], clamped;    the same mean
 *     noise, no clip:  mean = c[7] (x - c[8] F)
 *     x <- mean + c[6] eps
 *   x_init     (B,C,H,W) N(0,1) noise, the loop's start image (unscaled)
 *   noise      NULL -> device Philox noise (draw i + 1 at step i); else (n_steps - 1, B,C,H,W), row i read by step i.  A
 *              step whose c[6] == 0 reads neither; with a noise tensor the last row's c[6] must be 0.
 *   out        (clamp(x, -1, 1) + 1) / 2
 *   use_graph  one step is captured as a hipGraph, cached on the handle per (objective, clip, B, H, W, noise pointer) in
 *              the slot dm_sample / dm_sample_edm use. */
#define DM_CT_COEFS 16
#define DM_CT_PRED_NOISE 0
#define DM_CT_PRED_V 1
typedef struct dm_ct_args {
    int32_t objective;  /* DM_CT_PRED_* */
    int32_t clip;
    int32_t n_steps;
    const float* table_host;
    const float* x_init;
    const float* noise;
    uint64_t seed;
    uint64_t sample_offset;
    float* out;
    int32_t B, H, W;
    int32_t use_graph;
    void* stream;
} dm_ct_args;
int dm_sample_ct(dm_unet* u, const dm_ct_args* args);

/* DPM-Solver++ (2M: multistep, data prediction; arXiv 2211.01095, Algorithm 2) for the same two classes: a deterministic
 * few-step sampler of a model trained with dm_unet_loss_backward_ct.  The solver's half-log-SNR is lambda = log_snr / 2, so
 * the nodes l_0 > ... are log-SNR values themselves and the U-Net is fed the node; no inverse of the schedule is needed.
 * The HOST evaluates every scalar in float64 and rounds it to fp32 once; row i of the n_steps rows (DM_CT_COEFS floats) is
 *   c[0]=l_i   c[1]=alpha_i=sqrt(sigmoid(l_i))   c[2]=sigma_i=sqrt(sigmoid(-l_i))        (the meaning they have above)
 *   c[10]=c_x=sigma_{i+1} / sigma_i      c[11]=c_D=-alpha_{i+1} expm1(-h)      c[12]=g=h / (2 h_{i-1})
 *   with h = (l_{i+1} - l_i) / 2; g is 0 at order 1 and on row 0 (required); every other entry is 0.
 * Step i runs Unet(x, c[0]) and one elementwise pass:
 *   x_start = c[1] x - c[2] F (v) or (x - c[2] F) / c[1] (noise), clamped to [-1, 1] when clip
 *   D = x_start + c[12] (x_start - x_start of step i - 1)      (c[12] == 0: the history is not read)
 *   x <- c[10] x + c[11] D
 * so c[11] + c[10] alpha_i = alpha_{i+1} and c[10] sigma_i = sigma_{i+1}: with g == 0 the step is DDIM at eta = 0.  Nothing
 * is drawn after x_init; there is no special last row (log_snr(0) is finite, the last step lands on l_N).
 *   out        (clamp(x, -1, 1) + 1) / 2, as dm_sample_ct;   x_out (optional): the final x in front of that pass
 *   use_graph  one step is captured per (objective, clip, B, H, W) and serves any n_steps, order and node spacing; the
 *              graph is a kind of its own in the handle's slot, so dm_sample_ct's is captured again when the loops alternate.
 * The handle checks are those of dm_sample_ct (float time, no text or image condition, no sequence model). */
typedef struct dm_ct_dpmpp_args {
    int32_t objective;  /* DM_CT_PRED_* */
    int32_t clip;
    int32_t n_steps;
    const float* table_host;
    const float* x_init;
    float* out;
    float* x_out;       /* device (B,C,H,W) or NULL */
    int32_t B, H, W;
    int32_t use_graph;
    void* stream;
} dm_ct_dpmpp_args;
int dm_sample_ct_dpmpp(dm_unet* u, const dm_ct_dpmpp_args* args);

/* One p_losses (+ the normalisation of forward) and its backward pass on a handle armed by dm_unet_train_enable_ft:
 *   x0 = 2 images - 1 (normalize != 0: forward on images in [0, 1]) or images (normalize == 0: p_losses on x_start);
 *   x = x0 alpha_b + noise sigma_b;  F = Unet(x, log_snr_b);
 *   target = noise (DM_CT_PRED_NOISE) or alpha_b noise - sigma_b x0 (DM_CT_PRED_V);
 *   loss = loss_scale * mean_b( w_b * mean((F - target)^2) );  every parameter gradient.
 * coef_host: B rows of coef_stride floats (0: DM_CT_COEFS) with c[0] = log_snr_b, c[1] = alpha_b, c[2] = sigma_b and
 * c[9] = w_b (1, or min-SNR: clamp(snr_b, min = gamma) / snr_b).  loss_scale, accumulate and loss_out_host as in
 * dm_unet_loss_backward_edm. */
typedef struct dm_ct_train_args {
    const float* images;
    const float* noise;
    const float* coef_host;
    int32_t coef_stride;
    int32_t objective;
    float loss_scale;
    int32_t accumulate;
    int32_t B, H, W;
    int32_t normalize;
    float* loss_out_host;
    void* stream;
} dm_ct_train_args;
int dm_unet_loss_backward_ct(dm_unet* u, const dm_ct_train_args* args);

/* The passes on their own (tests).  c_host: rows == 1 (every image) or rows == B (row b for image b) in the layout
 * above; tensors are B * per floats, per % 4 == 0, 16-byte aligned; each call waits for its result.
 *   step:      as above on (x, F).  eps NULL: Philox draw `draw` (>= 1) under `seed`; a row with c[6] == 0 reads neither.
 *              x_start_out (optional) = x_start; it must be NULL for noise prediction without clipping.
 *   noise_in:  x0 = 2 images - 1 (normalize != 0) or images;  x = x0 c[1] + eps c[2];  target as above.
 *   loss:      c_host holds B rows.  *loss_out_host = loss_scale * mean_b(c[9] mean((F - target)^2));
 *              dF = loss_scale * c[9] * 2 (F - target) / (B * per).
 *   dpmpp_step: one pass of dm_sample_ct_dpmpp on (x, F) and a row with c[10..12]: out = the new x, hist (B * per device
 *              floats, aliasing no other tensor) = the new x_start; hist is read only where c[12] != 0. */
int dm_op_ct_dpmpp_step(const float* x, const float* F, float* hist, const float* c_host, int rows, int objective, int clip,
                        float* out, int B, int64_t per, void* stream);
int dm_op_ct_step(const float* x, const float* F, const float* eps, const float* c_host, int rows, int objective, int clip,
                  uint64_t seed, uint64_t draw, uint64_t element_offset, float* out, float* x_start_out, int B, int64_t per,
                  void* stream);
int dm_op_ct_noise_in(const float* images, const float* eps, const float* c_host, int rows, int objective, int normalize,
                      float* x, float* target, int B, int64_t per, void* stream);
int dm_op_ct_loss(const float* F, const float* target, const float* c_host, float loss_scale, float* dF,
                  float* loss_out_host, int B, int64_t per, void* stream);

/* The same call, and behind it the gradient of the loss with respect to the U-Net's INPUTS -- what a learned noise schedule
 * (DD/continuous_time_gaussian_diffusion.py:57-95: log_snr_b = net(t_b) reaches the loss through x = alpha_b x0 + sigma_b eps,
 * through the U-Net's time and through the loss weight) or any other differentiate-through-the-denoiser use needs:
 *   dX = dL/dx (B,C,H,W): the 7x7 input gradient of init_conv;   dt_b = dL/d(log_snr_b) through the time embedding;
 *   sched_out_host  (B, 4) floats, written after the call's own stream wait (NULL: not read back, nothing waited for it):
 *                   [ ga_b = sum dX x0 | gs_b = sum dX eps | dt_b | l_b = mean((F - target)^2), unweighted ]
 *                   (x0 the normalised image when normalize != 0).  With alpha, sigma, w functions of log_snr on the host,
 *                   d loss / d log_snr_b = ga_b alpha' + gs_b sigma' + dt_b + loss_scale l_b w' / B.
 *   dx_out, dtime_out   optional DEVICE buffers (B,C,H,W) / (B) that receive dX / dt.
 * The first 13 fields are dm_ct_train_args, field for field; loss, dF and every parameter gradient are what
 * dm_unet_loss_backward_ct produces on them.  The input-gradient kernels and their workspace exist in this entry only. */
typedef struct dm_ct_train_ig_args {
    const float* images;
    const float* noise;
    const float* coef_host;
    int32_t coef_stride;
    int32_t objective;
    float loss_scale;
    int32_t accumulate;
    int32_t B, H, W;
    int32_t normalize;
    float* loss_out_host;
    void* stream;
    float* sched_out_host;  /* (B, 4) host floats or NULL */
    float* dx_out;          /* device (B,C,H,W) or NULL */
    float* dtime_out;       /* device (B) or NULL */
} dm_ct_train_ig_args;
int dm_unet_loss_backward_ct_ig(dm_unet* u, const dm_ct_train_ig_args* args);

/* The three input-gradient passes on their own (tests); device tensors, each call waits for its result.
 *   conv7_dgrad:       dx (B,C,H,W) = input gradient of a 7x7 / pad 3 convolution from dy (B,Cout,H,W) and its
 *                      (Cout,C,7,7) weight; 1 <= C <= 8, any Cout; fp32, fixed accumulation order, every element of dx written.
 *   sinusoid_ft_tgrad: dt[b] = de0[b][0] + 2 pi sum_k freqs[k] (de_sin[b][k] cos[b][k] - de_cos[b][k] sin[b][k]) from the
 *                      taped rows e0[b] = [t | sin | cos] of width 2 half + 1 (layout of dm_op_sinusoid_ft_bwd).
 *   ct_sched_reduce:   out (B, 4) DEVICE rows [sum dx x0 | sum dx eps | dt[b], 0 when dt == NULL | mean((F - target)^2)],
 *                      x0 = 2 images - 1 (normalize != 0) or images; per % 4 == 0, 16-byte aligned tensors. */
int dm_op_conv7_dgrad(const float* dy_nchw, const float* weight, float* dx, int B, int H, int W, int Cout, int C, void* stream);
int dm_op_sinusoid_ft_tgrad(const float* de0, const float* e0, const float* freqs, float* dt, int B, int half, void* stream);
int dm_op_ct_sched_reduce(const float* dx, const float* images, const float* eps, const float* F, const float* target,
                          const float* dt, int normalize, float* out, int B, int64_t per, void* stream);

/* ---- RePaint inpainting (arXiv 2201.09865 as DD/repaint.py:614-681 has it): the DDPM loop over a trained U-Net with the
 * pixels where mask == 1 taken from a ground-truth image and the rest generated, and with "resampling" jumps back up the
 * chain.  The HOST unrolls the loop into n_rows rows, one U-Net evaluation each, and evaluates every scalar as the
 * reference's own 0-dim fp32 tensor expression; row r is DM_REPAINT_COEFS floats:
 *   c[0..7]  the DDPM row of dm_sample at the row's time t_r (DM_COEFS floats, same layout)
 *   c[8]=sqrt(alphas_cumprod[t_r])   c[9]=sqrt(1 - alphas_cumprod[t_r])         (the known region, noised to t_r)
 *   c[10]=sqrt(1 - betas[j])  c[11]=sqrt(betas[j])  c[12]=1 on a row that opens a resample iteration (j = resample_jump),
 *   else 1, 0, 0              c[13]=frame of all_steps the row's result goes to, or -1;  c[14], c[15] = 0
 * With g = 2 gt - 1 (applied whatever the caller's auto_normalize is, as the reference does) row r runs
 *   [x <- c[10] x + c[11] z_jump]                        when c[12] != 0
 *   x <- mask (c[8] g + c[9] z_known) + (1 - mask) x
 *   x <- the DDPM update of dm_sample (objective as there) on Unet(x, t_r), with z_step when c[5] != 0
 * and the last row ends with x <- mask g + (1 - mask) x.  The update of row r and the jump and blend of row r + 1 are one
 * kernel launch (the blend of row 0 is a launch of its own in front of the loop).
 *   times_host  n_rows int64 times;  table_host  n_rows x DM_REPAINT_COEFS floats
 *   x_T         (B,C,H,W) N(0,1) start image;  gt (B,C,H,W) in [0, 1];  mask (B,mask_channels,H,W), mask_channels 1 or C,
 *               any values (1 = known); all device pointers
 *   noise       NULL -> device Philox noise under `seed`: draw 0 is x_T (the caller's), row r draws 3r + 1 (jump), 3r + 2
 *               (known) and 3r + 3 (step); counters are global element indices as in dm_sample_ex (sample_offset).
 *               Else (n_rows, 3, B,C,H,W) with [r][0] = z_jump, [r][1] = z_known, [r][2] = z_step; unread entries are
 *               never touched.
 *   out         the result, (x + 1) / 2 when unnormalize != 0
 *   all_steps   NULL or (n_frames, B,C,H,W): frame 0 = x_T, frame c[13] = the row's result before the next row's jump
 *               and blend (never unnormalised)
 *   use_graph   one row is captured as a hipGraph, cached on the handle per (objective, mask_channels, B, H, W, noise and
 *               all_steps pointers) in the slot dm_sample uses; seed, offset, tables, row count, unnormalize, gt and mask
 *               values are device data and do not re-capture. */
#define DM_REPAINT_COEFS 16
#define DM_REPAINT_AUTO 0
#define DM_REPAINT_BLEND 1
#define DM_REPAINT_STEP 2
#define DM_REPAINT_STEP_NEXT 3
#define DM_REPAINT_LAST 4
typedef struct dm_repaint_args {
    int32_t objective;  /* DM_OBJ_* */
    int32_t n_rows;
    const int64_t* times_host;
    const float* table_host;
    const float* x_T;
    const float* noise;
    uint64_t seed;
    uint64_t sample_offset;
    const float* gt;
    const float* mask;
    int32_t mask_channels;
    int32_t unnormalize;
    float* out;
    float* all_steps;
    int32_t n_frames;
    int32_t B, H, W;
    int32_t use_graph;
    void* stream;
} dm_repaint_args;
int dm_sample_repaint(dm_unet* u, const dm_repaint_args* args);

/* The fused kernel on plain buffers for one row (tests, p_sample); tensors are (B,C,HW) floats, the mask (B,mask_channels,HW);
 * the call waits for its result.  c_host is the row's table row, followed by the next row's for DM_REPAINT_STEP_NEXT.
 *   DM_REPAINT_BLEND      out = mask (c[8] g + c[9] z_known) + (1 - mask) x               (eps may be NULL)
 *   DM_REPAINT_STEP       out = the DDPM update of (x, eps) with c[0..7] and z_step      (gt and mask may be NULL)
 *   DM_REPAINT_STEP_NEXT  that update, then the next row's jump and blend with c[16 + 8 .. 16 + 12]
 *   DM_REPAINT_LAST       that update, then out = mask g + (1 - mask) out, (out + 1) / 2 when unnormalize != 0
 * z_jump, z_known, z_step all NULL: the Philox draws of row `row` (of row + 1 for the jump and blend of STEP_NEXT) under
 * `seed`, element counters starting at element_offset (a multiple of 4).  Else the draws the row reads must be given.
 * x_start_out (optional) = the clamped x_start of the update.  out may be x. */
int dm_op_repaint_step(int mode, int objective, const float* x, const float* eps, const float* gt, const float* mask,
                       int mask_channels, const float* z_jump, const float* z_known, const float* z_step, const float* c_host,
                       int unnormalize, uint64_t seed, uint64_t row, uint64_t element_offset, float* out, float* x_start_out,
                       int B, int C, int HW, void* stream);

/* ---- LearnedGaussianDiffusion (Improved DDPM, arXiv 2102.09672, as DD/learned_gaussian_diffusion.py:61-146 has it): the
 * U-Net predicts 2 * channels maps per image (out_dim == 2 * channels, :70) -- the noise, then a per-pixel weight v that
 * interpolates between the two extreme posterior log-variances.  The handle has no text conditioning, an integer time and
 * input channels == channels (no self-conditioning, :71).
 *
 * Sampling (the base class's p_sample_loop, DD/denoising_diffusion.py:647-664, over p_mean_variance :93-111).  The HOST
 * gathers every per-step scalar in fp32 as `extract` does; row i is DM_LV_COEFS floats at the step's time t_i:
 *   c[0]=sqrt_recip_alphas_cumprod   c[1]=sqrt_recipm1_alphas_cumprod   c[2]=posterior_mean_coef1   c[3]=posterior_mean_coef2
 *   c[4]=min_log=posterior_log_variance_clipped   c[5]=1 if t_i > 0 else 0   c[6]=max_log=log(betas);  the rest 0.
 * Step i runs (eps | v) = Unet(x, t_i) and one elementwise pass:
 *   logvar = (v + 1) / 2 * c[6] + (1 - (v + 1) / 2) * c[4];   x_start = clamp(c[0] x - c[1] eps, -1, 1)
 *   x <- c[2] x_start + c[3] x + exp(0.5 logvar) * z          (z = 0 where c[5] == 0)
 * The first half is read as noise whatever the object's `objective` says, as in the reference.
 *   times_host  n_steps int64 times;  table_host  n_steps x DM_LV_COEFS floats
 *   x_T         (B,C,H,W) N(0,1) start image (device)
 *   noise       NULL -> device Philox noise under `seed` (draw 0 is x_T, the caller's; step i draws i + 1; counters are
 *               global element indices as in dm_sample_ex: sample_offset).  Else (n_steps, B,C,H,W), row i read by step i
 *               when its c[5] != 0.
 *   out         the result, (x + 1) / 2 when unnormalize != 0 (written by the last step's pass)
 *   all_steps   NULL or (n_steps + 1, B,C,H,W): frame 0 = x_T, frame i + 1 = x after step i (never unnormalised)
 *   use_graph   one step is captured as a hipGraph, cached on the handle per (B, H, W, noise and all_steps pointers) in
 *               the slot dm_sample uses, under a kind of its own; seed, offset, tables, step count and unnormalize are
 *               device data and do not re-capture. */
#define DM_LV_COEFS 16
typedef struct dm_lv_args {
    int32_t n_steps;
    const int64_t* times_host;
    const float* table_host;
    const float* x_T;
    const float* noise;
    uint64_t seed;
    uint64_t sample_offset;
    float* out;
    float* all_steps;
    int32_t B, H, W;
    int32_t unnormalize;
    int32_t use_graph;
    void* stream;
} dm_lv_args;
int dm_sample_lv(dm_unet* u, const dm_lv_args* args);

/* One p_losses (:113-146) and its backward pass on a handle armed by dm_unet_train_enable (which accepts
 * out_dim == 2 * channels; dm_unet_loss_backward* refuse such a handle and name this call):
 *   x_t = c[0] x_start + c[1] noise;  (pred | v) = Unet(x_t, t_b);  logvar as above from c[6] (min_log), c[8] (max_log);
 *   model_mean = c[4] x0 + c[5] x_t, x0 = c[2] x_t - c[3] pred [clamped when clip_denoised];  true_mean = c[4] x_start + c[5] x_t
 *   vb_b = meanflat(c[9] ? -discretized_gaussian_log_likelihood(x_start, model_mean, 0.5 logvar)
 *                        : normal_kl(true_mean, c[7], model_mean, logvar)) / ln 2           (an image runs its own branch only)
 *   loss = loss_scale * (mean((pred - noise)^2) + vb_loss_weight * mean_b(vb_b));  every parameter gradient.
 * The model mean is detached (:128): the vb term's gradient reaches only the variance half of the output, the MSE's only
 * the noise half.  coef_host: B rows of coef_stride floats (0: DM_LV_TRAIN_COEFS; 10 to 12):
 *   c[0]=sqrt_alphas_cumprod[t_b]  c[1]=sqrt_one_minus_alphas_cumprod[t_b]  c[2]=sqrt_recip_alphas_cumprod[t_b]
 *   c[3]=sqrt_recipm1_alphas_cumprod[t_b]  c[4]=posterior_mean_coef1[t_b]  c[5]=posterior_mean_coef2[t_b]
 *   c[6]=c[7]=posterior_log_variance_clipped[t_b] (min_log; the true log variance)  c[8]=log(betas)[t_b]  c[9]=1 if t_b == 0
 * loss_scale, accumulate, loss_out_host (NULL: the loss stays on the device, dm_unet_train_scalar) as in
 * dm_unet_loss_backward_ex; model_out (optional, device) receives the (B, 2C, H, W) model output. */
#define DM_LV_TRAIN_COEFS 12
typedef struct dm_lv_train_args {
    const float* x_start;
    const int64_t* t_host;
    const float* coef_host;
    int32_t coef_stride;
    const float* noise;
    float vb_loss_weight;
    int32_t clip_denoised;
    float loss_scale;
    int32_t accumulate;
    float* loss_out_host;
    float* model_out;
    int32_t B, H, W;
    void* stream;
} dm_lv_train_args;
int dm_unet_loss_backward_lv(dm_unet* u, const dm_lv_train_args* args);

/* The two kernels on their own (tests, p_sample, p_mean_variance).  Tensors are on the device, B * per floats (model_out and
 * dout 2 * B * per: image b's noise half, then its variance half), per % 4 == 0, 16-byte aligned; tables are on the host;
 * each call waits for its result.
 *   step:  one row of DM_LV_COEFS floats.  z NULL: Philox draw `draw` (>= 1) under `seed`, counters from element_offset;
 *          a row with c[5] == 0 reads neither.  out may be x.  mean_out, logvar_out, x_start_out (optional) are
 *          p_mean_variance's model_mean, model_log_variance and clamped x_start.
 *   loss:  B rows of DM_LV_TRAIN_COEFS floats.  *loss_out_host = the loss above; mse_part_out_host / vb_part_out_host
 *          (optional, B floats on the host) = mean((pred_b - noise_b)^2) and vb_b;  dout = d loss / d model_out. */
int dm_op_lv_step(const float* x, const float* model_out, const float* z, const float* c_host, uint64_t seed, uint64_t draw,
                  uint64_t element_offset, float* out, float* mean_out, float* logvar_out, float* x_start_out, int B,
                  int64_t per, void* stream);
int dm_op_lv_loss(const float* model_out, const float* x_start, const float* noise, const float* x_t, const float* c_host,
                  float vb_loss_weight, int clip_denoised, float loss_scale, float* dout, float* loss_out_host,
                  float* mse_part_out_host, float* vb_part_out_host, int B, int64_t per, void* stream);

/* ---- WeightedObjectiveGaussianDiffusion (DD/weighted_objective_gaussian_diffusion.py:14-74): the U-Net predicts
 * 2 * channels + 2 maps per image (out_dim == 2 * channels + 2, :25) -- the noise eps (C maps), x_start px (C maps) and two
 * weight maps w0, w1.  The softmax over the pair, s0 = sigmoid(w0 - w1), s1 = 1 - s0, blends the x_start derived from the
 * noise with the predicted one, pixel by pixel.  The handle has no text conditioning, an integer time, input channels ==
 * channels (no self-conditioning, :26) and out_dim <= 8 (channels <= 3: the thin-output final_conv kernels stop there).
 *
 * Sampling (the base class's p_sample_loop, DD/denoising_diffusion.py:647-664, over p_mean_variance :33-49; the reference's
 * own p_sample passes x_self_cond and unpacks four values, which this p_mean_variance does not take: the loop here calls it
 * with (x, t, clip_denoised = True) and takes its three values).  The HOST gathers every per-step scalar in fp32 as
 * `extract` does; row i is DM_WO_COEFS floats at the step's time t_i:
 *   c[0]=sqrt_recip_alphas_cumprod   c[1]=sqrt_recipm1_alphas_cumprod   c[2]=posterior_mean_coef1   c[3]=posterior_mean_coef2
 *   c[4]=posterior_log_variance_clipped   c[5]=1 if t_i > 0 else 0;  the rest 0.
 * Step i runs (eps | px | w0 | w1) = Unet(x, t_i) and one elementwise pass:
 *   x_start = clamp(s0 (c[0] x - c[1] eps) + s1 px, -1, 1);   x <- c[2] x_start + c[3] x + exp(0.5 c[4]) * z   (z = 0 where c[5] == 0)
 * Every field is dm_lv_args': times_host, table_host (n_steps x DM_WO_COEFS), x_T, noise, seed, sample_offset, out,
 * all_steps, unnormalize, use_graph (cached in the slot dm_sample uses, under a kind of its own), stream.  H * W % 4 == 0. */
#define DM_WO_COEFS 16
typedef struct dm_wo_args {
    int32_t n_steps;
    const int64_t* times_host;
    const float* table_host;
    const float* x_T;
    const float* noise;
    uint64_t seed;
    uint64_t sample_offset;
    float* out;
    float* all_steps;
    int32_t B, H, W;
    int32_t unnormalize;
    int32_t use_graph;
    void* stream;
} dm_wo_args;
int dm_sample_wo(dm_unet* u, const dm_wo_args* args);

/* One p_losses (:51-74) and its backward pass on a handle armed by dm_unet_train_enable (dm_unet_loss_backward* refuse such
 * a handle and name this call).  With N = B C H W:
 *   x_t = c[0] x_start + c[1] noise;  (pn | px | w0 | w1) = Unet(x_t, t_b);  xs = c[2] x_t - c[3] pn;  xc = clamp(xs, -2, 2)
 *   wx = s0 xc + s1 px
 *   loss = loss_scale * (mean((x_start - wx)^2) + pred_x_start_loss_weight * mean((x_start - px)^2)
 *                        + pred_noise_loss_weight * mean((noise - pn)^2));  every parameter gradient, from
 *   d pn = 2 / N [w_n (pn - noise) - (wx - x_start) s0 c[3] (-2 <= xs <= 2)]     (torch's clamp passes the gradient on the bounds)
 *   d px = 2 / N [w_x (px - x_start) + (wx - x_start) s1]
 *   d w0 = 2 / N sum_c (wx - x_start) (xc - px) s0 s1;   d w1 = -d w0
 * coef_host: B rows of coef_stride floats (0: DM_WO_TRAIN_COEFS; 4 to 12):
 *   c[0]=sqrt_alphas_cumprod[t_b]  c[1]=sqrt_one_minus_alphas_cumprod[t_b]  c[2]=sqrt_recip_alphas_cumprod[t_b]
 *   c[3]=sqrt_recipm1_alphas_cumprod[t_b];  the rest 0.
 * loss_scale, accumulate, loss_out_host (NULL: the loss stays on the device, dm_unet_train_scalar) as in
 * dm_unet_loss_backward_ex; model_out (optional, device) receives the (B, 2C + 2, H, W) model output. */
#define DM_WO_TRAIN_COEFS 12
typedef struct dm_wo_train_args {
    const float* x_start;
    const int64_t* t_host;
    const float* coef_host;
    int32_t coef_stride;
    const float* noise;
    float pred_noise_loss_weight;
    float pred_x_start_loss_weight;
    float loss_scale;
    int32_t accumulate;
    float* loss_out_host;
    float* model_out;
    int32_t B, H, W;
    void* stream;
} dm_wo_train_args;
int dm_unet_loss_backward_wo(dm_unet* u, const dm_wo_train_args* args);

/* The two kernels on their own (tests, p_sample, p_mean_variance).  Tensors are on the device: x, z, out, mean_out,
 * x_start_out, x_start, noise, x_t are (B, C, HW); model_out and dout (B, 2C + 2, HW); HW % 4 == 0, 16-byte aligned; tables
 * are on the host; each call waits for its result.
 *   step:  one row of DM_WO_COEFS floats.  clip_denoised != 0 clamps the weighted x_start to [-1, 1] (p_sample always
 *          does).  z NULL: Philox draw `draw` (>= 1) under `seed`, the counter of element b C HW + c HW + p from
 *          element_offset; a row with c[5] == 0 reads neither.  out may be x.  mean_out, x_start_out (optional) are
 *          p_mean_variance's model_mean and the weighted x_start.
 *   loss:  B rows of DM_WO_TRAIN_COEFS floats.  *loss_out_host = the loss above; weighted_part / x_start_part / noise_part
 *          (optional, B floats on the host) = the three per-image means, unweighted;  dout = d loss / d model_out. */
int dm_op_wo_step(const float* x, const float* model_out, const float* z, const float* c_host, int clip_denoised, uint64_t seed,
                  uint64_t draw, uint64_t element_offset, float* out, float* mean_out, float* x_start_out, int B, int C,
                  int64_t HW, void* stream);
int dm_op_wo_loss(const float* model_out, const float* x_start, const float* noise, const float* x_t, const float* c_host,
                  float pred_noise_loss_weight, float pred_x_start_loss_weight, float loss_scale, float* dout,
                  float* loss_out_host, float* weighted_part_out_host, float* x_start_part_out_host,
                  float* noise_part_out_host, int B, int C, int64_t HW, void* stream);

/* ---- Classifier-guided DDPM sampling (Sohl-Dickstein et al. 2015; Dhariwal & Nichol 2021; as DD/guided_diffusion.py:553-603
 * has it): after the U-Net has produced the posterior mean, the caller's cond_fn returns grad log p(y | x) AT THAT MEAN, the
 * mean is shifted by posterior_variance[t] * gradient, and the noise is added after that.  The handle has no text
 * conditioning, no image condition, an integer time and out_dim == channels; self-conditioning and the three objectives
 * are served.  Text, image condition and classifier-free guidance are refused with a message.
 *
 * The HOST gathers every per-step scalar; row i is DM_CG_COEFS floats: columns 0..7 are the DDPM row of dm_sample as it is
 * (c[4] = exp(0.5 posterior_log_variance_clipped), c[5] = 1 if t_i > 0 else 0), c[8] = posterior_variance[t_i] (unclipped:
 * 0 at t == 0, where the gradient has no effect), the rest 0.  Step i is two device halves with the host in between:
 *   front  [self-conditioning input]  model_out = Unet(x, t_i [, x_start]);  x_start = clamp(x_0 by objective, -1, 1);
 *          mean = c[2] x_start + c[3] x                                             (cg_mean_kernel writes `mean`)
 *   host   the run's stream is synchronised, then cond_cb(user, i, t_i) is called on the calling thread.  It reads `mean`,
 *          writes `grad`, and returns 0 only when `grad` is complete on the device (it synchronises whatever stream it used).
 *          A non-zero return ends the loop: the call fails with a message and launches nothing more; the handle stays usable.
 *   back   x <- (mean + c[8] grad) + c[4] z   (z = 0 where c[5] == 0)                (cg_finish_kernel)
 * The x_start that self-conditioning feeds to the next step is the unguided one.  With a zero gradient the result equals
 * dm_sample's DDPM loop bit for bit (same Philox draws: step i draws i + 1).
 *   objective, self_condition   as in dm_sample_args
 *   times_host  n_steps int64 times;  table_host  n_steps x DM_CG_COEFS floats
 *   x_T, noise, seed, sample_offset, out, all_steps, unnormalize   as in dm_lv_args
 *   mean, grad  caller-owned (B,C,H,W) device tensors, 16-byte aligned, distinct; they live until the call returns
 *   cond_cb     the callback above;  user  passed through to it
 *   stream      the stream of the call; with use_graph and the legacy default stream (NULL) the call runs on a stream of the
 *               handle, as dm_sample does.  Either way `mean` is complete when cond_cb is entered.
 *   use_graph   the two halves are captured once each into the handle's two graph slots, cached per (B, H, W, objective,
 *               self_condition, mean, grad, noise and all_steps pointers) under a kind of their own; seed, offset, tables,
 *               step count and unnormalize are device data and do not re-capture. */
#define DM_CG_COEFS 16
typedef struct dm_cguide_args {
    int32_t objective;
    int32_t self_condition;
    int32_t n_steps;
    int32_t reserved_;
    const int64_t* times_host;
    const float* table_host;
    const float* x_T;
    const float* noise;
    uint64_t seed;
    uint64_t sample_offset;
    float* mean;
    float* grad;
    int (*cond_cb)(void* user, int step, int64_t t);
    void* user;
    float* out;
    float* all_steps;
    int32_t B, H, W;
    int32_t unnormalize;
    int32_t use_graph;
    int32_t reserved2_;
    void* stream;
} dm_cguide_args;
int dm_sample_classifier_guided(dm_unet* u, const dm_cguide_args* args);

/* The two kernels on their own (tests, p_sample, condition_mean).  Tensors are on the device, B * per floats, per % 4 == 0,
 * 16-byte aligned; c_host is one row of DM_CG_COEFS floats on the host; each call waits for its result.
 *   mean:    mean = c[2] x_start + c[3] x with x_start as above; x_start_out (optional).  The outputs alias nothing.
 *   finish:  out = (mean + c[8] grad) + c[4] z.  z NULL: Philox draw `draw` (>= 1) under `seed`, counters from
 *            element_offset; a row with c[5] == 0 reads neither.  out may be mean.  guided_out (optional) = mean + c[8] grad. */
int dm_op_cg_mean(const float* x, const float* model_out, const float* c_host, int objective, float* mean, float* x_start_out,
                  int B, int64_t per, void* stream);
int dm_op_cg_finish(const float* mean, const float* grad, const float* z, const float* c_host, uint64_t seed, uint64_t draw,
                    uint64_t element_offset, float* out, float* guided_out, int B, int64_t per, void* stream);

/* ---- Bits-per-dim evaluation: the variational bound of a batch of real images (Improved DDPM, arXiv 2102.09672:
 * calc_bpd_loop / _vb_terms_bpd / _prior_bpd), written with the functions of DD/denoising_diffusion.py and
 * DD/learned_gaussian_diffusion.py.  Not in the reference.  x0 is the normalised image.  The HOST gathers every per-step
 * scalar in fp32 as `extract` does; row i is DM_BPD_COEFS floats at the step's time t_i:
 *   c[0]=sqrt_recip_alphas_cumprod   c[1]=sqrt_recipm1_alphas_cumprod   c[2]=posterior_mean_coef1   c[3]=posterior_mean_coef2
 *   c[4]=posterior_log_variance_clipped   c[5]=1 if t_i == 0 else 0   c[6]=sqrt_alphas_cumprod
 *   c[7]=sqrt_one_minus_alphas_cumprod   c[8]=log(betas);  the rest 0.
 * Step i, per image b (every step draws z, t_i == 0 included):
 *   x_t = c[6] x0 + c[7] z;   model_out = Unet(x_t, t_i [, ctx] [, cond behind x_t])
 *   pred = x_start by objective from (x_t, model_out) [clamped to [-1, 1] when clip_denoised];  model_mean = c[2] pred + c[3] x_t
 *   logvar = c[4], or with `learned` (model_out = (eps | v), objective pred_noise) (v + 1) / 2 * c[8] + (1 - (v + 1) / 2) * c[4]
 *   true_mean = c[2] x0 + c[3] x_t
 *   terms_out[i][b][0] = meanflat(c[5] ? -discretized_gaussian_log_likelihood(x0, model_mean, 0.5 logvar)
 *                                      : normal_kl(true_mean, c[4], model_mean, logvar)) / ln 2
 *   terms_out[i][b][1] = meanflat((pred - x0)^2)
 *   terms_out[i][b][2] = meanflat(((c[0] x_t - pred) / c[1] - z)^2)
 * and once per call  prior_out[b] = meanflat(normal_kl(prior_sqrt_ac x0, prior_logvar, 0, 0)) / ln 2  (the caller passes
 * sqrt_alphas_cumprod[T - 1] and log(1 - alphas_cumprod[T - 1])).
 * Sums run in double in a fixed order, by image: a result does not depend on the batch around it, nor on use_graph.
 * The prior term is formed in double as a whole (its fp32 expression cancels to the last ulp of expf).
 *   learned        1: the U-Net of LearnedGaussianDiffusion (out_dim == 2 * channels);  0: out_dim == channels
 *   objective      DM_OBJ_* (pred_noise with `learned`)
 *   times_host     n_steps int64 times;  table_host  n_steps x DM_BPD_COEFS floats
 *   x0             (B,C,H,W) device, C * H * W % 4 == 0
 *   noise          NULL -> device Philox noise under `seed` (step i draws i + 1; counters are global element indices:
 *                  sample_offset is the index of the call's first image in a global batch).  Else (n_steps, B,C,H,W).
 *   ctx, cond      as in dm_sample_args (text context; the image condition behind x_t)
 *   terms_out      (n_steps, B, 3) device;  prior_out  NULL or (B) device
 *   use_graph      one step is captured as a hipGraph, cached on the handle per (B, H, W, learned, objective,
 *                  clip_denoised, ctx_tokens, cond_channels, noise pointer) in the slot dm_sample uses, under a kind of its
 *                  own; times, tables, step count, seed and offset are device data and do not re-capture. */
#define DM_BPD_COEFS 16
#define DM_BPD_CHUNK 1024 /* elements of an image that one workgroup of the term kernel sums */
typedef struct dm_bpd_args {
    int32_t learned;
    int32_t objective;
    int32_t clip_denoised;
    int32_t n_steps;
    const int64_t* times_host;
    const float* table_host;
    const float* x0;
    const float* noise;
    uint64_t seed;
    uint64_t sample_offset;
    const float* ctx;
    int32_t ctx_tokens;
    int32_t cond_channels;
    const float* cond;
    float prior_sqrt_ac;
    float prior_logvar;
    float* terms_out;
    float* prior_out;
    int32_t B, H, W;
    int32_t use_graph;
    void* stream;
} dm_bpd_args;
int dm_eval_bpd(dm_unet* u, const dm_bpd_args* args);

/* The kernels on their own.  Tensors are on the device, B * per floats (model_out 2 * B * per with `learned`: image b's
 * prediction half, then its variance half), per % 4 == 0, 16-byte aligned; c_host is one row of DM_BPD_COEFS floats on the host.
 *   step_in:  x_t = c[6] x0 + c[7] z.  z NULL: Philox draw `draw` (>= 1) under `seed`, counters from element_offset.
 *   terms:    terms_out_host (B, 3) on the host, as terms_out[i] above, from the given model_out, x0, x_t and z.
 *   prior:    prior (B) on the device, as prior_out above; the call does not wait.
 * step_in and terms wait for their result. */
int dm_op_bpd_step_in(const float* x0, const float* z, const float* c_host, uint64_t seed, uint64_t draw, uint64_t element_offset,
                      float* x_t, int B, int64_t per, void* stream);
int dm_op_bpd_terms(const float* model_out, const float* x0, const float* x_t, const float* z, const float* c_host, int learned,
                    int objective, int clip_denoised, float* terms_out_host, int B, int64_t per, void* stream);
int dm_op_bpd_prior(const float* x0, float sqrt_ac, float logvar, float* prior, int B, int64_t per, void* stream);

/* ---- KarrasUnet: the EDM2 magnitude-preserving U-Net (DD/karras_unet.py:374-595; arXiv 2312.02696, config G) ------------
 *
 * A second network body behind the dm_unet handle.  dm_kunet_create returns a handle that dm_unet_set_param,
 * dm_unet_get_param_host, dm_unet_update_param, dm_unet_refresh, dm_unet_finalize, dm_unet_missing_params,
 * dm_unet_workspace_bytes, dm_unet_graph_captures and dm_unet_destroy serve as they serve an image U-Net's; the parameter
 * names and shapes are the reference's state_dict() ("input_block.weight" (dim, input_channels + 1, 3, 3),
 * "downs.3.block1.1.weight", "downs.3.to_emb.1.gain" (), "ups.0.attn.mem_kv" (2, heads, 4, dh), "to_time_emb.0.weights", ...).
 * The time of this network is real-valued: the handle runs dm_unet_forward_ft and dm_sample_edm (both kinds; the network
 * must then have input_channels == channels).  dm_unet_forward, every other dm_sample* loop, dm_eval_bpd and
 * dm_unet_train_enable* return an error and leave the handle usable.  H and W of every call are image_size.
 *
 * Every magnitude-preserving constant (forced weight normalisation, MPSiLU's 1 / 0.596, MPAdd, MPCat, Gain) is folded into
 * the packed weights at dm_unet_finalize / dm_unet_refresh, on the host, in double. */
typedef struct dm_kunet_cfg {
    int32_t image_size;
    int32_t dim;
    int32_t dim_max;
    int32_t num_classes;    /* 0 = no class condition */
    int32_t channels;
    int32_t input_channels; /* channels, or 2 channels with self-conditioning (the caller concatenates self_cond in front) */
    int32_t num_downsamples;
    int32_t num_blocks_per_stage;
    int32_t n_attn_res;
    int32_t attn_res[DM_MAX_STAGES]; /* resolutions whose blocks end in an attention layer */
    int32_t fourier_dim;
    int32_t attn_dim_head;  /* 32 or 64; heads of a layer = max(ceil(dim_out / attn_dim_head), 2) */
    float mp_cat_t;
    float mp_add_emb_t;
    float attn_res_mp_add_t;
    float resnet_mp_add_t;
} dm_kunet_cfg;
int dm_kunet_create(const dm_kunet_cfg* cfg, int device, dm_unet** out);
/* The class labels of the next calls with batch B on a handle with num_classes: labels_dev (B, num_classes) device floats,
 * ALREADY multiplied by sqrt(num_classes) (one-hot rows of integer labels, or soft labels).  They are copied into a buffer
 * of the handle that the conditioning head reads as device data: a captured step graph serves any labels.  The call
 * synchronises the device. */
int dm_kunet_set_class_labels(dm_unet* u, const float* labels_dev, int B);

/* The network's own kernels and blocks on their own (tests).  Device pointers; every call waits for its result.
 * The row passes take tensors as the library holds them (NHWC: rows of C channels, C % 4 == 0):
 *   pixelnorm:     y = x / max(||x||, 1e-4) sqrt(C) per row -> res_out = y res_scale, act_out = silu(y) (each may be NULL)
 *   avgpool2:      (B, H, W, C) -> (B, H/2, W/2, C), the 2x2 mean
 *   bilinear_up2:  (B, H, W, C) -> x_up (B, 2H, 2W, C) with 0.25 / 0.75 taps and edge clamp: up_out = x_up,
 *                  act_out = silu(x_up), res_out = x_up res_scale (each may be NULL)
 *   act:           act_out (rows, Ca + Cb) = cat(silu(ca a), silu(cb b)) (b NULL: Cb = 0), copy_out (rows, Ca) = a copy_scale
 *   attention:     qkv (B, n, 3 heads dh) as to_qkv leaves it, mem_kv (2, heads, 4, dh) as stored -> out (B, n, heads dh):
 *                  q, k, v and the memory rows pixel-normed along dh, softmax(q k^T dh^-0.5) v */
int dm_op_kunet_pixelnorm(const float* x, float* res_out, float* act_out, int64_t rows, int C, float res_scale, void* stream);
int dm_op_kunet_avgpool2(const float* x, float* y, int B, int H, int W, int C, void* stream);
int dm_op_kunet_bilinear_up2(const float* x, float* up_out, float* act_out, float* res_out, int B, int H, int W, int C,
                             float res_scale, void* stream);
int dm_op_kunet_act(const float* a, int Ca, float ca, const float* b, int Cb, float cb, float* act_out, float* copy_out,
                    float copy_scale, int64_t rows, void* stream);
int dm_op_kunet_attention(const float* qkv, const float* mem_kv, float* out, int B, int n, int heads, int dh, void* stream);
/* The conditioning head.  time (B) floats; labels (B, num_classes) already times sqrt(num_classes), or NULL with
 * num_classes = 0 (then class_w is NULL too); fourier_w (fourier_dim / 2), time_w (emb_dim, fourier_dim), class_w
 * (emb_dim, num_classes) as stored; to_emb_w: the to_emb.0.weight matrices of n_blocks blocks one behind the other
 * ((sum dout, emb_dim) rows) with their widths dout_host and gains gain_host (host arrays).  out (B, 2 sum dout): per block
 * dout values gain * to_emb(emb), then dout zeros -- the scale / shift rows the convolution epilogue reads. */
int dm_op_kunet_head(const float* time, const float* labels, const float* fourier_w, const float* time_w, const float* class_w,
                     const float* to_emb_w, const int32_t* dout_host, const float* gain_host, int n_blocks, int fourier_dim,
                     int emb_dim, int num_classes, float mp_add_emb_t, float* out, int B, void* stream);
/* input_block (x (B, C, H, W), weight (dim, C + 1, 3, 3)) and output_block (x (B, dim, H, W), weight (channels, dim, 3, 3),
 * the gain): NCHW in and out, weights as stored. */
int dm_op_kunet_input_block(const float* x, const float* weight, float* out, int B, int C, int H, int W, int dim, void* stream);
int dm_op_kunet_output_block(const float* x, const float* weight, float gain, float* out, int B, int dim, int H, int W,
                             int channels, void* stream);
/* One Encoder (decoder = 0; down: the downsampling form) or Decoder (decoder = 1; up: the upsampling form; skip: it takes the
 * skip tensor, whose skip_channels are the last of its din input channels), with attention behind it when attn != 0.  NCHW
 * tensors, weights as stored (NULL where the form has none: down_w, res_w -- a Decoder has a res_conv iff din != dout --,
 * mem_kv / qkv_w / out_w).  emb_scale (B, dout) = gain * to_emb(emb), as the head produces it.  out (B, dout, Ho, Wo). */
typedef struct dm_kunet_block_op {
    int32_t decoder, down, up, skip, attn;
    int32_t din, dout, skip_channels, dh;
    float mp_cat_t, attn_res_mp_add_t, resnet_mp_add_t;
    const float* x;
    const float* skip_x;
    const float* emb_scale;
    const float* down_w;
    const float* w1;
    const float* w2;
    const float* res_w;
    const float* mem_kv;
    const float* qkv_w;
    const float* out_w;
    float* out;
    int32_t B, H, W;
} dm_kunet_block_op;
int dm_op_kunet_block(const dm_kunet_block_op* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DM_HIP_H */
