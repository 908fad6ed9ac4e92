/* ld_mi355x.h — C ABI of the MI355X-native SD1.5 denoise hot path (libld_mi355x.so).
 *
 * Plain C: opaque handles, raw DEVICE pointers, sizes, a hipStream_t passed as void*.  No torch types.
 * Every function returns an LD_* status (0 = OK); nothing throws across the boundary.  After `*_reserve`
 * a handle performs no allocation: `ld_unet_forward` / `ld_vae_decode` only enqueue kernels on the given
 * stream (safe to capture into a hipGraph: fixed workspace addresses, no host sync, no malloc).
 *
 * What each entry point replaces in the reference (file:line into LightDiffusion.py = LD.py):
 *   ld_unet_forward      BaseModel.apply_model (LD.py:5828-5860) = EPS.calculate_input (1259-1261) →
 *                        ModelSamplingDiscrete.timestep (1336-1339) → UNetModel1.forward (5688-5767) →
 *                        EPS.calculate_denoised (1263-1265); i.e. what a `model_function_wrapper`
 *                        (LD.py:2558-2567, installed by ModelPatcher.set_model_unet_function_wrapper 3277)
 *                        must return: denoised x0, fp32, same shape as the input.
 *   ld_unet_set_context  the per-layer to_k / to_v projections of the cross-attention context
 *                        (CrossAttention.forward LD.py:4028-4036) — step-invariant, so hoisted out of the step.
 *   ld_vae_decode        VAE.decode (LD.py:6357-6381) = post_quant_conv + Decoder.forward (3470-3473, 3857-3882)
 *                        + process_output clamp + NCHW→NHWC.
 *   ld_esrgan_forward    RRDBNet.forward (LD.py:7025-7234), the model ImageUpscaleWithModel.upscale applies per tile (LD.py:7356-7395).
 *   ld_taesd_decode      TAESD.decode (LD.py:749-754) on Decoder2 (714-721), the latent preview taesd_preview shows per sampler step (761-768).
 *   ld_op_*              single operators, for parity tests: the `operations=` classes of LD.py:2342-2429
 *                        (Linear / Conv2d / GroupNorm / LayerNorm) and optimized_attention (3966-3988).
 */
#ifndef LD_MI355X_H
#define LD_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LD_OK 0
#define LD_ERR_ARG 1    /* null / inconsistent argument */
#define LD_ERR_SHAPE 2  /* shape or alignment not supported by the kernels */
#define LD_ERR_HIP 3    /* a HIP call or launch failed */
#define LD_ERR_STATE 4  /* call order (missing weights / reserve / context) */

#define LD_F16 0
#define LD_F32 1

/* whose launch a convolution operator reproduces (ld_op_conv, ld_op_conv_gn_partials, ld_op_groupnorm_conv): the scratch it plans under and the
 * form in which it asks for the GroupNorm statistics of its output */
#define LD_FORM_UNET 0  /* split partials, the counters and weight copy of the row-resident kernel; statistics with the chunk geometry (split-K second pass included) */
#define LD_FORM_VAE 1   /* 96 MB of split partials only; statistics from the kernels that sum what they store (the halo tile's epilogue), or none */

const char* ld_version(void);
const char* ld_status_string(int status);

/* ------------------------------------------------------------------ UNet (UNetModel1 ctor arguments, LD.py:5294-5340) */
typedef struct {
    int in_channels, out_channels, model_channels;
    int num_levels;
    int channel_mult[8];
    int num_res_blocks[8];
    int transformer_depth[16];        /* one per input ResBlock */
    int transformer_depth_output[24]; /* one per output ResBlock, in the reference's (popped-from-the-end) list order */
    int transformer_depth_middle;
    int context_dim, num_heads;
} ld_unet_config;

typedef struct ld_unet ld_unet;

int ld_unet_create(const ld_unet_config* cfg, ld_unet** out);
void ld_unet_destroy(ld_unet* u);
/* parameter table: checkpoint key names (minus "model.diffusion_model."), shapes as stored in the checkpoint */
int ld_unet_param_count(const ld_unet* u);
int ld_unet_param_info(const ld_unet* u, int index, const char** name, int* ndim, int64_t shape[4]);
/* copy + repack one checkpoint tensor (device pointer, LD_F16 or LD_F32, checkpoint layout: conv OIHW, linear [out,in]) */
int ld_unet_load_param(ld_unet* u, const char* name, const void* dev_src, int dtype, void* stream);
/* size the activation workspace for up to max_n UNet samples (= 2 x image batch under CFG) of max_h x max_w latents */
int ld_unet_reserve(ld_unet* u, int max_n, int max_h, int max_w, int max_ctx_tokens);
size_t ld_unet_workspace_bytes(const ld_unet* u);
size_t ld_unet_weight_bytes(const ld_unet* u);
/* ctx: [n][tokens][context_dim] (LD_F16 / LD_F32), batch order as the reference builds it: [uncond..., cond...] */
int ld_unet_set_context(ld_unet* u, const void* ctx, int dtype, int n, int tokens, void* stream);
/* ld_control: what a UNet forward adds where upstream calls apply_control — see the ControlNet section below */
typedef struct ld_control ld_control;
#define LD_FWD_EPS_ONLY 1   /* out = the raw UNet output (fp32 of the fp16 eps), not denoised */
#define LD_FWD_PAIR     2   /* CFG pair: x / sigma hold n samples, the batch run and written is 2n: [uncond.. ; cond..] */
/* x, out: [n][in_channels][h][w] fp32 NCHW; sigma: [n] fp32 (sigma, not t).  out = denoised = x - eps * sigma.
 * flags: LD_FWD_* bits.  LD_ERR_ARG, before anything is launched: a bit that is not a flag, LD_FWD_PAIR | LD_FWD_EPS_ONLY.
 * LD_FWD_PAIR is the classifier-free-guidance pair — what the reference's calc_cond_batch feeds the model every step: cat([x, x]) against
 * cat([uncond, cond]) (LD.py:2515-2547).  x: [n][in_channels][h][w], sigma: [n]; the resident context has 2 n rows ([uncond x n ; cond x n]);
 * out: [2 n][..] denoised, same order (n < 1: LD_ERR_SHAPE).  Same result as the plain forward on the duplicated inputs; the layers in front of the
 * first cross-attention (conv_in, the first ResBlock, the first transformer's GroupNorm / proj_in / self-attention) see identical inputs in both
 * halves and are evaluated ONCE, their outputs copied (exact; per sample the bits can differ from the plain forward where a contraction's tile /
 * split choice follows the row count).
 * ctl (may be NULL): the residuals of a control branch, added in ONE launch behind the middle block, when every skip tensor is complete and the
 * encoder reads none of them again.  ctl == NULL: the plain forward, launch for launch; strength == 0 launches nothing more either.
 * LD_ERR_SHAPE, before anything is launched: count is not the number of skip tensors, a shape is not its skip tensor's (the middle block's output),
 * r_n does not divide the batch.  LD_ERR_ARG: a NULL residual. */
int ld_unet_forward(ld_unet* u, const float* x, const float* sigma, float* out, int n, int h, int w, int flags, const ld_control* ctl, void* stream);
/* the same forward with a HIP-event pair around every launch (recorded on `stream`), summed per kernel class:
 * 0 conv3x3 (implicit GEMM)  1 linear / 1x1 GEMM  2 attention  3 GroupNorm  4 LayerNorm  5 misc.  Synchronises the stream.  With ctl the launch
 * table is the plain one with one control_add_kernel entry behind the middle block's last launch (ctl == NULL or strength == 0: the plain table). */
int ld_unet_profile(ld_unet* u, const float* x, const float* sigma, float* out, int n, int h, int w, int flags, const ld_control* ctl, void* stream,
                    double ms[6], double flops[6], int launches[6]);
/* per kernel INSTANTIATION (the names rocprofv3 --kernel-trace lists, abbreviated) of the last ld_unet_profile call:
 * one text line "name<TAB>launches<TAB>total ms<TAB>algorithmic FLOPs" each, NUL-terminated.  LD_ERR_ARG if buf is too small. */
int ld_unet_profile_kernels(const ld_unet* u, char* buf, size_t buf_bytes);
/* per LAUNCH of the last ld_unet_profile call, in launch order: "what<TAB>M<TAB>N<TAB>K<TAB>batch<TAB>algorithmic FLOPs<TAB>
 * microseconds<TAB>kernel" (contractions; GroupNorm rows carry images / pixels / channels / silu, attention rows batch*heads / Lq / Lk / d) */
int ld_unet_profile_launches(const ld_unet* u, char* buf, size_t buf_bytes);
/* LoRA patches of the RESIDENT weights — what ModelPatcher.patch_model / unpatch_model do with calculate_weight and a backup of the
 * original tensors (LD.py:3335-3354, 3407-3437), on the device and in the slots' resident layouts.  One low-rank term of a patch:
 * up [rows][rank], down [rank][cols], row-major device pointers, both LD_F16 or both LD_F32 (`dtype`); 1 <= rank <= 256; scale = strength * alpha / rank.
 * For a conv, cols = Cin*kh*kw in the checkpoint's (i, ky, kx) order (flatten(start_dim=1)). */
typedef struct { const void* up; const void* down; int dtype; int rank; float scale; } ld_lora_term;
/* slot = round_fp16(float(backup) + sum_j scale_j up_j down_j): fp32 products and sum, ONE rounding to nearest for all terms (1 <= n_terms <= 8).
 * The first patch of a slot snapshots its resident bytes into a device backup; every call recomputes from that backup, so re-patching is
 * not cumulative.  LD_ERR_ARG: unknown name, slot not loaded, a vector slot (bias / norm), rank or n_terms out of range.
 * Patch, unpatch and refresh are load-class calls: they may allocate, are ordered on `stream`, and must not be issued during stream capture
 * (LD_ERR_STATE).  Addresses do not move: captured hipGraphs stay valid, but the derived copies must be refreshed (below) and the context set again
 * (the resident cross-attention K / V^T were projected with attn2.to_k / to_v). */
int ld_unet_patch_param(ld_unet* u, const char* name, const ld_lora_term* terms, int n_terms, void* stream);
/* copy the backup back (bit-identical to before the first patch) and free it; name == NULL: every patched slot; never-patched slot: no-op.
 * ld_unet_load_param on a patched slot drops that slot's backup instead (the new load is the new base). */
int ld_unet_unpatch(ld_unet* u, const char* name, void* stream);
/* one parameter back in CHECKPOINT layout (conv OIHW, linear [out,in], GEGLU rows [value | gate]), fp16: dst_f16 holds the slot's element count */
int ld_unet_read_param(const ld_unet* u, const char* name, void* dst_f16, void* stream);
/* re-derive every copy derived from the resident weights (LayerNorm / skip / MLP-out / upsample folds, the row-resident conv layout) if a load,
 * patch or unpatch has happened since — what the next ld_unet_forward would do first; a replayed hipGraph does not, so call this after a batch of patches */
int ld_unet_refresh_derived(ld_unet* u, void* stream);
/* bytes of the patch backups currently held (not part of ld_unet_weight_bytes) */
size_t ld_unet_patch_bytes(const ld_unet* u);
/* number of kernel launches of the last forward, and algorithmic FLOPs of it (2*M*N*K over every contraction) */
int ld_unet_last_launches(const ld_unet* u);
double ld_unet_last_flops(const ld_unet* u);

/* ------------------------------------------------------------------ ControlNet (upstream ComfyUI's cldm.ControlNet; the reference keeps the seams —
 * apply_control1 at LD.py:5290, called at "middle" and "output" in UNetModel1.forward, LD.py:5742, 5747 — and fills none of them)
 * The control branch is an ld_unet in control mode: time_embed, input_blocks and middle_block of the UNet (same names, same routes), no output
 * blocks and no out.*, plus input_hint_block.{0,2,..,14} (the hint encoder: eight 3x3 convolutions hint_channels -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 ->
 * 256 -> model_channels, stride 2 at the third, fifth and seventh, SiLU behind all but the last), zero_convs.{i}.0 (1x1, one per input block) and
 * middle_block_out.0.  Every ld_unet_* call that is not a forward or a profile works on it unchanged: param_count / param_info / load_param /
 * read_param / reserve / set_context / weight_bytes / last_launches / last_flops / destroy.  LD_ERR_ARG: a UNet forward on a control handle, a
 * control call on a UNet handle. */
int ld_controlnet_create(const ld_unet_config* cfg, int hint_channels, ld_unet** out);
/* Encode the control image once per run: image_nchw fp32 [hb][hint_channels][H][W] (device), H = 8 h and W = 8 w of the latents that follow; hb is 1 or
 * divides the batch of the forwards (sample s reads hint s % hb).  The encoded hint [hb][h][w][model_channels] fp16 stays resident in the handle
 * until the next reserve.  Uses the handle's activation workspace: stream-ordered with the forwards.  LD_ERR_SHAPE: hb, H / 8 or W / 8 beyond the
 * reserved plan, H or W not a multiple of 8. */
int ld_controlnet_set_hint(ld_unet* cn, const float* image_nchw, int hb, int H, int W, void* stream);
/* The control branch on x [n][in_channels][h][w] / sigma [n] as ld_unet_forward reads them, against the handle's own resident context (n rows):
 * h = conv_in(x / sqrt(sigma^2 + 1)) + hint, the input blocks, the middle block; residual i = zero_convs.i.0 of input block i's output, the last one
 * middle_block_out.0 of the middle block's — raw fp16 NHWC, in buffers that persist in the handle (allocated by ld_unet_reserve for the reserved
 * maximum), valid until the next forward.  Only enqueues on `stream`; capturable.  LD_ERR_STATE: no hint set; LD_ERR_SHAPE: (h, w) is not the hint's. */
/* flags: LD_FWD_PAIR or 0 (LD_FWD_EPS_ONLY, a branch writes no output: LD_ERR_ARG).  LD_FWD_PAIR: x / sigma hold n samples, the context 2 n rows; the
 * residuals are those of the plain forward on cat([x, x]) (conv_in runs once per latent, everything else on all 2 n samples) */
int ld_controlnet_forward(ld_unet* cn, const float* x, const float* sigma, int n, int h, int w, int flags, void* stream);
/* residuals of the last forward: their number without the middle one (= input blocks), their batch, and residual i (i = count: the middle one) as a
 * device pointer to [batch][H][W][C] fp16 */
int ld_controlnet_residual_count(const ld_unet* cn);
int ld_controlnet_residual_batch(const ld_unet* cn);
int ld_controlnet_residual(const ld_unet* cn, int i, const void** ptr, int* C, int* H, int* W);
/* a copy of residual i into dst_f16 (device), ordered on `stream` */
int ld_controlnet_read_residual(const ld_unet* cn, int i, void* dst_f16, void* stream);
/* the encoded hint of the last ld_controlnet_set_hint: its shape [*hb][*h][*w][*C] (each pointer may be NULL) and, unless dst_f16 is NULL, a copy of
 * it into dst_f16 (device, fp16 NHWC), ordered on `stream`.  LD_ERR_STATE: no hint set since the last reserve. */
int ld_controlnet_read_hint(const ld_unet* cn, void* dst_f16, int* hb, int* h, int* w, int* C, void* stream);
/* ld_controlnet_forward with HIP events around every launch: ld_unet_profile_launches / ld_unet_profile_kernels then describe the control branch's
 * launches.  (ld_controlnet_set_hint counts its eight launches as a forward does: ld_unet_last_launches is 8 behind it.) */
int ld_controlnet_profile(ld_unet* cn, const float* x, const float* sigma, int n, int h, int w, int flags, void* stream);
/* What a UNet forward adds where upstream calls apply_control: residual[i] ([r_n][h[i]][w[i]][c[i]] fp16 NHWC, device) to skip tensor i — the output
 * of input block i; upstream pops control["output"] from the back in step with hs.pop() — and `middle` (shape entry `count`) to the middle block's
 * output, each as t = fp16(float(t) + strength * float(r)); sample s of the forward reads residual sample s % r_n. */
struct ld_control {
    const void* residual[16];
    int count;
    const void* middle;
    int r_n;
    float strength;
    int c[16], h[16], w[16];   /* of residual i; entry `count`: of the middle one */
};
/* the descriptor of a control handle's last forward (r_n <= 0: its batch) */
int ld_controlnet_fill_control(const ld_unet* cn, int r_n, float strength, ld_control* out);

/* ------------------------------------------------------------------ VAE decoder (Decoder ctor arguments, LD.py:6312-6323) */
typedef struct {
    int z_channels, ch, num_levels;
    int ch_mult[8];
    int num_res_blocks, out_ch;
    int with_encoder;   /* != 0: also hold encoder.* and quant_conv.* (VAE.encode path) */
} ld_vae_config;

typedef struct ld_vae ld_vae;

int ld_vae_create(const ld_vae_config* cfg, ld_vae** out);
void ld_vae_destroy(ld_vae* v);
int ld_vae_param_count(const ld_vae* v);
int ld_vae_param_info(const ld_vae* v, int index, const char** name, int* ndim, int64_t shape[4]);
int ld_vae_load_param(ld_vae* v, const char* name, const void* dev_src, int dtype, void* stream);
int ld_vae_reserve(ld_vae* v, int max_b, int max_h, int max_w);   /* latent size */
size_t ld_vae_workspace_bytes(const ld_vae* v);
/* workspace bytes ld_vae_reserve(b, h, w) would allocate (host-only dry run, nothing is allocated; 0 on an invalid shape): lets the host
 * split a batch by free device memory the way VAE.decode does (LD.py:6357-6362) */
size_t ld_vae_plan_bytes(ld_vae* v, int b, int h, int w);
/* z: [b][z_channels][h][w] fp32 (already divided by 0.18215); out: [b][8h][8w][3] fp32 in [0,1] */
int ld_vae_decode(ld_vae* v, const float* z, float* out, int b, int h, int w, void* stream);
/* VAE.encode's device part (LD.py:6383-6410): pixels fp32 NCHW [b][3][8h][8w] in [-1,1] -> moments fp32 NCHW [b][2z][h][w]
 * (mean | logvar, before DiagonalGaussianRegularizer's host-RNG sample, LD.py:3446-3458); (h, w) = latent size */
int ld_vae_encode(ld_vae* v, const float* pixels_nchw, float* moments, int b, int h, int w, void* stream);
/* ld_vae_decode with a HIP-event pair around every launch (recorded on `stream`; synchronises it), and the per-launch table of that
 * run in the format of ld_unet_profile_launches: the per-layer VAE table of profiles/ (TFLOP/s and bytes per stage) is built from it */
int ld_vae_profile(ld_vae* v, const float* z, float* out, int b, int h, int w, void* stream);
/* ld_vae_encode with a HIP-event pair around every launch (synchronises the stream); its table is read by ld_vae_profile_launches too */
int ld_vae_profile_encode(ld_vae* v, const float* pixels_nchw, float* moments, int b, int h, int w, void* stream);
int ld_vae_profile_launches(const ld_vae* v, char* buf, size_t buf_bytes);
int ld_vae_last_launches(const ld_vae* v);
double ld_vae_last_flops(const ld_vae* v);

/* ------------------------------------------------------------------ ESRGAN upscaler (RRDBNet, LD.py:7025-7234) */
typedef struct {
    int in_nc, out_nc;   /* 3, 3 */
    int nf, gc;          /* 64, 32 (the dense-block kernel's channel counts) */
    int nb;              /* RRDB blocks (23 in RealESRGAN_x4plus) */
    int scale;           /* 1, 2, 4 or 8: log2(scale) up-convolutions */
} ld_esrgan_config;

typedef struct ld_esrgan ld_esrgan;

/* LD_ERR_SHAPE for a config the kernels do not run.  Parameter names are the old-arch ones the reference normalises to (LD.py:7044-7055,
 * 7174-7192): model.0, model.1.sub.{b}.RDB{r}.conv{c}.0, model.1.sub.{nb}, model.{3k} (up-convolutions), model.{3n+2} (HR), model.{3n+4}
 * (last), each .weight (OIHW) / .bias */
int ld_esrgan_create(const ld_esrgan_config* cfg, ld_esrgan** out);
void ld_esrgan_destroy(ld_esrgan* e);
int ld_esrgan_param_count(const ld_esrgan* e);
int ld_esrgan_param_info(const ld_esrgan* e, int index, const char** name, int* ndim, int64_t shape[4]);
int ld_esrgan_load_param(ld_esrgan* e, const char* name, const void* dev_src, int dtype, void* stream);
int ld_esrgan_reserve(ld_esrgan* e, int max_b, int max_h, int max_w);   /* input size */
size_t ld_esrgan_workspace_bytes(const ld_esrgan* e);
/* workspace bytes ld_esrgan_reserve(b, h, w) would allocate (host-only dry run; 0 on an invalid shape) */
size_t ld_esrgan_plan_bytes(ld_esrgan* e, int b, int h, int w);
/* x: [b][h][w][3] fp32 NHWC (what ld_vae_decode writes); out: [b][h*scale][w*scale][3] fp32 NHWC, NOT clamped.  Only enqueues on `stream`. */
int ld_esrgan_forward(ld_esrgan* e, const float* x, float* out, int b, int h, int w, void* stream);
/* ld_esrgan_forward with a HIP-event pair around every launch (synchronises the stream), and that run's per-launch table in the format of
 * ld_unet_profile_launches */
int ld_esrgan_profile(ld_esrgan* e, const float* x, float* out, int b, int h, int w, void* stream);
int ld_esrgan_profile_launches(const ld_esrgan* e, char* buf, size_t buf_bytes);
int ld_esrgan_last_launches(const ld_esrgan* e);
/* 2 * pixels * cout * 9 cin over every convolution of the last forward, the two 3-channel ends included */
double ld_esrgan_last_flops(const ld_esrgan* e);

/* ------------------------------------------------------------------ TAESD latent preview (Decoder2 / TAESD.decode, LD.py:688-754) */
typedef struct ld_taesd ld_taesd;

/* The decoder has one shape; parameter names are the keys of taesd_decoder.safetensors (Decoder2's state dict), 67 tensors: 1.weight,
 * 1.bias, {3,4,5,8,9,10,13,14,15,18}.conv.{0,2,4}.{weight,bias}, {7,12,17}.weight, 19.weight, 19.bias (weights OIHW).  vae_shift = 0 and
 * vae_scale = 1 (LD.py:729-730) are not in that file and are those constants here. */
int ld_taesd_create(ld_taesd** out);
void ld_taesd_destroy(ld_taesd* t);
int ld_taesd_param_count(const ld_taesd* t);
int ld_taesd_param_info(const ld_taesd* t, int index, const char** name, int* ndim, int64_t shape[4]);
int ld_taesd_load_param(ld_taesd* t, const char* name, const void* dev_src, int dtype, void* stream);
int ld_taesd_reserve(ld_taesd* t, int max_b, int max_h, int max_w);   /* latent size */
size_t ld_taesd_workspace_bytes(const ld_taesd* t);
/* workspace bytes ld_taesd_reserve(b, h, w) would allocate (host-only dry run; 0 on an invalid shape) */
size_t ld_taesd_plan_bytes(ld_taesd* t, int b, int h, int w);
/* latent: [b][h][w][4] fp32 NHWC, the model-space x of the sampler loop; out_f32: [b][8h][8w][3] fp32 NHWC = (Decoder2(latent) - 0.5) * 2;
 * out_u8 (may be NULL): [b][8h][8w][3] uint8 = uint8(clip(255 ((out_f32 + 1) * 0.5), 0, 255)), fp32 in that order, truncated.  Only
 * enqueues on `stream`; allocates nothing once ld_taesd_reserve covers the shape (LD_ERR_SHAPE when it does not). */
int ld_taesd_decode(ld_taesd* t, const float* latent, float* out_f32, void* out_u8, int b, int h, int w, void* stream);
/* ld_taesd_decode with a HIP-event pair around every launch (synchronises the stream), and that run's per-launch table in the format of
 * ld_unet_profile_launches */
int ld_taesd_profile(ld_taesd* t, const float* latent, float* out_f32, void* out_u8, int b, int h, int w, void* stream);
int ld_taesd_profile_launches(const ld_taesd* t, char* buf, size_t buf_bytes);
int ld_taesd_last_launches(const ld_taesd* t);
/* 2 * pixels * cout * 9 cin over every convolution of the last decode, the two ends included */
double ld_taesd_last_flops(const ld_taesd* t);

/* ------------------------------------------------------------------ single operators (fp16 device tensors unless noted) */
/* y[M][N] = act(alpha * x[M][K] · w[N][K]^T + bias[N]) + residual[M][N];  act: 0 none, 1 SiLU, 3 quick-GELU, 2 GEGLU (w, bias in
 * checkpoint row order [value | gate]; y is [M][N/2]).  ws/ws_bytes: optional split-K scratch. */
int ld_op_linear(const void* x, const void* w, const void* bias, const void* residual, void* y, int M, int N, int K,
                 float alpha, int act, void* ws, size_t ws_bytes, void* stream);
/* y[batch][M][N] = alpha * x[batch][M][K] · w[batch][N][K]^T + bias[N] + bias_m[M], one problem per batch element at the element strides sA, sW, sC
 * (0: shared), row pitches lda, ldw (0 = K) and N.  Rows n_valid .. N-1 of w (n_valid 0 = N) read as zeros: those columns of y are stored as
 * bias + bias_m alone.  The three contractions of the VAE's AttnBlock at a width without a flash kernel.  ws/ws_bytes: split-K scratch (batch 1). */
int ld_op_linear_batched(const void* x, int lda, const void* w, int ldw, const void* bias, const void* bias_m, void* y, int M, int N, int K, int n_valid,
                         float alpha, int batch, long long sA, long long sW, long long sC, void* ws, size_t ws_bytes, void* stream);
/* NHWC conv, ksize 1 or 3, w in [Cout][ky][kx][Cin] order (see ld_op_repack_conv).  Two optional
 * NHWC sources are concatenated along channels; (hv, wv) != (h, w) resizes the input nearest-neighbour first.
 * pad: zeros above / left of the image, -1 = ksize / 2; ho, wo: the output's size, 0 = what pad ksize / 2 gives at this stride — the zeros below /
 * right of the image follow from it (pad 0 with ho = (h - 2) / 2 + 1 at stride 2: the VAE encoder's Downsample, F.pad (0, 1, 0, 1)).
 * n_valid (0 = cout): rows of wt that are read, the others count as zeros; ldc (0 = cout): row pitch of y, a multiple of 8 >= n_valid — the
 * VAE's output convolution on weights padded to 32 rows stores 8 columns.  form: LD_FORM_UNET or LD_FORM_VAE (ws >= 96 MB + 256 there). */
int ld_op_conv(const void* x1, int c1, const void* x2, int c2, int n, int h, int w, int hv, int wv, int stride, int ksize,
               const void* wt, const void* bias, const void* rowvec, const void* residual, void* y, int cout, int pad, int ho, int wo, int n_valid,
               int ldc, int form, void* ws, size_t ws_bytes, void* stream);
/* Host only: does the VAE executor run its output convolution [n][h][w][c] -> out_ch on the halo-tile kernel (ld_op_conv on weights zero-padded
 * to 32 rows with n_valid = 8, ldc = 8 and LD_FORM_VAE, then ld_op_vae_out_finish), 1, or on ld_op_small_conv_out (mode 1), 0? */
int ld_op_vae_conv_out_takes_halo_tile(int c, int n, int h, int w, int out_ch);
/* GroupNorm(32) + SiLU + 3x3 conv (stride 1, pad 1) over the channel concat of two NHWC sources — ResBlock1.in_layers /
 * out_layers (LD.py:5224-5262).  Where the conv runs on the halo-tile kernel the normalisation is fused into its A operand
 * (statistics pass only, no normalised tensor in HBM).  in_part / in_chunks (optional, one source only): the GroupNorm partial statistics
 * of x1 that its producer wrote, [n][in_chunks][32][2] floats — the statistics pass is skipped, as the UNet executor does behind a convolution
 * that emitted them.  part / chunks (both or neither): the partial statistics of y, as ld_op_conv_gn_partials.  form: LD_FORM_UNET, or
 * LD_FORM_VAE for a ResnetBlock half as the VAE executor launches it.  ws >= ld_op_groupnorm_conv_ws_bytes(...). */
size_t ld_op_groupnorm_conv_ws_bytes(int c1, int c2, int n, int h, int w, int cout);
int ld_op_groupnorm_conv(const void* x1, int c1, const void* x2, int c2, int n, int h, int w, const void* gamma, const void* beta, float eps,
                         const void* wt, const void* bias, const void* rowvec, const void* residual, void* y, int cout, float* in_part,
                         int in_chunks, float* part, int* chunks, int form, void* ws, size_t ws_bytes, void* stream);
int ld_op_repack_conv(const void* src_oihw, int dtype, int cout, int cin, void* dst, void* stream);
/* ResBlock1's out_layers convolution and its 1x1 skip_connection as ONE contraction (LD.py:5267, 5273-5287; the UNet executor's "skip
 * fold"):  y = conv3x3(x; wt) + bias + conv1x1(cat(s1, s2); wskip) + bskip (+ rowvec per image), stride 1, pad 1.  x [n][h][w][c];
 * s1 / s2 raw NHWC sources of the same spatial size with sc1 / sc2 channels (s2 may be NULL with sc2 = 0); wt [cout][9c] as ld_op_repack_conv
 * writes it; wskip [cout][sc1 + sc2].  The skip channels are a second segment of the K axis: the weights are concatenated to
 * [cout][9c + sc1 + sc2] in `ws` first (the executor keeps that copy resident).  ws >= ld_op_conv_skip_ws_bytes(...). */
size_t ld_op_conv_skip_ws_bytes(int c, int sc1, int sc2, int cout);
int ld_op_conv_skip(const void* x, int c, int n, int h, int w, const void* wt, const void* bias, const void* s1, int sc1, const void* s2, int sc2,
                    const void* wskip, const void* bskip, const void* rowvec, void* y, int cout, void* ws, size_t ws_bytes, void* stream);
/* The same behind out_layers' GroupNorm(32) + SiLU, as the UNet executor runs a ResBlock's second half:
 *   y = conv3x3(SiLU(GroupNorm(x)); wt) + bias + conv1x1(cat(s1, s2); wskip) + bskip (+ rowvec per image).
 * The skip sources enter RAW.  gamma / beta NULL: no normalisation (ld_op_conv_skip).  part / chunks (both or neither): the GroupNorm partial
 * statistics of y, as ld_op_conv_gn_partials; in_part / in_chunks: those of x from its producer, as ld_op_groupnorm_conv.
 * ws >= ld_op_groupnorm_conv_skip_ws_bytes(...). */
size_t ld_op_groupnorm_conv_skip_ws_bytes(int c, int sc1, int sc2, int cout, int n, int h, int w);
int ld_op_groupnorm_conv_skip(const void* x, int c, int n, int h, int w, const void* gamma, const void* beta, float eps, const void* wt, const void* bias,
                              const void* s1, int sc1, const void* s2, int sc2, const void* wskip, const void* bskip, const void* rowvec, void* y, int cout,
                              float* in_part, int in_chunks, float* part, int* chunks, void* ws, size_t ws_bytes, void* stream);
/* Host only: does the UNet executor run the 3x3 stride-1 convolution [n][h][w][c] -> cout of a ResBlock's out_layers on a kernel that takes the
 * 1x1 skip_connection as a second K segment (ld_op_groupnorm_conv_skip), 1, or does the skip run as a launch of its own in front (0)?  The
 * answer of the route planner under the executors' scratch. */
int ld_op_conv_takes_skip_segment(int c, int n, int h, int w, int cout);
/* Upsample1 (nearest resize to hv x wv, then 3x3 conv, stride 1, pad 1; LD.py:5141-5152) with the resize folded into the weights: for an exact
 * 2x resize the layer is four 2x2 convolutions of the SOURCE image, one per output phase (2y + py, 2x + px), whose weights are sums of the 3x3
 * taps.  ld_op_upconv2x_fold derives them once from wt [cout][9 cin] (ld_op_repack_conv's layout): wfold [py*2+px][cout][a*2+b][cin], 16 cout cin
 * halfs, fp32 sums rounded to fp16 once.  ld_op_upconv2x runs the layer as the UNet executor does: on the folded weights (4/9 of the
 * multiply-adds) when hv = 2h, wv = 2w and n > 2, otherwise exactly as ld_op_conv.  ws/ws_bytes: split-K scratch as ld_op_conv. */
int ld_op_upconv2x_fold(const void* wt, int cout, int cin, void* wfold, void* stream);
int ld_op_upconv2x(const void* x, int c, int n, int h, int w, int hv, int wv, const void* wt, const void* wfold, const void* bias, void* y, int cout,
                   void* ws, size_t ws_bytes, void* stream);
/* Convolution (ksize 1 or 3, any stride, two optional sources, hv = 2h: behind a nearest-2x upsampling; ld_op_conv's arguments) that also returns the GroupNorm(32) partial statistics of its OUTPUT
 * where the kernel that runs the shape writes them (the halo convolution's generic epilogue, the row-resident kernel, the split-K second
 * pass) — what lets the GroupNorm that follows (ResBlock1 out_layers / the next block's in_layers, LD.py:5224-5262; the VAE's ResnetBlock,
 * LD.py:3560-3576) skip its statistics pass.  part: [n][*chunks][32][2] floats (sum, sum of squares per image, pixel chunk, group), sized
 * ld_op_conv_gn_partials_floats(n, hv*wv); *chunks = 0 when this shape's kernel does not write them — under LD_FORM_VAE whenever the halo tile
 * does not take the shape: the caller then runs the two-pass GroupNorm.  pad .. form: as ld_op_conv.  For parity tests. */
size_t ld_op_conv_gn_partials_floats(int n, int hw);
int ld_op_conv_gn_partials(const void* x, int c, const void* x2, int c2, int n, int h, int w, int hv, int wv, int stride, int ksize, const void* wt,
                           const void* bias, const void* residual, void* y, int cout, int pad, int ho, int wo, int n_valid, int ldc, int form, float* part,
                           int* chunks, void* ws, size_t ws_bytes, void* stream);
/* GroupNorm(32) over the channel concat of two NHWC sources (+ optional SiLU); ws >= ld_op_groupnorm_ws_bytes */
size_t ld_op_groupnorm_ws_bytes(int n, int hw);
int ld_op_groupnorm(const void* x1, int c1, const void* x2, int c2, int n, int hw, const void* gamma, const void* beta,
                    float eps, int silu, void* y, void* ws, void* stream);
int ld_op_layernorm(const void* x, const void* gamma, const void* beta, void* y, int rows, int c, float eps, void* stream);
/* q [b][lq][heads*d], k [b][lk][heads*d], vt [b][heads*d][lk_pad] (V transposed, lk_pad = ldvt >= lk, multiple of 8);
 * causal != 0 masks keys after the query position (the CLIP text model's mask, LD.py:4440-4446) */
int ld_op_attention(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo, int b,
                    int heads, int lq, int lk, int d, float scale, int causal, void* stream);
/* the same with V row-major, v [b][lk][ldv] like k — the form the UNet executor runs on the output of its fused q|k|v projection
 * (q, k, v may be column blocks of one [b][l][3*heads*d] tensor: ldq = ldk = ldv = 3*heads*d; requires lq == lk then for the batch strides);
 * the kernel transposes V while it reads it from LDS (ds_read_b64_tr_b16) */
int ld_op_attention_rowv(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int b,
                         int heads, int lq, int lk, int d, float scale, int causal, void* stream);
int ld_op_softmax_rows(void* s, int rows, int cols, void* stream);
int ld_op_timestep_embed(const float* sigma, const float* log_sigmas, int n_sigmas, int n, int dim, void* out_f16, float* t_out,
                         void* stream);
/* guidance / sampler elementwise on fp32 latents: out = u + (c-u)*cfg with den2 = [u ; c];  x = a*x + b*y + c*z */
int ld_op_cfg_combine(const float* den2, float* out, float cfg, size_t n_half, void* stream);
int ld_op_axpby(float* x, float a, const float* y, float b, const float* z, float c, size_t n, void* stream);
/* Device-side guards of the model_function_wrapper hook (LD.py:2558-2567; the object on that seam replays a captured hipGraph the way the
 * reference's stable-fast patch does with enable_cuda_graph, LD.py:9896-9933): flags[0] = epoch when the 32-bit words of a and b differ
 * (the step's c_crossattn against the conditioning the resident cross-attention K / V^T were projected from), flags[1] = epoch when the two
 * halves of x (2 * half_words_x words) or of sigma (2 * half_sigma floats, half_sigma <= 256) differ (calc_cond_batch's cat([x_in, x_in]),
 * LD.py:2515-2547).  flags: two ints the device can write (device or pinned host memory); never reset — the host compares with its epoch. */
int ld_op_hook_check(const void* a, const void* b, size_t words_ab, const void* x, size_t half_words_x, const void* sigma, int half_sigma,
                     int* flags, int epoch, void* stream);

/* ---- The norm, boundary-convolution and fold kernels on their own, for element-wise parity tests (tests/errbound.py): each is the
 * kernel's launcher behind an argument check, no device code of its own. */
/* softmax_rows with a row pitch ld >= cols (elements, a multiple of 8) and `valid` <= cols real columns (0 = cols): columns >= valid are
 * written as zeros, elements cols .. ld-1 of a row are not touched */
int ld_op_softmax_rows_ld(void* s, int rows, int cols, long long ld, int valid, void* stream);
/* GroupNorm(32) in its consumer-facing forms.  ld_op_groupnorm_chunks: pixel chunks per image of the statistics pass.
 * ld_op_groupnorm_stats: part [n][chunks][32][2] floats (sum, sum of squares).  ld_op_groupnorm_from_partials: the apply pass alone over
 * part [n][pstat][32][2] a producer wrote (pstat >= 1, any chunking of the image's pixels).  ld_op_groupnorm_scale_shift: scale / shift
 * [n][c1 + c2] fp32 with  y = x * scale + shift  — the values the apply pass multiplies by, bit for bit; stats_ready = 0 runs the statistics
 * pass into ws (>= ld_op_groupnorm_ws_bytes), > 0 reads ws as [n][stats_ready][32][2]. */
int ld_op_groupnorm_chunks(int n, int hw);
int ld_op_groupnorm_stats(const void* x1, int c1, const void* x2, int c2, int n, int hw, float* part, void* stream);
int ld_op_groupnorm_from_partials(const void* x1, int c1, const void* x2, int c2, int n, int hw, const void* gamma, const void* beta, float eps,
                                  int silu, void* y, float* part, int pstat, void* stream);
int ld_op_groupnorm_scale_shift(const void* x1, int c1, const void* x2, int c2, int n, int hw, const void* gamma, const void* beta, float eps,
                                float* ws, int stats_ready, float* scale, float* shift, void* stream);
/* 3x3 pad-1 convolution from cin <= 4 channels: x fp32 NCHW [n][cin][h][w] -> y fp16 NHWC [n][h][w][cout], cout a multiple of 8, wt [cout][9 cin]
 * (tap-major).  scale_sigma [n] (optional): x is scaled by 1 / sqrt(sigma^2 + 1) and rounded to fp16 first; pre_w [cin][cin], pre_b (optional):
 * a 1x1 convolution in front, rounded to fp16; dup_off != 0: every output is stored a second time at y + dup_off (elements). */
int ld_op_small_conv_in(const float* x, const float* scale_sigma, const void* pre_w, const void* pre_b, const void* wt, const void* bias, void* y,
                        int n, int cin, int h, int w, int cout, long long dup_off, void* stream);
/* 3x3 pad-1 convolution to cout <= 4 channels from x fp16 NHWC [n][h][w][cin], cin a multiple of 8 up to 512, wt [cout][9 cin], out fp32.
 * mode 0: out NCHW = x_in - fp16(v) * sigma (x_in [n][cout][h][w], sigma [n]; in_mod > 0: both hold in_mod samples, sample i reads i % in_mod);
 * mode 1: out NHWC = clamp((v + 1) / 2, 0, 1);  mode 2: out NCHW = v. */
int ld_op_small_conv_out(const void* x, const void* wt, const void* bias, int n, int h, int w, int cin, int cout, int mode, const float* x_in,
                         const float* sigma, int in_mod, float* out, void* stream);
/* out fp32 NCHW [n][c][hw] = fp16(bias + w x) of x fp16 [n][hw][8], w [c][c]; c == 8 */
int ld_op_small_pointwise(const void* x, const void* wt, const void* bias, float* out, int n, int hw, int c, void* stream);
/* out fp32 [npix][cout] = clamp((t8 + 1) / 2, 0, 1) of the first cout <= 8 columns of t8 fp16 [npix][8] */
int ld_op_vae_out_finish(const void* t8, float* out, long long npix, int cout, void* stream);
/* ld_op_timestep_embed with sigma_mod > 0: sigma holds sigma_mod samples and sample i reads sigma[i % sigma_mod] */
int ld_op_timestep_embed_mod(const float* sigma, const float* log_sigmas, int n_sigmas, int n, int dim, void* out_f16, float* t_out, int sigma_mod,
                             void* stream);
/* count <= 3 ranges: bytes [base_i, base_i + bytes_i) are copied to [base_i + bytes_i, base_i + 2 bytes_i); bases and lengths multiples of 16 */
int ld_op_dup_halves(void* base0, size_t bytes0, void* base1, size_t bytes1, void* base2, size_t bytes2, int count, void* stream);
/* src [n][t][d] (dtype LD_F16 / LD_F32) -> dst fp16 [n][tp][d], rows t .. tp-1 zero */
int ld_op_ctx_pad(const void* src, int dtype, int n, int t, int tp, int d, void* dst, void* stream);
/* the cross-attention operands ld_unet_set_context projects once per context, per transformer: k_out [n][tp][c] = ctx16 wk^T and
 * vt_out [n][c][tp] = wv ctx16_b^T from the padded context ctx16 [n][tp][d] (ld_op_ctx_pad), wk / wv [c][d] */
int ld_op_ctx_kv(const void* ctx16, const void* wk, const void* wv, int n, int tp, int d, int c, void* k_out, void* vt_out, void* stream);
/* w_out [c][5c] = [wpo w2 | wpo], b_out = wpo b2 + bpo  (wpo [c][c], w2 [c][4c]): fp32 sums, one rounding to fp16 */
int ld_op_mlp_out_fold(const void* wpo, const void* w2, const void* b2, const void* bpo, int c, void* w_out, void* b_out, void* stream);
/* w_out [n][k] = fp16(w * gamma), b_out [n] = fp16(bias + w beta) (bias optional), wsum [n] = fp32 row sums of the ROUNDED w_out */
int ld_op_ln_fold(const void* w, int n, int k, const void* gamma, const void* beta, const void* bias, void* w_out, void* b_out, float* wsum,
                  void* stream);

/* The LayerNorm fold of the UNet's transformer blocks (BasicTransformerBlock, LD.py:4117-4162: every attention / GEGLU
 * projection reads LayerNorm(x)) as an operator pair, for parity tests: t[M][C] = x · w_prod^T + b_prod (the GEMM that writes the
 * residual stream, emitting per-row statistics) and y[M][N] = LayerNorm(t; gamma, beta, eps) · w^T + bias, finished on the fp32
 * accumulators of t · (w diag(gamma))^T.  residual [M][C] (optional) is added to t: the residual stream's own update, t += x · w_prod^T + b_prod.
 * ws: >= 2*N*C + 8*N + 8*((C+63)/64)*M + 1024 bytes. */
int ld_op_linear_ln(const void* x, const void* w_prod, const void* b_prod, const void* residual, const void* gamma, const void* beta, const void* w,
                    const void* bias, void* t_out, void* y, int M, int C, int N, float eps, void* ws, size_t ws_bytes, void* stream);
/* The same pair with the GEGLU of FeedForward.net[0] as the consumer (LD.py:4513-4515, 4524-4540): y[M][N/2] = a * gelu(g) with
 * [a | g] = LayerNorm(t) · w^T + bias — the transformer block's MLP input exactly as the executor runs it (row-panel kernel at C = 320).
 * ws: >= 4*N*C + 12*N + 8*((C+63)/64)*M + 2048 bytes. */
int ld_op_linear_ln_geglu(const void* x, const void* w_prod, const void* b_prod, const void* residual, const void* gamma, const void* beta, const void* w,
                          const void* bias, void* t_out, void* y, int M, int C, int N, float eps, void* ws, size_t ws_bytes, void* stream);
/* bislerp (LD.py:429-518, LatentUpscale.upscale 6639-6654): fp32 NCHW latents [n][c][h][w] -> [n][c][h_new][w_new];
 * tmp: n*c*h*w_new floats of scratch (the width pass runs first, as in the reference) */
int ld_op_bislerp(const float* x, float* tmp, float* y, int n, int c, int h, int w, int h_new, int w_new, void* stream);
/* The dense-block 3x3 convolution of RRDBNet (stride 1, pad 1) on its own kernel (ResidualDenseBlock_5C, LD.py:6905-6992):
 *   y[n][h][w][c_off .. c_off + cout) = epilogue(conv3x3(x[..][0 .. cin); wt) + bias),
 *   epilogue (fp32, one rounding): slope != 0: v = v > 0 ? v : slope v;  r1 != NULL: v = s1 v + r1;  r2 != NULL: v = s2 v + r2.
 * x: NHWC with pixel pitch ldx >= cin, cin a multiple of 32 in [64, 192]; cout 32 or 64; wt [cout][9 cin] as ld_op_repack_conv writes it;
 * r1 / r2: NHWC with pitches ldr1 / ldr2, cout channels read.  y may be x (same pointer and pitch) when c_off >= cin — the dense
 * concatenation in place; any other overlap of y with x is LD_ERR_ARG.  (h, w) is the output size; up != 0: x is [n][h/2][w/2] and is read
 * through a nearest-2x upsampling (upconv_block, LD.py:6995-7022).  Pitches and c_off are multiples of 8.  LD_ERR_SHAPE otherwise.
 * ld_op_esrgan_conv_y2 is the same call with a second store (ld_op_esrgan_conv passes y2 = NULL): y2 != NULL: the same cout values are also stored at y2[n][h][w][0 .. cout) (pitch ldy2 >= cout, a multiple of 8) — the RRDB's third block
 * writes the next RRDB's outer residual there, and y2 may be r2 itself (each element is read before it is overwritten, by the same lane);
 * y2 overlapping x: LD_ERR_ARG. */
int ld_op_esrgan_conv(const void* x, int ldx, int cin, int n, int h, int w, int up, const void* wt, const void* bias, void* y, int ldy, int c_off, int cout,
                      float slope, const void* r1, int ldr1, float s1, const void* r2, int ldr2, float s2, void* stream);
int ld_op_esrgan_conv_y2(const void* x, int ldx, int cin, int n, int h, int w, int up, const void* wt, const void* bias, void* y, int ldy, int c_off,
                         int cout, float slope, const void* r1, int ldr1, float s1, const void* r2, int ldr2, float s2, void* y2, int ldy2, void* stream);
/* TAESD's 64 -> 64 convolution (stride 1, pad 1) on the same halo-tile main loop under its own epilogue (Block, LD.py:695-702):
 *   y[n][h][w][64] = relu?(conv3x3(x; wt) + bias? + residual?)     (fp32, one rounding at the store)
 * x, residual, y: fp16 NHWC of pitch 64; wt [64][9 * 64] as ld_op_repack_conv writes it; bias, residual may be NULL.  (h, w) is the output
 * size; up != 0: x is [n][h/2][w/2][64] and is read through a nearest-2x upsampling (h, w even).  y overlapping x or residual: LD_ERR_ARG. */
int ld_op_taesd_conv(const void* x, int n, int h, int w, int up, const void* wt, const void* bias, const void* residual, int relu, void* y, void* stream);
/* The end convolutions of the upscaler and of the preview decoder alone (3x3, stride 1, pad 1; the launchers ld_esrgan_forward and
 * ld_taesd_decode call) — for parity tests.  Weights as ld_op_repack_conv writes them ([cout][ky][kx][cin]); pitches are multiples of 8 and
 * at least 64; a NULL x, wt, bias or output: LD_ERR_ARG; n, h, w < 1, a bad pitch or more pixels than a grid holds: LD_ERR_SHAPE — both
 * before any launch, and such a call leaves ld_op_last_kernel() as it was; a call that ran names its kernel there ("taesd_first_kernel").
 *   esrgan_first: x fp32 NHWC [n][h][w][3], rounded to fp16 once -> y fp16 [n][h][w][0 .. 64) at pixel pitch ldy, and the same 64 values at
 *                 y2 (pitch ldy2) when y2 != NULL.  No activation (conv_first, LD.py:7092-7099).
 *   esrgan_last:  the first 64 channels of x fp16 NHWC (pitch ldx) -> out fp32 NHWC [n][h][w][3], unclamped (conv_last, LD.py:7141-7149).
 *   taesd_first:  latent fp32 NHWC [n][h][w][4] -> relu(conv(round_fp16(3 tanh(x / 3))) + bias) fp16 [n][h][w][64] (LD.py:691-693, 716).
 *   taesd_last:   x fp16 [n][h][w][64] -> out_f32 [n][h][w][3] = (conv + bias - 0.5) * 2 and, when out_u8 != NULL, the preview image
 *                 uint8(clip(255 ((out_f32 + 1) * 0.5), 0, 255)) [n][h][w][3], truncated (LD.py:720, 753). */
int ld_op_esrgan_first(const float* x, const void* wt, const void* bias, void* y, int ldy, void* y2, int ldy2, int n, int h, int w, void* stream);
int ld_op_esrgan_last(const void* x, int ldx, const void* wt, const void* bias, float* out, int n, int h, int w, void* stream);
int ld_op_taesd_first(const float* x, const void* wt, const void* bias, void* y, int n, int h, int w, void* stream);
int ld_op_taesd_last(const void* x, const void* wt, const void* bias, float* out_f32, void* out_u8, int n, int h, int w, void* stream);
/* tiled_scale's accumulation (LD.py:7326-7352), fp32 NHWC: out[oh][ow][c] += ps[th][tw][c] * my[y] * mx[x] at offset (y0, x0) and
 * div[oh][ow] += my[y] * mx[x] (my, mx: the tile's two 1-D feather ramps); ps == NULL: the final out /= div. */
int ld_op_tile_blend(const float* ps, const float* my, const float* mx, int th, int tw, float* out, float* div, int oh, int ow, int y0, int x0, int c,
                     void* stream);
/* The contraction kernel instantiations (GEMM / convolution / attention, the names the profile tables use) that the calling thread's
 * last ld_op_* call dispatched, in launch order, joined with ';' (e.g. "gemm3_kernel<64,160,conv>+splitk_reduce_kernel").  Reset at
 * the start of every ld_op_* call; "" when that call dispatched no contraction.  Valid until the thread's next ld_op_* call.
 * (ld_op_esrgan_first / _last and ld_op_taesd_first / _last name their kernel too, and leave the string alone when they refuse a call.)
 * The two small convolutions name their instantiation too ("small_conv_in_kernel<3>", "small_conv_out_kernel<9,1>"). */
const char* ld_op_last_kernel(void);
/* EVERY launch of the calling thread's last ld_op_* call, in launch order and joined with ';', under the names the executors' launch tables
 * (ld_unet_profile_launches) print: the contractions as above, and the norm and boundary launches ("gn_stats_kernel+gn_finalize_kernel",
 * "gn_apply_kernel", "timestep_embed_kernel", "small_conv_in_kernel", "dup_halves_kernel", ...); ld_op_esrgan_conv / _first / _last and
 * ld_op_taesd_conv / _first / _last the names of ld_esrgan_profile_launches / ld_taesd_profile_launches ("esrgan_conv_kernel<64,up>",
 * "taesd_first_kernel").  Operators outside the four executors' forwards leave it "". */
const char* ld_op_last_launches(void);
/* The merge kernel of ld_unet_patch_param on a plain row-major matrix: dst[rows][cols] = round_fp16(float(base) + sum_j scale_j up_j down_j);
 * dst may alias base.  Also what the host's text model patches its weights with. */
int ld_op_lora_merge(const void* base_f16, void* dst_f16, int rows, int cols, const ld_lora_term* terms, int n_terms, void* stream);

/* ---- 8-bit image operators (UltimateSDUpscale's tile plumbing, LD.py:7629-7739, kept on the device).  Images are uint8, HWC (a mask: HW),
 * addressed by a pointer and a row pitch in BYTES, so a crop of a larger image costs nothing.  All arithmetic is integer and bit-identical
 * to Pillow's.  Channels: 1 to 4.
 *
 * Separable resize (Image.resize with LANCZOS or BICUBIC) of the in_w x in_h window at src to out_w x out_h: the horizontal pass first, then
 * the vertical, with a uint8 intermediate; each output byte is clip8((2^21 + sum pixel * tap) >> 22).  A pass runs exactly when its size
 * changes and must then be given its taps, otherwise NULL (both NULL: a copy).  hcoef / vcoef: DEVICE int arrays [out][2 + k] = first input
 * sample, tap count (<= k), taps in fixed point with 22 fractional bits; the caller builds them (Pillow's precompute_coeffs in double) and
 * guarantees first + count <= input size and 255 * sum |tap| + 2^21 < 2^31.  tmp: ld_op_u8_resample_tmp_bytes(in_h, out_w, channels) bytes,
 * read only when both passes run. */
int ld_op_u8_resample(const void* src, int src_pitch, int in_w, int in_h, int channels, void* dst, int dst_pitch, int out_w, int out_h, const int* hcoef,
                      int hk, const int* vcoef, int vk, void* tmp, void* stream);
size_t ld_op_u8_resample_tmp_bytes(int in_h, int out_w, int channels);
/* ImageFilter.GaussianBlur(radius) of the one-channel w x h image at src: three box passes along x, then three along y, uint8 after each;
 * edges replicate at the border of THIS image, so a caller that blurs a window of a larger image grows the window by the blur's reach,
 * 3 * (box_radius + 1) per side, or to the image's edge.  ld_op_u8_box_weights (host only) gives one pass's integer radius and weights,
 * computed in float32 in Pillow's order.  tmp: ld_op_u8_blur_tmp_bytes(w, h) bytes.  dst may be src. */
int ld_op_u8_box_weights(float radius, int* box_radius, unsigned* ww, unsigned* fw);
size_t ld_op_u8_blur_tmp_bytes(int w, int h);
int ld_op_u8_gaussian_blur(const void* src, int src_pitch, void* dst, int dst_pitch, int w, int h, float radius, void* tmp, void* stream);
/* One job's mask inside a w x h window: 0 everywhere except the pw x ph rectangle at (px, py), window coordinates, which may hang over any
 * edge: 255 (ImageDraw.rectangle) or pattern[ph][pw] (the pasted seam-fix gradient). */
int ld_op_u8_mask(void* dst, int dst_pitch, int w, int h, int px, int py, int pw, int ph, const void* pattern, int pattern_pitch, void* stream);
/* canvas[y0 .. y0 + h)[x0 .. x0 + w) = div255(tile * a + canvas * (255 - a)) per channel, div255(v) = ((v + 128) + ((v + 128) >> 8)) >> 8:
 * process_images' paste, putalpha, masked paste, alpha_composite and convert("RGB") over an opaque image.  The region must lie inside the
 * cw x ch canvas (LD_ERR_ARG otherwise); bytes outside it are not touched. */
int ld_op_u8_composite(void* canvas, int canvas_pitch, int cw, int ch, const void* tile, int tile_pitch, const void* alpha, int alpha_pitch, int x0, int y0,
                       int w, int h, int channels, void* stream);
/* tensor_to_pil (LD.py:7445-7449): y = uint8(clip(255 * x, 0, 255)), a truncation in fp32;  pil_to_tensor (LD.py:7452-7456): y = x / 255 as a
 * correctly rounded fp32 division.  n elements, contiguous. */
int ld_op_u8_from_f32(const float* x, void* y, size_t n, void* stream);
int ld_op_f32_from_u8(const void* x, float* y, size_t n, void* stream);

/* ---- fp32 image operators (the Detailer's per-segment plumbing, DetailerForEach.do_detail, LD.py:9402-9590, kept on the device).  The canvas is
 * fp32 HWC and a mask fp32 HW, addressed by a pointer and a row pitch in FLOATS; uint8 images as above, pitch in bytes.  Sides up to 16384,
 * channels 1 to 4.  Every argument is checked before anything is launched (LD_ERR_ARG: a NULL pointer, a size < 1, a window or origin outside
 * the canvas; LD_ERR_SHAPE: a pitch below its row, a side or a feather beyond the limits), and no kernel touches memory outside the windows
 * these arguments describe.
 *
 * tensor2pil of the window [y1, y2) x [x1, x2) of the cw x ch canvas: dst[y][x][c] = uint8(clip(255 * v, 0, 255)), one fp32 product, the clip,
 * a truncation (the arithmetic of ld_op_u8_from_f32).  The window must lie inside the canvas; the canvas is not written. */
int ld_op_f32_crop_u8(const float* canvas, int canvas_pitch, int cw, int ch, int channels, int x1, int y1, int x2, int y2, void* dst, int dst_pitch,
                      void* stream);
/* torchvision's GaussianBlur(kernel_size = 2 * feather + 1) of the w x h mask at src with reflect padding (-k -> k, n - 1 + k -> n - 1 - k): a
 * pass along x into tmp, then a pass along y into dst, out = sum_j taps[j] * in[reflect(i + j - feather)] with every product and every sum
 * rounded to fp32 on its own, j ascending from 0 — a result is the same bits run to run.  taps: DEVICE floats [2 * feather + 1], built by the caller
 * as torchvision builds them (linspace(-feather, feather), exp(-0.5 (x / sigma)^2), divided by their sum, in fp32).  feather 0 is a copy
 * (hipMemcpy2DAsync, no launch; taps and tmp may be NULL).  LD_ERR_SHAPE: feather >= min(w, h), which reflection cannot serve, or feather >
 * ld_op_f32_blur_max_feather() = 127, the tap buffer in LDS.  tmp: ld_op_f32_blur_tmp_bytes(w, h) bytes.  dst may be src. */
int ld_op_f32_blur_max_feather(void);
size_t ld_op_f32_blur_tmp_bytes(int w, int h);
int ld_op_f32_gaussian_blur(const float* src, int src_pitch, float* dst, int dst_pitch, int w, int h, int feather, const float* taps, float* tmp,
                            void* stream);
/* pil2tensor + tensor_paste in place: canvas[y0 + y][x0 + x][c] = (1 - a) * canvas + a * (tile / 255) with a = alpha[y][x], on the tw x th tile's
 * window clipped to the cw x ch canvas; the subtraction, the division, the two products and the sum are each rounded to fp32 (no FMA, no
 * reciprocal).  (x0, y0) must lie inside the canvas; floats outside the clipped window are not touched. */
int ld_op_f32_paste_u8(float* canvas, int canvas_pitch, int cw, int ch, int channels, const void* tile, int tile_pitch, const float* alpha, int alpha_pitch,
                       int tw, int th, int x0, int y0, void* stream);

/* ---- the masked sampler step (inpainting): the two blends upstream's KSamplerX0Inpaint makes around the model call, on fp32 NCHW latents
 * [B][C][HW] (HW = h * w, any positive value), contiguous.  The mask is fp32 [Bm][Cm][HW] with Bm in {1, B} and Cm in {1, C}, broadcast in the
 * kernel.  Every fp32 operation is rounded on its own, in the order written (no FMA), so a result is the bits of the expression evaluated
 * operation by operation.  Stream-ordered, no allocation, no host read: capturable.  LD_ERR_ARG: a NULL pointer; LD_ERR_SHAPE: B, C or HW < 1,
 * Bm not in {1, B}, Cm not in {1, C}, B * C * HW >= 2^31 (the kernels index in 32 bits).  Nothing is launched then.
 *
 * out = x * m + (noise * sigma[b] + latent) * (1 - m): x * m, noise * sigma, + latent, 1 - m, the product, the sum.  sigma: DEVICE floats [B], one per
 * sample.  out may be x; it may be neither the mask, the latent nor the noise. */
int ld_op_inpaint_in(const float* x, const float* mask, const float* latent, const float* noise, const float* sigma, float* out, int B, int C, int HW, int Bm,
                     int Cm, void* stream);
/* den = den * m + latent * (1 - m) in place: den * m, 1 - m, latent * that, the sum. */
int ld_op_inpaint_out(float* den, const float* mask, const float* latent, int B, int C, int HW, int Bm, int Cm, void* stream);

/* ---- regional conditioning: conditioning entries that carry an area, a mask or a strength (upstream's get_area_and_mult and the accumulate / divide
 * loops of calc_cond_batch; the reference keeps their skeleton with area = the whole latent and strength = 1, LD.py:2435-2458, 2492-2591), on fp32
 * NCHW latents [B][C][H][W], contiguous.  Both calls copy their descriptor array (HOST memory, read before the call returns) into the kernel
 * arguments; they are stream-ordered, allocate nothing and read nothing on the host afterwards: capturable.  Every fp32 operation is rounded on
 * its own, in the order written (no FMA).  LD_ERR_ARG: a NULL pointer (an entry's `out` included; `mask` may be NULL).  LD_ERR_SHAPE: a size < 1,
 * more than LD_REGIONAL_MAX_ENTRIES descriptors or none, a window or area that leaves the latent, list not in {0, 1}, mask_batch not in {1, B}
 * where there is a mask, a tensor of 2^31 floats or more (the kernels index in 32 bits).  Nothing is launched then. */
#define LD_REGIONAL_MAX_ENTRIES 16
typedef struct { int y0, x0; } ld_regional_window;
typedef struct {
    const float* out;   /* DEVICE: this entry's model output [B][C][h][w] (its rows of the group's batch) */
    const float* mask;  /* DEVICE: [mask_batch][H][W] on the latent's grid, or NULL */
    int list;           /* 0: positive (cond), 1: negative (uncond) */
    int mask_batch;     /* 1 or B; sample b reads plane b % mask_batch */
    int y0, x0, h, w;   /* the entry's area on the latent */
    float strength, mask_strength;
} ld_regional_entry;
/* out[(j * B + b)][c][y][x] = x[b][c][y0_j + y][x0_j + x] for the k windows, all h x w: the model input of one group of entries in one launch
 * (k windows that are the whole latent: the latent k times).  out: [k * B][C][h][w]; it may not overlap x. */
int ld_op_regional_gather(const float* x, float* out, int B, int C, int H, int W, int h, int w, const ld_regional_window* windows, int k, void* stream);
/* result[b][c][Y][X] = u + (c - u) * cond_scale, where for each list pred = num / den (IEEE division) with num = 0, den = 1e-37f and, for the
 * entries of the list that cover (Y, X), in array order: mult = (mask ? mask[b % mask_batch][Y][X] * mask_strength : 1) * strength; without a
 * mask, for the area's edges top, bottom, left, right that are not edges of the latent and a pixel t < 8 rows / columns from that edge,
 * mult = mult * (0.125f * (t + 1)); num += out * mult; den += mult.  A pixel no entry of a list covers gives 0 for that list.  result may not
 * overlap an input. */
int ld_op_regional_combine(const ld_regional_entry* entries, int n, float cond_scale, float* result, int B, int C, int H, int W, void* stream);

/* ---- ControlNet's two kernels (csrc/control/control.hip), for parity tests.
 * control add: for each of `count` (1 .. 16) segments, t[i] [n][per[i]] fp16 in place: t = fp16(float(t) + strength * float(r)), r[i] [r_n][per[i]] fp16,
 * sample s reads residual sample s % r_n (r_n divides n).  One fp32 product, one fp32 sum, each rounded on its own (no FMA), one rounding to fp16:
 * the bits of (t.float() + strength * r.float()).half().  t, r, per: HOST arrays of device pointers / halves per sample, read before the call
 * returns.  16-byte accesses where every per[i] is a multiple of 8 and every pointer 16-byte aligned, single halves otherwise: the same bits.
 * LD_ERR_SHAPE: count, n, r_n out of range, n * per[i] >= 2^31.  LD_ERR_ARG: a NULL pointer. */
int ld_op_control_add(void* const* t, const void* const* r, const long long* per, int count, int n, int r_n, float strength, void* stream);
/* one layer of the hint encoder: y [n][ho][wo][cout] fp16 = silu?(conv3x3, pad 1, stride 1 | 2, + bias), ho = (h - 1) / stride + 1; the input is
 * x_f16_nhwc [n][h][w][cin] (cin a multiple of 8) or x_f32_nchw [n][cin][h][w] (cin <= 4; every sample rounded to fp16 once) — exactly one of them;
 * wt [cout][ky][kx][cin] fp16 (what ld_op_repack_conv writes), cout a multiple of 8.  fp32 accumulation in the order (ky, kx, ci), + bias, SiLU in
 * fp32, one rounding at the store. */
int ld_op_hint_conv(const void* x_f16_nhwc, const float* x_f32_nchw, int n, int h, int w, int cin, const void* wt, const void* bias, int cout, int stride,
                    int silu, void* y, void* stream);

/* ---- CLIP text model input stage with textual-inversion vectors (CLIPEmbeddings + SDClipModel.set_up_textual_embeddings, LD.py:4394-4410, 4642-4690).
 * out[b][l] = round_fp16(float(row(ids[b*L + l])) + float(pos[l])), fp16 [B, L, h].  `table` is the resident fp16 token table [V, h] (EOS = row V-1),
 * `extra` the prompt's E custom vectors, fp32 [E, h] (may be NULL when E == 0), `pos` the fp16 position table (at least L rows of h).
 *   id <  V-1          : table[id]
 *   V-1 <= id < V-1+E  : extra[id - (V-1)]
 *   id == V-1+E        : table[V-1]   (the remapped EOS: again the largest id)
 * The table is read in place: nothing of V rows is built per prompt.  An id outside [0, V+E) reads no table memory and gives a row of zeros
 * (callers range-check ids on the host; the guard only keeps a bad id from reading out of bounds).
 * LD_ERR_SHAPE: h not a multiple of 8, a pointer not 16-byte aligned;  LD_ERR_ARG: a NULL pointer, a count < 1.  Nothing is launched then. */
int ld_op_clip_embed(const int* ids, const void* table, const float* extra, const void* pos, void* out, int B, int L, int V, int E, int h, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LD_MI355X_H */
