// Launcher declarations for the gfx950 kernels (internal to the shared library; the public C ABI is
// include/ld_mi355x.h).  Every launcher validates shapes on the host and returns an LD_* status.
#pragma once
#include <cstdint>
#include <cstdlib>
#include "common.h"
#include "gemm.h"

// ---- norm.hip
// pixel chunks per image: aim at ~2048 blocks (x 4 channel slabs x n images), at least 8 pixels per chunk, at most 256 chunks
static inline int gn_num_chunks(int n_img, int HW) {
    // workgroups per launch, measured (profiles/README.md): 512 is best at UNet batch 2 (GroupNorm 0.92 -> 0.74 ms per forward),
    // 1024 at UNet batch 16 (1.51 -> 1.40 ms), 2048 for the 512x512 VAE tensors
    const long long px = (long long)(n_img < 1 ? 1 : n_img) * HW;   // (sized by pixels: a batch-1 VAE image is one huge tensor)
    const int target = px <= 8192 ? 512 : (px <= 131072 ? 1024 : 2048);
    int p = target / (4 * (n_img < 1 ? 1 : n_img));
    if (p > HW / 8) p = HW / 8;
    if (p > 256) p = 256;
    return p < 1 ? 1 : p;
}
size_t groupnorm_workspace_bytes(int n_img, int HW);
// stats_ready: 0 = run the statistics pass; > 0 = `partial` already holds a producer's partial statistics with that many pixel chunks per
// image ([n_img][stats_ready][32][2]: gemm.h gn_part / conv8) and only the apply pass runs
int groupnorm_launch(const half_t* x1, int C1, const half_t* x2, int C2, int n_img, int HW, const half_t* gamma,
                     const half_t* beta, float eps, int silu, half_t* y, float* partial, hipStream_t stream, int stats_ready = 0);
// the statistics pass alone: partial [n_img][gn_num_chunks(n_img, HW)][32][2] (for a consumer that finishes the normalisation itself: conv8)
int groupnorm_stats_launch(const half_t* x1, int C1, const half_t* x2, int C2, int n_img, int HW, float* partial, hipStream_t stream);
// statistics pass + finalize only: scale / shift [n_img][C1 + C2] fp32 for a consumer that normalises on the fly (gemm.h gn_scale)
int groupnorm_scale_shift_launch(const half_t* x1, int C1, const half_t* x2, int C2, int n_img, int HW, const half_t* gamma, const half_t* beta,
                                 float eps, float* partial, float* scale, float* shift, hipStream_t stream, int stats_ready = 0);
int layernorm_launch(const half_t* x, const half_t* gamma, const half_t* beta, half_t* y, int rows, int C, float eps,
                     hipStream_t stream);
// in-place row softmax over fp16 scores; cols and ld multiples of 8; valid (0 = cols): columns >= valid are padding (written as 0)
int softmax_rows_launch(half_t* s, int rows, int cols, long long ld, hipStream_t stream, int valid = 0);

// ---- attention.hip
struct AttnParams {
    const half_t* Q = nullptr;   // element (b, l, h, dd) at Q + b*sQ + l*ldq + h*d + dd
    const half_t* K = nullptr;   // element (b, key, h, dd) at K + b*sK + key*ldk + h*d + dd
    const half_t* Vt = nullptr;  // element (b, h, dd, key) at Vt + b*sV + (h*d + dd)*ldvt + key   (V transposed)
    const half_t* V = nullptr;   // ... or row-major: element (b, key, h, dd) at V + b*sV + key*ldv + h*d + dd  (exactly one of Vt / V)
    int ldv = 0;
    half_t* O = nullptr;         // element (b, l, h, dd) at O + b*sO + l*ldo + h*d + dd
    int ldq = 0, ldk = 0, ldvt = 0, ldo = 0;
    long long sQ = 0, sK = 0, sV = 0, sO = 0;
    int B = 0, H = 0, Lq = 0, Lk = 0, d = 0;
    float scale = 1.0f;
    int causal = 0;              // key index <= query index only (CLIP text model, LD.py:4440-4446)
};
int attention_launch(const AttnParams& p, hipStream_t stream);
const char* attention_last_kernel_name();   // instantiation the calling thread's last attention_launch dispatched

// ---- misc.hip
int ln_fold_launch(const half_t* W, int N, int K, const half_t* gamma, const half_t* beta, const half_t* bias, half_t* Wout, half_t* bout,
                   float* wsum, hipStream_t stream);
// W'[C][5C] = [Wpo W2 | Wpo], b' = Wpo b2 + bpo (ff.net.2 followed by proj_out as one contraction; see misc.hip)
int mlp_out_fold_launch(const half_t* Wpo, const half_t* W2, const half_t* b2, const half_t* bpo, int C, half_t* Wout, half_t* bout, hipStream_t stream);
// W'[N][K9 + SC] = [W2 | Wsk], b' = b2 + bsk (a ResBlock's skip_connection as a second K segment of its out_layers convolution; see misc.hip)
int skip_fold_launch(const half_t* W2, const half_t* Wsk, const half_t* b2, const half_t* bsk, int N, int K9, int SC, half_t* Wout, half_t* bout,
                     hipStream_t stream);
// nearest-2x upsample + 3x3 convolution as four 2x2 convolutions of the source (gemm.h Wup): W [O][ky][kx][I] -> Wout [py*2+px][O][a*2+b][I], the
// 16 phase-tap matrices; a phase-tap is one 3x3 tap or the sum of two or four of them (fp32 sums, rounded to fp16 once; see misc.hip)
int upconv_fold_launch(const half_t* W, int O, int I, half_t* Wout, hipStream_t stream);
struct SmallConvInArgs {        // 3x3 pad-1 conv with <= 4 input channels from an fp32 NCHW tensor (conv_in of UNet / VAE)
    const float* x = nullptr;   // [N][Cin][H][W] fp32
    const float* scale_sigma = nullptr;  // optional [N]: input scaled by 1/sqrt(sigma^2+1) (EPS.calculate_input, LD.py:1259-1261)
    const half_t* pre_w = nullptr;       // optional 1x1 pre-conv [Cin][Cin] + bias (VAE post_quant_conv, LD.py:3467-3471)
    const half_t* pre_b = nullptr;
    const half_t* w = nullptr;  // [Cout][9*Cin] (tap-major, channel-minor)
    const half_t* b = nullptr;
    half_t* y = nullptr;        // NHWC [N][H][W][Cout]
    int N = 0, Cin = 0, H = 0, W = 0, Cout = 0;
    long long dup_off = 0;      // != 0: every output chunk is stored a second time at y + dup_off (elements): the second half of a CFG pair (unet.hip)
};
int small_conv_in_launch(const SmallConvInArgs& a, hipStream_t stream);

struct SmallConvOutArgs {       // 3x3 pad-1 conv to <= 4 output channels from an NHWC fp16 tensor
    const half_t* x = nullptr;  // [N][H][W][Cin]
    const half_t* w = nullptr;  // [Cout][9*Cin]
    const half_t* b = nullptr;
    int N = 0, H = 0, W = 0, Cin = 0, Cout = 0;
    int mode = 0;               // 0: UNet out -> denoised NCHW fp32 = x_in - fp16(eps)*sigma (EPS.calculate_denoised, LD.py:1263-1265)
                                // 1: VAE out  -> NHWC fp32 clamp((v+1)/2, 0, 1) (VAE.process_output, LD.py:6296-6298)
                                // 2: raw eps NCHW fp32 (tests)
    const float* x_in = nullptr;   // mode 0: [N][Cout][H][W] fp32
    const float* sigma = nullptr;  // mode 0: [N]
    float* out = nullptr;
    int in_mod = 0;                // > 0: x_in / sigma hold in_mod samples and sample n reads n % in_mod (CFG pair: both halves see the same latents)
};
int small_conv_out_launch(const SmallConvOutArgs& a, hipStream_t stream);
const char* small_conv_last_kernel_name();   // instantiation the calling thread's last small_conv_in_launch / small_conv_out_launch dispatched ("" = none)

// VAE output tail behind the MFMA output convolution: t8 [npix][8] fp16 (first `cout` columns valid) -> out [npix][cout] fp32 =
// clamp((v + 1) / 2, 0, 1)  (VAE.process_output, LD.py:6296-6298)
int vae_out_finish_launch(const half_t* t8, float* out, long long npix, int cout, hipStream_t stream);

int small_pointwise_launch(const half_t* x, const half_t* w, const half_t* b, float* out, int N, int HW, int C, hipStream_t stream);

// timestep lookup + sinusoidal embedding: sigma[N] -> t = argmin |log sigma - log_sigmas| -> [N][dim] fp16 (cos | sin)
// sigma_mod > 0: sigma holds sigma_mod samples and sample n reads sigma[n % sigma_mod] (CFG pair)
int timestep_embed_launch(const float* sigma, const float* log_sigmas, int n_sig, int N, int dim, half_t* out, float* t_out,
                          hipStream_t stream, int sigma_mod = 0);

// up to three ranges [base, base + bytes) copied to [base + bytes, base + 2 bytes) in one launch (the hand-over of a CFG pair's shared prefix, unet.hip)
struct DupArgs {
    char* base[3] = {nullptr, nullptr, nullptr};
    unsigned long long bytes[3] = {0, 0, 0};   // multiples of 16
    int count = 0;
};
int dup_halves_launch(const DupArgs& a, hipStream_t stream);

// weight repack (device side, run once at load)
int repack_conv3x3_launch(const void* src, int src_is_f32, int O, int I, half_t* dst, hipStream_t stream);  // OIHW -> [O][ky][kx][I]
int repack_rows_launch(const void* src, int src_is_f32, int rows, int cols, half_t* dst, int geglu_bn, hipStream_t stream);
int ctx_pad_launch(const void* src, int src_is_f32, int n, int T, int Tp, int D, half_t* dst, hipStream_t stream);

// sampler / guidance elementwise (fp32 latents)
int cfg_combine_launch(const float* den2, float* out, float cfg, size_t n_half, hipStream_t stream);   // out = u + (c-u)*cfg, den2=[u;c]
int axpby_launch(float* x, float a, const float* y, float b, const float* z, float c, size_t n, hipStream_t stream);  // x = a*x + b*y + c*z
// wrapper-hook guards: flags[0] = epoch when a != b (words_ab 32-bit words), flags[1] = epoch when the halves of x / sigma differ
int hook_check_launch(const void* a, const void* b, size_t words_ab, const void* x, size_t half_words_x, const void* sigma, int half_sigma,
                      int* flags, int epoch, hipStream_t stream);
// bislerp (LD.py:429-518): fp32 NCHW [n][c][h][w] -> [n][c][h_new][w_new]; tmp holds n*c*h*w_new floats (width pass first)
int bislerp_launch(const float* x, float* tmp, float* y, int n, int c, int h, int w, int h_new, int w_new, hipStream_t stream);

// ---- esrgan.hip
// The dense-block 3x3 convolution (stride 1, pad 1) of RRDBNet: y[.., c_off .. c_off + cout) = epilogue(conv3x3(x[.., 0 .. cin)))
//   v = acc + bias;  slope != 0: v = v > 0 ? v : slope v;  r1: v = s1 v + r1;  r2: v = s2 v + r2     (fp32, one rounding at the store)
// x: NHWC fp16, pixel pitch ldx >= cin (cin a multiple of 32 in [64, 192]); y: pitch ldy, cout in {32, 64}; y may be x itself with
// c_off >= cin (the dense concatenation in place), any other overlap of an output with the input is LD_ERR_ARG.  (h, w): the OUTPUT size;
// up != 0: x is [n][h / 2][w / 2] and is read through a nearest-2x upsampling.  y2: optional second copy of the output at channel 0.
struct EsrganConvArgs {
    const half_t* x = nullptr;
    int ldx = 0, cin = 0;
    int n = 0, h = 0, w = 0, up = 0;
    const half_t* wt = nullptr;     // [cout][ky][kx][cin]
    const half_t* bias = nullptr;   // [cout] or null
    half_t* y = nullptr;
    int ldy = 0, c_off = 0, cout = 0;
    half_t* y2 = nullptr;
    int ldy2 = 0;
    float slope = 0.f;
    const half_t* r1 = nullptr;
    int ldr1 = 0;
    float s1 = 1.f;
    const half_t* r2 = nullptr;
    int ldr2 = 0;
    float s2 = 1.f;
    int relu = 0;                   // read by TAESD's epilogue only (taesd.hip): v = relu?(acc + bias + r1)
};
int esrgan_conv_launch(const EsrganConvArgs& a, hipStream_t stream);
const char* esrgan_last_kernel_name();   // instantiation the calling thread's last esrgan_conv_launch dispatched ("" = none)
// The 3-channel ends of RRDBNet (LD.py:7092-7099, 7141-7149), one launch each.  conv_first: x fp32 NHWC [n][h][w][3], rounded to fp16 once,
// wt [64][ky][kx][3], to 64 channels at y (pixel pitch ldy >= 64) and, when given, a second copy at y2 (pitch ldy2); conv_last: the first 64
// channels of x (fp16 NHWC, pitch ldx >= 64), wt [3][ky][kx][64], to out fp32 NHWC [n][h][w][3].  Pitches are multiples of 8.
int esrgan_first_launch(const float* x, const half_t* wt, const half_t* bias, half_t* y, int ldy, half_t* y2, int ldy2, int n, int h, int w, hipStream_t stream);
int esrgan_last_launch(const half_t* x, int ldx, const half_t* wt, const half_t* bias, float* out, int n, int h, int w, hipStream_t stream);
// blocks of 256 threads for n * h * w pixels of `per_pixel` work items each (the end convolutions of esrgan.hip / taesd.hip); false when
// that is more than a grid's 2^31 - 1
static inline bool end_conv_grid(int n, int h, int w, int per_pixel, unsigned* blocks) {
    const long long nh = (long long)n * h;
    if (nh > 0x7fffffffLL) return false;
    const long long px = nh * w;                                   // below 2^62
    if (px > 0x7fffffffLL * 256 / per_pixel) return false;
    *blocks = (unsigned)((px * per_pixel + 255) / 256);
    return true;
}
// tiled_scale's blend (LD.py:7326-7352), fp32: out[oh][ow][c] += ps[th][tw][c] * my[y] * mx[x] at (y0, x0), div[oh][ow] += my[y] * mx[x];
// ps == null: the final out /= div
int tile_blend_launch(const float* ps, const float* my, const float* mx, int th, int tw, float* out, float* div, int oh, int ow, int y0, int x0, int c,
                      hipStream_t stream);

// ---- taesd.hip: the TAESD decoder's convolutions (LD.py:688-721), fp16 NHWC of pitch 64 between them
// 64 -> 64 on the halo-tile main loop of halo_conv.h: y = relu?(conv3x3(x) + bias? + residual?), fp32 to the one rounding at the store.
// (h, w): the OUTPUT size; up != 0: x is [n][h / 2][w / 2][64] and is read through a nearest-2x upsampling.  y must not overlap x;
// residual [n][h][w][64] may be any buffer but y.
int taesd_conv_launch(const half_t* x, int n, int h, int w, int up, const half_t* wt, const half_t* bias, const half_t* residual, int relu, half_t* y,
                      hipStream_t stream);
const char* taesd_last_kernel_name();   // instantiation the calling thread's last taesd_conv_launch dispatched ("" = none)
// The ends of the decoder, one launch each.  first: latent fp32 NHWC [n][h][w][4] -> 3 tanh(x / 3) rounded to fp16 once, wt [64][ky][kx][4], bias,
// ReLU -> y [n][h][w][64].  last: x [n][h][w][64], wt [3][ky][kx][64], bias -> out fp32 NHWC [n][h][w][3] = (v - 0.5) * 2 and, when img is
// given, the preview image uint8(clip(255 (out + 1) / 2, 0, 255)) [n][h][w][3].
int taesd_first_launch(const float* x, const half_t* wt, const half_t* bias, half_t* y, int n, int h, int w, hipStream_t stream);
int taesd_last_launch(const half_t* x, const half_t* wt, const half_t* bias, float* out, uint8_t* img, int n, int h, int w, hipStream_t stream);

// ---- image.hip: uint8 images, HWC (masks HW) with a row pitch in bytes, bit-identical to Pillow (see the file's header)
// separable resize of the in_w x in_h window at src to out_w x out_h: horizontal pass, then vertical, uint8 between them; a pass runs exactly when
// its size changes and then takes its taps (hcoef / vcoef: device [out][2 + k] ints = first input sample, tap count, k fixed-point taps with 22
// fractional bits, every (first + count) within the input: the host builds them); tmp: u8_resample_tmp_bytes(in_h, out_w, C), read when both run
int u8_resample_launch(const uint8_t* src, int spitch, int in_w, int in_h, int C, uint8_t* dst, int dpitch, int out_w, int out_h, const int* hcoef, int hk,
                       const int* vcoef, int vk, uint8_t* tmp, hipStream_t stream);
size_t u8_resample_tmp_bytes(int in_h, int out_w, int C);
// GaussianBlur(radius) of the one-channel w x h image at src (edges replicate at ITS border); tmp: u8_blur_tmp_bytes(w, h); src may be dst
int u8_box_weights(float radius, int* R, unsigned* ww, unsigned* fw);      // host only: one box pass's integer radius and weights
size_t u8_blur_tmp_bytes(int w, int h);
int u8_gaussian_blur_launch(const uint8_t* src, int spitch, uint8_t* dst, int dpitch, int w, int h, float radius, uint8_t* tmp, hipStream_t stream);
// dst[w x h] = 0 except the pw x ph rectangle at (px, py) (may hang over any edge): 255, or pat[ph][pw] when given
int u8_mask_launch(uint8_t* dst, int dpitch, int w, int h, int px, int py, int pw, int ph, const uint8_t* pat, int ppitch, hipStream_t stream);
// canvas[y0 .. y0 + h)[x0 .. x0 + w) = div255(tile a + canvas (255 - a)) per channel; the region must lie inside the cw x ch canvas
int u8_composite_launch(uint8_t* canvas, int cpitch, int cw, int ch, const uint8_t* tile, int tpitch, const uint8_t* alpha, int apitch, int x0, int y0, int w,
                        int h, int C, hipStream_t stream);
int u8_from_f32_launch(const float* x, uint8_t* y, size_t n, hipStream_t stream);    // uint8(clip(255 x, 0, 255)): truncation
int f32_from_u8_launch(const uint8_t* x, float* y, size_t n, hipStream_t stream);    // x / 255, correctly rounded

// ---- detail/detail_image.hip: the Detailer's fp32 canvas [H][W][C] and fp32 masks [H][W], pitches in FLOATS; uint8 images as above (see the file's header)
constexpr int F32_IMAGE_MAX_SIDE = 16384;      // a side of a canvas, tile or mask
constexpr int F32_BLUR_MAX_FEATHER = 127;      // 2 feather + 1 = 255 taps in LDS
// dst[y2 - y1][x2 - x1][C] = uint8(clip(255 x, 0, 255)), a truncation, of the window [y1, y2) x [x1, x2) of the cw x ch canvas; the window lies inside it
int f32_crop_u8_launch(const float* canvas, int cpitch, int cw, int ch, int C, int x1, int y1, int x2, int y2, uint8_t* dst, int dpitch, hipStream_t stream);
// the (2 feather + 1)^2 Gaussian of the w x h mask at src, reflect padding: a pass along x into tmp (f32_blur_tmp_bytes(w, h)), a pass along y into
// dst; taps: device [2 feather + 1] floats; feather 0: a copy (taps and tmp unused); feather < min(w, h) and <= F32_BLUR_MAX_FEATHER; dst may be src
size_t f32_blur_tmp_bytes(int w, int h);
int f32_gaussian_blur_launch(const float* src, int spitch, float* dst, int dpitch, int w, int h, int feather, const float* taps, float* tmp,
                             hipStream_t stream);
// canvas = (1 - a) canvas + a (tile / 255), every operation rounded, on the tw x th tile's window at (x0, y0) clipped to the cw x ch canvas
int f32_paste_u8_launch(float* canvas, int cpitch, int cw, int ch, int C, const uint8_t* tile, int tpitch, const float* alpha, int apitch, int tw, int th, int x0,
                        int y0, hipStream_t stream);

// ---- inpaint/inpaint.hip: the masked sampler step's two blends on fp32 NCHW latents [B][C][HW]; mask [Bm][Cm][HW], Bm in {1, B}, Cm in {1, C}, broadcast
// in the kernel; every fp32 operation rounded on its own, in the order written (see the file's header)
constexpr long long INPAINT_MAX_FLOATS = 1LL << 31;      // B * C * HW stays below it (32-bit indices): LD_ERR_SHAPE otherwise
// out = x * m + (noise * sigma[b] + latent) * (1 - m); sigma: device [B]; out may be x
int inpaint_blend_in_launch(const float* x, const float* mask, const float* latent, const float* noise, const float* sigma, float* out, int B, int C,
                            long long HW, int Bm, int Cm, hipStream_t stream);
// den = den * m + latent * (1 - m), in place
int inpaint_blend_out_launch(float* den, const float* mask, const float* latent, int B, int C, long long HW, int Bm, int Cm, hipStream_t stream);

// ---- regional/regional.hip: regional conditioning on fp32 NCHW latents [B][C][H][W] — one launch that builds a group's UNet input from its
// windows, one that reduces every group's output to the guided result; every fp32 operation rounded on its own, in the order written (see the
// file's header).  The descriptors are copied into the kernel arguments: the host arrays are read before the call returns.
constexpr int REGIONAL_MAX_ENTRIES = 16;                 // windows of one gather, entries of one combine: LD_ERR_SHAPE above it
constexpr long long REGIONAL_MAX_FLOATS = 1LL << 31;     // every tensor stays below it (32-bit indices): LD_ERR_SHAPE otherwise
struct RegionalWindow {                                  // (the layout of ld_regional_window)
    int y0, x0;
};
struct RegionalEntry {                                   // (the layout of ld_regional_entry)
    const float* out;                                    // the entry's UNet output [B][C][h][w]
    const float* mask;                                   // [mask_batch][H][W] on the latent's grid, or nullptr
    int list;                                            // 0: cond, 1: uncond
    int mask_batch;                                      // 1 or B (not looked at without a mask)
    int y0, x0, h, w;                                    // its area on the latent
    float strength, mask_strength;
};
// out[(j * B + b)][c][y][x] = x[b][c][y0_j + y][x0_j + x], j < k, all windows h x w
int regional_gather_launch(const float* x, float* out, int B, int C, int H, int W, int h, int w, const RegionalWindow* windows, int k, hipStream_t stream);
// result = u + (c - u) * cond_scale with, per list, pred = sum(out * mult) / (1e-37f + sum(mult)) over the entries that cover the pixel, in table order
int regional_combine_launch(const RegionalEntry* entries, int n, float cond_scale, float* result, int B, int C, int H, int W, hipStream_t stream);

// ---- control/control.hip: what ControlNet adds around the UNet executor's routes (see the file's header)
constexpr int CONTROL_MAX_SEGMENTS = 16;                 // segments of one control add: LD_ERR_SHAPE above it
constexpr long long CONTROL_MAX_HALFS = 1LL << 31;       // every tensor stays below it (32-bit indices): LD_ERR_SHAPE otherwise
struct ControlSegment {
    half_t* t;            // [n][per] fp16, updated in place
    const half_t* r;      // [r_n][per] fp16
    long long per;        // halves per sample
};
// t[s][e] = fp16(float(t[s][e]) + strength * float(r[s % r_n][e])) for every segment, one launch; r_n divides n.  The host array is read before the call returns.
int control_add_launch(const ControlSegment* segs, int count, int n, int r_n, float strength, hipStream_t stream);
// y [n][ho][wo][cout] = silu?(conv3x3 pad 1 at `stride` (1 | 2) of the input + bias), ho = (h - 1) / stride + 1; the input is x [n][h][w][cin] fp16 (cin a
// multiple of 8) or x_nchw_f32 [n][cin][h][w] fp32 (cin <= 4, rounded to fp16 once) — exactly one of the two; wt [cout][ky][kx][cin], cout a multiple of 8
int hint_conv_launch(const half_t* x, const float* x_nchw_f32, int n, int h, int w, int cin, const half_t* wt, const half_t* bias, int cout, int stride, int silu,
                     half_t* y, hipStream_t stream);

// LoRA merge into a resident weight slot (lora.hip; load-class, never on the per-step path):
//   dst = round_fp16( float(base) + sum_j scale_j * up_j[rows][rank_j] * down_j[rank_j][cols] ), fp32 products and sum, ONE rounding for all terms.
// (rows, cols) are the LOGICAL checkpoint matrix (a conv: cols = Cin * 9 in (i, ky, kx) order); base and dst are in the slot's RESIDENT layout
// `kind` (LORA_MAT rows as is, LORA_CONV3 [O][ky][kx][I], LORA_GEGLU the tile interleave of repack_rows_launch with geglu_bn = bn).
enum LoraLayoutKind { LORA_MAT = 0, LORA_CONV3 = 1, LORA_GEGLU = 2 };
struct LoraLayout {
    int kind = LORA_MAT;
    int rows = 0, cols = 0;
    int bn = 0;               // LORA_GEGLU: rows per interleaved tile
};
constexpr int LORA_MAX_TERMS = 8, LORA_MAX_RANK = 256;
struct LoraTerm {
    const void* up = nullptr;      // [rows][rank] row-major
    const void* down = nullptr;    // [rank][cols] row-major
    int f32 = 0;                   // both factors fp32 (else fp16)
    int rank = 0;
    float scale = 0.f;
};
struct LoraArgs {
    const half_t* base = nullptr;
    half_t* dst = nullptr;         // may alias base
    LoraLayout lay;
    int n_terms = 0;
    LoraTerm t[LORA_MAX_TERMS];
};
int lora_merge_launch(const LoraArgs& a, hipStream_t stream);
// resident layout -> checkpoint layout [rows][cols] (the inverse of the load-time repack; same index map as the merge)
int lora_read_launch(const half_t* resident, const LoraLayout& lay, half_t* dst, hipStream_t stream);

// ---- clip.hip
// CLIP input stage: out[b][l] = round_fp16(float(row(ids[b][l])) + float(pos[l])); row(id) = table[id] (id < V-1), extra[id - (V-1)] (fp32 side table
// of E textual-inversion vectors, V-1 <= id < V-1+E), table[V-1] (id == V-1+E: EOS stays the largest id); any other id: a row of zeros, no table read.
// h a multiple of 8, pointers 16-byte aligned; pos holds at least L rows.
int clip_embed_launch(const int* ids, const half_t* table, const float* extra, const half_t* pos, half_t* out, int B, int L, int V, int E, int h,
                      hipStream_t stream);
