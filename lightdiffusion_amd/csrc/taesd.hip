// TAESD's decoder (Decoder2 / TAESD.decode, LD.py:688-754) on the device: the latent preview of the sampler loop.  The 64 -> 64
// convolutions run on the halo-tile main loop of halo_conv.h (the ESRGAN dense-block kernel's) under TAESD's epilogue; the 4 -> 64 and
// 64 -> 3 ends are plain kernels modelled on esrgan_first_kernel / esrgan_last_kernel; ld_taesd is the executor of the C ABI.
#include "halo_conv.h"
#include "runtime.h"
#include "../../include/ld_mi355x.h"

namespace {

// taesd_conv_kernel: halo_conv_tile with v = acc + bias (+ R when given), ReLU when asked: a Block's three convolutions (the third carries
// the skip and the fuse ReLU, LD.py:695-702) and the bias-free convolution behind each nearest-2x upsampling (UP).
struct TaesdEpilogue {
    static __device__ __forceinline__ float apply(const EsrganConvArgs& p, float v, float r1, float) {
        if (p.r1 != nullptr) v = v + r1;
        if (p.relu) v = v > 0.f ? v : 0.f;
        return v;
    }
};

template <bool UP>
__global__ __launch_bounds__(512, 1) void taesd_conv_kernel(const EsrganConvArgs p) {
    halo_conv_tile<64, UP, TaesdEpilogue>(p);
}

// ---- Clamp + the first convolution + ReLU (LD.py:691-693, 716): the fp32 NHWC latent [n][h][w][4] -> 3 tanh(x / 3) in fp32, rounded to
// fp16 once, 3x3 pad-1 convolution to 64 channels, bias, ReLU.  One thread per (pixel, 8 output channels); the 64 x 36 weights sit in LDS.
__global__ __launch_bounds__(256) void taesd_first_kernel(const float* x, const half_t* wt, const half_t* bias, half_t* y, int n, int h, int w) {
    __shared__ float ws[64 * 36];
    for (int i = threadIdx.x; i < 64 * 36; i += 256) ws[i] = (float)wt[i];
    __syncthreads();
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long pix = q >> 3;
    const int cg = (int)(q & 7);
    if (pix >= (long long)n * h * w) return;
    const int ix = (int)(pix % w), iy = (int)((pix / w) % h);
    float v[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) v[o] = (float)bias[cg * 8 + o];
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const int sy = iy + ky - 1, sx = ix + kx - 1;
            if ((unsigned)sy >= (unsigned)h || (unsigned)sx >= (unsigned)w) continue;
            const float4 s = *reinterpret_cast<const float4*>(x + (pix + (long long)(ky - 1) * w + (kx - 1)) * 4);
            const float a[4] = {(float)(half_t)(tanhf(s.x / 3.0f) * 3.0f), (float)(half_t)(tanhf(s.y / 3.0f) * 3.0f),
                                (float)(half_t)(tanhf(s.z / 3.0f) * 3.0f), (float)(half_t)(tanhf(s.w / 3.0f) * 3.0f)};
            const float* wp = ws + (cg * 8) * 36 + (ky * 3 + kx) * 4;
#pragma unroll
            for (int o = 0; o < 8; ++o) v[o] += a[0] * wp[o * 36] + a[1] * wp[o * 36 + 1] + a[2] * wp[o * 36 + 2] + a[3] * wp[o * 36 + 3];
        }
#pragma unroll
    for (int o = 0; o < 8; ++o) v[o] = v[o] > 0.f ? v[o] : 0.f;
    st16(y + pix * 64 + cg * 8, pack8(v));
}

// ---- the last convolution (LD.py:720) and TAESD.decode's output map (LD.py:753): 64 -> 3 with bias, d = (c - 0.5) * 2 as fp32 NHWC
// [n][h][w][3]; with img != null also the preview image uint8(clip(255 ((d + 1) * 0.5), 0, 255)), fp32 in that order, truncated (what
// u8_from_f32_kernel makes of (d + 1) * 0.5).  One thread per pixel; packed fp16 dot products with fp32 accumulation.
__global__ __launch_bounds__(256) void taesd_last_kernel(const half_t* x, const half_t* wt, const half_t* bias, float* out, uint8_t* img, int n, int h, int w) {
    __shared__ __attribute__((aligned(16))) half_t ws[3 * 9 * 64];
    for (int i = threadIdx.x; i < 3 * 9 * 64 / 8; i += 256) st16(ws + i * 8, ld16(wt + i * 8));
    __syncthreads();
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)n * h * w) return;
    const int ix = (int)(pix % w), iy = (int)((pix / w) % h);
    float v[3] = {(float)bias[0], (float)bias[1], (float)bias[2]};
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const int sy = iy + ky - 1, sx = ix + kx - 1;
            if ((unsigned)sy >= (unsigned)h || (unsigned)sx >= (unsigned)w) continue;
            const half_t* src = x + (pix + (long long)(ky - 1) * w + (kx - 1)) * 64;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint4 a = ld16(src + c * 8);
                const unsigned aw[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    const uint4 b = ld16(ws + (o * 9 + ky * 3 + kx) * 64 + c * 8);
                    const unsigned bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[o] = __builtin_amdgcn_fdot2(__builtin_bit_cast(half2v, aw[e]), __builtin_bit_cast(half2v, bw[e]), v[o], false);
                }
            }
        }
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        const float d = (v[o] - 0.5f) * 2.0f;
        out[pix * 3 + o] = d;
        if (img != nullptr) {
            float t = 255.0f * ((d + 1.0f) * 0.5f);
            t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
            img[pix * 3 + o] = (uint8_t)(int)t;
        }
    }
}

thread_local const char* t_last_taesd_kernel = "";

inline bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const char *pa = (const char*)a, *pb = (const char*)b;
    return pa < pb + bbytes && pb < pa + abytes;
}

}  // namespace

const char* taesd_last_kernel_name() { return t_last_taesd_kernel; }

int taesd_first_launch(const float* x, const half_t* wt, const half_t* bias, half_t* y, int n, int h, int w, hipStream_t stream) {
    if (x == nullptr || wt == nullptr || bias == nullptr || y == nullptr) return LD_ERR_ARG;
    if (n < 1 || h < 1 || w < 1) return LD_ERR_SHAPE;
    unsigned blocks = 0;
    if (!end_conv_grid(n, h, w, 8, &blocks)) return LD_ERR_SHAPE;
    hipLaunchKernelGGL(taesd_first_kernel, dim3(blocks), dim3(256), 0, stream, x, wt, bias, y, n, h, w);
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}

int taesd_last_launch(const half_t* x, const half_t* wt, const half_t* bias, float* out, uint8_t* img, int n, int h, int w, hipStream_t stream) {
    if (x == nullptr || wt == nullptr || bias == nullptr || out == nullptr) return LD_ERR_ARG;
    if (n < 1 || h < 1 || w < 1) return LD_ERR_SHAPE;
    unsigned blocks = 0;
    if (!end_conv_grid(n, h, w, 1, &blocks)) return LD_ERR_SHAPE;
    hipLaunchKernelGGL(taesd_last_kernel, dim3(blocks), dim3(256), 0, stream, x, wt, bias, out, img, n, h, w);
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}

int taesd_conv_launch(const half_t* x, int n, int h, int w, int up, const half_t* wt, const half_t* bias, const half_t* residual, int relu, half_t* y,
                      hipStream_t stream) {
    t_last_taesd_kernel = "";
    if (x == nullptr || wt == nullptr || y == nullptr) return LD_ERR_ARG;
    if (n < 1 || h < 1 || w < 1) return LD_ERR_SHAPE;
    if (up && ((h | w) & 1)) return LD_ERR_SHAPE;
    const long long npix = (long long)n * h * w, nsrc = up ? npix / 4 : npix;
    const long long tiles = (long long)n * ((h + EG_TH - 1) / EG_TH) * ((w + EG_TW - 1) / EG_TW);
    if (tiles > 0x7fffffffLL) return LD_ERR_SHAPE;
    const size_t ybytes = (size_t)npix * 64 * sizeof(half_t);
    if (ranges_overlap(x, (size_t)nsrc * 64 * sizeof(half_t), y, ybytes)) return LD_ERR_ARG;   // a tile's halo is another tile's output
    if (residual != nullptr && ranges_overlap(residual, ybytes, y, ybytes)) return LD_ERR_ARG;
    EsrganConvArgs a;
    a.x = x; a.ldx = 64; a.cin = 64;
    a.n = n; a.h = h; a.w = w; a.up = up;
    a.wt = wt; a.bias = bias;
    a.y = y; a.ldy = 64; a.c_off = 0; a.cout = 64;
    a.r1 = residual; a.ldr1 = 64;
    a.relu = relu ? 1 : 0;
    const dim3 grid((unsigned)tiles), block(512);
    if (up) { hipLaunchKernelGGL((taesd_conv_kernel<true>), grid, block, 0, stream, a); t_last_taesd_kernel = "taesd_conv_kernel<up>"; }
    else { hipLaunchKernelGGL((taesd_conv_kernel<false>), grid, block, 0, stream, a); t_last_taesd_kernel = "taesd_conv_kernel"; }
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}

// =====================================================================================================================
// ld_taesd: Decoder2 (state-dict keys of taesd_decoder.safetensors) on the kernels above, 35 launches: the first convolution, three
// stages of 3 Blocks (3 convolutions each) + the upsampling convolution, one Block, the last convolution (which also writes the image).
// Workspace: three 64-channel buffers of the OUTPUT resolution that rotate: a Block reads its input, writes its two intermediates into the
// other two, and its result over the first intermediate; an upsampling convolution writes the next buffer.
// =====================================================================================================================
struct ld_taesd : Model {
    int first_w = -1, first_b = -1, last_w = -1, last_b = -1;
    int blk_w[10][3], blk_b[10][3];
    int up_w[3];
};

namespace {

int taesd_build(ld_taesd* t) {
    ParamTable& pt = t->pt;
    t->first_w = pt.add("1.weight", PK_CONV3, {64, 4, 3, 3});
    t->first_b = pt.add("1.bias", PK_VEC, {64});
    int idx = 3, blk = 0;
    auto block = [&] {
        for (int k = 0; k < 3; ++k) {
            const std::string base = std::to_string(idx) + ".conv." + std::to_string(2 * k);
            t->blk_w[blk][k] = pt.add(base + ".weight", PK_CONV3, {64, 64, 3, 3});
            t->blk_b[blk][k] = pt.add(base + ".bias", PK_VEC, {64});
        }
        ++idx;
        ++blk;
    };
    for (int s = 0; s < 3; ++s) {
        for (int j = 0; j < 3; ++j) block();
        ++idx;                                                       // nn.Upsample holds no parameters
        t->up_w[s] = pt.add(std::to_string(idx++) + ".weight", PK_CONV3, {64, 64, 3, 3});
    }
    block();
    t->last_w = pt.add(std::to_string(idx) + ".weight", PK_CONV3, {3, 64, 3, 3});
    t->last_b = pt.add(std::to_string(idx) + ".bias", PK_VEC, {3});
    return pt.finalize();
}

int taesd_run(ld_taesd* t, bool dry, const float* latent, float* out, uint8_t* img, int b, int h, int w, hipStream_t stream, size_t* dry_peak = nullptr) {
    if ((long long)b * h * w * 64 > 0x7fffffffLL) return LD_ERR_SHAPE;
    Arena plan;
    Exec ex = t->begin(dry, stream, plan);
    Arena& ar = *ex.arena;
    const ParamTable& pt = t->pt;
    const size_t opix = (size_t)b * h * w * 64;
    half_t* buf[3] = {ar.halfs(opix * 64), ar.halfs(opix * 64), ar.halfs(opix * 64)};
    int H = h, W = w, cur = 0;

    auto conv = [&](const half_t* x, int up, int wslot, int bslot, const half_t* res, int relu, half_t* y) {
        ex.launch(KC_CONV3, 2.0 * b * H * (double)W * 64 * 576, up ? "upconv3" : "conv3", (long long)b * H * W, 64, 576, 1, taesd_last_kernel_name,
                  [&] { return taesd_conv_launch(x, b, H, W, up, pt.ptr(wslot), pt.ptr(bslot), res, relu, y, stream); });
    };
    auto block = [&](int k) {   // relu(conv(relu(conv(relu(conv(x))))) + x)
        half_t *x = buf[cur], *t1 = buf[(cur + 1) % 3], *t2 = buf[(cur + 2) % 3];
        conv(x, 0, t->blk_w[k][0], t->blk_b[k][0], nullptr, 1, t1);
        conv(t1, 0, t->blk_w[k][1], t->blk_b[k][1], nullptr, 1, t2);
        conv(t2, 0, t->blk_w[k][2], t->blk_b[k][2], x, 1, t1);
        cur = (cur + 1) % 3;
    };

    const long long npix = (long long)b * h * w;
    ex.launch(KC_MISC, 2.0 * npix * 64 * 36, "conv_first", npix, 64, 36, 1, "taesd_first_kernel", [&] {
        return taesd_first_launch(latent, pt.ptr(t->first_w), pt.ptr(t->first_b), buf[0], b, h, w, stream);
    });
    int k = 0;
    for (int s = 0; s < 3; ++s) {
        for (int j = 0; j < 3; ++j) block(k++);
        H *= 2; W *= 2;
        conv(buf[cur], 1, t->up_w[s], -1, nullptr, 0, buf[(cur + 1) % 3]);
        cur = (cur + 1) % 3;
    }
    block(k);
    const long long lpix = (long long)b * H * W;
    ex.launch(KC_MISC, 2.0 * lpix * 3 * 576, "conv_last", lpix, 3, 576, 1, "taesd_last_kernel", [&] {
        return taesd_last_launch(buf[cur], pt.ptr(t->last_w), pt.ptr(t->last_b), out, img, b, H, W, stream);
    });
    return t->end(ex, dry_peak, !dry);
}

}  // namespace

extern "C" {

int ld_taesd_create(ld_taesd** out) {
    if (out == nullptr) return LD_ERR_ARG;
    ld_taesd* t = new ld_taesd();
    const int st = taesd_build(t);
    if (st != LD_OK) {
        ld_taesd_destroy(t);
        return st;
    }
    *out = t;
    return LD_OK;
}

void ld_taesd_destroy(ld_taesd* t) {
    if (t == nullptr) return;
    t->destroy_common();
    delete t;
}

int ld_taesd_param_count(const ld_taesd* t) { return abi_param_count(t); }
int ld_taesd_param_info(const ld_taesd* t, int i, const char** name, int* ndim, int64_t shape[4]) { return abi_param_info(t, i, name, ndim, shape); }
int ld_taesd_load_param(ld_taesd* t, const char* name, const void* src, int dtype, void* stream) { return abi_load_param(t, name, src, dtype, stream); }
size_t ld_taesd_workspace_bytes(const ld_taesd* t) { return abi_workspace_bytes(t); }
int ld_taesd_last_launches(const ld_taesd* t) { return abi_last_launches(t); }
double ld_taesd_last_flops(const ld_taesd* t) { return abi_last_flops(t); }
int ld_taesd_profile_launches(const ld_taesd* t, char* buf, size_t buf_bytes) { return abi_profile_launches(t, buf, buf_bytes); }

size_t ld_taesd_plan_bytes(ld_taesd* t, int b, int h, int w) {
    return abi_plan_bytes(t, b, h, w, [&](size_t* peak) { return taesd_run(t, true, nullptr, nullptr, nullptr, b, h, w, nullptr, peak); });
}

int ld_taesd_reserve(ld_taesd* t, int max_b, int max_h, int max_w) {
    if (t == nullptr || max_b < 1 || max_h < 1 || max_w < 1) return LD_ERR_ARG;
    const size_t bytes = ld_taesd_plan_bytes(t, max_b, max_h, max_w);   // (planned before the old workspace goes)
    if (bytes == 0) return LD_ERR_SHAPE;
    return t->set_workspace(bytes, bytes - 4096);
}

int ld_taesd_decode(ld_taesd* t, const float* latent, float* out_f32, void* out_u8, int b, int h, int w, void* stream) {
    if (t == nullptr || latent == nullptr || out_f32 == nullptr) return LD_ERR_ARG;
    return abi_checked_run(*t, true, b >= 1 && h >= 1 && w >= 1,
                           [&](size_t* peak) { return taesd_run(t, true, nullptr, nullptr, nullptr, b, h, w, nullptr, peak); },
                           [&] { return taesd_run(t, false, latent, out_f32, (uint8_t*)out_u8, b, h, w, (hipStream_t)stream); });
}

int ld_taesd_profile(ld_taesd* t, const float* latent, float* out_f32, void* out_u8, int b, int h, int w, void* stream) {
    return abi_profile(t, stream, [&] { return ld_taesd_decode(t, latent, out_f32, out_u8, b, h, w, stream); });
}

}  // extern "C"
