// 8-bit image kernels behind UltimateSDUpscale (usdu.py): the plumbing the reference does with Pillow on the host, for every tile on the
// whole canvas (process_images, LD.py:7629-7739), kept on the device and bit-identical to Pillow's integer arithmetic:
//   resample   Image.resize(LANCZOS / BICUBIC): two separable passes over fixed-point taps the host built (22 fractional bits), uint8 between
//   blur       ImageFilter.GaussianBlur on an "L" image: three box passes along x, three along y, uint8 after each
//   composite  paste + putalpha + masked paste + alpha_composite + convert("RGB") over an opaque canvas = one div255 blend per byte
//   mask       the white rectangle (ImageDraw.rectangle) or the pasted gradient tile of one job, written into the window the blur reads
//   u8 <-> f32 tensor_to_pil's truncation and pil_to_tensor's correctly rounded division
// Images are uint8 HWC (masks HW) with a row pitch in bytes, so a crop is a pointer and a pitch.  Every kernel is a grid-stride loop whose
// consecutive lanes touch consecutive bytes; the passes that treat a row as flat bytes (vertical resample, vertical box, conversions) move
// 4 bytes per lane as one word where pointer and pitch allow and fall back to byte accesses where they do not.
#include <cstdint>

#include "kernels.h"

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 4096;
inline int grid_of(long long n) {
    long long b = (n + kBlock - 1) / kBlock;
    return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}
inline bool word_aligned(const void* p, int pitch) { return (((uintptr_t)p | (uintptr_t)pitch) & 3u) == 0; }

// up to 4 bytes at p as one little-endian word; `vec`: p is 4-byte aligned and all 4 bytes exist
__device__ __forceinline__ unsigned load4(const uint8_t* p, int n, bool vec) {
    if (vec && n == 4) return *reinterpret_cast<const unsigned*>(p);
    unsigned v = 0;
    for (int i = 0; i < n; ++i) v |= (unsigned)p[i] << (8 * i);
    return v;
}
__device__ __forceinline__ void store4(uint8_t* p, unsigned v, int n, bool vec) {
    if (vec && n == 4) {
        *reinterpret_cast<unsigned*>(p) = v;
        return;
    }
    for (int i = 0; i < n; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
__device__ __forceinline__ unsigned clip8(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// ---- resample.  coef: [out][2 + K] ints = first input sample, tap count, K taps (22 fractional bits)
__global__ __launch_bounds__(kBlock) void resample_h_kernel(const uint8_t* __restrict__ src, int spitch, int rows, int C, uint8_t* __restrict__ dst,
                                                            int dpitch, int out_w, const int* __restrict__ coef, int K) {
    const long long total = (long long)rows * out_w;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int y = (int)(i / out_w), xx = (int)(i % out_w);
        const int* co = coef + (long long)xx * (2 + K);
        const int x0 = co[0], n = co[1];
        const uint8_t* s = src + (long long)y * spitch + (long long)x0 * C;
        uint8_t* d = dst + (long long)y * dpitch + (long long)xx * C;
        for (int c = 0; c < C; ++c) {
            int acc = 1 << 21;
            for (int j = 0; j < n; ++j) acc += (int)s[j * C + c] * co[2 + j];
            d[c] = (uint8_t)clip8(acc >> 22);
        }
    }
}

// a row is `rowb` flat bytes: 4 of them per lane
__global__ __launch_bounds__(kBlock) void resample_v_kernel(const uint8_t* __restrict__ src, int spitch, int rowb, uint8_t* __restrict__ dst, int dpitch,
                                                            int out_h, const int* __restrict__ coef, int K, int svec, int dvec) {
    const int words = (rowb + 3) / 4;
    const long long total = (long long)out_h * words;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int yy = (int)(i / words), x = (int)(i % words) * 4;
        const int nb = rowb - x < 4 ? rowb - x : 4;
        const int* co = coef + (long long)yy * (2 + K);
        const int y0 = co[0], n = co[1];
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
        for (int j = 0; j < n; ++j) {
            const unsigned v = load4(src + (long long)(y0 + j) * spitch + x, nb, svec != 0);
            const int k = co[2 + j];
            a0 += (int)(v & 255u) * k;
            a1 += (int)((v >> 8) & 255u) * k;
            a2 += (int)((v >> 16) & 255u) * k;
            a3 += (int)(v >> 24) * k;
        }
        // (packed as two byte pairs 16 bits apart: the plain c0 | c1 << 8 | ... form compiles to v_ashr_pk_u8_i32, whose result's upper 16
        // bits hipcc takes for zero while the MI355X leaves other bits there — bytes 2 and 3 came out OR-ed with them)
        const unsigned even = clip8(a0 >> 22) | (clip8(a2 >> 22) << 16), odd = clip8(a1 >> 22) | (clip8(a3 >> 22) << 16);
        const unsigned o = even | (odd << 8);
        store4(dst + (long long)yy * dpitch + x, o, nb, dvec != 0);
    }
}

// ---- box blur: out[x] = (ww sum_{|d| <= R} in[clamp(x + d)] + fw (in[clamp(x - R - 1)] + in[clamp(x + R + 1)]) + 2^23) >> 24
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// along x: 4 outputs per lane on one sliding sum
__global__ __launch_bounds__(kBlock) void box_h_kernel(const uint8_t* __restrict__ src, int spitch, uint8_t* __restrict__ dst, int dpitch, int w, int h, int R,
                                                       unsigned ww, unsigned fw, int dvec) {
    const int words = (w + 3) / 4;
    const long long total = (long long)h * words;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int y = (int)(i / words), x = (int)(i % words) * 4;
        const int nb = w - x < 4 ? w - x : 4;
        const uint8_t* s = src + (long long)y * spitch;
        unsigned acc = 0;
        for (int d = -R; d <= R; ++d) acc += s[clampi(x + d, w - 1)];
        unsigned o = 0;
        for (int t = 0; t < nb; ++t) {
            const unsigned edge = (unsigned)s[clampi(x + t - R - 1, w - 1)] + (unsigned)s[clampi(x + t + R + 1, w - 1)];
            o |= ((acc * ww + edge * fw + (1u << 23)) >> 24) << (8 * t);
            acc += (unsigned)s[clampi(x + t + R + 1, w - 1)];
            acc -= (unsigned)s[clampi(x + t - R, w - 1)];
        }
        store4(dst + (long long)y * dpitch + x, o, nb, dvec != 0);
    }
}

// along y: 4 columns per lane, one word per tap
__global__ __launch_bounds__(kBlock) void box_v_kernel(const uint8_t* __restrict__ src, int spitch, uint8_t* __restrict__ dst, int dpitch, int w, int h, int R,
                                                       unsigned ww, unsigned fw, int svec, int dvec) {
    const int words = (w + 3) / 4;
    const long long total = (long long)h * words;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int y = (int)(i / words), x = (int)(i % words) * 4;
        const int nb = w - x < 4 ? w - x : 4;
        unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (int d = -R; d <= R; ++d) {
            const unsigned v = load4(src + (long long)clampi(y + d, h - 1) * spitch + x, nb, svec != 0);
            a0 += v & 255u;
            a1 += (v >> 8) & 255u;
            a2 += (v >> 16) & 255u;
            a3 += v >> 24;
        }
        const unsigned lo = load4(src + (long long)clampi(y - R - 1, h - 1) * spitch + x, nb, svec != 0);
        const unsigned hi = load4(src + (long long)clampi(y + R + 1, h - 1) * spitch + x, nb, svec != 0);
        const unsigned e0 = (lo & 255u) + (hi & 255u), e1 = ((lo >> 8) & 255u) + ((hi >> 8) & 255u);
        const unsigned e2 = ((lo >> 16) & 255u) + ((hi >> 16) & 255u), e3 = (lo >> 24) + (hi >> 24);
        const unsigned o = ((a0 * ww + e0 * fw + (1u << 23)) >> 24) | (((a1 * ww + e1 * fw + (1u << 23)) >> 24) << 8) |
                           (((a2 * ww + e2 * fw + (1u << 23)) >> 24) << 16) | (((a3 * ww + e3 * fw + (1u << 23)) >> 24) << 24);
        store4(dst + (long long)y * dpitch + x, o, nb, dvec != 0);
    }
}

// ---- mask window: 255 (or the pattern) inside the rectangle at (px, py), 0 elsewhere
__global__ __launch_bounds__(kBlock) void mask_kernel(uint8_t* __restrict__ dst, int dpitch, int w, int h, int px, int py, int pw, int ph,
                                                      const uint8_t* __restrict__ pat, int ppitch, int dvec) {
    const int words = (w + 3) / 4;
    const long long total = (long long)h * words;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int y = (int)(i / words), x = (int)(i % words) * 4;
        const int nb = w - x < 4 ? w - x : 4;
        const int ry = y - py;
        unsigned o = 0;
        if (ry >= 0 && ry < ph) {
            for (int t = 0; t < nb; ++t) {
                const int rx = x + t - px;
                if (rx >= 0 && rx < pw) o |= (pat != nullptr ? (unsigned)pat[(long long)ry * ppitch + rx] : 255u) << (8 * t);
            }
        }
        store4(dst + (long long)y * dpitch + x, o, nb, dvec != 0);
    }
}

// ---- composite: canvas = div255(tile a + canvas (255 - a)), div255(v) = ((v + 128) + ((v + 128) >> 8)) >> 8.  `canvas` points at the region's origin.
__global__ __launch_bounds__(kBlock) void composite_kernel(uint8_t* __restrict__ canvas, int cpitch, const uint8_t* __restrict__ tile, int tpitch,
                                                           const uint8_t* __restrict__ alpha, int apitch, int w, int h, int C) {
    const long long total = (long long)h * w;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int y = (int)(i / w), x = (int)(i % w);
        const unsigned a = alpha[(long long)y * apitch + x];
        uint8_t* cv = canvas + (long long)y * cpitch + (long long)x * C;
        const uint8_t* tl = tile + (long long)y * tpitch + (long long)x * C;
        for (int c = 0; c < C; ++c) {
            const unsigned v = (unsigned)tl[c] * a + (unsigned)cv[c] * (255u - a) + 128u;
            cv[c] = (uint8_t)((v + (v >> 8)) >> 8);
        }
    }
}

// ---- conversions, 4 elements per lane
__global__ __launch_bounds__(kBlock) void u8_from_f32_kernel(const float* __restrict__ x, uint8_t* __restrict__ y, size_t n, int vec) {
    const size_t words = (n + 3) / 4;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < words; i += (size_t)gridDim.x * kBlock) {
        const int nb = n - 4 * i < 4 ? (int)(n - 4 * i) : 4;
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && nb == 4) {
            const float4 v = *reinterpret_cast<const float4*>(x + 4 * i);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
        } else {
            for (int t = 0; t < nb; ++t) f[t] = x[4 * i + t];
        }
        unsigned o = 0;
        for (int t = 0; t < 4; ++t) {
            float v = 255.0f * f[t];              // one fp32 product, then the clip, then a truncation (np.clip(255 x, 0, 255).astype(uint8))
            v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
            o |= (unsigned)(int)v << (8 * t);
        }
        store4(y + 4 * i, o, nb, vec != 0);
    }
}

__global__ __launch_bounds__(kBlock) void f32_from_u8_kernel(const uint8_t* __restrict__ x, float* __restrict__ y, size_t n, int vec) {
    const size_t words = (n + 3) / 4;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < words; i += (size_t)gridDim.x * kBlock) {
        const int nb = n - 4 * i < 4 ? (int)(n - 4 * i) : 4;
        const unsigned v = load4(x + 4 * i, nb, vec != 0);
        float f[4];
        for (int t = 0; t < 4; ++t) f[t] = __fdiv_rn((float)((v >> (8 * t)) & 255u), 255.0f);   // a division, not a reciprocal multiply
        if (vec && nb == 4) {
            *reinterpret_cast<float4*>(y + 4 * i) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
            for (int t = 0; t < nb; ++t) y[4 * i + t] = f[t];
        }
    }
}

inline int launched() { return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP; }
}  // namespace

int u8_resample_launch(const uint8_t* src, int spitch, int in_w, int in_h, int C, uint8_t* dst, int dpitch, int out_w, int out_h, const int* hcoef, int hk,
                       const int* vcoef, int vk, uint8_t* tmp, hipStream_t stream) {
    if (src == nullptr || dst == nullptr || in_w <= 0 || in_h <= 0 || out_w <= 0 || out_h <= 0) return LD_ERR_ARG;
    if (C < 1 || C > 4 || spitch < in_w * C || dpitch < out_w * C) return LD_ERR_SHAPE;
    // a pass runs exactly when its size changes, and then needs its taps
    if ((in_w != out_w) != (hcoef != nullptr) || (in_h != out_h) != (vcoef != nullptr)) return LD_ERR_ARG;
    if ((hcoef != nullptr && hk <= 0) || (vcoef != nullptr && vk <= 0)) return LD_ERR_ARG;
    if (hcoef != nullptr && vcoef != nullptr && tmp == nullptr) return LD_ERR_ARG;
    if (hcoef == nullptr && vcoef == nullptr) {
        HIP_CHECK_RET(hipMemcpy2DAsync(dst, dpitch, src, spitch, (size_t)in_w * C, in_h, hipMemcpyDeviceToDevice, stream));
        return LD_OK;
    }
    const int rowb = out_w * C;
    const int tpitch = (rowb + 15) / 16 * 16;     // tmp: in_h rows of this pitch
    const uint8_t* vsrc = src;
    int vpitch = spitch;
    if (hcoef != nullptr) {
        uint8_t* hd = vcoef != nullptr ? tmp : dst;
        const int hp = vcoef != nullptr ? tpitch : dpitch;
        hipLaunchKernelGGL(resample_h_kernel, dim3(grid_of((long long)in_h * out_w)), dim3(kBlock), 0, stream, src, spitch, in_h, C, hd, hp, out_w, hcoef, hk);
        vsrc = hd;
        vpitch = hp;
    }
    if (vcoef != nullptr) {
        hipLaunchKernelGGL(resample_v_kernel, dim3(grid_of((long long)out_h * ((rowb + 3) / 4))), dim3(kBlock), 0, stream, vsrc, vpitch, rowb, dst, dpitch, out_h,
                           vcoef, vk, (int)word_aligned(vsrc, vpitch), (int)word_aligned(dst, dpitch));
    }
    return launched();
}

size_t u8_resample_tmp_bytes(int in_h, int out_w, int C) { return (size_t)in_h * (size_t)(((long long)out_w * C + 15) / 16 * 16); }

// _gaussian_blur_radius(radius, 3) and ImagingLineBoxBlur8's weights, in float32 and in the C code's order (no contraction into FMAs)
int u8_box_weights(float radius, int* R, unsigned* ww, unsigned* fw) {
#pragma clang fp contract(off)
    if (!(radius > 0.0f)) return LD_ERR_ARG;
    const float s2 = radius * radius / 3.0f;
    const float L = sqrtf(12.0f * s2 + 1.0f);
    const float l = floorf((L - 1.0f) / 2.0f);
    float a = (2.0f * l + 1.0f) * (l * (l + 1.0f) - 3.0f * s2);
    a = a / (6.0f * (s2 - (l + 1.0f) * (l + 1.0f)));
    const float fr = l + a;
    if (!(fr >= 0.0f) || fr > 4096.0f) return LD_ERR_SHAPE;
    *R = (int)fr;
    *ww = (unsigned)((float)(1 << 24) / (fr * 2.0f + 1.0f));
    *fw = ((1u << 24) - (unsigned)(2 * *R + 1) * *ww) / 2u;
    return LD_OK;
}

size_t u8_blur_tmp_bytes(int w, int h) { return 2 * (size_t)h * (size_t)((w + 15) / 16 * 16); }

int u8_gaussian_blur_launch(const uint8_t* src, int spitch, uint8_t* dst, int dpitch, int w, int h, float radius, uint8_t* tmp, hipStream_t stream) {
    if (src == nullptr || dst == nullptr || tmp == nullptr || w <= 0 || h <= 0) return LD_ERR_ARG;
    if (spitch < w || dpitch < w) return LD_ERR_SHAPE;
    int R = 0;
    unsigned ww = 0, fw = 0;
    const int st = u8_box_weights(radius, &R, &ww, &fw);
    if (st != LD_OK) return st;
    const int tp = (w + 15) / 16 * 16;
    uint8_t* a = tmp;
    uint8_t* b = tmp + (size_t)h * tp;
    const dim3 grid(grid_of((long long)h * ((w + 3) / 4))), block(kBlock);
    const int tv = (int)word_aligned(tmp, tp);
    hipLaunchKernelGGL(box_h_kernel, grid, block, 0, stream, src, spitch, a, tp, w, h, R, ww, fw, tv);
    hipLaunchKernelGGL(box_h_kernel, grid, block, 0, stream, (const uint8_t*)a, tp, b, tp, w, h, R, ww, fw, tv);
    hipLaunchKernelGGL(box_h_kernel, grid, block, 0, stream, (const uint8_t*)b, tp, a, tp, w, h, R, ww, fw, tv);
    hipLaunchKernelGGL(box_v_kernel, grid, block, 0, stream, (const uint8_t*)a, tp, b, tp, w, h, R, ww, fw, tv, tv);
    hipLaunchKernelGGL(box_v_kernel, grid, block, 0, stream, (const uint8_t*)b, tp, a, tp, w, h, R, ww, fw, tv, tv);
    hipLaunchKernelGGL(box_v_kernel, grid, block, 0, stream, (const uint8_t*)a, tp, dst, dpitch, w, h, R, ww, fw, tv, (int)word_aligned(dst, dpitch));
    return launched();
}

int u8_mask_launch(uint8_t* dst, int dpitch, int w, int h, int px, int py, int pw, int ph, const uint8_t* pat, int ppitch, hipStream_t stream) {
    if (dst == nullptr || w <= 0 || h <= 0 || pw < 0 || ph < 0) return LD_ERR_ARG;
    if (dpitch < w || (pat != nullptr && ppitch < pw)) return LD_ERR_SHAPE;
    hipLaunchKernelGGL(mask_kernel, dim3(grid_of((long long)h * ((w + 3) / 4))), dim3(kBlock), 0, stream, dst, dpitch, w, h, px, py, pw, ph, pat, ppitch,
                       (int)word_aligned(dst, dpitch));
    return launched();
}

int u8_composite_launch(uint8_t* canvas, int cpitch, int cw, int ch, const uint8_t* tile, int tpitch, const uint8_t* alpha, int apitch, int x0, int y0, int w,
                        int h, int C, hipStream_t stream) {
    if (canvas == nullptr || tile == nullptr || alpha == nullptr || cw <= 0 || ch <= 0 || w <= 0 || h <= 0) return LD_ERR_ARG;
    if (C < 1 || C > 4 || cpitch < cw * C || tpitch < w * C || apitch < w) return LD_ERR_SHAPE;
    if (x0 < 0 || y0 < 0 || x0 > cw - w || y0 > ch - h) return LD_ERR_ARG;      // the region lies inside the canvas
    hipLaunchKernelGGL(composite_kernel, dim3(grid_of((long long)h * w)), dim3(kBlock), 0, stream, canvas + (size_t)y0 * cpitch + (size_t)x0 * C, cpitch, tile,
                       tpitch, alpha, apitch, w, h, C);
    return launched();
}

int u8_from_f32_launch(const float* x, uint8_t* y, size_t n, hipStream_t stream) {
    if (x == nullptr || y == nullptr) return LD_ERR_ARG;
    if (n == 0) return LD_OK;
    const int vec = (((uintptr_t)x & 15u) == 0 && ((uintptr_t)y & 3u) == 0) ? 1 : 0;
    hipLaunchKernelGGL(u8_from_f32_kernel, dim3(grid_of((long long)((n + 3) / 4))), dim3(kBlock), 0, stream, x, y, n, vec);
    return launched();
}

int f32_from_u8_launch(const uint8_t* x, float* y, size_t n, hipStream_t stream) {
    if (x == nullptr || y == nullptr) return LD_ERR_ARG;
    if (n == 0) return LD_OK;
    const int vec = (((uintptr_t)y & 15u) == 0 && ((uintptr_t)x & 3u) == 0) ? 1 : 0;
    hipLaunchKernelGGL(f32_from_u8_kernel, dim3(grid_of((long long)((n + 3) / 4))), dim3(kBlock), 0, stream, x, y, n, vec);
    return launched();
}
