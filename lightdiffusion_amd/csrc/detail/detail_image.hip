// fp32 image kernels behind the Detailer (detailer.py): the plumbing the reference does per segment on the host with numpy, torchvision and PIL
// (DetailerForEach.do_detail, LD.py:9402-9590), on a canvas that stays on the device as fp32 [H, W, 3]:
//   crop    tensor2pil of a window of the canvas: uint8(clip(255 x, 0, 255)) — one fp32 product, the clip, a truncation (the arithmetic of
//           image.hip's u8_from_f32_kernel, on a pitched source)
//   blur    torchvision's GaussianBlur(2 feather + 1, sigma) of an fp32 mask with reflect padding (no edge repeat): two separable passes from one
//           kernel (axis 0 = along x, then axis 1 = along y) over fp32 taps the host built, an fp32 temporary between them; every product and
//           every sum rounded on its own, in ascending tap order, so a result is the same bits run to run and the same bits as that order
//           written out in torch fp32 on the host
//   paste   pil2tensor + tensor_paste in place: canvas = (1 - a) canvas + a (tile / 255), five fp32 operations each rounded on its own
// Images are pitched — fp32 pitches in floats, uint8 pitches in bytes — so a window is a pointer and a pitch.  Every kernel is a grid-stride
// loop of 256-lane blocks on a capped grid whose consecutive lanes touch consecutive elements, and none reads or writes outside the windows
// it is given.  This unit is compiled with -ffp-contract=off (Makefile): __fmul_rn and its kin are plain operators in the HIP headers, and
// a product that feeds a sum would otherwise be contracted into one FMA.
#include <cstdint>

#include "../kernels.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 4096;
constexpr int kMaxTaps = 2 * F32_BLUR_MAX_FEATHER + 1;      // the LDS tap buffer
inline int grid_of(long long n) {
    long long b = (n + kBlock - 1) / kBlock;
    return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// ---- crop: a row is `rowf` flat floats, 4 of them per lane.  svec: every row of src starts 16-byte aligned; dvec: every row of dst 4-byte aligned
__global__ __launch_bounds__(kBlock) void crop_u8_kernel(const float* __restrict__ src, long long spitch, int rows, long long rowf, uint8_t* __restrict__ dst,
                                                         long long dpitch, int svec, int dvec) {
    const long long words = (rowf + 3) / 4;
    const long long total = (long long)rows * words;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const long long y = i / words, x = (i % words) * 4;
        const int nb = rowf - x < 4 ? (int)(rowf - x) : 4;
        const float* s = src + y * spitch + x;
        uint8_t* d = dst + y * dpitch + x;
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        if (svec && nb == 4) {
            const float4 v = *reinterpret_cast<const float4*>(s);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
        } else {
            for (int t = 0; t < nb; ++t) f[t] = s[t];
        }
        unsigned o = 0;
        for (int t = 0; t < 4; ++t) {
            float v = __fmul_rn(255.0f, f[t]);     // one fp32 product, then the clip, then a truncation (np.clip(255 x, 0, 255).astype(uint8))
            v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
            o |= (unsigned)(int)v << (8 * t);
        }
        if (dvec && nb == 4) {
            *reinterpret_cast<unsigned*>(d) = o;
        } else {
            for (int t = 0; t < nb; ++t) d[t] = (uint8_t)(o >> (8 * t));
        }
    }
}

// ---- blur: one pass along x (axis 0) or y (axis 1).  taps: 2 feather + 1 floats, staged in LDS; feather < the axis' length (the launch checks)
__device__ __forceinline__ int reflecti(int i, int n) {     // -k -> k, n - 1 + k -> n - 1 - k
    i = i < 0 ? -i : i;
    return i > n - 1 ? 2 * (n - 1) - i : i;
}

__global__ __launch_bounds__(kBlock) void gauss_axis_kernel(const float* __restrict__ src, long long spitch, float* __restrict__ dst, long long dpitch, int w,
                                                            int h, const float* __restrict__ taps, int feather, int axis) {
    __shared__ float st[kMaxTaps];
    const int n = 2 * feather + 1;
    for (int j = threadIdx.x; j < n; j += kBlock) st[j] = taps[j];
    __syncthreads();
    const long long total = (long long)h * w;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int y = (int)(i / w), x = (int)(i % w);
        float acc = 0.0f;
        if (axis == 0) {
            const float* s = src + (long long)y * spitch;
            for (int j = 0; j < n; ++j) acc = __fadd_rn(acc, __fmul_rn(st[j], s[reflecti(x + j - feather, w)]));
        } else {
            const float* s = src + x;
            for (int j = 0; j < n; ++j) acc = __fadd_rn(acc, __fmul_rn(st[j], s[(long long)reflecti(y + j - feather, h) * spitch]));
        }
        dst[(long long)y * dpitch + x] = acc;
    }
}

// ---- paste: one lane per canvas float of the window.  `canvas` points at the window's origin; a row of it is w C floats
__global__ __launch_bounds__(kBlock) void paste_u8_kernel(float* __restrict__ canvas, long long cpitch, const uint8_t* __restrict__ tile, long long tpitch,
                                                          const float* __restrict__ alpha, long long apitch, int w, int h, int C) {
    const int rowf = w * C;
    const long long total = (long long)h * rowf;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int y = (int)(i / rowf), xc = (int)(i % rowf);
        const float a = alpha[(long long)y * apitch + xc / C];
        float* cv = canvas + (long long)y * cpitch + xc;
        const float t = __fdiv_rn((float)tile[(long long)y * tpitch + xc], 255.0f);          // a division, not a reciprocal multiply
        *cv = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, a), *cv), __fmul_rn(a, t));                 // no FMA: every operation rounds
    }
}

inline int launched() { return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP; }
inline bool aligned(const void* p, long long pitch_bytes, unsigned to) { return (((uintptr_t)p | (uintptr_t)pitch_bytes) & (to - 1)) == 0; }
}  // namespace

int f32_crop_u8_launch(const float* canvas, int cpitch, int cw, int ch, int C, int x1, int y1, int x2, int y2, uint8_t* dst, int dpitch, hipStream_t stream) {
    if (canvas == nullptr || dst == nullptr || cw <= 0 || ch <= 0) return LD_ERR_ARG;
    if (!(0 <= x1 && x1 < x2 && x2 <= cw && 0 <= y1 && y1 < y2 && y2 <= ch)) return LD_ERR_ARG;      // the window lies inside the canvas
    if (C < 1 || C > 4 || cw > F32_IMAGE_MAX_SIDE || ch > F32_IMAGE_MAX_SIDE) return LD_ERR_SHAPE;
    long long rowf = (long long)(x2 - x1) * C;
    if (cpitch < cw * C || dpitch < rowf) return LD_ERR_SHAPE;
    const float* src = canvas + (long long)y1 * cpitch + (long long)x1 * C;
    int rows = y2 - y1;
    long long sp = cpitch, dp = dpitch;
    if (sp == rowf && dp == rowf) {               // dense on both sides: one flat row, so that only its tail leaves the vector path
        rowf *= rows;
        rows = 1;
        sp = dp = 0;
    }
    hipLaunchKernelGGL(crop_u8_kernel, dim3(grid_of(rows * ((rowf + 3) / 4))), dim3(kBlock), 0, stream, src, sp, rows, rowf, dst, dp,
                       (int)aligned(src, 4 * sp, 16), (int)aligned(dst, dp, 4));
    return launched();
}

size_t f32_blur_tmp_bytes(int w, int h) {
    if (w <= 0 || h <= 0) return 0;
    return (size_t)h * (size_t)((w + 3) / 4 * 4) * sizeof(float);
}

int f32_gaussian_blur_launch(const float* src, int spitch, float* dst, int dpitch, int w, int h, int feather, const float* taps, float* tmp,
                             hipStream_t stream) {
    if (src == nullptr || dst == nullptr || w <= 0 || h <= 0 || feather < 0) return LD_ERR_ARG;
    if (spitch < w || dpitch < w || w > F32_IMAGE_MAX_SIDE || h > F32_IMAGE_MAX_SIDE) return LD_ERR_SHAPE;
    if (feather >= (w < h ? w : h) || feather > F32_BLUR_MAX_FEATHER) return LD_ERR_SHAPE;      // reflection needs it; the LDS tap buffer
    if (feather == 0) {
        HIP_CHECK_RET(hipMemcpy2DAsync(dst, (size_t)dpitch * sizeof(float), src, (size_t)spitch * sizeof(float), (size_t)w * sizeof(float), h,
                                       hipMemcpyDeviceToDevice, stream));
        return LD_OK;
    }
    if (taps == nullptr || tmp == nullptr) return LD_ERR_ARG;
    const long long tp = (w + 3) / 4 * 4;
    const dim3 grid(grid_of((long long)h * w)), block(kBlock);
    hipLaunchKernelGGL(gauss_axis_kernel, grid, block, 0, stream, src, (long long)spitch, tmp, tp, w, h, taps, feather, 0);
    hipLaunchKernelGGL(gauss_axis_kernel, grid, block, 0, stream, (const float*)tmp, tp, dst, (long long)dpitch, w, h, taps, feather, 1);
    return launched();
}

int f32_paste_u8_launch(float* canvas, int cpitch, int cw, int ch, int C, const uint8_t* tile, int tpitch, const float* alpha, int apitch, int tw, int th, int x0,
                        int y0, hipStream_t stream) {
    if (canvas == nullptr || tile == nullptr || alpha == nullptr || cw <= 0 || ch <= 0 || tw <= 0 || th <= 0) return LD_ERR_ARG;
    if (x0 < 0 || y0 < 0 || x0 >= cw || y0 >= ch) return LD_ERR_ARG;                                   // the tile's origin lies inside the canvas
    if (C < 1 || C > 4 || cw > F32_IMAGE_MAX_SIDE || ch > F32_IMAGE_MAX_SIDE || tw > F32_IMAGE_MAX_SIDE || th > F32_IMAGE_MAX_SIDE) return LD_ERR_SHAPE;
    if (cpitch < cw * C || tpitch < tw * C || apitch < tw) return LD_ERR_SHAPE;
    const int w = (cw < x0 + tw ? cw : x0 + tw) - x0, h = (ch < y0 + th ? ch : y0 + th) - y0;          // the tile's window, clipped to the canvas
    hipLaunchKernelGGL(paste_u8_kernel, dim3(grid_of((long long)h * w * C)), dim3(kBlock), 0, stream, canvas + (long long)y0 * cpitch + (long long)x0 * C,
                       (long long)cpitch, tile, (long long)tpitch, alpha, (long long)apitch, w, h, C);
    return launched();
}
