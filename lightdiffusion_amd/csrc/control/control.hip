// ControlNet (upstream ComfyUI's cldm.ControlNet; the reference keeps its seams and fills none of them: apply_control1 returns h, LD.py:5290), the
// kernels around the control branch, which itself runs on the UNet executor's contraction, GroupNorm and attention routes (unet.hip):
//   control add   t[i] = fp16(float(t[i]) + strength * float(r[i % (r_n * per)])) in place, over a table of up to 16 segments in ONE launch: the skip
//                 tensors and the middle tensor of one UNet forward (apply_control1 at "output" and "middle"), and conv_in's output + the encoded hint
//                 (strength 1).  A segment is [n][per] halves, its residual [r_n][per]: sample s reads residual sample s % r_n.  One fp32 product and
//                 one fp32 sum, each rounded on its own (__fmul_rn / __fadd_rn: never an FMA), one rounding to fp16: the bits of the expression
//                 written in torch.  Bandwidth bound: 16-byte loads and stores where every segment's `per` is a multiple of 8 and every pointer
//                 is 16-byte aligned, single halves otherwise — the same bits either way.  The table travels BY VALUE in the kernel arguments
//                 (as regional.hip's): nothing to upload, capturable.
//   hint conv     one layer of the hint encoder (upstream's input_hint_block: eight 3x3 pad-1 convolutions 3 -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 ->
//                 256 -> model_channels, stride 2 at the third, fifth and seventh, SiLU behind all but the last).  The contraction family needs
//                 C1 % 64 == 0 (gemm.hip), so these widths have a direct kernel of their own: NHWC fp16 activations, weights [Cout][ky][kx][Cin],
//                 fp32 accumulation from zero in the order (ky, kx, ci), then + bias, SiLU (silu_f) in fp32, ONE rounding to fp16 at the store.  A
//                 work item is four output pixels of one row by eight output channels; blockIdx.y is the channel group, so the weights of a wave are
//                 uniform.  The first layer reads the fp32 NCHW image directly and rounds every sample to fp16 once (as esrgan_first / taesd_first
//                 do).  It runs once per sampler run, not per step: no MFMA pipeline.
// Indices are 32-bit inside a tensor: a tensor of 2^31 elements or more is refused.
#include <cstdint>

#include "../kernels.h"

// The control add's product must not be contracted into an FMA with the sum it feeds (the intrinsics alone do not stop hipcc; the Makefile gives
// the unit -ffp-contract=off as well, as it does for inpaint.hip and regional.hip).  The hint convolution's FMAs are explicit fmaf calls.
#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;
using I = unsigned;

struct ControlTable {
    half_t* t[CONTROL_MAX_SEGMENTS];
    const half_t* r[CONTROL_MAX_SEGMENTS];
    I per[CONTROL_MAX_SEGMENTS];
};

__device__ __forceinline__ half_t add1(half_t t, half_t r, float strength) { return (half_t)__fadd_rn((float)t, __fmul_rn(strength, (float)r)); }

// blockIdx.y: the segment.  One work item = V consecutive halves; V == 8: `per` is a multiple of 8, so the eight lie in one sample.  The grid-stride
// increment, at most 2^19 * V, added to an index below 2^31 / V cannot wrap.
template <int V>
__global__ __launch_bounds__(kBlock) void control_add_kernel(const ControlTable tab, I n, I r_n, float strength) {
    const int s = blockIdx.y;
    half_t* __restrict__ t = tab.t[s];
    const half_t* __restrict__ r = tab.r[s];
    const I per = tab.per[s], total = n * per / V, rmod = r_n * per;
    for (I i = (I)blockIdx.x * kBlock + threadIdx.x; i < total; i += (I)gridDim.x * kBlock) {
        const I e = i * V, re = e % rmod;
        if (V == 8) {
            H8 a, b;
            a.u = ld16(t + e);
            b.u = ld16(r + re);
#pragma unroll
            for (int k = 0; k < 8; ++k) a.e[k] = add1(a.e[k], b.e[k], strength);
            st16(t + e, a.u);
        } else {
            t[e] = add1(t[e], r[re], strength);
        }
    }
}

constexpr int kPx = 4, kCo = 8;     // output pixels (of one row) and output channels of a work item

struct HintConvArgs {
    const half_t* x;        // [N][H][W][Cin] fp16, or
    const float* x32;       // [N][Cin][H][W] fp32 (FIRST)
    const half_t* w;        // [Cout][3][3][Cin]
    const half_t* b;        // [Cout]
    half_t* y;              // [N][Ho][Wo][Cout]
    int N, H, W, Cin, Cout, stride, Ho, Wo, silu;
    I quads;                // N * Ho * ceil(Wo / 4)
};

template <bool FIRST>
__global__ __launch_bounds__(kBlock) void hint_conv_kernel(const HintConvArgs a) {
    const I q = (I)blockIdx.x * kBlock + threadIdx.x;
    if (q >= a.quads) return;
    const int wq = (a.Wo + kPx - 1) / kPx;
    const int xq = (int)(q % (I)wq), row = (int)(q / (I)wq), oy = row % a.Ho, img = row / a.Ho;
    const int co0 = blockIdx.y * kCo, ox0 = xq * kPx;
    float acc[kPx][kCo];
#pragma unroll
    for (int p = 0; p < kPx; ++p)
#pragma unroll
        for (int c = 0; c < kCo; ++c) acc[p][c] = 0.f;
    const size_t wrow = (size_t)9 * a.Cin;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * a.stride + ky - 1;
        if (iy < 0 || iy >= a.H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const half_t* wt = a.w + (size_t)co0 * wrow + (size_t)(ky * 3 + kx) * a.Cin;
            int ix[kPx];
            bool in[kPx];
#pragma unroll
            for (int p = 0; p < kPx; ++p) {
                ix[p] = (ox0 + p) * a.stride + kx - 1;
                in[p] = ox0 + p < a.Wo && ix[p] >= 0 && ix[p] < a.W;
            }
            if (FIRST) {
                for (int ci = 0; ci < a.Cin; ++ci) {
                    float wv[kCo];
#pragma unroll
                    for (int c = 0; c < kCo; ++c) wv[c] = (float)wt[(size_t)c * wrow + ci];
                    const float* src = a.x32 + (((size_t)img * a.Cin + ci) * a.H + iy) * a.W;
#pragma unroll
                    for (int p = 0; p < kPx; ++p) {
                        if (!in[p]) continue;
                        const float v = (float)(half_t)src[ix[p]];           // the image, rounded to fp16 once
#pragma unroll
                        for (int c = 0; c < kCo; ++c) acc[p][c] = fmaf(v, wv[c], acc[p][c]);
                    }
                }
            } else {
                const half_t* src = a.x + ((size_t)img * a.H + iy) * a.W * a.Cin;
                for (int ci = 0; ci < a.Cin; ci += 8) {
                    float xv[kPx][8];
#pragma unroll
                    for (int p = 0; p < kPx; ++p) {
                        if (in[p]) {
                            unpack8(ld16(src + (size_t)ix[p] * a.Cin + ci), xv[p]);
                        } else {
#pragma unroll
                            for (int k = 0; k < 8; ++k) xv[p][k] = 0.f;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < kCo; ++c) {
                        float wv[8];
                        unpack8(ld16(wt + (size_t)c * wrow + ci), wv);
#pragma unroll
                        for (int p = 0; p < kPx; ++p)
#pragma unroll
                            for (int k = 0; k < 8; ++k) acc[p][c] = fmaf(xv[p][k], wv[k], acc[p][c]);
                    }
                }
            }
        }
    }
    float bias[kCo];
    unpack8(ld16(a.b + co0), bias);
#pragma unroll
    for (int p = 0; p < kPx; ++p) {
        if (ox0 + p >= a.Wo) continue;
        float v[kCo];
#pragma unroll
        for (int c = 0; c < kCo; ++c) {
            v[c] = acc[p][c] + bias[c];
            if (a.silu) v[c] = silu_f(v[c]);
        }
        st16(a.y + (((size_t)img * a.Ho + oy) * a.Wo + ox0 + p) * a.Cout + co0, pack8(v));
    }
}

inline int launched() { return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

int control_add_launch(const ControlSegment* segs, int count, int n, int r_n, float strength, hipStream_t stream) {
    if (segs == nullptr) return LD_ERR_ARG;
    if (count < 1 || count > CONTROL_MAX_SEGMENTS || n < 1 || r_n < 1 || n % r_n != 0) return LD_ERR_SHAPE;   // (before the table is read: it has count rows)
    ControlTable tab = {};
    bool vec = true;
    long long most = 0;
    for (int s = 0; s < count; ++s) {
        if (segs[s].t == nullptr || segs[s].r == nullptr) return LD_ERR_ARG;
        if (segs[s].per < 1 || (long long)n * segs[s].per >= CONTROL_MAX_HALFS) return LD_ERR_SHAPE;
        tab.t[s] = segs[s].t;
        tab.r[s] = segs[s].r;
        tab.per[s] = (I)segs[s].per;
        vec = vec && segs[s].per % 8 == 0 && aligned16(segs[s].t) && aligned16(segs[s].r);
        if ((long long)n * segs[s].per > most) most = (long long)n * segs[s].per;
    }
    const long long items = (most / (vec ? 8 : 1) + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(items < 1 ? 1 : (items > kMaxBlocks ? kMaxBlocks : items)), (unsigned)count);
    if (vec) hipLaunchKernelGGL(control_add_kernel<8>, grid, dim3(kBlock), 0, stream, tab, (I)n, (I)r_n, strength);
    else hipLaunchKernelGGL(control_add_kernel<1>, grid, dim3(kBlock), 0, stream, tab, (I)n, (I)r_n, strength);
    return launched();
}

int hint_conv_launch(const half_t* x, const float* x_nchw_f32, int n, int h, int w, int cin, const half_t* wt, const half_t* bias, int cout, int stride, int silu,
                     half_t* y, hipStream_t stream) {
    if ((x == nullptr) == (x_nchw_f32 == nullptr) || wt == nullptr || bias == nullptr || y == nullptr) return LD_ERR_ARG;
    if (n < 1 || h < 1 || w < 1 || cin < 1 || cout < 8 || cout % 8 != 0 || (stride != 1 && stride != 2)) return LD_ERR_SHAPE;
    if (x != nullptr ? cin % 8 != 0 : cin > 4) return LD_ERR_SHAPE;           // fp16 input: 16-byte channel chunks; the fp32 image: a few planes
    if (!aligned16(wt) || !aligned16(bias) || !aligned16(y) || (x != nullptr && !aligned16(x))) return LD_ERR_SHAPE;
    HintConvArgs a;
    a.x = x; a.x32 = x_nchw_f32; a.w = wt; a.b = bias; a.y = y;
    a.N = n; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout; a.stride = stride; a.silu = silu;
    a.Ho = (h - 1) / stride + 1;
    a.Wo = (w - 1) / stride + 1;
    const long long in_elems = (long long)n * h * w * cin, out_elems = (long long)n * a.Ho * a.Wo * cout;
    const long long quads = (long long)n * a.Ho * ((a.Wo + kPx - 1) / kPx);
    if (in_elems >= CONTROL_MAX_HALFS || out_elems >= CONTROL_MAX_HALFS || quads >= CONTROL_MAX_HALFS) return LD_ERR_SHAPE;
    a.quads = (I)quads;
    const dim3 grid((unsigned)((quads + kBlock - 1) / kBlock), (unsigned)(cout / kCo));
    if (x != nullptr) hipLaunchKernelGGL(hint_conv_kernel<false>, grid, dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL(hint_conv_kernel<true>, grid, dim3(kBlock), 0, stream, a);
    return launched();
}
