// The two fp32 blends a masked sampler step makes around the model call (sampling.KSamplerX0Inpaint; upstream ComfyUI's KSamplerX0Inpaint, of which
// the reference's class, LD.py:2629-2636, keeps the signature and drops the mask), on NCHW latents [B][C][HW]:
//   in    out = x * m + (noise * sigma[b] + latent) * (1 - m)        noise * sigma + latent is EPS.noise_scaling, max_denoise = False (LD.py:1267-1274)
//   out   den = den * m + latent * (1 - m), in place
// Six and four fp32 operations, each rounded on its own, in the order written: x * m, noise * sigma, + latent, 1 - m, the product, the sum (den * m,
// 1 - m, latent * that, the sum).  This unit is compiled with -ffp-contract=off (Makefile), as detail/detail_image.hip is and for its reason: __fmul_rn
// and its kin are plain operators in the HIP headers, and a product that feeds a sum would otherwise be contracted into one FMA — the result would
// no longer be the bits of the expression evaluated operation by operation, which is what the tests hold these kernels to.
// The mask is [Bm][Cm][HW] with Bm in {1, B} and Cm in {1, C}: a sample's or a channel's plane is found by index, nothing is materialised.  sigma is
// read from device memory, one value per sample, so one captured launch serves every step.  Both kernels are grid-stride loops of 256-lane blocks on
// a capped grid whose consecutive lanes touch consecutive elements; a lane handles four floats of one plane as a float4 where HW is a multiple of 4
// and every pointer is 16-byte aligned (then every plane is), one float otherwise.  No allocation, no host read, no synchronisation.
#include <cstdint>

#include "../kernels.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 4096;
inline int grid_of(long long n) {
    long long b = (n + kBlock - 1) / kBlock;
    return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

struct Quad {
    float v[4];
};
template <int V>
__device__ __forceinline__ Quad load(const float* p) {
    Quad q;
    if (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        q.v[0] = t.x; q.v[1] = t.y; q.v[2] = t.z; q.v[3] = t.w;
    } else {
        q.v[0] = *p;
    }
    return q;
}
template <int V>
__device__ __forceinline__ void store(float* p, const Quad& q) {
    if (V == 4) *reinterpret_cast<float4*>(p) = make_float4(q.v[0], q.v[1], q.v[2], q.v[3]);
    else *p = q.v[0];
}

// One work item = V consecutive floats of one plane.  `per`: items per plane (HW / V).  x and out may be the same buffer (an item reads what it
// writes before it writes it), so neither is __restrict__.  Indices are 32-bit (the two divisions per item would be long software sequences in 64
// bits): the launch refuses a tensor of 2^31 floats or more, and the grid-stride increment, at most 2^20, added to an index below 2^31 cannot wrap.
using I = unsigned;
template <int V>
__global__ __launch_bounds__(kBlock) void inpaint_blend_in_kernel(const float* x, const float* __restrict__ mask, const float* __restrict__ latent,
                                                                  const float* __restrict__ noise, const float* __restrict__ sigma, float* out, I C, I HW,
                                                                  I per, I total, int bm_all, int cm_all) {
    for (I i = (I)blockIdx.x * kBlock + threadIdx.x; i < total; i += (I)gridDim.x * kBlock) {
        const I plane = i / per, e = (i - plane * per) * V;
        const I b = plane / C, c = plane - b * C;
        const I off = plane * HW + e;
        const I moff = ((bm_all ? b : 0) * (cm_all ? C : 1) + (cm_all ? c : 0)) * HW + e;
        const float s = sigma[b];
        const Quad xv = load<V>(x + off), mv = load<V>(mask + moff), lv = load<V>(latent + off), nv = load<V>(noise + off);
        Quad o;
#pragma unroll
        for (int t = 0; t < V; ++t) {
            const float keep = __fmul_rn(xv.v[t], mv.v[t]);
            const float noised = __fadd_rn(__fmul_rn(nv.v[t], s), lv.v[t]);
            o.v[t] = __fadd_rn(keep, __fmul_rn(noised, __fsub_rn(1.0f, mv.v[t])));
        }
        store<V>(out + off, o);
    }
}

template <int V>
__global__ __launch_bounds__(kBlock) void inpaint_blend_out_kernel(float* __restrict__ den, const float* __restrict__ mask, const float* __restrict__ latent,
                                                                   I C, I HW, I per, I total, int bm_all, int cm_all) {
    for (I i = (I)blockIdx.x * kBlock + threadIdx.x; i < total; i += (I)gridDim.x * kBlock) {
        const I plane = i / per, e = (i - plane * per) * V;
        const I b = plane / C, c = plane - b * C;
        const I off = plane * HW + e;
        const I moff = ((bm_all ? b : 0) * (cm_all ? C : 1) + (cm_all ? c : 0)) * HW + e;
        const Quad dv = load<V>(den + off), mv = load<V>(mask + moff), lv = load<V>(latent + off);
        Quad o;
#pragma unroll
        for (int t = 0; t < V; ++t)
            o.v[t] = __fadd_rn(__fmul_rn(dv.v[t], mv.v[t]), __fmul_rn(lv.v[t], __fsub_rn(1.0f, mv.v[t])));
        store<V>(den + off, o);
    }
}

inline int launched() { return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool shape_ok(int B, int C, long long HW, int Bm, int Cm) {
    return B > 0 && C > 0 && HW > 0 && (Bm == 1 || Bm == B) && (Cm == 1 || Cm == C) && (long long)B * C * HW < INPAINT_MAX_FLOATS;
}
}  // namespace

int inpaint_blend_in_launch(const float* x, const float* mask, const float* latent, const float* noise, const float* sigma, float* out, int B, int C,
                            long long HW, int Bm, int Cm, hipStream_t stream) {
    if (x == nullptr || mask == nullptr || latent == nullptr || noise == nullptr || sigma == nullptr || out == nullptr) return LD_ERR_ARG;
    if (!shape_ok(B, C, HW, Bm, Cm)) return LD_ERR_SHAPE;
    const long long planes = (long long)B * C;
    const int bm_all = Bm == B && B > 1, cm_all = Cm == C && C > 1;
    if (HW % 4 == 0 && aligned16(x) && aligned16(mask) && aligned16(latent) && aligned16(noise) && aligned16(out)) {
        const long long per = HW / 4, total = planes * per;
        hipLaunchKernelGGL(inpaint_blend_in_kernel<4>, dim3(grid_of(total)), dim3(kBlock), 0, stream, x, mask, latent, noise, sigma, out, (I)C, (I)HW, (I)per,
                           (I)total, bm_all, cm_all);
    } else {
        const long long total = planes * HW;
        hipLaunchKernelGGL(inpaint_blend_in_kernel<1>, dim3(grid_of(total)), dim3(kBlock), 0, stream, x, mask, latent, noise, sigma, out, (I)C, (I)HW, (I)HW,
                           (I)total, bm_all, cm_all);
    }
    return launched();
}

int inpaint_blend_out_launch(float* den, const float* mask, const float* latent, int B, int C, long long HW, int Bm, int Cm, hipStream_t stream) {
    if (den == nullptr || mask == nullptr || latent == nullptr) return LD_ERR_ARG;
    if (!shape_ok(B, C, HW, Bm, Cm)) return LD_ERR_SHAPE;
    const long long planes = (long long)B * C;
    const int bm_all = Bm == B && B > 1, cm_all = Cm == C && C > 1;
    if (HW % 4 == 0 && aligned16(den) && aligned16(mask) && aligned16(latent)) {
        const long long per = HW / 4, total = planes * per;
        hipLaunchKernelGGL(inpaint_blend_out_kernel<4>, dim3(grid_of(total)), dim3(kBlock), 0, stream, den, mask, latent, (I)C, (I)HW, (I)per, (I)total, bm_all,
                           cm_all);
    } else {
        const long long total = planes * HW;
        hipLaunchKernelGGL(inpaint_blend_out_kernel<1>, dim3(grid_of(total)), dim3(kBlock), 0, stream, den, mask, latent, (I)C, (I)HW, (I)HW, (I)total, bm_all,
                           cm_all);
    }
    return launched();
}
