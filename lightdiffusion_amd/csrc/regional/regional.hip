// Regional conditioning (sampling.sampling_function with "ld_cond_areas"; upstream ComfyUI's get_area_and_mult + calc_cond_batch, of which the
// reference keeps the skeleton with area = the full latent and strength = 1.0, LD.py:2435-2458, 2492-2591), on fp32 NCHW latents [B][C][H][W]:
//   gather    out[(j * B + b), c, y, x] = x[b, c, y0_j + y, x0_j + x] for the k windows of one group, all of one h x w: a group's UNet input in one
//             launch (k whole-latent windows: the latent replicated k times)
//   combine   per output element and per list (0: cond, 1: uncond)  num = 0, den = 1e-37f;  for every entry of the list that covers the pixel, in
//             table order:  mult = (mask ? mask[b % Bm, Y, X] * mask_strength : 1) * strength;  without a mask, for the edges top, bottom, left,
//             right of the area that are not edges of the latent, t < 8 rows / columns from the edge: mult = mult * (0.125f * (t + 1));
//             num += out * mult;  den += mult.   pred = num / den (IEEE);   result = u + (c - u) * scale.
// Every fp32 operation is rounded on its own, in the order written.  This unit is compiled with -ffp-contract=off (Makefile), as inpaint/inpaint.hip
// is and for its reason: the products that feed the sums must not become FMAs, the tests hold both kernels to the bits of the expression evaluated
// operation by operation.  The window and entry descriptors travel BY VALUE in the kernel arguments (at most 16, a plain struct): no table in device
// memory, nothing to upload, so a launch allocates nothing, reads nothing on the host and synchronises nothing, and is capturable.  Both kernels
// are grid-stride loops of 256-lane blocks on a capped grid, consecutive lanes on consecutive elements of the OUTPUT; a lane handles four floats
// of one row as a float4 where W and every window's x0 and w are multiples of 4 and every pointer is 16-byte aligned (four such floats then lie
// in one window or outside it together), one float otherwise — the same bits either way.  Indices are 32-bit: a tensor of 2^31 floats or more
// is refused.
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

struct WindowTable {
    int y0[REGIONAL_MAX_ENTRIES], x0[REGIONAL_MAX_ENTRIES];
};
struct EntryTable {
    RegionalEntry e[REGIONAL_MAX_ENTRIES];
};

// One work item = V consecutive floats of one output row.  The grid-stride increment, at most 2^20, added to an index below 2^31 cannot wrap.
using I = unsigned;
template <int V>
__global__ __launch_bounds__(kBlock) void regional_gather_kernel(const float* __restrict__ x, float* __restrict__ out, const WindowTable tab, I planes, I H,
                                                                 I W, I h, I wq, I total) {
    for (I i = (I)blockIdx.x * kBlock + threadIdx.x; i < total; i += (I)gridDim.x * kBlock) {
        const I row = i / wq, xq = i - row * wq;                 // row of the output: ((j * planes + plane) * h + y)
        const I t = row / h, y = row - t * h;
        const I j = t / planes, plane = t - j * planes;
        const I src = (plane * H + (I)tab.y0[j] + y) * W + (I)tab.x0[j] + xq * V;
        store<V>(out + i * V, load<V>(x + src));
    }
}

// The ramp of one edge: t rows / columns from it (t >= 0), eight of them: 0.125f * (t + 1), exact in fp32.
__device__ __forceinline__ float feather(float mult, int t) { return t < 8 ? __fmul_rn(mult, __fmul_rn(0.125f, (float)(t + 1))) : mult; }

template <int V>
__global__ __launch_bounds__(kBlock) void regional_combine_kernel(const EntryTable tab, int n, float scale, float* __restrict__ result, I C, I H, I W, I wq,
                                                                  I total) {
    for (I i = (I)blockIdx.x * kBlock + threadIdx.x; i < total; i += (I)gridDim.x * kBlock) {
        const I row = i / wq, X = (i - row * wq) * V;            // row of the result: (b * C + c) * H + Y
        const I plane = row / H, Y = row - plane * H;
        const I b = plane / C;
        float num[2][V], den[2][V];
#pragma unroll
        for (int t = 0; t < V; ++t) {
            num[0][t] = num[1][t] = 0.0f;
            den[0][t] = den[1][t] = 1e-37f;
        }
        for (int k = 0; k < n; ++k) {
            const RegionalEntry& e = tab.e[k];
            const int ly = (int)Y - e.y0, lx = (int)X - e.x0;
            // V == 4: x0 and w are multiples of 4, so the four floats are covered together
            if (ly < 0 || ly >= e.h || lx < 0 || lx >= e.w) continue;
            const Quad o = load<V>(e.out + (plane * (I)e.h + (I)ly) * (I)e.w + (I)lx);
            Quad m;
            if (e.mask != nullptr) {
                m = load<V>(e.mask + ((e.mask_batch == 1 ? 0u : b) * H + Y) * W + X);
#pragma unroll
                for (int t = 0; t < V; ++t) m.v[t] = __fmul_rn(__fmul_rn(m.v[t], e.mask_strength), e.strength);
            } else {
                float rows = __fmul_rn(1.0f, e.strength);
                if (e.y0 != 0) rows = feather(rows, ly);
                if (e.y0 + e.h < (int)H) rows = feather(rows, e.h - 1 - ly);
                const bool left = e.x0 != 0, right = e.x0 + e.w < (int)W;
#pragma unroll
                for (int t = 0; t < V; ++t) {
                    float mult = rows;
                    if (left) mult = feather(mult, lx + t);
                    if (right) mult = feather(mult, e.w - 1 - (lx + t));
                    m.v[t] = mult;
                }
            }
            const int l = e.list != 0;
#pragma unroll
            for (int t = 0; t < V; ++t) {
                const float term = __fmul_rn(o.v[t], m.v[t]);
                if (l) {
                    num[1][t] = __fadd_rn(num[1][t], term);
                    den[1][t] = __fadd_rn(den[1][t], m.v[t]);
                } else {
                    num[0][t] = __fadd_rn(num[0][t], term);
                    den[0][t] = __fadd_rn(den[0][t], m.v[t]);
                }
            }
        }
        Quad r;
#pragma unroll
        for (int t = 0; t < V; ++t) {
            const float c = __fdiv_rn(num[0][t], den[0][t]), u = __fdiv_rn(num[1][t], den[1][t]);
            r.v[t] = __fadd_rn(u, __fmul_rn(__fsub_rn(c, u), scale));
        }
        store<V>(result + i * V, r);
    }
}

inline int launched() { return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

int regional_gather_launch(const float* x, float* out, int B, int C, int H, int W, int h, int w, const RegionalWindow* windows, int k, hipStream_t stream) {
    if (x == nullptr || out == nullptr || windows == nullptr) return LD_ERR_ARG;
    if (B < 1 || C < 1 || H < 1 || W < 1 || h < 1 || w < 1 || h > H || w > W || k < 1 || k > REGIONAL_MAX_ENTRIES) return LD_ERR_SHAPE;
    const long long planes = (long long)B * C;
    if (planes * H * W >= REGIONAL_MAX_FLOATS || planes * h * w * k >= REGIONAL_MAX_FLOATS) return LD_ERR_SHAPE;
    WindowTable tab = {};
    bool vec = W % 4 == 0 && w % 4 == 0 && aligned16(x) && aligned16(out);
    for (int j = 0; j < k; ++j) {
        const RegionalWindow& r = windows[j];
        if (r.y0 < 0 || r.x0 < 0 || r.y0 > H - h || r.x0 > W - w) return LD_ERR_SHAPE;      // a window stays inside the latent
        tab.y0[j] = r.y0;
        tab.x0[j] = r.x0;
        vec = vec && r.x0 % 4 == 0;
    }
    if (vec) {
        const long long total = planes * k * h * (w / 4);
        hipLaunchKernelGGL(regional_gather_kernel<4>, dim3(grid_of(total)), dim3(kBlock), 0, stream, x, out, tab, (I)planes, (I)H, (I)W, (I)h, (I)(w / 4),
                           (I)total);
    } else {
        const long long total = planes * k * h * w;
        hipLaunchKernelGGL(regional_gather_kernel<1>, dim3(grid_of(total)), dim3(kBlock), 0, stream, x, out, tab, (I)planes, (I)H, (I)W, (I)h, (I)w, (I)total);
    }
    return launched();
}

int regional_combine_launch(const RegionalEntry* entries, int n, float cond_scale, float* result, int B, int C, int H, int W, hipStream_t stream) {
    if (entries == nullptr || result == nullptr) return LD_ERR_ARG;
    if (B < 1 || C < 1 || H < 1 || W < 1 || n < 1 || n > REGIONAL_MAX_ENTRIES) return LD_ERR_SHAPE;      // (before the table is read: it has n rows)
    for (int k = 0; k < n; ++k)
        if (entries[k].out == nullptr) return LD_ERR_ARG;
    const long long planes = (long long)B * C;
    if (planes * H * W >= REGIONAL_MAX_FLOATS) return LD_ERR_SHAPE;
    EntryTable tab = {};
    bool vec = W % 4 == 0 && aligned16(result);
    for (int k = 0; k < n; ++k) {
        const RegionalEntry& e = entries[k];
        if (e.h < 1 || e.w < 1 || e.y0 < 0 || e.x0 < 0 || e.h > H || e.w > W || e.y0 > H - e.h || e.x0 > W - e.w) return LD_ERR_SHAPE;   // an area stays inside the latent
        if ((e.list != 0 && e.list != 1) || (e.mask != nullptr && e.mask_batch != 1 && e.mask_batch != B)) return LD_ERR_SHAPE;
        tab.e[k] = e;
        vec = vec && e.x0 % 4 == 0 && e.w % 4 == 0 && aligned16(e.out) && (e.mask == nullptr || aligned16(e.mask));
    }
    if (vec) {
        const long long total = planes * H * (W / 4);
        hipLaunchKernelGGL(regional_combine_kernel<4>, dim3(grid_of(total)), dim3(kBlock), 0, stream, tab, n, cond_scale, result, (I)C, (I)H, (I)W, (I)(W / 4),
                           (I)total);
    } else {
        const long long total = planes * H * W;
        hipLaunchKernelGGL(regional_combine_kernel<1>, dim3(grid_of(total)), dim3(kBlock), 0, stream, tab, n, cond_scale, result, (I)C, (I)H, (I)W, (I)W, (I)total);
    }
    return launched();
}
