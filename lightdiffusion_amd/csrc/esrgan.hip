// ESRGAN (RRDBNet, LD.py:6839-7234) on the device: the dense-block 3x3 convolution kernel, the 3-channel end convolutions, the
// tiled_scale blend (LD.py:7282-7353), and the ld_esrgan executor of the C ABI.
#include "halo_conv.h"
#include "runtime.h"
#include "../../include/ld_mi355x.h"

namespace {

// esrgan_conv_kernel: halo_conv_tile (halo_conv.h) with RRDBNet's epilogue: v = acc + bias; LeakyReLU(slope) unless slope == 0; v = s1 v + R1; v = s2 v + R2.
struct EsrganEpilogue {
    static __device__ __forceinline__ float apply(const EsrganConvArgs& p, float v, float r1, float r2) {
        if (p.slope != 0.f) v = v > 0.f ? v : p.slope * v;
        if (p.r1 != nullptr) v = p.s1 * v + r1;
        if (p.r2 != nullptr) v = p.s2 * v + r2;
        return v;
    }
};

template <int COUT, bool UP>
__global__ __launch_bounds__(512, 1) void esrgan_conv_kernel(const EsrganConvArgs p) {
    halo_conv_tile<COUT, UP, EsrganEpilogue>(p);
}

// ---- conv_first (LD.py:7092-7099): 3x3 pad-1 convolution of the fp32 NHWC image [n][h][w][3], rounded to fp16 once, to 64 channels; no
// activation.  One thread per (pixel, 8 output channels); the 64 x 27 weights sit in LDS.  Written to y (pitch ldy) and, optionally, y2.
__global__ __launch_bounds__(256) void esrgan_first_kernel(const float* x, const half_t* wt, const half_t* bias, half_t* y, int ldy, half_t* y2, int ldy2,
                                                           int n, int h, int w) {
    __shared__ float ws[64 * 27];
    for (int i = threadIdx.x; i < 64 * 27; i += 256) ws[i] = (float)wt[i];
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
            const float* src = x + (pix + (long long)(ky - 1) * w + (kx - 1)) * 3;
            const float a0 = (float)(half_t)src[0], a1 = (float)(half_t)src[1], a2 = (float)(half_t)src[2];
            const float* wp = ws + (cg * 8) * 27 + (ky * 3 + kx) * 3;
#pragma unroll
            for (int o = 0; o < 8; ++o) v[o] += a0 * wp[o * 27] + a1 * wp[o * 27 + 1] + a2 * wp[o * 27 + 2];
        }
    const uint4 packed = pack8(v);
    st16(y + pix * ldy + cg * 8, packed);
    if (y2 != nullptr) st16(y2 + pix * ldy2 + cg * 8, packed);
}

// ---- conv_last (LD.py:7141-7149): 3x3 pad-1 convolution of the first 64 channels of an NHWC fp16 buffer (pitch ldx) to 3 channels, fp32
// NHWC out, unclamped.  One thread per pixel; packed fp16 dot products with fp32 accumulation (v_dot2_f32_f16).
__global__ __launch_bounds__(256) void esrgan_last_kernel(const half_t* x, int ldx, const half_t* wt, const half_t* bias, float* out, int n, int h, int w) {
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
            const half_t* src = x + (pix + (long long)(ky - 1) * w + (kx - 1)) * ldx;
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
    out[pix * 3] = v[0];
    out[pix * 3 + 1] = v[1];
    out[pix * 3 + 2] = v[2];
}

// ---- tiled_scale's accumulation (LD.py:7326-7350) for one tile: out[y0 + y][x0 + x][:] += ps[y][x][:] * my[y] * mx[x], div[y0 + y][x0 + x] += my[y] * mx[x]
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* ps, const float* my, const float* mx, int th, int tw, float* out, float* div, int ow,
                                                         int y0, int x0, int c) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)th * tw) return;
    const int y = (int)(q / tw), x = (int)(q - (long long)y * tw);
    const float m = my[y] * mx[x];
    const long long o = (long long)(y0 + y) * ow + x0 + x;
    for (int k = 0; k < c; ++k) out[o * c + k] += ps[q * c + k] * m;
    div[o] += m;
}
// ... and its final out / out_div (LD.py:7352)
__global__ __launch_bounds__(256) void tile_divide_kernel(float* out, const float* div, long long npix, int c) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= npix) return;
    const float d = div[q];
    for (int k = 0; k < c; ++k) out[q * c + k] = out[q * c + k] / d;
}

thread_local const char* t_last_esrgan_kernel = "";

inline bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const char *pa = (const char*)a, *pb = (const char*)b;
    return pa < pb + bbytes && pb < pa + abytes;
}

}  // namespace

const char* esrgan_last_kernel_name() { return t_last_esrgan_kernel; }

int esrgan_first_launch(const float* x, const half_t* wt, const half_t* bias, half_t* y, int ldy, half_t* y2, int ldy2, int n, int h, int w, hipStream_t stream) {
    if (x == nullptr || wt == nullptr || bias == nullptr || y == nullptr) return LD_ERR_ARG;
    if (n < 1 || h < 1 || w < 1) return LD_ERR_SHAPE;
    if (ldy < 64 || (ldy & 7) || (y2 != nullptr && (ldy2 < 64 || (ldy2 & 7)))) return LD_ERR_SHAPE;
    unsigned blocks = 0;
    if (!end_conv_grid(n, h, w, 8, &blocks)) return LD_ERR_SHAPE;
    hipLaunchKernelGGL(esrgan_first_kernel, dim3(blocks), dim3(256), 0, stream, x, wt, bias, y, ldy, y2, ldy2, n, h, w);
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}

int esrgan_last_launch(const half_t* x, int ldx, const half_t* wt, const half_t* bias, float* out, int n, int h, int w, hipStream_t stream) {
    if (x == nullptr || wt == nullptr || bias == nullptr || out == nullptr) return LD_ERR_ARG;
    if (n < 1 || h < 1 || w < 1) return LD_ERR_SHAPE;
    if (ldx < 64 || (ldx & 7)) return LD_ERR_SHAPE;
    unsigned blocks = 0;
    if (!end_conv_grid(n, h, w, 1, &blocks)) return LD_ERR_SHAPE;
    hipLaunchKernelGGL(esrgan_last_kernel, dim3(blocks), dim3(256), 0, stream, x, ldx, wt, bias, out, n, h, w);
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}

int esrgan_conv_launch(const EsrganConvArgs& a, hipStream_t stream) {
    t_last_esrgan_kernel = "";
    if (a.x == nullptr || a.wt == nullptr || a.y == nullptr) return LD_ERR_ARG;
    if (a.n < 1 || a.h < 1 || a.w < 1) return LD_ERR_SHAPE;
    if (a.cin < 64 || a.cin > 192 || (a.cin & 31) || (a.cout != 32 && a.cout != 64)) return LD_ERR_SHAPE;
    if (a.ldx < a.cin || (a.ldx & 7) || (a.ldy & 7) || (a.c_off & 7) || a.c_off < 0 || a.c_off + a.cout > a.ldy) return LD_ERR_SHAPE;
    if (a.up && ((a.h | a.w) & 1)) return LD_ERR_SHAPE;
    if ((a.r1 != nullptr && (a.ldr1 < a.cout || (a.ldr1 & 7))) || (a.r2 != nullptr && (a.ldr2 < a.cout || (a.ldr2 & 7)))) return LD_ERR_SHAPE;
    if (a.y2 != nullptr && (a.ldy2 < a.cout || (a.ldy2 & 7))) return LD_ERR_SHAPE;
    const long long npix = (long long)a.n * a.h * a.w, nsrc = a.up ? npix / 4 : npix;
    const long long tiles = (long long)a.n * ((a.h + EG_TH - 1) / EG_TH) * ((a.w + EG_TW - 1) / EG_TW);
    if (tiles > 0x7fffffffLL) return LD_ERR_SHAPE;
    // an output that shares memory with the input: only as the dense blocks use it — the same buffer, channels behind the ones read
    const size_t xbytes = (size_t)nsrc * a.ldx * sizeof(half_t);
    if (ranges_overlap(a.x, xbytes, a.y, (size_t)npix * a.ldy * sizeof(half_t)) && !(a.y == a.x && a.ldy == a.ldx && !a.up && a.c_off >= a.cin)) return LD_ERR_ARG;
    if (a.y2 != nullptr && ranges_overlap(a.x, xbytes, a.y2, (size_t)npix * a.ldy2 * sizeof(half_t))) return LD_ERR_ARG;
    const dim3 grid((unsigned)tiles), block(512);
    if (a.cout == 32) {
        if (a.up) { hipLaunchKernelGGL((esrgan_conv_kernel<32, true>), grid, block, 0, stream, a); t_last_esrgan_kernel = "esrgan_conv_kernel<32,up>"; }
        else { hipLaunchKernelGGL((esrgan_conv_kernel<32, false>), grid, block, 0, stream, a); t_last_esrgan_kernel = "esrgan_conv_kernel<32>"; }
    } else {
        if (a.up) { hipLaunchKernelGGL((esrgan_conv_kernel<64, true>), grid, block, 0, stream, a); t_last_esrgan_kernel = "esrgan_conv_kernel<64,up>"; }
        else { hipLaunchKernelGGL((esrgan_conv_kernel<64, false>), grid, block, 0, stream, a); t_last_esrgan_kernel = "esrgan_conv_kernel<64>"; }
    }
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}

int tile_blend_launch(const float* ps, const float* my, const float* mx, int th, int tw, float* out, float* div, int oh, int ow, int y0, int x0, int c,
                      hipStream_t stream) {
    if (out == nullptr || div == nullptr || oh < 1 || ow < 1 || c < 1) return LD_ERR_ARG;
    if (ps == nullptr) {   // the final divide
        const long long npix = (long long)oh * ow;
        hipLaunchKernelGGL(tile_divide_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, out, div, npix, c);
        return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
    }
    if (my == nullptr || mx == nullptr || th < 1 || tw < 1) return LD_ERR_ARG;
    if (y0 < 0 || x0 < 0 || y0 + th > oh || x0 + tw > ow) return LD_ERR_SHAPE;
    const long long q = (long long)th * tw;
    hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, stream, ps, my, mx, th, tw, out, div, ow, y0, x0, c);
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}

// =====================================================================================================================
// ld_esrgan: RRDBNet (old-arch parameter names, LD.py:7044-7055 / 7174-7192) on the kernels above.
// Workspace: two dense buffers of pitch nf + 4 gc = 192 (a block's convolutions 1-4 append their 32 channels in place, convolution 5
// writes the next block's first 64 channels into the other buffer), the RRDB input (the outer residual), the trunk input (the
// ShortcutBlock's residual), one 64-channel stage per up-convolution and one for the HR convolution.
// =====================================================================================================================
struct ld_esrgan : Model {
    ld_esrgan_config cfg;
    int first_w = -1, first_b = -1, trunk_w = -1, trunk_b = -1, hr_w = -1, hr_b = -1, last_w = -1, last_b = -1;
    std::vector<int> rdb_w, rdb_b;   // [(block * 3 + rdb) * 5 + conv]
    std::vector<int> up_w, up_b;
    int n_up = 0;
};

namespace {

int esrgan_build(ld_esrgan* e) {
    const ld_esrgan_config& c = e->cfg;
    if (c.in_nc != 3 || c.out_nc != 3 || c.nf != 64 || c.gc != 32 || c.nb < 1 || c.nb > 64) return LD_ERR_SHAPE;
    int n_up = 0;
    while ((1 << n_up) < c.scale) ++n_up;
    if ((1 << n_up) != c.scale || n_up > 3) return LD_ERR_SHAPE;
    e->n_up = n_up;
    ParamTable& pt = e->pt;
    auto conv = [&](const std::string& base, int o, int i, int& w, int& b) {
        w = pt.add(base + ".weight", PK_CONV3, {o, i, 3, 3});
        b = pt.add(base + ".bias", PK_VEC, {o});
    };
    conv("model.0", c.nf, c.in_nc, e->first_w, e->first_b);
    e->rdb_w.resize((size_t)c.nb * 15);
    e->rdb_b.resize((size_t)c.nb * 15);
    for (int b = 0; b < c.nb; ++b)
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 5; ++k) {
                const std::string base = "model.1.sub." + std::to_string(b) + ".RDB" + std::to_string(r + 1) + ".conv" + std::to_string(k + 1) + ".0";
                conv(base, k < 4 ? c.gc : c.nf, c.nf + k * c.gc, e->rdb_w[(b * 3 + r) * 5 + k], e->rdb_b[(b * 3 + r) * 5 + k]);
            }
    conv("model.1.sub." + std::to_string(c.nb), c.nf, c.nf, e->trunk_w, e->trunk_b);
    e->up_w.resize(n_up);
    e->up_b.resize(n_up);
    for (int u = 0; u < n_up; ++u) conv("model." + std::to_string(3 * (u + 1)), c.nf, c.nf, e->up_w[u], e->up_b[u]);
    conv("model." + std::to_string(3 * n_up + 2), c.nf, c.nf, e->hr_w, e->hr_b);
    conv("model." + std::to_string(3 * n_up + 4), c.out_nc, c.nf, e->last_w, e->last_b);
    return pt.finalize();
}

int esrgan_run(ld_esrgan* e, bool dry, const float* x, float* out, int b, int h, int w, hipStream_t stream, size_t* dry_peak = nullptr) {
    const ld_esrgan_config& c = e->cfg;
    if ((long long)b * h * w * c.scale * c.scale > 0x7fffffffLL) return LD_ERR_SHAPE;
    Arena plan;
    Exec ex = e->begin(dry, stream, plan);
    Arena& ar = *ex.arena;
    const ParamTable& pt = e->pt;
    const int nf = c.nf, gc = c.gc, ldd = nf + 4 * gc;
    const size_t npix = (size_t)b * h * w;
    half_t* dense[2] = {ar.halfs(npix * ldd), ar.halfs(npix * ldd)};
    half_t* rrdb_in = ar.halfs(npix * nf);
    half_t* trunk_in = ar.halfs(npix * nf);

    auto conv = [&](EsrganConvArgs a, int wslot, int bslot) {
        a.wt = pt.ptr(wslot);
        a.bias = pt.ptr(bslot);
        a.n = b;
        ex.launch(KC_CONV3, 2.0 * a.n * a.h * (double)a.w * a.cout * 9.0 * a.cin, a.up ? "upconv3" : "dense3", (long long)a.n * a.h * a.w, a.cout, 9 * a.cin, 1,
                  esrgan_last_kernel_name, [&] { return esrgan_conv_launch(a, stream); });
    };

    // conv_first: the trunk's input, and the first RRDB's (dense buffer 0 and the outer-residual copy)
    ex.launch(KC_MISC, 2.0 * npix * nf * 27, "conv_first", (long long)npix, nf, 27, 1, "esrgan_first_kernel", [&] {
        return esrgan_first_launch(x, pt.ptr(e->first_w), pt.ptr(e->first_b), dense[0], ldd, trunk_in, nf, b, h, w, stream);
    });
    if (!dry && ex.status == LD_OK)
        ex.note(hipMemcpyAsync(rrdb_in, trunk_in, npix * nf * sizeof(half_t), hipMemcpyDeviceToDevice, stream) == hipSuccess ? LD_OK : LD_ERR_HIP);
    int cur = 0;
    for (int blk = 0; blk < c.nb; ++blk)
        for (int r = 0; r < 3; ++r) {
            half_t* d = dense[cur];
            for (int k = 0; k < 5; ++k) {
                EsrganConvArgs a;
                a.x = d; a.ldx = ldd; a.cin = nf + k * gc; a.h = h; a.w = w;
                if (k < 4) {               // LeakyReLU(0.2), appended in place
                    a.y = d; a.ldy = ldd; a.c_off = a.cin; a.cout = gc; a.slope = 0.2f;
                } else {                   // x5 * 0.2 + x (LD.py:6992); the RRDB's third block also carries out * 0.2 + x (LD.py:6902)
                    a.y = dense[cur ^ 1]; a.ldy = ldd; a.c_off = 0; a.cout = nf;
                    a.r1 = d; a.ldr1 = ldd; a.s1 = 0.2f;
                    if (r == 2) { a.r2 = rrdb_in; a.ldr2 = nf; a.s2 = 0.2f; a.y2 = rrdb_in; a.ldy2 = nf; }
                }
                conv(a, e->rdb_w[(blk * 3 + r) * 5 + k], e->rdb_b[(blk * 3 + r) * 5 + k]);
            }
            cur ^= 1;
        }
    half_t* f = dense[cur ^ 1];
    int ldf = ldd;
    {   // trunk convolution + the ShortcutBlock add (LD.py:6787-6789)
        EsrganConvArgs a;
        a.x = dense[cur]; a.ldx = ldd; a.cin = nf; a.h = h; a.w = w;
        a.y = f; a.ldy = ldf; a.c_off = 0; a.cout = nf;
        a.r1 = trunk_in; a.ldr1 = nf; a.s1 = 1.0f;
        conv(a, e->trunk_w, e->trunk_b);
    }
    int H = h, W = w;
    for (int u = 0; u < e->n_up; ++u) {   // nearest 2x + convolution + LeakyReLU(0.2)
        H *= 2; W *= 2;
        half_t* g = ar.halfs((size_t)b * H * W * nf);
        EsrganConvArgs a;
        a.x = f; a.ldx = ldf; a.cin = nf; a.h = H; a.w = W; a.up = 1;
        a.y = g; a.ldy = nf; a.c_off = 0; a.cout = nf; a.slope = 0.2f;
        conv(a, e->up_w[u], e->up_b[u]);
        f = g; ldf = nf;
    }
    half_t* hr = ar.halfs((size_t)b * H * W * nf);
    {
        EsrganConvArgs a;
        a.x = f; a.ldx = ldf; a.cin = nf; a.h = H; a.w = W;
        a.y = hr; a.ldy = nf; a.c_off = 0; a.cout = nf; a.slope = 0.2f;
        conv(a, e->hr_w, e->hr_b);
    }
    const long long opix = (long long)b * H * W;
    ex.launch(KC_MISC, 2.0 * opix * c.out_nc * (9 * nf), "conv_last", opix, c.out_nc, 9 * nf, 1, "esrgan_last_kernel", [&] {
        return esrgan_last_launch(hr, nf, pt.ptr(e->last_w), pt.ptr(e->last_b), out, b, H, W, stream);
    });
    return e->end(ex, dry_peak, !dry);
}

}  // namespace

extern "C" {

int ld_esrgan_create(const ld_esrgan_config* cfg, ld_esrgan** out) {
    if (cfg == nullptr || out == nullptr) return LD_ERR_ARG;
    ld_esrgan* e = new ld_esrgan();
    e->cfg = *cfg;
    const int st = esrgan_build(e);
    if (st != LD_OK) {
        ld_esrgan_destroy(e);
        return st;
    }
    *out = e;
    return LD_OK;
}

void ld_esrgan_destroy(ld_esrgan* e) {
    if (e == nullptr) return;
    e->destroy_common();
    delete e;
}

int ld_esrgan_param_count(const ld_esrgan* e) { return abi_param_count(e); }
int ld_esrgan_param_info(const ld_esrgan* e, int i, const char** name, int* ndim, int64_t shape[4]) { return abi_param_info(e, i, name, ndim, shape); }
int ld_esrgan_load_param(ld_esrgan* e, const char* name, const void* src, int dtype, void* stream) { return abi_load_param(e, name, src, dtype, stream); }
size_t ld_esrgan_workspace_bytes(const ld_esrgan* e) { return abi_workspace_bytes(e); }
int ld_esrgan_last_launches(const ld_esrgan* e) { return abi_last_launches(e); }
double ld_esrgan_last_flops(const ld_esrgan* e) { return abi_last_flops(e); }
int ld_esrgan_profile_launches(const ld_esrgan* e, char* buf, size_t buf_bytes) { return abi_profile_launches(e, buf, buf_bytes); }

size_t ld_esrgan_plan_bytes(ld_esrgan* e, int b, int h, int w) {
    return abi_plan_bytes(e, b, h, w, [&](size_t* peak) { return esrgan_run(e, true, nullptr, nullptr, b, h, w, nullptr, peak); });
}

int ld_esrgan_reserve(ld_esrgan* e, int max_b, int max_h, int max_w) {
    if (e == nullptr || max_b < 1 || max_h < 1 || max_w < 1) return LD_ERR_ARG;
    const size_t bytes = ld_esrgan_plan_bytes(e, max_b, max_h, max_w);   // (planned before the old workspace goes)
    if (bytes == 0) return LD_ERR_SHAPE;
    return e->set_workspace(bytes, bytes - 4096);
}

int ld_esrgan_forward(ld_esrgan* e, const float* x, float* out, int b, int h, int w, void* stream) {
    if (e == nullptr || x == nullptr || out == nullptr) return LD_ERR_ARG;
    return abi_checked_run(*e, true, b >= 1 && h >= 1 && w >= 1,
                           [&](size_t* peak) { return esrgan_run(e, true, nullptr, nullptr, b, h, w, nullptr, peak); },
                           [&] { return esrgan_run(e, false, x, out, b, h, w, (hipStream_t)stream); });
}

int ld_esrgan_profile(ld_esrgan* e, const float* x, float* out, int b, int h, int w, void* stream) {
    return abi_profile(e, stream, [&] { return ld_esrgan_forward(e, x, out, b, h, w, stream); });
}

}  // extern "C"
