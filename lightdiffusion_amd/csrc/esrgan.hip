// ESRGAN (RRDBNet, LD.py:6839-7234) on the device: the dense-block 3x3 convolution kernel, the 3-channel end convolutions, the
// tiled_scale blend (LD.py:7282-7353), and the ld_esrgan executor of the C ABI.
#include "gemm_device.h"
#include "runtime.h"
#include "../../include/ld_mi355x.h"

namespace {

// =====================================================================================================================
// esrgan_conv_kernel: stride-1 pad-1 3x3 convolution for the dense blocks: N = 32 / 64 output channels, K = 9 * (64 .. 192), any H x W.
// A workgroup (8 waves) owns a TH x TW = 16 x 32 pixel tile of one image; wave w computes rows 4 (w >> 1) .. + 3, columns 16 (w & 1) .. + 15
// of it for ALL output channels (4 x COUT / 16 MFMA 16x16x32 tiles, operands swapped as in gemm_device.h: a lane ends up with 4 consecutive
// output channels of one pixel).  K runs slab-major (32 channels), tap-minor: per slab the 18 x 34 halo pixels of the tile (64 bytes each)
// and the slab's 9 x COUT weight rows are copied to LDS once by LDS-DMA and the nine taps read their fragments from them.  Halo and
// weights are double-buffered: slab s + 1 is in flight while slab s is multiplied; one counted wait and two barriers per slab.
// The A operand is the first `cin` channels of an NHWC buffer of pitch ldx >= cin; the output goes to channels [c_off, c_off + COUT) of a
// buffer of pitch ldy that may be the SAME buffer (c_off >= cin: the DMA reads only 16-byte chunks below cin, the stores only touch
// channels >= c_off, so no launch-wide ordering is needed).  Pixels outside the image — an image's own top / bottom rows included, never
// its batch neighbour's — come from the zero page; pixels of a ragged tile are masked at the store.
// LDS rows are 64 bytes with the 16-byte chunk XOR-swizzled by (row >> 2) & 3 on the DMA source address and on the fragment read: 16
// consecutive rows at one chunk index cover all 64 banks once, whatever the first row (the tap shift moves it).
// UP: the input is the nearest-2x upsampling of the source (upconv_block, LD.py:6995-7022): halo pixel (y, x) <- source (y >> 1, x >> 1).
// Epilogue on the fp32 accumulators, one rounding at the store: v = acc + bias; LeakyReLU(slope); v = s1 v + R1; v = s2 v + R2.
// =====================================================================================================================
constexpr int EG_TH = 16, EG_TW = 32;
constexpr int EG_HW2 = EG_TW + 2, EG_HP = (EG_TH + 2) * EG_HW2;   // halo row pitch (pixels), halo pixels (612)
constexpr int EG_HPIECES = (EG_HP + 15) / 16;                      // 1 KB pieces of a halo slab (39)
constexpr int EG_NH = (EG_HPIECES + 7) / 8;                        // ... per wave (5; the spare piece copies zeros)
constexpr int EG_HBYTES = EG_NH * 8 * 1024;

template <int COUT, bool UP>
__global__ __launch_bounds__(512, 1) void esrgan_conv_kernel(const EsrganConvArgs p) {
    constexpr int TN = COUT / 16, TM = 4;
    constexpr int BPIECES = 9 * COUT / 16;                          // weight pieces of a slab (16 rows of 64 bytes each)
    constexpr int NBW = (BPIECES + 7) / 8;                          // ... per wave; pieces beyond BPIECES copy zeros into a dump slot
    constexpr int BBYTES = (BPIECES + 1) * 1024;
    __shared__ __attribute__((aligned(16))) char smem[2 * EG_HBYTES + 2 * BBYTES];
    static_assert(2 * EG_HBYTES + 2 * BBYTES <= 163840, "LDS");

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = (p.w + EG_TW - 1) / EG_TW, tiles_y = (p.h + EG_TH - 1) / EG_TH;
    int bid = blockIdx.x;
    const int img = bid / (tiles_x * tiles_y);
    bid -= img * tiles_x * tiles_y;
    const int row0 = (bid / tiles_x) * EG_TH, col0 = (bid % tiles_x) * EG_TW;
    const int NS = p.cin / 32;
    const half_t* zp = reinterpret_cast<const half_t*>(g_zero_row);
    const int hs = UP ? p.h >> 1 : p.h, wsrc = UP ? p.w >> 1 : p.w;

    // ---- loader state: halo piece j of this wave covers halo pixels (wid + 8 j) * 16 .. + 15; lane -> (pixel, swizzled 16-byte chunk)
    long long hoff[EG_NH];                                          // element offset of the lane's chunk at slab 0, or -1 (outside / spare)
#pragma unroll
    for (int j = 0; j < EG_NH; ++j) {
        const int hp = (wid + 8 * j) * 16 + (lane >> 2);
        const int hy = hp / EG_HW2, hx = hp - hy * EG_HW2;
        const int iy = row0 + hy - 1, ix = col0 + hx - 1;
        const bool in = hp < EG_HP && (unsigned)iy < (unsigned)p.h && (unsigned)ix < (unsigned)p.w;
        const long long pix = (long long)img * hs * wsrc + (UP ? (long long)(iy >> 1) * wsrc + (ix >> 1) : (long long)iy * wsrc + ix);
        hoff[j] = in ? pix * p.ldx + (((lane & 3) ^ ((hp >> 2) & 3)) * 8) : -1;
    }
    int boff[NBW];                                                  // element offset of the lane's weight chunk at slab 0, or -1 (spare piece)
#pragma unroll
    for (int i = 0; i < NBW; ++i) {
        const int row = (wid + 8 * i) * 16 + (lane >> 2);
        const int tap = row / COUT, n = row - tap * COUT;
        boff[i] = wid + 8 * i < BPIECES ? n * 9 * p.cin + tap * p.cin + (((lane & 3) ^ ((row >> 2) & 3)) * 8) : -1;
    }
    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr(reinterpret_cast<const half_t*>(smem)));
    auto issue = [&](int s, int buf) {                             // channel slab s -> halo / weight buffer buf: EG_NH + NBW DMA instructions per wave
#pragma unroll
        for (int j = 0; j < EG_NH; ++j) {
            const half_t* g = hoff[j] >= 0 ? p.x + hoff[j] + s * 32 : zp + (lane & 3) * 8;
            glds16(g, smem_base + (unsigned)(buf * EG_HBYTES) + (unsigned)(wid + 8 * j) * 1024u);
        }
#pragma unroll
        for (int i = 0; i < NBW; ++i) {
            const half_t* g = boff[i] >= 0 ? p.wt + boff[i] + s * 32 : zp + (lane & 3) * 8;
            const int slot = wid + 8 * i < BPIECES ? wid + 8 * i : BPIECES;
            glds16(g, smem_base + (unsigned)(2 * EG_HBYTES + buf * BBYTES) + (unsigned)slot * 1024u);
        }
    };

    const int fr = lane & 15, fq = lane >> 4;
    const int wr = wid >> 1, wc = wid & 1;
    const int hp0 = wr * 4 * EG_HW2 + wc * 16 + fr;                 // halo pixel of (output row 0 of the wave, its column) at tap (0, 0)
    const unsigned bsw = (unsigned)(fq ^ ((fr >> 2) & 3)) << 4;

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    issue(0, 0);
    for (int s = 0; s < NS; ++s) {
        const int buf = s & 1;
        if (s + 1 < NS) {
            issue(s + 1, buf ^ 1);                                  // that buffer was last read in slab s - 1, behind the closing barrier
            wait_vmcnt<EG_NH + NBW>();                              // everything of mine but slab s + 1 has landed
        } else {
            wait_vmcnt<0>();
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        const char* rdA = smem + buf * EG_HBYTES;
        const char* rdB = smem + 2 * EG_HBYTES + buf * BBYTES + fr * 64 + bsw;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            half8 fa[TM], fb[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = as_half8(ld16(rdB + (t * COUT + j * 16) * 64));
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int hp = hp0 + (i + t / 3) * EG_HW2 + t % 3;
                fa[i] = as_half8(ld16(rdA + hp * 64 + ((fq ^ ((hp >> 2) & 3)) << 4)));
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
    }

    // ---- epilogue: lane (fr, fq) holds channels j * 16 + fq * 4 .. + 3 of pixel (row0 + 4 wr + i, col0 + 16 wc + fr)
    const int ox = col0 + wc * 16 + fr;
    half4 bias[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) bias[j] = p.bias != nullptr ? *reinterpret_cast<const half4*>(p.bias + j * 16 + fq * 4) : (half4){0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int oy = row0 + wr * 4 + i;
        if (oy >= p.h || ox >= p.w) continue;
        const long long pix = ((long long)img * p.h + oy) * p.w + ox;
        half4 r1[TN], r2[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            r1[j] = p.r1 != nullptr ? *reinterpret_cast<const half4*>(p.r1 + pix * p.ldr1 + j * 16 + fq * 4) : (half4){0, 0, 0, 0};
            r2[j] = p.r2 != nullptr ? *reinterpret_cast<const half4*>(p.r2 + pix * p.ldr2 + j * 16 + fq * 4) : (half4){0, 0, 0, 0};
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            half4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[i][j][r] + (float)bias[j][r];
                if (p.slope != 0.f) v = v > 0.f ? v : p.slope * v;
                if (p.r1 != nullptr) v = p.s1 * v + (float)r1[j][r];
                if (p.r2 != nullptr) v = p.s2 * v + (float)r2[j][r];
                o[r] = (half_t)v;
            }
            *reinterpret_cast<half4*>(p.y + pix * p.ldy + p.c_off + j * 16 + fq * 4) = o;
            if (p.y2 != nullptr) *reinterpret_cast<half4*>(p.y2 + pix * p.ldy2 + j * 16 + fq * 4) = o;
        }
    }
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
struct ld_esrgan {
    ld_esrgan_config cfg;
    ParamTable pt;
    int first_w = -1, first_b = -1, trunk_w = -1, trunk_b = -1, hr_w = -1, hr_b = -1, last_w = -1, last_b = -1;
    std::vector<int> rdb_w, rdb_b;   // [(block * 3 + rdb) * 5 + conv]
    std::vector<int> up_w, up_b;
    int n_up = 0;
    Arena arena;
    char* ws_base = nullptr;
    size_t ws_bytes = 0;
    int last_launches = 0;
    double last_flops = 0.0;
    Timing timing;
    bool want_timing = false;
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
    Exec ex;
    ex.stream = stream;
    ex.dry = dry;
    Arena plan;
    ex.arena = dry ? &plan : &e->arena;
    if (e->want_timing && !dry) {
        e->timing.reset();
        ex.timing = &e->timing;
    }
    Arena& ar = *ex.arena;
    ar.release(0);
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
    const auto launched = [] { return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP; };

    // conv_first: the trunk's input, and the first RRDB's (dense buffer 0 and the outer-residual copy)
    ex.launch(KC_MISC, 2.0 * npix * nf * 27, "conv_first", (long long)npix, nf, 27, 1, "esrgan_first_kernel", [&] {
        hipLaunchKernelGGL(esrgan_first_kernel, dim3((unsigned)((npix * 8 + 255) / 256)), dim3(256), 0, stream, x, pt.ptr(e->first_w), pt.ptr(e->first_b), dense[0],
                           ldd, trunk_in, nf, b, h, w);
        return launched();
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
        hipLaunchKernelGGL(esrgan_last_kernel, dim3((unsigned)((opix + 255) / 256)), dim3(256), 0, stream, hr, nf, pt.ptr(e->last_w), pt.ptr(e->last_b), out, b, H, W);
        return launched();
    });
    if (dry_peak != nullptr) *dry_peak = ar.peak;
    if (!dry) {
        e->last_launches = ex.launches;
        e->last_flops = ex.flops;
    }
    return ex.status;
}

}  // namespace

extern "C" {

int ld_esrgan_create(const ld_esrgan_config* cfg, ld_esrgan** out) {
    if (cfg == nullptr || out == nullptr) return LD_ERR_ARG;
    ld_esrgan* e = new ld_esrgan();
    e->cfg = *cfg;
    const int st = esrgan_build(e);
    if (st != LD_OK) {
        e->pt.destroy();
        delete e;
        return st;
    }
    *out = e;
    return LD_OK;
}

void ld_esrgan_destroy(ld_esrgan* e) {
    if (e == nullptr) return;
    e->pt.destroy();
    e->timing.destroy();
    if (e->ws_base) (void)hipFree(e->ws_base);
    delete e;
}

int ld_esrgan_param_count(const ld_esrgan* e) { return e ? (int)e->pt.slots.size() : 0; }

int ld_esrgan_param_info(const ld_esrgan* e, int i, const char** name, int* ndim, int64_t shape[4]) {
    return abi_param_info(e ? &e->pt : nullptr, i, name, ndim, shape);
}

int ld_esrgan_load_param(ld_esrgan* e, const char* name, const void* src, int dtype, void* stream) {
    return abi_load_param(e ? &e->pt : nullptr, name, src, dtype, stream);
}

size_t ld_esrgan_plan_bytes(ld_esrgan* e, int b, int h, int w) {
    if (e == nullptr || b < 1 || h < 1 || w < 1) return 0;
    size_t peak = 0;
    if (esrgan_run(e, true, nullptr, nullptr, b, h, w, nullptr, &peak) != LD_OK) return 0;
    return (peak + 4095) / 4096 * 4096 + 4096;
}

int ld_esrgan_reserve(ld_esrgan* e, int max_b, int max_h, int max_w) {
    if (e == nullptr || max_b < 1 || max_h < 1 || max_w < 1) return LD_ERR_ARG;
    const size_t bytes = ld_esrgan_plan_bytes(e, max_b, max_h, max_w);
    if (bytes == 0) return LD_ERR_SHAPE;
    if (e->ws_base) {
        (void)hipFree(e->ws_base);
        e->ws_base = nullptr;
    }
    e->arena = Arena();
    e->ws_bytes = 0;
    if (hipMalloc((void**)&e->ws_base, bytes) != hipSuccess) {
        e->ws_base = nullptr;
        return LD_ERR_HIP;
    }
    e->ws_bytes = bytes;
    e->arena.base = e->ws_base;
    e->arena.cap = bytes - 4096;
    return LD_OK;
}

size_t ld_esrgan_workspace_bytes(const ld_esrgan* e) { return e ? e->ws_bytes : 0; }

int ld_esrgan_forward(ld_esrgan* e, const float* x, float* out, int b, int h, int w, void* stream) {
    if (e == nullptr || x == nullptr || out == nullptr) return LD_ERR_ARG;
    if (e->ws_base == nullptr || !e->pt.all_loaded()) return LD_ERR_STATE;
    if (b < 1 || h < 1 || w < 1) return LD_ERR_SHAPE;
    size_t peak = 0;
    const int st = esrgan_run(e, true, nullptr, nullptr, b, h, w, nullptr, &peak);
    if (st != LD_OK) return st;
    if (peak > e->arena.cap) return LD_ERR_SHAPE;
    return esrgan_run(e, false, x, out, b, h, w, (hipStream_t)stream);
}

int ld_esrgan_profile(ld_esrgan* e, const float* x, float* out, int b, int h, int w, void* stream) {
    if (e == nullptr) return LD_ERR_ARG;
    e->want_timing = true;
    const int st = ld_esrgan_forward(e, x, out, b, h, w, stream);
    e->want_timing = false;
    return st != LD_OK ? st : abi_profile_collect(e->timing, stream);
}

int ld_esrgan_profile_launches(const ld_esrgan* e, char* buf, size_t buf_bytes) {
    return abi_profile_launches(e ? &e->timing : nullptr, buf, buf_bytes);
}

int ld_esrgan_last_launches(const ld_esrgan* e) { return e ? e->last_launches : 0; }
double ld_esrgan_last_flops(const ld_esrgan* e) { return e ? e->last_flops : 0.0; }

}  // extern "C"
