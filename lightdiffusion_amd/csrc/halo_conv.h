// The 16 x 32 halo-tile 3x3 convolution on fp16 NHWC with the weights and the halo in LDS: the main loop of esrgan_conv_kernel (esrgan.hip)
// and taesd_conv_kernel (taesd.hip), which differ in the epilogue policy only.
#pragma once
#include "gemm_device.h"
#include "kernels.h"

// =====================================================================================================================
// halo_conv_tile: the stride-1 pad-1 3x3 convolution tile that RRDBNet's dense blocks (esrgan.hip) and TAESD (taesd.hip) share:
// N = 32 / 64 output channels, K = 9 * (64 .. 192), any H x W.
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
// Epilogue on the fp32 accumulators, one rounding at the store: Epilogue::apply(p, acc + bias, R1, R2) -> the fp32 value that is stored
// (R1 / R2: the residual elements, 0 where the pointer is null).  The policy is the only thing an instantiating kernel chooses; each kernel
// is a __global__ __launch_bounds__(512, 1) function of 512 threads that calls halo_conv_tile once.
// =====================================================================================================================
constexpr int EG_TH = 16, EG_TW = 32;
constexpr int EG_HW2 = EG_TW + 2, EG_HP = (EG_TH + 2) * EG_HW2;   // halo row pitch (pixels), halo pixels (612)
constexpr int EG_HPIECES = (EG_HP + 15) / 16;                      // 1 KB pieces of a halo slab (39)
constexpr int EG_NH = (EG_HPIECES + 7) / 8;                        // ... per wave (5; the spare piece copies zeros)
constexpr int EG_HBYTES = EG_NH * 8 * 1024;

template <int COUT, bool UP, class Epilogue>
__device__ __forceinline__ void halo_conv_tile(const EsrganConvArgs& p) {
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
                o[r] = (half_t)Epilogue::apply(p, acc[i][j][r] + (float)bias[j][r], (float)r1[j][r], (float)r2[j][r]);
            }
            *reinterpret_cast<half4*>(p.y + pix * p.ldy + p.c_off + j * 16 + fq * 4) = o;
            if (p.y2 != nullptr) *reinterpret_cast<half4*>(p.y2 + pix * p.ldy2 + j * 16 + fq * 4) = o;
        }
    }
}
