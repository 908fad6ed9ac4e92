// conv6_kernel: the halo-tile 3x3 stride-1 convolution on the 256 x 320 skeleton (epilogues: gemm5_epilogue.h), and its launcher.
#include "gemm5_epilogue.h"

namespace {

// =====================================================================================================================
// v6: 3x3 stride-1 convolution on the v5 skeleton (256 x 320 tile, 8 waves, two wave groups half a step apart), with the A
// operand taken from a HALO tile: the 256 output pixels of a tile are 256 / W whole image rows, so for one 32-channel slab the
// (256 / W + 2) x (W + 2) input pixels they touch are copied to LDS ONCE (LDS-DMA, image border = zero page) and the nine taps
// read their fragments from it at literal offsets — K runs slab-major, tap-minor.  Against v5's implicit im2col the A share of
// the LDS-DMA falls from 16 pieces per 32-wide step to ceil(HP / 16) pieces per NINE steps (W = 64: 25), i.e. 36 -> 22.8 pieces
// per step in total, and every input byte leaves L2 once per tile instead of nine times.
// Weights stay in the checkpoint-derived [Cout][tap][Cin] order: the B pointer just walks  +Cin per tap, +32 - 8 Cin per slab.
// The halo is double-buffered (slab s+1 is fetched during the nine steps of slab s); its rows are 64 bytes, unswizzled: the
// four A fragment reads of a step are 2-way bank-conflicted (of 14 reads; the LDS port is ~25 % busy).
// Requirements (gemm_launch): ksize 3, stride 1, pad 1, no resize, Wo == W in {16, 32, 64, 128}, Ho * Wo % 256 == 0,
// C1 % 32 == 0, C2 % 32 == 0, N % 320 == 0; a split over K is a split over slabs.
// =====================================================================================================================
// Round 3: (i) the tile is W pixels wide but the IMAGE may be wider (W = 128 only: p.Wo = 256, 512, 1024 ... — a tile is then TR rows
// of one 128-pixel column band; the VAE's 256- and 512-pixel-row stages), (ii) BM = 512 (four rows of a 128-pixel band, wave tile
// 128 x BN/2) gives the N = 128 convolutions of the VAE's last level 32 MFMAs per phase instead of 16, (iii) UP: the input is the
// nearest-2x upsampling of the source (Upsample / Upsample1, LD.py:3498-3511, 5114-5152): halo pixel (y, x) comes from source pixel
// (y >> 1, x >> 1) — only the loader's address changes.
// Skip segment (SKIP, gemm.h S1 / S2): after the last 3x3 slab of the workgroup's K range come (SC1 + SC2) / 32 (split over K: its share of
// them) CENTRE-ONLY steps.  A skip step's A operand is the tile's own 256 output pixels x 32 channels of the RAW source: a dense 16 KB
// image, 16 one-KB LDS-DMA pieces (two per wave) — no border, no zero page, never normalised — in a four-slot ring laid over the halo
// buffers, rows swizzled like the B ring's (V5_SWZ) so that its fragment reads are conflict-free; its B operand is the next 32 of the
// weight row's appended columns [O][tap][I | skip].  The image of skip step j is issued two steps ahead (B: three): the first two during
// taps 7 and 8 of the last slab, into the slots that the halo buffer NOT holding that slab covers (whichever it is), the third at skip
// step 0, when nobody reads a halo any more.  22.8 -> 20 + 16 = 36 pieces per skip step, against 45 for a halo slab spent on one tap.
template <int W, bool GN, int BN = V5_BN, int BM = V5_BM, bool UP = false, bool SKIP = false>
                                            // GN: GroupNorm (+SiLU) of the input fused into the halo (separate instantiation: the plain conv keeps its
                                            // registers); BN: tile width 320 (the UNet's N = 320 k), 256 (the VAE's N = 256 / 512) or 128 (its N = 128)
__global__ __launch_bounds__(512, 2) void conv6_kernel(const GemmParams p) {
    constexpr int TM = BM / 64, TN = BN / 32;
    static_assert(BN == 320 || BN == 256 || BN == 160 || BN == 128 || BN == 32, "tile width");
    static_assert(BM == 256 || (BM == 512 && W == 128), "tile height: 256 pixels, or four rows of a 128-pixel band");
    static_assert(!GN || BN == V5_BN || (W == 128 && ((BN == 256 && BM == 256) || (BN == 128 && BM == 512))),
                  "the fused GroupNorm only pays where the output is one tile wide: the UNet's N = 320, the VAE's N = 256 / 128 at >= 256-pixel rows");
    static_assert(!(GN && UP), "no caller");
    constexpr int BPIECES = BN / 16, NB_ALL = BPIECES / 8, NB_EXTRA = BPIECES % 8;   // B pieces of a step: NB_ALL per wave + one more for waves < NB_EXTRA
    constexpr int TR = BM / W, HW2 = W + 2, HP = (TR + 2) * HW2;       // tile rows, halo row pitch (pixels), halo pixels
    constexpr int NH = ((HP + 15) / 16 + 7) / 8;                      // halo LDS-DMA pieces per wave and slab (uniform: spare pieces copy zeros)
    constexpr int HBYTES = NH * 8 * 1024;                              // one halo buffer
    constexpr int BSTAGE = BN * 64, NSTB = 4;                          // B ring: 4 stages of BN rows x 64 bytes
    constexpr int SKA_BYTES = 256 * 64, SKA_SLOTS = 4;                 // skip segment: one dense A image (256 pixels x 32 channels), slots of its ring
    static_assert(!SKIP || (W <= 64 && BN == V5_BN && BM == V5_BM && !UP), "skip segment: whole-image-width tiles of the 256 x 320 skeleton");
    constexpr int RING0 = (SKIP && 2 * HBYTES < SKA_SLOTS * SKA_BYTES) ? SKA_SLOTS * SKA_BYTES : 2 * HBYTES;   // byte offset of the B ring
    __shared__ __attribute__((aligned(16))) char smem5[RING0 + NSTB * BSTAGE];
    static_assert(RING0 + NSTB * BSTAGE <= 163840, "LDS");
    static_assert(!GN || NH <= 7, "fused GroupNorm: my (<= 7) pieces of the next slab are normalised in one go in the read phase of tap 3 (28 temporaries)");
    // fused GroupNorm: every wave keeps the 32 scales + 32 shifts of the slab being normalised in 256 bytes of LDS.  Where the
    // halo buffers and the B ring already take all 160 KB (W = 128) the tables live in spare piece slots of halo buffer 0 and the
    // spare (all-zero) pieces of every wave are sent to the last slot instead
    constexpr int HPIECES = (HP + 15) / 16;
    constexpr bool TBL_IN_HALO = 2 * HBYTES + NSTB * BSTAGE + 2048 > 163840;
    static_assert(!TBL_IN_HALO || NH * 8 - HPIECES >= 3, "two table slots and a dump slot");
    __shared__ __attribute__((aligned(16))) float gn_lds[(GN && !TBL_IN_HALO) ? 8 * 64 : 4];
    static_assert(8 * 2 * (BN == V5_BN ? V5_EPI_BYTES : 16 * (BN / 2 + 4) * 2) + 8 * (BN / 16) * 16 <= 2 * HBYTES + NSTB * BSTAGE,
                  "epilogue staging (+ the GroupNorm partials of the output) must fit");

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool grp1 = wid >= 4;
    const int wm = wid >> 1;
    const int wm0 = wm * (BM / 4), wn0 = (wid & 1) * (BN / 2);
    const int tiles_m = p.M / BM, tiles_n = p.N / BN;
    const int tiles = tiles_m * tiles_n;
    const int splitk = p.splitk > 1 ? p.splitk : 1;
    int bid = xcd_remap(blockIdx.x, tiles * splitk);
    const int ks = bid / tiles;
    bid -= ks * tiles;
    const int tn_i = bid % tiles_n, tm_i = bid / tiles_n;
    const int n0 = tn_i * BN;
    const int Cin = p.C1 + p.C2;
    const int NS = Cin / 32;                                           // channel slabs
    const int s_begin = (int)((long long)ks * NS / splitk), s_end = (int)((long long)(ks + 1) * NS / splitk);
    // skip segment: every slice over K takes an equal share of the skip steps behind its slabs (slices stay even; the bias is the reduce pass's)
    const int NQ = SKIP ? (p.SC1 + p.SC2) / 32 : 0;
    const int q_begin = SKIP ? (int)((long long)ks * NQ / splitk) : 0, nq = SKIP ? (int)((long long)(ks + 1) * NQ / splitk) - q_begin : 0;
    const int nk_main = (s_end - s_begin) * 9;
    const int nk = nk_main + nq;                                       // 32-wide steps of this workgroup (>= 9)

    const half_t* zp = reinterpret_cast<const half_t*>(g_zero_row);
    // this tile = rows row0 .. row0 + TR - 1, columns col0 .. col0 + W - 1 of image img (W < 128: the image is W wide, col0 = 0)
    const int Wimg = W == 128 ? p.Wo : W;
    const int HWo = p.Ho * Wimg;
    const int bands = Wimg / W, tiles_img = (p.Ho / TR) * bands;
    const int img = tm_i / tiles_img, t_in = tm_i - img * tiles_img;
    const int row0 = (t_in / bands) * TR, col0 = (t_in - (t_in / bands) * bands) * W;

    // ---- halo loader state: piece j of this wave covers halo pixels (wid + 8 j) * 16 .. + 15; lane -> (pixel, 16-byte chunk)
    int hpix[NH];                                                      // source pixel index inside the image, or -1 (border / spare)
#pragma unroll
    for (int j = 0; j < NH; ++j) {
        const int hp = (wid + 8 * j) * 16 + (lane >> 2);
        const int hy = hp / HW2, hx = hp - hy * HW2;
        const int iy = row0 + hy - 1, ix = col0 + hx - 1;
        const bool in = hp < HP && (unsigned)iy < (unsigned)p.Ho && (unsigned)ix < (unsigned)Wimg;
        hpix[j] = !in ? -1 : UP ? (iy >> 1) * (Wimg >> 1) + (ix >> 1) : iy * Wimg + ix;
    }
    const unsigned smem_base = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)(const __attribute__((address_space(3))) void*)smem5);
    auto issue_halo = [&](int s, int buf) {                            // channel slab s (32 channels of the concatenated input) -> halo buffer buf
        const int c0 = s * 32;
        const bool second = c0 >= p.C1;
        const half_t* src = (second ? p.A2 : p.A) + (long long)img * p.Hs * p.Ws * (second ? p.C2 : p.C1) + (second ? c0 - p.C1 : c0) + (lane & 3) * 8;
        const int Cs = second ? p.C2 : p.C1;
#pragma unroll
        for (int j = 0; j < NH; ++j) {
            const half_t* g = hpix[j] >= 0 ? src + (long long)hpix[j] * Cs : zp;
            const int slot = (GN && TBL_IN_HALO && wid + 8 * j >= HPIECES) ? NH * 8 - 1 : wid + 8 * j;
            glds16(g, smem_base + (unsigned)(buf * HBYTES) + (unsigned)slot * 1024u);
        }
    };
    // ---- fused GroupNorm (+SiLU) of the input (GN): y = x * scale[img][c] + shift[img][c], applied to the halo IN LDS, each lane on
    // the 16-byte chunks it copied itself (so only its own DMA wait orders it).  The 32 scales and 32 shifts of a slab are fetched by
    // ONE untracked load per lane (lane l: entry l of [scale | shift]) and parked in this wave's 256-byte LDS table.
    // Border pixels stay zero: the convolution pads the NORMALISED tensor.
    float gn_tbl = 0.f;
    auto gn_load = [&](int s) {          // issued BEFORE the halo pieces of the same slab: their wait covers it (in-order completion)
        const float* src = ((lane & 32) ? p.gn_shift : p.gn_scale) + (long long)img * Cin + s * 32 + (lane & 31);
        asm volatile("global_load_dword %0, %1, off" : "=&v"(gn_tbl) : "v"(src) : "memory");
    };
    float* const gn_mine = (TBL_IN_HALO ? reinterpret_cast<float*>(smem5 + HPIECES * 1024) : gn_lds) + wid * 64;
    auto gn_apply_slab = [&](int buf) {
        // runs at the head of a read phase, fenced off from the fragment reads behind it: the 56 fragment registers are dead there,
        // so the temporaries below cost no accumulator spills.  All NH pieces in one go: their LDS reads overlap each other.
        __builtin_amdgcn_sched_barrier(0);
        gn_mine[lane] = gn_tbl;          // same wave reads it back: in-order LDS, no barrier
        const float* tp = gn_mine + (lane & 3) * 8;
        H8 io[NH];
#pragma unroll
        for (int j = 0; j < NH; ++j) io[j].u = ld16(smem5 + buf * HBYTES + (wid + 8 * j) * 1024 + lane * 16);
        const f32x4 sc0 = *reinterpret_cast<const f32x4*>(tp), sc1 = *reinterpret_cast<const f32x4*>(tp + 4);
        const f32x4 sh0 = *reinterpret_cast<const f32x4*>(tp + 32), sh1 = *reinterpret_cast<const f32x4*>(tp + 36);
#pragma unroll
        for (int j = 0; j < NH; ++j) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = (float)io[j].e[e] * (e < 4 ? sc0[e & 3] : sc1[e & 3]) + (e < 4 ? sh0[e & 3] : sh1[e & 3]);
                if (p.gn_silu) v *= __builtin_amdgcn_rcpf(1.0f + __expf(-v));   // SiLU with v_rcp_f32 (1 ulp; rounded to fp16 anyway)
                io[j].e[e] = (half_t)v;
            }
            if (hpix[j] >= 0) st16(smem5 + buf * HBYTES + (wid + 8 * j) * 1024 + lane * 16, io[j].u);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    // ---- B loader state (as v5): NB_ALL pieces per wave and step, one more for waves < NB_EXTRA (BN = 320: 2 + waves 0-3)
    const int prow = lane >> 2;
    const int lchunk = (lane & 3) ^ ((V5_SWZ >> (2 * ((prow >> 2) & 3))) & 3);
    const bool b_extra = wid < NB_EXTRA;                                // (wave-uniform)
    unsigned b_off[NB_ALL + 1];
#pragma unroll
    for (int i = 0; i < NB_ALL + 1; ++i) {
        const int piece = i < NB_ALL ? wid * NB_ALL + i : 8 * NB_ALL + (wid % (NB_EXTRA > 0 ? NB_EXTRA : 1));
        const int n = n0 + piece * 16 + prow;
        b_off[i] = (unsigned)(((long long)n * p.ldw + lchunk * 8) * 2);
    }
    const half_t* b_base = p.W + (long long)s_begin * 32;              // step (slab s_begin, tap 0); wave-uniform
    int b_tap = 0;
    int b_main = nk_main;                                              // (SKIP) steps of the 3x3 segment still to issue
    unsigned st_issue = 0;                                             // byte offset (inside the B ring) of the stage the next step goes to
    auto issue_b = [&]() {
        const unsigned Bs = smem_base + (unsigned)RING0 + st_issue;
#pragma unroll
        for (int i = 0; i < NB_ALL; ++i) glds16s(b_off[i], b_base, Bs + (unsigned)(wid * NB_ALL + i) * 1024u);
        if (NB_EXTRA > 0 && b_extra) glds16s(b_off[NB_ALL], b_base, Bs + (unsigned)(8 * NB_ALL + wid) * 1024u);
        if (SKIP && --b_main <= 0) {                                    // behind the last tap of the last slab: the appended columns, 32 per step
            b_base = b_main == 0 ? p.W + 9 * Cin + q_begin * 32 : b_base + 32;
        } else if (b_tap == 8) {
            b_tap = 0;
            b_base += 32 - 8 * Cin;
        } else {
            ++b_tap;
            b_base += Cin;
        }
        st_issue = st_issue == (unsigned)((NSTB - 1) * BSTAGE) ? 0u : st_issue + (unsigned)BSTAGE;
    };
    // ---- skip segment loader: piece 2 wid + i of a step = tile pixels (2 wid + i) * 16 .. + 15 (consecutive pixels of the image: the tile is
    // whole rows), lane -> (pixel, swizzled 16-byte chunk); the source switches from S1 to S2 between steps (SC1 % 32 == 0)
    int ska_slot = 0;                                                  // ring slot of skip step 0, then of the next image to issue
    int ska_read = 0;                                                  // byte offset of the slot the next skip step reads
    if constexpr (SKIP) {
        // the last slab sits in halo buffer (slabs - 1) & 1; the first two images go where the OTHER buffer (or nothing) lies
        const bool last0 = ((s_end - s_begin - 1) & 1) == 0;
        ska_slot = last0 ? 2 : (HBYTES < 2 * SKA_BYTES ? 3 : 0);
        ska_read = ska_slot * SKA_BYTES;
    }
    auto issue_ska = [&](int q) {                                      // skip step q (32 channels of the concatenated skip sources) -> slot ska_slot
        const int c0 = q * 32;
        const bool second = c0 >= p.SC1;
        const int Cs = second ? p.SC2 : p.SC1;
        const half_t* src = (second ? p.S2 : p.S1) + ((long long)img * HWo + row0 * W + wid * 32) * Cs + (second ? c0 - p.SC1 : c0);
        const unsigned voff = (unsigned)((prow * Cs + lchunk * 8) * 2);
        const unsigned dst = smem_base + (unsigned)(ska_slot * SKA_BYTES) + (unsigned)wid * 2048u;
        glds16s(voff, src, dst);
        glds16s(voff, src + 16 * Cs, dst + 1024u);
        ska_slot = (ska_slot + 1) & (SKA_SLOTS - 1);
    };
    // "every LDS-DMA of mine but the n newest steps' B pieces (+ the halo pieces when they sit among those) has landed"
    // ska: this step issued a skip image (two pieces, in front of its B pieces; never in a step that leaves halo pieces in flight) — the
    // image issued one step earlier is among what has landed
    auto wait_keep = [&](int steps, bool halo, bool ska = false) {
        constexpr int PX = NB_ALL + 1, PA = NB_ALL;                      // pieces per step of a wave with / without the extra piece
        if (SKIP && ska) {
            if (NB_EXTRA > 0 && b_extra) {
                if (steps >= 2) wait_vmcnt<2 * PX + 2>(); else if (steps == 1) wait_vmcnt<PX + 2>(); else wait_vmcnt<0>();
            } else {
                if (steps >= 2) wait_vmcnt<2 * PA + 2>(); else if (steps == 1) wait_vmcnt<PA + 2>(); else wait_vmcnt<0>();
            }
            return;
        }
        if (NB_EXTRA > 0 && b_extra) {
            if (steps >= 2) { if (halo) wait_vmcnt<2 * PX + NH>(); else wait_vmcnt<2 * PX>(); }
            else if (steps == 1) { if (halo) wait_vmcnt<PX + NH>(); else wait_vmcnt<PX>(); }
            else wait_vmcnt<0>();
        } else {
            if (steps >= 2) { if (halo) wait_vmcnt<2 * PA + NH>(); else wait_vmcnt<2 * PA>(); }
            else if (steps == 1) { if (halo) wait_vmcnt<PA + NH>(); else wait_vmcnt<PA>(); }
            else wait_vmcnt<0>();
        }
    };

    // ---- fragment read bases: A = halo pixel of output pixel (wm0 + 16 i + fr) at tap (0,0), B as v5
    const int fr = lane & 15, fq = lane >> 4;
    const int oyw = wm0 / W, oxw = wm0 - oyw * W;                      // first output pixel of this wave inside the tile
    // the wave's BM / 4 output pixels are consecutive rows of the [M][N] output (one image row segment, or whole rows of a narrow image)
    const int m0 = img * HWo + (row0 + oyw) * Wimg + col0 + oxw - wm0;   // so that m0 + wm0 is the wave's first output row
    const char* rdA = smem5 + ((oyw * HW2 + oxw + fr) * 64 + fq * 16);
    const unsigned rchunk = (unsigned)(fq ^ ((V5_SWZ >> (2 * ((fr >> 2) & 3))) & 3)) << 4;
    const char* rdB = smem5 + RING0 + (wn0 + fr) * 64 + rchunk;
    int st_read = 0;

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    half8 fa[TM], fb[TN];

    // ---- prologue: halo of the first slab and B steps 0..2 in flight; step 0 + halo landed and published; group 1 one barrier behind
    if (GN) gn_load(s_begin);
    issue_halo(s_begin, 0);
    issue_b();
    issue_b();
    issue_b();
    wait_keep(2, false);
    if (GN) gn_apply_slab(0);
    __builtin_amdgcn_s_barrier();
    if (grp1) __builtin_amdgcn_s_barrier();

    int k = 0;
    for (int s = s_begin; s < s_end; ++s) {
        const int hb = (s - s_begin) & 1;
        const char* rdAs = rdA + hb * HBYTES;
#pragma unroll
        for (int t = 0; t < 9; ++t, ++k) {
            // ------------------------------------------------ read phase (the partner wave of this SIMD is in its MFMA phase)
            if (t == 0 && s + 1 < s_end) {
                if (GN) gn_load(s + 1);
                issue_halo(s + 1, hb ^ 1);                             // the other buffer was last read in slab s-1: free for everyone
            }
            if (GN && t == 3 && s + 1 < s_end) gn_apply_slab(hb ^ 1);   // my table load and halo pieces of slab s+1 landed at tap 2's wait
            const bool ska = SKIP && t >= 7 && s + 1 == s_end && t - 7 < nq;   // images of skip steps 0 and 1: the other halo buffer is free
            if (SKIP && ska) issue_ska(q_begin + t - 7);
            if (k + 3 < nk) issue_b();
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = as_half8(ld16(rdB + j * 1024));
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                // output pixel block i of this wave: 16 pixels of one image row; literal offset of its tap-(ky,kx) halo pixels
                const int pi = i * 16;                                   // (wm0 % W + 16 i) stays inside the row: W % 16 == 0 and wm0 % 16 == 0
                const int oy = (W >= 64) ? 0 : pi / W, ox = (W >= 64) ? pi : pi % W;
                fa[i] = as_half8(ld16(rdAs + ((oy + t / 3) * HW2 + ox + t % 3) * 64));
            }
            {
                const int d = st_read == NSTB - 1 ? -(NSTB - 1) * BSTAGE : BSTAGE;
                rdB += d;
                st_read = st_read == NSTB - 1 ? 0 : st_read + 1;
            }
            // my B pieces of step k+1 (and, from tap 2 on, the next slab's halo pieces) have landed; the barrier publishes them
            wait_keep(k + 3 < nk ? 2 : (k + 2 < nk ? 1 : 0), t < 2 && s + 1 < s_end, ska);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // ------------------------------------------------ MFMA phase (the partner reads / stages)
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (GN || SKIP)   // in-place form pinned in asm: with the fused-GroupNorm code (or the skip steps' second loop) around, hipcc
                              // otherwise renames the accumulators between the unrolled taps (D != C) and spills them inside this phase
                        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc[i][j]) : "v"(fb[j]), "v"(fa[i]));
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
                }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
        }
    }
    if constexpr (SKIP) {
        // ---- the skip steps: the same two phases, the A fragments from the dense image of the step (pixel wm0 + 16 i + fr, swizzled chunk)
        const char* rdS = smem5 + (wm0 + fr) * 64 + rchunk;
        for (int j = 0; j < nq; ++j, ++k) {
            const bool ska = j + 2 < nq;
            if (ska) issue_ska(q_begin + j + 2);                        // its slot was last read two steps ago
            if (k + 3 < nk) issue_b();
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) fb[jn] = as_half8(ld16(rdB + jn * 1024));
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = as_half8(ld16(rdS + ska_read + i * 1024));
            {
                const int d = st_read == NSTB - 1 ? -(NSTB - 1) * BSTAGE : BSTAGE;
                rdB += d;
                st_read = st_read == NSTB - 1 ? 0 : st_read + 1;
                ska_read = (ska_read + SKA_BYTES) & (SKA_SLOTS * SKA_BYTES - 1);
            }
            wait_keep(k + 3 < nk ? 2 : (k + 2 < nk ? 1 : 0), false, ska);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int jn = 0; jn < TN; ++jn) {
                    if (GN || SKIP) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc[i][jn]) : "v"(fb[jn]), "v"(fa[i]));   // (as above)
                    else acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[jn], fa[i], acc[i][jn], 0, 0, 0);
                }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
        }
    }
    if (!grp1) __builtin_amdgcn_s_barrier();                            // group 0 waits out group 1's last MFMA phase
    if (GN || SKIP) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");          // the asm MFMAs are invisible to hipcc's hazard recogniser: let the last ones retire before VALU reads the accumulators
    if constexpr (BN == V5_BN) v5_finish<0, false>(p, acc, smem5, nullptr, nullptr, 0, m0, n0, wm0, wn0, wid, lane, ks, splitk, tn_i);
    else v6_finish<TM, TN>(p, acc, smem5, m0, n0, wm0, wn0, wid, lane, ks, splitk, img, t_in);
}

template <int W, bool GN, int BN, int BM, bool UP, bool SKIP = false>
void launch_conv6_w(const GemmParams& p, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((conv6_kernel<W, GN, BN, BM, UP, SKIP>), grid, dim3(512), 0, s, p); }
// the tile widths gemm_plan hands each tile: every width for the 320-column tile, 64 and 128 for the plain 256-column tile, 128 for the rest
template <bool GN, int BN = V5_BN, int BM = V5_BM, bool UP = false>
void launch_conv6(int wc, const GemmParams& p, dim3 grid, hipStream_t s) {
    if constexpr (BN == V5_BN) {
        if (wc == 16) return launch_conv6_w<16, GN, BN, BM, UP>(p, grid, s);
        if (wc == 32) return launch_conv6_w<32, GN, BN, BM, UP>(p, grid, s);
    }
    if constexpr (BN == V5_BN || (BN == 256 && !GN)) {
        if (wc == 64) return launch_conv6_w<64, GN, BN, BM, UP>(p, grid, s);
    }
    launch_conv6_w<128, GN, BN, BM, UP>(p, grid, s);
}

}  // namespace

void conv6_launch(const GemmParams& p, const GemmPlan& pl, dim3 grid, hipStream_t s) {
    if (pl.skip) {   // (gemm_plan: 256 x 320 tiles of whole 16- / 32- / 64-pixel rows, no resize)
        if (pl.gn) {
            if (pl.wc == 16) launch_conv6_w<16, true, V5_BN, V5_BM, false, true>(p, grid, s);
            else if (pl.wc == 32) launch_conv6_w<32, true, V5_BN, V5_BM, false, true>(p, grid, s);
            else launch_conv6_w<64, true, V5_BN, V5_BM, false, true>(p, grid, s);
        } else {
            if (pl.wc == 16) launch_conv6_w<16, false, V5_BN, V5_BM, false, true>(p, grid, s);
            else if (pl.wc == 32) launch_conv6_w<32, false, V5_BN, V5_BM, false, true>(p, grid, s);
            else launch_conv6_w<64, false, V5_BN, V5_BM, false, true>(p, grid, s);
        }
    } else if (pl.gn) {
        if (pl.bn == 256) launch_conv6<true, 256>(pl.wc, p, grid, s);
        else if (pl.bn == 128) launch_conv6<true, 128, 512>(pl.wc, p, grid, s);
        else launch_conv6<true>(pl.wc, p, grid, s);
    } else if (pl.bn == 128) {
        launch_conv6<false, 128, 512>(pl.wc, p, grid, s);
    } else if (pl.bn == 32) {
        launch_conv6<false, 32, 512>(pl.wc, p, grid, s);
    } else if (pl.bn == 256) {
        if (pl.up) launch_conv6<false, 256, V5_BM, true>(pl.wc, p, grid, s);
        else launch_conv6<false, 256>(pl.wc, p, grid, s);
    } else {
        if (pl.up) launch_conv6<false, V5_BN, V5_BM, true>(pl.wc, p, grid, s);
        else launch_conv6<false>(pl.wc, p, grid, s);
    }
}
