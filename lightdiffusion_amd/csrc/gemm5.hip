// gemm5_kernel: the 256 x 320 tile for plain / LayerNorm-fold / GEGLU GEMMs, tap-major convolutions and the upconv route, and its launcher.
#include "gemm5_epilogue.h"

namespace {

// =====================================================================================================================
// v5: one 256 x 320 tile per workgroup, 8 waves (4 x 2, wave tile 64 x 160), 32-wide K steps in a 4-stage LDS-DMA ring, and the
// two wave groups (waves 0-3 / 4-7: the two waves of every SIMD) run HALF A STEP APART:
//     group 0:  | read k   | MFMA k   | read k+1 | MFMA k+1 | ...
//     group 1:  | (idle)   | read k   | MFMA k   | read k+1 | ...           ('|' = one s_barrier joining all 8 waves)
// so in every interval one wave of each SIMD issues 40 MFMAs (640 cycles) while its partner issues the 14 fragment reads
// of its next step and its share of the LDS-DMA for the step after next (4-5 one-KB pieces).  Fragments are single-buffered:
// the overlap comes from the partner wave, not from register double-buffering (160 accumulator + 56 fragment VGPRs at two
// waves per SIMD).  Against the 128 x 160 tile of v3 a step moves half the LDS-DMA pieces and 0.35 instead of 0.45
// fragment reads per MFMA, and nothing of the staging sits in front of the issuing wave's own MFMAs.
//   step k lives in stage k % 4; group 0 reads it in interval 2k, group 1 in 2k+1; it is overwritten (step k+4) from
//   interval 2k+2 on (three steps = 110 KB per CU in flight), and every wave waits for its own pieces of step k+1 (counted vmcnt) before the barrier that ends its
//   read phase k — hence before anybody reads step k+1.
// LDS rows are 64 bytes (4 chunks); chunk c of row r sits at physical chunk c ^ g[(r >> 2) & 3], g = {0, 2, 3, 1}: with the
// lane groups ds_read_b128 is served in ({0-3, 12-15, 20-27}, ...) the 16 lanes of a group then hit 16 distinct 16-byte slots.
// Epilogue: per wave, 16-row strips staged two at a time in the (then quiet) ring (rows padded to 328 bytes), 16-byte coalesced
// stores of 320-byte row segments with the same fused bias / row vector / activation / GEGLU / residual / LN-fold math as v3.
// Requirements (gemm_launch checks them): N % 320 == 0, K % 32 == 0, every split-K slice >= 2 steps, no ln_swapped.
// =====================================================================================================================
// UPF (upconv, with CONV): nearest-2x upsample + 3x3 convolution as four 2x2 convolutions of the source image (gemm.h Wup).  Rows are SOURCE
// pixels, columns [phase][Cout], K = [2x2 tap][Cin]; a column tile lies in one phase (Cout % 320 == 0), so the phase (py, px) is
// workgroup-uniform: tap (a, b) of the implicit-im2col loader reads source pixel (y + py - 1 + a, x + px - 1 + b) — outside the image the
// zero page, which is exactly the 3x3 convolution's padding of the upsampled image — and the epilogue stores row (img, y, x) to output pixel
// (2y + py, 2x + px).  A separate instantiation: the others keep their code and registers.
template <bool CONV, int EPI, bool UPF = false>
__global__ __launch_bounds__(512, 2) void gemm5_kernel(const GemmParams p) {
    constexpr int TM = 4, TN = 10;
    __shared__ __attribute__((aligned(16))) char smem5[V5_NST * V5_STAGE_BYTES];
    static_assert(8 * 2 * V5_EPI_BYTES <= V5_NST * V5_STAGE_BYTES, "epilogue staging must fit in the ring");
    __shared__ __attribute__((aligned(16))) float ln_mu[V5_BM], ln_rs[V5_BM];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool grp1 = wid >= 4;
    const int wm0 = (wid >> 1) * 64, wn0 = (wid & 1) * 160;
    const int z = blockIdx.z;
    const int tiles_m = (p.M + V5_BM - 1) / V5_BM, tiles_n = p.N / V5_BN;
    const int tiles = tiles_m * tiles_n;
    const int splitk = p.splitk > 1 ? p.splitk : 1;
    int bid = xcd_remap(blockIdx.x, tiles * splitk);
    const int ks = bid / tiles;
    bid -= ks * tiles;
    int tn_i = bid % tiles_n, tm_i = bid / tiles_n;
    if (!CONV && p.xcd_gm > 0) {
        // plain GEMM, XCD-blocked tile order: XCD x (a contiguous run of tiles / 8 logical ids) owns the block (x / gn, x % gn) of a gm x gn grid
        // over the tile matrix and walks it M-fastest — the workgroups that run together on one XCD share a few W tiles and A panels through
        // its L2.  (N-fastest over whole M panels made every XCD stream ALL of W once per M panel: 433 MB fetched per launch for the
        // 26 MB matrix of the level-2 GEGLU, profiles/pmc_traffic.json round 3.)
        const int gn = 8 / p.xcd_gm, per = tiles >> 3, x = bid / per, l = bid - x * per;
        const int bm_t = tiles_m / p.xcd_gm, bn_t = tiles_n / gn;
        tm_i = (x / gn) * bm_t + l % bm_t;
        tn_i = (x % gn) * bn_t + l / bm_t;
    }
    const int m0 = tm_i * V5_BM, n0 = tn_i * V5_BN;
    const int KT = p.K / V5_BK;
    const int kt_begin = (int)((long long)ks * KT / splitk), kt_end = (int)((long long)(ks + 1) * KT / splitk);
    const int nk = kt_end - kt_begin;                              // >= 2 (gemm_launch)

    const half_t* Ab = p.A + (long long)z * p.sA;
    const half_t* Wb = p.W + (long long)z * p.sW;
    const half_t* zp = reinterpret_cast<const half_t*>(g_zero_row);
    const int Cin = p.C1 + p.C2;

    // ---- loader state: 2 A pieces and 2 (waves 4-7) or 3 (waves 0-3) B pieces per wave and step; a piece = 16 rows x 64 bytes
    const int prow = lane >> 2;                                    // row inside a piece (piece rows start at multiples of 16)
    const int lchunk = (lane & 3) ^ ((V5_SWZ >> (2 * ((prow >> 2) & 3))) & 3);   // logical chunk this lane fetches
    const int a_row0 = wid * 32 + prow;                            // + 16 for the second piece
    const half_t* a_ptr[2];
    unsigned a_off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + a_row0 + i * 16;
        a_ptr[i] = zp;
        a_off[i] = CONV ? 0u : (unsigned)(((long long)(m < p.M ? m : p.M - 1) * p.lda + lchunk * 8) * 2);
    }
    const half_t* a_base = Ab + (long long)kt_begin * V5_BK;        // wave-uniform (plain GEMM)
    int seg_left = 0;
    int k_issue = kt_begin * V5_BK;                                 // K index of the next step to issue
    auto conv_seek = [&](int k0) {
        if constexpr (UPF) {
            const int tap = k0 / Cin, c0 = k0 - tap * Cin;          // tap = a * 2 + b; past the last step (tap 4) the zero page
            const int ph = n0 / (p.N >> 2);
            const int dy = (ph >> 1) - 1 + (tap >> 1), dx = (ph & 1) - 1 + (tap & 1);
            const int hw = p.Hs * p.Ws;
            seg_left = (Cin - c0) / V5_BK;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = m0 + a_row0 + i * 16;
                const int mm = m < p.M ? m : 0;
                const int img = mm / hw, rem = mm - img * hw;
                const int y = rem / p.Ws, x = rem - y * p.Ws;
                const int iy = y + dy, ix = x + dx;
                const bool ok = m < p.M && (unsigned)iy < (unsigned)p.Hs && (unsigned)ix < (unsigned)p.Ws && tap < 4;
                a_ptr[i] = ok ? Ab + (((long long)img * p.Hs + iy) * p.Ws + ix) * Cin + c0 + lchunk * 8 : zp + lchunk * 8;
            }
            return;
        }
        // (k0 beyond the taps: the second K segment — the 1x1 skip convolution's raw sources at the output pixel itself, gemm.h S1 / S2)
        const int K9 = p.ksize * p.ksize * Cin;
        const bool skp = k0 >= K9 && p.SC1 > 0;
        const int tap = skp ? 0 : k0 / Cin;
        const int c0 = skp ? k0 - K9 : k0 - tap * Cin;
        const int ky = skp ? p.pad : tap / p.ksize, kx = skp ? p.pad : tap - (tap / p.ksize) * p.ksize;
        const int Ca = skp ? p.SC1 : p.C1, Cb = skp ? p.SC2 : p.C2;
        const bool second = c0 >= Ca;
        const half_t* src = skp ? (second ? p.S2 : p.S1) : (second ? p.A2 : Ab);
        const int Cs = second ? Cb : Ca;
        const int cl = second ? c0 - Ca : c0;
        seg_left = ((second ? Ca + Cb : Ca) - c0) / V5_BK;
        const int hw = p.Ho * p.Wo;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + a_row0 + i * 16;
            const int mm = m < p.M ? m : 0;
            const int img = mm / hw, rem = mm - img * hw;
            const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
            const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
            const bool ok = m < p.M && (unsigned)iy < (unsigned)p.Hv && (unsigned)ix < (unsigned)p.Wv && tap < p.ksize * p.ksize && c0 < Ca + Cb;
            int sy = iy, sx = ix;
            if (p.Hv == 2 * p.Hs && p.Wv == 2 * p.Ws) {
                sy = iy >> 1;
                sx = ix >> 1;
            } else if (p.Hv != p.Hs || p.Wv != p.Ws) {
                sy = (int)((long long)iy * p.Hs / p.Hv);
                sx = (int)((long long)ix * p.Ws / p.Wv);
            }
            a_ptr[i] = ok ? src + (((long long)img * p.Hs + sy) * p.Ws + sx) * Cs + cl + lchunk * 8 : zp + lchunk * 8;
        }
    };
    unsigned b_off[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int piece = i < 2 ? wid * 2 + i : 16 + (wid & 3);
        const int row = piece * 16 + prow;
        const int n = n0 + row < p.n_valid ? n0 + row : p.n_valid - 1;
        b_off[i] = (unsigned)(((long long)n * p.ldw + lchunk * 8) * 2);
    }
    const half_t* b_base = Wb + (long long)kt_begin * V5_BK;        // wave-uniform

    const unsigned smem_base = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)(const __attribute__((address_space(3))) void*)smem5);
    unsigned st_issue = 0;                                          // byte offset of the stage the next issued step goes to
    auto issue = [&]() {
        const unsigned As = smem_base + st_issue + (unsigned)(wid * 2) * 1024u;
        const unsigned Bs = smem_base + st_issue + (unsigned)V5_A_BYTES;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (CONV) glds16(a_ptr[i], As + (unsigned)i * 1024u);
            else glds16s(a_off[i], a_base, As + (unsigned)i * 1024u);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16s(b_off[i], b_base, Bs + (unsigned)(wid * 2 + i) * 1024u);
        if (!grp1) glds16s(b_off[2], b_base, Bs + (unsigned)(16 + wid) * 1024u);
        k_issue += V5_BK;
        if (CONV) {
            if (--seg_left <= 0) {
                conv_seek(k_issue);
            } else {
                a_ptr[0] += V5_BK;
                a_ptr[1] += V5_BK;
            }
        } else {
            a_base += V5_BK;
        }
        b_base += V5_BK;
        st_issue = st_issue == (unsigned)((V5_NST - 1) * V5_STAGE_BYTES) ? 0u : st_issue + (unsigned)V5_STAGE_BYTES;
    };
    // "my pieces of every step but the n newest ones issued have landed" (in-order completion; 5 or 4 pieces per step and wave)
    auto wait_all_but = [&](int n) {
        if (!grp1) {
            if (n >= 2) wait_vmcnt<10>();
            else if (n == 1) wait_vmcnt<5>();
            else wait_vmcnt<0>();
        } else {
            if (n >= 2) wait_vmcnt<8>();
            else if (n == 1) wait_vmcnt<4>();
            else wait_vmcnt<0>();
        }
    };
    if (CONV) conv_seek(k_issue);

    const int fr = lane & 15, fq = lane >> 4;
    // fragment read bases (bytes into stage 0): A rows wm0 + 16 i + fr, B rows wn0 + 16 j + fr; (row >> 2) & 3 == (fr >> 2) & 3
    const unsigned rchunk = (unsigned)(fq ^ ((V5_SWZ >> (2 * ((fr >> 2) & 3))) & 3)) << 4;
    const char* rdA = smem5 + (wm0 + fr) * 64 + rchunk;
    const char* rdB = smem5 + V5_A_BYTES + (wn0 + fr) * 64 + rchunk;
    int st_read = 0;                                                // stage index of the step this wave reads next

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    half8 fa[TM], fb[TN];

    // ---- prologue: steps 0 .. 2 in flight, step 0 landed and published, group 1 one barrier behind
    issue();
    issue();
    if (nk > 2) issue();
    if (EPI != 0 && p.ln_stat != nullptr) ln_prepare<V5_BM, V5_BN>(p, ln_mu, ln_rs, z, m0, n0, tid);   // (the loop's barriers publish it)
    wait_all_but(nk > 2 ? 2 : 1);
    __builtin_amdgcn_s_barrier();
    if (grp1) __builtin_amdgcn_s_barrier();

    for (int k = 0; k < nk; ++k) {
        // ------------------------------------------------ read phase (the partner wave of this SIMD is in its MFMA phase)
        if (k + 3 < nk) issue();                                    // step k+3 -> the stage step k-1 left (both groups are done with it)
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = as_half8(ld16(rdB + j * 1024));
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = as_half8(ld16(rdA + i * 1024));
        {
            const int d = st_read == V5_NST - 1 ? -(V5_NST - 1) * V5_STAGE_BYTES : V5_STAGE_BYTES;
            rdA += d;
            rdB += d;
            st_read = st_read == V5_NST - 1 ? 0 : st_read + 1;
        }
        // my pieces of step k+1 have landed (steps k+2, k+3, if issued, may stay in flight); the barrier publishes them
        wait_all_but(k + 3 < nk ? 2 : (k + 2 < nk ? 1 : 0));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        // ------------------------------------------------ MFMA phase (the partner reads / stages)
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
    }
    if (!grp1) __builtin_amdgcn_s_barrier();                        // group 0 waits out group 1's last MFMA phase: every wave ran 2 nk + 2 barriers

    v5_finish<EPI, EPI != 0, UPF>(p, acc, smem5, ln_mu, ln_rs, z, m0, n0, wm0, wn0, wid, lane, ks, splitk, tn_i);
}

}  // namespace

void gemm5_launch(const GemmParams& p, const GemmPlan& pl, dim3 grid, hipStream_t s) {
    if (pl.route == GR_UPCONV) {
        hipLaunchKernelGGL((gemm5_kernel<true, 0, true>), grid, dim3(512), 0, s, p);
        return;
    }
    if (pl.conv) hipLaunchKernelGGL((gemm5_kernel<true, 0>), grid, dim3(512), 0, s, p);
    else if (pl.geglu) hipLaunchKernelGGL((gemm5_kernel<false, 2>), grid, dim3(512), 0, s, p);
    else if (pl.ln) hipLaunchKernelGGL((gemm5_kernel<false, 1>), grid, dim3(512), 0, s, p);
    else hipLaunchKernelGGL((gemm5_kernel<false, 0>), grid, dim3(512), 0, s, p);
}
