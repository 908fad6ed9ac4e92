// gemm7_kernel: the K = 320 row-panel GEMM (shared device helpers: gemm_device.h), and its launcher.
#include "gemm_device.h"
#include "gemm_kernels.h"

namespace {

// =====================================================================================================================
// v7: short-K row-panel GEMM (K = 320: every projection of the level-0 transformer blocks).  One workgroup owns 256 rows and ALL
// of N.  Its A panel never touches LDS: each wave loads the MFMA fragments of its 32 rows once (20 x 16 bytes per lane, 80 VGPRs)
// and keeps them for the whole launch.  W streams through a 2-stage LDS-DMA ring in 80-row tiles (51 KB: the full K of 80 output
// columns), so per 80-column step a wave issues 100 MFMAs against 7 DMA pieces and 50 fragment reads.
// The two wave groups (waves 0-3 / 4-7: the two waves of every SIMD) run HALF A STEP APART, as in v5, but here the second phase of
// a step is its EPILOGUE: while one wave of a SIMD issues the MFMAs of step j the other finishes and stores step j-1 (bias,
// LayerNorm fold, GEGLU, residual, row statistics) — the per-tile prologue + epilogue that costs the 128 x 160 kernel 60 % of its
// time at K = 320 is hidden behind the matrix pipe, and A is read from HBM exactly once.
//     group 0:  | MFMA j   | EPI j    | MFMA j+1 | EPI j+1  | ...
//     group 1:  | (idle)   | MFMA j   | EPI j    | MFMA j+1 | ...           ('|' = s_barrier joining all 8 waves)
//   step j lives in stage j & 1.  Group 0 issues its share of step j+1 in EPI j, group 1 its share of step j+2 in EPI j (the stage is
//   free by then for both); every interval ends with the DMA retired + lgkmcnt(0), so a step is complete one barrier before its first reader.
// The loop is LDS-bandwidth bound (phase clocks, profiles/README.md round 2: with an epilogue that staged its tile through LDS an interval took 4200
// clocks against 2000 for the fragment reads + DMA writes alone), so the epilogue stays OUT of LDS: the 16 W rows an MFMA tile
// reads are chosen such that a lane's accumulators of two neighbouring tiles are 8 CONSECUTIVE output columns —
//     tile jj < 4, MFMA index c  <-  W row 32 (jj >> 1) + 8 (c >> 2) + 4 (jj & 1) + (c & 3);   tile 4: row 64 + (c & 3) + 8 ((c >> 2) & 1) + 4 (c >> 3)
// — and results leave as 16-byte (tile pairs) / 8-byte (tile 4) stores straight from the accumulator layout: 64 + 64 + 32 bytes per
// row and step.  W rows are 640 bytes; chunk c of row r sits at physical chunk (c & ~7) | ((c & 7) ^ key(r)), key(r) = (r & 3) | ((r >> 3) & 1) << 2:
// the 8 rows a lane group reads together (r = x, x+1, x+2, x+3, x+8, .. x+11) have 8 distinct keys -> conflict-free ds_read_b128.
// GEGLU: steps alternate value / gate blocks of 80 columns; the value step's result waits as packed fp16 in 20 VGPRs.
// =====================================================================================================================
constexpr int V7_KS = V7_K / 32;
constexpr int V7_PIECES = 56, V7_STAGE_BYTES = V7_PIECES * 1024;      // 80 rows x 640 bytes = 50 pieces, padded to 7 per wave

template <bool GEGLU, bool LN>
__global__ __launch_bounds__(512, 2) void gemm7_kernel(const GemmParams p) {
    constexpr int TM = 2, TN = 5;
    __shared__ __attribute__((aligned(16))) char smem7[2 * V7_STAGE_BYTES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool grp1 = wid >= 4;
    const int fr = lane & 15, fq = lane >> 4;
    const int m0 = blockIdx.x * V7_BM, mw = m0 + wid * 32;              // this wave's 32 rows
    const int NS = p.N / V7_NB;                                         // steps (80 W rows each)

    // ---- A fragments: rows mw + 16 i + fr, k = 32 ks + 8 fq .. + 7 (rows past M are clamped; their outputs are never stored)
    // Round 5: requested in the prologue BEHIND the first W pieces and in k-step order, and not waited for there (the prologue's counted wait
    // leaves these 20 loads in flight): the first step's MFMAs start on k-step 0 while the later k-steps of the 164 KB panel are still
    // arriving — before, every workgroup sat through its whole panel load (all 256 at once: ~7 of a 32 us launch) before its first MFMA.
    half8 fa[TM][V7_KS];
    auto load_a = [&]() {
        const half_t* ar[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = mw + i * 16 + fr;
            ar[i] = p.A + (long long)(m < p.M ? m : p.M - 1) * p.lda + fq * 8;
        }
#pragma unroll
        for (int ks = 0; ks < V7_KS; ++ks)
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i][ks] = as_half8(ld16(ar[i] + ks * 32));
    };
    // ---- LayerNorm fold (consumer): (mu, rstd) of my rows from the producer's per-part (sum, sum of squares).  The whole affine part of
    // the epilogue,  v = rstd alpha (acc - mu wsum) + bias,  is folded into the accumulators' START value  bias / (rstd alpha) - mu wsum
    // (set at the head of a step's MFMA phase, which has vector-issue slack), so the epilogue is one multiply by rstd alpha.
    float rs_a[TM], inv_a[TM], mu_a[TM];
    auto ln_fill = [&]() {   // (prologue, behind the first W pieces: its loads are waited for at once — together with those pieces, which the prologue needs anyway)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            rs_a[i] = p.alpha;
            mu_a[i] = 0.f;
            if (LN) {
                const int m = mw + i * 16 + fr;
                float s1 = 0.f, s2 = 0.f;
                if (m < p.M) ln_sum_parts(p.ln_stat + (long long)m * 2, (long long)p.ln_rows * 2, p.ln_parts, s1, s2);
                const float mu = s1 * p.ln_inv_c;
                mu_a[i] = mu;
                rs_a[i] = rsqrtf(fmaxf(s2 * p.ln_inv_c - mu * mu, 0.f) + p.ln_eps) * p.alpha;     // (rows past M: finite garbage, never stored)
            }
            inv_a[i] = 1.0f / rs_a[i];
        }
    };
    auto key = [](int r) { return (r & 3) | (((r >> 3) & 1) << 2); };
    // ---- W loader: piece (wid + 8 i) of a stage, lane l -> LDS byte o = piece * 1024 + 16 l -> row o / 640, physical chunk (o % 640) / 16
    unsigned w_off[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int o = (wid + 8 * i) * 1024 + lane * 16;
        int row = o / 640;
        const int pc = (o - row * 640) >> 4;
        const int lc = (pc & ~7) | ((pc & 7) ^ key(row));
        if (row > V7_NB - 1) row = V7_NB - 1;                           // the 6 padding pieces re-read the last row (never read back)
        w_off[i] = (unsigned)(((long long)row * p.ldw + lc * 8) * 2);
    }
    // piece 50 (the first padding piece, issued by wave 2) carries the step's 80 bias halfs (bytes 51200 ..) and 80 LayerNorm-fold row
    // sums (bytes 51456 ..): the epilogue reads them from LDS instead of waiting on small global loads every step
    const char* aux_ptr = reinterpret_cast<const char*>(g_zero_row);
    int aux_step = 0;
    if (lane < 10 && p.bias_n != nullptr) {
        aux_ptr = reinterpret_cast<const char*>(p.bias_n + lane * 8);
        aux_step = V7_NB * 2;
    } else if (lane >= 16 && lane < 36 && p.ln_wsum != nullptr) {
        aux_ptr = reinterpret_cast<const char*>(p.ln_wsum + (lane - 16) * 4);
        aux_step = V7_NB * 4;
    }
    const char* p7 = wid == 2 ? aux_ptr : reinterpret_cast<const char*>(p.W) + w_off[6];   // every wave's 7th piece, as a per-lane pointer
    const long long step7 = wid == 2 ? (long long)aux_step : (long long)V7_NB * p.ldw * 2;
    // Step order: workgroup b walks the N / 80 steps starting at step j0(b) and wraps, so that the workgroups of an XCD (b, b + 8, ..)
    // do not all ask its L2 for the same W lines at the same moment.  GEGLU rotates by (value, gate) pairs.
    const int j0 = GEGLU ? 2 * (int)((blockIdx.x >> 3) % (unsigned)(NS >> 1)) : (int)((blockIdx.x >> 3) % (unsigned)NS);
    const unsigned smem_base = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)(const __attribute__((address_space(3))) void*)smem7);
    int n_issued = 0;
    auto issue = [&]() {
        int js = j0 + n_issued;
        if (js >= NS) js -= NS;
        const half_t* w_base = p.W + (long long)js * V7_NB * p.ldw;      // wave-uniform: W row block of step js
        const unsigned dst = smem_base + (unsigned)((n_issued & 1) * V7_STAGE_BYTES) + (unsigned)wid * 1024u;
#pragma unroll
        for (int i = 0; i < 6; ++i) glds16s(w_off[i], w_base, dst + (unsigned)(8 * i) * 1024u);
        glds16(reinterpret_cast<const half_t*>(p7 + js * step7), dst + 48u * 1024u);   // per-lane pointer form: wave 2 fetches bias / row sums here
        ++n_issued;
    };
    // fragment read bases: the lane that supplies MFMA index fr reads W row  const(jj) + 8 (fr >> 2) + (fr & 3)  (tiles 0..3) or
    // 64 + (fr & 3) + 8 ((fr >> 2) & 1) + 4 (fr >> 3)  (tile 4); both have key (fr & 3) | ((fr >> 2) & 1) << 2
    const int kf = (fr & 3) | (((fr >> 2) & 1) << 2);
    const char* rdP = smem7 + (8 * (fr >> 2) + (fr & 3)) * 640;          // + (32 (jj >> 1) + 4 (jj & 1)) * 640 per tile
    const char* rdL = smem7 + (64 + (fr & 3) + 8 * ((fr >> 2) & 1) + 4 * (fr >> 3)) * 640;
    int chunk_lo[2];                                                     // (fq ^ key) and ((4 + fq) ^ key): the low 3 bits for even / odd ks
    chunk_lo[0] = ((fq ^ kf) & 7) << 4;
    chunk_lo[1] = (((4 + fq) ^ kf) & 7) << 4;
    // ---- epilogue addressing (accumulator layout): rows mw + 16 i + fr; tile pair P -> columns 32 P + 8 fq .. + 7, tile 4 -> 64 + c8 .. + 3
    const int c8 = 64 + 8 * (fq & 1) + 4 * (fq >> 1);
    int o_c[TM], o_r[TM];                                                // element offsets relative to (row mw, column n_out)
    bool row_ok[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = mw + 16 * i + fr;
        row_ok[i] = m < p.M;
        o_c[i] = (16 * i + fr) * p.ldc;
        o_r[i] = ((row_ok[i] ? m : p.M - 1) - mw) * p.ldr;
    }

    f32x4 acc[TM][TN];
    unsigned vh[GEGLU ? TM * TN * 2 : 1];                               // GEGLU: the finished value block, packed fp16, waits for its gate block

    // ---- one MFMA phase: this step's 80 W rows x K = 320 against my A fragments
    auto mfma_step = [&](int stage) {
        const char* TP = rdP + stage * V7_STAGE_BYTES;
        const char* TL = rdL + stage * V7_STAGE_BYTES;
        auto rd = [&](int j, int ks) {
            const int co = ((ks >> 1) << 7) + chunk_lo[ks & 1];
            return as_half8(ld16(j < 4 ? TP + (32 * (j >> 1) + 4 * (j & 1)) * 640 + co : TL + co));
        };
        half8 fb[2][TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[0][j] = rd(j, 0);
        {   // accumulators start at  bias / (rstd alpha) - mu wsum  of my columns (tile jj < 4 -> 32 (jj >> 1) + 8 fq + 4 (jj & 1) .. + 3, tile 4 -> c8 .. + 3)
            const char* aux = smem7 + stage * V7_STAGE_BYTES + 50 * 1024;   // this step's bias (halfs; zeros when there is none) and, 256 bytes on, LayerNorm-fold row sums (floats)
            const uint4 b01 = ld16(aux + (8 * fq) * 2), b23 = ld16(aux + (32 + 8 * fq) * 2);
            const uint2 b4 = *reinterpret_cast<const uint2*>(aux + c8 * 2);
            const uint2 bt[TN] = {make_uint2(b01.x, b01.y), make_uint2(b01.z, b01.w), make_uint2(b23.x, b23.y), make_uint2(b23.z, b23.w), b4};
#pragma unroll
            for (int jj = 0; jj < TN; ++jj) {
                const half4 bh = __builtin_bit_cast(half4, bt[jj]);
                f32x4 bf, ws = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 4; ++r) bf[r] = (float)bh[r];
                if (LN) ws = *reinterpret_cast<const f32x4*>(aux + 256 + (jj < 4 ? 32 * (jj >> 1) + 8 * fq + 4 * (jj & 1) : c8) * 4);
#pragma unroll
                for (int i = 0; i < TM; ++i) acc[i][jj] = LN ? bf * inv_a[i] - mu_a[i] * ws : bf * inv_a[i];
            }
        }
#pragma unroll
        for (int ks = 0; ks < V7_KS; ++ks) {
            if (ks + 1 < V7_KS) {
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[(ks + 1) & 1][j] = rd(j, ks + 1);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[ks & 1][j], fa[i][ks], acc[i][j], 0, 0, 0);
        }
    };
    // group 0: its share of step j+1 (stage free since group 1's MFMA j-1); group 1: its share of step j+2 (stage free since its own MFMA j)
    auto issue_next = [&](int j) {
        if (!grp1) {
            if (j + 1 < NS) issue();
        } else {
            if (j + 2 < NS) issue();
        }
    };
    const bool full_tile = m0 + V7_BM <= p.M;
    // ---- one epilogue phase: step j (columns n_out .. n_out + 79 of the output; W / bias rows nb .. nb + 79); returns the number of
    // store instructions it left as the youngest vector-memory operations of this wave.  Branch-free, every LDS / global read of a
    // phase issued as one batch: tile-by-tile read-wait-convert chains measured at twice the MFMA phase they are meant to hide behind.
    auto epilogue = [&](int it_, int j) -> int {                         // it_: position in this workgroup's walk (stage parity), j: the step
        const int nb = j * V7_NB;                                        // row block of W / bias / wsum
        const int n_out = GEGLU ? (j >> 1) * V7_NB : nb;
        // The W pieces of a later step go out FIRST: they then have the whole epilogue to land, and the closing wait of the interval still
        // finds them older than this epilogue's output stores.  (The stage they overwrite is free: see issue_next; the bias / row-sum
        // piece this epilogue reads belongs to wave 2's share, which group 0 re-issues one interval later.)
        issue_next(it_);
        const bool has_res = !GEGLU && p.R != nullptr;
        uint4 r16[TM][2];                                                // residual, requested now, added after the activation
        uint2 r8[TM];
        if (has_res) {                                                   // (uniform; rows past M read row M - 1, their results are never stored; GEGLU: no residual here)
            const half_t* Rb = p.R + (long long)mw * p.ldr + n_out;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                r16[i][0] = ld16(Rb + o_r[i] + 8 * fq);
                r16[i][1] = ld16(Rb + o_r[i] + 32 + 8 * fq);
                r8[i] = *reinterpret_cast<const uint2*>(Rb + o_r[i] + c8);
            }
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                r16[i][0] = r16[i][1] = zero16();
                r8[i] = make_uint2(0u, 0u);
            }
        }
        auto affine = [&](int i, int jj) { return acc[i][jj] * rs_a[i]; };   // (bias and the LayerNorm shift went into the accumulators' start value)
        if (GEGLU && (j & 1) == 0) {                                     // value block: park it (one uniform branch, not one per tile:
#pragma unroll                                                           //  the gate step below must stay ONE basic block, see there)
            for (int jj = 0; jj < TN; ++jj)
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const f32x4 v = affine(i, jj);
                    vh[(i * TN + jj) * 2] = pk2h(v[0], v[1]);
                    vh[(i * TN + jj) * 2 + 1] = pk2h(v[2], v[3]);
                }
            return 0;
        }
        uint2 h[TM][TN];
#pragma unroll
        for (int jj = 0; jj < TN; ++jj) {
            f32x4 v[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) v[i] = affine(i, jj);
            if (GEGLU) {                                                 // gate step: out = value * gelu(gate), 8 at a time (common.h: geglu8_staged)
                const unsigned aw[4] = {vh[jj * 2], vh[jj * 2 + 1], vh[(TN + jj) * 2], vh[(TN + jj) * 2 + 1]};
                const f32x2 gp[4] = {{v[0][0], v[0][1]}, {v[0][2], v[0][3]}, {v[1][0], v[1][1]}, {v[1][2], v[1][3]}};
                unsigned ow[4];
                geglu8_staged(aw, gp, ow);
                h[0][jj] = make_uint2(ow[0], ow[1]);
                h[1][jj] = make_uint2(ow[2], ow[3]);
            } else {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    h[i][jj].x = pk2h(v[i][0], v[i][1]);
                    h[i][jj].y = pk2h(v[i][2], v[i][3]);
                }
            }
        }
        // Vector-memory operations retire in order: the residual is waited for with the builtin (which hipcc's waitcnt pass models: it
        // then adds no wait of its own), unconditionally (under `if (R)` the model still holds the loads outstanding on the merged path
        // and parks its own waits further down).  The W pieces issued above are older and retire with it — they have had the whole
        // finish to land; the output stores below stay the youngest operations, so the interval's closing wait can leave them in flight.
        if (!GEGLU) __builtin_amdgcn_s_waitcnt(0x0F70);                  // vmcnt(0)
        uint4 o16[TM][2];
        uint2 o8[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            o16[i][0] = make_uint4(h[i][0].x, h[i][0].y, h[i][1].x, h[i][1].y);
            o16[i][1] = make_uint4(h[i][2].x, h[i][2].y, h[i][3].x, h[i][3].y);
            o8[i] = h[i][4];
            if (has_res) {                                               // packed fp16 adds: the finished tile is fp16 already
                o16[i][0] = add8h(o16[i][0], r16[i][0]);
                o16[i][1] = add8h(o16[i][1], r16[i][1]);
                const uint4 t = add8h(make_uint4(o8[i].x, o8[i].y, 0u, 0u), make_uint4(r8[i].x, r8[i].y, 0u, 0u));
                o8[i] = make_uint2(t.x, t.y);
            }
        }
        if (!GEGLU && p.stat_out != nullptr) {   // LN-fold producer: (sum, sum of squares) of the fp16 results per row: 20 columns per lane, then across the 4 lanes of a row
            const half2v one2 = {(half_t)1.0f, (half_t)1.0f};
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const unsigned w[10] = {o16[i][0].x, o16[i][0].y, o16[i][0].z, o16[i][0].w, o16[i][1].x, o16[i][1].y, o16[i][1].z, o16[i][1].w, o8[i].x, o8[i].y};
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int e = 0; e < 10; ++e) {
                    const half2v hv = __builtin_bit_cast(half2v, w[e]);
                    s1 = __builtin_amdgcn_fdot2(hv, one2, s1, false);
                    s2 = __builtin_amdgcn_fdot2(hv, hv, s2, false);
                }
                // lanes fr, fr + 16, fr + 32, fr + 48 hold one row: two swap-and-add steps leave the row total in all four
                auto a1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(s1), __float_as_uint(s1), false, false);
                auto a2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(s2), __float_as_uint(s2), false, false);
                s1 = __uint_as_float(a1[0]) + __uint_as_float(a1[1]);
                s2 = __uint_as_float(a2[0]) + __uint_as_float(a2[1]);
                a1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(s1), __float_as_uint(s1), false, false);
                a2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(s2), __float_as_uint(s2), false, false);
                s1 = __uint_as_float(a1[0]) + __uint_as_float(a1[1]);
                s2 = __uint_as_float(a2[0]) + __uint_as_float(a2[1]);
                if (fq == 0 && row_ok[i]) *reinterpret_cast<float2*>(p.stat_out + ((long long)j * p.M + mw + 16 * i + fr) * 2) = make_float2(s1, s2);
            }
        }
        half_t* Cb = p.C + (long long)mw * p.ldc + n_out;
        if (full_tile) {                                                 // exactly 6 store instructions: the closing wait leaves them in flight
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                st16(Cb + o_c[i] + 8 * fq, o16[i][0]);
                st16(Cb + o_c[i] + 32 + 8 * fq, o16[i][1]);
                *reinterpret_cast<uint2*>(Cb + o_c[i] + c8) = o8[i];
            }
            return 6;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
            if (row_ok[i]) {
                st16(Cb + o_c[i] + 8 * fq, o16[i][0]);
                st16(Cb + o_c[i] + 32 + 8 * fq, o16[i][1]);
                *reinterpret_cast<uint2*>(Cb + o_c[i] + c8) = o8[i];
            }
        return 0;
    };
    auto end_interval = [&](int keep_stores) {
        if (keep_stores == 6) wait_vmcnt<6>();
        else wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
    };

    // ---- prologue: step 0 (everyone) and group 1's share of step 1 in flight; step 0 landed and published; group 1 one barrier behind
    issue();
    if (grp1 && NS > 1) issue();
    ln_fill();
    load_a();
    // every W piece issued above (and the LayerNorm statistics) is older than the TM * V7_KS loads of the A panel: this leaves exactly those in flight
    wait_vmcnt<TM * V7_KS>();
    __builtin_amdgcn_s_barrier();
    if (grp1) __builtin_amdgcn_s_barrier();
    int st = 0;
    for (int it_ = 0; it_ < NS; ++it_) {
        int j = j0 + it_;
        if (j >= NS) j -= NS;
        mfma_step(it_ & 1);
        end_interval(st);                                                // my DMA share is older than the last epilogue's stores: those may stay in flight
        // The epilogue runs at raised priority: on this chip a VALU stream and an MFMA stream of the two waves of a SIMD take the SUM of
        // their times when the MFMA wave has (equal or higher) priority — it holds the vector issue port while the matrix pipe is busy —
        // and the MAX when the VALU wave has priority (tools/micro/coexec.hip, profiles/README.md).
        __builtin_amdgcn_s_setprio(2);
        st = epilogue(it_, j);
        __builtin_amdgcn_s_setprio(0);
        end_interval(st);
    }
    if (!grp1) __builtin_amdgcn_s_barrier();                            // group 0 waits out group 1's last epilogue: every wave ran 2 NS + 2 barriers
}

}  // namespace

void gemm7_launch(const GemmParams& p, const GemmPlan& pl, dim3 grid, hipStream_t s) {
    if (pl.geglu && pl.ln) hipLaunchKernelGGL((gemm7_kernel<true, true>), grid, dim3(512), 0, s, p);
    else if (pl.geglu) hipLaunchKernelGGL((gemm7_kernel<true, false>), grid, dim3(512), 0, s, p);
    else if (pl.ln) hipLaunchKernelGGL((gemm7_kernel<false, true>), grid, dim3(512), 0, s, p);
    else hipLaunchKernelGGL((gemm7_kernel<false, false>), grid, dim3(512), 0, s, p);
}
