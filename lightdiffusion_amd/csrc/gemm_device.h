// MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950.
//
// Tile: BM x BN x 64, 4 waves (2x2), each wave (BM/2)x(BN/2) as 16x16x32 f16 MFMA tiles.
// Staging: global -> LDS by LDS-DMA (global_load_lds_dwordx4) into a ring of slabs, ONE barrier per 64-wide K slab.
// LDS tiles are [rows][64 halfs] with the 16-byte chunk index XOR-swizzled by (row & 7) on the DMA source address
// and on the fragment read: ds_read_b128 fragment reads are bank-conflict free (cdna guide T2, rule 21).
// MFMA operands are swapped (a := W fragment, b := A fragment) so that each lane ends up with 4 consecutive
// output channels of one output row -> 8-byte LDS writes / 16-byte split-K stores in the epilogue.
// Epilogue: accumulators -> fp16 tile in LDS -> row-wise 16-byte coalesced stores with the fused bias /
// time-embedding broadcast / SiLU / GEGLU / residual.
//
// This header: the device helpers every kernel family shares (internal to the gemm*.hip / conv6.hip sources).
#pragma once
#include "gemm.h"

namespace {

constexpr int BK = 64;
constexpr int NT = 256;

__device__ __forceinline__ void epilogue_store8(const GemmParams& p, int z, int m, int n_out, int n_bias, float (&v)[8]) {
    // v already holds alpha*acc (and, for GEGLU, the gated product with biases applied).  The operands are requested together, then
    // consumed: one memory latency instead of one per operand.
    const bool hb = p.bias_n != nullptr && p.act != 2, hv = p.rowvec != nullptr, hr = p.R != nullptr;
    const uint4 rb = hb ? ld16(p.bias_n + n_bias) : zero16();
    const uint4 rv = hv ? ld16(p.rowvec + (long long)(m / p.rows_per_vec) * p.ldrv + n_out) : zero16();
    const uint4 rr = hr ? ld16(p.R + (long long)z * p.sR + (long long)m * p.ldr + n_out) : zero16();
    const float bm = p.bias_m != nullptr ? (float)p.bias_m[m] : 0.f;
    float b[8], e[8], r[8];
    unpack8(rb, b);
    unpack8(rv, e);
    unpack8(rr, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] + b[j] + bm + e[j];
    if (p.act == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = silu_f(v[j]);
    } else if (p.act == 3) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = quick_gelu_f(v[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += r[j];
    st16(p.C + (long long)z * p.sC + (long long)m * p.ldc + n_out, pack8(v));
}

// Tile epilogue: the fp16 C tile sits in LDS; every thread owns EIT 16-byte chunks of it.  All global operands of the
// fused epilogue (bias, time-embedding row vector, residual) are loaded FIRST for every chunk, then consumed: the
// loads overlap each other instead of paying one full memory latency per chunk (the accumulators are dead here, so
// the registers are free).
// Round 5 (profiles/r05_gemm3_ablations.txt: at 16384 x 640 x 640 the tile epilogue took 8.7 of 23.5 us, 4.6 of them with
// neither residual loads nor stores): the epilogue no longer starts a memory round trip of its own.  `bias_s` = this tile's BN bias halfs,
// staged in LDS by the kernel's prologue (zeros when there is no bias); `pre` = the residual chunks of the first group of the plain interior
// path, requested by the caller BEFORE the tile is staged in LDS (epi_prefetch_residual); the second group's are requested before the first
// group is consumed.
template <int BM, int BN>
struct EpiPre {
    static constexpr int CPR = BN / 8, EIT = (BM * CPR + NT - 1) / NT, GRP = EIT > 5 ? (EIT + 1) / 2 : EIT;
    uint4 r[GRP];
    bool fast;        // the plain interior path runs (workgroup-uniform)
    bool bias_done;   // the bias is already in the staged tile (accumulator start value / LayerNorm-fold finish): the epilogue adds none
};
template <int BM, int BN>
__device__ __forceinline__ EpiPre<BM, BN> epi_prefetch_residual(const GemmParams& p, int z, int m0, int n0, int tid, bool bias_done) {
    EpiPre<BM, BN> e;
    e.bias_done = bias_done;
    constexpr int CPR = EpiPre<BM, BN>::CPR, GRP = EpiPre<BM, BN>::GRP;
    e.fast = (BM * CPR) % NT == 0 && m0 + BM <= p.M && n0 + BN <= p.N && p.act == 0 && p.bias_m == nullptr && bias_done;
#pragma unroll
    for (int k = 0; k < GRP; ++k) e.r[k] = zero16();
    if (e.fast && p.R != nullptr) {
        const half_t* Rb = p.R + (long long)z * p.sR + (long long)m0 * p.ldr + n0;
#pragma unroll
        for (int k = 0; k < GRP; ++k) {
            const int q = tid + k * NT;
            const int row = q / CPR, cc = q - row * CPR;
            e.r[k] = ld16(Rb + (long long)row * p.ldr + cc * 8);
        }
    }
    return e;
}

template <int BM, int BN>
__device__ __forceinline__ void epilogue_tile(const GemmParams& p, const half_t* Cs, int z, int m0, int n0, int tid, float* lds_scratch, const half_t* bias_s,
                                              const EpiPre<BM, BN>& pre) {
    constexpr int CLD = BN + 8;
    if (p.act == 2) {
        constexpr int CPR = BN / 16;
        constexpr int EIT = (BM * CPR + NT - 1) / NT;
        if ((BM * CPR) % NT == 0 && m0 + BM <= p.M && n0 + BN <= p.N && pre.bias_done) {
            // interior tile: branch-free, batched reads, stage-by-stage GELUs (common.h) on the packed value chunk; the value / gate biases
            // are in the staged tile already (accumulator start value / LayerNorm-fold finish), the residual is a packed fp16 add
            half_t* Cb = p.C + (long long)z * p.sC + (long long)m0 * p.ldc + n0 / 2;
            const bool hr = p.R != nullptr;
            const half_t* Rb = hr ? p.R + (long long)z * p.sR + (long long)m0 * p.ldr + n0 / 2 : nullptr;
            uint4 rres[EIT], ca[EIT], cg[EIT];
#pragma unroll
            for (int it = 0; it < EIT; ++it) {
                const int q = tid + it * NT;
                const int row = q / CPR, cc = q - row * CPR;
                rres[it] = hr ? ld16(Rb + (long long)row * p.ldr + cc * 8) : zero16();
                ca[it] = ld16(Cs + row * CLD + cc * 8);
                cg[it] = ld16(Cs + row * CLD + BN / 2 + cc * 8);
            }
#pragma unroll
            for (int it = 0; it < EIT; ++it) {
                const int q = tid + it * NT;
                const int row = q / CPR, cc = q - row * CPR;
                float g[8];
                unpack8(cg[it], g);
                const unsigned aw[4] = {ca[it].x, ca[it].y, ca[it].z, ca[it].w};
                const f32x2 gp[4] = {{g[0], g[1]}, {g[2], g[3]}, {g[4], g[5]}, {g[6], g[7]}};
                unsigned ow[4];
                geglu8_staged(aw, gp, ow);
                uint4 packed = make_uint4(ow[0], ow[1], ow[2], ow[3]);
                if (hr) packed = add8h(packed, rres[it]);
                st16(Cb + (long long)row * p.ldc + cc * 8, packed);
            }
            return;
        }
        uint4 rba[EIT], rbg[EIT], rres[EIT];
#pragma unroll
        for (int it = 0; it < EIT; ++it) {
            const int q = tid + it * NT;
            const int row = q / CPR, cc = q - row * CPR;
            const int m = m0 + row, nv = n0 + cc * 8, ng = nv + BN / 2;
            const bool ok = q < BM * CPR && m < p.M && ng < p.N;
            rba[it] = (ok && !pre.bias_done) ? ld16(p.bias_n + nv) : zero16();
            rbg[it] = (ok && !pre.bias_done) ? ld16(p.bias_n + ng) : zero16();
            rres[it] = (ok && p.R != nullptr) ? ld16(p.R + (long long)z * p.sR + (long long)m * p.ldr + n0 / 2 + cc * 8) : zero16();
        }
#pragma unroll
        for (int it = 0; it < EIT; ++it) {
            const int q = tid + it * NT;
            const int row = q / CPR, cc = q - row * CPR;
            const int m = m0 + row, ng = n0 + cc * 8 + BN / 2;
            if (q < BM * CPR && m < p.M && ng < p.N) {
                float a[8], g[8], ba[8], bg[8], r[8];
                unpack8(ld16(Cs + row * CLD + cc * 8), a);
                unpack8(ld16(Cs + row * CLD + BN / 2 + cc * 8), g);
                unpack8(rba[it], ba);
                unpack8(rbg[it], bg);
                unpack8(rres[it], r);
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = (a[j] + ba[j]) * gelu_f(g[j] + bg[j]) + r[j];
                st16(p.C + (long long)z * p.sC + (long long)m * p.ldc + n0 / 2 + cc * 8, pack8(a));
            }
        }
    } else {
        constexpr int CPR = BN / 8;
        constexpr int EIT = (BM * CPR + NT - 1) / NT;
        constexpr int GRP = EIT > 5 ? (EIT + 1) / 2 : EIT;   // two passes for the big tiles: bounds the live registers
        const bool hb = p.bias_n != nullptr && !pre.bias_done, hv = p.rowvec != nullptr, hr = p.R != nullptr;
        // Interior tiles without an activation: a branch-free path in PACKED fp16 (round 5; profiles/r05_gemm3_ablations.txt: with neither residual loads
        // nor stores the fp32 form of this path still took 4.6 of 23.5 us at 16384 x 640 x 640 — ~70 vector instructions per 16-byte chunk,
        // two workgroups per CU).  The bias is in the staged tile already (accumulator start value, or the LayerNorm-fold finish), so a chunk
        // is: tile chunk (+ time-embedding row) (+ residual) by v_pk_add_f16 — the sum of two fp16 values is exact in fp32, so ONE packed add
        // rounds exactly like the fp32 form did; a chunk that takes both the row vector and the residual is rounded once more (two packed
        // adds: round(round(tile + row) + residual), on top of the one rounding of acc * alpha + bias) — and the LayerNorm-fold row
        // statistics by v_dot2_f32_f16 on the packed result.
        if (pre.fast) {
            static_assert(GRP == EpiPre<BM, BN>::GRP, "group size");
            half_t* Cb = p.C + (long long)z * p.sC + (long long)m0 * p.ldc + n0;
            const half_t* Rb = hr ? p.R + (long long)z * p.sR + (long long)m0 * p.ldr + n0 : nullptr;
            uint4 rnext[GRP];                                   // the residual chunks of the group after the one being consumed
#pragma unroll
            for (int k = 0; k < GRP; ++k) rnext[k] = pre.r[k];
#pragma unroll
            for (int g0 = 0; g0 < EIT; g0 += GRP) {
                uint4 rv[GRP], rres[GRP], cv[GRP];
#pragma unroll
                for (int k = 0; k < GRP; ++k) rres[k] = rnext[k];
#pragma unroll
                for (int k = 0; k < GRP; ++k) {                 // next group's residual: in flight while this group is consumed
                    if (g0 + GRP + k >= EIT) continue;
                    const int q = tid + (g0 + GRP + k) * NT;
                    const int row = q / CPR, cc = q - row * CPR;
                    rnext[k] = hr ? ld16(Rb + (long long)row * p.ldr + cc * 8) : zero16();
                }
#pragma unroll
                for (int k = 0; k < GRP; ++k) {
                    if (g0 + k >= EIT) continue;
                    const int q = tid + (g0 + k) * NT;
                    const int row = q / CPR, cc = q - row * CPR;
                    rv[k] = hv ? ld16(p.rowvec + (long long)((m0 + row) / p.rows_per_vec) * p.ldrv + n0 + cc * 8) : zero16();
                    cv[k] = ld16(Cs + row * CLD + cc * 8);
                }
#pragma unroll
                for (int k = 0; k < GRP; ++k) {
                    if (g0 + k >= EIT) continue;
                    const int q = tid + (g0 + k) * NT;
                    const int row = q / CPR, cc = q - row * CPR;
                    uint4 packed = cv[k];
                    if (hv) packed = add8h(packed, rv[k]);
                    if (hr) packed = add8h(packed, rres[k]);
                    st16(Cb + (long long)row * p.ldc + cc * 8, packed);
                    if (lds_scratch != nullptr) {   // LN-fold producer: row statistics of what was actually stored (the fp16 values)
                        const half2v one2 = {(half_t)1.f, (half_t)1.f};
                        const half2v h0 = __builtin_bit_cast(half2v, packed.x), h1 = __builtin_bit_cast(half2v, packed.y);
                        const half2v h2 = __builtin_bit_cast(half2v, packed.z), h3 = __builtin_bit_cast(half2v, packed.w);
                        float s1 = __builtin_amdgcn_fdot2(h1, one2, __builtin_amdgcn_fdot2(h0, one2, 0.f, false), false);
                        float s2 = __builtin_amdgcn_fdot2(h1, h1, __builtin_amdgcn_fdot2(h0, h0, 0.f, false), false);
                        s1 = __builtin_amdgcn_fdot2(h3, one2, __builtin_amdgcn_fdot2(h2, one2, s1, false), false);
                        s2 = __builtin_amdgcn_fdot2(h3, h3, __builtin_amdgcn_fdot2(h2, h2, s2, false), false);
                        *reinterpret_cast<float2*>(lds_scratch + q * 2) = make_float2(s1, s2);
                    }
                }
            }
            if (lds_scratch != nullptr) {   // one owner per row sums its CPR chunk partials in chunk order (bitwise reproducible)
                __syncthreads();
                if (tid < BM) {
                    float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
                    for (int c = 0; c < CPR; ++c) {
                        const float2 t = *reinterpret_cast<const float2*>(lds_scratch + (tid * CPR + c) * 2);
                        s1 += t.x;
                        s2 += t.y;
                    }
                    *reinterpret_cast<float2*>(p.stat_out + ((long long)(n0 / BN) * p.M + m0 + tid) * 2) = make_float2(s1, s2);
                }
            }
            return;
        }
#pragma unroll
        for (int g0 = 0; g0 < EIT; g0 += GRP) {
            uint4 rb[GRP], rv[GRP], rres[GRP];
#pragma unroll
            for (int k = 0; k < GRP; ++k) {
                const int q = tid + (g0 + k) * NT;
                const int row = q / CPR, cc = q - row * CPR;
                const int m = m0 + row, n = n0 + cc * 8;
                const bool ok = (g0 + k) < EIT && q < BM * CPR && m < p.M && n < p.N;
                rb[k] = (ok && hb) ? ld16(p.bias_n + n) : zero16();
                rv[k] = (ok && hv) ? ld16(p.rowvec + (long long)(m / p.rows_per_vec) * p.ldrv + n) : zero16();
                rres[k] = (ok && hr) ? ld16(p.R + (long long)z * p.sR + (long long)m * p.ldr + n) : zero16();
            }
#pragma unroll
            for (int k = 0; k < GRP; ++k) {
                const int q = tid + (g0 + k) * NT;
                const int row = q / CPR, cc = q - row * CPR;
                const int m = m0 + row, n = n0 + cc * 8;
                if ((g0 + k) < EIT && q < BM * CPR && m < p.M && n < p.N) {
                    float v[8], b[8], e[8], r[8];
                    unpack8(ld16(Cs + row * CLD + cc * 8), v);
                    unpack8(rb[k], b);
                    unpack8(rv[k], e);
                    unpack8(rres[k], r);
                    const float bm = p.bias_m != nullptr ? (float)p.bias_m[m] : 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float t = v[j] + b[j] + bm + e[j];
                        if (p.act == 1) t = silu_tile_f(t);
                        else if (p.act == 3) t = quick_gelu_tile_f(t);
                        v[j] = t + r[j];
                    }
                    const uint4 packed = pack8(v);
                    st16(p.C + (long long)z * p.sC + (long long)m * p.ldc + n, packed);
                    if (lds_scratch != nullptr) {   // LN-fold producer: row statistics of what was actually stored (the fp16 values)
                        float f[8];
                        unpack8(packed, f);
                        float s1 = 0.f, s2 = 0.f;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            s1 += f[j];
                            s2 += f[j] * f[j];
                        }
                        lds_scratch[q * 2] = s1;
                        lds_scratch[q * 2 + 1] = s2;
                    }
                } else if (lds_scratch != nullptr && (g0 + k) < EIT && q < BM * CPR) {
                    lds_scratch[q * 2] = 0.f;
                    lds_scratch[q * 2 + 1] = 0.f;
                }
            }
        }
        if (lds_scratch != nullptr) {   // one owner per row sums its CPR chunk partials in chunk order (bitwise reproducible)
            __syncthreads();
            if (tid < BM && m0 + tid < p.M) {
                float s1 = 0.f, s2 = 0.f;
                for (int c = 0; c < CPR; ++c) {
                    s1 += lds_scratch[(tid * CPR + c) * 2];
                    s2 += lds_scratch[(tid * CPR + c) * 2 + 1];
                }
                float* o = p.stat_out + ((long long)(n0 / BN) * p.M + m0 + tid) * 2;
                o[0] = s1;
                o[1] = s2;
            }
        }
    }
}

// ---- LN fold, consumer side (v3 / v4).  ln_prepare: one thread per LN row of the tile finishes (mu, rstd) from the producer's
// per-N-tile partials, in part order, into LDS; ln_apply: acc <- rstd * (acc - mu * wsum) in fp32, before the tile is rounded to fp16.
// (sum, sum of squares) of one row over the producer's parts, in part order; the loads go out four parts at a time (one part after the
// other is one L2 round trip each — 8 in a row at C = 1280 — in the prologue of every consumer launch)
__device__ __forceinline__ void ln_sum_parts(const float* q, long long stride, int parts, float& s1, float& s2) {
    int t = 0;
    for (; t + 4 <= parts; t += 4) {
        float2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float2*>(q + (t + u) * stride);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s1 += v[u].x;
            s2 += v[u].y;
        }
    }
    for (; t < parts; ++t) {
        const float2 v = *reinterpret_cast<const float2*>(q + t * stride);
        s1 += v.x;
        s2 += v.y;
    }
}

template <int BM, int BN>
__device__ __forceinline__ void ln_prepare(const GemmParams& p, float* ln_mu, float* ln_rs, int z, int m0, int n0, int tid) {
    const int cnt = p.ln_swapped ? BN : BM;
    if (tid >= cnt) return;
    const bool ok = p.ln_swapped ? (n0 + tid < p.n_valid) : (m0 + tid < p.M);
    const long long row = p.ln_swapped ? (long long)z * p.ln_zrows + n0 + tid : (long long)m0 + tid;
    float s1 = 0.f, s2 = 0.f;
    if (ok) ln_sum_parts(p.ln_stat + row * 2, (long long)p.ln_rows * 2, p.ln_parts, s1, s2);
    const float mu = s1 * p.ln_inv_c;
    ln_mu[tid] = mu;
    // rows / columns beyond the problem get rstd = 0: their (never stored, or padding) outputs stay finite — a V^T padding column
    // scaled by rsqrt(eps) could overflow fp16 to inf, and the attention kernel multiplies it by P = 0
    ln_rs[tid] = ok ? rsqrtf(fmaxf(s2 * p.ln_inv_c - mu * mu, 0.f) + p.ln_eps) : 0.f;
}

template <int TM, int TN>
__device__ __forceinline__ void ln_apply(const GemmParams& p, f32x4 (&acc)[TM][TN], const float* ln_mu, const float* ln_rs, int m0, int n0, int wm0,
                                         int wn0, int fr, int fq, const float* wsum_s, const half_t* bias_s, bool add_bias) {
    if (!p.ln_swapped) {
        f32x4 ws[TN], bj[TN];  // this tile's row sums and (add_bias: act == 0, the epilogue then adds none) its bias / alpha, staged in LDS by the kernel's prologue
        const float inv_alpha = 1.0f / p.alpha;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            ws[j] = *reinterpret_cast<const f32x4*>(wsum_s + wn0 + j * 16 + fq * 4);
            const half4 bh = *reinterpret_cast<const half4*>(bias_s + wn0 + j * 16 + fq * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) bj[j][r] = add_bias ? (float)bh[r] * inv_alpha : 0.f;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float mu = ln_mu[wm0 + i * 16 + fr], rs = ln_rs[wm0 + i * 16 + fr];
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = (acc[i][j] - mu * ws[j]) * rs + bj[j];
        }
    } else {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm0 + i * 16 + fr;
            const float wsm = m < p.M ? p.ln_wsum[m] : 0.f;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const f32x4 mu4 = *reinterpret_cast<const f32x4*>(ln_mu + wn0 + j * 16 + fq * 4);
                const f32x4 rs4 = *reinterpret_cast<const f32x4*>(ln_rs + wn0 + j * 16 + fq * 4);
                acc[i][j] = (acc[i][j] - mu4 * wsm) * rs4;
            }
        }
    }
}

__device__ uint4 g_zero_row[4096];  // 64 KB of zeros: conv taps outside the image read it, stepped through like real data (one
                                    // tap's channel run at a time, so it only has to cover max(C1, C2) <= 32768 halfs)
                                    // (the library is built without relocatable device code, so every object whose kernels read the page
                                    // gets a copy of its own — five family objects, 320 KB of device memory; only zeros are ever read from it)

// Prologue staging of a tile's per-column epilogue operands into LDS: bias_s[BN] halfs (zeros without a bias) and, for a LayerNorm-fold
// consumer, wsum_s[BN] floats (zeros beyond N).  epi_stage_load issues the two loads as untracked asm (always a load, from a page of zeros
// where there is nothing to fetch) BEFORE the first LDS-DMA of the wave, so they are its oldest vector-memory operations;
// EPI_STAGE_WAIT(KEEP, ..) waits with a COUNTED vmcnt that leaves the KEEP LDS-DMA instructions issued since in flight (KEEP = 0 where the
// wave issues none, or fewer than the full prologue) and names the destination registers as operands of that wait (DESIGN "hipcc traps" (c));
// epi_stage_store writes them to LDS; the slab loop's barriers publish them long before the epilogue reads them.
// (the loaded values live in two f32x4 locals of the KERNEL — b: 8 bias halfs as a bit pattern, w: 4 row sums — so that the counted wait
// can name them as read-write operands: nothing that copies or spills them can be scheduled between a load and the wait)
template <int BN>
__device__ __forceinline__ void epi_stage_load(const GemmParams& p, int n0, int t, f32x4& b, f32x4& w) {   // t: thread index inside the loading role (>= BN / 4 threads)
    const char* zp = reinterpret_cast<const char*>(g_zero_row);
    const char* bp = (t < BN / 8 && p.bias_n != nullptr && n0 + t * 8 < p.N) ? reinterpret_cast<const char*>(p.bias_n + n0 + t * 8) : zp;
    const char* wp = (t < BN / 4 && p.ln_wsum != nullptr && !p.ln_swapped && n0 + t * 4 < p.N) ? reinterpret_cast<const char*>(p.ln_wsum + n0 + t * 4) : zp;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(b) : "v"(bp) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(w) : "v"(wp) : "memory");
}
#define EPI_STAGE_WAIT(KEEP, b, w) asm volatile("s_waitcnt vmcnt(%2)" : "+v"(b), "+v"(w) : "n"(KEEP) : "memory")
template <int BN>
__device__ __forceinline__ void epi_stage_store(const f32x4& b, const f32x4& w, half_t* bias_s, float* wsum_s, int t) {   // (behind EPI_STAGE_WAIT)
    if (t < BN / 8) *reinterpret_cast<f32x4*>(bias_s + t * 8) = b;
    if (t < BN / 4) *reinterpret_cast<f32x4*>(wsum_s + t * 4) = w;
}

__device__ __forceinline__ void glds16s(unsigned voff, const half_t* sbase, unsigned lds_base) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_base)
        : "memory");
}

}  // namespace
