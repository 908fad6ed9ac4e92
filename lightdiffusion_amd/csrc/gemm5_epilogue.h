// The epilogues of the 256 x 320 skeleton, shared by gemm5_kernel (gemm5.hip) and conv6_kernel (conv6.hip), and its LDS layout constants.
#pragma once
#include <type_traits>

#include "gemm_device.h"
#include "gemm_kernels.h"

namespace {

constexpr int V5_NST = 4;
constexpr int V5_A_BYTES = V5_BM * 64, V5_STAGE_BYTES = (V5_BM + V5_BN) * 64;
constexpr int V5_EPI_LD = 164;                       // halfs per staged row: 320 data bytes + 8 pad (ds_write_b64 conflict-free)
constexpr int V5_EPI_BYTES = 16 * V5_EPI_LD * 2;     // one 16-row strip of a wave
constexpr int V5_SWZ = 0x78;                         // g[x] = (0x78 >> 2x) & 3 = {0, 2, 3, 1}

// one 16-row x 160-column strip of a wave's tile: staged fp16 values -> fused epilogue -> 16-byte global stores
// EPI (compile time: one epilogue per kernel instantiation keeps its code and its register demand small — with all three inlined
// into one kernel hipcc spilled 160 registers there and the LayerNorm-folded GEGLU of level 2 ran at 234 us instead of 140):
//   0 plain (bias / row vector / activation / residual), 1 plain + LayerNorm-fold statistics out, 2 GEGLU
template <int EPI>
__device__ __forceinline__ void v5_epilogue_strip(const GemmParams& p, half_t* Cs, int z, int m_base, int n_base, int lane, int part, bool bias_done) {
    const bool rows_full = m_base + 16 <= p.M;                          // (wave-uniform) every row of the strip exists: the branch-free paths
    // (GEGLU keeps the predicated loop: with 40 accumulators of the next strips still live, the batched / interleaved form of the 128 x 160
    // kernel's epilogue spills here and measured 14 % slower per launch at 4096 x 10240 x 1280)
    if (EPI == 2) {   // GEGLU: the wave's 160 columns are one [80 value | 80 gate] block -> 80 outputs
        if (rows_full) {
            // Round 5: whole strips take the batched form — every global / LDS operand of the strip requested first, then the stage-by-stage
            // GELUs of common.h (8 per chunk; with the one-transcendental GELU its live set is 40 registers: no spills next to the 80
            // accumulators of the strips still waiting, which is what ruled this form out with round 4's GELU: -14 % per launch then).
            // 160 chunk pairs over 64 lanes: two full rounds and one of 32 lanes (the others recompute chunk 0 and do not store).
            half_t* Cb = p.C + (long long)z * p.sC + (long long)m_base * p.ldc + n_base / 2;
            const bool hr = p.R != nullptr;
            const half_t* Rb = hr ? p.R + (long long)z * p.sR + (long long)m_base * p.ldr + n_base / 2 : nullptr;
            // (the value / gate biases are in the staged strip already: v5_finish adds them in fp32 before the rounding)
            uint4 rres[3], ca[3], cg[3];
#pragma unroll
            for (int it = 0; it < 3; ++it) {
                const int q0 = lane + it * 64;
                const int q = q0 < 160 ? q0 : 0;
                const int row = q / 10, cc = q - row * 10;
                rres[it] = hr ? ld16(Rb + (long long)row * p.ldr + cc * 8) : zero16();
                ca[it] = ld16(Cs + row * V5_EPI_LD + cc * 8);
                cg[it] = ld16(Cs + row * V5_EPI_LD + 80 + cc * 8);
            }
#pragma unroll
            for (int it = 0; it < 3; ++it) {
                const int q0 = lane + it * 64;
                const int q = q0 < 160 ? q0 : 0;
                const int row = q / 10, cc = q - row * 10;
                float g[8];
                unpack8(cg[it], g);
                const unsigned aw[4] = {ca[it].x, ca[it].y, ca[it].z, ca[it].w};
                const f32x2 gp[4] = {{g[0], g[1]}, {g[2], g[3]}, {g[4], g[5]}, {g[6], g[7]}};
                unsigned ow[4];
                geglu8_staged(aw, gp, ow);
                uint4 packed = make_uint4(ow[0], ow[1], ow[2], ow[3]);
                if (hr) packed = add8h(packed, rres[it]);
                if (q0 < 160) st16(Cb + (long long)row * p.ldc + cc * 8, packed);
            }
            return;
        }
        uint4 rba[3], rbg[3], rres[3];
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int q = lane + it * 64;
            const int row = q / 10, cc = q - row * 10;
            const int m = m_base + row, nv = n_base + cc * 8;
            const bool ok = q < 160 && m < p.M;
            rba[it] = (ok && !bias_done) ? ld16(p.bias_n + nv) : zero16();
            rbg[it] = (ok && !bias_done) ? ld16(p.bias_n + nv + 80) : zero16();
            rres[it] = (ok && p.R != nullptr) ? ld16(p.R + (long long)z * p.sR + (long long)m * p.ldr + n_base / 2 + cc * 8) : zero16();
        }
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int q = lane + it * 64;
            const int row = q / 10, cc = q - row * 10;
            const int m = m_base + row;
            if (q < 160 && m < p.M) {
                float a[8], g[8], ba[8], bg[8], r[8];
                unpack8(ld16(Cs + row * V5_EPI_LD + cc * 8), a);
                unpack8(ld16(Cs + row * V5_EPI_LD + 80 + cc * 8), g);
                unpack8(rba[it], ba);
                unpack8(rbg[it], bg);
                unpack8(rres[it], r);
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = (a[j] + ba[j]) * gelu_f(g[j] + bg[j]) + r[j];
                st16(p.C + (long long)z * p.sC + (long long)m * p.ldc + n_base / 2 + cc * 8, pack8(a));
            }
        }
        return;
    }
    const bool hb = p.bias_n != nullptr && !bias_done, hv = p.rowvec != nullptr, hr = p.R != nullptr;
    if (rows_full && p.bias_m == nullptr && p.act == 0 && bias_done) {
        // branch-free, all five chunks of a lane requested as one batch, and in PACKED fp16 (round 5, as the 128 x 160 kernel's tile epilogue:
        // the bias is in the staged strip already — v5_finish adds it in fp32 before the one rounding — so a chunk is strip (+ time-embedding
        // row) (+ residual) by v_pk_add_f16, exact sums rounded once, and the LayerNorm-fold row statistics come from v_dot2_f32_f16)
        half_t* Cb = p.C + (long long)z * p.sC + (long long)m_base * p.ldc + n_base;
        const half_t* Rb = hr ? p.R + (long long)z * p.sR + (long long)m_base * p.ldr + n_base : nullptr;
        float s1[5], s2[5];
        uint4 rv[5], rres[5], cv[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int q = lane + k * 64;
            const int row = q / 20, cc = q - row * 20;
            rv[k] = hv ? ld16(p.rowvec + (long long)((m_base + row) / p.rows_per_vec) * p.ldrv + n_base + cc * 8) : zero16();
            rres[k] = hr ? ld16(Rb + (long long)row * p.ldr + cc * 8) : zero16();
            cv[k] = ld16(Cs + row * V5_EPI_LD + cc * 8);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int q = lane + k * 64;
            const int row = q / 20, cc = q - row * 20;
            uint4 packed = cv[k];
            if (hv) packed = add8h(packed, rv[k]);
            if (hr) packed = add8h(packed, rres[k]);
            st16(Cb + (long long)row * p.ldc + cc * 8, packed);
            if (EPI == 1 && p.stat_out != nullptr) {   // LN-fold producer: row statistics of the stored fp16 values
                const half2v one2 = {(half_t)1.f, (half_t)1.f};
                const half2v h0 = __builtin_bit_cast(half2v, packed.x), h1 = __builtin_bit_cast(half2v, packed.y);
                const half2v h2 = __builtin_bit_cast(half2v, packed.z), h3 = __builtin_bit_cast(half2v, packed.w);
                float a1 = __builtin_amdgcn_fdot2(h1, one2, __builtin_amdgcn_fdot2(h0, one2, 0.f, false), false);
                float a2 = __builtin_amdgcn_fdot2(h1, h1, __builtin_amdgcn_fdot2(h0, h0, 0.f, false), false);
                s1[k] = __builtin_amdgcn_fdot2(h3, one2, __builtin_amdgcn_fdot2(h2, one2, a1, false), false);
                s2[k] = __builtin_amdgcn_fdot2(h3, h3, __builtin_amdgcn_fdot2(h2, h2, a2, false), false);
            }
        }
        if (EPI == 1 && p.stat_out != nullptr) {   // chunk partials -> LDS (the strip has been consumed) -> one lane per row, in chunk order
            float* sc = reinterpret_cast<float*>(Cs);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int it = 0; it < 5; ++it) *reinterpret_cast<float2*>(sc + (lane + it * 64) * 2) = make_float2(s1[it], s2[it]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane < 16) {
                float a = 0.f, b = 0.f;
#pragma unroll 4
                for (int c = 0; c < 20; ++c) {
                    const float2 t = *reinterpret_cast<const float2*>(sc + (lane * 20 + c) * 2);
                    a += t.x;
                    b += t.y;
                }
                *reinterpret_cast<float2*>(p.stat_out + ((long long)part * p.M + m_base + lane) * 2) = make_float2(a, b);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        return;
    }
    uint4 rb[5], rv[5], rres[5];
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        const int q = lane + it * 64;
        const int row = q / 20, cc = q - row * 20;
        const int m = m_base + row, n = n_base + cc * 8;
        const bool ok = m < p.M;
        rb[it] = (ok && hb) ? ld16(p.bias_n + n) : zero16();
        rv[it] = (ok && hv) ? ld16(p.rowvec + (long long)(m / p.rows_per_vec) * p.ldrv + n) : zero16();
        rres[it] = (ok && hr) ? ld16(p.R + (long long)z * p.sR + (long long)m * p.ldr + n) : zero16();
    }
    float s1[5], s2[5];
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        const int q = lane + it * 64;
        const int row = q / 20, cc = q - row * 20;
        const int m = m_base + row, n = n_base + cc * 8;
        s1[it] = s2[it] = 0.f;
        if (m < p.M) {
            float v[8], b[8], e[8], r[8];
            unpack8(ld16(Cs + row * V5_EPI_LD + cc * 8), v);
            unpack8(rb[it], b);
            unpack8(rv[it], e);
            unpack8(rres[it], r);
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
            if (EPI == 1 && p.stat_out != nullptr) {   // LN-fold producer: row statistics of what was actually stored (the fp16 values)
                float f[8];
                unpack8(packed, f);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    s1[it] += f[j];
                    s2[it] += f[j] * f[j];
                }
            }
        }
    }
    if (EPI == 1 && p.stat_out != nullptr) {   // chunk partials -> LDS (the strip has been consumed) -> one lane per row sums them in chunk order
        float* sc = reinterpret_cast<float*>(Cs);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const int q = lane + it * 64;
            sc[q * 2] = s1[it];
            sc[q * 2 + 1] = s2[it];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane < 16 && m_base + lane < p.M) {
            float a = 0.f, b = 0.f;
            for (int c = 0; c < 20; ++c) {
                a += sc[(lane * 20 + c) * 2];
                b += sc[(lane * 20 + c) * 2 + 1];
            }
            float* o = p.stat_out + ((long long)part * p.M + m_base + lane) * 2;
            o[0] = a;
            o[1] = b;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// upconv (gemm5_kernel<true, 0, true>): one staged 16-row x 160-column strip -> depth-to-space store.  Row m = (img, y, x) of the SOURCE image is output
// pixel (2y + py, 2x + px); a row's 320-byte segment stays 16-byte chunks of one pixel's channels, only its base address changes (one lane per
// row works it out, the others fetch it by shuffle).  The bias is in the staged strip already; no residual, row vector or activation here.
__device__ __forceinline__ void v5_upconv_strip(const GemmParams& p, const half_t* Cs, int m_base, int col, int py, int px, int lane) {
    const int m = m_base + (lane & 15);
    const int mm = m < p.M ? m : p.M - 1;
    const int hw = p.Hs * p.Ws, img = mm / hw, rem = mm - img * hw, y = rem / p.Ws, x = rem - y * p.Ws;
    const int orow = (img * 2 * p.Hs + 2 * y + py) * (2 * p.Ws) + 2 * x + px;        // output pixel index (n * 4 * Hs * Ws < 2^31: gemm_plan)
    uint4 cv[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int q = lane + k * 64;
        const int row = q / 20, cc = q - row * 20;
        cv[k] = ld16(Cs + row * V5_EPI_LD + cc * 8);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int q = lane + k * 64;
        const int row = q / 20, cc = q - row * 20;
        const int o = __shfl(orow, row, 64);
        if (m_base + row < p.M) st16(p.C + (long long)o * p.ldc + col + cc * 8, cv[k]);
    }
}

// tail shared by the 256 x 320 tile kernels (v5 / v6): split-K slab store, or the staged fused epilogue (two 16-row strips at a
// time through this wave's 10.5 KB of the — by now quiet — LDS ring)
template <int EPI, bool LNC, bool UPF = false>   // EPI: see v5_epilogue_strip; LNC: LayerNorm-fold consumer (ln_mu / ln_rs valid); UPF: upconv (depth-to-space store)
__device__ __forceinline__ void v5_finish(const GemmParams& p, f32x4 (&acc)[4][10], char* smem5, const float* ln_mu, const float* ln_rs, int z, int m0,
                                          int n0, int wm0, int wn0, int wid, int lane, int ks, int splitk, int tn_i) {
    constexpr int TM = 4, TN = 10;
    const int fr = lane & 15, fq = lane >> 4;
    const int m_w = m0 + wm0, n_w = n0 + wn0;
    if (splitk > 1) {
        float* part = p.partial + (long long)ks * p.M * p.N;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_w + i * 16 + fr;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n_w + j * 16 + fq * 4;
                if (m < p.M) {
                    f32x4 v = acc[i][j];
                    v *= p.alpha;
                    *reinterpret_cast<f32x4*>(part + (long long)m * p.N + n) = v;
                }
            }
        }
        return;
    }
    // the ring is quiet (every wave is past its last fragment read and DMA wait): each wave stages two 16-row strips at a time in
    // its own 10.5 KB of it, so at most half of the accumulators are live next to the epilogue's prefetch registers
    half_t* Cs = reinterpret_cast<half_t*>(smem5 + wid * 2 * V5_EPI_BYTES);
    const int part = tn_i * 2 + (wid & 1);                          // LN-fold statistics: one part per 160-column half tile
    const bool ln = LNC && p.ln_stat != nullptr;
    // plain epilogues (no activation) and GEGLU: the bias is added HERE, in fp32 before the one rounding to fp16, and the strips add none
    const bool bias_done = EPI == 2 || p.act == 0;                 // (GEGLU: value and gate biases alike)
    const bool add_b = bias_done && p.bias_n != nullptr;
    // (always a load: an absent bias reads the zero page — a select around a load makes hipcc branch and wait per load; per strip, from L1 after
    // the first: a batch held for all four strips costs 20 registers next to the 160 accumulators and spilled)
    // (upconv: the tile lies in one phase's column block; bias and output columns count from that block's start)
    const int up_cout = UPF ? p.N >> 2 : 1, up_ph = UPF ? n0 / up_cout : 0, up_col = n_w - up_ph * up_cout;
    const half_t* bsrc = (add_b ? p.bias_n + (UPF ? up_col : n_w) : reinterpret_cast<const half_t*>(g_zero_row)) + fq * 4;
    auto stage = [&](auto I, half_t* dst) {                         // literal strip index: the accumulators stay in registers
        constexpr int i = decltype(I)::value;
        // LN-fold consumer: acc <- rstd * (acc - mu * wsum) in fp32, strip by strip (keeps the live registers low)
        const float mu = ln ? ln_mu[wm0 + i * 16 + fr] : 0.f, rs = ln ? ln_rs[wm0 + i * 16 + fr] : 1.f;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            f32x4 v = acc[i][j];
            if (ln) {
                const f32x4 ws = *reinterpret_cast<const f32x4*>(p.ln_wsum + n_w + j * 16 + fq * 4);
                v = (v - mu * ws) * rs;
            }
            const half4 bh = *reinterpret_cast<const half4*>(bsrc + j * 16);   // (L1-resident after the first strip; GEGLU: [80 value | 80 gate] biases, the strip's column order)
            f32x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = v[r] * p.alpha + (float)bh[r];
            *reinterpret_cast<uint2*>(dst + fr * V5_EPI_LD + j * 16 + fq * 4) = make_uint2(pk2h(o[0], o[1]), pk2h(o[2], o[3]));
        }
    };
    half_t* Cs1 = Cs + 16 * V5_EPI_LD;
    stage(std::integral_constant<int, 0>{}, Cs);
    stage(std::integral_constant<int, 1>{}, Cs1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // same wave, in-order LDS: the strips are complete
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (UPF) {
        v5_upconv_strip(p, Cs, m_w, up_col, up_ph >> 1, up_ph & 1, lane);
        v5_upconv_strip(p, Cs1, m_w + 16, up_col, up_ph >> 1, up_ph & 1, lane);
    } else {
        v5_epilogue_strip<EPI>(p, Cs, z, m_w, n_w, lane, part, bias_done);
        v5_epilogue_strip<EPI>(p, Cs1, z, m_w + 16, n_w, lane, part, bias_done);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // strips consumed before the next pair overwrites them
    __builtin_amdgcn_sched_barrier(0);
    stage(std::integral_constant<int, 2>{}, Cs);
    stage(std::integral_constant<int, 3>{}, Cs1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (UPF) {
        v5_upconv_strip(p, Cs, m_w + 32, up_col, up_ph >> 1, up_ph & 1, lane);
        v5_upconv_strip(p, Cs1, m_w + 48, up_col, up_ph >> 1, up_ph & 1, lane);
    } else {
        v5_epilogue_strip<EPI>(p, Cs, z, m_w + 32, n_w, lane, part, bias_done);
        v5_epilogue_strip<EPI>(p, Cs1, z, m_w + 48, n_w, lane, part, bias_done);
    }
}

// Epilogue of the halo-tile kernel's narrower tiles (256 x 256: the VAE's N = 256 / 512 convolutions; written for any width 16 TN per
// wave): wave tile 64 x WN, WN = 16 TN.  Convolutions carry no LayerNorm fold and no
// GEGLU, so this is the plain epilogue only (bias / bias_m / row vector / SiLU / residual), written once for every WN: two 16-row strips
// at a time through the wave's slice of the (quiet) LDS, operands of a strip requested as one batch, predicated stores.
template <int TM, int TN>
__device__ __forceinline__ void v6_finish(const GemmParams& p, f32x4 (&acc)[TM][TN], char* smem5, int m0, int n0, int wm0, int wn0, int wid, int lane, int ks,
                                          int splitk, int gimg, int gchunk) {
    static_assert(TM == 4 || TM == 8, "wave tile of 64 or 128 rows");
    constexpr int WN = TN * 16, LD = WN + 4, STRIP_BYTES = 16 * LD * 2;
    constexpr int CPR = WN / 8, TOT = 16 * CPR, ITS = (TOT + 63) / 64;
    const int fr = lane & 15, fq = lane >> 4;
    const int m_w = m0 + wm0, n_w = n0 + wn0;
    if (splitk > 1) {
        float* part = p.partial + (long long)ks * p.M * p.N;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m_w + i * 16 + fr;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (m < p.M) {
                    f32x4 v = acc[i][j];
                    v *= p.alpha;
                    *reinterpret_cast<f32x4*>(part + (long long)m * p.N + n_w + j * 16 + fq * 4) = v;
                }
            }
        }
        return;
    }
    half_t* Cs0 = reinterpret_cast<half_t*>(smem5 + wid * 2 * STRIP_BYTES);
    const bool hb = p.bias_n != nullptr, hv = p.rowvec != nullptr, hr = p.R != nullptr;
    // GroupNorm statistics of the OUTPUT (GemmParams::gn_part, host-checked: whole tiles of one image, groups of 4 or of whole 8-channel
    // chunks): a lane always handles the same 8-channel chunk, so it sums what it stores (the fp16-rounded values) over its rows —
    // (sum, sum of squares) of channels 0-3 / 4-7 apart when a group is 4 channels wide — and the tile's partials are put together below
    const bool gne = p.gn_part != nullptr, g4 = p.N == 128;
    float gs[4] = {0.f, 0.f, 0.f, 0.f};
    // plain epilogues (no activation, no per-row bias): the bias is added HERE, in fp32 before the one rounding to fp16, and the strips work
    // in packed fp16 (round 5, as v5_finish: the fp32 form cost ~70 vector instructions per 16-byte chunk — a quarter of the N = 128 convolutions'
    // launch time at K = 1152)
    const bool packed_ok = p.act == 0 && p.bias_m == nullptr;
    const half_t* bsrc = ((packed_ok && hb) ? p.bias_n + n_w : reinterpret_cast<const half_t*>(g_zero_row)) + fq * 4;   // (always a load: zero page without a bias)
    auto stage = [&](auto I, half_t* dst) {
        constexpr int i = decltype(I)::value;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const half4 bh = *reinterpret_cast<const half4*>(bsrc + j * 16);
            f32x4 v = acc[i][j] * p.alpha;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += (float)bh[r];
            *reinterpret_cast<uint2*>(dst + fr * LD + j * 16 + fq * 4) = make_uint2(pk2h(v[0], v[1]), pk2h(v[2], v[3]));
        }
    };
    auto strip = [&](const half_t* Cs, int m_base) {
        if (packed_ok) {
            uint4 rv[ITS], rres[ITS], cv[ITS];
#pragma unroll
            for (int it = 0; it < ITS; ++it) {
                const int q0 = lane + it * 64;
                const int q = (TOT % 64 == 0 || q0 < TOT) ? q0 : 0;
                const int row = q / CPR, cc = q - row * CPR;
                const int m = m_base + row < p.M ? m_base + row : p.M - 1;
                const int n = n_w + cc * 8;
                rv[it] = hv ? ld16(p.rowvec + (long long)(m / p.rows_per_vec) * p.ldrv + n) : zero16();
                rres[it] = hr ? ld16(p.R + (long long)m * p.ldr + n) : zero16();
                cv[it] = ld16(Cs + row * LD + cc * 8);
            }
#pragma unroll
            for (int it = 0; it < ITS; ++it) {
                const int q0 = lane + it * 64;
                const int q = (TOT % 64 == 0 || q0 < TOT) ? q0 : 0;
                const int row = q / CPR, cc = q - row * CPR;
                uint4 packed = cv[it];
                if (hv) packed = add8h(packed, rv[it]);
                if (hr) packed = add8h(packed, rres[it]);
                if ((TOT % 64 == 0 || q0 < TOT) && m_base + row < p.M && n_w + cc * 8 < p.n_valid) {
                    st16(p.C + (long long)(m_base + row) * p.ldc + n_w + cc * 8, packed);
                    if (gne) {   // v_dot2_f32_f16 on the packed pairs: 8 instructions per chunk
                        const half2v one2 = {(half_t)1.f, (half_t)1.f};
                        const half2v h0 = __builtin_bit_cast(half2v, packed.x), h1 = __builtin_bit_cast(half2v, packed.y);
                        const half2v h2 = __builtin_bit_cast(half2v, packed.z), h3 = __builtin_bit_cast(half2v, packed.w);
                        gs[0] = __builtin_amdgcn_fdot2(h1, one2, __builtin_amdgcn_fdot2(h0, one2, gs[0], false), false);     // channels 0-3
                        gs[1] = __builtin_amdgcn_fdot2(h1, h1, __builtin_amdgcn_fdot2(h0, h0, gs[1], false), false);
                        gs[2] = __builtin_amdgcn_fdot2(h3, one2, __builtin_amdgcn_fdot2(h2, one2, gs[2], false), false);     // channels 4-7
                        gs[3] = __builtin_amdgcn_fdot2(h3, h3, __builtin_amdgcn_fdot2(h2, h2, gs[3], false), false);
                    }
                }
            }
            return;
        }
        uint4 rb[ITS], rv[ITS], rres[ITS], cv[ITS];
        half_t rm[ITS];
#pragma unroll
        for (int it = 0; it < ITS; ++it) {
            const int q0 = lane + it * 64;
            const int q = (TOT % 64 == 0 || q0 < TOT) ? q0 : 0;
            const int row = q / CPR, cc = q - row * CPR;
            const int m = m_base + row < p.M ? m_base + row : p.M - 1;
            const int n = n_w + cc * 8;
            rb[it] = hb ? ld16(p.bias_n + n) : zero16();
            rv[it] = hv ? ld16(p.rowvec + (long long)(m / p.rows_per_vec) * p.ldrv + n) : zero16();
            rres[it] = hr ? ld16(p.R + (long long)m * p.ldr + n) : zero16();
            rm[it] = p.bias_m != nullptr ? p.bias_m[m] : (half_t)0.f;
            cv[it] = ld16(Cs + row * LD + cc * 8);
        }
#pragma unroll
        for (int it = 0; it < ITS; ++it) {
            const int q0 = lane + it * 64;
            const int q = (TOT % 64 == 0 || q0 < TOT) ? q0 : 0;
            const int row = q / CPR, cc = q - row * CPR;
            float v[8], b[8], e[8], r[8];
            unpack8(cv[it], v);
            unpack8(rb[it], b);
            unpack8(rv[it], e);
            unpack8(rres[it], r);
            const float bm = (float)rm[it];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float t = v[j] + b[j] + bm + e[j];
                if (p.act == 1) t = silu_tile_f(t);
                else if (p.act == 3) t = quick_gelu_tile_f(t);
                v[j] = t + r[j];
            }
            if ((TOT % 64 == 0 || q0 < TOT) && m_base + row < p.M && n_w + cc * 8 < p.n_valid) {
                const uint4 packed = pack8(v);
                st16(p.C + (long long)(m_base + row) * p.ldc + n_w + cc * 8, packed);
                if (gne) {   // v_dot2_f32_f16 on the packed pairs: 8 instructions per chunk
                    const half2v one2 = {(half_t)1.f, (half_t)1.f};
                    const half2v h0 = __builtin_bit_cast(half2v, packed.x), h1 = __builtin_bit_cast(half2v, packed.y);
                    const half2v h2 = __builtin_bit_cast(half2v, packed.z), h3 = __builtin_bit_cast(half2v, packed.w);
                    gs[0] = __builtin_amdgcn_fdot2(h1, one2, __builtin_amdgcn_fdot2(h0, one2, gs[0], false), false);     // channels 0-3
                    gs[1] = __builtin_amdgcn_fdot2(h1, h1, __builtin_amdgcn_fdot2(h0, h0, gs[1], false), false);
                    gs[2] = __builtin_amdgcn_fdot2(h3, one2, __builtin_amdgcn_fdot2(h2, one2, gs[2], false), false);     // channels 4-7
                    gs[3] = __builtin_amdgcn_fdot2(h3, h3, __builtin_amdgcn_fdot2(h2, h2, gs[3], false), false);
                }
            }
        }
    };
    half_t* Cs1 = Cs0 + 16 * LD;
    auto pair = [&](auto P) {                                            // strips 2P, 2P + 1 (literal indices: the accumulators stay in registers)
        constexpr int i0 = 2 * decltype(P)::value;
        stage(std::integral_constant<int, i0>{}, Cs0);
        stage(std::integral_constant<int, i0 + 1>{}, Cs1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // same wave, in-order LDS: the strips are complete
        __builtin_amdgcn_sched_barrier(0);
        strip(Cs0, m_w + 16 * i0);
        strip(Cs1, m_w + 16 * i0 + 16);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // strips consumed before the next pair overwrites them
        __builtin_amdgcn_sched_barrier(0);
    };
    pair(std::integral_constant<int, 0>{});
    pair(std::integral_constant<int, 1>{});
    if constexpr (TM == 8) {
        pair(std::integral_constant<int, 2>{});
        pair(std::integral_constant<int, 3>{});
    }
    if (gne && 64 % CPR == 0) {   // (workgroup-uniform; a lane keeps its chunk over the strips only when CPR divides 64: the host asks for it at BN = 256 / 128 only)
        if (!g4) {   // groups of whole chunks: the two halves of the chunk belong together
            gs[0] += gs[2];
            gs[1] += gs[3];
        }
#pragma unroll
        for (int o = CPR; o < 64; o <<= 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) gs[k] += __shfl_xor(gs[k], o, 64);
        }
        float* wp = reinterpret_cast<float*>(smem5 + 8 * 2 * STRIP_BYTES);      // [8 waves][CPR chunks][4], behind every wave's strips
        if (lane < CPR) *reinterpret_cast<float4*>(wp + (wid * CPR + lane) * 4) = make_float4(gs[0], gs[1], gs[2], gs[3]);
        __syncthreads();
        // one thread per group of the tile: the four waves of its column half top to bottom, the group's chunks left to right (fixed order)
        const int cpg = p.N / 32, tid = wid * 64 + lane;
        if (tid < 2 * WN / cpg) {
            const int col = tid * cpg, wn = col / WN, cf = (col - wn * WN) >> 3;
            const int nch = cpg >= 8 ? cpg >> 3 : 1, part = (cpg == 4 && (col & 4)) ? 2 : 0;
            float s = 0.f, ss = 0.f;
            for (int wmi = 0; wmi < 4; ++wmi)
                for (int c = 0; c < nch; ++c) {
                    const float* e = wp + ((wmi * 2 + wn) * CPR + cf + c) * 4 + part;
                    s += e[0];
                    ss += e[1];
                }
            float* o = p.gn_part + (((long long)gimg * p.gn_P + gchunk) * 32 + (n0 + col) / cpg) * 2;
            o[0] = s;
            o[1] = ss;
        }
    }
}

}  // namespace
