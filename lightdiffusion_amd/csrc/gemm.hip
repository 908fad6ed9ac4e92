// Contraction dispatch (gemm.h): the route planner gemm_plan, the dispatcher gemm_run and the split-K second passes.  The kernel
// families live in gemm3.hip, gemm5.hip, conv6.hip, gemm7.hip and conv8.hip; gemm_kernels.h is what this file sees of them.
#include <cstdlib>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "gemm_device.h"
#include "gemm_kernels.h"

namespace {

// the sum of a launch's split-K slabs for eight adjacent columns (`base`: the columns in slab 0; slabs `slab` floats apart): four slabs per
// batch of loads, summed in slab order (a split of 16 read one slab after the other is 16 memory latencies in a row: the reduce launches of
// the batch-1 step were latency-, not bandwidth-bound).  Returned by value: through a pointer to the caller's array the compiler keeps eight
// scalar accumulators and pairs them into two-wide adds, where both second passes had one eight-wide accumulator
struct F8 { float v[8]; };
__device__ __forceinline__ F8 slab_sum8(const float* base, long long slab, int splitk) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    int s = 0;
    for (; s + 4 <= splitk; s += 4) {
        f32x4 x0[4], x1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            x0[u] = *reinterpret_cast<const f32x4*>(base + (s + u) * slab);
            x1[u] = *reinterpret_cast<const f32x4*>(base + (s + u) * slab + 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] += x0[u][j];
                v[4 + j] += x1[u][j];
            }
    }
    for (; s < splitk; ++s) {
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(base + s * slab), x1 = *reinterpret_cast<const f32x4*>(base + s * slab + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] += x0[j];
            v[4 + j] += x1[j];
        }
    }
    F8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r.v[j] = v[j];
    return r;
}

// split-K second pass: sum the fp32 slabs and run the same epilogue
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmParams p, int bn) {
    const int out_n = p.act == 2 ? p.N / 2 : p.N;
    const int cpr = out_n / 8;
    const long long total = (long long)p.M * cpr;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(q / cpr), cc = (int)(q - (long long)m * cpr);
        float v[8];
        if (p.act == 2) {
            const int half_bn = bn / 2;
            const int no = cc * 8;
            const int tile = no / half_bn, within = no - tile * half_bn;
            const int nv = tile * bn + within, ng = nv + half_bn;
            float a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int s = 0; s < p.splitk; ++s) {
                const float* base = p.partial + ((long long)s * p.M + m) * p.N;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    a[j] += base[nv + j];
                    g[j] += base[ng + j];
                }
            }
            float ba[8], bg[8];
            unpack8(ld16(p.bias_n + nv), ba);
            unpack8(ld16(p.bias_n + ng), bg);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (a[j] + ba[j]) * gelu_f(g[j] + bg[j]);
            epilogue_store8(p, 0, m, no, 0, v);
        } else {
            const int n = cc * 8;
            const F8 r = slab_sum8(p.partial + (long long)m * p.N + n, (long long)p.M * p.N, p.splitk);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = r.v[j];
            epilogue_store8(p, 0, m, n, n, v);
        }
    }
}

// split-K second pass that also emits the GroupNorm partial statistics of its output (GemmParams::gn_part): block = (pixel chunk, image,
// slab of 8 groups), a thread owns one 8-channel chunk and strides over the chunk's pixels — thread mapping, LDS layout and summation
// order are those of gn_stats_kernel (norm.hip), so the partials (and the normalised tensor) are bit-identical to the two-launch path.
__global__ __launch_bounds__(256) void splitk_reduce_gn_kernel(const GemmParams p) {
    __shared__ float csum[2048], csq[2048];   // [rows_par][slab channels]
    const int C = p.N, cpg = C / 32;
    const int CS = C / 4, CHS = CS >> 3;
    const int n = blockIdx.y, pc = blockIdx.x, slab = blockIdx.z, tid = threadIdx.x;
    const int rows_par = 256 / CHS;
    const int cc = tid % CHS, prow = tid / CHS;
    const int c0 = slab * CS + cc * 8;
    const int p_begin = pc * p.gn_ppb, p_end = min(p.gn_HW, p_begin + p.gn_ppb);
    const long long slab_stride = (long long)p.M * p.N;
    if (prow < rows_par) {
        float s[8], ss[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = ss[j] = 0.f;
        for (int pix = p_begin + prow; pix < p_end; pix += rows_par) {
            const int m = n * p.gn_HW + pix;
            float v[8];
            const F8 r = slab_sum8(p.partial + (long long)m * p.N + c0, slab_stride, p.splitk);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = r.v[j];
            epilogue_store8(p, 0, m, c0, c0, v);                       // (v comes back as the values before the fp16 rounding)
            float f[8];
            unpack8(pack8(v), f);                                      // statistics of what was stored: the fp16 values, as gn_stats_kernel reads them
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s[j] += f[j];
                ss[j] += f[j] * f[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            csum[prow * CS + cc * 8 + j] = s[j];
            csq[prow * CS + cc * 8 + j] = ss[j];
        }
    }
    __syncthreads();
    {
        const int g = tid >> 5, sub = tid & 31;                  // 8 groups x 32 lanes
        const int cnt = rows_par * cpg;
        float a = 0.f, b = 0.f;
        for (int i = sub; i < cnt; i += 32) {
            const int pr = i / cpg, c = g * cpg + (i - pr * cpg);
            a += csum[pr * CS + c];
            b += csq[pr * CS + c];
        }
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            a += __shfl_xor(a, o, 64);
            b += __shfl_xor(b, o, 64);
        }
        if (sub == 0) {
            float* o = p.gn_part + (((long long)n * p.gn_P + pc) * 32 + slab * 8 + g) * 2;
            o[0] = a;
            o[1] = b;
        }
    }
}

// the profile name of a plan: composed here and nowhere else, once per distinct plan and thread.  conv6's name says what differs from the
// 256 x 320 tile: conv6_kernel<W64,halo+groupnorm>, conv6_kernel<W128,halo,128x512>, conv6_kernel<W64,halo,256,up>, ...
const char* plan_kernel_name(const GemmPlan& pl) {
    typedef unsigned long long u64;
    const u64 key = (u64)pl.route | (u64)pl.reduce << 3 | (u64)pl.conv << 5 | (u64)pl.geglu << 6 | (u64)pl.gn << 7 | (u64)pl.up << 8 | (u64)pl.ln << 9 |
                    (u64)pl.deep << 10 | (u64)pl.two_wg << 11 | (u64)pl.bm << 12 | (u64)pl.bn << 24 | (u64)pl.wc << 36;
    thread_local std::vector<std::pair<u64, const char*>> seen;   // (a handful per process)
    for (const auto& e : seen)
        if (e.first == key) return e.second;
    const std::string tile = std::to_string(pl.bm) + "," + std::to_string(pl.bn);
    std::string s;
    switch (pl.route) {
        case GR_UPCONV: s = "upconv_kernel<256,320>"; break;   // (gemm5_kernel<true, 0, true>: a family name of its own, see the kernel)
        case GR_CONV8: s = "conv8_kernel<W" + std::to_string(pl.wc) + (pl.up ? ",up>" : ">"); break;
        case GR_CONV6:
            s = "conv6_kernel<W" + std::to_string(pl.wc) + ",halo" + (pl.gn ? "+groupnorm" : "") +
                (pl.bn == V5_BN ? "" : "," + std::to_string(pl.bn) + (pl.bm == V5_BM ? "" : "x" + std::to_string(pl.bm))) + (pl.up ? ",up" : "") + ">";
            break;
        case GR_GEMM7: s = std::string("gemm7_kernel<256,K320,") + (pl.geglu ? "geglu" : "plain") + (pl.ln ? ",ln>" : ">"); break;
        case GR_GEMM5: s = std::string("gemm5_kernel<256,320,") + (pl.conv ? "conv" : pl.geglu ? "geglu" : pl.ln ? "lnfold" : "plain") + ">"; break;
        case GR_GEMM4: s = "gemm4_kernel<" + tile + (pl.conv ? ",conv" : ",plain") + (pl.two_wg ? ",2wg>" : ">"); break;
        default: s = "gemm3_kernel<" + tile + (pl.conv ? ",conv" : ",plain") + (pl.deep ? ",deep>" : ">"); break;
    }
    if (pl.reduce != GRD_NONE) s += pl.reduce == GRD_GROUPNORM ? "+splitk_reduce_gn_kernel" : pl.reduce == GRD_UPCONV ? "+upconv_reduce_kernel" : "+splitk_reduce_kernel";
    static std::mutex mu; static std::set<std::string> pool;   // stable storage
    std::lock_guard<std::mutex> lock(mu);
    const char* name = pool.insert(s).first->c_str();
    seen.push_back({key, name});
    return name;
}

}  // namespace

#ifdef LD_AB_BUILD
// tuning hook of the A/B build (tools/gemm_sweep.py, tools/ab_launches.py): force tile height / split-K for every following launch; 0 = automatic.
// Not part of the shipped library: `make ab` builds libld_mi355x_ab.so with it.
static int g_force_bm = 0, g_force_sk = 0;
// per-shape override (tools/ab_shape.py: candidates are timed launch by launch INSIDE the forward): M, N, K -> tile height, split
static int g_shape_ovr[5] = {0, 0, 0, 0, 0};
extern "C" void ld_debug_gemm_shape_override(int M, int N, int K, int bm, int splitk) {
    g_shape_ovr[0] = M; g_shape_ovr[1] = N; g_shape_ovr[2] = K; g_shape_ovr[3] = bm; g_shape_ovr[4] = splitk;
}
extern "C" void ld_debug_gemm_override(int bm, int splitk) {
    g_force_bm = bm;
    g_force_sk = splitk;
}
#endif

// the split-K second pass of a launch: the plain reduce, or the one that also emits GroupNorm partials (GemmParams::gn_part)
static void plan_reduce(const GemmParams& p, GemmPlan* pl) {
    if (pl->splitk <= 1) return;
    // (N >= 256: below that gn_stats_kernel uses fewer, wider channel slabs — norm.hip gn_slabs — and this kernel's four-slab order would
    // no longer reproduce its partials bit for bit)
    const bool gn = p.gn_part != nullptr && p.act != 2 && p.batch == 1 && p.gn_P > 0 && p.gn_HW > 0 && p.M % p.gn_HW == 0 && p.N % 32 == 0 && p.N <= 8192 && p.N >= 256 &&
                    p.ldc == p.N && (p.N / 4) % 8 == 0 && p.N / 32 <= 256;
    pl->reduce = gn ? GRD_GROUPNORM : GRD_PLAIN;
    if (gn) pl->gn_chunks = p.gn_P;
}

// does this convolution run on the upconv route (p.Wup set), and with which split over K?  Fills bm, bn, splitk, grid_x, reduce.
// Tiles are those of the launch's own view: M / 4 source pixels x 4 N columns, K = 4 Cin.
static bool upconv_plan(const GemmParams& p, GemmPlan* out) {
    if (!(p.conv && p.ksize == 3 && p.stride == 1 && p.pad == 1 && p.Hv == 2 * p.Hs && p.Wv == 2 * p.Ws && p.Ho == p.Hv && p.Wo == p.Wv && p.C2 == 0 &&
          p.SC1 == 0 && p.C1 % V5_BK == 0 && p.N % V5_BN == 0 && p.n_valid == p.N && p.bm == 0 && p.bn == 0 && p.splitk == 0 && p.batch == 1 && p.act == 0 &&
          p.alpha == 1.0f && p.rowvec == nullptr && p.R == nullptr && p.bias_m == nullptr && p.stat_out == nullptr && p.ln_stat == nullptr && p.ldc == p.N))
        return false;
    if ((long long)p.M * 4 > 0x7fffffffll) return false;             // (the epilogue's pixel index is an int)
    if (p.M / (p.Ho * p.Wo) <= 2) return false;                      // one or two images (the batch-1 step) keep today's routes, whichever kernel takes the shape
    const int Ms = p.M / 4, K = 4 * p.C1;
    const long long tiles = (long long)((Ms + V5_BM - 1) / V5_BM) * (4 * p.N / V5_BN);
    // fewer tiles than fill the chip: slices over K up to one workgroup per CU, each keeping >= 640 of K (the rule of the other split routes);
    // the second pass is upconv_reduce_kernel
    int sk = 1;
    if (tiles < 192 && p.partial != nullptr) {
        sk = (int)((256 + tiles - 1) / tiles);
        const int cap = K / 640 < 1 ? 1 : K / 640;
        if (sk > cap) sk = cap;
        while (sk > 1 && (size_t)sk * Ms * 4 * p.N * sizeof(float) > p.partial_bytes) --sk;
    }
    out->bm = V5_BM; out->bn = V5_BN; out->splitk = sk; out->up = true;
    out->grid_x = (unsigned)(tiles * sk); out->grid_z = 1;
    out->reduce = sk > 1 ? GRD_UPCONV : GRD_NONE;
    return true;
}

// does this convolution run on the halo-tile kernel (v6), and with which tile (rows x columns), split over K and loader (up)?
// gn: gn_scale / gn_shift are, or will be, set.  Fills bm, bn, wc, splitk, up.
static bool v6_plan(const GemmParams& p, bool gn, GemmPlan* out) {
    const bool same = p.Hv == p.Hs && p.Wv == p.Ws;
    const bool up = p.Hv == 2 * p.Hs && p.Wv == 2 * p.Ws;           // exact nearest 2x (Upsample: LD.py:3498-3511; Upsample1 when the skip is 2x)
    if (!(p.conv && p.ksize == 3 && p.stride == 1 && (p.pad < 0 || p.pad == 1) && (same || up) && p.Ho == p.Hv && p.Wo == p.Wv &&
          p.C1 % 32 == 0 && p.C2 % 32 == 0 && p.bm == 0 && p.bn == 0 && p.splitk == 0 && p.batch == 1 && p.act != 2))
        return false;
    if (up && (p.C2 != 0 || gn)) return false;
    const int wc = (p.Wo == 16 || p.Wo == 32 || p.Wo == 64 || p.Wo == 128) ? p.Wo : (p.Wo > 128 && p.Wo % 128 == 0) ? 128 : 0;
    if (wc == 0) return false;
    // tile: 320 columns for the UNet's N = 320 k; 256 for the VAE's N = 256 / 512 at >= 64-pixel rows (VAE decode b=8 29.9 -> 28.8 ms);
    // 512 pixels x 128 columns for its N = 128 (a 256 x 128 tile would leave a wave 16 MFMAs per phase: the step's fixed cost dominates).
    // (256 x 160 tiles for level 1 — 256 unsplit tiles instead of 128 + split — measured a net loss per launch inside the forward:
    // 16384 x 640 x 5760 737 vs 748 us per 6 launches, but 317 vs 291 / 217 vs 213 / 176 vs 170 us at K = 17280 / 11520 / 8640: a
    // 64 x 80 wave tile reads 1.3x the LDS bytes per MFMA and halves the MFMAs a step's fixed cost is spread over.)
    int bn = 0, bm = V5_BM;
    if (p.N % V5_BN == 0) {
        bn = V5_BN;
    } else if (p.N % 256 == 0 && wc >= 64 && (!gn || (p.N == 256 && wc == 128 && !up))) {   // (fused GroupNorm: one tile wide, 128-pixel bands)
        bn = 256;
    } else if (p.N % 128 == 0 && wc == 128 && !up && (!gn || p.N == 128)) {   // (!up: this tile has no nearest-2x loader instantiated)
        bn = 128;
        bm = 512;
    } else if (p.N == 32 && wc == 128 && !gn && !up) {
        // a <= 8-channel output convolution (the VAE's conv_out, weights zero-padded to 32 rows by the caller, n_valid = 8): 8 MFMAs per
        // wave and phase — the step's fixed cost dominates, but the halo tile is read once instead of nine times per pixel
        bn = 32;
        bm = 512;
    } else {
        return false;
    }
    if (p.Ho % (bm / wc) != 0 || p.M % bm != 0) return false;       // whole tiles: bm / wc image rows each
    // a second K segment (gemm.h S1 / S2) runs as centre-only steps behind the slabs (conv6.hip): 256 x 320 tiles of whole image rows, no resize.
    // The 128-pixel bands, the VAE's tiles and the nearest-2x loader have no such instantiation; a one-tile-wide output WITHOUT the fused GroupNorm
    // has no caller in the UNet (level 0's out_layers always brings its norm) and stays with the 256 x 320 tap-major kernel's fold.
    // skip_ok: this geometry takes the segment (asked with SC1 = 0 by Exec::conv_takes_skip_segment, before the GroupNorm is offered).
    const bool skip_ok = same && wc <= 64 && bn == V5_BN && bm == V5_BM && p.stride == 1 && (p.SC1 + p.SC2) % 32 == 0;
    if (p.SC1 > 0 && !(skip_ok && (gn || p.N != V5_BN))) return false;
    const long long tm = p.M / bm;
    const long long t6 = tm * (p.N / bn);
    const int NS = (p.C1 + p.C2) / 32;
    const int K9 = 9 * (p.C1 + p.C2);                                // (the split rule below was measured on the 3x3 segment alone: a skip segment does not move it)
    int sk6 = 1;
    // (split over K only from K = 8640 on: per launch inside the UNet forward (tools/ab_launches.py) the split + reduce pair loses to
    // the unsplit 128 x 160 kernel at 16384 x 640 x 5760 — 133 vs 124 us — and wins from 8640 on: 171 vs 176, 208 vs 227, 285 vs 329 us)
    if (t6 < 192 && p.partial != nullptr && K9 >= 8640) {
        sk6 = (int)((256 + t6 - 1) / t6);
        const int cap = K9 / 2560;
        if (sk6 > cap) sk6 = cap;
        if (sk6 > NS) sk6 = NS;
        while (sk6 > 1 && (size_t)sk6 * p.M * p.N * sizeof(float) > p.partial_bytes) --sk6;
    }
#ifdef LD_AB_BUILD
    if (p.partial != nullptr && bn == V5_BN) {   // split-factor sweep of the halo convolution (tools/conv6_split_sweep.py): LD_V6_SK_W<width> = slices over K
        static const char* names[4] = {"LD_V6_SK_W16", "LD_V6_SK_W32", "LD_V6_SK_W64", "LD_V6_SK_W128"};
        const char* e = getenv(names[wc == 16 ? 0 : wc == 32 ? 1 : wc == 64 ? 2 : 3]);
        if (e != nullptr) {
            int want = atoi(e);
            if (want < 1) want = 1;
            if (want > NS) want = NS;
            while (want > 1 && (size_t)want * p.M * p.N * sizeof(float) > p.partial_bytes) --want;
            sk6 = want;
        }
    }
#endif
    out->splitk = sk6; out->bn = bn; out->bm = bm; out->wc = wc; out->up = up;
    out->skip = p.SC1 > 0; out->takes_skip_segment = skip_ok;
    out->grid_x = (unsigned)(t6 * sk6);
    return t6 * sk6 >= 192;
}

GemmPlan gemm_plan(const GemmParams& pin, bool gn_offer) {
    GemmPlan pl;
    GemmParams p = pin;
    const bool gn = gn_offer || p.gn_scale != nullptr;
    const auto fail = [](int st) { GemmPlan f; f.status = st; return f; };
    const auto done = [&pl](int route) { pl.route = route; pl.kernel = plan_kernel_name(pl); return pl; };
#ifdef LD_AB_BUILD
    if (g_force_bm) p.bm = g_force_bm;
    if (g_force_sk) p.splitk = g_force_sk;
    if (g_shape_ovr[0] == p.M && g_shape_ovr[1] == p.N && g_shape_ovr[2] == p.K && p.batch == 1 && !gn) {
        p.bm = g_shape_ovr[3];
        p.splitk = g_shape_ovr[4];
    }
#endif
    // ---- validate
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.A == nullptr || p.W == nullptr || p.C == nullptr) return fail(LD_ERR_ARG);
    if ((p.N & 7) || (p.K & 7) || (p.ldw & 7) || (p.ldc & 7)) return fail(LD_ERR_SHAPE);
    if (p.conv) {
        const int Cin = p.C1 + p.C2;
        if (p.ksize != 1 && p.ksize != 3) return fail(LD_ERR_ARG);
        if (p.pad < 0) p.pad = p.ksize >> 1;
        if (p.SC1 < 0 || p.SC2 < 0 || (p.SC1 == 0 && p.SC2 != 0)) return fail(LD_ERR_ARG);
        if (Cin <= 0 || (p.C1 % 64) || (p.C2 % 64) || (p.SC1 % 64) || (p.SC2 % 64) || p.K != p.ksize * p.ksize * Cin + p.SC1 + p.SC2) return fail(LD_ERR_SHAPE);
        if (p.SC1 > 0) {   // second K segment (gemm.h): raw sources of the output's size, read at the output pixel itself
            if (p.S1 == nullptr || (p.SC2 > 0 && p.S2 == nullptr)) return fail(LD_ERR_ARG);
            if (p.stride != 1 || p.Hv != p.Hs || p.Wv != p.Ws || p.Ho != p.Hv || p.Wo != p.Wv || p.pad != p.ksize / 2 || p.SC1 > 32768 || p.SC2 > 32768) return fail(LD_ERR_SHAPE);
        }
        if (p.C1 > 32768 || p.C2 > 32768) return fail(LD_ERR_SHAPE);   // the stepped zero row (g_zero_row) covers one tap's channel run
        if (p.C2 > 0 && p.A2 == nullptr) return fail(LD_ERR_ARG);
        if (p.M % (p.Ho * p.Wo)) return fail(LD_ERR_SHAPE);
        if (p.batch != 1) return fail(LD_ERR_ARG);
    } else if (p.lda & 7) {
        return fail(LD_ERR_SHAPE);
    }
    if (p.act == 2 && (p.bias_n == nullptr || (p.N & 15))) return fail(LD_ERR_ARG);
    if (p.R != nullptr && (p.ldr & 7)) return fail(LD_ERR_SHAPE);
    if (p.n_valid <= 0 || p.n_valid > p.N) p.n_valid = p.N;
    pl.conv = p.conv != 0; pl.geglu = p.act == 2;

    // ---- conv8 (row-resident, weights streamed once, in-launch slab reduction): the two-image 16x16 / 8x8 levels of a batch-1 step
    if (!gn && conv8_plan(p, &pl.c8_S)) {
        pl.wc = p.Wo; pl.up = p.Hv == 2 * p.Hs;
        if (p.gn_part != nullptr) pl.gn_chunks = p.Wo * p.Wo / 16;   // the kernel emits the GroupNorm partials of its output itself
        return done(GR_CONV8);
    }
    // ---- upconv (nearest-2x folded into 2x2 phase weights, gemm.h Wup): the caller holds the folded weights and the resize is exactly 2x.
    // The route executes 4/9 of the multiply-adds of the 3x3 convolution it implements: M / 4 source pixels x 4 N columns x 4/9 K.
    if (p.Wup != nullptr && !gn && upconv_plan(p, &pl)) return done(GR_UPCONV);
    // ---- v6 (halo-tile 3x3 convolution on the v5 skeleton): stride-1 convs whose tiles are whole image rows and fill the chip
    if (GemmPlan v6 = pl; v6_plan(p, gn, &v6)) {
        pl = v6;
        const int bn6 = pl.bn, wc = pl.wc;
        if (gn) {
            if ((p.gn_scale != nullptr && p.gn_shift == nullptr) || pl.up) return fail(LD_ERR_ARG);
            if (bn6 != V5_BN && (wc != 128 || p.N != bn6 || !((bn6 == 256 && pl.bm == V5_BM) || (bn6 == 128 && pl.bm == 512)))) return fail(LD_ERR_ARG);
            // Measured (profiles/r02_ab_groupnorm_fusion.txt, same process): fused vs two-pass GroupNorm + the same halo conv: +4 % at N = 320 (level 0, one N
            // tile per M tile), +-0 % at N = 640, -3 % at N = 1280 — every N tile of an M tile normalises the same halo again, so the fusion
            // only pays where the output is one tile wide.
            // Round 5: also the VAE decoder's one-tile-wide stages — N = 256 at 256-pixel rows, N = 128 at 512-pixel rows (128-pixel bands) — where a
            // two-pass GroupNorm writes and re-reads 134 - 537 MB per convolution.
            // (the 128 -> 3 output convolution — 8 MFMAs per phase — measured a loss with its norm_out fused: VAE decode +0.15 ms, profiles/r05_ab_vae_gn_fused.txt)
            pl.can_fuse_groupnorm = bn6 != V5_BN || p.N == V5_BN;   // (a 256- / 128-column tile got here as the whole output's width only)
            if (gn_offer && !pl.can_fuse_groupnorm) return fail(LD_ERR_ARG);
            pl.gn = true;
        }
        if (pl.splitk == 1 && p.gn_part != nullptr) {
            // the generic epilogue (v6_finish) also writes the GroupNorm partial statistics of the OUTPUT, one chunk per tile of an image
            const int cpg = p.N / 32, tiles_img = (p.Ho / (pl.bm / wc)) * (p.Wo / wc);
            const bool ok = (bn6 == 256 || bn6 == 128) && p.N % 32 == 0 && (p.N == 128 || cpg % 8 == 0) && bn6 % cpg == 0 && p.act == 0;
            if (ok) pl.gn_chunks = tiles_img;
        }
        plan_reduce(p, &pl);
        pl.halo_tile = true;
        return done(GR_CONV6);
    }
    if (gn) return fail(LD_ERR_ARG);   // only the halo kernel applies a fused GroupNorm (ask with gn_offer first)
    // every 3x3 convolution from here on walks K tap-major
    pl.takes_skip_segment = p.conv && p.ksize == 3 && p.stride == 1 && p.Hv == p.Hs && p.Wv == p.Ws && p.SC1 == 0;
    // ---- v7 (row-panel kernel, A fragments in registers): the K = 320 projections whose 256-row panels fill the chip
    if (!p.conv && p.K == V7_K && p.batch == 1 && !p.ln_swapped && p.bias_m == nullptr && p.rowvec == nullptr && p.bm == 0 && (p.bn == 0 || p.bn == 160) &&
        p.splitk == 0 && (p.n_valid <= 0 || p.n_valid >= p.N) && p.N % (p.act == 2 ? 160 : V7_NB) == 0 && (p.M + V7_BM - 1) / V7_BM >= 192 &&
        (p.act == 0 || (p.act == 2 && p.bias_n != nullptr && p.stat_out == nullptr && p.R == nullptr))) {
        pl.stat_parts = p.N / V7_NB;
        pl.grid_x = (unsigned)((p.M + V7_BM - 1) / V7_BM); pl.ln = p.ln_stat != nullptr;
        return done(GR_GEMM7);
    }
    // ---- v5 (256 x 320 tile, 8 waves, staggered wave groups): whenever its tiles (x an optional split over K) fill the chip
    {
        // measured per launch inside the UNet forward against v3 (tools/ab_launches.py, profiles/README.md): +5..10 % on the 3x3 convolutions
        // the halo kernel cannot take and on the K = 1280 GEGLU; plain GEMMs / 1x1 convs with one tile per CU and K <= 1600 LOSE (16384 x
        // 1280 x 640: 69 vs 50 us, 65536 x 320 x 1600: 108 vs 103 us — nothing overlaps a short tile's prologue and epilogue), and so does
        // a split over K (4096 x 1280 x 11520: the 128 x 160 kernel's own split is 3 % ahead)
        const bool conv3 = p.conv && p.ksize == 3;
        const bool shape_ok = !p.ln_swapped && p.bm == 0 && (p.bn == 0 || p.bn == 160) && p.N % V5_BN == 0 && p.K % V5_BK == 0 &&
                              p.K >= (p.act == 2 ? 1280 : conv3 ? 640 : 2560) && (p.n_valid == p.N || p.n_valid <= 0 || p.n_valid > p.N) &&
                              p.splitk == 0 && p.M >= 1024;
        const int tm5 = (p.M + V5_BM - 1) / V5_BM, tn5 = p.N / V5_BN;
        if (shape_ok && (long long)tm5 * tn5 * p.batch >= 192 && !(p.act == 2 && p.stat_out != nullptr)) {
            pl.ln = p.ln_stat != nullptr || p.stat_out != nullptr;
            if (p.conv && (pl.ln || p.act == 2)) return fail(LD_ERR_ARG);          // (no caller: convolutions carry neither the LayerNorm fold nor GEGLU)
            pl.stat_parts = 2 * tn5;
            pl.bm = V5_BM; pl.bn = V5_BN;
            pl.grid_x = (unsigned)(tm5 * tn5); pl.grid_z = (unsigned)p.batch;
            pl.xcd_gm = p.xcd_gm;
            if (!p.conv) {
                // XCD-blocked tile order (see the kernel): the split of the 8 XCDs over (M, N) that moves the fewest bytes, A once per
                // N group and W once per M group
                pl.xcd_gm = 0;
                if (p.batch == 1 && (tm5 * tn5) % 8 == 0 && p.M % V5_BM == 0) {
                    double best = 0;
                    for (int gm = 1; gm <= 8; gm <<= 1) {
                        const int gn5 = 8 / gm;
                        if (tm5 % gm || tn5 % gn5) continue;
                        const double cost = (double)p.M * gn5 + (double)p.N * gm;     // x K x 2 bytes
                        if (pl.xcd_gm == 0 || cost < best) {
                            best = cost;
                            pl.xcd_gm = gm;
                        }
                    }
                }
            }
            return done(GR_GEMM5);
        }
    }
    // ---- v3 / v4 (64 / 128-row tiles of 64 / 128 / 160 columns, optional split over K)
    int bn = p.bn ? p.bn : gemm_pick_bn(p.N);
    // Skinny plain GEMMs (the batch-1 step's M = 128..2048 projections): with <= 128 tiles of 64 x 160 most CUs idle while
    // each busy one streams 28.7 KB per slab through its one LDS-DMA path; 64 x 64 tiles spread the same work over 2.5x more CUs
    // at 16 KB per slab: 512x1280x1280 12.8 -> 8.0 us, 128x1280x1280 12.4 -> 7.6 us; batch-1 step +6 % (same box), batch 8 neutral.
    // Measured no better: the same for convs (their split-K already fills the chip: 156.5 vs 163.0 steps/s), 32-row tiles
    // below it (166.2 vs 165.8); thresholds 128 / 256 / 512: 162.0 / 163.6 / 164.2 at B=1, 49.25 / 49.38 / 48.48 at B=8.
    constexpr int skinny_max = 256;
    const bool skinny_ok = !p.conv && p.act != 2 && p.bn == 0 && p.bm == 0 && (p.N % 64) == 0;
    if (skinny_ok) {
        const long long t160 = (long long)((p.M + 63) / 64) * ((p.N + bn - 1) / bn) * p.batch;
        if (t160 <= skinny_max && (p.N + bn - 1) / bn <= 8) bn = 64;      // (wide outputs keep the 160-column tile: 512 x 2560 x 1280 -9 % in the forward)
    }
    // Round 5: the batch-1 step's 1x1 contractions over two sources (ResBlock skip_connection on the concatenated input, the MLP-out fold at
    // K = 3200) take the same 64 x 64 tiles UNSPLIT on the producer / consumer kernel with two workgroups per CU, instead of 64 x 160 tiles
    // split over K + a reduce launch.  Per shape inside the batch-1 forward (profiles/r05_ab_skinny_conv1.txt):
    // 2048 x 640 x 3200 32.2 -> 27.7 us, 2048 x 640 x 1920 26.1 -> 19.4, 512 x 1280 x 2560 25.3 -> 21.4; K = 6400 (100 slabs in one
    // workgroup) loses: 31.8 -> 37.1 us, and as two slices of 3200 + reduce 31.5 -> 34.4 us, so K stops at 3200.  (Without a split there are no GroupNorm partials from the reduce pass: the next
    // GroupNorm runs its own statistics pass — counted in the whole-forward A/B: 5.225 -> 5.207 ms before K was capped.)
    bool skinny_conv1 = false;
    if (p.conv && p.ksize == 1 && p.act == 0 && p.bn == 0 && p.bm == 0 && p.splitk == 0 && p.batch == 1 && (p.N % 64) == 0 && p.SC1 == 0) {
        const long long t64 = (long long)((p.M + 63) / 64) * (p.N / 64);
        if (t64 > 128 && t64 <= 512 && p.K >= 1280 && p.K <= 3200) {
            bn = 64;
            skinny_conv1 = true;
        }
    }
    if (bn != 128 && bn != 160 && bn != 64) return fail(LD_ERR_ARG);
    if (p.act == 2 && (p.N % bn)) return fail(LD_ERR_SHAPE);
    const int tiles_n = (p.N + bn - 1) / bn;
    const int KT = (p.K + BK - 1) / BK;          // 64-wide K slabs
    // Tile height and split-K, fitted to a per-shape sweep of every contraction of the SD1.5 UNet at UNet batch 2 and 16
    // (tools/gemm_sweep.py, profiles/README.md): bigger tiles win whenever they fill the chip; a split only pays when each
    // slice keeps >= ~640 of K (its second pass is a ~6 us launch plus fp32 slab traffic); short-K problems prefer
    // 64-row tiles and no split; long-K problems prefer 128-row tiles and a split up to ~2 blocks per CU.
    const int tiles128 = ((p.M + 127) / 128) * tiles_n * p.batch;
    const bool can_split = p.batch == 1 && p.partial != nullptr;
    const int sk_cap = p.K / 640 < 1 ? 1 : (p.K / 640 > 16 ? 16 : p.K / 640);   // (640: in-forward sweep, tools/ab_shape.py — 128 x 1280 x 2560: split 4 -14 %)
    int bm = p.bm, sk = p.splitk;
    if (bm == 0) {
        // (second and third line re-fitted launch by launch INSIDE the forward, tools/ab_shape.py: an isolated sweep keeps a shape's
        // weights in L2 / MALL and mis-ranks the candidates.  512 x 1280 x 11520: 64-row tiles + split 8 -11 % against 128 / 15;
        // 4096 x 1280 x 1280: 128-row tiles -6 %)
        if (tiles128 >= 512) bm = 128;
        else if (p.K >= 4096 && can_split && (tiles128 >= 128 || (p.K >= 8192 && tiles128 >= 64))) bm = 128;
        else if (!p.conv && tiles128 >= 256) bm = 128;
        else bm = 64;
    }
    if (bn == 64) bm = 64;
    if (skinny_conv1) sk = 1;
    if (bm != 64 && bm != 128) return fail(LD_ERR_ARG);
    const int tiles = ((p.M + bm - 1) / bm) * tiles_n;
    // Convolutions on 64 x 160 tiles with very few tiles (<= 32: the 8 x 8 level of a batch-1 step) or exactly one round of them (256 .. 511)
    // run the 4-stage ring with ONE workgroup per CU and a split aimed at 256 workgroups: three slabs in flight per workgroup hide the
    // HBM latency of their cold weights better than two co-resident 2-stage workgroups (per launch inside the batch-1 forward,
    // tools/ab_launches.py: 128 x 1280 x 11520 24.3 -> 22.2 us, 8192 x 320 x 1600 32 -> 26 us; 64 .. 128 tiles with long K lose 10 %).
    const bool deep = p.conv && bm == 64 && bn == 160 && p.batch == 1 && p.splitk == 0 && (tiles <= 32 || (tiles >= 256 && tiles < 512));
    if (sk == 0) {
        sk = 1;
        if (can_split && tiles * p.batch < 512) {
            sk = ((deep ? 256 : 512) + tiles - 1) / tiles;
            if (sk > sk_cap) sk = sk_cap;
        }
    }
    if (sk > 1) {
        if (p.batch != 1 || p.partial == nullptr) return fail(LD_ERR_ARG);
        while (sk > 1 && (size_t)sk * p.M * p.N * sizeof(float) > p.partial_bytes) --sk;
        if (sk > KT) sk = KT;
    }
    if (p.stat_out != nullptr || p.ln_stat != nullptr) {   // LN fold: v3 / v4 kernels, whole K in one workgroup
        if (p.act == 2 && p.stat_out != nullptr) return fail(LD_ERR_ARG);
        sk = 1;
        pl.stat_parts = tiles_n;
    }
    if (sk < 1) sk = 1;
    pl.bm = bm; pl.bn = bn; pl.splitk = sk;
    pl.grid_x = (unsigned)(tiles * sk); pl.grid_z = (unsigned)p.batch;
    // measured (profiles/r01_b): n-fastest wins on every SD1.5 shape — the 9 taps of a 3x3 conv and the N tiles of one
    // M panel re-read the same activations through the XCD's L2, which matters more than re-streaming the weights
    // Round 5: a plain GEMM with few M panels and a large weight matrix (the batch-1 step's M = 512 GEGLU: 4 panels x 26 MB) walks its tiles
    // M-fastest, so the panels of one N tile run together on one XCD and the weight tile leaves HBM once instead of once per panel
    // (profiles/pmc_traffic.json round 4: 113 MB per launch for 26 MB of weights)
    pl.m_fastest = p.m_fastest;
    if (p.m_fastest < 0) {
        const int tiles_m = (p.M + bm - 1) / bm;
        pl.m_fastest = (!p.conv && p.batch == 1 && tiles_m >= 2 && tiles_m <= 8 && (long long)p.N * p.K * 2 >= (8ll << 20)) ? 1 : 0;
    }
    plan_reduce(p, &pl);
    const long long blocks = (long long)tiles * sk * p.batch;
    {
        // skinny projections with more tiles than CUs: the producer / consumer kernel with two workgroups per CU (see gemm4_kernel, WPS).
        // Measured per launch inside the batch-1 forward (profiles/r05_ab_gemm4_rings.txt): 2048 x 640 x 640
        // (320 tiles, 10 slabs) 14.3 -> 11.7 us against the 2-stage kernel; 8192 x 320 x 320 (640 tiles, 5 slabs) 12.3 -> 14.4: short K stays.
        // An 8-stage ring for <= 256 tiles measured +-0 (512 x 1280 x 1280: 13.6 vs 13.4 us): these launches are not short of bytes in
        // flight — an ablated kernel that only runs its prologue and barriers takes 4.7 of 8.3 us (same record).
        const bool plain_2wg = bn == 64 && !p.conv && blocks > V4_MAX_BLOCKS && blocks <= 512 && p.K >= 640;
        // every unsplit 1x1 convolution that ends on 64 x 64 tiles with at most two workgroups per CU takes the 2wg kernel: the skinny_conv1 shapes
        // and the few-tile shapes of the older skinny_max rule alike
        const bool conv1_2wg = bn == 64 && p.conv && p.ksize == 1 && sk <= 1 && (long long)tiles * p.batch <= 512;
        pl.two_wg = plain_2wg || conv1_2wg;
        if (pl.two_wg) return done(GR_GEMM4);
    }
    // producer/consumer kernel: wins where a plain GEMM leaves at most one workgroup per CU (batch-1 step: +5.6 % whole step,
    // same box A/B); loses on convs and wherever two v3 workgroups share a CU.
    if (!p.conv && blocks <= V4_MAX_BLOCKS) return done(GR_GEMM4);
    pl.deep = deep;   // (64 x 160 convolutions only, by its rule above)
    return done(GR_GEMM3);
}

int gemm_run(const GemmParams& pin, const GemmPlan& pl, hipStream_t stream) {
    if (pl.status != LD_OK) return pl.status;
    if (pl.gn != (pin.gn_scale != nullptr) || (pl.gn && pin.gn_shift == nullptr)) return LD_ERR_ARG;   // (a plan made with gn_offer, run without the operands — or the reverse)
    GemmParams p = pin;
    if (p.conv && p.pad < 0) p.pad = p.ksize >> 1;
    if (p.n_valid <= 0 || p.n_valid > p.N) p.n_valid = p.N;
    const dim3 grid(pl.grid_x, 1, pl.grid_z);
    switch (pl.route) {
        case GR_CONV8:
            if (const int st = conv8_launch(p, pl.c8_S, stream); st != LD_OK) return st;
            break;
        case GR_CONV6:
            p.splitk = pl.splitk;
            if (pl.bn != 32) p.n_valid = p.N;                            // (the 32-column tile stores only the caller's n_valid columns)
            if (pl.splitk == 1 && p.gn_part != nullptr) {                // the tile epilogue writes the GroupNorm partials, or nobody does
                if (pl.gn_chunks > 0) p.gn_P = pl.gn_chunks;
                else p.gn_part = nullptr;
            }
            conv6_launch(p, pl, grid, stream);
            break;
        case GR_UPCONV: {
            // the launch's own view of the problem: rows = source pixels, columns [phase][Cout], K = [2x2 tap][Cin] (the caller's M, N, K stay those
            // of the 3x3 convolution this implements)
            p.W = p.Wup; p.K = 4 * p.C1; p.ldw = p.K; p.M = pin.M / 4; p.N = 4 * pin.N; p.n_valid = p.N;
            p.splitk = pl.splitk; p.bn = 160; p.xcd_gm = 0;
            gemm5_launch(p, pl, grid, stream);
            if (pl.reduce == GRD_UPCONV) {
                if (const int st = upconv_reduce_launch(p, stream); st != LD_OK) return st;   // (misc.hip: an element-wise pass over the slabs)
            }
            return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
        }
        case GR_GEMM7:
            gemm7_launch(p, pl, grid, stream);
            break;
        case GR_GEMM5:
            p.splitk = 1; p.bn = 160; p.xcd_gm = pl.xcd_gm;
            gemm5_launch(p, pl, grid, stream);
            break;
        default:
            p.splitk = pl.splitk; p.bn = pl.bn; p.m_fastest = pl.m_fastest;
            gemm3_launch(p, pl, grid, stream);
            break;
    }
    if (pl.reduce == GRD_GROUPNORM) {
        hipLaunchKernelGGL(splitk_reduce_gn_kernel, dim3(p.gn_P, p.M / p.gn_HW, 4), dim3(256), 0, stream, p);
    } else if (pl.reduce == GRD_PLAIN) {
        const int out_n = p.act == 2 ? p.N / 2 : p.N;
        const long long total = (long long)p.M * (out_n / 8);
        int blocks = (int)((total + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, stream, p, pl.route == GR_CONV6 ? 160 : pl.bn);
    }
    return hipGetLastError() == hipSuccess ? LD_OK : LD_ERR_HIP;
}
