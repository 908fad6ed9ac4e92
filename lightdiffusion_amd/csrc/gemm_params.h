// Where a GemmParams is filled in (host only).  Every contraction the executors (unet.hip, vae.hip) and the operator seam (capi.hip)
// launch is described by one of these builders: they derive every field that follows from the shape, so a caller sets only what the
// shape does not decide (row vector, residual, W8 / Wup, batch and its strides, alpha, bias_m, n_valid).  GemmParams stays a plain aggregate
// (it is passed to the kernels by value): free functions, not members.
#pragma once
#include "kernels.h"

// ksize x ksize NHWC convolution (ksize 1 or 3) of n images over the channel concat of (x1, C1) and (x2, C2; may be null / 0): sources
// Hs x Ws, seen at Hv x Wv through a nearest resize, weights [cout][ksize^2 (C1 + C2)], out NHWC [n][Ho][Wo][cout].
// pad: top / left zero padding, -1 = ksize / 2.  Ho, Wo: 0 = what pad ksize / 2 gives at this stride; explicit for the VAE encoder's
// asymmetrically padded downsampling (bottom / right padding is implied by them).
inline GemmParams conv_params(const half_t* x1, int C1, const half_t* x2, int C2, int n, int Hs, int Ws, int Hv, int Wv, int stride, int ksize,
                              const half_t* w, const half_t* bias, int cout, half_t* out, int pad = -1, int Ho = 0, int Wo = 0) {
    GemmParams p;
    p.conv = 1;
    p.ksize = ksize;
    p.pad = pad;
    p.A = x1; p.A2 = x2; p.C1 = C1; p.C2 = C2;
    p.Hs = Hs; p.Ws = Ws; p.Hv = Hv; p.Wv = Wv; p.stride = stride;
    p.Ho = Ho ? Ho : (ksize == 3 ? (Hv - 1) / stride + 1 : Hv);
    p.Wo = Wo ? Wo : (ksize == 3 ? (Wv - 1) / stride + 1 : Wv);
    p.M = n * p.Ho * p.Wo; p.N = cout; p.K = ksize * ksize * (C1 + C2);
    p.W = w; p.ldw = p.K;
    p.bias_n = bias;
    p.rows_per_vec = p.Ho * p.Wo;   // (a row vector, where the caller sets one, is per image)
    p.ldr = cout;
    p.C = out; p.ldc = cout;
    return p;
}

// y[M][N] = act(x[M][K] · w[N][K]^T + bias): plain, act (1 SiLU, 3 quick-GELU) or GEGLU (act 2: y is [M][N / 2], w / bias rows
// tile-interleaved with `bn`, gemm_pick_bn).  A residual, where the caller sets one, has the output's row pitch.  ldw: w's row pitch, 0 = K.
inline GemmParams linear_params(const half_t* x, int lda, const half_t* w, const half_t* bias, int M, int N, int K, half_t* y, int act = 0, int bn = 0,
                                int ldw = 0) {
    GemmParams p;
    p.A = x; p.lda = lda;
    p.W = w; p.ldw = ldw ? ldw : K;
    p.M = M; p.N = N; p.K = K;
    p.bias_n = bias;
    p.act = act; p.bn = bn;
    p.C = y; p.ldc = p.ldr = (act == 2 ? N / 2 : N);
    return p;
}

// GroupNorm partial statistics of p's output (gemm.h gn_part), n images of HW pixels, for the GroupNorm that reads the output next: where the
// launch can emit them (its split-K second pass, the halo tile's epilogue, the row-resident kernel) its plan's gn_chunks is the chunk count
// per image and that GroupNorm skips its statistics launch; otherwise gn_chunks is 0
inline void want_gn_partials(GemmParams& p, int n, int HW, float* buf) {
    p.gn_part = buf;
    p.gn_P = gn_num_chunks(n, HW);
    p.gn_HW = HW;
    p.gn_ppb = (HW + p.gn_P - 1) / p.gn_P;
}
// ... from the kernels that sum what they store (halo-tile epilogue, row-resident kernel) only: without the chunk geometry a split over K
// keeps its plain second pass (gemm.hip plan_reduce asks for gn_P).  The VAE's form; not equivalent to the one above, which would move a
// convolution of the VAE that splits over K onto the reduce pass that also writes statistics.
inline void want_gn_tile_partials(GemmParams& p, float* buf) { p.gn_part = buf; }

// A 1x1 convolution over the raw sources (s1, sc1) and (s2, sc2; may be null / 0) of the output's size, appended to the 3x3 convolution p
// as a second K segment (gemm.h S1 / S2): wfold = [W | Wskip] ([N][K + sc1 + sc2]) and bfold = b + bskip (skip_fold_launch).  The sum
// replaces p's residual; the row-resident kernel has no such segment.
inline void add_skip_segment(GemmParams& p, const half_t* s1, int sc1, const half_t* s2, int sc2, const half_t* wfold, const half_t* bfold) {
    p.S1 = s1; p.SC1 = sc1; p.S2 = s2; p.SC2 = sc2;
    p.K = p.ksize * p.ksize * (p.C1 + p.C2) + sc1 + sc2;
    p.W = wfold; p.ldw = p.K;
    p.bias_n = bfold;
    p.R = nullptr;
    p.W8 = nullptr;
}

// LayerNorm fold (gemm.h stat_out / ln_stat).  Producer: the GEMM that writes the residual stream also writes per-row (sum, sum of squares)
// partials of its fp16 outputs to `stat`, in as many parts per row as its plan's stat_parts says
inline void ln_producer(GemmParams& p, float* stat) { p.stat_out = stat; }
// Consumer: a projection of LayerNorm(x; eps) over C channels on the gamma / beta-folded weights (ln_fold_launch; wsum their fp32 row sums),
// finished on the accumulators from the producer's `parts` partials per row of its `rows` rows
inline void ln_consumer(GemmParams& p, const float* stat, int parts, int rows, int C, float eps, const float* wsum) {
    p.ln_stat = stat; p.ln_parts = parts; p.ln_rows = rows;
    p.ln_inv_c = 1.0f / (float)C; p.ln_eps = eps;
    p.ln_wsum = wsum;
}
