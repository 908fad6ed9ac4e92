// Single-operator entry points of the C ABI (include/ld_mi355x.h) — thin, argument-checked wrappers over the
// kernel launchers; used by the parity tests and by hosts that want to compose their own graphs.
#include <string>

#include "runtime.h"
#include "../../include/ld_mi355x.h"

namespace {
inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// ld_op_last_kernel: the contraction instantiations the calling thread's last ld_op_* call dispatched, in launch order, joined with ';'
thread_local std::string t_op_kernels;
// ld_op_last_launches: every launch of that call under the name the executors' profile tables print for it, norm and misc launches included
thread_local std::string t_op_launches;
inline void op_begin() {
    t_op_kernels.clear();
    t_op_launches.clear();
}
inline int noted(int st, const char* name) {
    note_kernel(&t_op_kernels, name);
    return st;
}
// a launcher called directly (no Exec): the name the executors time that launch under
inline int launched(int st, const char* table_name) {
    if (st == LD_OK) note_kernel(&t_op_launches, table_name);
    return st;
}

constexpr size_t kSyncBytes = LD_SYNC_INTS * sizeof(int);
constexpr size_t kCompositeSplitBytes = (size_t)96 << 20;   // split-K partials of the GroupNorm / skip composites: what the executors reserve
// the row-resident kernel's (conv8.hip) share of a caller's scratch: the counters of its in-launch reduction and, where the shape can have one, a
// copy of the weights in its layout
inline size_t conv8_scratch_head(int cout, int cin) { return kSyncBytes + (conv8_weight_eligible(cout, cin) ? align256(conv8_weight_bytes(cout, cin)) : 0); }

// One ld_op_* call: an Exec (runtime.h) over the caller's scratch.  The arena's base is the `ws` pointer, the split-K partials, the counters
// and the row-resident kernel's weight copy are carved from it, and the name sink is ld_op_last_kernel's string — so the operators launch
// through Exec::gemm / Exec::attention / Exec::gn_silu_conv, the functions the UNet and VAE executors run.  (The scratch handed to a launch
// decides its split over K, so the sizes carved here are part of an operator's route: tests/test_cabi_cpu.py pins what *_ws_bytes returns.)
struct Op {
    Arena arena;
    Exec ex;
    Op(void* ws, size_t ws_bytes, void* stream) {
        arena.base = (char*)ws;
        arena.cap = ws != nullptr ? ws_bytes : 0;
        ex.arena = &arena;
        ex.stream = (hipStream_t)stream;
        ex.names = &t_op_kernels;
        ex.all_names = &t_op_launches;
    }
    Op(const Op&) = delete;
    bool fits() const { return align256(arena.peak) <= arena.cap; }   // everything carved so far lies inside the caller's buffer
    // split-K partials: `bytes` of the scratch, or all that is left of it
    void splitk(size_t bytes) {
        ex.splitk_ws = (float*)arena.alloc(bytes);
        ex.splitk_bytes = bytes;
    }
    void splitk_rest() {
        const size_t at = align256(arena.off);
        if (arena.base != nullptr && at <= arena.cap) splitk(arena.cap - at);
    }
    // The row-resident kernel (conv8.hip) from a caller's scratch: counters | weight copy (p.W8, where the shape can have one) | split partials.
    // In front of that kernel, and of no other, a caller's scratch needs per call: the counters zeroed (not known to be zero) and the weights
    // `wt` repacked (the UNet executor keeps that copy resident)
    void conv8_scratch(GemmParams& p, const void* wt, size_t partial_bytes) {
        const int cin = p.C1 + p.C2;
        ex.sync_ws = (int*)arena.alloc(kSyncBytes);
        p.W8 = conv8_weight_eligible(p.N, cin) ? (const half_t*)arena.alloc(conv8_weight_bytes(p.N, cin)) : nullptr;
        splitk(partial_bytes);
        ex.before_gemm = [](const GemmParams& q, const GemmPlan& plan, const void* wt, hipStream_t s) {
            if (plan.route != GR_CONV8) return (int)LD_OK;
            if (hipMemsetAsync(q.sync, 0, kSyncBytes, s) != hipSuccess) return (int)LD_ERR_HIP;
            return conv8_repack_launch((const half_t*)wt, q.N, q.C1 + q.C2, const_cast<half_t*>(q.W8), s);
        };
        ex.before_gemm_arg = wt;
    }
};
}  // namespace

extern "C" {

const char* ld_version(void) { return "ld_mi355x 0.1 (gfx950)"; }

const char* ld_op_last_kernel(void) { return t_op_kernels.c_str(); }

const char* ld_op_last_launches(void) { return t_op_launches.c_str(); }

const char* ld_status_string(int s) {
    switch (s) {
        case LD_OK: return "ok";
        case LD_ERR_ARG: return "invalid argument";
        case LD_ERR_SHAPE: return "unsupported shape or alignment";
        case LD_ERR_HIP: return "HIP runtime error";
        case LD_ERR_STATE: return "invalid call order (weights / reserve / context missing)";
        default: return "unknown status";
    }
}

int ld_op_linear(const void* x, const void* w, const void* bias, const void* residual, void* y, int M, int N, int K, float alpha,
                 int act, void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    Op op(ws, ws_bytes, stream);
    GemmParams p = linear_params((const half_t*)x, K, (const half_t*)w, (const half_t*)bias, M, N, K, (half_t*)y, act);
    p.alpha = alpha;
    p.R = (const half_t*)residual;
    if (act == 2) {   // the op takes weights in checkpoint row order: repack [value | gate] rows into the tile-interleaved order the fused epilogue expects
        if (bias == nullptr || (N & 15)) return LD_ERR_ARG;
        const int bn = gemm_pick_bn(N);
        if (N % bn) return LD_ERR_SHAPE;
        half_t* w2 = op.arena.halfs((size_t)N * K);
        half_t* b2 = op.arena.halfs((size_t)N);
        if (ws == nullptr || !op.fits()) return LD_ERR_ARG;
        int st = repack_rows_launch(w, 0, N, K, w2, bn, op.ex.stream);
        if (st != LD_OK) return st;
        st = repack_rows_launch(bias, 0, N, 1, b2, bn, op.ex.stream);
        if (st != LD_OK) return st;
        p.W = w2;
        p.bias_n = b2;
        p.bn = bn;
    }
    op.splitk_rest();
    op.ex.gemm(p);
    return op.ex.status;
}

// What ld_op_conv / ld_op_conv_gn_partials take beyond the symmetric convolution: pad (top / left zeros, -1 = ksize / 2) with an explicit
// output size ho x wo (0 = what pad ksize / 2 gives; the bottom / right zeros follow from it — the VAE encoder's Downsample), n_valid rows of
// wt that exist (0 = cout) stored at a row pitch of ldc (0 = cout) — the VAE's padded output convolution — and the executor whose launch it is.
struct ConvGeom {
    int pad = -1, ho = 0, wo = 0, n_valid = 0, ldc = 0, form = LD_FORM_UNET;
    bool ok(int ksize, int cout) const {
        if (pad < -1 || pad > ksize / 2 || ho < 0 || wo < 0 || (ho == 0) != (wo == 0)) return false;
        if (n_valid < 0 || n_valid > cout || ldc < 0 || (ldc & 7) || (ldc > 0 && ldc < (n_valid > 0 ? n_valid : cout))) return false;
        return form == LD_FORM_UNET || form == LD_FORM_VAE;
    }
};

int ld_op_linear_batched(const void* x, int lda, const void* w, int ldw, const void* bias, const void* bias_m, void* y, int M, int N, int K, int n_valid,
                         float alpha, int batch, long long sA, long long sW, long long sC, void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    // the batched contractions of the VAE's attention at a width without a flash kernel (vae.hip VRun::attn), by the same builder: rows
    // n_valid .. N-1 of w read as zeros, a bias along the rows of y, one problem per batch element at the three strides
    if (x == nullptr || w == nullptr || y == nullptr || batch < 1 || n_valid < 0 || n_valid > N || sA < 0 || sW < 0 || sC < 0) return LD_ERR_ARG;
    GemmParams p = linear_params((const half_t*)x, lda, (const half_t*)w, (const half_t*)bias, M, N, K, (half_t*)y, 0, 0, ldw);
    p.n_valid = n_valid; p.bias_m = (const half_t*)bias_m; p.alpha = alpha;
    p.batch = batch; p.sA = sA; p.sW = sW; p.sC = sC;
    Op op(ws, ws_bytes, stream);
    op.splitk_rest();
    op.ex.gemm(p);
    return op.ex.status;
}

static int op_conv(const void* x1, int c1, const void* x2, int c2, int n, int h, int w, int hv, int wv, int stride, int ksize,
                   const void* wt, const void* bias, const void* rowvec, const void* residual, void* y, int cout, void* ws,
                   size_t ws_bytes, void* stream, float* gn_part, int* gn_chunks, const void* wup = nullptr, const ConvGeom& g = ConvGeom()) {
    if (stride < 1 || (ksize != 1 && ksize != 3)) return LD_ERR_ARG;
    if (!g.ok(ksize, cout)) return LD_ERR_ARG;
    GemmParams p = conv_params((const half_t*)x1, c1, (const half_t*)x2, c2, n, h, w, hv, wv, stride, ksize, (const half_t*)wt, (const half_t*)bias, cout, (half_t*)y,
                               g.pad, g.ho, g.wo);
    p.Wup = (const half_t*)wup;
    p.rowvec = (const half_t*)rowvec; p.ldrv = cout;
    p.R = (const half_t*)residual;
    if (g.n_valid > 0) p.n_valid = g.n_valid;
    if (g.ldc > 0) p.ldc = p.ldr = g.ldc;
    // the close of every route below: the chunk count of the launch's plan to the caller, the executor's status back
    const auto ran = [gn_chunks](const Op& o, const GemmPlan& pl) {
        if (gn_chunks != nullptr) *gn_chunks = pl.gn_chunks;
        return o.ex.status;
    };
    if (g.form == LD_FORM_VAE) {
        // the VAE executor's launch (vae.hip VRun::conv): statistics from the kernels that sum what they store only, no chunk geometry; its scratch
        // is the split partials alone — no counters and no weight copy, so the row-resident kernel is never offered
        if (gn_part != nullptr) want_gn_tile_partials(p, gn_part);
        Op op(ws, ws_bytes, stream);
        op.splitk(kCompositeSplitBytes);
        if (ws == nullptr || !op.fits()) return LD_ERR_ARG;
        if (p.ldc < p.N) {
            // fewer stored columns than weight rows: only the halo tile's 32-column tile stores n_valid columns; every other kernel stores all N
            // at the pitch ldc (the executor asks the plan first, and so does this)
            const GemmPlan pl = op.ex.plan(p);
            if (!(pl.halo_tile && pl.bn == 32 && p.n_valid > 0 && p.n_valid <= p.ldc)) return LD_ERR_SHAPE;
            return ran(op, op.ex.gemm(p, &pl));
        }
        return ran(op, op.ex.gemm(p));
    }
    if (p.ldc < p.N) return LD_ERR_SHAPE;   // (the narrow store is the VAE output convolution's)
    if (gn_part != nullptr) want_gn_partials(p, n, p.Ho * p.Wo, gn_part);   // (as the executors ask)
    const size_t head = conv8_scratch_head(cout, c1 + c2);
    if (ws != nullptr && ksize == 3 && conv8_weight_eligible(cout, c1 + c2) && ws_bytes > head + ((size_t)8 << 20)) {
        // a roomy scratch buffer: the row-resident kernel where it takes the shape, by a carving of its own; the general kernels keep the
        // whole buffer for their split
        Op c8(ws, ws_bytes, stream);
        GemmParams q = p;
        c8.conv8_scratch(q, wt, ws_bytes - head);
        if (const GemmPlan plan = c8.ex.plan(q); plan.route == GR_CONV8) return ran(c8, c8.ex.gemm(q, &plan));
    }
    Op op(ws, ws_bytes, stream);
    op.splitk_rest();
    return ran(op, op.ex.gemm(p));
}

int ld_op_conv(const void* x1, int c1, const void* x2, int c2, int n, int h, int w, int hv, int wv, int stride, int ksize,
               const void* wt, const void* bias, const void* rowvec, const void* residual, void* y, int cout, int pad, int ho, int wo, int n_valid,
               int ldc, int form, void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    ConvGeom g;
    g.pad = pad; g.ho = ho; g.wo = wo; g.n_valid = n_valid; g.ldc = ldc; g.form = form;
    return op_conv(x1, c1, x2, c2, n, h, w, hv, wv, stride, ksize, wt, bias, rowvec, residual, y, cout, ws, ws_bytes, stream, nullptr, nullptr, nullptr, g);
}

int ld_op_upconv2x_fold(const void* wt, int cout, int cin, void* wfold, void* stream) {
    op_begin();
    return upconv_fold_launch((const half_t*)wt, cout, cin, (half_t*)wfold, (hipStream_t)stream);
}

int ld_op_upconv2x(const void* x, int c, int n, int h, int w, int hv, int wv, const void* wt, const void* wfold, const void* bias, void* y, int cout,
                   void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    // Upsample1 as the UNet executor runs it (unet.hip L_UP: the same builder, the same Exec::gemm): the folded weights are an offer that the
    // planner takes for an exact 2x resize of more than two images; every other case is ld_op_conv's route
    if (wfold == nullptr) return LD_ERR_ARG;
    return op_conv(x, c, nullptr, 0, n, h, w, hv, wv, 1, 3, wt, bias, nullptr, nullptr, y, cout, ws, ws_bytes, stream, nullptr, nullptr, wfold);
}

size_t ld_op_conv_gn_partials_floats(int n, int hw) {
    op_begin();
    return groupnorm_workspace_bytes(n, hw) / sizeof(float);
}

int ld_op_conv_gn_partials(const void* x, int c, const void* x2, int c2, int n, int h, int w, int hv, int wv, int stride, int ksize, const void* wt,
                           const void* bias, const void* residual, void* y, int cout, int pad, int ho, int wo, int n_valid, int ldc, int form, float* part,
                           int* chunks, void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    if (part == nullptr || chunks == nullptr) return LD_ERR_ARG;
    *chunks = 0;
    ConvGeom g;
    g.pad = pad; g.ho = ho; g.wo = wo; g.n_valid = n_valid; g.ldc = ldc; g.form = form;
    return op_conv(x, c, x2, c2, n, h, w, hv, wv, stride, ksize, wt, bias, nullptr, residual, y, cout, ws, ws_bytes, stream, part, chunks, nullptr, g);
}

int ld_op_vae_conv_out_takes_halo_tile(int c, int n, int h, int w, int out_ch) {
    op_begin();
    // what vae.hip run_decode asks of its output convolution: the weights zero-padded to 32 rows, 8 stored columns, planned under the VAE's
    // scratch.  Host only: the plan reads no operand, so any non-null address stands for them.
    if (c <= 0 || n <= 0 || h <= 0 || w <= 0 || out_ch <= 0 || out_ch > 8) return 0;
    static const half_t any[8] = {};
    GemmParams q = conv_params(any, c, nullptr, 0, n, h, w, h, w, 1, 3, any, any, 32, const_cast<half_t*>(any));
    q.n_valid = 8; q.ldc = 8;
    Exec ex;
    ex.splitk_ws = reinterpret_cast<float*>(const_cast<half_t*>(any));
    ex.splitk_bytes = kCompositeSplitBytes;
    return ex.plan(q).halo_tile ? 1 : 0;
}

int ld_op_conv_takes_skip_segment(int c, int n, int h, int w, int cout) {
    op_begin();
    // what unet.hip Run::resblock asks of out_layers' convolution as it stands before the skip joins it (Exec::conv_takes_skip_segment), under
    // the scratch every executor launch has: split partials, counters and, where the shape can have one, the row-resident kernel's weight copy.
    // Host only: the plan reads no operand, so any non-null address stands for them.
    if (c <= 0 || n <= 0 || h <= 0 || w <= 0 || cout <= 0) return 0;
    static const half_t any[8] = {};
    GemmParams p = conv_params(any, c, nullptr, 0, n, h, w, h, w, 1, 3, any, any, cout, const_cast<half_t*>(any));
    p.W8 = conv8_weight_eligible(cout, c) ? any : nullptr;
    Exec ex;
    ex.splitk_ws = reinterpret_cast<float*>(const_cast<half_t*>(any));
    ex.splitk_bytes = kCompositeSplitBytes;
    ex.sync_ws = reinterpret_cast<int*>(const_cast<half_t*>(any));
    return ex.conv_takes_skip_segment(p) ? 1 : 0;
}

size_t ld_op_groupnorm_conv_ws_bytes(int c1, int c2, int n, int h, int w, int cout) {
    op_begin();
    const size_t C = (size_t)c1 + c2, HW = (size_t)h * w;
    return align256(groupnorm_workspace_bytes(n, (int)HW)) + 2 * align256((size_t)n * C * sizeof(float)) + align256((size_t)n * HW * C * sizeof(half_t)) +
           conv8_scratch_head(cout, c1 + c2) + kCompositeSplitBytes;
}

int ld_op_groupnorm_conv(const void* x1, int c1, const void* x2, int c2, int n, int h, int w, const void* gamma, const void* beta, float eps,
                         const void* wt, const void* bias, const void* rowvec, const void* residual, void* y, int cout, float* in_part, int in_chunks,
                         float* part, int* chunks, int form, void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    if (form != LD_FORM_UNET && form != LD_FORM_VAE) return LD_ERR_ARG;
    // in_part / in_chunks: GroupNorm partial statistics of x1 that its producer wrote ([n][in_chunks][32][2]; one source only): the statistics
    // pass is skipped, as in Run::resblock.  part / chunks (both or neither): the partial statistics of y, as ld_op_conv_gn_partials.
    if ((part == nullptr) != (chunks == nullptr) || in_chunks < 0 || (in_part != nullptr && (in_chunks == 0 || c2 != 0))) return LD_ERR_ARG;
    if (chunks != nullptr) *chunks = 0;
    // GroupNorm(32) + SiLU + 3x3 convolution (stride 1, pad 1): the reference's ResBlock1.in_layers / out_layers (LD.py:5224-5262), by
    // Exec::gn_silu_conv — fused into the halo tile's loader where the plan says so, else the two-pass GroupNorm (which the row-resident kernel
    // takes too), then the convolution.  The scratch: normalised tensor | counters | weight copy | split partials | statistics, scale, shift.
    if (x1 == nullptr || gamma == nullptr || beta == nullptr || wt == nullptr || y == nullptr || ws == nullptr) return LD_ERR_ARG;
    if (ws_bytes < ld_op_groupnorm_conv_ws_bytes(c1, c2, n, h, w, cout)) return LD_ERR_ARG;
    Op op(ws, ws_bytes, stream);
    half_t* g = op.arena.halfs((size_t)n * h * w * (c1 + c2));
    GemmParams p = conv_params((const half_t*)x1, c1, (const half_t*)x2, c2, n, h, w, h, w, 1, 3, (const half_t*)wt, (const half_t*)bias, cout, (half_t*)y);
    p.rowvec = (const half_t*)rowvec; p.ldrv = cout;
    p.R = (const half_t*)residual;
    if (form == LD_FORM_VAE) {   // vae.hip VRun::gn_conv: the tile epilogue's statistics or none, split partials as the only scratch
        if (part != nullptr) want_gn_tile_partials(p, part);
        op.splitk(kCompositeSplitBytes);
    } else {
        if (part != nullptr) want_gn_partials(p, n, h * w, part);
        op.conv8_scratch(p, wt, kCompositeSplitBytes);
    }
    const GemmPlan pl = op.ex.gn_silu_conv(p, n, h * w, (const half_t*)gamma, (const half_t*)beta, eps, g, gn_stats(in_part, in_chunks));
    if (chunks != nullptr) *chunks = pl.gn_chunks;
    return op.ex.status;
}

size_t ld_op_conv_skip_ws_bytes(int c, int sc1, int sc2, int cout) {
    op_begin();
    return align256((size_t)cout * (9 * (size_t)c + sc1 + sc2) * sizeof(half_t)) + align256((size_t)cout * sizeof(half_t)) + kCompositeSplitBytes;
}

// ResBlock1's out_layers as the executor runs them (unet.hip Run::resblock; the same builders, add_skip_segment and Exec::gn_silu_conv):
// [GroupNorm + SiLU of x] + 3x3 convolution + the 1x1 skip_connection over s1 / s2 as a second K segment, one contraction on the folded weights.
// gamma / beta null: x is taken as it is.  part / chunks (optional): the GroupNorm partial statistics of the OUTPUT where the launch writes
// them (as ld_op_conv_gn_partials).  The scratch: folded weights | folded bias | [normalised tensor] | split partials | [statistics, scale, shift].
static int op_conv_skip(const void* x, int c, int n, int h, int w, const void* wt, const void* bias, const void* s1, int sc1, const void* s2, int sc2,
                        const void* wskip, const void* bskip, const void* rowvec, const void* gamma, const void* beta, float eps, void* y, int cout,
                        float* in_part, int in_chunks, float* part, int* chunks, void* ws, size_t ws_bytes, void* stream) {
    Op op(ws, ws_bytes, stream);
    const int K9 = 9 * c, SC = sc1 + sc2, HW = h * w;
    half_t* wf = op.arena.halfs((size_t)cout * (K9 + SC));
    half_t* bf = op.arena.halfs((size_t)cout);
    const int st = skip_fold_launch((const half_t*)wt, (const half_t*)wskip, (const half_t*)bias, (const half_t*)bskip, cout, K9, SC, wf, bf, op.ex.stream);
    if (st != LD_OK) return st;
    GemmParams p = conv_params((const half_t*)x, c, nullptr, 0, n, h, w, h, w, 1, 3, (const half_t*)wt, (const half_t*)bias, cout, (half_t*)y);
    add_skip_segment(p, (const half_t*)s1, sc1, (const half_t*)s2, sc2, wf, bf);
    p.rowvec = (const half_t*)rowvec; p.ldrv = cout;
    if (part != nullptr) want_gn_partials(p, n, HW, part);
    GemmPlan pl;
    if (gamma == nullptr) {
        op.splitk(kCompositeSplitBytes);
        pl = op.ex.gemm(p);
    } else {
        half_t* g = op.arena.halfs((size_t)n * HW * c);
        op.splitk(kCompositeSplitBytes);
        pl = op.ex.gn_silu_conv(p, n, HW, (const half_t*)gamma, (const half_t*)beta, eps, g, gn_stats(in_part, in_chunks));
    }
    if (chunks != nullptr) *chunks = pl.gn_chunks;
    return op.ex.status;
}

int ld_op_conv_skip(const void* x, int c, int n, int h, int w, const void* wt, const void* bias, const void* s1, int sc1, const void* s2, int sc2,
                    const void* wskip, const void* bskip, const void* rowvec, void* y, int cout, void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    if (x == nullptr || wt == nullptr || bias == nullptr || s1 == nullptr || wskip == nullptr || bskip == nullptr || y == nullptr || ws == nullptr) return LD_ERR_ARG;
    if (c <= 0 || sc1 <= 0 || sc2 < 0 || (sc2 > 0 && s2 == nullptr) || cout <= 0 || n <= 0 || h <= 0 || w <= 0) return LD_ERR_ARG;
    if (ws_bytes < ld_op_conv_skip_ws_bytes(c, sc1, sc2, cout)) return LD_ERR_ARG;
    return op_conv_skip(x, c, n, h, w, wt, bias, s1, sc1, s2, sc2, wskip, bskip, rowvec, nullptr, nullptr, 0.f, y, cout, nullptr, 0, nullptr, nullptr, ws, ws_bytes, stream);
}

size_t ld_op_groupnorm_conv_skip_ws_bytes(int c, int sc1, int sc2, int cout, int n, int h, int w) {
    op_begin();
    const size_t HW = (size_t)h * w;
    return ld_op_conv_skip_ws_bytes(c, sc1, sc2, cout) + align256(groupnorm_workspace_bytes(n, (int)HW)) + 2 * align256((size_t)n * c * sizeof(float)) +
           align256((size_t)n * HW * c * sizeof(half_t));
}

int ld_op_groupnorm_conv_skip(const void* x, int c, int n, int h, int w, const void* gamma, const void* beta, float eps, const void* wt, const void* bias,
                              const void* s1, int sc1, const void* s2, int sc2, const void* wskip, const void* bskip, const void* rowvec, void* y, int cout,
                              float* in_part, int in_chunks, float* part, int* chunks, void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    // in_part / in_chunks: GroupNorm partial statistics of x from its producer ([n][in_chunks][32][2]), as ld_op_groupnorm_conv
    if (in_chunks < 0 || (in_part != nullptr && (in_chunks == 0 || gamma == nullptr))) return LD_ERR_ARG;
    if (x == nullptr || wt == nullptr || bias == nullptr || s1 == nullptr || wskip == nullptr || bskip == nullptr || y == nullptr || ws == nullptr) return LD_ERR_ARG;
    if (c <= 0 || sc1 <= 0 || sc2 < 0 || (sc2 > 0 && s2 == nullptr) || cout <= 0 || n <= 0 || h <= 0 || w <= 0) return LD_ERR_ARG;
    if ((gamma == nullptr) != (beta == nullptr) || (part == nullptr) != (chunks == nullptr)) return LD_ERR_ARG;
    if (ws_bytes < ld_op_groupnorm_conv_skip_ws_bytes(c, sc1, sc2, cout, n, h, w)) return LD_ERR_ARG;
    if (chunks != nullptr) *chunks = 0;
    return op_conv_skip(x, c, n, h, w, wt, bias, s1, sc1, s2, sc2, wskip, bskip, rowvec, gamma, beta, eps, y, cout, in_part, in_chunks, part, chunks, ws, ws_bytes, stream);
}

int ld_op_repack_conv(const void* src, int dtype, int cout, int cin, void* dst, void* stream) {
    op_begin();
    return repack_conv3x3_launch(src, dtype == LD_F32, cout, cin, (half_t*)dst, (hipStream_t)stream);
}

size_t ld_op_groupnorm_ws_bytes(int n, int hw) {
    op_begin();
    return groupnorm_workspace_bytes(n, hw);
}

int ld_op_groupnorm(const void* x1, int c1, const void* x2, int c2, int n, int hw, const void* gamma, const void* beta, float eps,
                    int silu, void* y, void* ws, void* stream) {
    op_begin();
    return launched(groupnorm_launch((const half_t*)x1, c1, (const half_t*)x2, c2, n, hw, (const half_t*)gamma, (const half_t*)beta, eps,
                                     silu, (half_t*)y, (float*)ws, (hipStream_t)stream), "gn_stats_kernel+gn_apply_kernel");
}

int ld_op_layernorm(const void* x, const void* gamma, const void* beta, void* y, int rows, int c, float eps, void* stream) {
    op_begin();
    return launched(layernorm_launch((const half_t*)x, (const half_t*)gamma, (const half_t*)beta, (half_t*)y, rows, c, eps, (hipStream_t)stream),
                    "layernorm_kernel");
}

int ld_op_attention(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo, int b, int heads,
                    int lq, int lk, int d, float scale, int causal, void* stream) {
    op_begin();
    AttnParams a;
    a.Q = (const half_t*)q; a.ldq = ldq; a.sQ = (long long)lq * ldq;
    a.K = (const half_t*)k; a.ldk = ldk; a.sK = (long long)lk * ldk;
    a.Vt = (const half_t*)vt; a.ldvt = ldvt; a.sV = (long long)heads * d * ldvt;
    a.O = (half_t*)o; a.ldo = ldo; a.sO = (long long)lq * ldo;
    a.B = b; a.H = heads; a.Lq = lq; a.Lk = lk; a.d = d; a.scale = scale; a.causal = causal;
    Op op(nullptr, 0, stream);
    op.ex.attention(a);
    return op.ex.status;
}

int ld_op_attention_rowv(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int b, int heads,
                         int lq, int lk, int d, float scale, int causal, void* stream) {
    op_begin();
    // q, k, v as column blocks of one fused [b][l][ldq] tensor (ldq == ldk == ldv with overlapping row ranges) share ONE batch stride,
    // which the per-operand strides below only reproduce when lq == lk
    const char *qb = (const char*)q, *kb = (const char*)k, *vb = (const char*)v;
    const long long rowb = (long long)ldq * 2;
    const bool fused = ldq == ldk && ldk == ldv && rowb > 0 && (kb - qb >= 0 ? kb - qb : qb - kb) < rowb && (vb - qb >= 0 ? vb - qb : qb - vb) < rowb;
    if (fused && lq != lk) return LD_ERR_SHAPE;
    AttnParams a;
    a.Q = (const half_t*)q; a.ldq = ldq; a.sQ = (long long)lq * ldq;
    a.K = (const half_t*)k; a.ldk = ldk; a.sK = (long long)lk * ldk;
    a.V = (const half_t*)v; a.ldv = ldv; a.sV = (long long)lk * ldv;
    a.O = (half_t*)o; a.ldo = ldo; a.sO = (long long)lq * ldo;
    a.B = b; a.H = heads; a.Lq = lq; a.Lk = lk; a.d = d; a.scale = scale; a.causal = causal;
    Op op(nullptr, 0, stream);
    op.ex.attention(a);
    return op.ex.status;
}

int ld_op_softmax_rows(void* s, int rows, int cols, void* stream) {
    op_begin();
    return softmax_rows_launch((half_t*)s, rows, cols, cols, (hipStream_t)stream);
}

int ld_op_timestep_embed(const float* sigma, const float* log_sigmas, int n_sigmas, int n, int dim, void* out, float* t_out, void* stream) {
    op_begin();
    return timestep_embed_launch(sigma, log_sigmas, n_sigmas, n, dim, (half_t*)out, t_out, (hipStream_t)stream);
}

int ld_op_cfg_combine(const float* den2, float* out, float cfg, size_t n_half, void* stream) {
    op_begin();
    return cfg_combine_launch(den2, out, cfg, n_half, (hipStream_t)stream);
}

int ld_op_hook_check(const void* a, const void* b, size_t words_ab, const void* x, size_t half_words_x, const void* sigma, int half_sigma,
                     int* flags, int epoch, void* stream) {
    op_begin();
    return hook_check_launch(a, b, words_ab, x, half_words_x, sigma, half_sigma, flags, epoch, (hipStream_t)stream);
}

int ld_op_axpby(float* x, float a, const float* y, float b, const float* z, float c, size_t n, void* stream) {
    op_begin();
    return axpby_launch(x, a, y, b, z, c, n, (hipStream_t)stream);
}

// ---- the norm, boundary-convolution and fold kernels on their own (tests/test_norm_gpu.py, tests/test_small_kernels_gpu.py)
int ld_op_softmax_rows_ld(void* s, int rows, int cols, long long ld, int valid, void* stream) {
    op_begin();
    if (valid < 0 || ld < cols) return LD_ERR_SHAPE;
    return launched(softmax_rows_launch((half_t*)s, rows, cols, ld, (hipStream_t)stream, valid), "softmax_rows_kernel");
}

int ld_op_groupnorm_chunks(int n, int hw) {
    op_begin();
    return gn_num_chunks(n, hw);
}

int ld_op_groupnorm_stats(const void* x1, int c1, const void* x2, int c2, int n, int hw, float* part, void* stream) {
    op_begin();
    return groupnorm_stats_launch((const half_t*)x1, c1, (const half_t*)x2, c2, n, hw, part, (hipStream_t)stream);
}

int ld_op_groupnorm_from_partials(const void* x1, int c1, const void* x2, int c2, int n, int hw, const void* gamma, const void* beta, float eps,
                                  int silu, void* y, float* part, int pstat, void* stream) {
    op_begin();
    if (pstat < 1) return LD_ERR_ARG;
    return launched(groupnorm_launch((const half_t*)x1, c1, (const half_t*)x2, c2, n, hw, (const half_t*)gamma, (const half_t*)beta, eps, silu, (half_t*)y, part,
                                     (hipStream_t)stream, pstat), "gn_apply_kernel");
}

int ld_op_groupnorm_scale_shift(const void* x1, int c1, const void* x2, int c2, int n, int hw, const void* gamma, const void* beta, float eps,
                                float* ws, int stats_ready, float* scale, float* shift, void* stream) {
    op_begin();
    if (stats_ready < 0) return LD_ERR_ARG;
    return groupnorm_scale_shift_launch((const half_t*)x1, c1, (const half_t*)x2, c2, n, hw, (const half_t*)gamma, (const half_t*)beta, eps, ws, scale,
                                        shift, (hipStream_t)stream, stats_ready);
}

int ld_op_small_conv_in(const float* x, const float* scale_sigma, const void* pre_w, const void* pre_b, const void* wt, const void* bias, void* y,
                        int n, int cin, int h, int w, int cout, long long dup_off, void* stream) {
    op_begin();
    if ((pre_w == nullptr) != (pre_b == nullptr) || n <= 0 || h <= 0 || w <= 0 || (dup_off & 7)) return LD_ERR_ARG;
    SmallConvInArgs a;
    a.x = x; a.scale_sigma = scale_sigma; a.pre_w = (const half_t*)pre_w; a.pre_b = (const half_t*)pre_b;
    a.w = (const half_t*)wt; a.b = (const half_t*)bias; a.y = (half_t*)y;
    a.N = n; a.Cin = cin; a.H = h; a.W = w; a.Cout = cout; a.dup_off = dup_off;
    const int st = launched(small_conv_in_launch(a, (hipStream_t)stream), "small_conv_in_kernel");
    return noted(st, small_conv_last_kernel_name());
}

int ld_op_small_conv_out(const void* x, const void* wt, const void* bias, int n, int h, int w, int cin, int cout, int mode, const float* x_in,
                         const float* sigma, int in_mod, float* out, void* stream) {
    op_begin();
    if (n <= 0 || h <= 0 || w <= 0 || mode < 0 || mode > 2 || in_mod < 0) return LD_ERR_ARG;
    SmallConvOutArgs a;
    a.x = (const half_t*)x; a.w = (const half_t*)wt; a.b = (const half_t*)bias;
    a.N = n; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout; a.mode = mode;
    a.x_in = x_in; a.sigma = sigma; a.in_mod = in_mod; a.out = out;
    const int st = launched(small_conv_out_launch(a, (hipStream_t)stream), "small_conv_out_kernel");
    return noted(st, small_conv_last_kernel_name());
}

int ld_op_small_pointwise(const void* x, const void* wt, const void* bias, float* out, int n, int hw, int c, void* stream) {
    op_begin();
    return launched(small_pointwise_launch((const half_t*)x, (const half_t*)wt, (const half_t*)bias, out, n, hw, c, (hipStream_t)stream), "small_pointwise_kernel");
}

int ld_op_vae_out_finish(const void* t8, float* out, long long npix, int cout, void* stream) {
    op_begin();
    return launched(vae_out_finish_launch((const half_t*)t8, out, npix, cout, (hipStream_t)stream), "vae_out_finish_kernel");
}

int ld_op_timestep_embed_mod(const float* sigma, const float* log_sigmas, int n_sigmas, int n, int dim, void* out, float* t_out, int sigma_mod,
                             void* stream) {
    op_begin();
    return launched(timestep_embed_launch(sigma, log_sigmas, n_sigmas, n, dim, (half_t*)out, t_out, (hipStream_t)stream, sigma_mod), "timestep_embed_kernel");
}

int ld_op_dup_halves(void* base0, size_t bytes0, void* base1, size_t bytes1, void* base2, size_t bytes2, int count, void* stream) {
    op_begin();
    DupArgs a;
    a.base[0] = (char*)base0; a.bytes[0] = bytes0;
    a.base[1] = (char*)base1; a.bytes[1] = bytes1;
    a.base[2] = (char*)base2; a.bytes[2] = bytes2;
    a.count = count;
    return launched(dup_halves_launch(a, (hipStream_t)stream), "dup_halves_kernel");
}

int ld_op_ctx_pad(const void* src, int dtype, int n, int t, int tp, int d, void* dst, void* stream) {
    op_begin();
    if ((dtype != LD_F16 && dtype != LD_F32) || n <= 0 || t <= 0 || d <= 0) return LD_ERR_ARG;
    return ctx_pad_launch(src, dtype == LD_F32, n, t, tp, d, (half_t*)dst, (hipStream_t)stream);
}

int ld_op_ctx_kv(const void* ctx16, const void* wk, const void* wv, int n, int tp, int d, int c, void* k_out, void* vt_out, void* stream) {
    op_begin();
    // the two launches ld_unet_set_context makes per transformer, by the same builders: K = ctx Wk^T [n tp][c] and, per sample, V^T = Wv ctx^T [c][tp]
    if (ctx16 == nullptr || wk == nullptr || wv == nullptr || k_out == nullptr || vt_out == nullptr || n <= 0 || tp <= 0 || d <= 0 || c <= 0) return LD_ERR_ARG;
    const GemmParams k = linear_params((const half_t*)ctx16, d, (const half_t*)wk, nullptr, n * tp, c, d, (half_t*)k_out);
    const GemmPlan kp = gemm_plan(k);
    const int st = gemm_run(k, kp, (hipStream_t)stream);
    if (st != LD_OK) return st;
    note_kernel(&t_op_kernels, kp.kernel);
    GemmParams v = linear_params((const half_t*)wv, d, (const half_t*)ctx16, nullptr, c, tp, d, (half_t*)vt_out);
    v.batch = n; v.sW = (long long)tp * d; v.sC = (long long)c * tp;
    const GemmPlan vp = gemm_plan(v);
    return noted(gemm_run(v, vp, (hipStream_t)stream), vp.kernel);
}

int ld_op_mlp_out_fold(const void* wpo, const void* w2, const void* b2, const void* bpo, int c, void* w_out, void* b_out, void* stream) {
    op_begin();
    return mlp_out_fold_launch((const half_t*)wpo, (const half_t*)w2, (const half_t*)b2, (const half_t*)bpo, c, (half_t*)w_out, (half_t*)b_out,
                               (hipStream_t)stream);
}

int ld_op_ln_fold(const void* w, int n, int k, const void* gamma, const void* beta, const void* bias, void* w_out, void* b_out, float* wsum,
                  void* stream) {
    op_begin();
    return ln_fold_launch((const half_t*)w, n, k, (const half_t*)gamma, (const half_t*)beta, (const half_t*)bias, (half_t*)w_out, (half_t*)b_out, wsum,
                          (hipStream_t)stream);
}

// the UNet's LayerNorm fold (unet.hip Run::transformer, gemm.h) as a stand-alone operator pair on the executor's builders (ln_producer / ln_consumer):
//   t = x · w_prod^T + b_prod         (producer: also emits per-row (sum, sum of squares) partials of the fp16 t)
//   y = LayerNorm(t; gamma, beta, eps) · w^T + bias   computed as rstd * (t · W'^T - mu * wsum) + b' on the accumulators
// geglu: the transformer block's MLP input — y[M][N/2] = a * gelu(g), [a | g] = LayerNorm(t) · w^T + bias (GEGLU, LD.py:4513-4515); w rows are
// repacked into the tile-interleaved [value | gate] order first, then folded (the fold is row-wise).
static int op_linear_ln(const void* x, const void* w_prod, const void* b_prod, const void* residual, const void* gamma, const void* beta, const void* w, const void* bias,
                        void* t_out, void* y, int M, int C, int N, float eps, void* ws, size_t ws_bytes, void* stream, bool geglu) {
    if (x == nullptr || w_prod == nullptr || gamma == nullptr || beta == nullptr || w == nullptr || (geglu && bias == nullptr) || t_out == nullptr ||
        y == nullptr || ws == nullptr)
        return LD_ERR_ARG;
    const int bn = geglu ? gemm_pick_bn(N) : 0;
    if (geglu && ((N & 15) || (N % bn))) return LD_ERR_SHAPE;
    Op op(ws, ws_bytes, stream);
    const half_t* wr = (const half_t*)w;      // rows as the fold reads them: repacked for GEGLU
    const half_t* br = (const half_t*)bias;
    if (geglu) {
        wr = op.arena.halfs((size_t)N * C);
        br = op.arena.halfs((size_t)N);
    }
    half_t* w2 = op.arena.halfs((size_t)N * C);   // folded
    half_t* b2 = op.arena.halfs((size_t)N);
    float* wsum = (float*)op.arena.alloc((size_t)N * sizeof(float));
    float* stat = (float*)op.arena.alloc((size_t)((C + 63) / 64) * M * 2 * sizeof(float));
    if (!op.fits()) return LD_ERR_ARG;
    int st = LD_OK;
    if (geglu) {
        st = repack_rows_launch(w, 0, N, C, const_cast<half_t*>(wr), bn, op.ex.stream);
        if (st == LD_OK) st = repack_rows_launch(bias, 0, N, 1, const_cast<half_t*>(br), bn, op.ex.stream);
    }
    if (st == LD_OK) st = ln_fold_launch(wr, N, C, (const half_t*)gamma, (const half_t*)beta, br, w2, b2, wsum, op.ex.stream);
    if (st != LD_OK) return st;
    GemmParams a = linear_params((const half_t*)x, C, (const half_t*)w_prod, (const half_t*)b_prod, M, C, C, (half_t*)t_out);
    a.R = (const half_t*)residual;   // (the residual stream itself in Run::transformer: t += ...)
    ln_producer(a, stat);
    const int parts = op.ex.gemm(a).stat_parts;
    GemmParams b = linear_params((const half_t*)t_out, C, w2, b2, M, N, C, (half_t*)y, geglu ? 2 : 0, bn);
    ln_consumer(b, stat, parts, M, C, eps, wsum);
    op.ex.gemm(b);   // (not launched when the producer failed)
    return op.ex.status;
}

int ld_op_linear_ln(const void* x, const void* w_prod, const void* b_prod, const void* residual, const void* gamma, const void* beta, const void* w,
                    const void* bias, void* t_out, void* y, int M, int C, int N, float eps, void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    return op_linear_ln(x, w_prod, b_prod, residual, gamma, beta, w, bias, t_out, y, M, C, N, eps, ws, ws_bytes, stream, false);
}

int ld_op_linear_ln_geglu(const void* x, const void* w_prod, const void* b_prod, const void* residual, const void* gamma, const void* beta, const void* w,
                          const void* bias, void* t_out, void* y, int M, int C, int N, float eps, void* ws, size_t ws_bytes, void* stream) {
    op_begin();
    return op_linear_ln(x, w_prod, b_prod, residual, gamma, beta, w, bias, t_out, y, M, C, N, eps, ws, ws_bytes, stream, true);
}

int ld_op_lora_merge(const void* base_f16, void* dst_f16, int rows, int cols, const ld_lora_term* terms, int n_terms, void* stream) {
    op_begin();
    if (terms == nullptr || n_terms < 1 || n_terms > LORA_MAX_TERMS) return LD_ERR_ARG;
    LoraArgs a;
    a.base = (const half_t*)base_f16;
    a.dst = (half_t*)dst_f16;
    a.lay.kind = LORA_MAT;
    a.lay.rows = rows;
    a.lay.cols = cols;
    a.n_terms = n_terms;
    for (int j = 0; j < n_terms; ++j) {
        if (terms[j].dtype != LD_F16 && terms[j].dtype != LD_F32) return LD_ERR_ARG;
        a.t[j].up = terms[j].up; a.t[j].down = terms[j].down; a.t[j].f32 = terms[j].dtype == LD_F32;
        a.t[j].rank = terms[j].rank; a.t[j].scale = terms[j].scale;
    }
    return lora_merge_launch(a, (hipStream_t)stream);
}

// the 21-argument entry point every earlier caller has, and the same with the second store (y2, ldy2) that only the RRDB's third block uses
int ld_op_esrgan_conv_y2(const void* x, int ldx, int cin, int n, int h, int w, int up, const void* wt, const void* bias, void* y, int ldy, int c_off,
                         int cout, float slope, const void* r1, int ldr1, float s1, const void* r2, int ldr2, float s2, void* y2, int ldy2, void* stream) {
    op_begin();
    EsrganConvArgs a;
    a.x = (const half_t*)x; a.ldx = ldx; a.cin = cin;
    a.n = n; a.h = h; a.w = w; a.up = up;
    a.wt = (const half_t*)wt; a.bias = (const half_t*)bias;
    a.y = (half_t*)y; a.ldy = ldy; a.c_off = c_off; a.cout = cout;
    a.slope = slope;
    a.r1 = (const half_t*)r1; a.ldr1 = ldr1; a.s1 = s1;
    a.r2 = (const half_t*)r2; a.ldr2 = ldr2; a.s2 = s2;
    a.y2 = (half_t*)y2; a.ldy2 = ldy2;
    const int st = esrgan_conv_launch(a, (hipStream_t)stream);
    return noted(launched(st, esrgan_last_kernel_name()), esrgan_last_kernel_name());
}

int ld_op_esrgan_conv(const void* x, int ldx, int cin, int n, int h, int w, int up, const void* wt, const void* bias, void* y, int ldy, int c_off, int cout,
                      float slope, const void* r1, int ldr1, float s1, const void* r2, int ldr2, float s2, void* stream) {
    return ld_op_esrgan_conv_y2(x, ldx, cin, n, h, w, up, wt, bias, y, ldy, c_off, cout, slope, r1, ldr1, s1, r2, ldr2, s2, nullptr, 0, stream);
}

int ld_op_taesd_conv(const void* x, int n, int h, int w, int up, const void* wt, const void* bias, const void* residual, int relu, void* y, void* stream) {
    op_begin();
    const int st = taesd_conv_launch((const half_t*)x, n, h, w, up, (const half_t*)wt, (const half_t*)bias, (const half_t*)residual, relu, (half_t*)y,
                                     (hipStream_t)stream);
    return noted(launched(st, taesd_last_kernel_name()), taesd_last_kernel_name());
}

// the 3- and 4-channel end convolutions of the upscaler and the preview decoder alone: for parity tests (the launchers the executors call).
// A call the launcher refuses launched nothing and leaves ld_op_last_kernel() as it was.
int ld_op_esrgan_first(const float* x, const void* wt, const void* bias, void* y, int ldy, void* y2, int ldy2, int n, int h, int w, void* stream) {
    const int st = esrgan_first_launch(x, (const half_t*)wt, (const half_t*)bias, (half_t*)y, ldy, (half_t*)y2, ldy2, n, h, w, (hipStream_t)stream);
    if (st != LD_OK) return st;
    op_begin();
    return noted(launched(st, "esrgan_first_kernel"), "esrgan_first_kernel");
}

int ld_op_esrgan_last(const void* x, int ldx, const void* wt, const void* bias, float* out, int n, int h, int w, void* stream) {
    const int st = esrgan_last_launch((const half_t*)x, ldx, (const half_t*)wt, (const half_t*)bias, out, n, h, w, (hipStream_t)stream);
    if (st != LD_OK) return st;
    op_begin();
    return noted(launched(st, "esrgan_last_kernel"), "esrgan_last_kernel");
}

int ld_op_taesd_first(const float* x, const void* wt, const void* bias, void* y, int n, int h, int w, void* stream) {
    const int st = taesd_first_launch(x, (const half_t*)wt, (const half_t*)bias, (half_t*)y, n, h, w, (hipStream_t)stream);
    if (st != LD_OK) return st;
    op_begin();
    return noted(launched(st, "taesd_first_kernel"), "taesd_first_kernel");
}

int ld_op_taesd_last(const void* x, const void* wt, const void* bias, float* out_f32, void* out_u8, int n, int h, int w, void* stream) {
    const int st = taesd_last_launch((const half_t*)x, (const half_t*)wt, (const half_t*)bias, out_f32, (uint8_t*)out_u8, n, h, w, (hipStream_t)stream);
    if (st != LD_OK) return st;
    op_begin();
    return noted(launched(st, "taesd_last_kernel"), "taesd_last_kernel");
}

int ld_op_tile_blend(const float* ps, const float* my, const float* mx, int th, int tw, float* out, float* div, int oh, int ow, int y0, int x0, int c,
                     void* stream) {
    op_begin();
    return tile_blend_launch(ps, my, mx, th, tw, out, div, oh, ow, y0, x0, c, (hipStream_t)stream);
}

int ld_op_bislerp(const float* x, float* tmp, float* y, int n, int c, int h, int w, int h_new, int w_new, void* stream) {
    op_begin();
    return bislerp_launch(x, tmp, y, n, c, h, w, h_new, w_new, (hipStream_t)stream);
}

int ld_op_u8_resample(const void* src, int src_pitch, int in_w, int in_h, int channels, void* dst, int dst_pitch, int out_w, int out_h, const int* hcoef,
                      int hk, const int* vcoef, int vk, void* tmp, void* stream) {
    op_begin();
    return u8_resample_launch((const uint8_t*)src, src_pitch, in_w, in_h, channels, (uint8_t*)dst, dst_pitch, out_w, out_h, hcoef, hk, vcoef, vk,
                              (uint8_t*)tmp, (hipStream_t)stream);
}

size_t ld_op_u8_resample_tmp_bytes(int in_h, int out_w, int channels) { return u8_resample_tmp_bytes(in_h, out_w, channels); }

int ld_op_u8_box_weights(float radius, int* box_radius, unsigned* ww, unsigned* fw) {
    if (box_radius == nullptr || ww == nullptr || fw == nullptr) return LD_ERR_ARG;
    return u8_box_weights(radius, box_radius, ww, fw);
}

size_t ld_op_u8_blur_tmp_bytes(int w, int h) { return u8_blur_tmp_bytes(w, h); }

int ld_op_u8_gaussian_blur(const void* src, int src_pitch, void* dst, int dst_pitch, int w, int h, float radius, void* tmp, void* stream) {
    op_begin();
    return u8_gaussian_blur_launch((const uint8_t*)src, src_pitch, (uint8_t*)dst, dst_pitch, w, h, radius, (uint8_t*)tmp, (hipStream_t)stream);
}

int ld_op_u8_mask(void* dst, int dst_pitch, int w, int h, int px, int py, int pw, int ph, const void* pattern, int pattern_pitch, void* stream) {
    op_begin();
    return u8_mask_launch((uint8_t*)dst, dst_pitch, w, h, px, py, pw, ph, (const uint8_t*)pattern, pattern_pitch, (hipStream_t)stream);
}

int ld_op_u8_composite(void* canvas, int canvas_pitch, int cw, int ch, const void* tile, int tile_pitch, const void* alpha, int alpha_pitch, int x0, int y0,
                       int w, int h, int channels, void* stream) {
    op_begin();
    return u8_composite_launch((uint8_t*)canvas, canvas_pitch, cw, ch, (const uint8_t*)tile, tile_pitch, (const uint8_t*)alpha, alpha_pitch, x0, y0, w, h,
                               channels, (hipStream_t)stream);
}

int ld_op_u8_from_f32(const float* x, void* y, size_t n, void* stream) {
    op_begin();
    return u8_from_f32_launch(x, (uint8_t*)y, n, (hipStream_t)stream);
}

int ld_op_f32_from_u8(const void* x, float* y, size_t n, void* stream) {
    op_begin();
    return f32_from_u8_launch((const uint8_t*)x, y, n, (hipStream_t)stream);
}

int ld_op_f32_crop_u8(const float* canvas, int canvas_pitch, int cw, int ch, int channels, int x1, int y1, int x2, int y2, void* dst, int dst_pitch,
                      void* stream) {
    op_begin();
    return f32_crop_u8_launch(canvas, canvas_pitch, cw, ch, channels, x1, y1, x2, y2, (uint8_t*)dst, dst_pitch, (hipStream_t)stream);
}

int ld_op_f32_blur_max_feather(void) { return F32_BLUR_MAX_FEATHER; }

size_t ld_op_f32_blur_tmp_bytes(int w, int h) { return f32_blur_tmp_bytes(w, h); }

int ld_op_f32_gaussian_blur(const float* src, int src_pitch, float* dst, int dst_pitch, int w, int h, int feather, const float* taps, float* tmp,
                            void* stream) {
    op_begin();
    return f32_gaussian_blur_launch(src, src_pitch, dst, dst_pitch, w, h, feather, taps, tmp, (hipStream_t)stream);
}

int ld_op_f32_paste_u8(float* canvas, int canvas_pitch, int cw, int ch, int channels, const void* tile, int tile_pitch, const float* alpha, int alpha_pitch,
                       int tw, int th, int x0, int y0, void* stream) {
    op_begin();
    return f32_paste_u8_launch(canvas, canvas_pitch, cw, ch, channels, (const uint8_t*)tile, tile_pitch, alpha, alpha_pitch, tw, th, x0, y0,
                               (hipStream_t)stream);
}

int ld_op_inpaint_in(const float* x, const float* mask, const float* latent, const float* noise, const float* sigma, float* out, int B, int C, int HW, int Bm,
                     int Cm, void* stream) {
    op_begin();
    return inpaint_blend_in_launch(x, mask, latent, noise, sigma, out, B, C, HW, Bm, Cm, (hipStream_t)stream);
}

int ld_op_inpaint_out(float* den, const float* mask, const float* latent, int B, int C, int HW, int Bm, int Cm, void* stream) {
    op_begin();
    return inpaint_blend_out_launch(den, mask, latent, B, C, HW, Bm, Cm, (hipStream_t)stream);
}

static_assert(sizeof(ld_regional_window) == sizeof(RegionalWindow) && sizeof(ld_regional_entry) == sizeof(RegionalEntry) &&
                  offsetof(ld_regional_entry, mask_strength) == offsetof(RegionalEntry, mask_strength),
              "the ABI's regional descriptors are the kernels' own");

int ld_op_regional_gather(const float* x, float* out, int B, int C, int H, int W, int h, int w, const ld_regional_window* windows, int k, void* stream) {
    op_begin();
    return regional_gather_launch(x, out, B, C, H, W, h, w, reinterpret_cast<const RegionalWindow*>(windows), k, (hipStream_t)stream);
}

int ld_op_regional_combine(const ld_regional_entry* entries, int n, float cond_scale, float* result, int B, int C, int H, int W, void* stream) {
    op_begin();
    return regional_combine_launch(reinterpret_cast<const RegionalEntry*>(entries), n, cond_scale, result, B, C, H, W, (hipStream_t)stream);
}

int ld_op_control_add(void* const* t, const void* const* r, const long long* per, int count, int n, int r_n, float strength, void* stream) {
    op_begin();
    if (t == nullptr || r == nullptr || per == nullptr) return LD_ERR_ARG;
    if (count < 1 || count > CONTROL_MAX_SEGMENTS) return LD_ERR_SHAPE;
    ControlSegment segs[CONTROL_MAX_SEGMENTS];
    for (int i = 0; i < count; ++i) segs[i] = {(half_t*)t[i], (const half_t*)r[i], per[i]};
    return launched(control_add_launch(segs, count, n, r_n, strength, (hipStream_t)stream), "control_add_kernel");
}

int ld_op_hint_conv(const void* x_f16_nhwc, const float* x_f32_nchw, int n, int h, int w, int cin, const void* wt, const void* bias, int cout, int stride, int silu,
                    void* y, void* stream) {
    op_begin();
    return launched(hint_conv_launch((const half_t*)x_f16_nhwc, x_f32_nchw, n, h, w, cin, (const half_t*)wt, (const half_t*)bias, cout, stride, silu, (half_t*)y,
                                     (hipStream_t)stream), "hint_conv_kernel");
}

int ld_op_clip_embed(const int* ids, const void* table, const float* extra, const void* pos, void* out, int B, int L, int V, int E, int h, void* stream) {
    op_begin();
    return launched(clip_embed_launch(ids, (const half_t*)table, extra, (const half_t*)pos, (half_t*)out, B, L, V, E, h, (hipStream_t)stream),
                    "clip_embed_kernel");
}

}  // extern "C"
