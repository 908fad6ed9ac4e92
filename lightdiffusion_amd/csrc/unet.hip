// SD1.x UNet executor (host side).  Walks the same block structure UNetModel1.__init__ builds (LD.py:5379-5686)
// and UNetModel1.forward runs (LD.py:5688-5767), but on NHWC fp16 activations — in that layout a feature map IS the
// [tokens, channels] matrix of the SpatialTransformer, so the reference's 32 NCHW<->NLC transposing copies
// (LD.py:4251, 4259) disappear, the skip concats are virtual (two-source A loaders), nearest-upsample is an
// index map inside the conv loader, and every bias / time-embedding add / residual / SiLU / GEGLU is an epilogue.
#include <cstring>

#include "runtime.h"
#include "../../include/ld_mi355x.h"

namespace {

struct ResW {
    std::string prefix;
    int cin = 0, cout = 0, emb_off = 0;
    int gn1_g, gn1_b, c1_w, c1_b, emb_w, emb_b, gn2_g, gn2_b, c2_w, c2_b, sk_w = -1, sk_b = -1;
    // skip fold (derived with the LayerNorm folds): [W2 | Wskip] ([cout][9 cout + cin]) and b2 + bskip — the 1x1 skip_connection runs as a
    // second K segment of out_layers' convolution where that convolution runs on a tap-major kernel (gemm.h S1 / S2); byte offsets into fold_base
    size_t f_c2_w = 0, f_c2_b = 0;
};
struct StW {
    int c = 0, bn = 0, ctx_slot = 0;
    // LN fold (derived at the first forward after a weight load): gamma-folded weights / beta-folded biases (byte offsets into
    // ld_unet::fold_base) and their fp32 row sums, for the projections that consume LN1 (q|k, v), LN2 (q of attn2), LN3 (GEGLU)
    size_t f_qk_w = 0, f_q2_w = 0, f_ff1_w = 0, f_qk_b = 0, f_q2_b = 0, f_ff1_b = 0, f_qk_s = 0, f_q2_s = 0,
           f_ff1_s = 0;
    // MLP-out fold: [Wpo W2 | Wpo] ([C][5C]) and Wpo b2 + bpo — ff.net.2 and proj_out run as ONE two-source contraction
    size_t f_mo_w = 0, f_mo_b = 0;
    int gn_g, gn_b, pin_w, pin_b, ln1_g, ln1_b, q1_w, k1_w, v1_w, o1_w, o1_b, ln2_g, ln2_b, q2_w, k2_w, v2_w, o2_w, o2_b, ln3_g,
        ln3_b, ff1_w, ff1_b, ff2_w, ff2_b, pout_w, pout_b;
};
struct ConvW {
    int cin = 0, cout = 0, w = -1, b = -1;
    // Upsample1 only: the nearest-2x resize folded into the weights — the 16 phase-tap matrices [py*2+px][cout][a*2+b][cin] (gemm.h Wup), derived
    // with the other folds; byte offset into fold_base, or -1
    long long f_up = -1;
};
enum LayerKind { L_CONV_IN, L_RES, L_ST, L_DOWN, L_UP };
struct Layer {
    int kind, idx;
};
struct Feat {
    half_t* p;
    int C, H, W;
    GnStats stats;         // GroupNorm partial statistics of this tensor, where its producer wrote them
};

// every piece of the resident layouts (derived weight copies, the hint encoder's buffers) takes a multiple of 256 bytes
constexpr size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace

struct ld_unet : Model {
    ld_unet_config cfg;
    std::vector<ResW> res;
    std::vector<StW> st;
    std::vector<ConvW> convs;
    std::vector<std::vector<Layer>> in_blocks, out_blocks;
    std::vector<Layer> mid_block;
    int te0_w, te0_b, te2_w, te2_b, outn_g, outn_b, outc_w, outc_b;
    int emb_total = 0, ted = 0;
    float* log_sigmas = nullptr;   // 1000-entry table, device
    // context (cross-attention K / V^T per transformer, hoisted out of the step)
    int max_n = 0, max_h = 0, max_w = 0, max_tok = 0;
    half_t* ctx16 = nullptr;
    std::vector<half_t*> ctx_k, ctx_vt;
    int ctx_n = 0, ctx_tok = 0, ctx_tpad = 0;
    PlanKey planned;               // (n, h, w, pair) validated last
    // derived copies of the 3x3 convolution weights in the row-resident kernel's layout (conv8.hip), re-derived with the LayerNorm folds
    struct W8 { int slot, N, Cin; size_t off; };
    std::vector<W8> w8_list;
    std::vector<long long> w8_of_slot;   // byte offset into w8_base per parameter slot, -1: none
    char* w8_base = nullptr;
    size_t w8_bytes = 0;
    const half_t* w8(int slot) const {
        return (w8_base != nullptr && slot >= 0 && slot < (int)w8_of_slot.size() && w8_of_slot[slot] >= 0) ? reinterpret_cast<const half_t*>(w8_base + w8_of_slot[slot]) : nullptr;
    }
    void want_w8(int slot, int N, int Cin) {
        if (!conv8_weight_eligible(N, Cin)) return;
        w8_list.push_back({slot, N, Cin, w8_bytes});
        w8_bytes += pad256(conv8_weight_bytes(N, Cin));
    }
    char* fold_base = nullptr;     // LN-folded copies of the LN-consuming projections (see StW)
    size_t fold_bytes = 0;
    // the next piece of the fold buffer: its byte offset into fold_base.  The order of the takes IS the resident layout.
    size_t take_fold(size_t bytes) {
        const size_t off = fold_bytes;
        fold_bytes += pad256(bytes);
        return off;
    }
    bool fold_dirty = true;        // set by every ld_unet_load_param / patch / unpatch; cleared when the fold kernels have run
    // LoRA patches (ld_unet_patch_param): per patched slot a device snapshot of its resident bytes as they were before the first patch — a
    // further resident copy, held only while the slot is patched.  Every merge reads the snapshot, ld_unet_unpatch copies it back.
    std::unordered_map<int, half_t*> backups;
    size_t patch_bytes = 0;
    // "control" mode (ld_controlnet_create; upstream's cldm.ControlNet): time_embed, input_blocks and middle_block as above, no output blocks and
    // no out.*; instead the hint encoder (input_hint_block), one 1x1 zero convolution per input block and middle_block_out.  A forward writes
    // the zero convolutions' raw outputs — the residuals — into buffers that persist in the handle (carved from the workspace by ld_unet_reserve).
    bool control = false;
    int hint_channels = 0;
    struct HintW { int w, b, cin, cout, stride; };
    std::vector<HintW> hint_convs;
    std::vector<int> zc_w, zc_b;                    // zero_convs.{i}.0 of input block i; the last pair is middle_block_out.0
    half_t* hint = nullptr;                         // the encoded hint [hint_b][hint_h][hint_w][model_channels]
    int hint_b = 0, hint_h = 0, hint_w = 0;         // 0: none set since the last reserve
    std::vector<half_t*> res_buf;                   // one per zero convolution, each for the reserved maximum
    struct ResShape { int C = 0, H = 0, W = 0; };
    std::vector<ResShape> res_shape;                // of the last forward; its batch: res_n
    int res_n = 0;
    void drop_backup(int slot) {
        auto it = backups.find(slot);
        if (it == backups.end()) return;
        (void)hipFree(it->second);
        patch_bytes -= pt.slots[slot].elems * sizeof(half_t);
        backups.erase(it);
    }
};

namespace {

std::string S(const char* fmt, int a = 0, int b = 0) {
    char buf[160];
    snprintf(buf, sizeof buf, fmt, a, b);
    return buf;
}

int add_res(ld_unet* u, const std::string& p, int cin, int cout) {
    ParamTable& t = u->pt;
    ResW r;
    r.prefix = p;
    r.cin = cin;
    r.cout = cout;
    r.gn1_g = t.add(p + ".in_layers.0.weight", PK_VEC, {cin});
    r.gn1_b = t.add(p + ".in_layers.0.bias", PK_VEC, {cin});
    r.c1_w = t.add(p + ".in_layers.2.weight", PK_CONV3, {cout, cin, 3, 3});
    r.c1_b = t.add(p + ".in_layers.2.bias", PK_VEC, {cout});
    u->want_w8(r.c1_w, cout, cin);
    r.gn2_g = t.add(p + ".out_layers.0.weight", PK_VEC, {cout});
    r.gn2_b = t.add(p + ".out_layers.0.bias", PK_VEC, {cout});
    r.c2_w = t.add(p + ".out_layers.3.weight", PK_CONV3, {cout, cout, 3, 3});
    r.c2_b = t.add(p + ".out_layers.3.bias", PK_VEC, {cout});
    u->want_w8(r.c2_w, cout, cout);
    if (cin != cout) {
        r.sk_w = t.add(p + ".skip_connection.weight", PK_MAT, {cout, cin, 1, 1});
        r.sk_b = t.add(p + ".skip_connection.bias", PK_VEC, {cout});
        r.f_c2_w = u->take_fold((size_t)cout * (9 * cout + cin) * sizeof(half_t));
        r.f_c2_b = u->take_fold((size_t)cout * sizeof(half_t));
    }
    r.emb_off = u->emb_total;
    u->emb_total += cout;
    u->res.push_back(r);
    return (int)u->res.size() - 1;
}

int add_st(ld_unet* u, const std::string& p, int c) {
    ParamTable& t = u->pt;
    const int ctx = u->cfg.context_dim;
    StW s;
    s.c = c;
    s.bn = gemm_pick_bn(8 * c);
    s.ctx_slot = (int)u->st.size();
    s.gn_g = t.add(p + ".norm.weight", PK_VEC, {c});
    s.gn_b = t.add(p + ".norm.bias", PK_VEC, {c});
    s.pin_w = t.add(p + ".proj_in.weight", PK_MAT, {c, c, 1, 1});
    s.pin_b = t.add(p + ".proj_in.bias", PK_VEC, {c});
    const std::string b = p + ".transformer_blocks.0";
    s.ln1_g = t.add(b + ".norm1.weight", PK_VEC, {c});
    s.ln1_b = t.add(b + ".norm1.bias", PK_VEC, {c});
    s.q1_w = t.add(b + ".attn1.to_q.weight", PK_MAT, {c, c});
    s.k1_w = t.add(b + ".attn1.to_k.weight", PK_MAT, {c, c}, 16);   // contiguous with to_q: one [2C][C] projection
    s.v1_w = t.add(b + ".attn1.to_v.weight", PK_MAT, {c, c}, 16);   // ... and to_v: one [3C][C] projection (the attention kernel reads V row-major)
    s.o1_w = t.add(b + ".attn1.to_out.0.weight", PK_MAT, {c, c});
    s.o1_b = t.add(b + ".attn1.to_out.0.bias", PK_VEC, {c});
    s.ln2_g = t.add(b + ".norm2.weight", PK_VEC, {c});
    s.ln2_b = t.add(b + ".norm2.bias", PK_VEC, {c});
    s.q2_w = t.add(b + ".attn2.to_q.weight", PK_MAT, {c, c});
    s.k2_w = t.add(b + ".attn2.to_k.weight", PK_MAT, {c, ctx});
    s.v2_w = t.add(b + ".attn2.to_v.weight", PK_MAT, {c, ctx});
    s.o2_w = t.add(b + ".attn2.to_out.0.weight", PK_MAT, {c, c});
    s.o2_b = t.add(b + ".attn2.to_out.0.bias", PK_VEC, {c});
    s.ln3_g = t.add(b + ".norm3.weight", PK_VEC, {c});
    s.ln3_b = t.add(b + ".norm3.bias", PK_VEC, {c});
    s.ff1_w = t.add(b + ".ff.net.0.proj.weight", PK_GEGLU_W, {8 * c, c}, 256, s.bn);
    s.ff1_b = t.add(b + ".ff.net.0.proj.bias", PK_GEGLU_B, {8 * c}, 256, s.bn);
    s.ff2_w = t.add(b + ".ff.net.2.weight", PK_MAT, {c, 4 * c});
    s.ff2_b = t.add(b + ".ff.net.2.bias", PK_VEC, {c});
    s.pout_w = t.add(p + ".proj_out.weight", PK_MAT, {c, c, 1, 1});
    s.pout_b = t.add(p + ".proj_out.bias", PK_VEC, {c});
    {   // LN-fold buffer layout (256-byte aligned pieces)
        const size_t C = (size_t)c;
        s.f_qk_w = u->take_fold(3 * C * C * sizeof(half_t));   // [Wq ; Wk ; Wv] of attn1
        s.f_q2_w = u->take_fold(C * C * sizeof(half_t));
        s.f_ff1_w = u->take_fold(8 * C * C * sizeof(half_t));
        s.f_qk_b = u->take_fold(3 * C * sizeof(half_t));
        s.f_q2_b = u->take_fold(C * sizeof(half_t));
        s.f_ff1_b = u->take_fold(8 * C * sizeof(half_t));
        s.f_qk_s = u->take_fold(3 * C * sizeof(float));
        s.f_q2_s = u->take_fold(C * sizeof(float));
        s.f_ff1_s = u->take_fold(8 * C * sizeof(float));
        s.f_mo_w = u->take_fold(5 * C * C * sizeof(half_t));
        s.f_mo_b = u->take_fold(C * sizeof(half_t));
    }
    u->st.push_back(s);
    return (int)u->st.size() - 1;
}

int add_conv(ld_unet* u, const std::string& p, int cin, int cout) {
    ConvW c;
    c.cin = cin;
    c.cout = cout;
    c.w = u->pt.add(p + ".weight", PK_CONV3, {cout, cin, 3, 3});
    c.b = u->pt.add(p + ".bias", PK_VEC, {cout});
    u->convs.push_back(c);
    return (int)u->convs.size() - 1;
}

int build(ld_unet* u) {
    const ld_unet_config& c = u->cfg;
    if (c.num_levels < 1 || c.num_levels > 8 || c.model_channels % 32 || c.num_heads < 1) return LD_ERR_ARG;
    const int mc = c.model_channels;
    u->ted = mc * 4;
    ParamTable& t = u->pt;
    u->te0_w = t.add("time_embed.0.weight", PK_MAT, {u->ted, mc});
    u->te0_b = t.add("time_embed.0.bias", PK_VEC, {u->ted});
    u->te2_w = t.add("time_embed.2.weight", PK_MAT, {u->ted, u->ted});
    u->te2_b = t.add("time_embed.2.bias", PK_VEC, {u->ted});
    u->in_blocks.push_back({{L_CONV_IN, add_conv(u, "input_blocks.0.0", c.in_channels, mc)}});
    int ch = mc, idx = 1, td = 0;
    std::vector<int> chans{mc};
    for (int lvl = 0; lvl < c.num_levels; ++lvl) {
        for (int r = 0; r < c.num_res_blocks[lvl]; ++r) {
            std::vector<Layer> L;
            L.push_back({L_RES, add_res(u, S("input_blocks.%d.0", idx), ch, c.channel_mult[lvl] * mc)});
            ch = c.channel_mult[lvl] * mc;
            if (c.transformer_depth[td++] > 0) L.push_back({L_ST, add_st(u, S("input_blocks.%d.1", idx), ch)});
            u->in_blocks.push_back(L);
            chans.push_back(ch);
            ++idx;
        }
        if (lvl != c.num_levels - 1) {
            u->in_blocks.push_back({{L_DOWN, add_conv(u, S("input_blocks.%d.0.op", idx), ch, ch)}});
            chans.push_back(ch);
            ++idx;
        }
    }
    u->mid_block.push_back({L_RES, add_res(u, "middle_block.0", ch, ch)});
    if (c.transformer_depth_middle > 0) u->mid_block.push_back({L_ST, add_st(u, "middle_block.1", ch)});
    u->mid_block.push_back({L_RES, add_res(u, "middle_block.2", ch, ch)});
    if (u->control) {   // upstream's cldm.ControlNet: the encoder half above, then
        if (u->hint_channels < 1 || u->hint_channels > 4 || u->in_blocks.size() + 1 > (size_t)CONTROL_MAX_SEGMENTS) return LD_ERR_ARG;
        const int hc[9] = {u->hint_channels, 16, 16, 32, 32, 96, 96, 256, mc};
        for (int i = 0; i < 8; ++i) {   // input_hint_block: conv, SiLU, conv, SiLU, ... conv — the convolutions at the even indices
            ld_unet::HintW hw;
            hw.cin = hc[i];
            hw.cout = hc[i + 1];
            hw.stride = (i == 2 || i == 4 || i == 6) ? 2 : 1;
            hw.w = t.add(S("input_hint_block.%d.weight", 2 * i), PK_CONV3, {hw.cout, hw.cin, 3, 3});
            hw.b = t.add(S("input_hint_block.%d.bias", 2 * i), PK_VEC, {hw.cout});
            u->hint_convs.push_back(hw);
        }
        for (size_t i = 0; i < chans.size(); ++i) {
            u->zc_w.push_back(t.add(S("zero_convs.%d.0.weight", (int)i), PK_MAT, {chans[i], chans[i], 1, 1}));
            u->zc_b.push_back(t.add(S("zero_convs.%d.0.bias", (int)i), PK_VEC, {chans[i]}));
        }
        u->zc_w.push_back(t.add("middle_block_out.0.weight", PK_MAT, {ch, ch, 1, 1}));
        u->zc_b.push_back(t.add("middle_block_out.0.bias", PK_VEC, {ch}));
        for (size_t i = 0; i < u->res.size(); ++i)
            u->res[i].emb_w = t.add(u->res[i].prefix + ".emb_layers.1.weight", PK_MAT, {u->res[i].cout, u->ted}, i == 0 ? 256 : 16);
        for (size_t i = 0; i < u->res.size(); ++i)
            u->res[i].emb_b = t.add(u->res[i].prefix + ".emb_layers.1.bias", PK_VEC, {u->res[i].cout}, i == 0 ? 256 : 16);
        u->outn_g = u->outn_b = u->outc_w = u->outc_b = -1;
        return t.finalize();
    }
    // the reference pops transformer_depth_output from the END of the list (LD.py:5621)
    int n_out = 0;
    for (int lvl = 0; lvl < c.num_levels; ++lvl) n_out += c.num_res_blocks[lvl] + 1;
    int tdo = n_out;
    idx = 0;
    for (int lvl = c.num_levels - 1; lvl >= 0; --lvl) {
        for (int i = 0; i <= c.num_res_blocks[lvl]; ++i) {
            const int ich = chans.back();
            chans.pop_back();
            std::vector<Layer> L;
            L.push_back({L_RES, add_res(u, S("output_blocks.%d.0", idx), ch + ich, mc * c.channel_mult[lvl])});
            ch = mc * c.channel_mult[lvl];
            int j = 1;
            if (c.transformer_depth_output[--tdo] > 0) {
                L.push_back({L_ST, add_st(u, S("output_blocks.%d.%d", idx, j), ch)});
                ++j;
            }
            if (lvl && i == c.num_res_blocks[lvl]) {
                L.push_back({L_UP, add_conv(u, S("output_blocks.%d.%d.conv", idx, j), ch, ch)});
                u->want_w8(u->convs.back().w, ch, ch);
                u->convs.back().f_up = (long long)u->take_fold(16 * (size_t)ch * ch * sizeof(half_t));
            }
            u->out_blocks.push_back(L);
            ++idx;
        }
    }
    u->outn_g = t.add("out.0.weight", PK_VEC, {ch});
    u->outn_b = t.add("out.0.bias", PK_VEC, {ch});
    u->outc_w = t.add("out.2.weight", PK_CONV3, {c.out_channels, mc, 3, 3});
    u->outc_b = t.add("out.2.bias", PK_VEC, {c.out_channels});
    // the 22 emb_layers Linears as ONE [sum(Cout)][4*mc] matrix (tightly packed) -> one GEMM per step
    for (size_t i = 0; i < u->res.size(); ++i)
        u->res[i].emb_w = t.add(u->res[i].prefix + ".emb_layers.1.weight", PK_MAT, {u->res[i].cout, u->ted}, i == 0 ? 256 : 16);
    for (size_t i = 0; i < u->res.size(); ++i)
        u->res[i].emb_b = t.add(u->res[i].prefix + ".emb_layers.1.bias", PK_VEC, {u->res[i].cout}, i == 0 ? 256 : 16);
    return t.finalize();
}

// ---------------------------------------------------------------------------------------------------- forward pieces
struct Run {
    ld_unet* u;
    Exec ex;
    int n;                   // samples the kernels run on
    int n_alloc;             // samples every tensor is SIZED for (= n, except in front of the first cross-attention of a CFG pair)
    bool pair_pending = false;   // CFG pair (LD_FWD_PAIR): the layers in front of the first cross-attention see the same input in the uncond and
                                 // the cond half of the batch, so they run ONCE on n = n_alloc / 2 samples and their results are copied into the second half
    const half_t* emb_all;   // [n_alloc][emb_total]
    Run(ld_unet* u_, int n_) : u(u_), n(n_), n_alloc(n_) {}
    half_t* P(int slot) const { return u->pt.ptr(slot); }
    // The two ends of a CFG pair's shared prefix, and the only writers of n and pair_pending.  begin_pair: the kernels run on the first half of the
    // batch.  hand_over: the first halves (half_bytes each) of the tensors that are read again become their second halves too, and the kernels run on
    // all n_alloc samples.  SD1.5's hand-over, inside its first transformer, copies three tensors in one dup_halves launch; a layout whose shared
    // prefix ends elsewhere copies one, as a memcpy node of the step's hipGraph; with nothing left to share nothing is launched.
    void begin_pair() {
        n = n_alloc / 2;
        pair_pending = true;
    }
    void hand_over(std::initializer_list<const half_t*> firsts = {}, size_t half_bytes = 0) {
        if (firsts.size() == 1) {
            char* base = reinterpret_cast<char*>(const_cast<half_t*>(*firsts.begin()));
            ex.launch(KC_MISC, 0.0, "dup", (long long)half_bytes, 0, 0, 1, "hipMemcpyAsync(pair)", [&] {
                return hipMemcpyAsync(base + half_bytes, base, half_bytes, hipMemcpyDeviceToDevice, ex.stream) == hipSuccess ? LD_OK : LD_ERR_HIP;
            });
        } else if (firsts.size() > 1) {
            DupArgs da;
            for (const half_t* t : firsts) {
                da.base[da.count] = reinterpret_cast<char*>(const_cast<half_t*>(t));
                da.bytes[da.count++] = half_bytes;
            }
            ex.launch(KC_MISC, 0.0, "dup3", (long long)half_bytes, 0, 0, 1, "dup_halves_kernel", [&] { return dup_halves_launch(da, ex.stream); });
        }
        n = n_alloc;
        pair_pending = false;
    }

    // a convolution of this run's n images on resident weights, with the row-resident kernel's copy of them where there is one
    GemmParams conv_of(const half_t* x1, int C1, const half_t* x2, int C2, int Hs, int Ws, int Hv, int Wv, int stride, int ksize, int wslot, int bslot,
                       int cout, half_t* out) const {
        GemmParams p = conv_params(x1, C1, x2, C2, n, Hs, Ws, Hv, Wv, stride, ksize, P(wslot), P(bslot), cout, out);
        p.W8 = ksize == 3 ? u->w8(wslot) : nullptr;
        return p;
    }

    // stats: a buffer for the GroupNorm partial statistics of the output (want_gn_partials); returns them where the launch wrote them
    GnStats conv3(const half_t* x1, int C1, const half_t* x2, int C2, int Hs, int Ws, int Hv, int Wv, int stride, int wslot, int bslot,
                  int cout, half_t* out, int ksize = 3, float* stats = nullptr, const half_t* wup = nullptr) {
        GemmParams p = conv_of(x1, C1, x2, C2, Hs, Ws, Hv, Wv, stride, ksize, wslot, bslot, cout, out);
        p.Wup = wup;
        if (stats != nullptr) want_gn_partials(p, n, p.Ho * p.Wo, stats);
        return gn_stats(stats, ex.gemm(p).gn_chunks);
    }

    void linear(const half_t* x, int lda, int wslot, int bslot, const half_t* R, half_t* y, int M, int N, int K, int act = 0, int bn = 0) {
        GemmParams p = linear_params(x, lda, P(wslot), bslot >= 0 ? P(bslot) : nullptr, M, N, K, y, act, bn);
        p.R = R;
        ex.gemm(p);
    }

    // ResBlock1._forward, LD.py:5273-5287.  Input = channel concat of (x1,C1) and (x2,C2).
    // in_stats: GroupNorm partial statistics of x1 from its producer (only usable when there is no second source)
    Feat resblock(const ResW& r, const half_t* x1, int C1, const half_t* x2, int C2, int H, int W, GnStats in_stats = {}) {
        Arena& ar = *ex.arena;
        const size_t M = (size_t)n_alloc * H * W;                   // rows the tensors are sized for (the kernels run on n * H * W)
        half_t* out = ar.halfs(M * r.cout);
        float* gno = ex.gn_buffer(n_alloc, H * W);                  // statistics of `out` (for the next GroupNorm)
        if (C2 != 0) in_stats = {};
        const size_t mk = ar.mark();
        // in_layers: GroupNorm + SiLU + conv3x3 (+ the time-embedding row vector); out_layers: GroupNorm + SiLU + conv3x3 (+ skip).
        // Each GroupNorm is fused into its convolution's A operand where that convolution runs on the halo-tile kernel
        // (Exec::gn_silu_conv); g1 / g2 are only written on the two-pass route.
        auto conv = [&](const half_t* a1, int c1, const half_t* a2, int c2, int wslot, int bslot, half_t* dst) {
            return conv_of(a1, c1, a2, c2, H, W, H, W, 1, 3, wslot, bslot, r.cout, dst);
        };
        half_t* g1 = ar.halfs(M * r.cin);
        half_t* h1 = ar.halfs(M * r.cout);
        // The 1x1 skip_connection (LD.py:5267): folded into out_layers' convolution as a second K segment where that convolution runs on a
        // tap-major kernel or on the halo-tile kernel's 256 x 320 tiles (centre-only steps, conv6.hip) — same FLOPs at the 3x3 kernels' rate,
        // one launch and one [M][cout] round trip less; a launch of its own in front of the row-resident kernel and the 128-pixel bands.  (On a second stream beside in_layers in a batch-1 step it measured 2.9 % SLOWER than in
        // order: tools/experiments/fork_join_skip_conv_r05.patch.txt.)
        const half_t* skip = x1;
        bool fold_skip = false;
        if (r.sk_w >= 0) {
            // (asked of out_layers' convolution as it stands before the skip joins it, as a residual or as a K segment)
            fold_skip = u->fold_base != nullptr && ex.conv_takes_skip_segment(conv(h1, r.cout, nullptr, 0, r.c2_w, r.c2_b, out));
            half_t* sk = (!fold_skip || ex.dry) ? ar.halfs(M * r.cout) : nullptr;   // (a planning run sizes for either route: ld_unet_reserve plans before the split-K scratch exists)
            if (!fold_skip) {
                conv3(x1, C1, x2, C2, H, W, H, W, 1, r.sk_w, r.sk_b, r.cout, sk, 1);
                skip = sk;
            }
        }
        // the GroupNorm statistics of h1 (out_layers' norm) come from conv1's split-K second pass where it has one (gemm.h gn_part)
        float* gnp = ex.gn_buffer(n_alloc, H * W);
        GemmParams c1 = conv(x1, C1, x2, C2, r.c1_w, r.c1_b, h1);
        c1.rowvec = emb_all + r.emb_off; c1.ldrv = u->emb_total;
        want_gn_partials(c1, n, H * W, gnp);
        const GnStats h1_stats = gn_stats(gnp, ex.gn_silu_conv(c1, n, H * W, P(r.gn1_g), P(r.gn1_b), 1e-5f, g1, in_stats).gn_chunks);
        half_t* g2 = g1;   // g1 is dead once conv1 has consumed it (stream order); reuse when it is large enough
        if (r.cout > r.cin) g2 = ar.halfs(M * r.cout);
        GemmParams c2 = conv(h1, r.cout, nullptr, 0, r.c2_w, r.c2_b, out);
        if (fold_skip)
            add_skip_segment(c2, x1, C1, x2, C2, reinterpret_cast<const half_t*>(u->fold_base + r.f_c2_w), reinterpret_cast<const half_t*>(u->fold_base + r.f_c2_b));
        else
            c2.R = skip;
        want_gn_partials(c2, n, H * W, gno);
        const GnStats out_stats = gn_stats(gno, ex.gn_silu_conv(c2, n, H * W, P(r.gn2_g), P(r.gn2_b), 1e-5f, g2, h1_stats).gn_chunks);
        ar.release(mk);
        return {out, r.cout, H, W, out_stats};
    }

    // SpatialTransformer.forward (LD.py:4239-4262) around BasicTransformerBlock._forward (LD.py:4117-4162)
    Feat transformer(const StW& s, const half_t* x, int H, int W, GnStats in_stats = {}) {
        Arena& ar = *ex.arena;
        const int C = s.c, L = H * W, heads = u->cfg.num_heads, d = C / heads;
        int M = n * L;                                           // rows the kernels run on (doubles at the split of a CFG pair, below)
        const size_t Ma = (size_t)n_alloc * L;                      // rows the tensors are sized for
        half_t* out = ar.halfs(Ma * C);
        float* gno = ex.gn_buffer(n_alloc, L);                      // statistics of `out` (for the next GroupNorm)
        const size_t mk = ar.mark();
        half_t* g = ar.halfs(Ma * C);
        ex.groupnorm(x, C, nullptr, 0, n, L, P(s.gn_g), P(s.gn_b), 1e-6f, 0, g, in_stats);
        half_t* t = ar.halfs(Ma * C);
        half_t* qkv = ar.halfs(Ma * 3 * C);
        half_t* ao = ar.halfs(Ma * C);
        half_t* ff = nullptr;
        // LN fold: the three LayerNorms disappear into the GEMMs around them.  The GEMM that WRITES the residual stream t also
        // writes per-row (sum, sum of squares) partials of t (one pair per N tile); the projections that read LN(t) run on t itself
        // with gamma folded into their weights and finish  rstd * (acc - mu * wsum) + b'  in the epilogue (gemm.h).
        float* stat = reinterpret_cast<float*>(ar.alloc((size_t)((C + 63) / 64) * Ma * 2 * sizeof(float)));
        int parts = 0;
        char* fb = u->fold_base;
        auto producer = [&](const half_t* x_, int wslot, int bslot, const half_t* R) {   // t = x_ W^T + b (+ R), with row stats
            GemmParams p = linear_params(x_, C, P(wslot), P(bslot), M, C, C, t);
            p.R = R;
            ln_producer(p, stat);
            parts = ex.gemm(p).stat_parts;
        };
        // out = LN(t) W^T + b on the folded weights / bias / row sums at these offsets of the fold buffer
        auto consumer = [&](size_t w_off, size_t b_off, size_t wsum_off, int N, half_t* dst, int act = 0, int bn = 0) {
            GemmParams p = linear_params(t, C, reinterpret_cast<const half_t*>(fb + w_off), reinterpret_cast<const half_t*>(fb + b_off), M, N, C, dst, act, bn);
            ln_consumer(p, stat, parts, M, C, 1e-5f, reinterpret_cast<const float*>(fb + wsum_off));
            ex.gemm(p);
        };
        producer(g, s.pin_w, s.pin_b, nullptr);
        // ---- self attention: x += to_out(attn(LN1(x)))
        // [q | k | v] = LN1(t) [Wq ; Wk ; Wv]^T — one launch; the attention kernel reads V row-major (transposing LDS reads), so there
        // is no V^T projection
        consumer(s.f_qk_w, s.f_qk_b, s.f_qk_s, 3 * C, qkv);
        {
            AttnParams a;
            a.Q = qkv; a.ldq = 3 * C; a.sQ = (long long)L * 3 * C;
            a.K = qkv + C; a.ldk = 3 * C; a.sK = (long long)L * 3 * C;
            a.V = qkv + 2 * C; a.ldv = 3 * C; a.sV = (long long)L * 3 * C;
            a.O = ao; a.ldo = C; a.sO = (long long)L * C;
            a.B = n; a.H = heads; a.Lq = L; a.Lk = L; a.d = d;
            a.scale = 1.0f / sqrtf((float)d);
            ex.attention(a);
        }
        // CFG pair: everything up to the cross-attention's K / V sees the same input in both halves of the batch and runs on the first half only
        // — also the out-projection of attn1, the LayerNorm-2 statistics it emits and the q projection of attn2 (only K / V of attn2 read the
        // conditioning).  Then the residual stream t, q2 and the block's input (its residual at the end) are copied into the second half and
        // everything else runs on all n_alloc samples (the statistics of the first half are not needed again: the out-projection of attn2
        // rewrites them for all rows).
        producer(ao, s.o1_w, s.o1_b, t);
        // ---- cross attention against the hoisted context K / V^T
        half_t* q2 = qkv;   // reuse
        consumer(s.f_q2_w, s.f_q2_b, s.f_q2_s, C, q2);
        if (pair_pending) {
            hand_over({t, q2, x}, (size_t)M * C * sizeof(half_t));
            M = n * L;
        }
        {
            const int Tp = u->ctx_tpad;
            AttnParams a;
            a.Q = q2; a.ldq = C; a.sQ = (long long)L * C;
            a.K = u->ctx_k[s.ctx_slot]; a.ldk = C; a.sK = (long long)Tp * C;
            a.Vt = u->ctx_vt[s.ctx_slot]; a.ldvt = Tp; a.sV = (long long)C * Tp;
            a.O = ao; a.ldo = C; a.sO = (long long)L * C;
            a.B = n; a.H = heads; a.Lq = L; a.Lk = u->ctx_tok; a.d = d;
            a.scale = 1.0f / sqrtf((float)d);
            ex.attention(a);
        }
        producer(ao, s.o2_w, s.o2_b, t);
        // ---- GEGLU feed-forward: x = ff2(a * gelu(gate)) + x
        ff = ar.halfs(Ma * 4 * C);
        consumer(s.f_ff1_w, s.f_ff1_b, s.f_ff1_s, 8 * C, ff, 2, s.bn);
        // out = x + proj_out(t + ff2(ff)) as one contraction over [ff | t] (K = 5C) against the folded [Wpo W2 | Wpo] (misc.hip)
        GemmParams p = conv_params(ff, 4 * C, t, C, n, H, W, H, W, 1, 1, reinterpret_cast<const half_t*>(fb + s.f_mo_w),
                                   reinterpret_cast<const half_t*>(fb + s.f_mo_b), C, out);
        p.R = x;
        want_gn_partials(p, n, L, gno);
        const GnStats out_stats = gn_stats(gno, ex.gemm(p).gn_chunks);
        ar.release(mk);
        return {out, C, H, W, out_stats};
    }
};

// LN fold: derive W' = W diag(gamma), b' = b + W beta and the fp32 row sums of W' for the projections that read LN1 / LN2 / LN3
// (64 small launches, once per weight load; stream-ordered before the forward that needs them).
int fold_layernorms(ld_unet* u, hipStream_t stream) {
    for (const StW& s : u->st) {
        const int C = s.c;
        char* fb = u->fold_base;
        auto H = [&](size_t off) { return reinterpret_cast<half_t*>(fb + off); };
        auto F = [&](size_t off) { return reinterpret_cast<float*>(fb + off); };
        const half_t* P_q1 = u->pt.ptr(s.q1_w);   // to_q and to_k are contiguous: one [2C][C] matrix
        int st = ln_fold_launch(P_q1, 3 * C, C, u->pt.ptr(s.ln1_g), u->pt.ptr(s.ln1_b), nullptr, H(s.f_qk_w), H(s.f_qk_b), F(s.f_qk_s), stream);
        if (st == LD_OK) st = ln_fold_launch(u->pt.ptr(s.q2_w), C, C, u->pt.ptr(s.ln2_g), u->pt.ptr(s.ln2_b), nullptr, H(s.f_q2_w), H(s.f_q2_b), F(s.f_q2_s), stream);
        if (st == LD_OK) st = ln_fold_launch(u->pt.ptr(s.ff1_w), 8 * C, C, u->pt.ptr(s.ln3_g), u->pt.ptr(s.ln3_b), u->pt.ptr(s.ff1_b), H(s.f_ff1_w), H(s.f_ff1_b), F(s.f_ff1_s), stream);
        if (st == LD_OK) st = mlp_out_fold_launch(u->pt.ptr(s.pout_w), u->pt.ptr(s.ff2_w), u->pt.ptr(s.ff2_b), u->pt.ptr(s.pout_b), C, H(s.f_mo_w), H(s.f_mo_b), stream);
        if (st != LD_OK) return st;
    }
    for (const ResW& r : u->res) {
        if (r.sk_w < 0) continue;
        const int st = skip_fold_launch(u->pt.ptr(r.c2_w), u->pt.ptr(r.sk_w), u->pt.ptr(r.c2_b), u->pt.ptr(r.sk_b), r.cout, 9 * r.cout, r.cin,
                                        reinterpret_cast<half_t*>(u->fold_base + r.f_c2_w), reinterpret_cast<half_t*>(u->fold_base + r.f_c2_b), stream);
        if (st != LD_OK) return st;
    }
    for (const ConvW& c : u->convs) {
        if (c.f_up < 0) continue;
        const int st = upconv_fold_launch(u->pt.ptr(c.w), c.cout, c.cin, reinterpret_cast<half_t*>(u->fold_base + c.f_up), stream);
        if (st != LD_OK) return st;
    }
    u->fold_dirty = false;
    return LD_OK;
}

// the row-resident kernel's copies of the 3x3 convolution weights (conv8.hip), once per weight load
int derive_conv8_weights(ld_unet* u, hipStream_t stream) {
    for (const ld_unet::W8& w : u->w8_list) {
        const int st = conv8_repack_launch(u->pt.ptr(w.slot), w.N, w.Cin, reinterpret_cast<half_t*>(u->w8_base + w.off), stream);
        if (st != LD_OK) return st;
    }
    return LD_OK;
}

// every copy derived from the resident weights, re-derived when a load, a patch or an unpatch has changed them (fold_dirty)
int refresh_derived(ld_unet* u, hipStream_t stream) {
    if (!u->fold_dirty) return LD_OK;
    if (u->w8_base != nullptr) {
        const int st = derive_conv8_weights(u, stream);
        if (st != LD_OK) return st;
    }
    const int st = fold_layernorms(u, stream);
    if (st != LD_OK) return st;
    u->fold_dirty = false;
    return LD_OK;
}

// (C, H, W) of the skip tensors of an h x w latent, one per input block, as the walk below produces them
std::vector<ld_unet::ResShape> skip_shapes(const ld_unet* u, int h, int w) {
    std::vector<ld_unet::ResShape> s;
    int C = u->cfg.model_channels, H = h, W = w;
    for (const auto& block : u->in_blocks) {
        for (const Layer& L : block) {
            if (L.kind == L_RES) C = u->res[L.idx].cout;
            else if (L.kind == L_DOWN) {
                C = u->convs[L.idx].cout;
                H = (H - 1) / 2 + 1;
                W = (W - 1) / 2 + 1;
            }
        }
        s.push_back({C, H, W});
    }
    return s;
}

// does `ctl` fit the skip tensors and the middle tensor of an n x h x w forward of this UNet?
int check_control(const ld_unet* u, const ld_control* ctl, int n, int h, int w) {
    if (ctl == nullptr) return LD_OK;
    const std::vector<ld_unet::ResShape> s = skip_shapes(u, h, w);
    if (ctl->count != (int)s.size() || ctl->count + 1 > CONTROL_MAX_SEGMENTS || ctl->r_n < 1 || n % ctl->r_n != 0) return LD_ERR_SHAPE;
    for (int i = 0; i <= ctl->count; ++i) {
        const ld_unet::ResShape& want = s[i < ctl->count ? i : ctl->count - 1];   // (the middle block keeps the last skip's shape)
        if (ctl->c[i] != want.C || ctl->h[i] != want.H || ctl->w[i] != want.W) return LD_ERR_SHAPE;
        if ((i < ctl->count ? ctl->residual[i] : ctl->middle) == nullptr) return LD_ERR_ARG;
    }
    return LD_OK;
}

// `pair`: classifier-free-guidance pair (LD_FWD_PAIR).  x / sigma hold n / 2 samples; the batch is [uncond x n/2 ; cond x n/2] of the SAME latents
// (what calc_cond_batch feeds the model: cat([x, x]), LD.py:2515-2547); the resident context has n rows.  The layers in front of the first
// cross-attention run once on n / 2 samples (Run::pair_pending), everything else on n.  out: n samples.
// `ctl` (a UNet, may be null): ControlNet residuals added to every skip tensor and to the middle block's output, once the encoder is done with them.
int run_forward(ld_unet* u, bool dry, const float* x, const float* sigma, float* out, int n, int h, int w, int eps_only, hipStream_t stream,
                size_t* dry_peak = nullptr, bool pair = false, const ld_control* ctl = nullptr) {
    if (!dry) {
        const int st = refresh_derived(u, stream);
        if (st != LD_OK) return st;
    }
    if (pair && (n & 1)) return LD_ERR_SHAPE;
    Run R(u, n);
    Arena plan;
    Exec& ex = R.ex = u->begin(dry, stream, plan);
    Arena& ar = *ex.arena;
    const ld_unet_config& c = u->cfg;
    const int mc = c.model_channels, ted = u->ted;
    const int in_mod = pair ? n / 2 : 0;   // CFG pair: x / sigma hold n / 2 samples; the kernels that read them per sample index n % in_mod
    // (the control branch shares no prefix: its pair form reads x / sigma per sample % (n / 2), duplicates conv_in's output and runs all n samples)
    if (pair && !u->control) R.begin_pair();
    // one launch of the control add over `count` segments of n samples each
    auto control_add = [&](const ControlSegment* segs, int count, int r_n, float strength) {
        long long bytes = 0;
        for (int i = 0; i < count; ++i) bytes += (long long)n * segs[i].per * (long long)sizeof(half_t);
        ex.launch(KC_MISC, 0.0, "ctl_add", bytes, count, r_n, 1, "control_add_kernel", [&] { return control_add_launch(segs, count, n, r_n, strength, stream); });
    };
    // control mode: residual i = zero convolution i (1x1) of the block's output, into the handle's persistent buffer
    auto zero_conv = [&](size_t i, const Feat& f) {
        R.conv3(f.p, f.C, nullptr, 0, f.H, f.W, f.H, f.W, 1, u->zc_w[i], u->zc_b[i], f.C, dry ? nullptr : u->res_buf[i], 1);
        if (!dry) u->res_shape[i] = {f.C, f.H, f.W};
    };

    // timestep embedding -> time_embed MLP -> all ResBlock emb_layers at once (every consumer applies SiLU first)
    half_t* temb = ar.halfs((size_t)n * mc);
    ex.launch(KC_MISC, 0.0, "", 0, 0, 0, 0, "timestep_embed_kernel", [&] { return timestep_embed_launch(sigma, u->log_sigmas, 1000, n, mc, temb, nullptr, stream, in_mod); });
    half_t* e1 = ar.halfs((size_t)n * ted);
    R.linear(temb, mc, u->te0_w, u->te0_b, nullptr, e1, n, ted, mc, 1);
    half_t* semb = ar.halfs((size_t)n * ted);
    R.linear(e1, ted, u->te2_w, u->te2_b, nullptr, semb, n, ted, ted, 1);
    half_t* emb_all = ar.halfs((size_t)n * u->emb_total);
    R.linear(semb, ted, u->res[0].emb_w, u->res[0].emb_b, nullptr, emb_all, n, u->emb_total, ted);
    R.emb_all = emb_all;

    auto run_layers = [&](const std::vector<Layer>& layers, Feat f, const half_t* x2, int C2, int outH, int outW) -> Feat {
        for (const Layer& L : layers) {
            switch (L.kind) {
                case L_RES: {
                    f = R.resblock(u->res[L.idx], f.p, f.C, x2, C2, f.H, f.W, f.stats);
                    x2 = nullptr;
                    C2 = 0;
                    break;
                }
                case L_ST: f = R.transformer(u->st[L.idx], f.p, f.H, f.W, f.stats); break;
                case L_DOWN: {
                    const ConvW& cw = u->convs[L.idx];
                    const int Ho = (f.H - 1) / 2 + 1, Wo = (f.W - 1) / 2 + 1;
                    if (R.pair_pending)                           // (not in front of the first transformer of any supported layout; be safe)
                        R.hand_over({f.p}, (size_t)R.n * f.H * f.W * f.C * sizeof(half_t));
                    half_t* o = ar.halfs((size_t)n * Ho * Wo * cw.cout);
                    float* gno = ex.gn_buffer(n, Ho * Wo);
                    f = {o, cw.cout, Ho, Wo, R.conv3(f.p, f.C, nullptr, 0, f.H, f.W, f.H, f.W, 2, cw.w, cw.b, cw.cout, o, 3, gno)};
                    break;
                }
                case L_UP: {   // Upsample1: nearest resize to the next skip's H x W, then conv (LD.py:5141-5152)
                    const ConvW& cw = u->convs[L.idx];
                    const int Hv = outH > 0 ? outH : f.H * 2, Wv = outW > 0 ? outW : f.W * 2;
                    half_t* o = ar.halfs((size_t)n * Hv * Wv * cw.cout);
                    // (the folded weights are an offer: gemm_plan takes them for an exact 2x resize above the row-resident kernel's batch.  The launch is
                    // counted as the 3x3 convolution it implements — last_flops is algorithmic work — and executes 4/9 of it)
                    const half_t* wup = (u->fold_base != nullptr && cw.f_up >= 0) ? reinterpret_cast<const half_t*>(u->fold_base + cw.f_up) : nullptr;
                    R.conv3(f.p, f.C, nullptr, 0, f.H, f.W, Hv, Wv, 1, cw.w, cw.b, cw.cout, o, 3, nullptr, wup);
                    f = {o, cw.cout, Hv, Wv};
                    break;
                }
                default: break;
            }
        }
        return f;
    };

    std::vector<Feat> hs;
    Feat f{nullptr, 0, h, w};
    {   // input_blocks[0]: conv_in fused with EPS.calculate_input and the fp32 NCHW -> fp16 NHWC layout change
        const ConvW& cw = u->convs[u->in_blocks[0][0].idx];
        half_t* o = ar.halfs((size_t)n * h * w * mc);
        SmallConvInArgs a;
        a.x = x; a.scale_sigma = sigma; a.w = u->pt.ptr(cw.w); a.b = u->pt.ptr(cw.b); a.y = o;
        a.N = R.n; a.Cin = c.in_channels; a.H = h; a.W = w; a.Cout = mc;
        if (R.pair_pending) a.dup_off = (long long)R.n * h * w * mc;   // a skip connection: read by the last output block on all n samples
        if (u->control && pair) {                                 // the control branch's pair form: conv_in once per latent, stored for both halves
            a.N = n / 2;
            a.dup_off = (long long)a.N * h * w * mc;
        }
        ex.launch(KC_MISC, 2.0 * a.N * h * w * mc * 9.0 * c.in_channels, "", 0, 0, 0, 0, "small_conv_in_kernel", [&] { return small_conv_in_launch(a, stream); });
        f = {o, mc, h, w};
        hs.push_back(f);
        if (u->control) {                                         // h = conv_in(x) + hint (cldm.ControlNet.forward: guided_hint joins the first block's output)
            const ControlSegment seg{o, u->hint, (long long)h * w * mc};
            control_add(&seg, 1, dry ? 1 : u->hint_b, 1.0f);
            zero_conv(0, f);
        }
    }
    for (size_t b = 1; b < u->in_blocks.size(); ++b) {
        f = run_layers(u->in_blocks[b], f, nullptr, 0, 0, 0);
        if (u->control) zero_conv(b, f);
        if (R.pair_pending && b == 1) {                          // no transformer in the first block: its output is the last shared tensor
            R.hand_over({f.p}, (size_t)R.n * f.H * f.W * f.C * sizeof(half_t));
            f.stats = {};                                        // (its statistics cover the first half of the batch only)
        }
        hs.push_back(f);
    }
    if (R.pair_pending) R.hand_over();                           // (a UNet without input blocks: nothing left to share)
    f = run_layers(u->mid_block, f, nullptr, 0, 0, 0);
    if (u->control) {                                            // middle_block_out; a control branch ends here
        zero_conv(u->in_blocks.size(), f);
        if (!dry) u->res_n = n;
        return u->end(ex, dry_peak, true);
    }
    if (ctl != nullptr && ctl->strength != 0.0f) {
        // apply_control1 at "output" and "middle" (LD.py:5290, 5742, 5747), all of it in one launch: every skip tensor is complete (on the pair
        // route the second halves of the first two were filled by the hand-over above) and the encoder reads none of them again.  Residual i
        // belongs to hs[i]: upstream pops control["output"] from the back in step with hs.pop().  A strength of 0 adds nothing and launches nothing.
        ControlSegment segs[CONTROL_MAX_SEGMENTS];
        int k = 0;
        for (; k < (int)hs.size() && k < ctl->count && k < CONTROL_MAX_SEGMENTS - 1; ++k)
            segs[k] = {hs[k].p, static_cast<const half_t*>(ctl->residual[k]), (long long)hs[k].H * hs[k].W * hs[k].C};
        segs[k++] = {f.p, static_cast<const half_t*>(ctl->middle), (long long)f.H * f.W * f.C};
        control_add(segs, k, ctl->r_n, ctl->strength);
        f.stats = {};                                            // (they describe the middle tensor as it was before the add)
    }
    for (size_t b = 0; b < u->out_blocks.size(); ++b) {
        const Feat skip = hs.back();
        hs.pop_back();
        if (skip.H != f.H || skip.W != f.W) ex.note(LD_ERR_SHAPE);
        const int oh = hs.empty() ? 0 : hs.back().H, ow = hs.empty() ? 0 : hs.back().W;
        f = run_layers(u->out_blocks[b], f, skip.p, skip.C, oh, ow);
    }
    {   // out: GroupNorm + SiLU, 3x3 conv to 4 channels fused with EPS.calculate_denoised, back to fp32 NCHW
        half_t* g = ar.halfs((size_t)n * f.H * f.W * f.C);
        ex.groupnorm(f.p, f.C, nullptr, 0, n, f.H * f.W, u->pt.ptr(u->outn_g), u->pt.ptr(u->outn_b), 1e-5f, 1, g, f.stats);
        SmallConvOutArgs a;
        a.x = g; a.w = u->pt.ptr(u->outc_w); a.b = u->pt.ptr(u->outc_b);
        a.N = n; a.H = f.H; a.W = f.W; a.Cin = f.C; a.Cout = c.out_channels;
        a.mode = eps_only ? 2 : 0;
        a.x_in = x; a.sigma = sigma; a.out = out; a.in_mod = in_mod;
        ex.launch(KC_MISC, 2.0 * n * f.H * f.W * f.C * 9.0 * c.out_channels, "", 0, 0, 0, 0, "small_conv_out_kernel", [&] { return small_conv_out_launch(a, stream); });
    }
    return u->end(ex, dry_peak, true);
}

// The regions that stay resident behind the activations and the contractions' scratch, each for the reserved maximum and starting on a multiple
// of 256 bytes: the padded context, every transformer's cross-attention K and V^T and, in control mode, the encoded hint and one residual buffer per
// zero convolution.  Stores the pointers in the handle and returns the bytes taken.  ld_unet_reserve carves twice: an arena without a base gives the
// byte count that sizes the workspace, the arena behind the scratch the addresses.
size_t carve_resident(ld_unet* u, Arena& ar, int max_n, int max_h, int max_w) {
    const size_t rows = (size_t)max_n * u->ctx_tpad;
    u->ctx16 = ar.halfs(rows * u->cfg.context_dim);
    for (size_t i = 0; i < u->st.size(); ++i) {
        u->ctx_k[i] = ar.halfs(rows * u->st[i].c);
        u->ctx_vt[i] = ar.halfs(rows * u->st[i].c);
    }
    u->hint = nullptr;
    u->res_buf.clear();
    if (u->control) {
        std::vector<ld_unet::ResShape> rs = skip_shapes(u, max_h, max_w);
        rs.push_back(rs.back());       // (middle_block_out: the middle block keeps the last skip's shape)
        u->hint = ar.halfs((size_t)max_n * max_h * max_w * u->cfg.model_channels);
        for (const auto& r : rs) u->res_buf.push_back(ar.halfs((size_t)max_n * r.H * r.W * r.C));
        u->res_shape.assign(rs.size(), ld_unet::ResShape());
    }
    ar.alloc(0);                       // (the last region takes its padded size too)
    return ar.off;
}

}  // namespace

// ==================================================================================================== C ABI
// LoRA patches: slot -> layout, capture guard
namespace {
// the logical matrix of a slot as a checkpoint stores it, and how the slot keeps it resident (ParamTable::load)
LoraLayout slot_layout(const ParamSlot& s) {
    LoraLayout L;
    switch (s.kind) {
        case PK_CONV3: L.kind = LORA_CONV3; L.rows = (int)s.shape[0]; L.cols = (int)s.shape[1] * 9; break;
        case PK_GEGLU_W: L.kind = LORA_GEGLU; L.rows = (int)s.shape[0]; L.cols = (int)s.shape[1]; L.bn = s.geglu_bn; break;
        case PK_GEGLU_B: L.kind = LORA_GEGLU; L.rows = (int)s.shape[0]; L.cols = 1; L.bn = s.geglu_bn; break;
        case PK_MAT: L.kind = LORA_MAT; L.rows = (int)s.shape[0]; L.cols = (int)(s.elems / s.shape[0]); break;
        default: L.kind = LORA_MAT; L.rows = 1; L.cols = (int)s.elems; break;
    }
    if (L.kind == LORA_GEGLU && L.bn <= 0) L.kind = LORA_MAT;
    return L;
}
bool capturing(hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
}  // namespace

extern "C" {

static int create_handle(const ld_unet_config* cfg, bool control, int hint_channels, ld_unet** out);

int ld_unet_create(const ld_unet_config* cfg, ld_unet** out) { return create_handle(cfg, false, 0, out); }
int ld_controlnet_create(const ld_unet_config* cfg, int hint_channels, ld_unet** out) { return create_handle(cfg, true, hint_channels, out); }

static int create_handle(const ld_unet_config* cfg, bool control, int hint_channels, ld_unet** out) {
    if (cfg == nullptr || out == nullptr) return LD_ERR_ARG;
    ld_unet* u = new ld_unet();
    u->cfg = *cfg;
    u->control = control;
    u->hint_channels = hint_channels;
    const int st = build(u);
    if (st != LD_OK) {
        ld_unet_destroy(u);
        return st;
    }
    // sigma table of ModelSamplingDiscrete (LD.py:1300-1326): scaled-linear betas in fp64, log taken in fp64
    std::vector<float> ls(1000);
    {
        const double b0 = sqrt(0.00085), b1 = sqrt(0.012);
        double ac = 1.0;
        for (int i = 0; i < 1000; ++i) {
            const double sb = b0 + (b1 - b0) * (double)i / 999.0;
            ac *= 1.0 - sb * sb;
            ls[i] = (float)log(sqrt((1.0 - ac) / ac));
        }
    }
    u->w8_of_slot.assign(u->pt.slots.size(), -1);
    for (const ld_unet::W8& w : u->w8_list) u->w8_of_slot[w.slot] = (long long)w.off;
    if (u->w8_bytes > 0 && hipMalloc((void**)&u->w8_base, u->w8_bytes) != hipSuccess) u->w8_base = nullptr;   // (without the copies the general kernels run)
    if ((u->fold_bytes > 0 && hipMalloc((void**)&u->fold_base, u->fold_bytes) != hipSuccess) ||
        hipMalloc((void**)&u->sync_ws, LD_SYNC_INTS * sizeof(int)) != hipSuccess || hipMemset(u->sync_ws, 0, LD_SYNC_INTS * sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&u->log_sigmas, 1000 * sizeof(float)) != hipSuccess ||
        hipMemcpy(u->log_sigmas, ls.data(), 1000 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        ld_unet_destroy(u);
        return LD_ERR_HIP;
    }
    *out = u;
    return LD_OK;
}

void ld_unet_destroy(ld_unet* u) {
    if (u == nullptr) return;
    u->destroy_common();
    if (u->log_sigmas) (void)hipFree(u->log_sigmas);
    if (u->sync_ws) (void)hipFree(u->sync_ws);
    if (u->w8_base) (void)hipFree(u->w8_base);
    if (u->fold_base) (void)hipFree(u->fold_base);
    for (auto& b : u->backups) (void)hipFree(b.second);
    delete u;
}

int ld_unet_param_count(const ld_unet* u) { return abi_param_count(u); }
int ld_unet_param_info(const ld_unet* u, int i, const char** name, int* ndim, int64_t shape[4]) { return abi_param_info(u, i, name, ndim, shape); }
size_t ld_unet_workspace_bytes(const ld_unet* u) { return abi_workspace_bytes(u); }
int ld_unet_last_launches(const ld_unet* u) { return abi_last_launches(u); }
double ld_unet_last_flops(const ld_unet* u) { return abi_last_flops(u); }
int ld_unet_profile_launches(const ld_unet* u, char* buf, size_t buf_bytes) { return abi_profile_launches(u, buf, buf_bytes); }

int ld_unet_load_param(ld_unet* u, const char* name, const void* src, int dtype, void* stream) {
    if (u == nullptr || name == nullptr) return LD_ERR_ARG;
    u->fold_dirty = true;   // the LN-folded copies are re-derived at the next forward
    auto it = u->pt.index.find(name);
    if (it != u->pt.index.end() && u->backups.count(it->second)) {   // a load onto a patched slot is the new base: its backup is dropped
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return LD_ERR_HIP;
        u->drop_backup(it->second);
    }
    return abi_load_param(u, name, src, dtype, stream);
}

// ---------------------------------------------------------------------------------------------------- LoRA patches (load-class calls)
int ld_unet_patch_param(ld_unet* u, const char* name, const ld_lora_term* terms, int n_terms, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (u == nullptr || name == nullptr || terms == nullptr || n_terms < 1 || n_terms > LORA_MAX_TERMS) return LD_ERR_ARG;
    auto it = u->pt.index.find(name);
    if (it == u->pt.index.end()) return LD_ERR_ARG;
    const int slot = it->second;
    const ParamSlot& s = u->pt.slots[slot];
    if (!s.loaded || (s.kind != PK_MAT && s.kind != PK_CONV3 && s.kind != PK_GEGLU_W)) return LD_ERR_ARG;
    LoraArgs a;
    a.lay = slot_layout(s);
    a.n_terms = n_terms;
    for (int j = 0; j < n_terms; ++j) {
        const ld_lora_term& t = terms[j];
        if (t.up == nullptr || t.down == nullptr || t.rank < 1 || t.rank > LORA_MAX_RANK || (t.dtype != LD_F16 && t.dtype != LD_F32)) return LD_ERR_ARG;
        a.t[j].up = t.up; a.t[j].down = t.down; a.t[j].f32 = t.dtype == LD_F32; a.t[j].rank = t.rank; a.t[j].scale = t.scale;
    }
    if (capturing(stream)) return LD_ERR_STATE;
    const size_t bytes = s.elems * sizeof(half_t);
    auto bk = u->backups.find(slot);
    if (bk == u->backups.end()) {   // first patch of this slot: snapshot its resident bytes
        half_t* b = nullptr;
        if (hipMalloc((void**)&b, bytes) != hipSuccess) return LD_ERR_HIP;
        if (hipMemcpyAsync(b, u->pt.ptr(slot), bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess) {
            (void)hipFree(b);
            return LD_ERR_HIP;
        }
        bk = u->backups.emplace(slot, b).first;
        u->patch_bytes += bytes;
    }
    a.base = bk->second;            // always from the backup: re-patching is not cumulative
    a.dst = u->pt.ptr(slot);
    u->fold_dirty = true;
    return lora_merge_launch(a, stream);
}

int ld_unet_unpatch(ld_unet* u, const char* name, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (u == nullptr) return LD_ERR_ARG;
    std::vector<int> which;
    if (name != nullptr) {
        auto it = u->pt.index.find(name);
        if (it == u->pt.index.end()) return LD_ERR_ARG;
        if (u->backups.count(it->second)) which.push_back(it->second);
    } else {
        for (const auto& b : u->backups) which.push_back(b.first);
    }
    if (which.empty()) return LD_OK;
    if (capturing(stream)) return LD_ERR_STATE;
    for (int slot : which)
        if (hipMemcpyAsync(u->pt.ptr(slot), u->backups[slot], u->pt.slots[slot].elems * sizeof(half_t), hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return LD_ERR_HIP;
    u->fold_dirty = true;
    if (hipStreamSynchronize(stream) != hipSuccess) return LD_ERR_HIP;   // the copies have read the backups before they are freed
    for (int slot : which) u->drop_backup(slot);
    return LD_OK;
}

int ld_unet_read_param(const ld_unet* u, const char* name, void* dst_f16, void* stream) {
    if (u == nullptr || name == nullptr || dst_f16 == nullptr) return LD_ERR_ARG;
    auto it = u->pt.index.find(name);
    if (it == u->pt.index.end() || !u->pt.slots[it->second].loaded) return LD_ERR_ARG;
    return lora_read_launch(u->pt.ptr(it->second), slot_layout(u->pt.slots[it->second]), (half_t*)dst_f16, (hipStream_t)stream);
}

size_t ld_unet_patch_bytes(const ld_unet* u) { return u ? u->patch_bytes : 0; }

// what a forward runs under fold_dirty, on the caller's stream: a replayed hipGraph never executes that host code, so the host layer calls
// this after a batch of patches
int ld_unet_refresh_derived(ld_unet* u, void* stream) {
    if (u == nullptr) return LD_ERR_ARG;
    if (!u->pt.all_loaded()) return LD_ERR_STATE;
    if (u->fold_dirty && capturing((hipStream_t)stream)) return LD_ERR_STATE;
    return refresh_derived(u, (hipStream_t)stream);
}

size_t ld_unet_weight_bytes(const ld_unet* u) { return u ? u->pt.bytes + (u->fold_base ? u->fold_bytes : 0) + (u->w8_base ? u->w8_bytes : 0) : 0; }

int ld_unet_reserve(ld_unet* u, int max_n, int max_h, int max_w, int max_tok) {
    if (u == nullptr || max_n < 1 || max_h < 1 || max_w < 1 || max_tok < 1) return LD_ERR_ARG;
    u->free_workspace();   // (the old workspace goes before the new one is planned)
    // plan: dry-run the executor to find the activation peak
    u->planned = PlanKey();
    u->ctx_tok = max_tok;
    u->ctx_tpad = (max_tok + 7) & ~7;
    u->ctx_k.assign(u->st.size(), nullptr);
    u->ctx_vt.assign(u->st.size(), nullptr);
    size_t peak = 0;
    int st = run_forward(u, true, nullptr, nullptr, nullptr, max_n, max_h, max_w, 0, nullptr, &peak);
    if (st != LD_OK) return st;
    if (!(max_n & 1)) {   // the CFG-pair route (LD_FWD_PAIR) keeps the duplicated inputs in the arena as well
        size_t peak2 = 0;
        st = run_forward(u, true, nullptr, nullptr, nullptr, max_n, max_h, max_w, 0, nullptr, &peak2, true);
        if (st != LD_OK) return st;
        if (peak2 > peak) peak = peak2;
    }
    // control mode: the hint encoder's two ping-pong buffers (its widest layer: 16 channels at 8h x 8w) share the activations' arena — it never
    // runs beside a forward
    if (u->control) {
        const size_t hint_ws = 2 * pad256((size_t)max_n * 64 * max_h * max_w * 16 * sizeof(half_t));
        if (hint_ws > peak) peak = hint_ws;
    }
    u->hint_b = u->hint_h = u->hint_w = u->res_n = 0;
    u->splitk_bytes = SPLITK_BYTES;
    Arena sizes;                       // (no base: the regions' byte count)
    const size_t resident = carve_resident(u, sizes, max_n, max_h, max_w);
    const size_t bytes = Model::padded(peak, SPLITK_BYTES + resident), act = bytes - SPLITK_BYTES - resident - 4096;
    st = u->set_workspace(bytes, act);
    if (st != LD_OK) return st;
    u->splitk_ws = reinterpret_cast<float*>(u->ws_base + act);   // behind the activations: the contractions' scratch, then the resident regions
    Arena behind;
    behind.base = u->ws_base + act + u->splitk_bytes;
    carve_resident(u, behind, max_n, max_h, max_w);
    if (getenv("LD_PROFILE_DUMP") != nullptr)   // (where the allocations landed: tools/alloc_probe.py)
        fprintf(stderr, "[ld_reserve] workspace %p (%zu MiB)  weights %p  folds %p  conv8 weights %p\n", (void*)u->ws_base, u->ws_bytes >> 20, (void*)u->pt.base,
                (void*)u->fold_base, (void*)u->w8_base);
    u->max_n = max_n;
    u->max_h = max_h;
    u->max_w = max_w;
    u->max_tok = max_tok;
    u->ctx_n = 0;
    return LD_OK;
}

int ld_unet_set_context(ld_unet* u, const void* ctx, int dtype, int n, int tokens, void* stream_) {
    if (u == nullptr || ctx == nullptr) return LD_ERR_ARG;
    if (u->ws_base == nullptr || !u->pt.all_loaded()) return LD_ERR_STATE;
    if (n < 1 || n > u->max_n || tokens < 1 || tokens > u->max_tok) return LD_ERR_SHAPE;
    hipStream_t stream = (hipStream_t)stream_;
    const int D = u->cfg.context_dim, Tp = (tokens + 7) & ~7;
    int st = ctx_pad_launch(ctx, dtype == LD_F32, n, tokens, Tp, D, u->ctx16, stream);
    if (st != LD_OK) return st;
    for (size_t i = 0; i < u->st.size(); ++i) {
        const StW& s = u->st[i];
        // K = ctx · Wk^T : [n*Tp][C]
        st = gemm_launch(linear_params(u->ctx16, D, u->pt.ptr(s.k2_w), nullptr, n * Tp, s.c, D, u->ctx_k[i]), stream);
        if (st != LD_OK) return st;
        GemmParams v = linear_params(u->pt.ptr(s.v2_w), D, u->ctx16, nullptr, s.c, Tp, D, u->ctx_vt[i]);   // V^T[b] = Wv · ctx_b^T : [C][Tp]
        v.batch = n; v.sW = (long long)Tp * D; v.sC = (long long)s.c * Tp;
        st = gemm_launch(v, stream);
        if (st != LD_OK) return st;
    }
    u->ctx_n = n;
    u->ctx_tok = tokens;
    u->ctx_tpad = Tp;
    return LD_OK;
}

// What both forwards ask of their flags, on the host: LD_ERR_ARG for a bit that is not a flag, for eps of a pair (no kernel writes it) and for eps
// of a control branch (it writes no output); LD_ERR_SHAPE for a pair of no samples.  *n: the samples x / sigma hold -> the batch that runs.
static int check_flags(int flags, bool control, int* n) {
    if ((flags & ~(LD_FWD_EPS_ONLY | LD_FWD_PAIR)) != 0 || flags == (LD_FWD_EPS_ONLY | LD_FWD_PAIR) || (control && (flags & LD_FWD_EPS_ONLY))) return LD_ERR_ARG;
    if (flags & LD_FWD_PAIR) {
        if (*n < 1) return LD_ERR_SHAPE;
        *n *= 2;
    }
    return LD_OK;
}

static int forward_checked(ld_unet* u, const float* x, const float* sigma, float* out, int n, int h, int w, int flags, const ld_control* ctl, void* stream) {
    int st = check_flags(flags, false, &n);
    if (st != LD_OK) return st;
    if (u == nullptr || x == nullptr || sigma == nullptr || out == nullptr || u->control) return LD_ERR_ARG;
    if (ctl != nullptr && h >= 1 && w >= 1 && n >= 1) {
        st = check_control(u, ctl, n, h, w);
        if (st != LD_OK) return st;
    }
    const bool pair = flags & LD_FWD_PAIR;
    const int eps_only = flags & LD_FWD_EPS_ONLY;
    return abi_checked_run(*u, u->ctx_n != 0, n == u->ctx_n && n <= u->max_n && h >= 1 && w >= 1,
                           [&](size_t* peak) { return run_forward(u, true, nullptr, nullptr, nullptr, n, h, w, eps_only, nullptr, peak, pair); },
                           [&] { return run_forward(u, false, x, sigma, out, n, h, w, eps_only, (hipStream_t)stream, nullptr, pair, ctl); },
                           &u->planned, PlanKey{{n, h, w, (int)pair}});
}

// ---------------------------------------------------------------------------------------------------- ControlNet
int ld_controlnet_set_hint(ld_unet* cn, const float* image_nchw, int hb, int H, int W, void* stream_) {
    if (cn == nullptr || image_nchw == nullptr || !cn->control) return LD_ERR_ARG;
    if (cn->ws_base == nullptr || !cn->pt.all_loaded()) return LD_ERR_STATE;
    if (hb < 1 || hb > cn->max_n || H < 8 || W < 8 || H % 8 != 0 || W % 8 != 0 || H / 8 > cn->max_h || W / 8 > cn->max_w) return LD_ERR_SHAPE;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t half_ws = pad256((size_t)hb * H * W * 16 * sizeof(half_t));   // the widest layer's output
    if (2 * half_ws > cn->arena.cap) return LD_ERR_SHAPE;
    half_t* buf[2] = {reinterpret_cast<half_t*>(cn->ws_base), reinterpret_cast<half_t*>(cn->ws_base + half_ws)};
    cn->hint_b = 0;
    const half_t* src = nullptr;
    int h = H, w = W;
    Arena none;
    Exec ex = cn->begin(false, stream, none);   // counted and named as a forward's launches are: last_launches is 8 behind a set_hint
    for (size_t i = 0; i < cn->hint_convs.size(); ++i) {
        const ld_unet::HintW& L = cn->hint_convs[i];
        const bool last = i + 1 == cn->hint_convs.size();
        half_t* dst = last ? cn->hint : buf[i & 1];
        const int ho = (h - 1) / L.stride + 1, wo = (w - 1) / L.stride + 1;
        ex.launch(KC_MISC, 2.0 * hb * ho * wo * L.cout * 9.0 * L.cin, "hint_conv", (long long)hb * ho * wo, L.cout, 9 * L.cin, L.stride, "hint_conv_kernel", [&] {
            return hint_conv_launch(src, i == 0 ? image_nchw : nullptr, hb, h, w, L.cin, cn->pt.ptr(L.w), cn->pt.ptr(L.b), L.cout, L.stride, !last, dst, stream);
        });
        h = ho;
        w = wo;
        src = dst;
    }
    const int st = cn->end(ex, nullptr, true);
    if (st != LD_OK) return st;
    cn->hint_b = hb;
    cn->hint_h = h;
    cn->hint_w = w;
    return LD_OK;
}

static int control_forward_checked(ld_unet* cn, const float* x, const float* sigma, int n, int h, int w, int flags, void* stream) {
    const int st = check_flags(flags, true, &n);
    if (st != LD_OK) return st;
    if (cn == nullptr || x == nullptr || sigma == nullptr || !cn->control) return LD_ERR_ARG;
    if (cn->hint_b == 0) return LD_ERR_STATE;
    const bool pair = flags & LD_FWD_PAIR;
    const bool shape_ok = n == cn->ctx_n && n <= cn->max_n && h >= 1 && w >= 1 && h <= cn->max_h && w <= cn->max_w && h == cn->hint_h && w == cn->hint_w &&
                          n % cn->hint_b == 0;
    return abi_checked_run(*cn, cn->ctx_n != 0, shape_ok,
                           [&](size_t* peak) { return run_forward(cn, true, nullptr, nullptr, nullptr, n, h, w, 0, nullptr, peak, pair); },
                           [&] { return run_forward(cn, false, x, sigma, nullptr, n, h, w, 0, (hipStream_t)stream, nullptr, pair); },
                           &cn->planned, PlanKey{{n, h, w, (int)pair}});
}

int ld_controlnet_forward(ld_unet* cn, const float* x, const float* sigma, int n, int h, int w, int flags, void* stream) {
    return control_forward_checked(cn, x, sigma, n, h, w, flags, stream);
}

int ld_controlnet_profile(ld_unet* cn, const float* x, const float* sigma, int n, int h, int w, int flags, void* stream) {
    return abi_profile(cn, stream, [&] { return control_forward_checked(cn, x, sigma, n, h, w, flags, stream); });
}

int ld_controlnet_read_hint(const ld_unet* cn, void* dst_f16, int* hb, int* h, int* w, int* C, void* stream) {
    if (cn == nullptr || !cn->control) return LD_ERR_ARG;
    if (cn->hint_b == 0 || cn->hint == nullptr) return LD_ERR_STATE;
    if (hb) *hb = cn->hint_b;
    if (h) *h = cn->hint_h;
    if (w) *w = cn->hint_w;
    if (C) *C = cn->cfg.model_channels;
    if (dst_f16 == nullptr) return LD_OK;
    const size_t bytes = (size_t)cn->hint_b * cn->hint_h * cn->hint_w * cn->cfg.model_channels * sizeof(half_t);
    return hipMemcpyAsync(dst_f16, cn->hint, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? LD_OK : LD_ERR_HIP;
}

int ld_controlnet_residual_count(const ld_unet* cn) { return cn != nullptr && cn->control ? (int)cn->in_blocks.size() : 0; }

int ld_controlnet_residual_batch(const ld_unet* cn) { return cn != nullptr && cn->control ? cn->res_n : 0; }

int ld_controlnet_residual(const ld_unet* cn, int i, const void** ptr, int* C, int* H, int* W) {
    if (cn == nullptr || !cn->control || i < 0 || i > (int)cn->in_blocks.size()) return LD_ERR_ARG;
    if (cn->res_n == 0 || cn->res_buf.size() <= (size_t)i) return LD_ERR_STATE;
    if (ptr) *ptr = cn->res_buf[i];
    if (C) *C = cn->res_shape[i].C;
    if (H) *H = cn->res_shape[i].H;
    if (W) *W = cn->res_shape[i].W;
    return LD_OK;
}

int ld_controlnet_read_residual(const ld_unet* cn, int i, void* dst_f16, void* stream) {
    const void* p = nullptr;
    int C = 0, H = 0, W = 0;
    if (dst_f16 == nullptr) return LD_ERR_ARG;
    const int st = ld_controlnet_residual(cn, i, &p, &C, &H, &W);
    if (st != LD_OK) return st;
    return hipMemcpyAsync(dst_f16, p, (size_t)cn->res_n * C * H * W * sizeof(half_t), hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? LD_OK : LD_ERR_HIP;
}

int ld_controlnet_fill_control(const ld_unet* cn, int r_n, float strength, ld_control* out) {
    if (out == nullptr) return LD_ERR_ARG;
    const int count = ld_controlnet_residual_count(cn);
    if (count < 1 || count + 1 > CONTROL_MAX_SEGMENTS) return LD_ERR_ARG;
    memset(out, 0, sizeof *out);
    for (int i = 0; i <= count; ++i) {
        const void* p = nullptr;
        const int st = ld_controlnet_residual(cn, i, &p, &out->c[i], &out->h[i], &out->w[i]);
        if (st != LD_OK) return st;
        if (i < count) out->residual[i] = p;
        else out->middle = p;
    }
    out->count = count;
    out->r_n = r_n > 0 ? r_n : cn->res_n;
    out->strength = strength;
    return LD_OK;
}

int ld_unet_forward(ld_unet* u, const float* x, const float* sigma, float* out, int n, int h, int w, int flags, const ld_control* ctl, void* stream) {
    return forward_checked(u, x, sigma, out, n, h, w, flags, ctl, stream);
}

int ld_unet_profile(ld_unet* u, const float* x, const float* sigma, float* out, int n, int h, int w, int flags, const ld_control* ctl, void* stream,
                    double ms[6], double flops[6], int launches[6]) {
    if (u == nullptr || ms == nullptr || flops == nullptr || launches == nullptr) return LD_ERR_ARG;
    const int st = abi_profile(u, stream, [&] { return forward_checked(u, x, sigma, out, n, h, w, flags, ctl, stream); });
    if (st != LD_OK) return st;
    for (int i = 0; i < KC_COUNT; ++i) {
        ms[i] = u->timing.ms[i];
        flops[i] = u->timing.flops[i];
        launches[i] = u->timing.launches[i];
    }
    return LD_OK;
}

int ld_unet_profile_kernels(const ld_unet* u, char* buf, size_t buf_bytes) {
    if (u == nullptr || buf == nullptr || buf_bytes == 0) return LD_ERR_ARG;
    size_t off = 0;
    buf[0] = 0;
    for (const auto& kv : u->timing.per_kernel) {
        const int w = snprintf(buf + off, buf_bytes - off, "%s\t%d\t%.6f\t%.0f\n", kv.first.c_str(), kv.second.launches, kv.second.ms, kv.second.flops);
        if (w < 0 || (size_t)w >= buf_bytes - off) return LD_ERR_ARG;   // buffer too small
        off += (size_t)w;
    }
    return LD_OK;
}

}  // extern "C"
