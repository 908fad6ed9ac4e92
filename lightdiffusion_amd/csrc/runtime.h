// Host-side runtime shared by the executors (UNet, VAE, ESRGAN, TAESD): resident weight table (checkpoint names -> repacked
// fp16 device tensors), a bump arena for activations with mark/release (stack discipline, deterministic addresses
// so a whole forward can be captured into a hipGraph), and an Exec context that counts launches / FLOPs and
// doubles as a dry-run planner (sizes the arena without touching the GPU).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <vector>

#include "gemm_params.h"

enum ParamKind { PK_VEC = 0, PK_MAT = 1, PK_CONV3 = 2, PK_GEGLU_W = 3, PK_GEGLU_B = 4 };

struct ParamSlot {
    std::string name;
    int ndim = 0;
    int64_t shape[4] = {0, 0, 0, 0};
    int kind = PK_VEC;
    int geglu_bn = 0;
    size_t elems = 0, offset = 0;
    bool loaded = false;
};

struct ParamTable {
    std::vector<ParamSlot> slots;
    std::unordered_map<std::string, int> index;
    size_t bytes = 0;
    char* base = nullptr;

    int add(const std::string& name, int kind, std::initializer_list<int64_t> shape, size_t align = 256, int geglu_bn = 0) {
        ParamSlot s;
        s.name = name;
        s.kind = kind;
        s.geglu_bn = geglu_bn;
        s.ndim = (int)shape.size();
        s.elems = 1;
        int i = 0;
        for (int64_t d : shape) {
            s.shape[i++] = d;
            s.elems *= (size_t)d;
        }
        bytes = (bytes + align - 1) / align * align;
        s.offset = bytes;
        bytes += s.elems * sizeof(half_t);
        index[name] = (int)slots.size();
        slots.push_back(s);
        return (int)slots.size() - 1;
    }
    int finalize() {
        bytes = (bytes + 255) / 256 * 256;
        if (hipMalloc((void**)&base, bytes + 256) != hipSuccess) return LD_ERR_HIP;
        return LD_OK;
    }
    void destroy() {
        if (base) (void)hipFree(base);
        base = nullptr;
    }
    half_t* ptr(int slot) const { return slot < 0 ? nullptr : reinterpret_cast<half_t*>(base + slots[slot].offset); }
    bool all_loaded() const {
        for (const auto& s : slots)
            if (!s.loaded) return false;
        return true;
    }
    int load(const char* name, const void* src, int dtype, hipStream_t stream) {
        auto it = index.find(name);
        if (it == index.end() || src == nullptr || base == nullptr) return LD_ERR_ARG;
        ParamSlot& s = slots[it->second];
        half_t* dst = ptr(it->second);
        int st;
        const int f32 = dtype == 1;
        switch (s.kind) {
            case PK_CONV3: st = repack_conv3x3_launch(src, f32, (int)s.shape[0], (int)s.shape[1], dst, stream); break;
            case PK_GEGLU_W: st = repack_rows_launch(src, f32, (int)s.shape[0], (int)s.shape[1], dst, s.geglu_bn, stream); break;
            case PK_GEGLU_B: st = repack_rows_launch(src, f32, (int)s.shape[0], 1, dst, s.geglu_bn, stream); break;
            case PK_MAT: st = repack_rows_launch(src, f32, (int)s.shape[0], (int)(s.elems / s.shape[0]), dst, 0, stream); break;
            default: st = repack_rows_launch(src, f32, 1, (int)s.elems, dst, 0, stream); break;
        }
        if (st == LD_OK) s.loaded = true;
        return st;
    }
};

struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0, peak = 0;
    void* alloc(size_t bytes) {
        off = (off + 255) / 256 * 256;
        void* p = base + off;
        off += bytes;
        if (off > peak) peak = off;
        return p;
    }
    half_t* halfs(size_t n) { return reinterpret_cast<half_t*>(alloc(n * sizeof(half_t))); }
    size_t mark() const { return off; }
    void release(size_t m) { off = m; }
};

// kernel classes for the per-class timing mode (ld_unet_profile): HIP events recorded on the launch stream
enum KClass { KC_CONV3 = 0, KC_GEMM = 1, KC_ATTN = 2, KC_GNORM = 3, KC_LNORM = 4, KC_MISC = 5, KC_COUNT = 6 };

struct Timing {
    std::vector<hipEvent_t> ev;     // pool, pairs (start, stop)
    std::vector<int> cls;
    std::vector<std::string> desc;   // per launch, only when LD_PROFILE_DUMP is set
    std::vector<const char*> kname;  // per launch: the kernel instantiation that ran (static strings)
    std::vector<double> kflops;      // per launch: algorithmic FLOPs
    struct PerKernel {
        double ms = 0, flops = 0;
        int launches = 0;
    };
    std::vector<std::pair<std::string, PerKernel>> per_kernel;   // filled by collect(), in first-seen order
    struct Launch {                  // one record per timed launch (ld_*_profile_launches)
        const char* what = "";
        long long a = 0, b = 0, d = 0, e = 0;
        float us = 0.f;
    };
    std::vector<Launch> rec;
    bool verbose = false;
    size_t used = 0;
    double ms[KC_COUNT] = {0}, flops[KC_COUNT] = {0};
    int launches[KC_COUNT] = {0};
    hipEvent_t next() {
        if (used == ev.size()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            ev.push_back(e);
        }
        return ev[used++];
    }
    void reset() {
        used = 0;
        cls.clear();
        desc.clear();
        kname.clear();
        kflops.clear();
        per_kernel.clear();
        rec.clear();
        verbose = getenv("LD_PROFILE_DUMP") != nullptr;
        for (int i = 0; i < KC_COUNT; ++i) ms[i] = flops[i] = 0, launches[i] = 0;
    }
    void collect() {
        for (size_t i = 0; i + 1 < used; i += 2) {
            float t = 0.f;
            (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
            ms[cls[i / 2]] += t;
            const char* kn = i / 2 < kname.size() && kname[i / 2] ? kname[i / 2] : "?";
            size_t j = 0;
            while (j < per_kernel.size() && per_kernel[j].first != kn) ++j;
            if (j == per_kernel.size()) per_kernel.push_back({kn, PerKernel()});
            per_kernel[j].second.ms += t;
            per_kernel[j].second.flops += i / 2 < kflops.size() ? kflops[i / 2] : 0.0;
            per_kernel[j].second.launches += 1;
            if (i / 2 < rec.size()) rec[i / 2].us = t * 1e3f;
            if (verbose && i / 2 < desc.size()) fprintf(stderr, "[ld_profile] %8.1f us  %s  %s\n", t * 1e3, desc[i / 2].c_str(), kn);
        }
    }
    void destroy() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
    }
    // "what\ta\tb\tc\td\tflops\tmicroseconds\tkernel\n" per timed launch of the last profiled run, in launch order
    int format_launches(char* buf, size_t buf_bytes) const {
        if (buf == nullptr || buf_bytes == 0) return LD_ERR_ARG;
        size_t off = 0;
        buf[0] = 0;
        for (size_t i = 0; i < rec.size(); ++i) {
            const Launch& r = rec[i];
            const int w = snprintf(buf + off, buf_bytes - off, "%s\t%lld\t%lld\t%lld\t%lld\t%.0f\t%.2f\t%s\n", r.what, r.a, r.b, r.d, r.e,
                                   i < kflops.size() ? kflops[i] : 0.0, r.us, i < kname.size() && kname[i] ? kname[i] : "?");
            if (w < 0 || (size_t)w >= buf_bytes - off) return LD_ERR_ARG;   // buffer too small
            off += (size_t)w;
        }
        return LD_OK;
    }
};

// the name sink of an Exec (Exec::names): kernel names in launch order, joined with ';' (the launchers reset their name on entry: empty = nothing was dispatched)
inline void note_kernel(std::string* sink, const char* name) {
    if (sink == nullptr || name == nullptr || *name == '\0') return;
    if (!sink->empty()) *sink += ';';
    *sink += name;
}

// GroupNorm partial statistics that a tensor's producer left for the GroupNorm that reads the tensor next (gemm.h gn_part: [n][chunks][32][2]
// floats), or none.  The only way statistics travel: gn_stats makes one from the buffer a contraction was asked to fill (want_gn_partials /
// want_gn_tile_partials) and the gn_chunks of the plan that Exec::gemm / Exec::gn_silu_conv returned, and it is empty where that is 0.
struct GnStats {
    float* part = nullptr;
    int chunks = 0;   // pixel chunks per image
    explicit operator bool() const { return chunks > 0; }
};
inline GnStats gn_stats(float* buf, int chunks) { return buf != nullptr && chunks > 0 ? GnStats{buf, chunks} : GnStats{}; }

struct Exec {
    Timing* timing = nullptr;
    hipStream_t stream = nullptr;
    bool dry = false;
    Arena* arena = nullptr;          // activations and per-launch temporaries: the executor's reserved workspace, a private one without a base (dry), or a caller's scratch (capi.hip)
    int status = LD_OK;
    int launches = 0;
    double flops = 0.0;
    float* splitk_ws = nullptr;
    size_t splitk_bytes = 0;
    int* sync_ws = nullptr;          // LD_SYNC_INTS zeroed ints for the in-launch reductions (gemm.h GemmParams::sync); null: those kernels are not used
    std::string* names = nullptr;    // optional: receives the contraction and attention kernels this Exec dispatched (ld_op_last_kernel)
    std::string* all_names = nullptr;   // optional: receives the name of EVERY launch, as the profile tables print it (ld_op_last_launches)
    // optional: runs in front of a contraction's kernel, once its plan is known, with before_gemm_arg; a status other than LD_OK takes the
    // launch's place (capi.hip: what the row-resident kernel needs from a caller's scratch)
    int (*before_gemm)(const GemmParams&, const GemmPlan&, const void* arg, hipStream_t) = nullptr;
    const void* before_gemm_arg = nullptr;

    void note(int st) {
        if (st != LD_OK && status == LD_OK) status = st;
    }
    bool overflow() const { return !dry && arena->peak > arena->cap; }

    void t_begin(int c, double fl, int nl, const char* what = "", long long a = 0, long long b = 0, long long d = 0, long long e = 0) {
        if (timing == nullptr || dry) return;
        timing->cls.push_back(c);
        if (timing->verbose) {
            char buf[160];
            snprintf(buf, sizeof buf, "%-10s %8lld %6lld %6lld %4lld  %.2f GFLOP", what, a, b, d, e, fl * 1e-9);
            timing->desc.push_back(buf);
        }
        timing->flops[c] += fl;
        timing->launches[c] += nl;
        timing->kflops.push_back(fl);
        Timing::Launch r;
        r.what = what;
        r.a = a; r.b = b; r.d = d; r.e = e;
        timing->rec.push_back(r);
        (void)hipEventRecord(timing->next(), stream);
    }
    void t_end(const char* kernel_name = "misc") {
        if (timing == nullptr || dry) return;
        (void)hipEventRecord(timing->next(), stream);
        timing->kname.push_back(kernel_name);
    }

    // Every launch of an executor: counts it (nl kernels behind one timing record) and its algorithmic FLOPs, opens the timing record
    // (class, what, four dimensions), runs fn — which launches and returns an LD_* status — unless this is a dry run or an earlier launch
    // failed, notes the status and closes the record under the kernel's name.
    template <class F>
    void launch(int cls, double fl, const char* what, long long a, long long b, long long d, long long e, const char* kernel_name, F&& fn, int nl = 1) {
        if (open(cls, fl, nl, what, a, b, d, e)) {
            note(fn());
            note_kernel(all_names, kernel_name);
        }
        t_end(kernel_name);
    }
    // ... under the name one of the launchers' last-kernel functions (attention_last_kernel_name ...) gives after fn ran
    template <class F>
    void launch(int cls, double fl, const char* what, long long a, long long b, long long d, long long e, const char* (*last_kernel)(), F&& fn) {
        const bool run = open(cls, fl, 1, what, a, b, d, e);
        if (run) {
            note(fn());
            note_kernel(all_names, last_kernel());
        }
        t_end(run ? last_kernel() : "");
    }
    bool open(int cls, double fl, int nl, const char* what, long long a, long long b, long long d, long long e) {
        flops += fl;
        launches += nl;
        t_begin(cls, fl, nl, what, a, b, d, e);
        return !dry && status == LD_OK;
    }

    // the scratch every contraction of this executor launches with: set before planning, so that the plan is the launch's
    void with_scratch(GemmParams& p) const {
        if (p.batch != 1) return;
        p.partial = splitk_ws; p.partial_bytes = splitk_bytes; p.sync = sync_ws;
    }
    // the plan gemm() launches p by
    GemmPlan plan(GemmParams p) const {
        with_scratch(p);
        return gemm_plan(p);
    }
    // `planned`: gemm_plan of p with this executor's scratch, where the caller already asked for it.  Returns the plan it ran, which says what
    // the launch left behind (kernel, stat_parts, gn_chunks): a default plan — no kernel, no statistics — where it launched nothing (a dry
    // run, or behind a launch that failed), so a dry run sizes the arena for a consumer that computes its own statistics
    GemmPlan gemm(GemmParams p, const GemmPlan* planned = nullptr) {
        with_scratch(p);
        GemmPlan pl;
        if (open(p.conv && p.ksize == 3 ? KC_CONV3 : KC_GEMM, 2.0 * p.M * (double)p.N * p.K * p.batch, 1,
                 p.conv ? (p.ksize == 3 ? "conv3" : "conv1") : (p.act == 2 ? "geglu" : "gemm"), p.M, p.N, p.K, p.batch)) {
            pl = planned != nullptr ? *planned : gemm_plan(p);
            int st = before_gemm != nullptr ? before_gemm(p, pl, before_gemm_arg, stream) : LD_OK;
            if (st == LD_OK) st = gemm_run(p, pl, stream);
            else pl = GemmPlan();
            note(st);
            note_kernel(names, pl.kernel);
            note_kernel(all_names, pl.kernel);
        }
        t_end(pl.kernel);
        return pl;
    }
    // would gemm() run this 3x3 convolution on a kernel that takes a second K segment (gemm.h S1 / S2)?
    bool conv_takes_skip_segment(const GemmParams& p) const { return plan(p).takes_skip_segment; }
    // a buffer for the GroupNorm partial statistics of n images of HW pixels (gemm.h gn_part, norm.hip)
    float* gn_buffer(int n, int HW) { return reinterpret_cast<float*>(arena->alloc(groupnorm_workspace_bytes(n, HW))); }
    // `ready`: partial statistics the producer already wrote: the statistics launch is skipped
    void groupnorm(const half_t* x1, int C1, const half_t* x2, int C2, int n, int HW, const half_t* g, const half_t* b, float eps,
                   int silu, half_t* y, GnStats ready = {}) {
        const size_t m = arena->mark();
        float* ws = ready ? ready.part : gn_buffer(n, HW);
        launch(KC_GNORM, 0.0, "groupnorm", n, HW, C1 + C2, silu, ready ? "gn_apply_kernel" : "gn_stats_kernel+gn_apply_kernel",
               [&] { return groupnorm_launch(x1, C1, x2, C2, n, HW, g, b, eps, silu, y, ws, stream, ready.chunks); }, ready ? 1 : 2);
        arena->release(m);
    }
    // GroupNorm(32) + SiLU feeding a 3x3 convolution.  When the convolution runs on the halo-tile kernel the normalisation is fused
    // into its A operand: only the statistics pass + a tiny finalize run here (scale / shift per image and channel), the conv reads the
    // RAW tensor(s) — no normalised copy is written or read back.  Otherwise: the two-pass GroupNorm into `g` (caller-provided), then the conv.
    // `p`: the convolution with A / A2 = the RAW sources; returns through p.C as usual, and the convolution's plan as gemm() does.
    // `ready`: GroupNorm partial statistics of the input that its producer already wrote (see groupnorm)
    GemmPlan gn_silu_conv(GemmParams p, int n_img, int HW, const half_t* gamma, const half_t* beta, float eps, half_t* g, GnStats ready = {}) {
        with_scratch(p);
        const GemmPlan fused = gemm_plan(p, /*gn_offer=*/true);
        if (fused.can_fuse_groupnorm) {
            const int C = p.C1 + p.C2;
            const size_t m = arena->mark();
            float* ws = ready ? ready.part : gn_buffer(n_img, HW);
            float* scale = reinterpret_cast<float*>(arena->alloc((size_t)n_img * C * sizeof(float)));
            float* shift = reinterpret_cast<float*>(arena->alloc((size_t)n_img * C * sizeof(float)));
            launch(KC_GNORM, 0.0, "gn_stats", n_img, HW, C, 1, ready ? "gn_finalize_kernel" : "gn_stats_kernel+gn_finalize_kernel", [&] {
                return groupnorm_scale_shift_launch(p.A, p.C1, p.A2, p.C2, n_img, HW, gamma, beta, eps, ws, scale, shift, stream, ready.chunks);
            }, ready ? 1 : 2);
            p.gn_scale = scale;
            p.gn_shift = shift;
            p.gn_silu = 1;
            const GemmPlan ran = gemm(p, &fused);
            arena->release(m);
            return ran;
        }
        groupnorm(p.A, p.C1, p.A2, p.C2, n_img, HW, gamma, beta, eps, 1, g, ready);
        p.A = g;
        p.A2 = nullptr;
        p.C1 = p.C1 + p.C2;
        p.C2 = 0;
        return gemm(p);
    }
    void attention(const AttnParams& p) {
        launch(KC_ATTN, 4.0 * p.B * p.H * (double)p.Lq * p.Lk * p.d, "attention", (long long)p.B * p.H, p.Lq, p.Lk, p.d, attention_last_kernel_name, [&] {
            const int st = attention_launch(p, stream);
            note_kernel(names, attention_last_kernel_name());
            return st;
        });
    }
};

constexpr size_t SPLITK_BYTES = (size_t)96 << 20;   // the scratch of the contractions the UNet and the VAE carve behind their activations

// ---- What the four resident models (ld_unet, ld_vae, ld_esrgan, ld_taesd) share: the weight table, the reserved workspace, the last run's
// counts and the timing of a profiled run.  Each family derives its handle from this, adds its own slots and state, and walks its own blocks.
struct Model {
    ParamTable pt;
    Arena arena;                     // activations: the front of the workspace
    char* ws_base = nullptr;
    size_t ws_bytes = 0;
    float* splitk_ws = nullptr;      // scratch of the contractions inside the workspace (UNet, VAE); null: the family has none
    size_t splitk_bytes = 0;
    int* sync_ws = nullptr;          // LD_SYNC_INTS zeroed ints for the in-launch reductions (gemm.h GemmParams::sync); UNet only
    int last_launches = 0;
    double last_flops = 0.0;
    Timing timing;
    bool want_timing = false;

    // the opening of every run: a dry run bumps the caller's private arena (no base: sizes only), a real one the reserved workspace
    Exec begin(bool dry, hipStream_t stream, Arena& dry_arena) {
        Exec ex;
        ex.stream = stream;
        ex.dry = dry;
        ex.arena = dry ? &dry_arena : &arena;
        ex.splitk_ws = splitk_ws;
        ex.splitk_bytes = splitk_bytes;
        ex.sync_ws = sync_ws;
        if (want_timing && !dry) {
            timing.reset();
            ex.timing = &timing;
        }
        ex.arena->release(0);
        return ex;
    }
    // ... and its close.  `record`: keep the run's counts as last_*; the UNet and the VAE do so on every run, ESRGAN and TAESD on real runs only
    int end(const Exec& ex, size_t* dry_peak, bool record) {
        if (record) {
            last_launches = ex.launches;
            last_flops = ex.flops;
        }
        if (dry_peak != nullptr) *dry_peak = ex.arena->peak;
        return ex.status;
    }

    // bytes of a workspace whose activations peak at `peak`: rounded up to 4096, the family's regions behind them (`extra`), a 4096-byte guard
    static size_t padded(size_t peak, size_t extra = 0) { return (peak + 4095) / 4096 * 4096 + extra + 4096; }
    void free_workspace() {
        if (ws_base) (void)hipFree(ws_base);
        ws_base = nullptr;
        arena = Arena();
    }
    // replaces the workspace: `total_bytes` in all, the first `act_bytes` of them the arena
    int set_workspace(size_t total_bytes, size_t act_bytes) {
        free_workspace();
        ws_bytes = 0;
        if (hipMalloc((void**)&ws_base, total_bytes) != hipSuccess) {
            ws_base = nullptr;
            return LD_ERR_HIP;
        }
        ws_bytes = total_bytes;
        arena.base = ws_base;
        arena.cap = act_bytes;
        return LD_OK;
    }
    void destroy_common() {
        pt.destroy();
        timing.destroy();
        free_workspace();
    }
};

// ---- the C ABI the four families export alike, over the handle's base (null for a null handle)
inline int abi_param_count(const Model* m) { return m ? (int)m->pt.slots.size() : 0; }
inline size_t abi_workspace_bytes(const Model* m) { return m ? m->ws_bytes : 0; }
inline int abi_last_launches(const Model* m) { return m ? m->last_launches : 0; }
inline double abi_last_flops(const Model* m) { return m ? m->last_flops : 0.0; }
inline int abi_profile_launches(const Model* m, char* buf, size_t buf_bytes) { return m ? m->timing.format_launches(buf, buf_bytes) : LD_ERR_ARG; }
inline int abi_param_info(const Model* m, int i, const char** name, int* ndim, int64_t shape[4]) {
    if (m == nullptr || i < 0 || i >= (int)m->pt.slots.size()) return LD_ERR_ARG;
    const ParamSlot& s = m->pt.slots[i];
    if (name) *name = s.name.c_str();
    if (ndim) *ndim = s.ndim;
    if (shape)
        for (int k = 0; k < 4; ++k) shape[k] = s.shape[k];
    return LD_OK;
}
inline int abi_load_param(Model* m, const char* name, const void* src, int dtype, void* stream) {
    if (m == nullptr || name == nullptr) return LD_ERR_ARG;
    return m->pt.load(name, src, dtype, (hipStream_t)stream);
}
// the workspace a (b, h, w) run needs; dry_run(&peak): the family's host-only dry run(s).  0: no handle, no such shape
template <class Dry>
size_t abi_plan_bytes(const Model* m, int b, int h, int w, Dry&& dry_run, size_t extra_bytes = 0) {
    size_t peak = 0;
    if (m == nullptr || b < 1 || h < 1 || w < 1 || dry_run(&peak) != LD_OK) return 0;
    return Model::padded(peak, extra_bytes);
}
// the last shape (and route) a family validated against the reserved arena, so that a repeated call skips the dry run; zeros: none
struct PlanKey {
    int v[4] = {0, 0, 0, 0};
    bool operator==(const PlanKey& o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2] && v[3] == o.v[3]; }
};
// a real run behind the family's argument check: the handle's state, the shape, a dry run against the reserved arena (unless `planned`
// already holds `shape`), then real()
template <class Dry, class Real>
int abi_checked_run(Model& m, bool state_ok, bool shape_ok, Dry&& dry_run, Real&& real, PlanKey* planned = nullptr, PlanKey shape = PlanKey()) {
    if (m.ws_base == nullptr || !m.pt.all_loaded() || !state_ok) return LD_ERR_STATE;
    if (!shape_ok) return LD_ERR_SHAPE;
    if (planned == nullptr || !(*planned == shape)) {   // new shape: plan it on the host before touching the GPU
        size_t peak = 0;
        const int st = dry_run(&peak);
        if (st != LD_OK) return st;
        if (peak > m.arena.cap) return LD_ERR_SHAPE;
        if (planned != nullptr) *planned = shape;
    }
    return real();
}
// run() with HIP events around every launch; behind one that returned LD_OK: wait for its launches, then read their events
template <class Run>
int abi_profile(Model* m, void* stream, Run&& run) {
    if (m == nullptr) return LD_ERR_ARG;
    m->want_timing = true;
    const int st = run();
    m->want_timing = false;
    if (st != LD_OK) return st;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return LD_ERR_HIP;
    m->timing.collect();
    return LD_OK;
}
