// ---------------------------------------------------------------------------------------------------------------------
// Training rollout of the latent propagator: forward with a tape, backward through time  (included by lns_engine.cpp)
//
// Reference: LatentDynamics.forward (train_stage2_ns2d.py:126-141; SW / two-phase: the same text) -- z_pred[:, t] =
// propagator(z_pred[:, t-1]), started at z_in -- whose loss feeds loss.backward() at train_stage2_ns2d.py:215.  The
// loss function is the caller's (a Python callable in the reference): this module takes dL/dz_pred and returns the
// gradient of every propagator parameter and of z_in.
//
// Forward materialises what the backward needs (the inference plan fuses GroupNorm / GELU into the convolutions and
// never stores their inputs): per step the tape holds, for each DilatedResidualBlock (train_stage2_ns2d.py:25-53),
//   x, n1 = GN1(x), u1 = conv.1(n1), a1 = GELU(u1), u2 = conv.3(a1), a2 = GELU(u2), x1 = x + conv.5(a2),
//   n2 = GN1(x1), v = ffn.1(n2), g = GELU(v), x2 = x1 + ffn.3(g)           and the GroupNorm (mean, rstd).
// Every contraction of this path runs on the exact-fp32 matrix instruction (forward and data-gradient: the inference
// path's conv_mfma_kernel, the latter with transposed + mirrored weight packs; weight-gradient: conv_wgrad_kernel).
// Parameters are read from the caller's DEVICE tensors at every call (an optimiser changes them between calls), and
// packed on the device.  Both propagator kinds: the plain one (NS2d, SW, two-phase) and the conditional one
// (train_stage2_twophase_conditional.py:25-121): there the block is
//   emb = cond_emb(ce) ; h = conv1.3(GELU(conv1.1(GN1(x)))) + emb ; x1 = x + cond_conv1.2(GELU(GN1(h))) ;
//   m = cond_conv2(emb) (GroupNorm / 1x1 convs on [B, D, 1, 1]) ; x2 = x1 + ffn(x1 (1 + m)),
// with ce = cond_emb_proj(fourier_embedding(param)).  ce / emb / m depend on `param` only: they are computed once per
// call, their gradients are accumulated over the steps ([B, D] per block) and pushed through the vector network once.
// lns_train_backward_ex adds the state-only adjoint (no parameter gradient at all) and the gradient w.r.t. `param`; the
// latent fit built on them (observation loss, lns_fit_step) is at the end of this file.
// ---------------------------------------------------------------------------------------------------------------------
#include "lns_train_kernels.h"

namespace {

size_t round64(size_t floats) { return (floats + 63) / 64 * 64; }
size_t round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

struct TConv {                       // one convolution geometry with its gather maps on the device
    int Cin = 0, Cout = 0, k = 1, dil = 1, kc_log2 = 3, Cin_pad = 0, Cout_pad = 0, variant = 0;
    int wg_S = 1;                    // slices of the batch-parallel weight gradient (wgrad_split_slices of the plan's shape)
    ConvArgs base;                   // everything but x / y / w / bias / res
    int* d_maps = nullptr;           // forward kernel's tile maps (rowmap | colmap)
    int* d_full = nullptr;           // whole-image maps of the weight-gradient kernel (rowmap | colmap)
    int full_rows = 0;
    size_t pack_floats() const { return (size_t)k * k * Cin_pad * Cout_pad; }
};

struct TrainPlan {
    int B = 0, H = 0, W = 0, D = 0, c = 0, nb = 0, dil = 1, E = 0; bool cond = false;
    TConv in_proj, in_proj_T, c_d1, c_dd, c_1, out_proj, out_proj_T;     // D->D convs are their own transposes' geometry
    void release() {
        for (TConv* t : {&in_proj, &in_proj_T, &c_d1, &c_dd, &c_1, &out_proj, &out_proj_T}) {
            if (t->d_maps) (void)hipFree(t->d_maps);
            if (t->d_full) (void)hipFree(t->d_full);
            t->d_maps = t->d_full = nullptr;
        }
    }
};

// Training plans hold device memory (tile maps), so they are keyed by the DEVICE as well as by engine and shape; the map is
// shared by every engine of the process and guarded by a mutex (two engines may train from two host threads).  A plan is
// never erased while its engine lives (std::map nodes are stable), so the pointer handed out stays valid after unlock.
struct TrainKey {
    const lns_engine* e; int device; long shape;
    bool operator<(const TrainKey& o) const { return std::tie(e, device, shape) < std::tie(o.e, o.device, o.shape); }
};
std::map<TrainKey, TrainPlan> g_train_plans;
std::mutex g_train_mutex;

// the device a training call runs on = the device its tensors live on (not the engine's inference device, which is -1
// before any lns_finalize_weights and may be another GPU)
int train_device_of(lns_engine* e, const void* dev_ptr, int* device) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, dev_ptr) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        e->err = "training rollout: tensors must be HIP device memory";
        return LNS_EINVAL;
    }
    *device = at.device;
    return LNS_OK;
}
int train_same_device(lns_engine* e, int device, const void* p, const char* what) {
    if (!p) return LNS_OK;
    int d = -1;
    if (int rc = train_device_of(e, p, &d)) return rc;
    if (d != device) { e->err = fmt("training rollout: %s lives on device %d, z_in on device %d", what, d, device); return LNS_EINVAL; }
    return LNS_OK;
}

// channel counts and pads of a convolution: all the workspace layout needs (no device, no tiling)
void tconv_dims(TConv& t, int Cin, int Cout, int k, int dil) {
    t.Cin = Cin; t.Cout = Cout; t.k = k; t.dil = dil;
    const ConvPadded ps = conv_padded_sizes(k, Cin, Cout);
    t.kc_log2 = ps.kc_log2; t.Cin_pad = ps.Cin_pad; t.Cout_pad = ps.Cout_pad;
}

// tiling, device maps and launch arguments of a convolution whose dims train_plan_dims has set
int tconv_setup(lns_engine* e, TConv& t, int B, int H, int W, int my, int mx) {
    const int Cin = t.Cin, Cout = t.Cout, k = t.k, dil = t.dil;
    const int p = dil * (k - 1) / 2;
    const int pad[4] = {p, p, p, p};
    ConvGeom g;
    if (!conv_geometry(g, B, Cout, H, W, k, 1, dil, pad, t.kc_log2, t.Cout_pad, -1)) { e->err = "training: no conv tiling"; return LNS_EINVAL; }
    t.variant = g.variant;
    std::vector<int> rm, cm, fr, fc;
    conv_tile_maps(rm, cm, g, 1, H, W, H, W, 0.0f, 0.0f, pad, my, mx);
    build_axis_map(fr, H + 2 * p, H, H, 0.0f, p, p, my);
    build_axis_map(fc, W + 2 * p, W, W, 0.0f, p, p, mx);
    HIPCHK(e, hipMalloc(reinterpret_cast<void**>(&t.d_maps), (rm.size() + cm.size()) * 4));
    HIPCHK(e, hipMemcpy(t.d_maps, rm.data(), rm.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(t.d_maps + rm.size(), cm.data(), cm.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(e, hipMalloc(reinterpret_cast<void**>(&t.d_full), (fr.size() + fc.size()) * 4));
    HIPCHK(e, hipMemcpy(t.d_full, fr.data(), fr.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(t.d_full + fr.size(), fc.data(), fc.size() * 4, hipMemcpyHostToDevice));
    t.full_rows = (int)fr.size();
    ConvArgs& a = t.base;
    memset(&a, 0, sizeof a);
    conv_set_geometry(a, g, B, Cin, H, W, Cout, k, 1, dil, t.Cin_pad, t.Cout_pad);    // "same" padding: the output plane is H x W
    a.rowmap = t.d_maps; a.colmap = t.d_maps + rm.size();
    a.res_bs = a.y_bs;
    a.unscale = conv_unscale(g.variant, 1.0f);
    return LNS_OK;
}

// sizes of a plan without its device maps: what train_layout reads (the workspace size is known without a GPU)
int train_plan_dims(lns_engine* e, int B, int H, int W, TrainPlan& p) {
    const lns_config& c = e->cfg;
    if (c.prop_kind != LNS_PROP_PLAIN && c.prop_kind != LNS_PROP_CONDITIONAL) { e->err = "training rollout: engine has no propagator"; return LNS_EINVAL; }
    if (H <= 0 || W <= 0 || H > 4096 || W > 4096) { e->err = "training rollout: bad latent size"; return LNS_EINVAL; }
    p.B = B; p.D = c.prop_n_embd; p.c = c.latent_dim; p.nb = c.prop_n_block; p.dil = c.prop_dilation;
    p.H = H; p.W = W;
    p.cond = c.prop_kind == LNS_PROP_CONDITIONAL; p.E = c.cond_emb_dim;
    tconv_dims(p.in_proj, p.c, p.D, 1, 1); tconv_dims(p.in_proj_T, p.D, p.c, 1, 1);
    tconv_dims(p.c_d1, p.D, p.D, 3, 1); tconv_dims(p.c_dd, p.D, p.D, 3, p.dil); tconv_dims(p.c_1, p.D, p.D, 1, 1);
    tconv_dims(p.out_proj, p.D, p.c, 1, 1); tconv_dims(p.out_proj_T, p.c, p.D, 1, 1);
    for (TConv* t : {&p.in_proj, &p.c_d1, &p.c_dd, &p.c_1, &p.out_proj}) t->wg_S = wgrad_split_slices(B, H, W, t->Cin, t->Cout, t->k);
    return LNS_OK;
}

int get_train_plan(lns_engine* e, int device, int B, int H, int W, TrainPlan** out) {
    const TrainKey key{e, device, ((long)B << 32) | ((long)H << 16) | (long)W};
    std::lock_guard<std::mutex> lock(g_train_mutex);
    auto it = g_train_plans.find(key);
    if (it != g_train_plans.end()) { *out = &it->second; return LNS_OK; }
    const lns_config& c = e->cfg;
    TrainPlan p;
    int rc;
    if ((rc = train_plan_dims(e, B, H, W, p))) return rc;
    HIPCHK(e, init_train_kernels());      // dynamic-LDS attributes of the batch-parallel weight gradient: per device, at plan build
    const int my = c.prop_pad_y, mx = c.prop_pad_x;
    for (TConv* t : {&p.in_proj, &p.in_proj_T, &p.c_d1, &p.c_dd, &p.c_1, &p.out_proj, &p.out_proj_T})
        if ((rc = tconv_setup(e, *t, B, p.H, p.W, my, mx))) { p.release(); return rc; }
    auto res = g_train_plans.emplace(key, p);
    *out = &res.first->second;
    return LNS_OK;
}

// parameter-table indices of everything the propagator owns, in network order
struct PropParams {
    int in_w = -1, in_b = -1, out_g = -1, out_be = -1, out_w = -1, out_b = -1;
    struct Blk { int g1, b1, c1w, c1b, c3w, c3b, c5w, c5b, g2, b2, f1w, f3w;
                 // conditional extras: cond_emb Linear, cond_conv1 GN (c5w / c5b hold cond_conv1.2), cond_conv2 GN + two 1x1
                 int ce_w = -1, ce_b = -1, cg = -1, cb = -1, vg = -1, vb = -1, v1w = -1, v1b = -1, v3w = -1, v3b = -1; };
    std::vector<Blk> blk;
    int m0w = -1, m0b = -1, m2w = -1, m2b = -1;        // cond_emb_proj
    std::vector<int> all;                              // every index above (null checks)
};
int find_param(const lns_engine* e, const std::string& key) {
    auto it = e->pindex.find(key);
    return it == e->pindex.end() ? -1 : it->second;
}
int build_prop_params(lns_engine* e, PropParams& pp) {
    const std::string p = e->cfg.prop_prefix;
    const bool cond = e->cfg.prop_kind == LNS_PROP_CONDITIONAL;
    bool ok = true;
    auto F = [&](const std::string& key) { const int i = find_param(e, key); ok = ok && i >= 0; pp.all.push_back(i); return i; };
    pp.in_w = F(p + "in_proj.weight"); pp.in_b = F(p + "in_proj.bias");
    pp.out_g = F(p + "out_proj.0.gn.weight"); pp.out_be = F(p + "out_proj.0.gn.bias");
    pp.out_w = F(p + "out_proj.1.weight"); pp.out_b = F(p + "out_proj.1.bias");
    if (cond) {
        pp.m0w = F(p + "cond_emb_proj.0.weight"); pp.m0b = F(p + "cond_emb_proj.0.bias");
        pp.m2w = F(p + "cond_emb_proj.2.weight"); pp.m2b = F(p + "cond_emb_proj.2.bias");
    }
    for (int i = 0; i < e->cfg.prop_n_block; ++i) {
        const std::string q = p + "net." + std::to_string(i);
        PropParams::Blk b;
        if (!cond) {
            b.g1 = F(q + ".conv.0.weight"); b.b1 = F(q + ".conv.0.bias");
            b.c1w = F(q + ".conv.1.weight"); b.c1b = F(q + ".conv.1.bias");
            b.c3w = F(q + ".conv.3.weight"); b.c3b = F(q + ".conv.3.bias");
            b.c5w = F(q + ".conv.5.weight"); b.c5b = F(q + ".conv.5.bias");
        } else {
            b.ce_w = F(q + ".cond_emb.weight"); b.ce_b = F(q + ".cond_emb.bias");
            b.g1 = F(q + ".conv1.0.weight"); b.b1 = F(q + ".conv1.0.bias");
            b.c1w = F(q + ".conv1.1.weight"); b.c1b = F(q + ".conv1.1.bias");
            b.c3w = F(q + ".conv1.3.weight"); b.c3b = F(q + ".conv1.3.bias");
            b.cg = F(q + ".cond_conv1.0.weight"); b.cb = F(q + ".cond_conv1.0.bias");
            b.c5w = F(q + ".cond_conv1.2.weight"); b.c5b = F(q + ".cond_conv1.2.bias");
            b.vg = F(q + ".cond_conv2.0.weight"); b.vb = F(q + ".cond_conv2.0.bias");
            b.v1w = F(q + ".cond_conv2.1.weight"); b.v1b = F(q + ".cond_conv2.1.bias");
            b.v3w = F(q + ".cond_conv2.3.weight"); b.v3b = F(q + ".cond_conv2.3.bias");
        }
        b.g2 = F(q + ".ffn.0.weight"); b.b2 = F(q + ".ffn.0.bias");
        b.f1w = F(q + ".ffn.1.weight"); b.f3w = F(q + ".ffn.3.weight");
        pp.blk.push_back(b);
    }
    if (!ok) { e->err = "training rollout: propagator parameter missing from the table"; return LNS_EINVAL; }
    return LNS_OK;
}
// The table never changes after lns_create: the indices are looked up once per engine (every training call needs them).
std::map<const lns_engine*, PropParams> g_prop_params;
int prop_params(lns_engine* e, const PropParams** out) {
    std::lock_guard<std::mutex> lock(g_train_mutex);
    auto it = g_prop_params.find(e);
    if (it == g_prop_params.end()) {
        PropParams pp;
        if (int rc = build_prop_params(e, pp)) return rc;
        it = g_prop_params.emplace(e, std::move(pp)).first;
    }
    *out = &it->second;
    return LNS_OK;
}

// The five convolutions of a DilatedResidualBlock (plain or conditional): geometry in the plan, weight and bias (null: none) in
// PropParams::Blk.  in_proj and out_proj (Cin != Cout: the transposed convolution has a geometry of its own) stay outside.
enum BlkConv { BC_C1 = 0, BC_C3, BC_C5, BC_F1, BC_F3, BC_COUNT };      // conv.1, conv.3, conv.5 / cond_conv1.2, ffn.1, ffn.3
struct BlkConvRow { TConv TrainPlan::*geom; int PropParams::Blk::*w; int PropParams::Blk::*b; };
const BlkConvRow kBlkConv[BC_COUNT] = {
    {&TrainPlan::c_d1, &PropParams::Blk::c1w, &PropParams::Blk::c1b},
    {&TrainPlan::c_dd, &PropParams::Blk::c3w, &PropParams::Blk::c3b},
    {&TrainPlan::c_d1, &PropParams::Blk::c5w, &PropParams::Blk::c5b},
    {&TrainPlan::c_1, &PropParams::Blk::f1w, nullptr},
    {&TrainPlan::c_1, &PropParams::Blk::f3w, nullptr},
};

// workspace layout (floats): weight packs | tape[T] | backward scratch [| partial sums of the batch-parallel weight gradient]
struct TrainLayout {
    int nb = 0;
    size_t n = 0, nl = 0;                          // B*D*HW, B*c*HW
    size_t pk_in = 0, pk_inT = 0, pk_out = 0, pk_outT = 0;
    std::vector<size_t> pk_blk;                    // [block][BlkConv][forward | flipped]
    size_t pk(int i, int conv, bool flipped = false) const { return pk_blk[((size_t)i * BC_COUNT + conv) * 2 + (flipped ? 1 : 0)]; }
    size_t tape0 = 0, tape_step = 0, st_blk = 0;   // per step: x0 | blocks | nO | stats
    size_t scratch = 0, total = 0;
    size_t wg_part = 0, wg_floats = 0;             // option "train_wgrad" = 1: [S][Cout][Cin][k*k] of the plan's largest launch
    size_t vec0 = 0, vec_blk = 0, vec_glob = 0, vstat = 0;     // conditional: per-block vectors | fe, l0, l0g, ce, d_ce | GN stats
    // tape offsets inside a step
    size_t off_x0 = 0, off_blk = 0, blk_stride = 0, off_nO = 0, off_stats = 0;
};
enum { TB_N1 = 0, TB_U1, TB_A1, TB_U2, TB_A2, TB_X1, TB_N2, TB_V, TB_G, TB_X2, TB_NC, TB_XM, TB_COUNT };
// (conditional block: TB_U2 = h = conv1.3(a1) + emb, TB_NC = GN(h), TB_A2 = GELU(TB_NC), TB_XM = x1 (1 + m))
enum { TV_EMB = 0, TV_VG, TV_C1, TV_C1G, TV_M, TV_DEMB, TV_DM, TV_COUNT };     // per-block [B][D] vectors

void train_layout(const TrainPlan& p, int T, TrainLayout& L, int wgrad_form) {
    const size_t HW = (size_t)p.H * p.W;
    L.nb = p.nb; L.n = (size_t)p.B * p.D * HW; L.nl = (size_t)p.B * p.c * HW;
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t o = off; off += round64(floats); return o; };
    L.pk_in = take(p.in_proj.pack_floats()); L.pk_inT = take(p.in_proj_T.pack_floats());
    L.pk_out = take(p.out_proj.pack_floats()); L.pk_outT = take(p.out_proj_T.pack_floats());
    for (int i = 0; i < p.nb; ++i)
        for (const BlkConvRow& r : kBlkConv)
            for (int flipped = 0; flipped < 2; ++flipped) L.pk_blk.push_back(take((p.*r.geom).pack_floats()));
    // one step of tape
    size_t so = 0;
    auto stake = [&](size_t floats) { const size_t o = so; so += round64(floats); return o; };
    L.off_x0 = stake(L.n);
    L.off_blk = so; L.blk_stride = TB_COUNT * round64(L.n);
    so += (size_t)p.nb * L.blk_stride;
    L.off_nO = stake(L.n);
    L.off_stats = so;                                            // per block 3 x [B][1][2], then [B][32][2]
    L.st_blk = 3 * round64((size_t)p.B * 2);
    so += (size_t)p.nb * L.st_blk + round64((size_t)p.B * 32 * 2);
    L.tape_step = so;
    L.tape0 = off; off += (size_t)T * L.tape_step;
    L.scratch = off;
    off += 4 * round64(L.n) + 2 * round64(L.nl) + round64((size_t)p.B * p.D * 2);
    if (p.cond) {
        const size_t vd = round64((size_t)p.B * p.D), ve = round64((size_t)p.B * std::max(p.E, p.D));
        L.vec0 = off; L.vec_blk = TV_COUNT * vd; off += (size_t)p.nb * L.vec_blk;
        L.vec_glob = off; off += 8 * ve;                          // fe, l0, l0g, ce, d_ce, 3 scratch vectors
        L.vstat = off; off += (size_t)p.nb * round64((size_t)p.B * 2);
    }
    if (wgrad_form == 1) {                                           // appended: everything above keeps its offset
        for (const TConv* t : {&p.in_proj, &p.c_d1, &p.c_dd, &p.c_1, &p.out_proj})
            L.wg_floats = std::max(L.wg_floats, (size_t)t->wg_S * t->Cout * t->Cin * t->k * t->k);
        L.wg_part = take(L.wg_floats);
    }
    L.total = off;
}

// One step of tape by name (the layout's offsets are used here and nowhere else).  F = float: the forward, which writes the
// tape; const float: the backward and the tangent walk, which read it.
template <typename F>
struct TapeStepT {
    const TrainLayout& L; F* tp;
    TapeStepT(const TrainLayout& L_, F* W, int t) : L(L_), tp(W + L_.tape0 + (size_t)t * L_.tape_step) {}
    F* x0() const { return tp + L.off_x0; }                                                  // in_proj's output
    F* t(int i, int which) const { return tp + L.off_blk + (size_t)i * L.blk_stride + (size_t)which * (L.blk_stride / TB_COUNT); }
    F* block_in(int i) const { return i == 0 ? x0() : t(i - 1, TB_X2); }
    // (mean, rstd) of block i's GroupNorms -- slot 0: conv.0 / conv1.0, 1: ffn.0, 2: cond_conv1.0
    F* stats(int i, int slot) const { return tp + L.off_stats + (size_t)i * L.st_blk + (size_t)slot * (L.st_blk / 3); }
    F* nO() const { return tp + L.off_nO; }                                                  // out_proj's GroupNorm output
    F* stats_out() const { return stats(L.nb, 0); }
    F* last_x() const { return block_in(L.nb); }                                             // the last block's output
};
using TapeStep = TapeStepT<float>;
using ConstTapeStep = TapeStepT<const float>;

int run_tconv(lns_engine* e, const TConv& t, const float* x, const float* wpack, const float* bias, float* y, const float* res,
              hipStream_t s) {
    ConvArgs a = t.base;
    a.x = x; a.w = wpack; a.bias = bias; a.y = y; a.res = res;
    HIPCHK(e, launch_conv(t.variant, a, s));
    return LNS_OK;
}
// part: the layout's partial-sum area (batch-parallel form) or null (one block per output tile); x_bs: floats between two
// samples of x, which only the batch-parallel form takes other than Cin*H*W
int run_wgrad(lns_engine* e, const TConv& t, const TrainPlan& p, const float* dy, const float* x, long x_bs, float* dw, int accumulate,
              float* part, hipStream_t s) {
    WgradArgs a;
    memset(&a, 0, sizeof a);
    a.dy = dy; a.x = x; a.rowmap = t.d_full; a.colmap = t.d_full + t.full_rows; a.dw = dw;
    a.B = p.B; a.Cin = t.Cin; a.Cout = t.Cout; a.H = p.H; a.W = p.W; a.k = t.k; a.dil = t.dil; a.accumulate = accumulate;
    a.x_bs = x_bs; a.part = part; a.S = t.wg_S;
    if (part) HIPCHK(e, launch_conv_wgrad_split(a, s));
    else HIPCHK(e, launch_conv_wgrad(a, s));
    return LNS_OK;
}

int pack_all(lns_engine* e, const TrainPlan& p, const TrainLayout& L, const PropParams& pp, const float* const* P, float* ws, bool with_T,
             hipStream_t s) {
    // flipped: the pack of the transposed convolution, whose geometry object tT (Cin <-> Cout; a D -> D conv's own) gives the pads
    auto pack = [&](const TConv& t, const TConv& tT, int widx, size_t off, int flipped) -> hipError_t {
        const TConv& pads = flipped ? tT : t;
        return launch_pack_conv_w(P[widx], ws + off, t.Cout, t.Cin, t.k, pads.Cin_pad, pads.Cout_pad, flipped, s);
    };
    const int sides = with_T ? 2 : 1;                                         // the forward packs, then the flipped ones
    for (int flipped = 0; flipped < sides; ++flipped) {
        HIPCHK(e, pack(p.in_proj, p.in_proj_T, pp.in_w, flipped ? L.pk_inT : L.pk_in, flipped));
        HIPCHK(e, pack(p.out_proj, p.out_proj_T, pp.out_w, flipped ? L.pk_outT : L.pk_out, flipped));
    }
    for (int i = 0; i < p.nb; ++i)
        for (int flipped = 0; flipped < sides; ++flipped)
            for (int c = 0; c < BC_COUNT; ++c) {
                const TConv& t = p.*kBlkConv[c].geom;
                HIPCHK(e, pack(t, t, pp.blk[i].*kBlkConv[c].w, L.pk(i, c, flipped), flipped));
            }
    return LNS_OK;
}

int check_params(lns_engine* e, const PropParams& pp, const float* const* P, const char* what) {
    for (int v : pp.all)
        if (!P[v]) { e->err = fmt("training rollout: a propagator %s pointer is null (%s)", what, e->params[v].key.c_str()); return LNS_EINVAL; }
    return LNS_OK;
}

GnTrainArgs gn_args(const TrainPlan& p, int groups, float eps, const float* x, float* y, float* stats, const float* gamma, const float* beta) {
    GnTrainArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.y = y; a.stats = stats; a.gamma = gamma; a.beta = beta;
    a.B = p.B; a.C = p.D; a.HW = p.H * p.W; a.groups = groups; a.eps = eps;
    return a;
}

// The tail of a size query: the plan itself (device maps) is built now when a device is there -- the caller's current one, as
// torch sets it (no tensor in such a call) -- so that the first run call does not; the size does not need one.
int prebuild_train_plan(lns_engine* e, int B, int H, int W) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return LNS_OK; }
    TrainPlan* p;
    return get_train_plan(e, device, B, H, W, &p);
}

}  // namespace

void lns_train_release(const lns_engine* e) {
    std::lock_guard<std::mutex> lock(g_train_mutex);
    g_prop_params.erase(e);
    for (auto it = g_train_plans.begin(); it != g_train_plans.end();) {
        if (it->first.e == e) {
            DeviceGuard dg(it->first.device);
            it->second.release();
            it = g_train_plans.erase(it);
        } else ++it;
    }
}

int lns_train_workspace_bytes(lns_engine* e, int B, int H, int W, int T, size_t* bytes) {
    if (!e || B <= 0 || T <= 0 || !bytes) return LNS_EINVAL;
    if (int brc = check_batch(e, B)) return brc;
    TrainPlan dims; int rc;
    if ((rc = train_plan_dims(e, B, H, W, dims))) return rc;
    TrainLayout L;
    train_layout(dims, T, L, e->opt_train_wgrad);
    *bytes = L.total * 4;
    return prebuild_train_plan(e, B, H, W);
}

// the per-sample vector network of the conditional propagator (step-invariant): ce, and per block emb and m
struct VecView {
    float *fe, *l0, *l0g, *ce, *dce, *t1, *t2, *t3;
    float *blk0, *vstat0; size_t vd, vs;           // per-block vectors and GroupNorm statistics: base and slot size
    float* blk(int i, int which) const { return blk0 + ((size_t)i * TV_COUNT + which) * vd; }       // which: TV_*
    float* vstat(int i) const { return vstat0 + (size_t)i * vs; }
};
VecView vec_view(const TrainPlan& p, const TrainLayout& L, float* W) {
    const size_t ve = round64((size_t)p.B * std::max(p.E, p.D));
    float* g = W + L.vec_glob;
    return VecView{g, g + ve, g + 2 * ve, g + 3 * ve, g + 4 * ve, g + 5 * ve, g + 6 * ve, g + 7 * ve,
                   W + L.vec0, W + L.vstat, L.vec_blk / TV_COUNT, round64((size_t)p.B * 2)};
}
int cond_vectors_forward(lns_engine* e, const TrainPlan& p, const TrainLayout& L, const PropParams& pp, const float* const* P,
                         const float* param, float* W, hipStream_t s) {
    const VecView v = vec_view(p, L, W);
    const int B = p.B, E = p.E, D = p.D;
    HIPCHK(e, launch_vec_fourier(param, v.fe, B, E, s));
    HIPCHK(e, launch_vec_linear_fwd(v.fe, P[pp.m0w], P[pp.m0b], v.l0, B, E, E, s));
    HIPCHK(e, launch_vec_gelu(v.l0, nullptr, v.l0g, B * E, s));
    HIPCHK(e, launch_vec_linear_fwd(v.l0g, P[pp.m2w], P[pp.m2b], v.ce, B, E, E, s));
    for (int i = 0; i < p.nb; ++i) {
        const PropParams::Blk& b = pp.blk[i];
        float* emb = v.blk(i, TV_EMB);
        HIPCHK(e, launch_vec_linear_fwd(v.ce, P[b.ce_w], P[b.ce_b], emb, B, E, D, s));
        HIPCHK(e, launch_vec_gn(emb, P[b.vg], P[b.vb], v.blk(i, TV_VG), v.vstat(i), nullptr, nullptr, nullptr, nullptr, 0, B, D, 1e-5f, s));
        HIPCHK(e, launch_vec_linear_fwd(v.blk(i, TV_VG), P[b.v1w], P[b.v1b], v.blk(i, TV_C1), B, D, D, s));
        HIPCHK(e, launch_vec_gelu(v.blk(i, TV_C1), nullptr, v.blk(i, TV_C1G), B * D, s));
        HIPCHK(e, launch_vec_linear_fwd(v.blk(i, TV_C1G), P[b.v3w], P[b.v3b], v.blk(i, TV_M), B, D, D, s));
    }
    return LNS_OK;
}

int lns_train_forward(lns_engine* e, const float* const* params, const float* z_in, const float* param, int B, int H, int Wd, int T,
                      float* z_pred, void* ws, size_t ws_bytes, void* stream) {
    if (!e || !params || !z_in || !z_pred || B <= 0 || T <= 0) return LNS_EINVAL;
    if (int brc = check_batch(e, B)) return brc;
    int device = -1, rc;
    if ((rc = train_device_of(e, z_in, &device)) || (rc = train_same_device(e, device, z_pred, "z_pred")) ||
        (rc = train_same_device(e, device, ws, "the workspace")) || (rc = train_same_device(e, device, param, "param"))) return rc;
    DeviceGuard dg(device);
    HIPCHK(e, init_kernels());
    TrainPlan* pl;
    if ((rc = get_train_plan(e, device, B, H, Wd, &pl))) return rc;
    const TrainPlan& p = *pl;
    if (p.cond && !param) { e->err = "conditional propagator needs param"; return LNS_EINVAL; }
    TrainLayout L;
    train_layout(p, T, L, e->opt_train_wgrad);
    if (!ws || ws_bytes < L.total * 4) { e->err = fmt("training workspace too small: need %zu bytes", L.total * 4); return LNS_ENOMEM; }
    const PropParams* ppp;
    if ((rc = prop_params(e, &ppp)) || (rc = check_params(e, *ppp, params, "parameter"))) return rc;
    const PropParams& pp = *ppp;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* W = static_cast<float*>(ws);
    if ((rc = pack_all(e, p, L, pp, params, W, false, s))) return rc;
    if (p.cond && (rc = cond_vectors_forward(e, p, L, pp, params, param, W, s))) return rc;
    const VecView vv = p.cond ? vec_view(p, L, W) : VecView{};
    const long n = (long)L.n;
    const size_t HW = (size_t)p.H * p.W;
    const int BD = p.B * p.D;
    for (int t = 0; t < T; ++t) {
        const TapeStep tape(L, W, t);
        const float* zin = t == 0 ? z_in : z_pred + (size_t)(t - 1) * p.c * HW;
        // z_pred is [B][T][c][h][w]: step t reads / writes through a batch stride of T*c*HW
        ConvArgs ain = p.in_proj.base;
        ain.x = zin; ain.x_bs = t == 0 ? (long)p.c * HW : (long)T * p.c * HW;
        ain.w = W + L.pk_in; ain.bias = params[pp.in_b]; ain.y = tape.x0();
        HIPCHK(e, launch_conv(p.in_proj.variant, ain, s));
        for (int i = 0; i < p.nb; ++i) {
            const PropParams::Blk& b = pp.blk[i];
            const float* x = tape.block_in(i);
            HIPCHK(e, launch_gn_train_fwd(gn_args(p, 1, 1e-5f, x, tape.t(i, TB_N1), tape.stats(i, 0), params[b.g1], params[b.b1]), s));
            if ((rc = run_tconv(e, p.c_d1, tape.t(i, TB_N1), W + L.pk(i, BC_C1), params[b.c1b], tape.t(i, TB_U1), nullptr, s))) return rc;
            HIPCHK(e, launch_gelu_fwd(tape.t(i, TB_U1), tape.t(i, TB_A1), n, s));
            const float* ffn_in;
            if (!p.cond) {
                if ((rc = run_tconv(e, p.c_dd, tape.t(i, TB_A1), W + L.pk(i, BC_C3), params[b.c3b], tape.t(i, TB_U2), nullptr, s))) return rc;
                HIPCHK(e, launch_gelu_fwd(tape.t(i, TB_U2), tape.t(i, TB_A2), n, s));
                if ((rc = run_tconv(e, p.c_d1, tape.t(i, TB_A2), W + L.pk(i, BC_C5), params[b.c5b], tape.t(i, TB_X1), x, s))) return rc;
                ffn_in = tape.t(i, TB_X1);
            } else {
                // h = conv1.3(a1) + emb (per-sample broadcast add in the conv epilogue) ; x1 = x + cond_conv1.2(GELU(GN(h)))
                ConvArgs ah = p.c_dd.base;
                ah.x = tape.t(i, TB_A1); ah.w = W + L.pk(i, BC_C3); ah.bias = params[b.c3b]; ah.y = tape.t(i, TB_U2);
                ah.badd = vv.blk(i, TV_EMB);
                HIPCHK(e, launch_conv(p.c_dd.variant, ah, s));
                HIPCHK(e, launch_gn_train_fwd(gn_args(p, 1, 1e-5f, tape.t(i, TB_U2), tape.t(i, TB_NC), tape.stats(i, 2), params[b.cg], params[b.cb]), s));
                HIPCHK(e, launch_gelu_fwd(tape.t(i, TB_NC), tape.t(i, TB_A2), n, s));
                if ((rc = run_tconv(e, p.c_d1, tape.t(i, TB_A2), W + L.pk(i, BC_C5), params[b.c5b], tape.t(i, TB_X1), x, s))) return rc;
                HIPCHK(e, launch_chan_scale(tape.t(i, TB_X1), vv.blk(i, TV_M), nullptr, tape.t(i, TB_XM), BD, (int)HW, s));
                ffn_in = tape.t(i, TB_XM);
            }
            HIPCHK(e, launch_gn_train_fwd(gn_args(p, 1, 1e-5f, ffn_in, tape.t(i, TB_N2), tape.stats(i, 1), params[b.g2], params[b.b2]), s));
            if ((rc = run_tconv(e, p.c_1, tape.t(i, TB_N2), W + L.pk(i, BC_F1), nullptr, tape.t(i, TB_V), nullptr, s))) return rc;
            HIPCHK(e, launch_gelu_fwd(tape.t(i, TB_V), tape.t(i, TB_G), n, s));
            if ((rc = run_tconv(e, p.c_1, tape.t(i, TB_G), W + L.pk(i, BC_F3), nullptr, tape.t(i, TB_X2), tape.t(i, TB_X1), s))) return rc;
        }
        HIPCHK(e, launch_gn_train_fwd(gn_args(p, 32, 1e-6f, tape.last_x(), tape.nO(), tape.stats_out(), params[pp.out_g], params[pp.out_be]), s));
        ConvArgs ao = p.out_proj.base;
        ao.x = tape.nO(); ao.w = W + L.pk_out; ao.bias = params[pp.out_b];
        ao.y = z_pred + (size_t)t * p.c * HW; ao.y_bs = (long)T * p.c * HW;
        HIPCHK(e, launch_conv(p.out_proj.variant, ao, s));
    }
    return LNS_OK;
}

// grads == null: the state-only adjoint -- every launch below that only produces a parameter gradient is left out (so),
// the data path is the same kernels in the same order.  grad_param: d loss / d param of the conditional propagator.
int lns_train_backward_ex(lns_engine* e, const float* const* params, const float* z_in, const float* z_pred, const float* grad_z_pred,
                          int B, int H, int Wd, int T, float* const* grads, float* grad_z_in, void* ws, size_t ws_bytes, void* stream,
                          float* grad_param) {
    if (!e || !params || !z_in || !z_pred || !grad_z_pred || B <= 0 || T <= 0) return LNS_EINVAL;
    if (int brc = check_batch(e, B)) return brc;
    if (grad_param && e->cfg.prop_kind != LNS_PROP_CONDITIONAL) { e->err = "training rollout: grad_param needs the conditional propagator"; return LNS_EINVAL; }
    const bool so = grads == nullptr;
    int device = -1, rc;
    if ((rc = train_device_of(e, z_in, &device)) || (rc = train_same_device(e, device, z_pred, "z_pred")) ||
        (rc = train_same_device(e, device, grad_z_pred, "grad_z_pred")) || (rc = train_same_device(e, device, ws, "the workspace")) ||
        (rc = train_same_device(e, device, grad_z_in, "grad_z_in")) || (rc = train_same_device(e, device, grad_param, "grad_param"))) return rc;
    DeviceGuard dg(device);
    TrainPlan* pl;
    if ((rc = get_train_plan(e, device, B, H, Wd, &pl))) return rc;
    const TrainPlan& p = *pl;
    TrainLayout L;
    // the partial-sum area of the batch-parallel weight gradient is appended to the layout: without weight gradients a
    // workspace sized under either "train_wgrad" value covers what is used
    const int wgrad_form = so ? 0 : e->opt_train_wgrad;
    train_layout(p, T, L, wgrad_form);
    if (!ws || ws_bytes < L.total * 4) { e->err = fmt("training workspace too small: need %zu bytes", L.total * 4); return LNS_ENOMEM; }
    const PropParams* ppp;
    if ((rc = prop_params(e, &ppp)) || (rc = check_params(e, *ppp, params, "parameter")) ||
        (!so && (rc = check_params(e, *ppp, const_cast<const float* const*>(grads), "gradient")))) return rc;
    const PropParams& pp = *ppp;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* W = static_cast<float*>(ws);
    if ((rc = pack_all(e, p, L, pp, params, W, true, s))) return rc;
    const VecView vv = p.cond ? vec_view(p, L, W) : VecView{};
    const long n = (long)L.n;
    const size_t HW = (size_t)p.H * p.W, np = round64(L.n), nlp = round64(L.nl);
    float* dA = W + L.scratch; float* dB = dA + np; float* dC = dB + np; float* dD = dC + np;
    float* dz = dD + np;                 // [B][c][HW] gradient w.r.t. the step's output (contiguous)
    float* dz2 = dz + nlp;
    float* part = dz2 + nlp;             // [B][D][2]
    float* wgp = wgrad_form == 1 ? W + L.wg_part : nullptr;      // batch-parallel weight gradient: its partial sums
    const long nbs = (long)p.D * HW;     // sample stride of the D-channel tensors
    const int Bn = p.B, BD = p.B * p.D;
    int acc = 0;                         // parameter gradients: written at the first processed step, accumulated after
    // The walk's two idioms, each holding the state-only condition once.  conv_bwd: d bias (bidx >= 0), d weight from (dy, the
    // convolution's input x), then d input = the transposed convolution tT on the flipped pack at packT, into dxo.
    auto conv_bwd = [&](const TConv& t, const TConv& tT, int bidx, int widx, const float* dy, const float* x, long x_bs, size_t packT,
                        float* dxo) -> int {
        if (!so) {
            if (bidx >= 0) HIPCHK(e, launch_bias_grad(dy, Bn, t.Cout, (int)HW, grads[bidx], acc, s));
            if (int wrc = run_wgrad(e, t, p, dy, x, x_bs, grads[widx], acc, wgp, s)) return wrc;
        }
        return run_tconv(e, tT, dy, W + packT, nullptr, dxo, nullptr, s);
    };
    auto blk_conv_bwd = [&](int i, BlkConv k, const float* dy, const float* x, float* dxo) -> int {
        const BlkConvRow& r = kBlkConv[k];
        const PropParams::Blk& b = pp.blk[i];
        return conv_bwd(p.*r.geom, p.*r.geom, r.b ? b.*r.b : -1, b.*r.w, dy, x, nbs, L.pk(i, k, true), dxo);
    };
    // gn_bwd: dxo = add + GroupNorm backward of dy (x, stats: the forward's input and statistics), then d gamma / d beta
    auto gn_bwd = [&](int groups, float eps, const float* x, const float* stats, int gidx, int bidx, const float* dy, const float* add,
                      float* dxo) -> int {
        GnTrainArgs g = gn_args(p, groups, eps, x, nullptr, const_cast<float*>(stats), params[gidx], params[bidx]);      // (read only)
        g.dy = dy; g.dx = dxo; g.add = add; g.part = part;
        HIPCHK(e, launch_gn_train_bwd(g, s));
        if (!so) HIPCHK(e, launch_colsum2(part, Bn, p.D, grads[gidx], grads[bidx], acc, s));
        return LNS_OK;
    };
    for (int t = T - 1; t >= 0; --t) {
        acc = t == T - 1 ? 0 : 1;
        const ConstTapeStep tape(L, W, t);
        // gradient w.r.t. z_pred[:, t] = caller's + what flowed back from step t+1 (in dz2), made contiguous in dz
        // (rows of the [B][T][c][HW] tensors are T*c*HW apart)
        HIPCHK(e, launch_add_rows(grad_z_pred + (size_t)t * p.c * HW, (long)T * p.c * HW, t == T - 1 ? nullptr : dz2, (long)p.c * HW, dz,
                                  (long)p.c * HW, Bn, (long)(p.c * HW), s));
        // ---- out_proj: z = conv1(nO) + b ; nO = GN32(xL)
        if ((rc = conv_bwd(p.out_proj, p.out_proj_T, pp.out_b, pp.out_w, dz, tape.nO(), nbs, L.pk_outT, dA))) return rc;      // d nO
        if ((rc = gn_bwd(32, 1e-6f, tape.last_x(), tape.stats_out(), pp.out_g, pp.out_be, dA, nullptr, dB))) return rc;
        float* dx = dB;                    // gradient w.r.t. the current block's output x2
        float* f1 = dA; float* f2 = dC; float* f3 = dD;     // free scratch tensors
        for (int i = p.nb - 1; i >= 0; --i) {
            const PropParams::Blk& b = pp.blk[i];
            // x2 = x1 + ffn.3(g): d w(f3), d g
            if ((rc = blk_conv_bwd(i, BC_F3, dx, tape.t(i, TB_G), f1))) return rc;                               // d g
            HIPCHK(e, launch_gelu_bwd(f1, tape.t(i, TB_V), f2, n, s));                                           // d v
            if ((rc = blk_conv_bwd(i, BC_F1, f2, tape.t(i, TB_N2), f1))) return rc;                              // d n2
            float* dx1;                                                                                          // gradient w.r.t. x1
            if (!p.cond) {
                if ((rc = gn_bwd(1, 1e-5f, tape.t(i, TB_X1), tape.stats(i, 1), b.g2, b.b2, f1, dx, f3))) return rc;     // d x1 = d x2 + GN path
                dx1 = f3;
            } else {
                // ffn input was xm = x1 (1 + m): d xm through the GroupNorm, then d m += <d xm, x1>, d x1 = d x2 + d xm (1 + m)
                if ((rc = gn_bwd(1, 1e-5f, tape.t(i, TB_XM), tape.stats(i, 1), b.g2, b.b2, f1, nullptr, f3))) return rc;
                HIPCHK(e, launch_chan_dot(f3, tape.t(i, TB_X1), vv.blk(i, TV_DM), BD, (int)HW, acc, s));
                HIPCHK(e, launch_chan_scale(f3, vv.blk(i, TV_M), dx, f1, BD, (int)HW, s));
                dx1 = f1;
            }
            float* g1 = dx1 == f3 ? f1 : f3;           // two scratch tensors besides dx1 (dx is free from here on)
            float* g2 = f2;
            // x1 = x + conv.5 / cond_conv1.2 (a2)
            if ((rc = blk_conv_bwd(i, BC_C5, dx1, tape.t(i, TB_A2), g1))) return rc;                             // d a2
            if (!p.cond) {
                HIPCHK(e, launch_gelu_bwd(g1, tape.t(i, TB_U2), g2, n, s));                                      // d u2
            } else {
                HIPCHK(e, launch_gelu_bwd(g1, tape.t(i, TB_NC), g2, n, s));                                      // d GN(h)
                if ((rc = gn_bwd(1, 1e-5f, tape.t(i, TB_U2), tape.stats(i, 2), b.cg, b.cb, g2, nullptr, g1))) return rc;     // d h
                HIPCHK(e, launch_chan_dot(g1, nullptr, vv.blk(i, TV_DEMB), BD, (int)HW, acc, s));                // h = .. + emb
                std::swap(g1, g2);                                                                               // d h is in g2 now
            }
            if ((rc = blk_conv_bwd(i, BC_C3, g2, tape.t(i, TB_A1), g1))) return rc;                              // d a1
            HIPCHK(e, launch_gelu_bwd(g1, tape.t(i, TB_U1), g2, n, s));                                          // d u1
            if ((rc = blk_conv_bwd(i, BC_C1, g2, tape.t(i, TB_N1), g1))) return rc;                              // d n1
            if ((rc = gn_bwd(1, 1e-5f, tape.block_in(i), tape.stats(i, 0), b.g1, b.b1, g1, dx1, dx))) return rc;     // d x = d x1 + GN path
        }
        // ---- in_proj: x0 = conv1(z_in) + b
        const float* zin = t == 0 ? z_in : z_pred + (size_t)(t - 1) * p.c * HW;
        // the weight-gradient kernel reads x with a plain [B][Cin][HW] layout: step t > 0 reads z_pred through its T-strided batch
        // axis, so it is copied to a contiguous buffer first (small: B x c x HW; the batch-parallel form takes a batch stride and
        // reads z_pred in place).  The copy's launch follows the bias gradient's, which is therefore issued here and not by conv_bwd.
        if (!so) HIPCHK(e, launch_bias_grad(dx, Bn, p.D, (int)HW, grads[pp.in_b], acc, s));
        const float* zc = zin;
        long zbs = t == 0 ? (long)p.c * HW : (long)T * p.c * HW;
        if (t > 0 && !wgp && !so) {                          // (state-only: nothing reads the copy)
            HIPCHK(e, launch_add_rows(zin, (long)T * p.c * HW, nullptr, 0, dz, (long)p.c * HW, Bn, (long)(p.c * HW), s));
            zc = dz; zbs = (long)p.c * HW;
        }
        float* dzin = t == 0 ? (grad_z_in ? grad_z_in : dz2) : dz2;
        if ((rc = conv_bwd(p.in_proj, p.in_proj_T, -1, pp.in_w, dx, zc, zbs, L.pk_inT, dzin))) return rc;           // d z_{t-1}
    }
    if (p.cond && (!so || grad_param)) {
        // the vector network, once: accumulated d m / d emb of every block -> cond_conv2, cond_emb, cond_emb_proj.
        // G(i): the parameter-gradient output of a vector kernel, null in the state-only adjoint (the kernel then leaves
        // that output out: nothing is written, there is no sink buffer)
        auto G = [&](int i) -> float* { return so ? nullptr : grads[i]; };
        const int E = p.E, D = p.D;
        for (int i = 0; i < p.nb; ++i) {
            const PropParams::Blk& b = pp.blk[i];
            float* dm = vv.blk(i, TV_DM);
            float* demb = vv.blk(i, TV_DEMB);
            // m = W3 c1g + b3 ; c1g = GELU(c1) ; c1 = W1 vg + b1 ; vg = GN(emb)
            HIPCHK(e, launch_vec_linear_bwd(dm, vv.blk(i, TV_C1G), params[b.v3w], vv.t1, 0, G(b.v3w), G(b.v3b), 0, Bn, D, D, s));
            HIPCHK(e, launch_vec_gelu(vv.blk(i, TV_C1), vv.t1, vv.t2, Bn * D, s));
            HIPCHK(e, launch_vec_linear_bwd(vv.t2, vv.blk(i, TV_VG), params[b.v1w], vv.t1, 0, G(b.v1w), G(b.v1b), 0, Bn, D, D, s));
            HIPCHK(e, launch_vec_gn(vv.blk(i, TV_EMB), params[b.vg], params[b.vb], nullptr, nullptr, vv.t1, vv.t2, G(b.vg), G(b.vb), 0, Bn, D, 1e-5f, s));
            HIPCHK(e, launch_add(vv.t2, demb, vv.t3, (long)Bn * D, s));                                          // d emb, both paths
            // emb = Wce ce + bce : d ce accumulates over the blocks
            HIPCHK(e, launch_vec_linear_bwd(vv.t3, vv.ce, params[b.ce_w], vv.dce, i > 0 ? 1 : 0, G(b.ce_w), G(b.ce_b), 0, Bn, E, D, s));
        }
        // ce = W2 GELU(l0) + b2 ; l0 = W0 fe + b0
        HIPCHK(e, launch_vec_linear_bwd(vv.dce, vv.l0g, params[pp.m2w], vv.t1, 0, G(pp.m2w), G(pp.m2b), 0, Bn, E, E, s));
        HIPCHK(e, launch_vec_gelu(vv.l0, vv.t1, vv.t2, Bn * E, s));
        // l0 = W0 fe + b0: d fe only when d param is asked for, into vv.t1 (free: vec_gelu above was its last reader)
        HIPCHK(e, launch_vec_linear_bwd(vv.t2, vv.fe, params[pp.m0w], grad_param ? vv.t1 : nullptr, 0, G(pp.m0w), G(pp.m0b), 0, Bn, E, E, s));
        // fe = [cos(param f_k) | sin(param f_k)]: the forward's fe is the derivative's sin / cos
        if (grad_param) HIPCHK(e, launch_vec_fourier_bwd(vv.fe, vv.t1, grad_param, Bn, E, s));
    }
    return LNS_OK;
}

int lns_train_backward(lns_engine* e, const float* const* params, const float* z_in, const float* z_pred, const float* grad_z_pred,
                       int B, int H, int Wd, int T, float* const* grads, float* grad_z_in, void* ws, size_t ws_bytes, void* stream) {
    if (e && !grads) return LNS_EINVAL;              // the state-only adjoint is lns_train_backward_ex's
    return lns_train_backward_ex(e, params, z_in, z_pred, grad_z_pred, B, H, Wd, T, grads, grad_z_in, ws, ws_bytes, stream, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------------
// The device-resident training step (include/lns.h): loss + gradient, multi-tensor Adam, and the whole step.
// Reference: train_stage2_ns2d.py:210-216.  Every argument check below is host-only and precedes the first HIP call.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

// lns_adam_spec -> the kernel's scalars; the bias corrections in double from the host-side step count
int adam_scalars(const lns_adam_spec* sp, AdamScalars& sc, std::string& err) {
    if (!sp || sp->size != sizeof(lns_adam_spec)) { err = "adam spec is null or its size field is not sizeof(lns_adam_spec)"; return LNS_EINVAL; }
    if (!(sp->lr >= 0.0) || !std::isfinite(sp->lr)) { err = "adam spec: lr must be >= 0"; return LNS_EINVAL; }
    if (!(sp->beta1 >= 0.0 && sp->beta1 < 1.0)) { err = "adam spec: beta1 must be in [0, 1)"; return LNS_EINVAL; }
    if (!(sp->beta2 >= 0.0 && sp->beta2 < 1.0)) { err = "adam spec: beta2 must be in [0, 1)"; return LNS_EINVAL; }
    if (!(sp->eps > 0.0) || !std::isfinite(sp->eps) || (float)sp->eps <= 0.0f) { err = "adam spec: eps must be > 0"; return LNS_EINVAL; }
    if (!(sp->weight_decay >= 0.0) || !std::isfinite(sp->weight_decay)) { err = "adam spec: weight_decay must be >= 0"; return LNS_EINVAL; }
    if (sp->step < 1) { err = "adam spec: step is the 1-based count of this update (>= 1)"; return LNS_EINVAL; }
    const double b1 = sp->beta1, b2 = sp->beta2, t = (double)sp->step;
    const double bc1 = 1.0 - std::pow(b1, t), bc2 = 1.0 - std::pow(b2, t);
    sc.step_size = (float)(sp->lr / bc1);
    sc.beta1 = (float)b1; sc.one_minus_beta1 = (float)(1.0 - b1);      // each rounded once from the caller's double
    sc.beta2 = (float)b2; sc.one_minus_beta2 = (float)(1.0 - b2);
    sc.bc2_sqrt = (float)std::sqrt(bc2);
    sc.eps = (float)sp->eps; sc.weight_decay = (float)sp->weight_decay;
    return LNS_OK;
}

// max_norm as the norm kernel takes it: 0 = no clipping.  A positive double below fp32's smallest denormal stays positive
// (it clips to ~0, as torch would) instead of rounding to "no clipping"; beyond fp32's range it is inf, which clips nothing.
float clip_threshold(double max_norm) {
    if (!(max_norm > 0.0)) return 0.0f;
    const float f = (float)max_norm;
    return f > 0.0f ? f : 1.401298464e-45f;                  // FLT_TRUE_MIN
}

// lns_update_spec -> the scalars of the clipped / decoupled update; what lns_adam_spec shares is checked by adam_scalars
struct UpdatePlan { AdamScalars sc; int decoupled = 0; float decay = 1.0f; float max_norm = 0.0f; int skip = 0; };
int update_scalars(const lns_update_spec* sp, UpdatePlan& u, std::string& err) {
    if (!sp || sp->size != sizeof(lns_update_spec)) { err = "update spec is null or its size field is not sizeof(lns_update_spec)"; return LNS_EINVAL; }
    if (sp->flags & ~(LNS_UPDATE_DECOUPLED_WD | LNS_UPDATE_SKIP_NONFINITE)) { err = fmt("update spec: unknown flags 0x%x", sp->flags); return LNS_EINVAL; }
    if (std::isnan(sp->max_norm)) { err = "update spec: max_norm is NaN (<= 0 means: no clipping)"; return LNS_EINVAL; }
    lns_adam_spec as;
    as.size = sizeof(lns_adam_spec); as.reserved = 0;
    as.lr = sp->lr; as.beta1 = sp->beta1; as.beta2 = sp->beta2; as.eps = sp->eps; as.weight_decay = sp->weight_decay; as.step = sp->step;
    if (int rc = adam_scalars(&as, u.sc, err)) return rc;
    u.decoupled = (sp->flags & LNS_UPDATE_DECOUPLED_WD) ? 1 : 0;
    u.skip = (sp->flags & LNS_UPDATE_SKIP_NONFINITE) ? 1 : 0;
    if (u.decoupled) {                                                // torch.optim.AdamW: param.mul_(1 - lr * weight_decay)
        u.decay = (float)(1.0 - sp->lr * sp->weight_decay);
        u.sc.weight_decay = 0.0f;
    }
    u.max_norm = clip_threshold(sp->max_norm);
    return LNS_OK;
}

static_assert(LNS_NORM_CHUNK == 2048, "include/lns.h names the chunk of grad_sumsq_multi_kernel (lns_optim.inc: ADAM_CHUNK)");
// n gradient tensors -> the norm kernel's table (null gradients left out) and the scratch the whole list needs
int norm_tensors(int n, const float* const* grads, const int64_t* numel, std::vector<NormTensor>* tt, size_t& bytes, std::string& err) {
    if (n < 0 || (n > 0 && !numel)) { err = "grad norm: numel is null"; return LNS_EINVAL; }
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 1 || numel[i] >= (int64_t)1 << 31) { err = fmt("grad norm: tensor %d has %lld elements (1 .. 2^31 - 1)", i, (long long)numel[i]); return LNS_EINVAL; }
        chunks += (numel[i] + LNS_NORM_CHUNK - 1) / LNS_NORM_CHUNK;
        if (tt && grads[i]) tt->push_back(NormTensor{grads[i], (unsigned)numel[i], 0u});
    }
    if (chunks >= (int64_t)1 << 31) { err = "grad norm: more than 2^31 - 1 chunks in one call"; return LNS_EINVAL; }
    bytes = round256((size_t)chunks * 8);
    return LNS_OK;
}

static_assert(LNS_SL1_CHUNK == SL1_CHUNK, "include/lns.h and lns_train_kernels.h name the same chunk");
constexpr int64_t SL1_MAX_N = (int64_t)SL1_CHUNK << 30;       // 2^30 blocks: grid and partial count stay 32-bit
int loss_check(int64_t n, float beta, const void* loss_out, std::string& err) {
    if (n < 1 || n > SL1_MAX_N) { err = fmt("smooth_l1: n must be in 1 .. %lld", (long long)SL1_MAX_N); return LNS_EINVAL; }
    if (!(beta > 0.0f) || !std::isfinite(beta)) { err = "smooth_l1: beta must be > 0 (beta = 0 is the L1 loss, which this kernel does not compute)"; return LNS_EINVAL; }
    if (!loss_out) { err = "smooth_l1: loss_out is null"; return LNS_EINVAL; }
    return LNS_OK;
}

// workspace of the whole step (bytes): training workspace | z_pred | dL/dz_pred | loss partials
struct StepLayout { size_t train = 0, z_pred = 0, dz = 0, part = 0, total = 0, n = 0; };
int step_layout(lns_engine* e, int B, int H, int W, int T, StepLayout& S) {
    TrainPlan dims; int rc;
    if ((rc = train_plan_dims(e, B, H, W, dims))) return rc;
    TrainLayout L;
    train_layout(dims, T, L, e->opt_train_wgrad);
    S.n = (size_t)B * T * dims.c * H * W;
    S.train = L.total * 4;
    S.z_pred = round256(S.train);
    S.dz = S.z_pred + round256(S.n * 4);
    S.part = S.dz + round256(S.n * 4);
    S.total = S.part + round256((size_t)smooth_l1_partials((long)S.n) * 4);
    return LNS_OK;
}

// tail of the clipped step's workspace (bytes from its start): norm partials | coefficient | norm | counter of skipped steps
struct ClipLayout { size_t part = 0, coef = 0, norm = 0, counter = 0, total = 0; };
void clip_layout(const lns_engine* e, const PropParams& pp, const StepLayout& S, ClipLayout& C) {
    size_t chunks = 0;
    for (int v : pp.all) chunks += (e->params[v].numel() + LNS_NORM_CHUNK - 1) / LNS_NORM_CHUNK;
    C.part = S.total;
    C.coef = C.part + round256(chunks * 8);
    C.norm = C.coef + 256;
    C.counter = C.norm + 256;
    C.total = C.counter + 256;
}

}  // namespace

int lns_loss_smooth_l1(const float* pred, const float* target, int64_t n, float beta, float* loss_out, float* grad_out,
                       float* scratch, size_t scratch_floats, void* stream) {
    std::string& err = g_create_error;
    if (!pred || !target) { err = "smooth_l1: pred / target is null"; return LNS_EINVAL; }
    if (int rc = loss_check(n, beta, loss_out, err)) return rc;
    if (!scratch || scratch_floats < (size_t)smooth_l1_partials((long)n)) {
        err = fmt("smooth_l1: scratch must hold %ld floats", smooth_l1_partials((long)n));
        return LNS_ENOMEM;
    }
    const hipError_t rc = launch_smooth_l1(pred, target, (long)n, beta, loss_out, grad_out, scratch, static_cast<hipStream_t>(stream));
    if (rc != hipSuccess) { err = std::string("smooth_l1: ") + hipGetErrorString(rc); return LNS_EHIP; }
    return LNS_OK;
}

int lns_adam_step_tensors(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, const int64_t* numel, const lns_adam_spec* spec, void* stream) {
    std::string& err = g_create_error;
    if (n < 0 || (n > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numel))) { err = "adam: null pointer array"; return LNS_EINVAL; }
    AdamScalars sc;
    if (int rc = adam_scalars(spec, sc, err)) return rc;
    std::vector<AdamTensor> tt;
    tt.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]) continue;
        if (numel[i] < 1 || numel[i] >= (int64_t)1 << 31) { err = fmt("adam: tensor %d has %lld elements (1 .. 2^31 - 1)", i, (long long)numel[i]); return LNS_EINVAL; }
        tt.push_back(AdamTensor{params[i], grads[i], exp_avg[i], exp_avg_sq[i], (unsigned)numel[i], 0u});
    }
    if (tt.empty()) return LNS_OK;
    const hipError_t rc = launch_adam_multi(tt.data(), (int)tt.size(), sc, static_cast<hipStream_t>(stream));
    if (rc != hipSuccess) { err = std::string("adam: ") + hipGetErrorString(rc); return LNS_EHIP; }
    return LNS_OK;
}

// the engine's tensors: lengths from the parameter table
static int adam_engine(lns_engine* e, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       const AdamScalars& sc, hipStream_t s) {
    std::vector<AdamTensor> tt;
    tt.reserve(e->params.size());
    for (size_t i = 0; i < e->params.size(); ++i) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]) continue;
        const size_t n = e->params[i].numel();
        if (n < 1 || n >= (size_t)1 << 31) continue;
        tt.push_back(AdamTensor{params[i], grads[i], exp_avg[i], exp_avg_sq[i], (unsigned)n, 0u});
    }
    if (tt.empty()) return LNS_OK;
    HIPCHK(e, launch_adam_multi(tt.data(), (int)tt.size(), sc, s));
    return LNS_OK;
}

int lns_adam_step(lns_engine* e, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const lns_adam_spec* spec, void* stream) {
    if (!e) return LNS_EINVAL;
    if (!params || !grads || !exp_avg || !exp_avg_sq) { e->err = "adam: null pointer array"; return LNS_EINVAL; }
    AdamScalars sc;
    if (int rc = adam_scalars(spec, sc, e->err)) return rc;
    return adam_engine(e, params, grads, exp_avg, exp_avg_sq, sc, static_cast<hipStream_t>(stream));
}

int lns_train_step_workspace_bytes(lns_engine* e, int B, int H, int W, int T, size_t* bytes) {
    if (!e) return LNS_EINVAL;
    if (B < 1) { e->err = "training step: B must be >= 1"; return LNS_EINVAL; }
    if (T < 1) { e->err = "training step: T must be >= 1"; return LNS_EINVAL; }
    if (!bytes) { e->err = "training step: bytes is null"; return LNS_EINVAL; }
    if (e->cfg.prop_kind != LNS_PROP_PLAIN && e->cfg.prop_kind != LNS_PROP_CONDITIONAL) { e->err = "training step: engine has no propagator"; return LNS_ESTATE; }
    if (int brc = check_batch(e, B)) return brc;
    StepLayout S; int rc;
    if ((rc = step_layout(e, B, H, W, T, S))) return rc;
    *bytes = S.total;
    return prebuild_train_plan(e, B, H, W);
}

// lns_train_step (adam_spec or neither) and lns_train_step_clip (update_spec): one body, so the two cannot drift apart
static int train_step_impl(lns_engine* e, float* const* params, const float* z_in, const float* z_out, const float* param,
                           int B, int H, int W, int T, float beta, float* const* grads, float* const* exp_avg,
                           float* const* exp_avg_sq, const lns_adam_spec* adam_spec, const lns_update_spec* update_spec, bool clip,
                           float* loss_out, float* norm_out, void* ws, size_t ws_bytes, void* stream) {
    if (!e) return LNS_EINVAL;
    // ---- host-only checks ----
    if (e->cfg.prop_kind != LNS_PROP_PLAIN && e->cfg.prop_kind != LNS_PROP_CONDITIONAL) { e->err = "training step: engine has no propagator"; return LNS_ESTATE; }
    if (B < 1) { e->err = "training step: B must be >= 1"; return LNS_EINVAL; }
    if (T < 1) { e->err = "training step: T must be >= 1"; return LNS_EINVAL; }
    if (int brc = check_batch(e, B)) return brc;
    if (!params || !grads) { e->err = "training step: params / grads array is null"; return LNS_EINVAL; }
    if (!z_in || !z_out) { e->err = "training step: z_in / z_out is null"; return LNS_EINVAL; }
    if (e->cfg.prop_kind == LNS_PROP_CONDITIONAL && !param) { e->err = "training step: conditional propagator needs param"; return LNS_EINVAL; }
    int rc;
    AdamScalars sc;
    UpdatePlan up;
    if (adam_spec && (rc = adam_scalars(adam_spec, sc, e->err))) return rc;
    if (clip && (rc = update_scalars(update_spec, up, e->err))) return rc;
    const PropParams* pp;
    if ((rc = prop_params(e, &pp)) || (rc = check_params(e, *pp, params, "parameter")) ||
        (rc = check_params(e, *pp, const_cast<const float* const*>(grads), "gradient"))) return rc;
    if (adam_spec || clip) {
        if (!exp_avg || !exp_avg_sq) { e->err = "training step: exp_avg / exp_avg_sq array is null (adam_spec is given)"; return LNS_EINVAL; }
        if ((rc = check_params(e, *pp, const_cast<const float* const*>(exp_avg), "exp_avg")) ||
            (rc = check_params(e, *pp, const_cast<const float* const*>(exp_avg_sq), "exp_avg_sq"))) return rc;
    }
    StepLayout S;
    if ((rc = step_layout(e, B, H, W, T, S)) || (rc = loss_check((int64_t)S.n, beta, loss_out, e->err))) return rc;
    ClipLayout C;
    if (clip) clip_layout(e, *pp, S, C);
    const size_t need = clip ? C.total : S.total;
    if (!ws || ws_bytes < need) { e->err = fmt("training step workspace too small: need %zu bytes", need); return LNS_ENOMEM; }
    // ---- where the tensors live (pointer attributes: the first HIP calls), still before anything is enqueued ----
    int device = -1;
    if ((rc = train_device_of(e, z_in, &device)) || (rc = train_same_device(e, device, z_out, "z_out")) ||
        (rc = train_same_device(e, device, loss_out, "loss_out")) || (rc = train_same_device(e, device, ws, "the workspace"))) return rc;
    if (clip && norm_out && (rc = train_same_device(e, device, norm_out, "norm_out"))) return rc;
    // ---- device work, in stream order ----
    char* base = static_cast<char*>(ws);
    float* z_pred = reinterpret_cast<float*>(base + S.z_pred);
    float* dz = reinterpret_cast<float*>(base + S.dz);
    float* part = reinterpret_cast<float*>(base + S.part);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = lns_train_forward(e, params, z_in, param, B, H, W, T, z_pred, ws, S.train, stream))) return rc;
    DeviceGuard dg(device);
    HIPCHK(e, launch_smooth_l1(z_pred, z_out, (long)S.n, beta, loss_out, dz, part, s));
    if ((rc = lns_train_backward(e, params, z_in, z_pred, dz, B, H, W, T, grads, nullptr, ws, S.train, stream))) return rc;
    if (!adam_spec && !clip) return LNS_OK;
    // only the propagator's tensors: other entries of the arrays are not this step's business
    std::vector<AdamTensor> tt;
    tt.reserve(pp->all.size());
    for (int v : pp->all) tt.push_back(AdamTensor{params[v], grads[v], exp_avg[v], exp_avg_sq[v], (unsigned)e->params[v].numel(), 0u});
    if (!clip) {
        HIPCHK(e, launch_adam_multi(tt.data(), (int)tt.size(), sc, s));
        return LNS_OK;
    }
    std::vector<NormTensor> nt;
    nt.reserve(tt.size());
    for (const AdamTensor& t : tt) nt.push_back(NormTensor{t.g, t.n, 0u});
    float* coef = reinterpret_cast<float*>(base + C.coef);
    HIPCHK(e, launch_grad_norm(nt.data(), (int)nt.size(), up.max_norm, up.skip, norm_out ? norm_out : reinterpret_cast<float*>(base + C.norm),
                               coef, reinterpret_cast<unsigned*>(base + C.counter), reinterpret_cast<double*>(base + C.part), s));
    HIPCHK(e, launch_update_multi(tt.data(), (int)tt.size(), up.sc, coef, up.decoupled, up.decay, s));
    return LNS_OK;
}

int lns_train_step(lns_engine* e, float* const* params, const float* z_in, const float* z_out, const float* param,
                   int B, int H, int W, int T, float beta, float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const lns_adam_spec* adam_spec, float* loss_out, void* ws,
                   size_t ws_bytes, void* stream) {
    return train_step_impl(e, params, z_in, z_out, param, B, H, W, T, beta, grads, exp_avg, exp_avg_sq, adam_spec, nullptr, false,
                           loss_out, nullptr, ws, ws_bytes, stream);
}

int lns_train_step_clip(lns_engine* e, float* const* params, const float* z_in, const float* z_out, const float* param,
                        int B, int H, int W, int T, float beta, float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const lns_update_spec* spec, float* loss_out, float* norm_out, void* ws,
                        size_t ws_bytes, void* stream) {
    return train_step_impl(e, params, z_in, z_out, param, B, H, W, T, beta, grads, exp_avg, exp_avg_sq, nullptr, spec, true,
                           loss_out, norm_out, ws, ws_bytes, stream);
}

int lns_train_step_clip_workspace_bytes(lns_engine* e, int B, int H, int W, int T, size_t* bytes) {
    size_t step = 0;
    if (e && !bytes) { e->err = "training step: bytes is null"; return LNS_EINVAL; }
    if (int rc = lns_train_step_workspace_bytes(e, B, H, W, T, &step)) return rc;
    const PropParams* pp;
    if (int rc = prop_params(e, &pp)) return rc;
    StepLayout S; ClipLayout C;
    S.total = step;
    clip_layout(e, *pp, S, C);
    *bytes = C.total;
    return LNS_OK;
}

// ---- the norm and the update on their own: any n fp32 tensors (lns_amd/optim.py) ----
int lns_grad_norm_scratch_bytes(int n, const int64_t* numel, size_t* bytes) {
    std::string& err = g_create_error;
    if (!bytes) { err = "grad norm: bytes is null"; return LNS_EINVAL; }
    return norm_tensors(n, nullptr, numel, nullptr, *bytes, err);
}

int lns_grad_norm_tensors(int n, const float* const* grads, const int64_t* numel, double max_norm, float* norm_out, float* coef_out,
                          uint32_t* skipped, uint32_t flags, void* scratch, size_t scratch_bytes, void* stream) {
    std::string& err = g_create_error;
    if (n < 0 || (n > 0 && !grads)) { err = "grad norm: grads is null"; return LNS_EINVAL; }
    if (flags & ~(LNS_UPDATE_DECOUPLED_WD | LNS_UPDATE_SKIP_NONFINITE)) { err = fmt("grad norm: unknown flags 0x%x", flags); return LNS_EINVAL; }
    if (std::isnan(max_norm)) { err = "grad norm: max_norm is NaN (<= 0 means: no clipping)"; return LNS_EINVAL; }
    std::vector<NormTensor> tt;
    size_t need = 0;
    if (int rc = norm_tensors(n, grads, numel, &tt, need, err)) return rc;
    if (need > 0 && (!scratch || scratch_bytes < need)) { err = fmt("grad norm: scratch must hold %zu bytes", need); return LNS_ENOMEM; }
    const hipError_t rc = launch_grad_norm(tt.data(), (int)tt.size(), clip_threshold(max_norm), (flags & LNS_UPDATE_SKIP_NONFINITE) ? 1 : 0, norm_out, coef_out,
                                           skipped, static_cast<double*>(scratch), static_cast<hipStream_t>(stream));
    if (rc != hipSuccess) { err = std::string("grad norm: ") + hipGetErrorString(rc); return LNS_EHIP; }
    return LNS_OK;
}

int lns_grad_scale_tensors(int n, float* const* grads, const int64_t* numel, const float* coef, void* stream) {
    std::string& err = g_create_error;
    if (n < 0 || (n > 0 && !grads)) { err = "grad scale: grads is null"; return LNS_EINVAL; }
    if (!coef) { err = "grad scale: coef is null"; return LNS_EINVAL; }
    std::vector<NormTensor> tt;
    size_t unused = 0;
    if (int rc = norm_tensors(n, grads, numel, &tt, unused, err)) return rc;
    if (tt.empty()) return LNS_OK;
    const hipError_t rc = launch_grad_scale(tt.data(), (int)tt.size(), coef, static_cast<hipStream_t>(stream));
    if (rc != hipSuccess) { err = std::string("grad scale: ") + hipGetErrorString(rc); return LNS_EHIP; }
    return LNS_OK;
}

int lns_update_step_tensors(int n, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                            const int64_t* numel, const lns_update_spec* spec, const float* coef, void* stream) {
    std::string& err = g_create_error;
    if (n < 0 || (n > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numel))) { err = "update: null pointer array"; return LNS_EINVAL; }
    UpdatePlan up;
    if (int rc = update_scalars(spec, up, err)) return rc;
    std::vector<AdamTensor> tt;
    tt.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]) continue;
        if (numel[i] < 1 || numel[i] >= (int64_t)1 << 31) { err = fmt("update: tensor %d has %lld elements (1 .. 2^31 - 1)", i, (long long)numel[i]); return LNS_EINVAL; }
        tt.push_back(AdamTensor{params[i], grads[i], exp_avg[i], exp_avg_sq[i], (unsigned)numel[i], 0u});
    }
    if (tt.empty()) return LNS_OK;
    const hipError_t rc = launch_update_multi(tt.data(), (int)tt.size(), up.sc, coef, up.decoupled, up.decay, static_cast<hipStream_t>(stream));
    if (rc != hipSuccess) { err = std::string("update: ") + hipGetErrorString(rc); return LNS_EHIP; }
    return LNS_OK;
}

// ---- weight gradient of a stride-1 "same" convolution, both forms (csrc/lns_train_kernels.hip, csrc/wgrad_split.inc) ----
static int wgrad_op_check(int B, int Cin, int Cout, int H, int W, int ksize, int form) {
    if (B < 1 || B > LNS_MAX_BATCH || Cin < 1 || Cout < 1 || Cin > 65536 || Cout > 65536 || H < 1 || W < 1 || H > 4096 || W > 4096) {
        g_create_error = "conv_wgrad: B in 1..65535, Cin / Cout in 1..65536, H / W in 1..4096"; return LNS_EINVAL;
    }
    if (ksize != 1 && ksize != 3) { g_create_error = "conv_wgrad: ksize must be 1 or 3"; return LNS_EINVAL; }
    if (form != 0 && form != 1) { g_create_error = "conv_wgrad: form must be 0 (one block per output tile) or 1 (batch-parallel)"; return LNS_EINVAL; }
    return LNS_OK;
}
int lns_op_conv_wgrad_scratch_bytes(int B, int Cin, int Cout, int H, int W, int ksize, int form, size_t* bytes) {
    if (!bytes) { g_create_error = "conv_wgrad: bytes is null"; return LNS_EINVAL; }
    if (int rc = wgrad_op_check(B, Cin, Cout, H, W, ksize, form)) return rc;
    *bytes = form == 1 ? round64(wgrad_split_scratch_floats(B, H, W, Cin, Cout, ksize)) * 4 : 0;
    return LNS_OK;
}
int lns_op_conv_wgrad(const float* dy, const float* x, int B, int Cin, int Cout, int H, int W, int ksize, int dilation, int pad_y,
                      int pad_x, int form, int accumulate, float* dw, void* scratch, size_t scratch_bytes, void* stream) {
    // every check precedes the first HIP call
    if (!dy || !x || !dw) { g_create_error = "conv_wgrad: dy / x / dw is null"; return LNS_EINVAL; }
    if (int rc = wgrad_op_check(B, Cin, Cout, H, W, ksize, form)) return rc;
    if (dilation < 1 || dilation > 64) { g_create_error = "conv_wgrad: dilation must be in 1..64"; return LNS_EINVAL; }
    if ((pad_y != LNS_PAD_ZEROS && pad_y != LNS_PAD_CIRCULAR) || (pad_x != LNS_PAD_ZEROS && pad_x != LNS_PAD_CIRCULAR)) {
        g_create_error = "conv_wgrad: pad_y / pad_x must be LNS_PAD_ZEROS or LNS_PAD_CIRCULAR"; return LNS_EINVAL;
    }
    if (accumulate != 0 && accumulate != 1) { g_create_error = "conv_wgrad: accumulate must be 0 or 1"; return LNS_EINVAL; }
    size_t need = 0;
    (void)lns_op_conv_wgrad_scratch_bytes(B, Cin, Cout, H, W, ksize, form, &need);
    if (form == 1 && (!scratch || scratch_bytes < need)) { g_create_error = fmt("conv_wgrad: scratch too small: need %zu bytes", need); return LNS_ENOMEM; }
    const int p = dilation * (ksize - 1) / 2;
    std::vector<int> fr, fc;                                     // the whole-image maps, as tconv_setup builds them
    build_axis_map(fr, H + 2 * p, H, H, 0.0f, p, p, pad_y);
    build_axis_map(fc, W + 2 * p, W, W, 0.0f, p, p, pad_x);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (form == 1) OPCHK(init_train_kernels());
    int* dmap = nullptr;
    OPCHK(hipMalloc(reinterpret_cast<void**>(&dmap), (fr.size() + fc.size()) * 4));
    hipError_t he = hipMemcpy(dmap, fr.data(), fr.size() * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(dmap + fr.size(), fc.data(), fc.size() * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) {
        WgradArgs a;
        memset(&a, 0, sizeof a);
        a.dy = dy; a.x = x; a.rowmap = dmap; a.colmap = dmap + fr.size(); a.dw = dw;
        a.B = B; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.k = ksize; a.dil = dilation; a.accumulate = accumulate;
        a.x_bs = (long)Cin * H * W; a.part = static_cast<float*>(scratch); a.S = wgrad_split_slices(B, H, W, Cin, Cout, ksize);
        he = form == 1 ? launch_conv_wgrad_split(a, s) : launch_conv_wgrad(a, s);
    }
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    (void)hipFree(dmap);
    OPCHK(he);
    return LNS_OK;
}

// ---- elementwise / reduction kernels of the backward pass on their own (csrc/lns_train_kernels.hip): the launchers the
// training rollout calls, nothing else.  Every check precedes the first HIP call; each call synchronises `stream`. ----
int lns_op_groupnorm_train(const float* x, int B, int C, int HW, int groups, float eps, const float* gamma, const float* beta,
                           float* y, float* stats, const float* dy, const float* add, float* dx, float* dgamma, float* dbeta,
                           int accumulate, float* part, void* stream) {
    if (!x || !gamma || !beta || !y || !stats) { g_create_error = "groupnorm_train: x / gamma / beta / y / stats is null"; return LNS_EINVAL; }
    if (B < 1 || B > LNS_MAX_BATCH || C < 1 || C > 65536 || HW < 1 || HW > 4096 * 4096 || groups < 1 || groups > C || C % groups != 0) {
        g_create_error = "groupnorm_train: B in 1..65535, C in 1..65536, HW in 1..4096*4096, groups a divisor of C"; return LNS_EINVAL;
    }
    if (!(eps > 0.0f) || !std::isfinite(eps)) { g_create_error = "groupnorm_train: eps must be positive and finite"; return LNS_EINVAL; }
    if (dy && (!dx || !dgamma || !dbeta || !part)) { g_create_error = "groupnorm_train: the backward (dy given) needs dx, dgamma, dbeta and part"; return LNS_EINVAL; }
    if (!dy && add) { g_create_error = "groupnorm_train: add belongs to the backward (dy is null)"; return LNS_EINVAL; }
    if (accumulate != 0 && accumulate != 1) { g_create_error = "groupnorm_train: accumulate must be 0 or 1"; return LNS_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    GnTrainArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.y = y; a.stats = stats; a.gamma = gamma; a.beta = beta;
    a.B = B; a.C = C; a.HW = HW; a.groups = groups; a.eps = eps;
    OPCHK(launch_gn_train_fwd(a, s));
    if (dy) {
        a.dy = dy; a.dx = dx; a.add = add; a.part = part;
        OPCHK(launch_gn_train_bwd(a, s));
        OPCHK(launch_colsum2(part, B, C, dgamma, dbeta, accumulate, s));
    }
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

int lns_op_gelu_grad(const float* dy, const float* u, float* du, int64_t n, void* stream) {
    if (!dy || !u || !du) { g_create_error = "gelu_grad: dy / u / du is null"; return LNS_EINVAL; }
    if (n < 1 || n > ((int64_t)1 << 40)) { g_create_error = "gelu_grad: n in 1..2^40"; return LNS_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    OPCHK(launch_gelu_bwd(dy, u, du, (long)n, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

int lns_op_bias_grad(const float* dy, int B, int C, int HW, float* db, int accumulate, void* stream) {
    if (!dy || !db) { g_create_error = "bias_grad: dy / db is null"; return LNS_EINVAL; }
    if (B < 1 || B > LNS_MAX_BATCH || C < 1 || C > 65536 || HW < 1 || HW > 4096 * 4096) {
        g_create_error = "bias_grad: B in 1..65535, C in 1..65536, HW in 1..4096*4096"; return LNS_EINVAL;
    }
    if (accumulate != 0 && accumulate != 1) { g_create_error = "bias_grad: accumulate must be 0 or 1"; return LNS_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    OPCHK(launch_bias_grad(dy, B, C, HW, db, accumulate, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Latent fit (include/lns.h "latent fit"): the observation loss of a rollout, and one iteration of fitting the initial
// latent and / or `param` to observed latents -- training forward, observation loss, state-only adjoint, Adam on z0 / param.
// No reference counterpart (the reference never differentiates with respect to its inputs).  Every argument check is
// host-only and precedes the first HIP call.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

static_assert(LNS_OBS_MAX == OBS_MAX, "include/lns.h and lns_train_kernels.h name the same table length");

// the observation table -> the kernels' argument; T < 0: the steps only have to ascend
int obs_table(int n_obs, const int* steps, const double* weight, int T, int64_t n, double lambda, bool has_bg, ObsTable& tb, std::string& err) {
    if (n_obs < 1 || n_obs > OBS_MAX) { err = fmt("obs loss: n_obs must be in 1 .. %d, got %d", OBS_MAX, n_obs); return LNS_EINVAL; }
    if (!steps) { err = "obs loss: obs_steps is null"; return LNS_EINVAL; }
    if (n < 1 || n >= (int64_t)1 << 31) { err = "obs loss: n (elements of a latent) must be in 1 .. 2^31 - 1"; return LNS_EINVAL; }
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) { err = "obs loss: background must be finite and >= 0"; return LNS_EINVAL; }
    memset(&tb, 0, sizeof tb);
    tb.n_obs = n_obs; tb.has_bg = has_bg ? 1 : 0;
    tb.inv_n = 1.0 / (double)n; tb.lambda = lambda;
    tb.coef_bg = (float)(2.0 * lambda / (double)n);
    for (int k = 0; k < n_obs; ++k) {
        if (steps[k] < 0 || steps[k] >= (1 << 24) || (T >= 0 && steps[k] >= T) || (k > 0 && steps[k] <= steps[k - 1])) {
            err = fmt("obs loss: obs_steps must be strictly ascending 0-based steps%s (entry %d is %d)", T >= 0 ? " below T" : "", k, steps[k]);
            return LNS_EINVAL;
        }
        const double w = weight ? weight[k] : 1.0;
        if (!(w >= 0.0) || !std::isfinite(w)) { err = fmt("obs loss: obs_weight must be finite and >= 0 (entry %d)", k); return LNS_EINVAL; }
        tb.steps[k] = steps[k]; tb.weight[k] = w;
        tb.coef[k] = (float)(2.0 * w / (double)n);                  // rounded once from double
    }
    return LNS_OK;
}

size_t obs_part_bytes(int B, int n_obs) { return round256((size_t)B * (size_t)(n_obs + 1) * 8); }

// workspace of the fit step (bytes): lns_train_step's layout for T steps | double partials | gradient of the background term
struct FitLayout { StepLayout S; size_t part = 0, gbg = 0, total = 0; };
int fit_layout(lns_engine* e, int B, int H, int W, int T, int n_obs, FitLayout& F) {
    if (int rc = step_layout(e, B, H, W, T, F.S)) return rc;
    F.part = F.S.total;
    F.gbg = F.part + obs_part_bytes(B, n_obs);
    F.total = F.gbg + round256(F.S.n / (size_t)T * 4);
    return LNS_OK;
}

// an update spec of the fit: lns_update_spec's checks, and neither flags nor clipping (there is no norm pass in the step)
int fit_update(const lns_update_spec* sp, const char* which, UpdatePlan& u, std::string& err) {
    std::string inner;
    if (int rc = update_scalars(sp, u, inner)) { err = fmt("fit step: %s: %s", which, inner.c_str()); return rc; }
    if (sp->flags != 0) { err = fmt("fit step: %s.flags must be 0", which); return LNS_EINVAL; }
    if (sp->max_norm != 0.0) { err = fmt("fit step: %s.max_norm must be 0 (no clipping inside the fit step)", which); return LNS_EINVAL; }
    return LNS_OK;
}

}  // namespace

int lns_loss_obs_mse_scratch_bytes(int B, int n_obs, size_t* bytes) {
    std::string& err = g_create_error;
    if (!bytes) { err = "obs loss: bytes is null"; return LNS_EINVAL; }
    if (B < 1 || B > LNS_MAX_BATCH) { err = fmt("obs loss: B must be in 1 .. %d", LNS_MAX_BATCH); return LNS_EINVAL; }
    if (n_obs < 1 || n_obs > OBS_MAX) { err = fmt("obs loss: n_obs must be in 1 .. %d, got %d", OBS_MAX, n_obs); return LNS_EINVAL; }
    *bytes = obs_part_bytes(B, n_obs);
    return LNS_OK;
}

int lns_loss_obs_mse(const float* z_pred, const float* obs, int B, int T, int64_t n, int n_obs, const int* obs_steps,
                     const double* obs_weight, const float* z0, const float* z_background, double background, float* per,
                     float* loss, float* grad_z_pred, float* grad_z0_bg, void* scratch, size_t scratch_bytes, void* stream) {
    std::string& err = g_create_error;
    if (!z_pred || !obs) { err = "obs loss: z_pred / obs is null"; return LNS_EINVAL; }
    if (!loss || !grad_z_pred) { err = "obs loss: loss / grad_z_pred is null"; return LNS_EINVAL; }
    if (B < 1 || B > LNS_MAX_BATCH) { err = fmt("obs loss: B must be in 1 .. %d", LNS_MAX_BATCH); return LNS_EINVAL; }
    if (T < 1) { err = "obs loss: T must be >= 1"; return LNS_EINVAL; }
    if ((z0 == nullptr) != (z_background == nullptr)) { err = "obs loss: z0 and z_background come together (the background term) or not at all"; return LNS_EINVAL; }
    const bool has_bg = z0 != nullptr;
    if (!has_bg && background > 0.0) { err = "obs loss: background > 0 needs z0 and z_background"; return LNS_EINVAL; }
    if (!has_bg && grad_z0_bg) { err = "obs loss: grad_z0_bg needs z0 and z_background"; return LNS_EINVAL; }
    ObsTable tb;
    if (int rc = obs_table(n_obs, obs_steps, obs_weight, T, n, background, has_bg, tb, err)) return rc;
    const size_t need = obs_part_bytes(B, n_obs);
    if (!scratch || scratch_bytes < need) { err = fmt("obs loss: scratch must hold %zu bytes", need); return LNS_ENOMEM; }
    const hipError_t rc = launch_obs_mse(tb, z_pred, obs, z0, z_background, B, T, (long)n, per, loss, grad_z_pred, grad_z0_bg,
                                         static_cast<double*>(scratch), static_cast<hipStream_t>(stream));
    if (rc != hipSuccess) { err = std::string("obs loss: ") + hipGetErrorString(rc); return LNS_EHIP; }
    return LNS_OK;
}

int lns_fit_step_workspace_bytes(lns_engine* e, int B, int H, int W, int T, int n_obs, size_t* bytes) {
    if (!e) return LNS_EINVAL;
    if (B < 1) { e->err = "fit step: B must be >= 1"; return LNS_EINVAL; }
    if (T < 1) { e->err = "fit step: T must be >= 1"; return LNS_EINVAL; }
    if (n_obs < 1 || n_obs > OBS_MAX) { e->err = fmt("fit step: n_obs must be in 1 .. %d, got %d", OBS_MAX, n_obs); return LNS_EINVAL; }
    if (!bytes) { e->err = "fit step: bytes is null"; return LNS_EINVAL; }
    if (e->cfg.prop_kind != LNS_PROP_PLAIN && e->cfg.prop_kind != LNS_PROP_CONDITIONAL) { e->err = "fit step: engine has no propagator"; return LNS_ESTATE; }
    if (int brc = check_batch(e, B)) return brc;
    FitLayout F; int rc;
    if ((rc = fit_layout(e, B, H, W, T, n_obs, F))) return rc;
    *bytes = F.total;
    return prebuild_train_plan(e, B, H, W);
}

int lns_fit_step(lns_engine* e, const float* const* params, float* z0, float* param, const float* obs, const float* z_background,
                 int B, int H, int W, const lns_fit_spec* spec, float* g_z, float* exp_avg_z, float* exp_avg_sq_z, float* g_p,
                 float* exp_avg_p, float* exp_avg_sq_p, float* loss, float* per, void* ws, size_t ws_bytes, void* stream) {
    if (!e) return LNS_EINVAL;
    // ---- host-only checks ----
    const bool cond = e->cfg.prop_kind == LNS_PROP_CONDITIONAL;
    if (e->cfg.prop_kind != LNS_PROP_PLAIN && !cond) { e->err = "fit step: engine has no propagator"; return LNS_ESTATE; }
    if (!spec || spec->size != sizeof(lns_fit_spec)) { e->err = "fit step: spec is null or its size field is not sizeof(lns_fit_spec)"; return LNS_EINVAL; }
    if ((spec->flags & ~(LNS_FIT_STATE | LNS_FIT_PARAM)) || !(spec->flags & (LNS_FIT_STATE | LNS_FIT_PARAM))) {
        e->err = fmt("fit step: flags 0x%x: LNS_FIT_STATE and / or LNS_FIT_PARAM, nothing else", spec->flags); return LNS_EINVAL;
    }
    const bool fit_z = spec->flags & LNS_FIT_STATE, fit_p = spec->flags & LNS_FIT_PARAM;
    if (fit_p && !cond) { e->err = "fit step: flags: LNS_FIT_PARAM needs the conditional propagator"; return LNS_EINVAL; }
    if (B < 1) { e->err = "fit step: B must be >= 1"; return LNS_EINVAL; }
    if (int brc = check_batch(e, B)) return brc;
    if (!params) { e->err = "fit step: params array is null"; return LNS_EINVAL; }
    if (!z0 || !obs) { e->err = "fit step: z0 / obs is null"; return LNS_EINVAL; }
    if (cond && !param) { e->err = "fit step: conditional propagator needs param"; return LNS_EINVAL; }
    if (!loss) { e->err = "fit step: loss is null"; return LNS_EINVAL; }
    if (fit_z && (!g_z || !exp_avg_z || !exp_avg_sq_z)) { e->err = "fit step: LNS_FIT_STATE needs g_z, exp_avg_z and exp_avg_sq_z"; return LNS_EINVAL; }
    if (fit_p && (!g_p || !exp_avg_p || !exp_avg_sq_p)) { e->err = "fit step: LNS_FIT_PARAM needs g_p, exp_avg_p and exp_avg_sq_p"; return LNS_EINVAL; }
    int rc;
    TrainPlan dims;
    if ((rc = train_plan_dims(e, B, H, W, dims))) return rc;
    const int64_t n = (int64_t)dims.c * H * W;
    if ((int64_t)B * n >= (int64_t)1 << 31) { e->err = "fit step: z0 has 2^31 or more elements"; return LNS_EINVAL; }
    const bool has_bg = z_background != nullptr;
    if (!has_bg && spec->background > 0.0) { e->err = "fit step: background > 0 needs z_background"; return LNS_EINVAL; }
    ObsTable tb;
    if ((rc = obs_table(spec->n_obs, spec->obs_steps, spec->obs_weight, -1, n, spec->background, has_bg, tb, e->err))) return rc;
    const int T = spec->obs_steps[spec->n_obs - 1] + 1;
    UpdatePlan uz, up;
    if (fit_z && (rc = fit_update(&spec->state, "state", uz, e->err))) return rc;
    if (fit_p && (rc = fit_update(&spec->param, "param", up, e->err))) return rc;
    const PropParams* pp;
    if ((rc = prop_params(e, &pp)) || (rc = check_params(e, *pp, params, "parameter"))) return rc;
    FitLayout F;
    if ((rc = fit_layout(e, B, H, W, T, spec->n_obs, F))) return rc;
    if (!ws || ws_bytes < F.total) { e->err = fmt("fit step workspace too small: need %zu bytes", F.total); return LNS_ENOMEM; }
    // ---- where the tensors live (pointer attributes: the first HIP calls), still before anything is enqueued ----
    int device = -1;
    if ((rc = train_device_of(e, z0, &device)) || (rc = train_same_device(e, device, obs, "obs")) ||
        (rc = train_same_device(e, device, z_background, "z_background")) || (rc = train_same_device(e, device, loss, "loss")) ||
        (rc = train_same_device(e, device, per, "per")) || (rc = train_same_device(e, device, ws, "the workspace")) ||
        (rc = train_same_device(e, device, g_z, "g_z")) || (rc = train_same_device(e, device, g_p, "g_p"))) return rc;
    // ---- device work, in stream order ----
    char* base = static_cast<char*>(ws);
    float* z_pred = reinterpret_cast<float*>(base + F.S.z_pred);
    float* dz = reinterpret_cast<float*>(base + F.S.dz);
    double* part = reinterpret_cast<double*>(base + F.part);
    float* gbg = fit_z && has_bg ? reinterpret_cast<float*>(base + F.gbg) : nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = lns_train_forward(e, params, z0, param, B, H, W, T, z_pred, ws, F.S.train, stream))) return rc;
    DeviceGuard dg(device);
    HIPCHK(e, launch_obs_mse(tb, z_pred, obs, has_bg ? z0 : nullptr, z_background, B, T, (long)n, per, loss, dz, gbg, part, s));
    if ((rc = lns_train_backward_ex(e, params, z0, z_pred, dz, B, H, W, T, nullptr, fit_z ? g_z : nullptr, ws, F.S.train, stream,
                                    fit_p ? g_p : nullptr))) return rc;
    if (gbg) HIPCHK(e, launch_add(g_z, gbg, g_z, (long)((int64_t)B * n), s));          // g_z = grad_z_in + grad_z0_bg, on its own
    if (fit_z) {
        AdamTensor t{z0, g_z, exp_avg_z, exp_avg_sq_z, (unsigned)((int64_t)B * n), 0u};
        HIPCHK(e, launch_update_multi(&t, 1, uz.sc, nullptr, uz.decoupled, uz.decay, s));
    }
    if (fit_p) {
        AdamTensor t{param, g_p, exp_avg_p, exp_avg_sq_p, (unsigned)B, 0u};
        HIPCHK(e, launch_update_multi(&t, 1, up.sc, nullptr, up.decoupled, up.decay, s));
    }
    return LNS_OK;
}
