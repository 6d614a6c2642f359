// ---------------------------------------------------------------------------------------------------------------------
// Tangent-linear rollout of the latent propagator (include/lns.h "tangent-linear rollout"; included by lns_engine.cpp after
// lns_train.inc, whose plans, layout, tape view and run_tconv it uses).
//
// lns_train_tangent carries K perturbations of every sample's initial latent forward along the trajectory a preceding
// lns_train_forward computed: v <- J_t v for t = t0 .. t0 + nsteps - 1, J_t the Jacobian of propagator step t with respect
// to its input latent.  It reads that call's tape (GroupNorm inputs and statistics, GELU pre-activations, the conditional
// vectors) and its forward weight packs, and follows lns_train_forward line by line: every convolution is the same launch
// without bias on the plan of batch B*K, GroupNorm / GELU / the channel scale are their JVP kernels (tangent.inc).  The
// conditional propagator's emb and m depend on `param` only, so their tangents are zero: dh = conv1.3(da1) with no broadcast
// add, dxm = dx1 (1 + m).  No reference counterpart (the reference never linearises its propagator).
//
// Weight packs and the plan's batch: a pack is [tap][Cin_pad][Cout_pad] with the pads of conv_padded_sizes(k, Cin, Cout) --
// TConv::pack_floats(), launch_pack_conv_w and conv_padded_sizes take no batch, and conv_geometry is handed Cout_pad and the
// pack's kc_log2 instead of choosing them.  What the batch does choose is the tile variant (the 64 / 32-cout fp32 forms by
// block count), which only has to divide Cout_pad.  So the packs the forward wrote for batch B serve the plan of batch B*K;
// the tiling, and with it the summation order inside a convolution, may differ between two values of B*K.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

// bytes: lns_train_workspace_bytes' layout, untouched | 4 tangent tensors [B*K][D][HW] | one latent tangent [B*K][c][HW]
struct TangentLayout { TrainLayout L; size_t scratch = 0, tn = 0, z = 0, total = 0; };
void tangent_layout(const TrainPlan& dimsB, int T, int K, int wgrad_form, TangentLayout& G) {
    train_layout(dimsB, T, G.L, wgrad_form);
    G.scratch = round256(G.L.total * 4);
    G.tn = round256(G.L.n * (size_t)K * 4);
    G.z = G.scratch + 4 * G.tn;
    G.total = G.z + round256(G.L.nl * (size_t)K * 4);
}

// what both entry points refuse, in include/lns.h's order, before any HIP call (the null checks are the caller's)
int tangent_refusal(lns_engine* e, int B, int H, int W, int T, int K, int t0, int nsteps, TrainPlan& dims) {
    if (K < 1 || K > LNS_TANGENT_MAX) { e->err = fmt("tangent rollout: K must be in 1 .. %d, got %d", LNS_TANGENT_MAX, K); return LNS_EINVAL; }
    if (B < 1) { e->err = "tangent rollout: B must be >= 1"; return LNS_EINVAL; }
    if ((long)B * K > LNS_MAX_BATCH) { e->err = fmt("tangent rollout: B * K = %ld rows exceed the maximum of %d per call", (long)B * K, LNS_MAX_BATCH); return LNS_EINVAL; }
    if (T < 1 || t0 < 0 || nsteps < 1 || (long)t0 + nsteps > T) {
        e->err = fmt("tangent rollout: steps t0 .. t0 + nsteps - 1 must lie in 0 .. T - 1 (T %d, t0 %d, nsteps %d)", T, t0, nsteps);
        return LNS_EINVAL;
    }
    if (e->cfg.prop_kind != LNS_PROP_PLAIN && e->cfg.prop_kind != LNS_PROP_CONDITIONAL) { e->err = "tangent rollout: engine has no propagator"; return LNS_ESTATE; }
    return train_plan_dims(e, B, H, W, dims);
}

}  // namespace

int lns_train_tangent_workspace_bytes(lns_engine* e, int B, int H, int W, int T, int K, size_t* bytes) {
    if (!e) return LNS_EINVAL;
    if (!bytes) { e->err = "tangent rollout: bytes is null"; return LNS_EINVAL; }
    TrainPlan dims;
    if (int rc = tangent_refusal(e, B, H, W, T, K, 0, 1, dims)) return rc;
    TangentLayout G;
    tangent_layout(dims, T, K, e->opt_train_wgrad, G);
    *bytes = G.total;
    return LNS_OK;
}

int lns_train_tangent(lns_engine* e, const float* const* params, int B, int H, int Wd, int T, int K, int t0, int nsteps, float* v,
                      float* jv_out, void* ws, size_t ws_bytes, void* stream) {
    if (!e) return LNS_EINVAL;
    if (!params) { e->err = "tangent rollout: params array is null"; return LNS_EINVAL; }
    if (!v) { e->err = "tangent rollout: v is null"; return LNS_EINVAL; }
    TrainPlan dims;
    int rc, device = -1;
    if ((rc = tangent_refusal(e, B, H, Wd, T, K, t0, nsteps, dims))) return rc;
    if ((rc = train_device_of(e, v, &device)) || (rc = train_same_device(e, device, jv_out, "jv_out")) ||
        (rc = train_same_device(e, device, ws, "the workspace"))) return rc;
    TangentLayout G;
    tangent_layout(dims, T, K, e->opt_train_wgrad, G);
    if (!ws || ws_bytes < G.total) { e->err = fmt("tangent workspace too small: need %zu bytes", G.total); return LNS_ENOMEM; }
    const PropParams* ppp;
    if ((rc = prop_params(e, &ppp)) || (rc = check_params(e, *ppp, params, "parameter"))) return rc;
    const PropParams& pp = *ppp;
    // ---- device work, in stream order ----
    DeviceGuard dg(device);
    HIPCHK(e, init_kernels());
    const int R = B * K;
    TrainPlan* pl;
    if ((rc = get_train_plan(e, device, R, H, Wd, &pl))) return rc;
    const TrainPlan& p = *pl;                      // the convolutions' plan: batch B*K; the tape's layout is batch B's (dims, L)
    const TrainLayout& L = G.L;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* W = static_cast<float*>(ws);
    char* base = static_cast<char*>(ws);
    float* buf[4];
    for (int i = 0; i < 4; ++i) buf[i] = reinterpret_cast<float*>(base + G.scratch + (size_t)i * G.tn);
    float* zt = reinterpret_cast<float*>(base + G.z);                 // [R][c][HW]: the tangent after the step just run
    const VecView vv = p.cond ? vec_view(dims, L, W) : VecView{};
    const int HW = p.H * p.W, D = p.D;
    const long ns = (long)D * HW;                                     // elements of one sample of a D-channel tensor
    const long nz = (long)p.c * HW;
    auto gn = [&](int groups, const float* x, const float* stats, const float* gamma, const float* dx, const float* add, float* dy) {
        GnJvpArgs a;
        memset(&a, 0, sizeof a);
        a.x = x; a.stats = stats; a.gamma = gamma; a.dx = dx; a.add = add; a.dy = dy;
        a.B = B; a.K = K; a.C = D; a.HW = HW; a.groups = groups;
        return launch_gn_train_jvp(a, s);
    };
    for (int t = t0; t < t0 + nsteps; ++t) {
        const ConstTapeStep tape(L, W, t);
        float *dx = buf[0], *f1 = buf[1], *f2 = buf[2], *f3 = buf[3];         // dx: tangent of the current block's input
        if ((rc = run_tconv(e, p.in_proj, t == t0 ? v : zt, W + L.pk_in, nullptr, dx, nullptr, s))) return rc;
        for (int i = 0; i < p.nb; ++i) {
            const PropParams::Blk& b = pp.blk[i];
            HIPCHK(e, gn(1, tape.block_in(i), tape.stats(i, 0), params[b.g1], dx, nullptr, f1));                // d n1
            if ((rc = run_tconv(e, p.c_d1, f1, W + L.pk(i, BC_C1), nullptr, f2, nullptr, s))) return rc;        // d u1
            HIPCHK(e, launch_gelu_jvp(f2, tape.t(i, TB_U1), f2, R, K, ns, s));                                  // d a1
            if ((rc = run_tconv(e, p.c_dd, f2, W + L.pk(i, BC_C3), nullptr, f1, nullptr, s))) return rc;        // d u2 / d h (emb: none)
            float* dx1;                                                                                         // tangent of x1
            if (!p.cond) {
                HIPCHK(e, launch_gelu_jvp(f1, tape.t(i, TB_U2), f1, R, K, ns, s));                              // d a2
                if ((rc = run_tconv(e, p.c_d1, f1, W + L.pk(i, BC_C5), nullptr, f2, dx, s))) return rc;         // d x1 = d x + conv.5
                dx1 = f2;
                HIPCHK(e, gn(1, tape.t(i, TB_X1), tape.stats(i, 1), params[b.g2], dx1, nullptr, f1));           // d n2
            } else {
                HIPCHK(e, gn(1, tape.t(i, TB_U2), tape.stats(i, 2), params[b.cg], f1, nullptr, f2));            // d GN(h)
                HIPCHK(e, launch_gelu_jvp(f2, tape.t(i, TB_NC), f2, R, K, ns, s));                              // d a2
                if ((rc = run_tconv(e, p.c_d1, f2, W + L.pk(i, BC_C5), nullptr, f3, dx, s))) return rc;         // d x1
                dx1 = f3;
                HIPCHK(e, launch_chan_scale_rows(dx1, vv.blk(i, TV_M), f2, R, K, D, HW, s));                    // d xm
                HIPCHK(e, gn(1, tape.t(i, TB_XM), tape.stats(i, 1), params[b.g2], f2, nullptr, f1));            // d n2
            }
            float* g = dx1 == f2 ? f3 : f2;                                   // free: neither d x1 nor d n2
            if ((rc = run_tconv(e, p.c_1, f1, W + L.pk(i, BC_F1), nullptr, g, nullptr, s))) return rc;          // d v
            HIPCHK(e, launch_gelu_jvp(g, tape.t(i, TB_V), g, R, K, ns, s));                                     // d g
            if ((rc = run_tconv(e, p.c_1, g, W + L.pk(i, BC_F3), nullptr, dx, dx1, s))) return rc;              // d x2 = d x1 + ffn.3
        }
        HIPCHK(e, gn(32, tape.last_x(), tape.stats_out(), params[pp.out_g], dx, nullptr, f1));
        if ((rc = run_tconv(e, p.out_proj, f1, W + L.pk_out, nullptr, zt, nullptr, s))) return rc;
        if (jv_out)                                  // jv_out is [B][K][nsteps][c][HW]: a row's steps are nsteps*c*HW apart
            HIPCHK(e, launch_add_rows(zt, nz, nullptr, 0, jv_out + (size_t)(t - t0) * nz, (long)nsteps * nz, R, nz, s));
    }
    HIPCHK(e, launch_add_rows(zt, nz, nullptr, 0, v, nz, R, nz, s));
    return LNS_OK;
}

int lns_op_orthonormalize(float* v, int B, int K, int64_t n, double* r, double* logr_acc, void* stream) {
    std::string& err = g_create_error;
    if (!v) { err = "orthonormalize: v is null"; return LNS_EINVAL; }
    if (K < 1 || K > LNS_TANGENT_MAX) { err = fmt("orthonormalize: K must be in 1 .. %d, got %d", LNS_TANGENT_MAX, K); return LNS_EINVAL; }
    if (n < 1) { err = "orthonormalize: n must be >= 1"; return LNS_EINVAL; }
    if (B < 1) { err = "orthonormalize: B must be >= 1"; return LNS_EINVAL; }
    const hipError_t rc = launch_orthonormalize(v, B, K, (long)n, r, logr_acc, static_cast<hipStream_t>(stream));
    if (rc != hipSuccess) { err = std::string("orthonormalize: ") + hipGetErrorString(rc); return LNS_EHIP; }
    return LNS_OK;
}
