// ---------------------------------------------------------------------------------------------------------------------
// Gauss-Newton latent fit (include/lns.h "latent fit: Gauss-Newton"; included by lns_engine.cpp after lns_tangent.inc, whose
// layout it extends, and lns_train.inc, whose observation table, forward and state-only adjoint it calls).
//
// lns_train_gn_product: H v = sum_k (2 w_k / n) J_k^T (J_k v) + (2 lambda / n + mu) v on the tape of a preceding
// lns_train_forward -- lns_train_tangent (K = 1, every step kept) into the cotangent area, gn_weight_kernel in place, the
// state-only lns_train_backward_ex, gn_finish.  lns_op_cg_start / lns_op_cg_update: conjugate gradients per sample.
// lns_fit_gn_step: one outer iteration, the bits of its parts called one after the other.  No reference counterpart.
// Every argument check is host-only and precedes the first HIP call.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

// bytes: lns_train_tangent_workspace_bytes(B, h, w, T, 1)'s layout, untouched | cotangent [B][T][n] | double partials
struct GnProductLayout { TangentLayout G; size_t cot = 0, part = 0, total = 0; };
void gn_product_layout(const TrainPlan& dims, int T, int n_obs, int wgrad_form, GnProductLayout& P) {
    tangent_layout(dims, T, 1, wgrad_form, P.G);
    P.cot = P.G.total;
    P.part = P.cot + round256(P.G.L.nl * (size_t)T * 4);
    P.total = P.part + obs_part_bytes(dims.B, n_obs);
}

// bytes: the product's layout | z_pred [B][T][n] | grad_z0_bg | g | x | r | p | hp, [B][n] each | rs, rs0, vhv: [B] doubles each
struct GnStepLayout { GnProductLayout P; size_t z_pred = 0, gbg = 0, vec = 0, nv = 0, scal = 0, ns = 0, total = 0; };
void gn_step_layout(const TrainPlan& dims, int T, int n_obs, int wgrad_form, GnStepLayout& S) {
    gn_product_layout(dims, T, n_obs, wgrad_form, S.P);
    S.nv = round256(S.P.G.L.nl * 4);
    S.ns = round256((size_t)dims.B * 8);
    S.z_pred = S.P.total;
    S.gbg = S.z_pred + round256(S.P.G.L.nl * (size_t)T * 4);
    S.vec = S.gbg + S.nv;
    S.scal = S.vec + 5 * S.nv;
    S.total = S.scal + 3 * S.ns;
}

// What the product and the step refuse about the problem itself, in include/lns.h's order (after the null checks, which are
// the caller's): no propagator, B, the latent size, the observation table, T, the damping.  T_given < 0: T follows the table.
struct GnProblem { TrainPlan dims; int64_t n = 0; int T = 0; ObsTable tb; GnTable gt; };
int gn_problem(lns_engine* e, const char* who, int B, int H, int W, int T_given, int n_obs, const int* steps, const double* weight,
               double lambda, double mu, bool has_bg, GnProblem& q) {
    if (e->cfg.prop_kind != LNS_PROP_PLAIN && e->cfg.prop_kind != LNS_PROP_CONDITIONAL) { e->err = fmt("%s: engine has no propagator", who); return LNS_ESTATE; }
    if (B < 1) { e->err = fmt("%s: B must be >= 1", who); return LNS_EINVAL; }
    if (int brc = check_batch(e, B)) return brc;
    int rc;
    if ((rc = train_plan_dims(e, B, H, W, q.dims))) return rc;
    q.n = (int64_t)q.dims.c * H * W;
    if ((int64_t)B * q.n >= (int64_t)1 << 31) { e->err = fmt("%s: a latent batch has 2^31 or more elements", who); return LNS_EINVAL; }
    if ((rc = obs_table(n_obs, steps, weight, -1, q.n, lambda, has_bg, q.tb, e->err))) return rc;
    q.T = steps[n_obs - 1] + 1;
    if (T_given >= 0 && T_given != q.T) {
        e->err = fmt("%s: T must be the last observed step + 1 = %d, got %d (the cotangent has grad_z_pred's layout)", who, q.T, T_given);
        return LNS_EINVAL;
    }
    if (!(mu >= 0.0) || !std::isfinite(mu)) { e->err = fmt("%s: damping must be finite and >= 0", who); return LNS_EINVAL; }
    GnTable& g = q.gt;
    memset(&g, 0, sizeof g);
    g.n_obs = n_obs;
    for (int k = 0; k < n_obs; ++k) {
        g.steps[k] = q.tb.steps[k]; g.coef[k] = q.tb.coef[k];
        g.cw[k] = 2.0 * q.tb.weight[k] / (double)q.n;               // the double that coef[k] is rounded from
    }
    g.cd = 2.0 * lambda / (double)q.n + mu;
    g.c_d = (float)g.cd;
    return LNS_OK;
}

// the product's launches; every check has been made
int gn_product_enqueue(lns_engine* e, const float* const* params, const float* z_in, const float* z_pred, int B, int H, int W,
                       const GnProblem& q, const float* v, float* hv, double* vhv, void* ws, const GnProductLayout& P, int device,
                       void* stream) {
    DeviceGuard dg(device);
    char* base = static_cast<char*>(ws);
    float* zt = reinterpret_cast<float*>(base + P.G.z);               // the workspace's latent tangent: v is not modified
    float* cot = reinterpret_cast<float*>(base + P.cot);
    double* part = reinterpret_cast<double*>(base + P.part);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long n = (long)q.n;
    int rc;
    HIPCHK(e, launch_add_rows(v, n, nullptr, 0, zt, n, B, n, s));
    if ((rc = lns_train_tangent(e, params, B, H, W, q.T, 1, 0, q.T, zt, cot, ws, P.G.total, stream))) return rc;
    HIPCHK(e, launch_gn_weight(q.gt, cot, v, B, q.T, n, part, s));
    if ((rc = lns_train_backward_ex(e, params, z_in, z_pred, cot, B, H, W, q.T, nullptr, hv, ws, P.G.scratch, stream, nullptr))) return rc;
    HIPCHK(e, launch_gn_finish(q.gt, part, hv, v, B, n, vhv, s));
    return LNS_OK;
}

int cg_check(const char* who, int B, int64_t n, std::string& err) {
    if (B < 1 || B > LNS_MAX_BATCH) { err = fmt("%s: B must be in 1 .. %d", who, LNS_MAX_BATCH); return LNS_EINVAL; }
    if (n < 1 || n >= (int64_t)1 << 31) { err = fmt("%s: n must be in 1 .. 2^31 - 1", who); return LNS_EINVAL; }
    return LNS_OK;
}

}  // namespace

int lns_train_gn_product_workspace_bytes(lns_engine* e, int B, int H, int W, int T, int n_obs, size_t* bytes) {
    if (!e) return LNS_EINVAL;
    if (!bytes) { e->err = "gn product: bytes is null"; return LNS_EINVAL; }
    if (e->cfg.prop_kind != LNS_PROP_PLAIN && e->cfg.prop_kind != LNS_PROP_CONDITIONAL) { e->err = "gn product: engine has no propagator"; return LNS_ESTATE; }
    if (B < 1) { e->err = "gn product: B must be >= 1"; return LNS_EINVAL; }
    if (int brc = check_batch(e, B)) return brc;
    if (T < 1) { e->err = "gn product: T must be >= 1"; return LNS_EINVAL; }
    if (n_obs < 1 || n_obs > OBS_MAX) { e->err = fmt("gn product: n_obs must be in 1 .. %d, got %d", OBS_MAX, n_obs); return LNS_EINVAL; }
    TrainPlan dims;
    if (int rc = train_plan_dims(e, B, H, W, dims)) return rc;
    GnProductLayout P;
    gn_product_layout(dims, T, n_obs, e->opt_train_wgrad, P);
    *bytes = P.total;
    return LNS_OK;
}

int lns_train_gn_product(lns_engine* e, const float* const* params, const float* z_in, const float* z_pred, int B, int H, int W, int T,
                         int n_obs, const int* obs_steps, const double* obs_weight, double background, double damping, const float* v,
                         float* hv, double* vhv, void* ws, size_t ws_bytes, void* stream) {
    if (!e) return LNS_EINVAL;
    if (!params) { e->err = "gn product: params array is null"; return LNS_EINVAL; }
    if (!z_in || !z_pred) { e->err = "gn product: z_in / z_pred is null"; return LNS_EINVAL; }
    if (!v || !hv) { e->err = "gn product: v / hv is null"; return LNS_EINVAL; }
    if (v == hv) { e->err = "gn product: hv must not be v"; return LNS_EINVAL; }
    GnProblem q;
    int rc, device = -1;
    if ((rc = gn_problem(e, "gn product", B, H, W, T, n_obs, obs_steps, obs_weight, background, damping, false, q))) return rc;
    const PropParams* pp;
    if ((rc = prop_params(e, &pp)) || (rc = check_params(e, *pp, params, "parameter"))) return rc;
    GnProductLayout P;
    gn_product_layout(q.dims, q.T, n_obs, e->opt_train_wgrad, P);
    if (!ws || ws_bytes < P.total) { e->err = fmt("gn product workspace too small: need %zu bytes", P.total); return LNS_ENOMEM; }
    // ---- where the tensors live (pointer attributes: the first HIP calls), still before anything is enqueued ----
    if ((rc = train_device_of(e, z_in, &device)) || (rc = train_same_device(e, device, z_pred, "z_pred")) ||
        (rc = train_same_device(e, device, v, "v")) || (rc = train_same_device(e, device, hv, "hv")) ||
        (rc = train_same_device(e, device, vhv, "vhv")) || (rc = train_same_device(e, device, ws, "the workspace"))) return rc;
    return gn_product_enqueue(e, params, z_in, z_pred, B, H, W, q, v, hv, vhv, ws, P, device, stream);
}

int lns_op_cg_start(const float* g, float* x, float* r, float* p, int B, int64_t n, double* rs, double* rs0, void* stream) {
    std::string& err = g_create_error;
    if (!g || !x || !r || !p) { err = "cg start: g / x / r / p is null"; return LNS_EINVAL; }
    if (!rs || !rs0) { err = "cg start: rs / rs0 is null"; return LNS_EINVAL; }
    if (int rc = cg_check("cg start", B, n, err)) return rc;
    const hipError_t rc = launch_cg_start(g, x, r, p, B, (long)n, rs, rs0, static_cast<hipStream_t>(stream));
    if (rc != hipSuccess) { err = std::string("cg start: ") + hipGetErrorString(rc); return LNS_EHIP; }
    return LNS_OK;
}

int lns_op_cg_update(float* x, float* r, float* p, const float* hp, const double* php, int B, int64_t n, double tol, double* rs,
                     const double* rs0, int32_t* applied, void* stream) {
    std::string& err = g_create_error;
    if (!x || !r || !p || !hp) { err = "cg update: x / r / p / hp is null"; return LNS_EINVAL; }
    if (!rs || !rs0) { err = "cg update: rs / rs0 is null"; return LNS_EINVAL; }
    if (int rc = cg_check("cg update", B, n, err)) return rc;
    if (!(tol >= 0.0) || !std::isfinite(tol)) { err = "cg update: tol must be finite and >= 0"; return LNS_EINVAL; }
    const hipError_t rc = launch_cg_update(x, r, p, hp, php, B, (long)n, tol * tol, rs, rs0, applied, static_cast<hipStream_t>(stream));
    if (rc != hipSuccess) { err = std::string("cg update: ") + hipGetErrorString(rc); return LNS_EHIP; }
    return LNS_OK;
}

int lns_fit_gn_step_workspace_bytes(lns_engine* e, int B, int H, int W, int T, int n_obs, size_t* bytes) {
    if (!e) return LNS_EINVAL;
    if (!bytes) { e->err = "gn step: bytes is null"; return LNS_EINVAL; }
    if (e->cfg.prop_kind != LNS_PROP_PLAIN && e->cfg.prop_kind != LNS_PROP_CONDITIONAL) { e->err = "gn step: engine has no propagator"; return LNS_ESTATE; }
    if (B < 1) { e->err = "gn step: B must be >= 1"; return LNS_EINVAL; }
    if (int brc = check_batch(e, B)) return brc;
    if (T < 1) { e->err = "gn step: T must be >= 1"; return LNS_EINVAL; }
    if (n_obs < 1 || n_obs > OBS_MAX) { e->err = fmt("gn step: n_obs must be in 1 .. %d, got %d", OBS_MAX, n_obs); return LNS_EINVAL; }
    TrainPlan dims;
    if (int rc = train_plan_dims(e, B, H, W, dims)) return rc;
    GnStepLayout S;
    gn_step_layout(dims, T, n_obs, e->opt_train_wgrad, S);
    *bytes = S.total;
    return prebuild_train_plan(e, B, H, W);
}

int lns_fit_gn_step(lns_engine* e, const float* const* params, float* z0, const float* param, const float* obs, const float* z_background,
                    int B, int H, int W, const lns_gn_spec* spec, float* loss, float* per, float* cg_resid, int32_t* applied, void* ws,
                    size_t ws_bytes, void* stream) {
    if (!e) return LNS_EINVAL;
    // ---- host-only checks ----
    const bool cond = e->cfg.prop_kind == LNS_PROP_CONDITIONAL;
    if (e->cfg.prop_kind != LNS_PROP_PLAIN && !cond) { e->err = "gn step: engine has no propagator"; return LNS_ESTATE; }
    if (!spec || spec->size != sizeof(lns_gn_spec)) { e->err = "gn step: spec is null or its size field is not sizeof(lns_gn_spec)"; return LNS_EINVAL; }
    if (spec->flags != 0) { e->err = fmt("gn step: flags 0x%x: must be 0", spec->flags); return LNS_EINVAL; }
    if (spec->n_cg < 1 || spec->n_cg > LNS_GN_CG_MAX) { e->err = fmt("gn step: n_cg must be in 1 .. %d, got %d", LNS_GN_CG_MAX, spec->n_cg); return LNS_EINVAL; }
    if (!(spec->cg_tol >= 0.0) || !std::isfinite(spec->cg_tol)) { e->err = "gn step: cg_tol must be finite and >= 0"; return LNS_EINVAL; }
    if (!params) { e->err = "gn step: params array is null"; return LNS_EINVAL; }
    if (!z0 || !obs) { e->err = "gn step: z0 / obs is null"; return LNS_EINVAL; }
    if (cond && !param) { e->err = "gn step: conditional propagator needs param"; return LNS_EINVAL; }
    if (!loss) { e->err = "gn step: loss is null"; return LNS_EINVAL; }
    const bool has_bg = z_background != nullptr;
    if (!has_bg && spec->background > 0.0) { e->err = "gn step: background > 0 needs z_background"; return LNS_EINVAL; }
    GnProblem q;
    int rc;
    if ((rc = gn_problem(e, "gn step", B, H, W, -1, spec->n_obs, spec->obs_steps, spec->obs_weight, spec->background, spec->damping,
                         has_bg, q))) return rc;
    const PropParams* pp;
    if ((rc = prop_params(e, &pp)) || (rc = check_params(e, *pp, params, "parameter"))) return rc;
    GnStepLayout S;
    gn_step_layout(q.dims, q.T, spec->n_obs, e->opt_train_wgrad, S);
    if (!ws || ws_bytes < S.total) { e->err = fmt("gn step workspace too small: need %zu bytes", S.total); return LNS_ENOMEM; }
    // ---- where the tensors live (pointer attributes: the first HIP calls), still before anything is enqueued ----
    int device = -1;
    if ((rc = train_device_of(e, z0, &device)) || (rc = train_same_device(e, device, obs, "obs")) ||
        (rc = train_same_device(e, device, z_background, "z_background")) || (rc = train_same_device(e, device, loss, "loss")) ||
        (rc = train_same_device(e, device, per, "per")) || (rc = train_same_device(e, device, cg_resid, "cg_resid")) ||
        (rc = train_same_device(e, device, applied, "applied")) || (rc = train_same_device(e, device, ws, "the workspace"))) return rc;
    // ---- device work, in stream order ----
    char* base = static_cast<char*>(ws);
    auto vec = [&](int i) { return reinterpret_cast<float*>(base + S.vec + (size_t)i * S.nv); };
    auto scal = [&](int i) { return reinterpret_cast<double*>(base + S.scal + (size_t)i * S.ns); };
    float* z_pred = reinterpret_cast<float*>(base + S.z_pred);
    float* cot = reinterpret_cast<float*>(base + S.P.cot);            // first dL/dz_pred, then every product's cotangent
    double* part = reinterpret_cast<double*>(base + S.P.part);
    float* gbg = has_bg ? reinterpret_cast<float*>(base + S.gbg) : nullptr;
    float *g = vec(0), *x = vec(1), *r = vec(2), *p = vec(3), *hp = vec(4);
    double *rs = scal(0), *rs0 = scal(1), *vhv = scal(2);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long n = (long)q.n, Bn = (long)B * n;
    if ((rc = lns_train_forward(e, params, z0, param, B, H, W, q.T, z_pred, ws, S.P.G.scratch, stream))) return rc;
    DeviceGuard dg(device);
    HIPCHK(e, launch_obs_mse(q.tb, z_pred, obs, has_bg ? z0 : nullptr, z_background, B, q.T, n, per, loss, cot, gbg, part, s));
    if ((rc = lns_train_backward_ex(e, params, z0, z_pred, cot, B, H, W, q.T, nullptr, g, ws, S.P.G.scratch, stream, nullptr))) return rc;
    if (gbg) HIPCHK(e, launch_add(g, gbg, g, Bn, s));                  // g = grad_z_in + grad_z0_bg, on its own
    if (applied) HIPCHK(e, hipMemsetAsync(applied, 0, (size_t)B * 4, s));
    HIPCHK(e, launch_cg_start(g, x, r, p, B, n, rs, rs0, s));
    const double tol2 = spec->cg_tol * spec->cg_tol;
    for (int it = 0; it < spec->n_cg; ++it) {
        if ((rc = gn_product_enqueue(e, params, z0, z_pred, B, H, W, q, p, hp, vhv, ws, S.P, device, stream))) return rc;
        HIPCHK(e, launch_cg_update(x, r, p, hp, vhv, B, n, tol2, rs, rs0, applied, s));
    }
    HIPCHK(e, launch_add(z0, x, z0, Bn, s));
    if (cg_resid) HIPCHK(e, launch_cg_resid(rs, rs0, B, cg_resid, s));
    return LNS_OK;
}
