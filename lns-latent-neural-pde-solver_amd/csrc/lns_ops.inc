// ---------------------------------------------------------------------------------------------------------------------
// The planner-independent entry points: lns_op_*, lns_metric_rel_l2*, lns_fourier_block_*  (included by lns_engine.cpp,
// inside its extern "C" region: they use that file's static helpers)
//
// A new lns_op_* follows one shape: every check first, each refusal through op_refuse (or a helper that calls it), no HIP
// call before the last of them; then an OpScratch (lns_op_scratch.h) for the device memory of the call; then the launches,
// each `if (sc.ok()) sc.note(launch_...)`; then `OPCHK(sc.finish(s)); return LNS_OK;`.  No hipMalloc / hipFree here.
// ---------------------------------------------------------------------------------------------------------------------
#define OPCHK(call)                                                                                   \
    do { hipError_t err__ = (call);                                                                   \
         if (err__ != hipSuccess) { fprintf(stderr, "lns_op: %s: %s\n", #call, hipGetErrorString(err__)); return LNS_EHIP; } } while (0)

// an entry point's refusal, under the op's name
static int op_refuse(const char* op, const std::string& m) { g_create_error = std::string(op) + ": " + m; return LNS_EINVAL; }

// a conv launch prepared from host weights (device buffers owned by the struct, freed with it)
struct OpConv {
    ConvArgs a;
    int variant = -1;
    OpScratch mem;                 // owns the three below
    float* dw = nullptr;
    int* dmaps = nullptr;
    unsigned* damax = nullptr;     // [B] running max |x| of the input (dynamic activation scale of the split kernels)
    bool defer_amax = false;       // op_conv_prepare launches nothing: the caller runs op_conv_amax after its own checks
    void release() { mem.release(); dw = nullptr; dmaps = nullptr; damax = nullptr; }     // before preparing again
};

static int op_conv_prepare(OpConv& oc, const float* x, int B, int Cin, int Hin, int Win, int Hv, int Wv,
                           const float* w_host, const float* bias_host, int Cout, int ksize, int stride, int dilation,
                           int pad_t, int pad_b, int pad_l, int pad_r, int mode_y, int mode_x, const float* ss, int act_in,
                           int act_out, const float* residual, const float* badd, float* y, int tile_variant, hipStream_t stream) {
    if (!x || !w_host || !y || (ksize != 1 && ksize != 3)) return LNS_EINVAL;
    if (act_in != ACT_NONE && act_in != ACT_SWISH) return LNS_EINVAL;   // prologue: GroupNorm scale/shift + Swish only
    OPCHK(init_kernels());
    // test code: tensor layouts in the high bits of tile_variant (>= 0 only): 0x100 = x is OCT8 ([Cin/8][H*W][8] per sample),
    // 0x200 = y and the residual are OCT8 (include/lns.h)
    const int layout = tile_variant >= 0 ? (tile_variant & 0x300) : 0;
    if (tile_variant >= 0) tile_variant &= 0xff;
    const bool stationary = tile_variant == 8;      // test code: 1x1 bf16x3 kernel in its input-stationary form
    if (stationary) tile_variant = CV_B1;
    const bool w8 = tile_variant == 19;             // test code: f16x2 3x3 kernel in its 8-wave form (conv3_w8.inc)
    const bool forced = tile_variant >= 0;
    if (w8) tile_variant = CV_F64;
    const bool up2r = tile_variant == 18;           // test code: ... its resident-patch form (conv3_up2r.inc)
    const bool up2q = tile_variant == 20;           // test code: ... its quad-phase form (conv3_up2q.inc)
    const bool up2d = tile_variant == 21;           // ... its dual-phase form (conv3_up2d.inc): the planner's form where it fits
    const bool up2 = tile_variant == 17 || up2r || up2q || up2d;    // test code: f16x2 3x3 kernel, phase form of an exactly-2x nearest upsample
    if (up2) {
        if (ksize != 3 || stride != 1 || dilation != 1 || Hv != 2 * Hin || Wv != 2 * Win || pad_t != 1 || pad_b != 1 || pad_l != 1 || pad_r != 1) return LNS_EINVAL;
        tile_variant = CV_F64; Hv = Hin; Wv = Win;
    }
    ConvPadded pk = conv_padded_sizes(ksize, Cin, Cout);
    if (tile_variant >= 0) {
        const int TM = conv_variant_info(tile_variant).TM;
        pk.Cout_pad = (Cout + TM - 1) / TM * TM;
        if (pk.Cout_pad < 32) pk.Cout_pad = 32;
    }
    if (Hv <= 0) Hv = Hin;
    if (Wv <= 0) Wv = Win;
    const int pad[4] = {pad_t, pad_b, pad_l, pad_r};
    ConvGeom g;
    if (!conv_geometry(g, B, Cout, Hv, Wv, ksize, stride, dilation, pad, pk.kc_log2, pk.Cout_pad, tile_variant, false, false, 1 << 30, false,
                       false, up2q ? 4 : -1)) return LNS_EINVAL;
    std::vector<int> rm, cm;
    if (up2) { g.Hout = 2 * Hin; g.Wout = 2 * Win; }
    const float sch = (Hv == 2 * Hin) ? 0.5f : 0.0f, scw = (Wv == 2 * Win) ? 0.5f : 0.0f;
    conv_tile_maps(rm, cm, g, stride, Hin, Win, Hv, Wv, sch, scw, pad, mode_y, mode_x);
    const size_t wcount = (size_t)ksize * ksize * pk.Cin_pad * pk.Cout_pad;
    std::vector<float> hw(wcount + pk.Cout_pad, 0.0f);
    pack_conv_weight(hw.data(), w_host, 0, Cout, Cin, ksize, pk.Cin_pad, pk.Cout_pad);
    if (bias_host) memcpy(hw.data() + wcount, bias_host, (size_t)Cout * 4);
    float wscale = 1.0f;
    if (cv_is_f16x2_3x3(g.variant) || (g.variant == CV_B1 && convb1_is_f16())) {
        float mx = 0.0f;
        for (size_t i = 0; i < (size_t)Cout * Cin * ksize * ksize; ++i) mx = std::max(mx, fabsf(w_host[i]));
        if (mx > 0.0f) wscale = conv_f16_weight_scale(mx);
        if (up2) wscale *= 0.25f;
    }
    const size_t wb_floats = up2 ? convu_weight_bytes(Cout, pk.Cin_pad) / 4 : cv_is_split_3x3(g.variant) ? convb_weight_bytes(Cout, pk.Cin_pad) / 4
                           : g.variant == CV_B1 ? convb1_weight_bytes(Cout, pk.Cin_pad) / 4 : 0;
    if (wb_floats) {
        hw.resize(hw.size() + wb_floats, 0.0f);
        if (up2) convu_pack_weight(hw.data() + wcount + pk.Cout_pad, w_host, 0, Cout, Cin, pk.Cin_pad, wscale);
        else if (cv_is_f16x2_3x3(g.variant)) convf_pack_weight(hw.data() + wcount + pk.Cout_pad, w_host, 0, Cout, Cin, pk.Cin_pad, wscale);
        else if (g.variant != CV_B1) convb_pack_weight(hw.data() + wcount + pk.Cout_pad, w_host, 0, Cout, Cin, pk.Cin_pad);
        else convb1_pack_weight(hw.data() + wcount + pk.Cout_pad, w_host, 0, Cout, Cin, pk.Cin_pad, wscale);
    }
    OpScratch& mem = oc.mem;       // (an early return below leaves the buffers to oc)
    oc.dw = static_cast<float*>(mem.alloc(hw.size()));
    oc.dmaps = static_cast<int*>(mem.alloc(rm.size() + cm.size()));
    OPCHK(mem.err);
    mem.copy_in(oc.dw, hw.data(), hw.size());
    mem.copy_in(oc.dmaps, rm.data(), rm.size());
    mem.copy_in(oc.dmaps + rm.size(), cm.data(), cm.size());
    OPCHK(mem.err);
    ConvArgs& a = oc.a;
    memset(&a, 0, sizeof a);
    conv_set_geometry(a, g, B, Cin, Hin, Win, Cout, ksize, stride, dilation, pk.Cin_pad, pk.Cout_pad);
    a.x = x; a.y = y;
    a.w = oc.dw; a.bias = bias_host ? oc.dw + wcount : nullptr; a.ss = ss; a.act_in = act_in; a.act_out = act_out;
    if (wb_floats) a.wb = oc.dw + wcount + pk.Cout_pad;
    a.rowmap = oc.dmaps; a.colmap = oc.dmaps + rm.size();
    conv_set_map_arith(a, g.variant, ksize, Hin, Win, Hv, Wv, pad, mode_y, mode_x);
    a.res = residual; a.res_bs = a.y_bs; a.badd = badd;
    a.unscale = conv_unscale(g.variant, wscale);
    a.up2 = up2 ? 1 : 0;
    // the input's per-sample maximum, as the producing kernel of a plan would have recorded it
    oc.damax = static_cast<unsigned*>(mem.alloc((size_t)B * LNS_AMAX_SUB));
    // (on the CALLER's stream: x may still be being produced there, and a non-blocking stream does not order with the
    //  null stream -- a maximum taken too early would give a scale that overflows fp16)
    if (!oc.defer_amax) {
        mem.fill(oc.damax, 0, (size_t)B * LNS_AMAX_SUB, stream);
        if (mem.ok()) mem.note(launch_amax(x, a.x_bs, (long)Cin * Hin * Win, B, oc.damax, stream));
    }
    OPCHK(mem.err);
    a.amax_in = oc.damax;
    if (up2r) {
        a.up2 = 2;
        if (!convur_fits(a)) return LNS_EINVAL;
    }
    if (up2q) {
        a.up2 = 3;
        if (!convuq_fits(a)) return LNS_EINVAL;
    }
    a.w8 = w8 ? 1 : (forced ? -1 : 0);              // a forced tile variant means that kernel
    a.x_oct = (layout & 0x100) ? 1 : 0; a.y_oct = (layout & 0x200) ? 1 : 0;
    if ((a.x_oct && (Cin & 7)) || (a.y_oct && (Cout & 7))) return LNS_EINVAL;
    if (up2d) {
        if (!convud_fits(a)) return LNS_EINVAL;
        a.up2 = 4;
    }
    if (stationary) {
        if (pk.Cin_pad > 64) return LNS_EINVAL;
        a.ct_per_block = g.cout_tiles < 3 ? g.cout_tiles : 3;
    }
    oc.variant = g.variant;
    return LNS_OK;
}

int lns_op_conv2d(const float* x, int B, int Cin, int Hin, int Win, int Hv, int Wv, const float* w_host,
                  const float* bias_host, int Cout, int ksize, int stride, int dilation, int pad_t, int pad_b, int pad_l,
                  int pad_r, int mode_y, int mode_x, const float* ss, int act_in, int act_out, const float* residual,
                  const float* badd, float* y, int tile_variant, void* stream, unsigned* amax_out) {
    OpConv oc;
    const int rc = op_conv_prepare(oc, x, B, Cin, Hin, Win, Hv, Wv, w_host, bias_host, Cout, ksize, stride, dilation, pad_t,
                                   pad_b, pad_l, pad_r, mode_y, mode_x, ss, act_in, act_out, residual, badd, y, tile_variant,
                                   static_cast<hipStream_t>(stream));
    if (rc) return rc;
    oc.a.amax_out = amax_out;
    hipStream_t s = static_cast<hipStream_t>(stream);
#ifdef LNS_TS
    // diagnostic build: per-block phase timestamps of the split-operand kernels, appended to $LNS_TS_FILE
    // (an upper bound for the input-stationary 1x1 form; the phase forms of the upsampling conv: four / two blocks per source tile)
    const long nblk = (long)oc.a.tiles_x * oc.a.tiles_y * oc.a.cout_tiles * oc.a.B * (oc.a.up2 == 1 ? 4 : oc.a.up2 == 4 ? 2 : 1);
    hipError_t lrc = hipSuccess;
    if ((cv_is_split_3x3(oc.variant) || oc.variant == CV_B1) &&
        ts_capture(nblk, 8, fmt("# launch B=%d Cin=%d Cout=%d H=%d W=%d blocks=%ld", B, Cin, Cout, Hv, Wv, nblk), s, lrc,
                   [&](long long* ts) { oc.a.dbg_ts = ts; return launch_conv(oc.variant, oc.a, s); })) {
        OPCHK(lrc);
        return LNS_OK;
    }
#endif
    oc.mem.note(launch_conv(oc.variant, oc.a, s));
    OPCHK(oc.mem.finish(s));
    return LNS_OK;
}

// GroupNorm from the tile statistics of its producer (include/lns.h): producer convolution with ConvArgs::stat_part set by
// gn_tile_rule, then the finalize kernel and / or a consumer convolution whose prologue merges the partials (conv_fold_gn,
// gn_output_bound: the planner's calls).  Nothing is launched before the last check.
int lns_op_conv_gn(const lns_conv_gn_args* p, void* stream) {
    if (!p) return op_refuse("conv_gn", "args is null");
    if (!p->x || !p->w_host || !p->y) return op_refuse("conv_gn", "x / w_host / y is null");
    if (p->B < 1 || p->B > LNS_MAX_BATCH || p->Cout < 1 || p->groups < 1 || p->Cout % p->groups != 0)
        return op_refuse("conv_gn", "B in 1..65535, groups a divisor of Cout");
    if (!(p->eps > 0.0f) || !std::isfinite(p->eps)) return op_refuse("conv_gn", "eps must be positive and finite");
    const bool consumer = p->w2_host != nullptr;
    if (consumer && (!p->y2 || p->Cout2 < 1 || (p->ksize2 != 1 && p->ksize2 != 3)))
        return op_refuse("conv_gn", "the consumer needs y2, Cout2 >= 1, ksize2 1 or 3");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int B = p->B, C = p->Cout;
    OpConv prod, cons;
    prod.defer_amax = cons.defer_amax = true;
    int rc = op_conv_prepare(prod, p->x, B, p->Cin, p->Hin, p->Win, p->Hv, p->Wv, p->w_host, p->bias_host, C, p->ksize, p->stride,
                             p->dilation, p->pad_t, p->pad_b, p->pad_l, p->pad_r, p->mode_y, p->mode_x, p->ss, p->act_in, p->act_out,
                             p->residual, p->badd, p->y, p->tile_variant, s);
    if (rc) return rc == LNS_EINVAL ? op_refuse("conv_gn", "no such producer convolution (lns_op_conv2d's rules)") : rc;
    const int H = prod.a.Hout, W = prod.a.Wout;
    if (prod.a.up2 == 2 || prod.a.up2 == 3 || prod.a.w8 == 1) return op_refuse("conv_gn", "the experimental producer forms are not covered");
    GnTileRule r;
    if (!gn_tile_rule(r, prod.a, prod.variant, H, W, p->groups, p->premul != nullptr, B, ~(size_t)0))
        return op_refuse("conv_gn",
                         fmt("the planner attaches no tile statistics to this producer (variant %d%s%s, %d x %d plane, %d x %d tiles%s): "
                             "split-operand 3x3 / streaming 1x1 kernels, exact tiles from 256 pixels, ragged tiles without upsampling",
                             prod.variant, prod.a.up2 ? ", upsampling" : "", prod.a.ct_per_block ? ", input-stationary" : "", H, W,
                             prod.a.tiles_x, prod.a.tiles_y, p->premul ? ", premul" : ""));
    if (consumer) {
        if (!r.foldable)
            return op_refuse("conv_gn",
                             fmt("the rule does not fold this merge into a consumer (%d partials, %d channels in %d groups%s): at most "
                                 "2 partials of exact tiles or one ragged tile, <= 512 channels, premul with one group only, channels "
                                 "per group a power of two <= 64", r.tiles, C, p->groups, p->premul ? ", premul" : ""));
        const int v2 = p->variant2 & 0xff;
        if (p->variant2 < 0 || (p->variant2 & ~0x1ff) || !(v2 == CV_F64 || v2 == CV_F32 || v2 == CV_B1) || (v2 == CV_B1) != (p->ksize2 == 1))
            return op_refuse("conv_gn", "consumer: variant2 11 / 13 with ksize2 3, or 7 with ksize2 1");
        if (((p->variant2 & 0x100) != 0) != (prod.a.y_oct != 0))
            return op_refuse("conv_gn", "consumer: variant2 | 0x100 exactly when the producer stores OCT8");
        if (prod.a.y_oct && v2 == CV_B1) return op_refuse("conv_gn", "consumer: the 1x1 kernel reads planar tensors, the producer stores OCT8");
        const int pd = p->ksize2 / 2;
        rc = op_conv_prepare(cons, p->y, B, C, H, W, H, W, p->w2_host, p->bias2_host, p->Cout2, p->ksize2, 1, 1, pd, pd, pd, pd,
                             p->mode_y, p->mode_x, nullptr, p->act_in2, ACT_NONE, nullptr, nullptr, p->y2, p->variant2, s);
        if (rc) return rc == LNS_EINVAL ? op_refuse("conv_gn", "no such consumer convolution (lns_op_conv2d's rules)") : rc;
        if (cons.variant != v2 || cons.a.ct_per_block) return op_refuse("conv_gn", "consumer: not the requested kernel form");
    }
    // ---- every check is done ----
    const size_t npart = (size_t)B * r.tiles * C * 2;
    OpScratch sc;
    float* dbuf = static_cast<float*>(sc.alloc(npart + 2 * (size_t)C));     // partials [B][tiles][C][2], gamma [C], beta [C]
    OPCHK(sc.err);                              // (nothing is on the stream yet)
    float *dpart = dbuf, *dgamma = p->gamma_host ? dbuf + npart : nullptr, *dbeta = p->beta_host ? dbuf + npart + C : nullptr;
    if (dgamma) sc.copy_in(dgamma, p->gamma_host, C);
    if (dbeta) sc.copy_in(dbeta, p->beta_host, C);
    if (p->geom) {
        const int g8[8] = {prod.a.tiles_x, prod.a.tiles_y, prod.a.bw_log2, prod.a.ks == 1 ? 1 : 0, prod.a.up2 ? 4 : 1, r.mode, r.foldable ? 1 : 0, r.tiles};
        memcpy(p->geom, g8, sizeof g8);
    }
    // an entry the epilogue does not write stays NaN
    sc.fill(dpart, 0xFF, npart, s);
    sc.fill(prod.damax, 0, (size_t)B * LNS_AMAX_SUB, s);
    if (sc.ok()) sc.note(launch_amax(p->x, prod.a.x_bs, prod.a.x_bs, B, prod.damax, s));
    prod.a.stat_part = dpart; prod.a.stat_count = r.stat_count;
    if (sc.ok()) sc.note(launch_conv(prod.variant, prod.a, s));
    if (p->part_out && sc.ok()) sc.note(hipMemcpyAsync(p->part_out, dpart, npart * 4, hipMemcpyDeviceToDevice, s));
    const float* merge = p->part_in ? p->part_in : dpart;
    if (p->ss_out && sc.ok()) {
        GnStatsArgs g;
        memset(&g, 0, sizeof g);
        g.C = C; g.HW = H * W; g.groups = p->groups; g.eps = p->eps; g.gamma = dgamma; g.beta = dbeta; g.premul = p->premul;
        g.ss = p->ss_out; g.B = B;
        sc.note(launch_gn_tile_finalize(g, merge, r.tiles, r.gn_count < 0 ? 0 : r.gn_count, r.geom, s));
    }
    if (consumer && sc.ok()) {
        ConvArgs& a = cons.a;
        conv_fold_gn(a, merge, r.tiles, r.gn_count, p->groups, p->eps, p->premul, dgamma, dbeta);
        float gmax = p->gamma_host ? 0.0f : 1.0f, bmax = 0.0f;
        for (int c = 0; c < C; ++c) {
            if (p->gamma_host) gmax = std::max(gmax, fabsf(p->gamma_host[c]));
            if (p->beta_host) bmax = std::max(bmax, fabsf(p->beta_host[c]));
        }
        conv_set_final_bound(a, gn_output_bound(gmax, bmax, C / p->groups, H, W));
        sc.note(launch_conv(cons.variant, a, s));
    }
    OPCHK(sc.finish(s));
    return LNS_OK;
}

// Diagnostic: two convolutions launched repeatedly on two streams (so their workgroups share CUs), each
// compared bit for bit with the result it gives alone.  A: ksize_a x ksize_a, B: ksize_b x ksize_b, both on
// [B, C, H, W] inputs with a GroupNorm+Swish prologue; variants as in lns_op_conv2d (-1 = automatic fp32).
int lns_op_conv_pair_stress(int B, int H, int W, int cin_a, int cout_a, int ksize_a, int variant_a, int cin_b, int cout_b,
                            int ksize_b, int variant_b, int rounds, int launches, long long* mismatches_a,
                            long long* mismatches_b) {
    // (members are destroyed last to first: the conv's buffers and x / y / ss are freed, which waits for the device, then the stream)
    struct Side {
        hipStream_t st = nullptr; OpScratch mem; OpConv oc; float *x = nullptr, *y = nullptr, *ss = nullptr;
        std::vector<float> ref, out, hx, hw, hs; size_t ny = 0;
        ~Side() { if (st) (void)hipStreamDestroy(st); }
    };
    bool dumped = false;
    Side S[2];
    const int cin[2] = {cin_a, cin_b}, cout[2] = {cout_a, cout_b}, ks[2] = {ksize_a, ksize_b}, var[2] = {variant_a, variant_b};
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (float)((seed >> 40) & 0xFFFF) / 32768.0f - 1.0f; };
    for (int i = 0; i < 2; ++i) OPCHK(hipStreamCreateWithFlags(&S[i].st, hipStreamNonBlocking));
    hipStream_t st[2] = {S[0].st, S[1].st};
    for (int i = 0; i < 2; ++i) {
        Side& s = S[i];
        const size_t nx = (size_t)B * cin[i] * H * W;
        s.ny = (size_t)B * cout[i] * H * W;
        std::vector<float>&hx = s.hx, &hw = s.hw, &hs = s.hs;
        hx.resize(nx); hw.resize((size_t)cout[i] * cin[i] * ks[i] * ks[i]); hs.resize((size_t)B * cin[i] * 2);
        for (auto& v : hx) v = rnd();
        for (auto& v : hw) v = rnd() / sqrtf((float)cin[i] * ks[i] * ks[i]);
        for (size_t k = 0; k < hs.size(); ++k) hs[k] = (k & 1) ? 0.1f * rnd() : 1.0f + 0.1f * rnd();
        s.x = static_cast<float*>(s.mem.alloc(nx));
        s.y = static_cast<float*>(s.mem.alloc(s.ny));
        s.ss = static_cast<float*>(s.mem.alloc(hs.size()));
        s.mem.copy_in(s.x, hx.data(), nx);
        s.mem.copy_in(s.ss, hs.data(), hs.size());
        OPCHK(s.mem.err);
        const int p = ks[i] / 2;
        const int rc = op_conv_prepare(s.oc, s.x, B, cin[i], H, W, H, W, hw.data(), nullptr, cout[i], ks[i], 1, 1, p, p, p, p,
                                       1, 1, s.ss, ACT_SWISH, ACT_NONE, nullptr, nullptr, s.y, var[i], st[i]);
        if (rc) return rc;
        s.ref.resize(s.ny); s.out.resize(s.ny);
        OPCHK(launch_conv(s.oc.variant, s.oc.a, st[i]));
        OPCHK(hipStreamSynchronize(st[i]));
        OPCHK(hipMemcpy(s.ref.data(), s.y, s.ny * 4, hipMemcpyDeviceToHost));
    }
    long long bad[2] = {0, 0};
    for (int r = 0; r < rounds; ++r) {
        for (int i = 0; i < 2; ++i) OPCHK(hipMemsetAsync(S[i].y, 0xFF, S[i].ny * 4, st[i]));
        for (int l = 0; l < launches; ++l)
            for (int i = 0; i < 2; ++i) OPCHK(launch_conv(S[i].oc.variant, S[i].oc.a, st[i]));
        for (int i = 0; i < 2; ++i) {
            OPCHK(hipStreamSynchronize(st[i]));
            OPCHK(hipMemcpy(S[i].out.data(), S[i].y, S[i].ny * 4, hipMemcpyDeviceToHost));
            long long nb = 0;
            for (size_t k = 0; k < S[i].ny; ++k)
                if (memcmp(&S[i].out[k], &S[i].ref[k], 4) != 0) {
                    if (nb < 6 && getenv("LNS_STRESS_VERBOSE")) {
                        const size_t hw = (size_t)H * W, per = (size_t)cout[i] * hw;
                        fprintf(stderr, "  side %c round %d: sample %zu channel %zu pixel %zu  got %.9g  want %.9g\n", 'A' + i, r,
                                k / per, (k % per) / hw, k % hw, S[i].out[k], S[i].ref[k]);
                    }
                    ++nb;
                }
            if (nb && getenv("LNS_STRESS_VERBOSE")) fprintf(stderr, "  side %c round %d: %lld words differ\n", 'A' + i, r, nb);
            if (nb && getenv("LNS_STRESS_DUMP") && !dumped) {
                dumped = true;
                const std::string d = getenv("LNS_STRESS_DUMP");
                auto put = [&](const char* nm, const void* p, size_t bytes) {
                    FILE* f = fopen((d + "/" + nm).c_str(), "wb");
                    if (f) { fwrite(p, 1, bytes, f); fclose(f); }
                };
                put("out.bin", S[i].out.data(), S[i].ny * 4);
                put("ref.bin", S[i].ref.data(), S[i].ny * 4);
                put("x.bin", S[i].hx.data(), S[i].hx.size() * 4);
                put("w.bin", S[i].hw.data(), S[i].hw.size() * 4);
                put("ss.bin", S[i].hs.data(), S[i].hs.size() * 4);
                fprintf(stderr, "  dumped side %c (B=%d C=%d->%d k=%d HW=%dx%d)\n", 'A' + i, B, cin[i], cout[i], ks[i], H, W);
            }
            bad[i] += nb;
        }
    }
    if (mismatches_a) *mismatches_a = bad[0];
    if (mismatches_b) *mismatches_b = bad[1];
    return LNS_OK;
}

// ensemble_stats_kernel on its own: frames [B][M][per] -> mean [B][per], var [B][per] (nullable)
int lns_op_ensemble_stats(const float* frames, int B, int M, int64_t per, float* mean, float* var, void* stream) {
    if (!frames || !mean) return op_refuse("ensemble_stats", "frames / mean is null");
    if (B < 1 || B > LNS_MAX_BATCH || M < 1 || M > 65536 || per < 1 || per > ((int64_t)1 << 40))
        return op_refuse("ensemble_stats", "B in 1..65535, M in 1..65536, per in 1..2^40");
    if (var && M < 2) return op_refuse("ensemble_stats", "var needs M >= 2");
    hipStream_t s = static_cast<hipStream_t>(stream);
    EnsembleStatsArgs a;
    a.frames = frames; a.mean = mean; a.var = var; a.per = (long)per; a.out_bs = (long)per; a.B = B; a.M = M; a.kk = 1;
    OPCHK(launch_ensemble_stats(a, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

// The refusals of an lns_op_*'s spec, under the op's name: null or of the wrong size, or (C given) the per-channel form for
// more than 8 channels.  An op asks twice, where its other checks stand between the two (the order is interface).
static bool op_spec_refused(const char* op, const lns_eval_spec* spec, int C = 0) {
    if (!spec || spec->size != sizeof(lns_eval_spec)) g_create_error = fmt("%s: spec is null or its size field is not sizeof(lns_eval_spec)", op);
    else if (spec->per_channel && C > LNS_METRIC_MAX_CH) g_create_error = fmt("%s: the per-channel form needs C <= 8", op);
    else return false;
    return true;
}

// The shape bounds of the ops on stored member fields [n][B][M][C][H][W], and of those on stored fields [B][T][C][H][W]
static bool op_ensemble_shape_refused(const char* op, int n, int B, int C, int H, int W) {
    if (n >= 1 && B >= 1 && B <= LNS_MAX_BATCH && C >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 30) && (int64_t)n * B * C <= 0x7fffffffLL)
        return false;
    op_refuse(op, "n >= 1, B in 1..65535, C, H, W >= 1, H * W <= 2^30, n * B * C < 2^31");
    return true;
}
static bool op_stored_shape_refused(const char* op, int B, int T, int C, int H, int W) {
    if (B >= 1 && T >= 1 && C >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= (1LL << 30) && (int64_t)B * T * C <= 0x7fffffffLL) return false;
    op_refuse(op, "B, T, C, H, W >= 1, H * W <= 2^30 and B * T * C < 2^31");
    return true;
}

// ensemble_score_kernel and its finish kernel on stored member fields: frames [n][B][M][C][H][W], y [B][n][C][H][W]
int lns_op_ensemble_score(const float* frames, const float* y, int n, int B, int M, int C, int H, int W, const lns_eval_spec* spec,
                          float* scores_out, float* seq_out, int32_t* rank_out, float* pixel_out, void* stream) {
    if (!frames || !y || !scores_out) return op_refuse("ensemble_score", "frames / y / scores_out is null");
    if (op_spec_refused("ensemble_score", spec)) return LNS_EINVAL;
    if (M < 2 || M > LNS_SCORE_MAX_MEMBERS) return op_refuse("ensemble_score", "M in 2 .. 128");
    if (op_ensemble_shape_refused("ensemble_score", n, B, C, H, W)) return LNS_EINVAL;
    if (op_spec_refused("ensemble_score", spec, C)) return LNS_EINVAL;
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    EnsembleScoreArgs a;
    a.frames = frames; a.y = y; a.scores = scores_out; a.rank = rank_out; a.pixel = pixel_out;
    a.B = B; a.M = M; a.C = C; a.H = H; a.W = W; a.kk = n; a.y_T = n; a.y_t = 0;
    score_norm(spec, C, &a.norm);
    OPCHK(launch_ensemble_score(a, s));
    OPCHK(launch_ensemble_score_finish(scores_out, B, n, C, H * W, spec->eps, seq_out, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

// ensemble_quantile_kernel on stored member fields: frames [n][B][M][C][H][W] -> quant_out [B][n][n_q][C][H][W], prob_out [B][n][n_thr][C][H][W]
int lns_op_ensemble_quantiles(const float* frames, int n, int B, int M, int C, int H, int W, const lns_ensemble_quantile_spec* qspec,
                              const lns_eval_spec* norm, float* quant_out, float* prob_out, void* stream) {
    if (!frames) return op_refuse("ensemble_quantiles", "frames is null");
    if (const char* why = quantile_spec_refusal(qspec, quant_out, prob_out)) return op_refuse("ensemble_quantiles", why);
    if (norm && op_spec_refused("ensemble_quantiles", norm)) return LNS_EINVAL;
    if (M < 1 || M > LNS_SCORE_MAX_MEMBERS) return op_refuse("ensemble_quantiles", "M in 1 .. 128");
    if (op_ensemble_shape_refused("ensemble_quantiles", n, B, C, H, W)) return LNS_EINVAL;
    if (qspec->n_thr > 0 && C > LNS_METRIC_MAX_CH) return op_refuse("ensemble_quantiles", "thresholds need C <= 8");
    if (norm && op_spec_refused("ensemble_quantiles", norm, C)) return LNS_EINVAL;
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    EnsembleQuantileArgs a;
    quantile_args(qspec, norm, B, M, C, H, W, quant_out, prob_out, &a);
    a.frames = frames; a.kk = n; a.o_T = n; a.o_t = 0;
    OPCHK(launch_ensemble_quantile(a, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

// ensemble_exceed_kernel on stored member fields: frames [n][B][M][C][H][W] against y [B][n][C][H][W] -> table_out [B][n][n_thr][C][2][M + 1]
int lns_op_ensemble_exceed(const float* frames, const float* y, int n, int B, int M, int C, int H, int W,
                           const lns_ensemble_exceed_spec* xspec, const lns_eval_spec* norm, int32_t* table_out, void* stream) {
    if (!frames || !y) return op_refuse("ensemble_exceed", "frames or y is null");
    if (const char* why = exceed_spec_refusal(xspec, table_out)) return op_refuse("ensemble_exceed", why);
    if (norm && op_spec_refused("ensemble_exceed", norm)) return LNS_EINVAL;
    if (M < 1 || M > LNS_SCORE_MAX_MEMBERS) return op_refuse("ensemble_exceed", "M in 1 .. 128");
    if (op_ensemble_shape_refused("ensemble_exceed", n, B, C, H, W)) return LNS_EINVAL;
    if (C > LNS_METRIC_MAX_CH) return op_refuse("ensemble_exceed", "thresholds need C <= 8");
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    EnsembleExceedArgs a;
    exceed_args(xspec, norm, y, B, M, C, H, W, table_out, &a);
    a.frames = frames; a.kk = n; a.y_T = a.o_T = n; a.y_t = a.o_t = 0;
    OPCHK(hipMemsetAsync(table_out, 0, exceed_table_bytes(B, n, xspec->n_thr, C, M), s));   // the kernel adds
    OPCHK(launch_ensemble_exceed(a, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

// ensemble_obs_gram_kernel and its finish kernel on stored member fields: frames [n][B][M][C][H][W] against y_obs [B][n][C][H][W]
// under rinv (+ b * rinv_bs + i * rinv_ss) -> S_out [B][n][M][M], g_out [B][n][M], stat_out [B][n][3], double
int lns_op_ensemble_obs_gram(const float* frames, const float* y_obs, const float* rinv, int64_t rinv_bs, int64_t rinv_ss, int n, int B,
                             int M, int C, int H, int W, const lns_eval_spec* norm, double* S_out, double* g_out, double* stat_out,
                             void* stream) {
    if (!frames || !y_obs || !rinv) return op_refuse("ensemble_obs_gram", "frames, y_obs or rinv is null");
    if (!S_out || !g_out || !stat_out) return op_refuse("ensemble_obs_gram", "S_out, g_out or stat_out is null");
    if (norm && op_spec_refused("ensemble_obs_gram", norm)) return LNS_EINVAL;
    if (const char* why = etkf_members_refusal(M)) return op_refuse("ensemble_obs_gram", why);
    if (op_ensemble_shape_refused("ensemble_obs_gram", n, B, C, H, W)) return LNS_EINVAL;
    if (rinv_bs < 0 || rinv_ss < 0) return op_refuse("ensemble_obs_gram", "the strides of rinv must be >= 0 (0: shared)");
    if (norm && op_spec_refused("ensemble_obs_gram", norm, C)) return LNS_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    EnsembleObsGramArgs a;
    obs_gram_args(norm, y_obs, rinv, rinv_bs, rinv_ss, B, M, C, H, W, &a);
    a.frames = frames; a.kk = n; a.y_T = a.o_T = n; a.y_t = a.o_t = 0;
    OpScratch sc;
    a.part = static_cast<double*>(sc.alloc((size_t)B * n * a.nsl * etkf_part_doubles(M) * 2));
    if (sc.ok()) sc.note(init_kernels());
    if (sc.ok()) sc.note(launch_ensemble_obs_gram(a, s));
    if (sc.ok()) sc.note(launch_ensemble_obs_gram_finish(a.part, B * n, a.nsl, M, S_out, g_out, stat_out, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

// etkf_transform_kernel: S [B][n][M][M], g [B][n][M] -> X [B][M][M], wbar [B][M], lam [B][M], status [B]; never synchronises
int lns_op_etkf_transform(const double* S, const double* g, int B, int n, int M, double rho, double* X, double* wbar, double* lam,
                          int32_t* status, void* stream) {
    if (!S || !g) return op_refuse("etkf_transform", "S or g is null");
    if (!X || !wbar || !lam || !status) return op_refuse("etkf_transform", "X, wbar, lam or status is null");
    if (const char* why = etkf_members_refusal(M)) return op_refuse("etkf_transform", why);
    if (B < 1 || n < 1) return op_refuse("etkf_transform", "B, n >= 1");
    if (const char* why = etkf_rho_refusal(rho)) return op_refuse("etkf_transform", why);
    OPCHK(init_kernels());
    const EtkfTransformArgs a = {S, g, X, wbar, lam, status, rho, B, n, M};
    OPCHK(launch_etkf_transform(a, static_cast<hipStream_t>(stream)));
    return LNS_OK;
}

// ensemble_transform_kernel: z [B][M][n], X [B][M][M] -> out [B][M][n] (may be z); never synchronises
int lns_op_ensemble_transform(const float* z, const double* X, int B, int M, int64_t n, float* out, void* stream) {
    if (!z || !X || !out) return op_refuse("ensemble_transform", "z, X or out is null");
    if (const char* why = etkf_members_refusal(M)) return op_refuse("ensemble_transform", why);
    if (B < 1 || B > LNS_MAX_BATCH || n < 1 || n > ((int64_t)1 << 38)) return op_refuse("ensemble_transform", "B in 1..65535, n in 1..2^38");
    OPCHK(init_kernels());
    OPCHK(launch_ensemble_transform(z, X, B, M, (long)n, out, static_cast<hipStream_t>(stream)));
    return LNS_OK;
}

// the latent grid of the three localised ops: h, w >= 1 and h * w <= LNS_LETKF_MAX_DOMAINS
static_assert(LNS_LETKF_MAX_DOMAINS == 4096, "the messages here and in lns_engine.cpp say 4096");
static const char* letkf_grid_refusal(int h, int w) {
    return h < 1 || w < 1 || (int64_t)h * w > LNS_LETKF_MAX_DOMAINS ? "h, w >= 1 and h * w <= 4096 (the latent grid)" : nullptr;
}

// letkf_patch_gram_kernel on stored member fields: frames [n][B][M][C][H][W] against y_obs [B][n][C][H][W] under rinv (+ b * rinv_bs
// + i * rinv_ss), the frame cut into h x w patches -> part_out [B][n][h*w][M*M + M + 3] double; never synchronises
int lns_op_ensemble_patch_gram(const float* frames, const float* y_obs, const float* rinv, int64_t rinv_bs, int64_t rinv_ss, int n, int B,
                               int M, int C, int H, int W, int h, int w, const lns_eval_spec* norm, double* part_out, void* stream) {
    if (!frames || !y_obs || !rinv) return op_refuse("ensemble_patch_gram", "frames, y_obs or rinv is null");
    if (!part_out) return op_refuse("ensemble_patch_gram", "part_out is null");
    if (norm && op_spec_refused("ensemble_patch_gram", norm)) return LNS_EINVAL;
    if (const char* why = etkf_members_refusal(M)) return op_refuse("ensemble_patch_gram", why);
    if (op_ensemble_shape_refused("ensemble_patch_gram", n, B, C, H, W)) return LNS_EINVAL;
    if (n > 65535) return op_refuse("ensemble_patch_gram", "n in 1..65535");
    if (const char* why = letkf_grid_refusal(h, w)) return op_refuse("ensemble_patch_gram", why);
    if (rinv_bs < 0 || rinv_ss < 0) return op_refuse("ensemble_patch_gram", "the strides of rinv must be >= 0 (0: shared)");
    if (norm && op_spec_refused("ensemble_patch_gram", norm, C)) return LNS_EINVAL;
    OPCHK(init_kernels());
    LetkfPatchGramArgs a;
    patch_gram_args(norm, y_obs, rinv, rinv_bs, rinv_ss, B, M, C, H, W, h, w, &a);
    a.frames = frames; a.part = part_out; a.kk = n; a.y_T = a.o_T = n; a.y_t = a.o_t = 0;
    OPCHK(launch_letkf_patch_gram(a, static_cast<hipStream_t>(stream)));
    return LNS_OK;
}

// letkf_combine_kernel: part [B][n][h*w][M*M + M + 3] -> S_local [B][h*w][M][M], g_local [B][h*w][M], S_glob [B][M][M], g_glob [B][M],
// stat [B][n][3] (nullable); never synchronises
int lns_op_letkf_combine(const double* part, int B, int n, int M, int h, int w, double loc_radius, int bc_y, int bc_x, double* S_local,
                         double* g_local, double* S_glob, double* g_glob, double* stat, void* stream) {
    if (!part) return op_refuse("letkf_combine", "part is null");
    if (!S_local || !g_local || !S_glob || !g_glob) return op_refuse("letkf_combine", "S_local, g_local, S_glob or g_glob is null");
    if (const char* why = etkf_members_refusal(M)) return op_refuse("letkf_combine", why);
    if (B < 1 || B > LNS_MAX_BATCH || n < 1) return op_refuse("letkf_combine", "B in 1..65535, n >= 1");
    if (const char* why = letkf_grid_refusal(h, w)) return op_refuse("letkf_combine", why);
    if (const char* why = letkf_radius_refusal(loc_radius)) return op_refuse("letkf_combine", why);
    if (const char* why = letkf_bc_refusal(bc_y, bc_x)) return op_refuse("letkf_combine", why);
    OPCHK(init_kernels());
    const LetkfCombineArgs a = {part, S_local, g_local, S_glob, g_glob, stat, loc_radius, B, n, M, h, w, bc_y, bc_x};
    OPCHK(launch_letkf_combine(a, static_cast<hipStream_t>(stream)));
    return LNS_OK;
}

// letkf_update_kernel: z [B][M][c][h][w], X_local [B][h*w][M][M] -> out [B][M][c][h][w] (may be z); never synchronises
int lns_op_ensemble_transform_local(const float* z, const double* X_local, int B, int M, int c, int h, int w, float* out, void* stream) {
    if (!z || !X_local || !out) return op_refuse("ensemble_transform_local", "z, X_local or out is null");
    if (const char* why = etkf_members_refusal(M)) return op_refuse("ensemble_transform_local", why);
    if (B < 1 || B > LNS_MAX_BATCH || c < 1 || c > 65536) return op_refuse("ensemble_transform_local", "B in 1..65535, c in 1..65536");
    if (const char* why = letkf_grid_refusal(h, w)) return op_refuse("ensemble_transform_local", why);
    OPCHK(init_kernels());
    const LetkfUpdateArgs a = {z, X_local, out, B, M, c, h * w};
    OPCHK(launch_letkf_update(a, static_cast<hipStream_t>(stream)));
    return LNS_OK;
}

int lns_spectrum_bins(int H, int W) {
    const int S = lns_spectrum::bins(H, W);
    return S < 0 ? LNS_EINVAL : S;
}

static_assert(LNS_SPECTRUM_DFT == lns_spectrum::DFT && LNS_SPECTRUM_DCT == lns_spectrum::DCT, "the header's and the kernels' basis codes differ");

int lns_spectrum_bins_basis(int H, int W, int basis_y, int basis_x) {
    const int S = lns_spectrum::bins(H, W, basis_y, basis_x);
    return S < 0 ? LNS_EINVAL : S;
}

// spectrum_stored_kernel on stored fields: the per-plane body of the streaming call (spectrum_plane / spectrum_plane_basis)
int lns_op_energy_spectrum_basis(const float* yhat, const float* y, int B, int T, int C, int H, int W, const lns_eval_spec* spec,
                                 float* out, void* stream, int basis_y, int basis_x) {
    if (!yhat || !out) return op_refuse("energy_spectrum", "yhat / out is null");
    if (op_spec_refused("energy_spectrum", spec)) return LNS_EINVAL;
    if (B < 1 || T < 1 || C < 1 || (int64_t)B * T * C > 0x7fffffffLL) return op_refuse("energy_spectrum", "B, T, C >= 1 and B * T * C < 2^31");
    if (!lns_spectrum::supported(H, W)) return op_refuse("energy_spectrum", "the plane needs 1 <= H, W <= 192 and H * W <= 18432");
    if (!lns_spectrum::basis_ok(basis_y, basis_x)) return op_refuse("energy_spectrum", "basis_y, basis_x: LNS_SPECTRUM_DFT (0) or LNS_SPECTRUM_DCT (1)");
    if (op_spec_refused("energy_spectrum", spec, C)) return LNS_EINVAL;
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    SpectrumArgs a;
    memset(&a, 0, sizeof a);
    a.frames = yhat; a.y = y; a.out = out;
    a.B = B; a.C = C; a.H = H; a.W = W; a.S = lns_spectrum::bins(H, W, basis_y, basis_x); a.K = y ? 3 : 1; a.n = T;
    a.basis = basis_y | basis_x << 1;
    score_norm(spec, C, &a.norm);
    OPCHK(launch_spectrum_stored(a, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

int lns_op_energy_spectrum(const float* yhat, const float* y, int B, int T, int C, int H, int W, const lns_eval_spec* spec,
                           float* out, void* stream) {
    return lns_op_energy_spectrum_basis(yhat, y, B, T, C, H, W, spec, out, stream, LNS_SPECTRUM_DFT, LNS_SPECTRUM_DFT);
}

static_assert(LNS_FIELD_STATS_N == LNS_FIELD_STATS, "the kernels' and the header's number of statistics differ");

// field_stats_stored_kernel on stored fields: the per-plane body of the streaming call (field_stats_plane)
int lns_op_field_stats(const float* yhat, const float* y, int B, int T, int C, int H, int W, const lns_eval_spec* spec,
                       const lns_stats_spec* hspec, float* stats_out, int32_t* hist_out, void* stream) {
    if (!yhat || !y || !stats_out) return op_refuse("field_stats", "yhat / y / stats_out is null");
    if (op_spec_refused("field_stats", spec)) return LNS_EINVAL;
    if (op_stored_shape_refused("field_stats", B, T, C, H, W)) return LNS_EINVAL;
    if (op_spec_refused("field_stats", spec, C)) return LNS_EINVAL;
    FieldStatsArgs a;
    memset(&a, 0, sizeof a);
    if (const char* why = stats_hist_args(hspec, hist_out, C, &a)) return op_refuse("field_stats", why);
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    a.frames = yhat; a.y = y; a.stats = stats_out;
    a.B = B; a.C = C; a.H = H; a.W = W; a.n = T;
    a.eps = spec->eps;
    score_norm(spec, C, &a.norm);
    OPCHK(launch_field_stats_stored(a, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

static_assert(LNS_FLOW_STATS_N == LNS_FLOW_STATS, "the kernels' and the header's number of flow statistics differ");

// The shape bounds of the flow ops on stored fields [B][T][C][H][W]: one block (row of blocks) per frame, 256 threads each
static bool op_flow_shape_refused(const char* op, int B, int T, int C, int H, int W) {
    if (B >= 1 && T >= 1 && C >= 2 && H >= 1 && W >= 1 && (int64_t)H * W <= (1LL << 30) && (int64_t)B * T < (1LL << 24)) return false;
    op_refuse(op, "B, T, H, W >= 1, C >= 2, H * W <= 2^30 and B * T < 2^24");
    return true;
}

// flow_stats_stored_kernel on stored fields: the per-frame body of the streaming call (flow_stats_plane)
int lns_op_flow_stats(const float* yhat, const float* y, int B, int T, int C, int H, int W, const lns_eval_spec* spec,
                      const lns_flow_spec* fspec, float* flow_out, int32_t* hist_out, void* stream) {
    if (!yhat || !y || !flow_out) return op_refuse("flow_stats", "yhat / y / flow_out is null");
    if (op_spec_refused("flow_stats", spec)) return LNS_EINVAL;
    if (op_flow_shape_refused("flow_stats", B, T, C, H, W)) return LNS_EINVAL;
    if (op_spec_refused("flow_stats", spec, C)) return LNS_EINVAL;
    if (const char* why = flow_spec_refusal(fspec, C, hist_out)) return op_refuse("flow_stats", why);
    OpScratch sc;                                    // (no device memory of its own: the first failure and the final wait)
    hipStream_t s = static_cast<hipStream_t>(stream);
    FlowStatsArgs a;
    flow_args(fspec, spec, B, C, H, W, &a);
    a.frames = yhat; a.y = y; a.stats = flow_out; a.hist = hist_out; a.n = T;
    if (sc.ok()) sc.note(init_kernels());
    if (sc.ok()) sc.note(launch_flow_stats_stored(a, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

// vorticity_stored_kernel on stored fields: the pixel function of the statistics, pointwise
int lns_op_vorticity(const float* fields, int B, int T, int C, int H, int W, const lns_eval_spec* spec, const lns_flow_spec* fspec,
                     float* vort_out, void* stream) {
    if (!fields || !vort_out) return op_refuse("vorticity", "fields / vort_out is null");
    if (op_spec_refused("vorticity", spec)) return LNS_EINVAL;
    if (op_flow_shape_refused("vorticity", B, T, C, H, W)) return LNS_EINVAL;
    if (op_spec_refused("vorticity", spec, C)) return LNS_EINVAL;
    if (const char* why = flow_spec_refusal(fspec, C, nullptr)) return op_refuse("vorticity", why);
    OpScratch sc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FlowStatsArgs a;
    flow_args(fspec, spec, B, C, H, W, &a);
    a.frames = fields; a.vort = vort_out; a.n = T;
    if (sc.ok()) sc.note(init_kernels());
    if (sc.ok()) sc.note(launch_vorticity_stored(a, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

static_assert(LNS_TIME_MAPS_N == LNS_TIME_MAPS, "the kernels' and the header's number of time maps differ");

int lns_time_maps_state_bytes(int B, int C, int H, int W, size_t* bytes) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || (int64_t)H * W > (1LL << 30) || (int64_t)C * H * W > (1LL << 38))
        return op_refuse("time_maps", "B, C, H, W >= 1, H * W <= 2^30 and C * H * W <= 2^38");
    if (bytes) *bytes = time_maps_state_bytes((size_t)B, (size_t)C, (size_t)H, (size_t)W);
    return LNS_OK;
}

// the accumulation and finish kernels of lns_rollout_eval_maps on stored fields (one device function with the streaming call)
int lns_op_time_maps(const float* yhat, const float* y, int B, int T, int C, int H, int W, const lns_eval_spec* spec, int map_from,
                     int map_every, float* maps_out, void* state, size_t state_bytes, void* stream) {
    if (!yhat || !y || !maps_out) return op_refuse("time_maps", "yhat / y / maps_out is null");
    if (op_spec_refused("time_maps", spec)) return LNS_EINVAL;
    if (T < 1 || B > LNS_MAX_BATCH) return op_refuse("time_maps", "T >= 1 and B <= 65535");
    size_t need = 0;
    if (int rc = lns_time_maps_state_bytes(B, C, H, W, &need)) return rc;
    if (op_spec_refused("time_maps", spec, C)) return LNS_EINVAL;
    if (map_every < 1) return op_refuse("time_maps", "map_every must be at least 1");
    if (map_from < 0 || map_from >= T) return op_refuse("time_maps", fmt("map_from must be a step in [0, %d), got %d", T, map_from));
    if (!state || (reinterpret_cast<uintptr_t>(state) & 7)) return op_refuse("time_maps", "state is null or not 8-byte aligned");
    if (state_bytes < need) { g_create_error = fmt("time_maps: state too small: need %zu bytes, got %zu", need, state_bytes); return LNS_ENOMEM; }
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    TimeMapsArgs a;
    memset(&a, 0, sizeof a);
    a.frames = yhat; a.y = y; a.state = state; a.maps = maps_out;
    a.B = B; a.C = C; a.H = H; a.W = W; a.y_T = T; a.first = map_from; a.every = map_every;
    a.n = a.count = (T - 1 - map_from) / map_every + 1;
    score_norm(spec, C, &a.norm);
    OPCHK(hipMemsetAsync(state, 0, (size_t)B * C * H * W * LNS_TIME_MAPS_STATE_PER_PIXEL, s));
    OPCHK(launch_time_maps_stored(a, s));
    OPCHK(launch_time_maps_finish(a, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

// attrib_group_kernel and attrib_finish_kernel of lns_rollout_eval_attrib on stored fields
int lns_op_eval_attrib(const float* yhat, const float* r, const float* y, int B, int T, int C, int H, int W,
                       const lns_eval_spec* spec, float* prop_frame, float* prop_seq, float* cross_frame, float* cross_seq,
                       void* stream) {
    if (!yhat || !r || !y) return op_refuse("eval_attrib", "yhat / r / y is null");
    if (!prop_frame && !prop_seq && !cross_frame && !cross_seq) return op_refuse("eval_attrib", "no output is set");
    if (op_spec_refused("eval_attrib", spec)) return LNS_EINVAL;
    if (op_stored_shape_refused("eval_attrib", B, T, C, H, W)) return LNS_EINVAL;
    if (op_spec_refused("eval_attrib", spec, C)) return LNS_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t planes = (size_t)B * T * C;
    OpScratch sc;
    float* pp = static_cast<float*>(sc.alloc(planes * 3));      // (PP, XX, G) per plane
    AttribGroupArgs a;
    a.frames = yhat; a.recon = r; a.y = y; a.part = pp;
    a.B = 1; a.C = C; a.H = H; a.W = W; a.kk = B * T; a.y_T = B * T; a.y_t = 0; a.p_T = B * T; a.p_t = 0;
    score_norm(spec, C, &a.norm);
    if (sc.ok()) sc.note(launch_attrib_group(a, s));
    if (sc.ok()) sc.note(launch_attrib_finish(pp, B, T, C, spec->eps, prop_frame, prop_seq, cross_frame, cross_seq, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

// latent_err_group_kernel of lns_rollout_eval_attrib on one stored group: z [T][B][zper] (a ring group's layout) against
// ztrue [T][B][zstride] (the staging buffer's), then the metric's finish kernel with C = 1
int lns_op_latent_err(const float* z, const float* ztrue, int B, int T, int zper, int64_t zstride, float eps, float* frame_out,
                      float* seq_out, void* stream) {
    if (!z || !ztrue || (!frame_out && !seq_out)) return op_refuse("latent_err", "z / ztrue is null, or frame_out and seq_out are");
    if (B < 1 || T < 1 || zper < 1 || (int64_t)B * T > 0x7fffffffLL) return op_refuse("latent_err", "B, T, zper >= 1 and B * T < 2^31");
    if (zstride < zper || (zstride & 3) || (reinterpret_cast<uintptr_t>(ztrue) & 15))
        return op_refuse("latent_err", "zstride must be a multiple of 4 floats, at least zper, and ztrue 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    OpScratch sc;
    float* part = static_cast<float*>(sc.alloc((size_t)B * T * 2));
    LatentErrArgs a;
    a.z = z; a.ztrue = ztrue; a.part = part; a.zstride = (long)zstride; a.zper = zper; a.B = B; a.kk = T; a.T_total = T; a.t = 0;
    a.mean = 0.0f; a.sd = 1.0f;
    if (sc.ok()) sc.note(launch_latent_err_group(a, s));
    if (sc.ok()) sc.note(launch_metric_finish(part, B, T, 1, eps, frame_out, seq_out, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

int lns_metric_rel_l2(const float* yhat, const float* y, int B, int T, int C, int HW, float mean, float std, float eps,
                      float* frame_out, float* seq_out, float* scratch, void* stream) {
    if (!yhat || !y || !scratch || B <= 0 || T <= 0 || C <= 0 || HW <= 0 || (!frame_out && !seq_out)) return LNS_EINVAL;
    OPCHK(launch_metric_rel_l2(yhat, y, B, T, C, HW, mean, std, eps, frame_out, seq_out, scratch, static_cast<hipStream_t>(stream)));
    return LNS_OK;
}

int lns_metric_rel_l2_ch(const float* yhat, const float* y, int B, int T, int C, int H, int W, const float* mean_host,
                         const float* std_host, const int* flags_host, float clamp_lo, float clamp_hi, float eps,
                         float* frame_out, float* seq_out, float* scratch, void* stream) {
    if (!yhat || !y || !scratch || B <= 0 || T <= 0 || C <= 0 || C > LNS_METRIC_MAX_CH || H <= 0 || W <= 0 ||
        (!frame_out && !seq_out))
        return LNS_EINVAL;
    MetricChannelSpec spec;
    for (int c = 0; c < LNS_METRIC_MAX_CH; ++c) {
        spec.mean[c] = (mean_host && c < C) ? mean_host[c] : 0.0f;
        spec.std[c] = (std_host && c < C) ? std_host[c] : 1.0f;
        spec.flags[c] = (flags_host && c < C) ? flags_host[c] : 0;
    }
    spec.lo = clamp_lo; spec.hi = clamp_hi;
    OPCHK(launch_metric_rel_l2_ch(yhat, y, B, T, C, H, W, spec, eps, frame_out, seq_out, scratch, static_cast<hipStream_t>(stream)));
    return LNS_OK;
}

int lns_op_groupnorm_stats(const float* x, int B, int C, int HW, int groups, float eps, const float* gamma_host,
                           const float* beta_host, const float* premul, float* ss, void* stream) {
    if (!x || !ss || C % groups) return LNS_EINVAL;
    OpScratch sc;
    float* dgb = static_cast<float*>(sc.alloc((size_t)2 * C));
    OPCHK(sc.err);                              // (nothing is on the stream yet)
    if (gamma_host) sc.copy_in(dgb, gamma_host, C);
    if (beta_host) sc.copy_in(dgb + C, beta_host, C);
    GnStatsArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.x_bs = (long)C * HW; a.C = C; a.HW = HW; a.groups = groups; a.eps = eps;
    a.gamma = gamma_host ? dgb : nullptr; a.beta = beta_host ? dgb + C : nullptr; a.premul = premul; a.ss = ss; a.B = B;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(sc.alloc((size_t)B * C * 2));
    if (sc.ok()) sc.note(launch_gn_stats(a, part, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

int lns_op_attention(const float* qkv, int B, int heads, int dim_head, int n, float scale, float* o, void* stream) {
    if (!qkv || !o) return LNS_EINVAL;
    AttnArgs a = {qkv, B, heads, dim_head, n, scale, o, nullptr};
    hipStream_t s = static_cast<hipStream_t>(stream);
    // max |qkv| per sample (what the qkv convolution records inside a plan): enables the f16x2 form
    OpScratch sc;
    unsigned* damax = sc.amax_words(B, s);
    const long per = 3L * heads * dim_head * n;
    if (sc.ok()) sc.note(launch_amax(qkv, per, per, B, damax, s));
    a.amax_in = damax;
    if (sc.ok()) sc.note(launch_attention(a, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

int lns_op_fa_sandwich(const float* u, const float* kx, const float* ky, int B, int heads, int C, int H, int W, float eps,
                       int apply_instance_norm, float* out, void* stream) {
    if (!u || !kx || !ky || !out) return LNS_EINVAL;
    OPCHK(init_kernels());
    FaSandwichArgs a = {u, kx, ky, B, heads, C, H, W, eps, apply_instance_norm, out, nullptr, 0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    // max |u| per sample (what the in_proj convolution records inside a plan): enables the f16x2 form
    OpScratch sc;
    unsigned* damax = sc.amax_words(B, s);
    if (sc.ok()) sc.note(launch_amax(u, (long)heads * C * H * W, (long)heads * C * H * W, B, damax, s));
    a.amax_u = damax;
    if (sc.ok()) sc.note(launch_fa_sandwich(a, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

int lns_op_fa_pool(const float* x, int64_t x_bs, const float* ss, int B, int C, int H, int W, float* mx, float* my, void* stream) {
    if (!x || !mx || !my || B <= 0 || C <= 0 || H <= 0 || W <= 0 || x_bs < (int64_t)C * H * W) return LNS_EINVAL;
    OPCHK(init_kernels());
    FaPoolArgs a = {x, (long)x_bs, ss, B, C, H, W, mx, my};
    hipStream_t s = static_cast<hipStream_t>(stream);
    OPCHK(launch_fa_pool(a, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

// FABlock2D with in_proj inside the sandwich (include/lns.h): the input split pre-pass, then the fused kernel, their arguments
// set as Planner::lower_fa sets them (fa_fused_weight_scale, fa_fused_gpb_rule).  No HIP call before the last check.
int lns_op_fa_fused(const lns_fa_fused_args* p, void* stream) {
    if (!p) return op_refuse("fa_fused", "args is null");
    if (!p->x || !p->w_host || !p->kx || !p->ky || !p->out) return op_refuse("fa_fused", "x / w_host / kx / ky / out is null");
    if (p->B < 1 || p->B > LNS_MAX_BATCH || p->heads < 1 || p->heads > 65535) return op_refuse("fa_fused", "B and heads in 1..65535");
    if (p->dim_head < 1 || !fa_fused_fits(p->H, p->W, p->Cin, p->dim_head))
        return op_refuse("fa_fused",
                         fmt("no fused kernel for %d x %d planes, %d channels, dim_head %d: 64 x 64 with 64 channels or 32 x 32 with 64 / 128, "
                             "dim_head a multiple of 16", p->H, p->W, p->Cin, p->dim_head));
    const int B = p->B, heads = p->heads, dh = p->dim_head, C = p->Cin, H = p->H, W = p->W, groups = dh / 16, planes = heads * dh;
    if ((long)B * heads * groups > 0x7fffffffL) return op_refuse("fa_fused", "B * heads * dim_head / 16 exceeds the grid");
    if (p->gpb < 0 || (p->gpb > 0 && groups % p->gpb != 0))
        return op_refuse("fa_fused", fmt("gpb %d does not divide the %d plane groups of a head (0 = automatic)", p->gpb, groups));
    if (p->form < 0 || p->form > 2 || (p->form != 0 && H == 32))
        return op_refuse("fa_fused", "form 0 (double-buffered), 1 (single-buffered) or 2 (generic) at 64 x 64, 0 at 32 x 32");
    if (!(p->bound > 0.0f)) return op_refuse("fa_fused", "bound must be positive");
    if (p->x_bs < (int64_t)C * H * W) return op_refuse("fa_fused", "x_bs is shorter than a sample");
    // ---- every check is done ----
    const FaWeightScale ws = fa_fused_weight_scale(p->w_host, planes, C);
    std::vector<float> img(fa_fused_weight_bytes(planes, C) / 4);
    fa_fused_pack_weight(img.data(), p->w_host, planes, C, ws.wscale);
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t amax_words = (size_t)B * LNS_AMAX_SUB;
    OpScratch sc;
    void* dgs = sc.alloc(fa_fused_gs_bytes(B, H, W, C) / 4);
    void* dwp = sc.alloc(img.size());
    unsigned* damax = static_cast<unsigned*>(sc.alloc(amax_words));
    if (sc.ok()) sc.note(hipMemcpyAsync(dwp, img.data(), img.size() * 4, hipMemcpyHostToDevice, s));
    sc.fill(damax, 0, amax_words, s);
    if (sc.ok()) {
        FaGsplitArgs g = {};
        g.x = p->x; g.x_bs = (long)p->x_bs; g.Cin = C; g.HW = H * W; g.ss = p->ss; g.bound = p->bound;
        g.gs = dgs; g.amax_out = damax; g.B = B;
        sc.note(launch_fa_gsplit(g, s));
    }
    if (sc.ok()) {
        FaFusedArgs a = {};
        a.gs = dgs; a.amax_g = damax; a.bound = p->bound;
        a.wp = dwp; a.w_inv = 1.0f / ws.wscale; a.wrow_max = ws.wrow_max;
        a.kx = p->kx; a.ky = p->ky;
        a.B = B; a.heads = heads; a.C = dh; a.Cin = C; a.H = H; a.W = W; a.eps = p->eps; a.instnorm = p->instnorm ? 1 : 0;
        a.out = p->out; a.b_rev = p->b_rev ? 1 : 0; a.single_buffer = p->form;
        a.gpb = p->gpb > 0 ? p->gpb : fa_fused_gpb_rule(0, groups, B, heads);
        sc.note(launch_fa_fused(a, s));
    }
    OPCHK(sc.finish(s));                                    // (img, the source of the weight copy, lives until here)
    if (p->amax_out) OPCHK(amax_words_to_float(damax, B, p->amax_out));     // max |G| of a sample
    return LNS_OK;
}

// ---- the FABlock axis kernels, ln_pe and apply at op level (include/lns.h, "op_fa_axis") ---------------------------------
int lns_fa_reducer_fits(int C, int Hid, int Out, int merged) { return fa_reducer_fits(C, Hid, Out, merged != 0) ? 1 : 0; }
int lns_fa_lrk_fits(int DK, int n) { return fa_lrk_fits(DK, n) ? 1 : 0; }
int lns_rotary_table(int n, const float* inv_freq_host, int half, float* out_host) {
    if (n < 1 || half < 1 || !inv_freq_host || !out_host) return LNS_EINVAL;
    rotary_table_fill(n, inv_freq_host, half, out_host);
    return LNS_OK;
}

static std::vector<float> transposed(const float* src, size_t rows, size_t cols) {
    std::vector<float> t(rows * cols);
    transpose_rows(t.data(), src, rows, cols);
    return t;
}

int lns_op_fa_reducer(const lns_fa_reducer_args* p, void* stream) {
    if (!p) return op_refuse("fa_reducer", "args is null");
    const bool has_y = p->my != nullptr;
    if (!p->mx || !p->ux || !p->to_in_x || !p->ln_g_x || !p->ln_b_x || !p->w1_x || !p->w2_x || !p->b2_x)
        return op_refuse("fa_reducer", "mx / ux or a weight of the x axis is null");
    if (has_y && (!p->uy || !p->to_in_y || !p->ln_g_y || !p->ln_b_y || !p->w1_y || !p->w2_y || !p->b2_y))
        return op_refuse("fa_reducer", "my is set but uy or a weight of the y axis is null");
    if (p->form != 0 && p->form != 1) return op_refuse("fa_reducer", "form 0 (both axes in one launch) or 1 (one launch per axis)");
    if (p->form == 0 && !has_y) return op_refuse("fa_reducer", "form 0 (the merged launch) needs both axes");
    if (p->B < 1 || p->B > LNS_MAX_BATCH) return op_refuse("fa_reducer", "B in 1..65535");
    if (p->nx < 1 || p->nx > 65535 || (has_y && (p->ny < 1 || p->ny > 65535))) return op_refuse("fa_reducer", "nx and ny in 1..65535");
    if (!fa_reducer_fits(p->C, p->Hid, p->Out, p->form == 0))
        return op_refuse("fa_reducer", std::string(p->form == 0 ? "no merged kernel for " : "no kernel for ") + fa_axis_limits(p->C, p->Hid, p->Out));
    // ---- every check is done ----
    const int B = p->B, C = p->C, Hid = p->Hid, Out = p->Out;
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    OpScratch sc;
    FaReducerArgs fr[2];
    for (int ax = 0; ax < (has_y ? 2 : 1); ++ax) {               // Planner::lower_fa's fill_reducer on the caller's operands
        FaReducerArgs& a = fr[ax];
        memset(&a, 0, sizeof a);
        const int n = ax == 0 ? p->nx : p->ny;
        a.m = ax == 0 ? p->mx : p->my; a.rows = (long)B * n; a.n = n; a.C = C; a.Hid = Hid; a.Out = Out;
        a.win_t = sc.upload(transposed(ax == 0 ? p->to_in_x : p->to_in_y, C, C));
        a.ln_g = sc.upload(ax == 0 ? p->ln_g_x : p->ln_g_y, C); a.ln_b = sc.upload(ax == 0 ? p->ln_b_x : p->ln_b_y, C);
        a.w1_t = sc.upload(transposed(ax == 0 ? p->w1_x : p->w1_y, Hid, C));
        a.w2_t = sc.upload(transposed(ax == 0 ? p->w2_x : p->w2_y, Out, Hid));
        a.b2 = sc.upload(ax == 0 ? p->b2_x : p->b2_y, Out);
        a.u = ax == 0 ? p->ux : p->uy;
        a.amax_out = sc.amax_words(B, s);
    }
    if (sc.ok() && p->form == 0) sc.note(launch_fa_reducer2(fr[0], fr[1], s));
    if (sc.ok() && p->form != 0) sc.note(launch_fa_reducer(fr[0], s));
    if (sc.ok() && p->form != 0 && has_y) sc.note(launch_fa_reducer(fr[1], s));
    OPCHK(sc.finish(s));
    if (p->amax_x) OPCHK(amax_words_to_float(fr[0].amax_out, B, p->amax_x));
    if (has_y && p->amax_y) OPCHK(amax_words_to_float(fr[1].amax_out, B, p->amax_y));
    return LNS_OK;
}

int lns_op_fa_lrk(const lns_fa_lrk_args* p, void* stream) {
    if (!p) return op_refuse("fa_lrk", "args is null");
    const bool has_y = p->qk_y != nullptr;
    if (!p->qk_x || !p->inv_freq_x || !p->kx) return op_refuse("fa_lrk", "qk_x / inv_freq_x / kx is null");
    if (has_y && (!p->inv_freq_y || !p->ky)) return op_refuse("fa_lrk", "qk_y is set but inv_freq_y / ky is null");
    if (p->form != 0 && p->form != 1) return op_refuse("fa_lrk", "form 0 (both axes in one launch) or 1 (one launch per axis)");
    if (p->form == 0 && !has_y) return op_refuse("fa_lrk", "form 0 (the merged launch) needs both axes");
    const int Bs[2] = {p->B_x, p->B_y}, hs[2] = {p->heads_x, p->heads_y}, dks[2] = {p->DK_x, p->DK_y}, ns[2] = {p->nx, p->ny};
    for (int ax = 0; ax < (has_y ? 2 : 1); ++ax) {
        if (Bs[ax] < 1 || Bs[ax] > LNS_MAX_BATCH || hs[ax] < 1 || hs[ax] > 65535) return op_refuse("fa_lrk", "B and heads in 1..65535");
        if (dks[ax] < 2 || dks[ax] % 2)
            return op_refuse("fa_lrk", fmt("DK = %d: the rotary embedding pairs channel d with d + DK / 2, DK must be even", dks[ax]));
        if (ns[ax] < 1) return op_refuse("fa_lrk", "nx and ny must be positive");
    }
    if (p->form == 0 && (Bs[0] != Bs[1] || hs[0] != hs[1] || dks[0] != dks[1]))
        return op_refuse("fa_lrk", "the merged launch needs the same B, heads and DK on both axes");
    for (int ax = 0; ax < (has_y ? 2 : 1); ++ax)
        if (!fa_lrk_fits(dks[ax], ns[ax]))
            return op_refuse("fa_lrk", fmt("no kernel for DK = %d, n = %d: q' and k' need %zu bytes of LDS, the limit is %d", dks[ax], ns[ax],
                                           fa_lrk_lds_bytes(dks[ax], ns[ax]), (int)FA_AXIS_LDS_LIMIT));
    // ---- every check is done ----
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    OpScratch sc;
    FaLrkArgs fl[2];
    for (int ax = 0; ax < (has_y ? 2 : 1); ++ax) {
        std::vector<float> cs((size_t)ns[ax] * (dks[ax] / 2) * 2);
        rotary_table_fill(ns[ax], ax == 0 ? p->inv_freq_x : p->inv_freq_y, dks[ax] / 2, cs.data());
        FaLrkArgs& a = fl[ax];
        memset(&a, 0, sizeof a);
        a.qk = ax == 0 ? p->qk_x : p->qk_y; a.B = Bs[ax]; a.heads = hs[ax]; a.DK = dks[ax]; a.n = ns[ax];
        a.cs = sc.upload(cs); a.kmat = ax == 0 ? p->kx : p->ky;
    }
    if (sc.ok() && p->form == 0) sc.note(launch_fa_lrk2(fl[0], fl[1], s));
    if (sc.ok() && p->form != 0) sc.note(launch_fa_lrk(fl[0], s));
    if (sc.ok() && p->form != 0 && has_y) sc.note(launch_fa_lrk(fl[1], s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

int lns_op_ln_pe(const float* x, int64_t x_bs, int B, int C, int n, const float* gamma_host, const float* beta_host,
                 const float* pe_host, int pe_len, float eps, float* h, float* bound_out, void* stream) {
    if (!x || !h || !gamma_host || !beta_host) return op_refuse("ln_pe", "x / h / gamma / beta is null");
    if (B < 1 || B > LNS_MAX_BATCH) return op_refuse("ln_pe", "B in 1..65535");
    if (C < 1 || n < 1 || (int64_t)C * n > 0x7fffffffLL) return op_refuse("ln_pe", "C, n >= 1 and C * n < 2^31");
    if (x_bs < (int64_t)C * n) return op_refuse("ln_pe", "x_bs is shorter than a sample");
    if (pe_host && pe_len < n) return op_refuse("ln_pe", "more tokens than positional table rows");
    if (!(eps > 0.0f)) return op_refuse("ln_pe", "eps must be positive");
    // ---- every check is done ----
    auto absmax = [](const float* v, size_t count) { float m = 0.0f; for (size_t i = 0; v && i < count; ++i) m = std::max(m, fabsf(v[i])); return m; };
    if (bound_out) *bound_out = ln_pe_bound(C, absmax(gamma_host, C), absmax(beta_host, C), absmax(pe_host, (size_t)pe_len * C));
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    OpScratch sc;
    LnPeArgs a;
    memset(&a, 0, sizeof a);                                     // Planner::lower_sa's arguments
    a.x = x; a.x_bs = (long)x_bs; a.C = C; a.n = n; a.eps = eps;
    a.gamma = sc.upload(gamma_host, C); a.beta = sc.upload(beta_host, C);
    a.pe_t = pe_host ? sc.upload(transposed(pe_host, pe_len, C)) : nullptr; a.pe_stride = pe_len;
    a.h = h; a.B = B;
    if (sc.ok()) sc.note(launch_ln_pe(a, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

int lns_op_apply(const float* x, int64_t x_bs, const float* ss, int act, int B, int C, int HW, float* y, unsigned* amax_out,
                 void* stream) {
    if (!x || !y) return op_refuse("apply", "x / y is null");
    if (act < ACT_NONE || act > ACT_SIGMOID) return op_refuse("apply", "act in 0..5 (none, swish, gelu, relu, tanh, sigmoid)");
    if (B < 1 || B > LNS_MAX_BATCH) return op_refuse("apply", "B in 1..65535");
    if (C < 1 || HW < 1 || (int64_t)C * HW > 0x7fffffffLL) return op_refuse("apply", "C, HW >= 1 and C * HW < 2^31");
    if (x_bs < (int64_t)C * HW) return op_refuse("apply", "x_bs is shorter than a sample");
    // ---- every check is done ----
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    ApplyArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.x_bs = (long)x_bs; a.ss = ss; a.act = act; a.y = y; a.B = B; a.C = C; a.HW = HW; a.amax_out = amax_out;
    OPCHK(launch_apply(a, s));
    OPCHK(hipStreamSynchronize(s));
    return LNS_OK;
}

int lns_op_fourier_block(const float* x, int B, int Cin, int Cout, int H, int W, int m1, int m2, const float* w1_host,
                         const float* w2_host, const float* conv_w_host, const float* conv_b_host, const float* cond,
                         const float* freq_w_host, const float* freq_b_host, const float* lin_w_host,
                         const float* lin_b_host, int activation, int residual, float* y, void* stream) {
    if (!x || !y || !w1_host || !w2_host || !conv_w_host || B <= 0 || Cin <= 0 || Cout <= 0 || 2 * m1 > H || m2 > W / 2 + 1)
        return LNS_EINVAL;
    if (cond && (!freq_w_host || !freq_b_host || !lin_w_host || !lin_b_host)) return LNS_EINVAL;
    if (residual && Cin != Cout) return LNS_EINVAL;                // x_skip + out needs matching shapes (basics.py:581-582)
    if (activation < ACT_SWISH || activation > ACT_SIGMOID) return LNS_EINVAL;
    OPCHK(init_kernels());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nw = (size_t)Cin * Cout * m1 * m2 * 2, nf = (size_t)4 * m1 * m2;
    const size_t t1n = (size_t)B * std::max(Cin, Cout) * H * m2 * 2, xfi = (size_t)B * Cin * 2 * m1 * m2 * 2,
                 xfo = (size_t)B * Cout * 2 * m1 * m2 * 2, act = (size_t)B * Cout * H * W;
    // one scratch allocation: [w1 | w2 | freq_w | freq_b | lin_w | lin_b | emb | e | t1 | xf | of | x1 | x2]
    // (conditional block: the conditioning vector has in_planes entries, fourier_cond.py:102-104)
    std::vector<size_t> sz = {nw, nw, (size_t)Cin * nf, nf, (size_t)Cout * Cin, (size_t)Cout, (size_t)B * nf, (size_t)B * Cout,
                              t1n, xfi, xfo, act, act};
    std::vector<size_t> off(sz.size());
    size_t tot = 0;
    for (size_t i = 0; i < sz.size(); ++i) { off[i] = tot; tot += (sz[i] + 63) / 64 * 64; }
    OpScratch sc;
    float* d = static_cast<float*>(sc.alloc(tot));
    OPCHK(sc.err);                              // (nothing is on the stream yet)
    sc.copy_in(d + off[0], w1_host, nw);
    sc.copy_in(d + off[1], w2_host, nw);
    if (cond) {
        sc.copy_in(d + off[2], freq_w_host, (size_t)Cin * nf);
        sc.copy_in(d + off[3], freq_b_host, nf);
        sc.copy_in(d + off[4], lin_w_host, (size_t)Cout * Cin);
        sc.copy_in(d + off[5], lin_b_host, (size_t)Cout);
        // FreqLinear: h = cond @ weights[Cin, 4 m1 m2] + bias      (fourier_cond.py:25-29)
        VecLinearArgs fl = {cond, d + off[2], d + off[3], d + off[6], B, Cin, (int)nf, 1, (int)nf};
        if (sc.ok()) sc.note(launch_vec_linear(fl, s));
        // emb_out = Linear(cond): weight [out, in]                (fourier_cond.py:104,111)
        VecLinearArgs ll = {cond, d + off[4], d + off[5], d + off[7], B, Cin, Cout, Cin, 1};
        if (sc.ok()) sc.note(launch_vec_linear(ll, s));
    }
    SpectralArgs sp;
    memset(&sp, 0, sizeof sp);
    sp.x = x; sp.x_bs = (long)Cin * H * W; sp.B = B; sp.Cin = Cin; sp.Cout = Cout; sp.H = H; sp.W = W; sp.m1 = m1; sp.m2 = m2;
    sp.w1 = d + off[0]; sp.w2 = d + off[1]; sp.emb = cond ? d + off[6] : nullptr;
    sp.t1 = d + off[8]; sp.xf = d + off[9]; sp.of = d + off[10]; sp.y = d + off[11];
    if (sc.ok()) sc.note(launch_spectral(sp, s));
    const int rc = !sc.ok() ? 0 : lns_op_conv2d(x, B, Cin, H, W, H, W, conv_w_host, conv_b_host, Cout, 1, 1, 1, 0, 0, 0, 0, 0, 0, nullptr, 0,
                                                0, nullptr, nullptr, d + off[12], -1, stream, nullptr);
    if (rc) { (void)sc.finish(s); return rc; }
    FourierCombineArgs fc = {d + off[11], d + off[12], cond ? d + off[7] : nullptr, residual ? x : nullptr, (long)Cin * H * W, y,
                             (long)Cout * H * W, B, Cout, H * W, nullptr, activation};
    if (sc.ok()) sc.note(launch_fourier_combine(fc, s));
    OPCHK(sc.finish(s));
    return LNS_OK;
}

// ---- Fourier block with device-resident weights (the module objects of lns_amd.modules.fourier_cond) -----------------
// lns_op_fourier_block uploads every weight on every call (a unit-test entry point); a module that is called repeatedly
// keeps them on the device: create once per (weights, device), forward launches only.
struct lns_fourier_block {
    int Cin = 0, Cout = 0, m1 = 0, m2 = 0, conditional = 0, activation = ACT_GELU, residual = 1, device = 0;
    std::vector<float> conv_w, conv_b;      // host copies: the 1x1 convolution's launch is prepared per (B, H, W)
    float* dwt = nullptr;                    // [w1 | w2 | freq_w | freq_b | lin_w | lin_b]
    size_t woff[6] = {0, 0, 0, 0, 0, 0};
    float* scratch = nullptr; size_t scratch_floats = 0;
    OpConv oc; bool oc_ready = false; int oc_B = 0, oc_H = 0, oc_W = 0; const float* oc_x = nullptr; float* oc_y = nullptr;
    ~lns_fourier_block() { oc.release(); (void)hipFree(dwt); (void)hipFree(scratch); }     // under the owner's DeviceGuard
};

int lns_fourier_block_create(int Cin, int Cout, int m1, int m2, const float* w1_host, const float* w2_host,
                             const float* conv_w_host, const float* conv_b_host, const float* freq_w_host,
                             const float* freq_b_host, const float* lin_w_host, const float* lin_b_host, int activation,
                             int residual, int device, lns_fourier_block** out) {
    if (!out || !w1_host || !w2_host || !conv_w_host || Cin <= 0 || Cout <= 0 || m1 <= 0 || m2 <= 0) return LNS_EINVAL;
    const bool cond = freq_w_host != nullptr;
    if (cond && (!freq_b_host || !lin_w_host || !lin_b_host)) return LNS_EINVAL;
    if (residual && Cin != Cout) return LNS_EINVAL;
    if (activation < ACT_SWISH || activation > ACT_SIGMOID) return LNS_EINVAL;
    DeviceGuard guard(device);
    OPCHK(init_kernels());
    std::unique_ptr<lns_fourier_block> h(new lns_fourier_block);
    h->Cin = Cin; h->Cout = Cout; h->m1 = m1; h->m2 = m2; h->conditional = cond; h->activation = activation;
    h->residual = residual; h->device = device;
    h->conv_w.assign(conv_w_host, conv_w_host + (size_t)Cout * Cin);
    if (conv_b_host) h->conv_b.assign(conv_b_host, conv_b_host + Cout);
    const size_t nw = (size_t)Cin * Cout * m1 * m2 * 2, nf = (size_t)4 * m1 * m2;
    const size_t sz[6] = {nw, nw, cond ? (size_t)Cin * nf : 0, cond ? nf : 0, cond ? (size_t)Cout * Cin : 0, cond ? (size_t)Cout : 0};
    const float* src[6] = {w1_host, w2_host, freq_w_host, freq_b_host, lin_w_host, lin_b_host};
    size_t tot = 0;
    for (int i = 0; i < 6; ++i) { h->woff[i] = tot; tot += (sz[i] + 63) / 64 * 64; }
    OPCHK(hipMalloc(reinterpret_cast<void**>(&h->dwt), std::max<size_t>(tot, 64) * 4));
    for (int i = 0; i < 6; ++i)
        if (sz[i]) OPCHK(hipMemcpy(h->dwt + h->woff[i], src[i], sz[i] * 4, hipMemcpyHostToDevice));
    *out = h.release();
    return LNS_OK;
}

void lns_fourier_block_destroy(lns_fourier_block* h) {
    if (!h) return;
    DeviceGuard guard(h->device);                // (outlives the delete: the handle's memory is freed on its device)
    delete h;
}

int lns_fourier_block_forward(lns_fourier_block* h, const float* x, const float* cond, int B, int H, int W, float* y, void* stream) {
    if (!h || !x || !y || B <= 0 || 2 * h->m1 > H || h->m2 > W / 2 + 1) return LNS_EINVAL;
    if ((cond != nullptr) != (h->conditional != 0)) return LNS_EINVAL;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Cin = h->Cin, Cout = h->Cout, m1 = h->m1, m2 = h->m2;
    const size_t nf = (size_t)4 * m1 * m2;
    // scratch: [emb | e | t1 | xf | of | x1 | x2]; grown when a larger shape arrives (the only allocation after create)
    const size_t sz[7] = {(size_t)B * nf, (size_t)B * Cout, (size_t)B * std::max(Cin, Cout) * H * m2 * 2, (size_t)B * Cin * 2 * m1 * m2 * 2,
                          (size_t)B * Cout * 2 * m1 * m2 * 2, (size_t)B * Cout * H * W, (size_t)B * Cout * H * W};
    size_t off[7], tot = 0;
    for (int i = 0; i < 7; ++i) { off[i] = tot; tot += (sz[i] + 63) / 64 * 64; }
    if (tot > h->scratch_floats) {
        OPCHK(hipStreamSynchronize(s));
        (void)hipFree(h->scratch); h->scratch = nullptr; h->scratch_floats = 0;
        h->oc.release(); h->oc_ready = false;                     // (its output pointer lived in the old scratch)
        OPCHK(hipMalloc(reinterpret_cast<void**>(&h->scratch), tot * 4));
        h->scratch_floats = tot;
    }
    float* d = h->scratch;
    if (cond) {
        VecLinearArgs fl = {cond, h->dwt + h->woff[2], h->dwt + h->woff[3], d + off[0], B, Cin, (int)nf, 1, (int)nf};
        OPCHK(launch_vec_linear(fl, s));
        VecLinearArgs ll = {cond, h->dwt + h->woff[4], h->dwt + h->woff[5], d + off[1], B, Cin, Cout, Cin, 1};
        OPCHK(launch_vec_linear(ll, s));
    }
    SpectralArgs sp;
    memset(&sp, 0, sizeof sp);
    sp.x = x; sp.x_bs = (long)Cin * H * W; sp.B = B; sp.Cin = Cin; sp.Cout = Cout; sp.H = H; sp.W = W; sp.m1 = m1; sp.m2 = m2;
    sp.w1 = h->dwt + h->woff[0]; sp.w2 = h->dwt + h->woff[1]; sp.emb = cond ? d + off[0] : nullptr;
    sp.t1 = d + off[2]; sp.xf = d + off[3]; sp.of = d + off[4]; sp.y = d + off[5];
    OPCHK(launch_spectral(sp, s));
    if (!h->oc_ready || h->oc_B != B || h->oc_H != H || h->oc_W != W) {
        OPCHK(hipStreamSynchronize(s));
        h->oc.release(); h->oc_ready = false;
        const int rc = op_conv_prepare(h->oc, x, B, Cin, H, W, H, W, h->conv_w.data(), h->conv_b.empty() ? nullptr : h->conv_b.data(), Cout,
                                       1, 1, 1, 0, 0, 0, 0, 0, 0, nullptr, 0, 0, nullptr, nullptr, d + off[6], -1, s);
        if (rc) return rc;                                        // (what it allocated goes with the next release)
        h->oc_ready = true; h->oc_B = B; h->oc_H = H; h->oc_W = W;
    } else {          // same launch, new input: its per-sample maximum again (dynamic activation scale)
        h->oc.a.x = x; h->oc.a.y = d + off[6];
        OPCHK(hipMemsetAsync(h->oc.damax, 0, (size_t)B * LNS_AMAX_SUB * 4, s));
        OPCHK(launch_amax(x, h->oc.a.x_bs, (long)Cin * H * W, B, h->oc.damax, s));
    }
    OPCHK(launch_conv(h->oc.variant, h->oc.a, s));
    FourierCombineArgs fc = {d + off[5], d + off[6], cond ? d + off[1] : nullptr, h->residual ? x : nullptr, (long)Cin * H * W, y,
                             (long)Cout * H * W, B, Cout, H * W, nullptr, h->activation};
    OPCHK(launch_fourier_combine(fc, s));
    return LNS_OK;
}
