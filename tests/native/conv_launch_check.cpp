// Stand-alone host check of the conv launch rules (csrc/lns_conv_launch.h): padded pack sizes, the fp16-split weight scale,
// the patch division constant, the arithmetic-map rule, map lengths, the GroupNorm fold and bound, geometry -> ConvArgs.
// Links the built library (conv_geometry asks it which tiles fit), calls host functions only (no GPU, no HIP call); built
// and run by tests/test_conv_launch_cpu.py, which pins the printed lines against values derived by hand from the rules.
#include <cstdio>
#include <cstring>

#include "lns_conv_launch.h"

using namespace lns;

static ConvArgs zeroed() {
    ConvArgs a;
    memset(&a, 0, sizeof a);
    return a;
}

static void padded(const char* what, int k, int cin, int cout) {
    const ConvPadded p = conv_padded_sizes(k, cin, cout);
    printf("padded %s: kc_log2 %d Cin_pad %d Cout_pad %d\n", what, p.kc_log2, p.Cin_pad, p.Cout_pad);
}

static void arith(const char* what, int variant, int k, int Hv, int Wv, int pad, int my, int mx) {
    ConvArgs a = zeroed();
    const int pads[4] = {pad, pad, pad, pad};
    conv_set_map_arith(a, variant, k, 16, 16, Hv, Wv, pads, my, mx);
    printf("arith %s: on %d circ %d %d pad %d %d ext %d %d\n", what, a.map_arith, a.map_circ[0], a.map_circ[1], a.map_pad[0],
           a.map_pad[1], a.map_ext[0], a.map_ext[1]);
}

int main() {
    padded("k3 3->4", 3, 3, 4);
    padded("k1 40->100", 1, 40, 100);
    for (int cout : {33, 64, 65, 129}) printf("padded cout %d: Cout_pad %d\n", cout, conv_padded_sizes(3, 8, cout).Cout_pad);

    for (float m : {1.0f, 2.0f, 16000.0f, 16001.0f}) printf("scale max %.0f: %.10g\n", m, conv_f16_weight_scale(m));
    printf("unscale: f16x2 %.10g b1 %.10g fp32 %.10g\n", conv_unscale(CV_F64, 4096.0f), conv_unscale(CV_B1, 8.0f), conv_unscale(CV_L64, 8.0f));

    for (int PH : {1, 6, 34}) {
        ConvGeom g;
        memset(&g, 0, sizeof g);
        g.PH = PH; g.PW = 1;
        ConvArgs a = zeroed();
        conv_set_geometry(a, g, 1, 8, 4, 4, 8, 3, 1, 1, 8, 32);
        printf("ph_magic PH %d: %u\n", PH, a.ph_magic);
    }

    const int Z = LNS_PAD_ZEROS, C = LNS_PAD_CIRCULAR;
    arith("zeros zeros", CV_F64, 3, 16, 16, 1, Z, Z);
    arith("circular zeros", CV_F64, 3, 16, 16, 1, C, Z);
    arith("zeros circular", CV_F64, 3, 16, 16, 1, Z, C);
    arith("circular circular", CV_F64, 3, 16, 16, 1, C, C);
    arith("pad 4 dilation 4", CV_F64, 3, 16, 16, 4, C, C);
    arith("fp32 variant", CV_L64, 3, 16, 16, 1, Z, Z);
    arith("resized 2x, not the phase form", CV_F64, 3, 32, 32, 1, Z, Z);
    arith("pad 17", CV_F64, 3, 16, 16, 17, C, C);
    arith("other padding mode", CV_F64, 3, 16, 16, 1, 2, Z);

    {   // a 21 x 37 plane, 64 -> 64 channels, pad 1, on the f16x2 tiles; rows circular, columns zeros
        const int pad[4] = {1, 1, 1, 1};
        ConvGeom g;
        const bool ok = conv_geometry(g, 1, 64, 21, 37, 3, 1, 1, pad, 3, 64, CV_F64);
        printf("tiling 21x37: found %d bw_log2 %d tiles_x %d tiles_y %d PH %d PW %d TN %d\n", (int)ok, g.bw_log2, g.tiles_x, g.tiles_y,
               g.PH, g.PW, conv_variant_info(g.variant).TN);
        std::vector<int> rm, cm;
        conv_tile_maps(rm, cm, g, 1, 21, 37, 21, 37, 0.0f, 0.0f, pad, C, Z);
        printf("rowmap: len %zu r0 %d r1 %d r21 %d r22 %d r23 %d last %d\n", rm.size(), rm[0], rm[1], rm[21], rm[22], rm[23], rm.back());
        printf("colmap: len %zu c0 %d c1 %d c37 %d c38 %d last %d\n", cm.size(), cm[0], cm[1], cm[37], cm[38], cm.back());
    }

    {
        float table = 0.0f, part = 0.0f, gamma = 0.0f, beta = 0.0f, premul = 0.0f;
        ConvArgs a = zeroed();
        a.ss = &table;
        conv_fold_gn(a, &part, 2, GN_TILE_PIXELS, 32, 1e-6f, nullptr, &gamma, &beta);
        printf("fold exact tiles: gn_count %d gn_tiles %d gn_groups %d ss_null %d part %d gamma %d beta %d premul_null %d eps %.1e\n", a.gn_count,
               a.gn_tiles, a.gn_groups, a.ss == nullptr, a.gn_part == &part, a.gn_gamma == &gamma, a.gn_beta == &beta,
               a.gn_premul == nullptr, a.gn_eps);
        a = zeroed();
        a.ss = &table;
        conv_fold_gn(a, &part, 1, 7 * 15, 1, 1e-5f, &premul, nullptr, nullptr);
        printf("fold ragged single tile: gn_count %d gn_tiles %d gn_groups %d ss_null %d premul %d\n", a.gn_count, a.gn_tiles, a.gn_groups,
               a.ss == nullptr, a.gn_premul == &premul);
        unsigned amax = 0;
        a.amax_in = &amax;
        conv_set_final_bound(a, gn_output_bound(2.0f, 0.5f, 8, 4, 4));
        printf("gn bound: value %.6f final %d amax_null %d\n", a.amax_in_const, a.bound_final, a.amax_in == nullptr);
    }

    {   // every field a ConvGeom and the layer's static facts decide
        const ConvGeom g = {CV_F64, 4, 3, 5, 2, 10, 18, 21, 37, 3, 2};
        ConvArgs a = zeroed();
        conv_set_geometry(a, g, 7, 40, 21, 37, 100, 3, 1, 2, 40, 128);
        printf("geom: kc_log2 %d tiles_x %d tiles_y %d cout_tiles %d bw_log2 %d PH %d PW %d B %d ph_magic %u ks %d stride %d dil %d "
               "Cin_pad %d Cout_pad %d vec4 %d Cin %d Hin %d Win %d Cout %d Hout %d Wout %d x_bs %ld y_bs %ld\n", a.kc_log2, a.tiles_x,
               a.tiles_y, a.cout_tiles, a.bw_log2, a.PH, a.PW, a.B, a.ph_magic, a.ks, a.stride, a.dil, a.Cin_pad, a.Cout_pad, a.vec4,
               a.Cin, a.Hin, a.Win, a.Cout, a.Hout, a.Wout, a.x_bs, a.y_bs);
        ConvGeom g1 = g;
        g1.PH = g1.PW = 1; g1.Hout = 4; g1.Wout = 4;
        a = zeroed();
        conv_set_geometry(a, g1, 1, 64, 4, 4, 64, 1, 1, 1, 64, 64);
        printf("vec4 1x1 on 16 pixels: %d\n", a.vec4);
        g1.Hout = 21; g1.Wout = 37;
        conv_set_geometry(a, g1, 1, 64, 21, 37, 64, 1, 1, 1, 64, 64);
        printf("vec4 1x1 on 777 pixels: %d\n", a.vec4);
    }
    printf("ALL DONE\n");
    return 0;
}
