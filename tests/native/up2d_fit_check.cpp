// Stand-alone host check of the dual-phase upsampling conv's per-layer rule (csrc/conv3_up2d.inc: convud_fits,
// convud_lds_bytes).  Links the built library, calls host functions only (no GPU, no HIP call); built and run by
// tests/test_up2_dual_cpu.py, which pins the printed lines.
#include <cstdio>
#include <cstring>

#include "lns_kernels.h"

using namespace lns;

static ConvArgs base() {
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.ks = 3; a.stride = 1; a.dil = 1; a.up2 = 1; a.wb = &a;
    a.Cin = 64; a.Cin_pad = 64; a.Cout = 64; a.Hin = 64; a.Win = 64; a.Hout = 128; a.Wout = 128;
    a.PH = 6; a.PW = 34;                       // 4 x 32 source tile + halo
    return a;
}

int main() {
    ConvArgs a = base();
    printf("decoder layer 64->64 at 128^2: fits %d lds %zu\n", (int)convud_fits(a), convud_lds_bytes(a));
    a = base(); a.PH = 16; a.PW = 16;          // the largest patch one unit per thread covers
    printf("patch 256: fits %d\n", (int)convud_fits(a));
    a.PH = 1; a.PW = 257;
    printf("patch 257: fits %d\n", (int)convud_fits(a));
    // the largest shape the rule admits: a 256-unit patch and the most channel stages whose tables still fit in 80 KB
    a = base(); a.PH = 16; a.PW = 16;
    int cmax = 0;
    for (int c = 8; c <= 16384; c += 8) { a.Cin = a.Cin_pad = c; if (convud_fits(a)) cmax = c; }
    a.Cin = a.Cin_pad = cmax;
    printf("largest: Cin_pad %d lds %zu fits %d\n", cmax, convud_lds_bytes(a), (int)convud_fits(a));
    a.Cin = a.Cin_pad = cmax + 8;
    printf("past the largest: lds %zu fits %d\n", convud_lds_bytes(a), (int)convud_fits(a));
    a = base(); a.up2 = 0;       printf("refuse not upsampling: %d\n", (int)convud_fits(a));
    a = base(); a.x_oct = 1;     printf("refuse OCT8 input: %d\n", (int)convud_fits(a));
    a = base(); a.y_oct = 1;     printf("refuse OCT8 output: %d\n", (int)convud_fits(a));
    a = base(); a.w2 = a.x = reinterpret_cast<const float*>(&a); printf("refuse fused 1x1: %d\n", (int)convud_fits(a));
    a = base(); a.Cin_pad = 60;  printf("refuse ragged stage pad: %d\n", (int)convud_fits(a));
    a = base(); a.wb = nullptr;  printf("refuse no phase slabs: %d\n", (int)convud_fits(a));
    a = base(); a.Wout = 127;    printf("refuse odd width: %d\n", (int)convud_fits(a));
    a = base(); a.Cout = 512; a.Hout = 1024; a.Wout = 1024; printf("refuse 2 GB sample: %d\n", (int)convud_fits(a));
    a = base(); a.res = reinterpret_cast<const float*>(&a); a.Cout = 100; a.Cin = 40; a.Cin_pad = 40;
    printf("residual, ragged channels: fits %d\n", (int)convud_fits(a));
    printf("ALL DONE\n");
    return 0;
}
