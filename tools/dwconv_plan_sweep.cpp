// Stand-alone host program: mmg_dwconv7_plan and the planning functions of mmg-clip_amd/csrc/dwconv_plan.hip swept over every door, shape
// edge (the checks' bounds and the int limits included), CU count and knob value, for a sanitizer build of that host-only file (nothing
// here touches a GPU; not a pytest test):
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         mmg-clip_amd/csrc/dwconv_plan.hip tools/dwconv_plan_sweep.cpp -o tools/dwconv_plan_sweep && tools/dwconv_plan_sweep
//
// It stands in for the two core.hip functions dwconv_plan.hip calls (error text, CU count).
#include "../mmg-clip_amd/csrc/dwconv_plan.h"
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static char g_err[512];
void mmg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int mmg_cu_count_cached(void) { return 256; }
extern "C" const char* mmg_dwconv7_plan(int op, int n, int H, int W, int C, int flip, int add, int cus);

static int failures = 0;
#define EXPECT(cond)                                                                                                        \
    do {                                                                                                                    \
        if (!(cond)) { ++failures; printf("FAILED %s: op=%d n=%d H=%d W=%d C=%d cus=%d [%s]\n", #cond, op, n, H, W, C, cus, text); } \
    } while (0)

static void set_knob(const char* name, const char* v) {
    if (v) setenv(name, v, 1);
    else unsetenv(name);
}

int main() {
    const int ns[] = {INT_MIN, -1, 0, 1, 7, 8, 64, 65535, 65536, 1 << 20, INT_MAX};
    const int dims[] = {INT_MIN, 0, 1, 7, 16, 17, 22, 56, 1024, 4080, 4081, 1 << 19, INT_MAX};
    const int Cs[] = {-32, 0, 32, 48, 96, 1024, 2016, 2048, 32 * 1025, 95296, 95328, 32 * 65535, 32 * 65536, 1 << 21, INT_MAX - 31};
    const int cuss[] = {0, 1, 2, 8, 256, 304, INT_MAX};
    const char* doors[3] = {"mmg_dwconv7_nhwc:", "mmg_dwconv7_nhwc_mfma:", "mmg_dwconv7_wgrad:"};
    const char* onoff[] = {nullptr, "0", "1", "7"};
    const char* ths[] = {nullptr, "8", "16", "12"};
    const char* waves[] = {nullptr, "8", "16", "4"};
    long valid = 0, rejected = 0;
    // the knobs of one door at a time (they do not interact across doors): op 0 ROWS2 x TH, op 1 WAVES, op 2 ROWS2 x DWG_TH x ALIGN
    for (int op = 0; op < 3; ++op)
        for (int k = 0; k < (op == 0 ? 16 : op == 1 ? 4 : 64); ++k) {
            if (op == 0) { set_knob("MMG_DWCONV_ROWS2", onoff[k % 4]); set_knob("MMG_DWCONV_TH", ths[k / 4]); }
            if (op == 1) set_knob("MMG_DWM_WAVES", waves[k]);
            if (op == 2) { set_knob("MMG_DWCONV_ROWS2", onoff[k % 4]); set_knob("MMG_DWG_TH", ths[(k / 4) % 4]); set_knob("MMG_DWG_ALIGN", onoff[k / 16]); }
            const DwKnobs kn = dw_knobs();
            for (int n : ns) for (int H : dims) for (int W : dims) for (int C : Cs) for (int cus : cuss) {
                if (op != 1 && cus != 256) continue;                    // only the matrix-core door reads the CU count
                const int add = (n ^ H ^ cus) & 1, flip = (W ^ C / 32) & 1;
                const char* text = mmg_dwconv7_plan(op, n, H, W, C, op == 2 ? 0 : flip, op == 2 ? 0 : add, cus);
                if (!text[0]) {
                    ++rejected;
                    EXPECT(strncmp(g_err, doors[op], strlen(doors[op])) == 0);
                    EXPECT(dw_check(op, DwArgs{n, H, W, C, 1}) != 0);
                    continue;
                }
                ++valid;
                EXPECT(dw_check(op, DwArgs{n, H, W, C, 1}) == 0 && dw_check(op, DwArgs{n, H, W, C, 0}) != 0);
                const DwPlan p = dw_plan(op, n, H, W, C, op == 2 ? 0 : flip, op == 2 ? 0 : add, cus ? cus : 256, kn);
                const char* name = dw_kernel_name(p.kernel);
                EXPECT(name[0] && strncmp(text, name, strlen(name)) == 0 && text[strlen(name)] == ' ');
                EXPECT(p.gx >= 1 && p.gy >= 1 && p.gz >= 1 && p.gy <= 65535 && p.gz <= 65535);
                EXPECT((p.block == 256 || p.block == 512 || p.block == 1024) && p.lds > 0 && p.lds <= 160 * 1024 && (p.nt == 0 || p.nt == 1));
                // every pixel lies in a tile, no tile row or column is empty
                EXPECT((long long)p.tiles_h * p.th >= H && (long long)(p.tiles_h - 1) * p.th < H && (long long)p.tiles_w * p.tw >= W && (long long)(p.tiles_w - 1) * p.tw < W);
                EXPECT(p.items == (long long)n * p.tiles_w * p.tiles_h && p.slabs == C / 32);
                if (op == 0) EXPECT(p.gx == p.tiles_w * p.tiles_h && p.gy == p.slabs && p.gz == n);
                if (op == 1) EXPECT(p.gx % 8 == 0 && p.gx / 8 >= p.slabs && p.gy == 1 && p.gz == 1 && p.block == (kn.mfma_waves == 8 ? 512 : 1024) && p.by_image == (n >= 8));
                if (op == 2) EXPECT(p.gx <= 1024 && p.gx <= p.items && p.gy == p.slabs && p.gz == 1 && p.nt == 0);
            }
        }
    // an id outside the table has no name
    for (int id = -2; id < 1024; ++id) {
        int listed = 0;
#define KV(FLIP) listed |= id == DK_fwd_##FLIP;
#define KR(FLIP, TH) listed |= id == DK_rows2_##FLIP##_##TH;
#define KM(FLIP, NW, ADD) listed |= id == DK_mfma_##FLIP##_##NW##_##ADD;
#define KG() listed |= id == DK_wgrad;
#define KG2(TH) listed |= id == DK_wgrad2_##TH;
        DW_KERNELS(KV, KR, KM, KG, KG2)
        if (listed != (dw_kernel_name(id)[0] != 0)) { ++failures; printf("FAILED kernel id %d: listed=%d name=[%s]\n", id, listed, dw_kernel_name(id)); }
    }
    printf("dwconv_plan_sweep: %ld plans checked, %ld shapes rejected, %d failures\n", valid, rejected, failures);
    return failures != 0;
}
