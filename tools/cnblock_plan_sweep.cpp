// Stand-alone host program: mmg_cnblock_plan and the planning functions of mmg-clip_amd/csrc/cnblock_plan.hip swept over every entry
// point, width, row-count edge, mode, CU count and knob value, for a sanitizer build of that host-only file (nothing here touches a GPU;
// not a pytest test):
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         mmg-clip_amd/csrc/cnblock_plan.hip tools/cnblock_plan_sweep.cpp -o tools/cnblock_plan_sweep && tools/cnblock_plan_sweep
//
// It stands in for the two core.hip functions cnblock_plan.hip calls (error text, CU count).
#include "../mmg-clip_amd/csrc/cnblock_plan.h"
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
extern "C" const char* mmg_cnblock_plan(int op, long long M, int C, int save, int ln, int cus);

static int failures = 0;
#define EXPECT(cond)                                                                                                        \
    do {                                                                                                                    \
        if (!(cond)) { ++failures; printf("FAILED %s: op=%d M=%lld C=%d save=%d ln=%d cus=%d [%s]\n", #cond, op, M, C, save, ln, cus, text); } \
    } while (0)

static void set_knob(const char* name, const char* v) {
    if (v) setenv(name, v, 1);
    else unsetenv(name);
}

int main() {
    const long long Ms[] = {0, 1, 63, 64, 65, 127, 128, 129, 1LL << 24, (1LL << 36) - 1, 1LL << 36};
    const int cuss[] = {1, 2, 256, 304};
    const char* doors[3] = {"mmg_cnblock_mlp_fwd:", "mmg_cnblock_mlp_bwd:", "mmg_cnblock_bwdw:"};
    const char* res[] = {nullptr, "0", "8", "12", "7"};
    const char* nts[] = {nullptr, "0", "1"};
    const char* vars[] = {nullptr, "0", "1", "2", "3"};
    const char* onoff[] = {nullptr, "0", "1"};
    long valid = 0, rejected = 0, wrapped = 0;
    // the knobs of one entry point at a time (they do not interact across entry points): op 0 RES x NT, op 1 NT, op 2 VAR x HTO x W12
    for (int op = 0; op < 3; ++op)
        for (int k = 0; k < (op == 0 ? 15 : op == 1 ? 3 : 45); ++k) {
            if (op == 0) { set_knob("MMG_MLP_FWD_RES", res[k % 5]); set_knob("MMG_MLP_NT_STORE", nts[k / 5]); }
            if (op == 1) set_knob("MMG_MLP_NT_STORE", nts[k]);
            if (op == 2) { set_knob("MMG_BWDW_VAR", vars[k % 5]); set_knob("MMG_BWDW_HTO", onoff[(k / 5) % 3]); set_knob("MMG_BWDW_W12", onoff[k / 15]); }
            const CnKnobs kn = cn_knobs();
            for (int C = 32; C <= 1024; C += 32) for (long long M : Ms) for (int save = 0; save < 2; ++save) for (int ln = 0; ln < 2; ++ln) for (int cus : cuss) {
                const char* text = mmg_cnblock_plan(op, M, C, save, ln, cus);
                if (!text[0]) {
                    ++rejected;
                    const bool mode = (save && op != 0) || (ln && op != 1);
                    EXPECT(strncmp(g_err, mode ? "mmg_cnblock_plan:" : doors[op], strlen(mode ? "mmg_cnblock_plan:" : doors[op])) == 0);
                    continue;
                }
                ++valid;
                const CnPlan p = cn_plan(op, M, C, save, ln, cus, kn);
                const char* name = cn_plan_name(p);
                EXPECT(name[0] && strncmp(text, name, strlen(name)) == 0 && cn_kernel_name(p.kernel)[0] && (op == 2) == (p.kernel2 != 0));
                EXPECT(!p.kernel2 || cn_kernel_name(p.kernel2)[0]);
                EXPECT(p.block >= 256 && p.block <= 768 && p.block % 64 == 0 && p.lds > 0 && p.lds <= 160 * 1024 && (p.nt == 0 || p.nt == 1));
                // the one known exception is listed, not hidden: the resident forward counts 32-row tiles in an int, which M >= 2^36 - 31
                // passes (2^31 tiles: 13 TB of rows at C = 96); the launchers before this layer did the same
                if (op == 0 && p.tile == 32 && M > (1LL << 36) - 32) { ++wrapped; continue; }
                // every row lies in a tile, no tile is empty, no workgroup is without a tile
                const int walkers = p.tile == 32 ? p.block / 64 : 1;
                EXPECT((long long)p.ntiles * p.tile >= M && (long long)(p.ntiles - 1) * p.tile < M);
                EXPECT(p.grid >= 1 && p.grid <= 3 * cus && (long long)(p.grid - 1) * walkers < p.ntiles);
            }
        }
    printf("cnblock_plan_sweep: %ld plans checked (%ld with a wrapped tile count), %ld shapes rejected, %d failures\n", valid, wrapped, rejected, failures);
    return failures != 0;
}
