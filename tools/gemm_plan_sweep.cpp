// Stand-alone host program: the invariant sweep of tests/test_gemm_plan_cpu.py run directly on the planning functions of
// mmg-clip_amd/csrc/gemm_plan.hip, for a sanitizer build of that host-only file (nothing here touches a GPU; not a pytest test):
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         mmg-clip_amd/csrc/gemm_plan.hip tools/gemm_plan_sweep.cpp -o gemm_plan_sweep && ./gemm_plan_sweep
//
// It stands in for the two core.hip functions gemm_plan.hip calls (error text, CU count).
#include "../mmg-clip_amd/csrc/gemm_plan.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

static char g_err[512];
void mmg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int mmg_cu_count_cached(void) { return 256; }
extern "C" const char* mmg_gemm_plan(int op, int M, int N, int K, int cus);

static long cdivl(long a, long b) { return (a + b - 1) / b; }
static int failures = 0;
#define EXPECT(cond)                                                                                        \
    do {                                                                                                    \
        if (!(cond)) { ++failures; printf("FAILED %s: op=%d M=%d N=%d K=%d [%s]\n", #cond, op, M, N, K, text); } \
    } while (0)

int main() {
    const int Ms[] = {1, 37, 4095, 4096, 65535, 65536, 4194304 + 17};
    const int Ns[] = {8, 96, 128, 192, 200, 256, 384, 392, 768, 3072};
    const char* doors[7] = {"mmg_gemm_nt_bf16", "mmg_gemm_nt_fp8", "mmg_gemm_nt_fp8_bwd", "mmg_gemm_nt_fp8_bwd", "mmg_gemm_tn_bf16", "mmg_gemm_tn_fp8", "mmg_gemm_tn_fp8"};
    const GemmKnobs kn = gemm_knobs(GEMM_LIVE_NT | GEMM_LIVE_TN | GEMM_LIVE_TN8);
    int valid = 0, rejected = 0;
    for (int M : Ms) for (int N : Ns) for (int K : Ns) for (int op = 0; op < 7; ++op) {
        const char* text = mmg_gemm_plan(op, M, N, K, 256);
        if (!text[0]) {
            ++rejected;
            EXPECT(strncmp(g_err, doors[op], strlen(doors[op])) == 0 && g_err[strlen(doors[op])] == ':');
            continue;
        }
        ++valid;
        const GemmPlan p = op < 4 ? plan_nt(op, M, N, K, kn) : op == 4 ? plan_tn(M, N, K, kn) : plan_tn8(op == 5, M, N, K, 256, kn);
        EXPECT(strncmp(text, gemm_kernel_name(p.kernel), strlen(gemm_kernel_name(p.kernel))) == 0 && p.kernel > GK_NONE && p.kernel < GK_COUNT);
        EXPECT(p.grid_x >= 1 && p.grid_y >= 1 && p.grid_y <= 65535 && (p.block == 256 || p.block == 512));
        EXPECT(p.lds > 0 && p.lds <= 160 * 1024);
        EXPECT(p.tiles1 >= 1 && p.tiles2 >= 1);
        if (op < 4) {
            int bm = 0, bn = 0;
            sscanf(gemm_kernel_name(p.kernel), "gemm_nt_kernel<%d, %d", &bm, &bn);
            EXPECT(bm > 0 && (long)p.tiles1 * bm >= M && (long)p.tiles2 * bn >= N && p.grid_x == p.tiles1 * p.tiles2);
            continue;
        }
        const int stage = gemm_kernel_stage_rows(p.kernel);
        const int n1 = p.swapped ? K : N, n2 = p.swapped ? N : K;
        int t1 = 0, t2 = 0;
        if (sscanf(gemm_kernel_name(p.kernel), "gemm_tn_kernel<%d, %d", &t1, &t2) == 2) { t1 *= 128; t2 *= 128; }
        else if (sscanf(gemm_kernel_name(p.kernel), "gemm_tn_wide_kernel<%d, %d", &t1, &t2) == 2) {}
        else t1 = t2 = strstr(gemm_kernel_name(p.kernel), "wide") ? 256 : 128;
        EXPECT(stage > 0 && p.chunks >= 1 && p.rows_per_chunk % stage == 0 && (long)p.chunks * p.rows_per_chunk >= M);
        EXPECT((long)p.tiles1 * t1 >= n1 && (long)p.tiles2 * t2 >= n2);
        EXPECT((long)p.grid_x * p.grid_y >= (long)cdivl(n1, t1) * cdivl(n2, t2) * p.chunks);
    }
    printf("gemm_plan_sweep: %d plans checked, %d shapes rejected, %d failures\n", valid, rejected, failures);
    return failures != 0;
}
