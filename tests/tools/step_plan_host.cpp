// step_plan_host.cpp - TEST INFRASTRUCTURE: the step plan (vmap_amd/csrc/step_plan.h) walked over the grid of
// tests/tools/step_plan_dump.py on the host, part by part - shape check, (a) family, (b) rounds, (c) sections - for both values of
// measurement_build, then the pointer-free argument block and the two block maps.  A stand-alone program for the sanitizers:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I tests/sim -I tests/sim/include -I vmap_amd/csrc
//           tests/tools/step_plan_host.cpp -o step_plan_host && ./step_plan_host
// Prints how many entries each build's plan accepts and a checksum of the plans; exit status 0 when every accepted plan's sections
// are in order and end at its total.
#include <cstdarg>
#include <cstdio>

#include "step_plan.h"

static char g_err[512];
int vl::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int main() {
    const int n_obj[] = {1, 7, 8, 9, 20, 32, 50, 256, 257}, rays[] = {1, 12, 120, 150, 256, 300, 600, 1200, 4800};
    const int samples[] = {1, 10, 14, 32, 33, 64, 65, 96, 128, 129}, hidden[] = {16, 32, 48, 64, 96, 128, 256, 288};
    const int weights[] = {0, 1, 3}, max_steps[] = {1, 20, 256, 257};
    // {workgroups_per_object, kernel, generic_finalize, ws_flags}; the first entry stands for "no tuning struct"
    const vmapstep_tuning tunings[] = {{0, 0, 0, 0}, {0, 1, 0, 0}, {0, 2, 0, 0}, {0, 3, 0, 0}, {0, 4, 0, 0}, {0, 5, 0, 0}, {0, 6, 0, 0}, {0, 7, 0, 0},
                                       {0, 8, 0, 0}, {0, 17, 0, 0}, {0, -1, 0, 0}, {1, 0, 0, 0}, {2, 0, 0, 0}, {50, 0, 0, 0}, {1000, 0, 0, 0},
                                       {0, 0, 0, 1}, {0, 0, 0, 2}, {0, 0, 0, 4}, {0, 0, 0, 8}, {50, 0, 0, 2}, {0, 0, 1, 0}};
    long long accepted[2] = {0, 0}, refused[2] = {0, 0}, bad = 0;
    unsigned long long sum = 0;
    for (int n : n_obj) for (int R : rays) for (int S : samples) for (int H : hidden) for (int w : weights)
        for (const vmapstep_tuning& t : tunings) for (int steps : max_steps) for (int mb = 0; mb < 2; ++mb) {
            const vmapstep_shape sh = {n, R, S, H, w, 0, &t == &tunings[0] ? nullptr : &t};
            vl::Layout L;
            vl::Plan pl;
            vl::make_layout(H, L);
            if (vl::check_shape(&sh, steps) || vl::plan_family(&sh, mb != 0, pl.family) || vl::plan_rounds(&sh, mb != 0, pl) ||
                vl::plan_sections(&sh, steps, L, pl)) {
                ++refused[mb];
                continue;
            }
            ++accepted[mb];
            vk::StepArgs a;
            vl::fill_step_plan(a, &sh, pl, L);
            const size_t offs[] = {pl.off_ploss, pl.off_imgtab, pl.off_tab_wt, pl.off_row_tab, pl.off_pgrad, pl.off_wimg, pl.off_scratch,
                                   pl.off_flags, pl.off_stats, pl.total};
            for (int i = 0; i + 1 < 10; ++i) bad += offs[i] > offs[i + 1] || offs[i] % vl::kAlign != 0;
            for (size_t o : offs) sum = sum * 1000003ull + o;
            sum = sum * 1000003ull + (unsigned)(pl.family + 8 * pl.G + 4096 * pl.tiles + 16384 * a.xcd_affine + 32768 * vl::finalize_xcd_affine(a, true)) +
                  ((unsigned long long)pl.NG << 20) + ((unsigned long long)pl.NW << 40) + (unsigned)vl::main_workgroups(a);
        }
    for (int mb = 0; mb < 2; ++mb) printf("measurement_build=%d: %lld plans, %lld refusals\n", mb, accepted[mb], refused[mb]);
    printf("checksum %016llx, %lld sections out of order\n", sum, bad);
    return bad ? 1 : 0;
}
