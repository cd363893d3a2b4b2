/* stage_host_check.c — drives the engine's host-only stage queries through
 * the C ABI, for running the engine's host code under a sanitizer on a CPU.
 * No device is touched: every pointer is a stand-in used for its alignment.
 *
 * For each rank of a 2 x 3 grid it builds the plan flavours of the stage
 * snapshot (plain, composite, wire with and without grouped converting
 * kernels, scaled, keep, grouped split / join, keep with grouped split / join),
 * asks pa_plan_stage_launches for n = 1 and 3 and pa_plan_stage_launches_soa
 * for n = 2 and 5 on aligned and on offset pointers, and destroys the plans.
 * It prints the number of rows it saw; a sanitizer report is the failure.
 *
 * Build and run (CPU only):
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -c \
 *       -Xarch_host -fsanitize=address,undefined \
 *       -I include pencilarrays_amd/csrc/pencilhip.hip -o pencilhip_san.o
 *   hipcc -x c -c -g -fsanitize=address,undefined -I include \
 *       tools/stage_host_check.c -o stage_host_check.o
 *   hipcc -fsanitize=address,undefined pencilhip_san.o stage_host_check.o \
 *       -L/opt/rocm/lib -lrccl -lamdhip64 -o stage_host_check
 *   ./stage_host_check
 */

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pencilhip.h"

#define MAX_ROWS 64

static long g_rows = 0, g_errors = 0;

static void count(pa_status st, int nrows)
{
    if (st)
        g_errors++; /* refusals are part of the surface: their text is built */
    else
        g_rows += nrows;
}

static void query(pa_plan *p, int off)
{
    int64_t rows[MAX_ROWS][4];
    int nrows = 0;
    const void *srcs[5];
    void *dsts[5], *fields[5];
    for (int f = 0; f < 5; f++) {
        srcs[f] = (const void *)(uintptr_t)((1u << 24) + (f << 20) + off * f);
        dsts[f] = (void *)(uintptr_t)((2u << 24) + (f << 20) + off * (f + 1));
        fields[f] = dsts[f];
    }
    void *aos = (void *)(uintptr_t)((3u << 24) + off);
    pa_plan_set_buffers(p, (void *)(uintptr_t)(4u << 24),
                        (void *)(uintptr_t)((5u << 24) + off));
    for (int n = 1; n <= 3; n += 2)
        for (int stage = 0; stage < 3; stage++)
            count(pa_plan_stage_launches(p, n, stage, srcs, dsts, MAX_ROWS,
                                         rows, &nrows), nrows);
    for (int n = 2; n <= 5; n += 3)
        for (int dir = PA_SOA_SPLIT; dir <= PA_SOA_JOIN; dir++)
            for (int stage = 0; stage < 3; stage++)
                count(pa_plan_stage_launches_soa(
                          p, n, dir, stage, aos,
                          (const void *const *)fields, MAX_ROWS, rows,
                          &nrows), nrows);
}

int main(void)
{
    const int64_t dims[3] = {5, 7, 6}, pdims[2] = {2, 3};
    const int32_t decomp_i[2] = {1, 2}, decomp_o[2] = {0, 2};
    const int32_t perm_o[3] = {1, 2, 0};
    const int64_t keep_a[3] = {2, 7, 2}, keep_b[3] = {1, 0, 2};
    const int64_t extra[1] = {3};

    pa_topology *topo;
    pa_pencil *pin, *pout;
    if (pa_topology_create(2, pdims, &topo) ||
        pa_pencil_create(topo, 3, dims, decomp_i, NULL, &pin) ||
        pa_pencil_create(topo, 3, dims, decomp_o, perm_o, &pout)) {
        fprintf(stderr, "setup failed: %s\n", pa_last_error());
        return 1;
    }
    for (int rank = 0; rank < pa_topology_nranks(topo); rank++)
        for (int e = 0; e <= 1; e++) {
            pa_plan *pl[9] = {0};
            int np = 0;
            pa_status st = 0;
            st |= pa_plan_create(pin, pout, 8, e, extra, rank, 0, &pl[np++]);
            st |= pa_plan_create_comp(pin, pout, 4, 3, e, extra, rank, 0,
                                      &pl[np++]);
            st |= pa_plan_create_wire(pin, pout, PA_WIRE_F32_F16, 2, e, extra,
                                      rank, 0, &pl[np++]);
            st |= pa_plan_create_wire(pin, pout, PA_WIRE_F64_F32, 1, e, extra,
                                      rank, PA_PLAN_GROUP_CVT, &pl[np++]);
            st |= pa_plan_create_comp(pin, pout, 4, 2, e, extra, rank, 0,
                                      &pl[np++]);
            if (!st) st |= pa_plan_set_scale(pl[np - 1], PA_SCALAR_F32, 0.5);
            st |= pa_plan_create_keep(pin, pout, 8, 1, e, extra, rank, 0,
                                      keep_a, keep_b, PA_FILL_ZERO, &pl[np++]);
            st |= pa_plan_create(pin, pout, 4, e, extra, rank,
                                 PA_PLAN_GROUP_SOA, &pl[np++]);
            st |= pa_plan_create(pin, pout, 8, e, extra, rank, 0, &pl[np++]);
            st |= pa_plan_create_keep(pin, pout, 4, 1, e, extra, rank,
                                      PA_PLAN_GROUP_SOA, keep_a, keep_b,
                                      PA_FILL_ZERO, &pl[np++]);
            if (st) {
                fprintf(stderr, "plan creation failed: %s\n", pa_last_error());
                return 1;
            }
            for (int i = 0; i < np; i++) {
                for (int off = 0; off <= 8; off += 4) query(pl[i], off);
                pa_plan_destroy(pl[i]);
            }
        }
    pa_pencil_destroy(pin);
    pa_pencil_destroy(pout);
    pa_topology_destroy(topo);
    printf("stage_host_check: %ld rows, %ld refusals\n", g_rows, g_errors);
    return g_rows > 0 ? 0 : 1;
}
