// TEST INFRASTRUCTURE ONLY.  Host build of the device-side 3-D grid planner: obca_amd/csrc/obca_plan3d.h compiled with -DOBCA_EMU, where every loop over a workgroup's
// threads is one sequential loop over the grid nodes (ascending, or descending with reverse = 1), the barriers are nothing and the wave reduction of the descent is a loop
// over the 26 neighbours.  tests/test_plan3d_cpu.py compares it with the host A* (obca_plan_astar3d) on a machine without a GPU; tests/test_gpu_plan3d.py compares the
// device with it bit for bit.  It is never linked into libobca_plan3d.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include "../../obca_amd/csrc/obca_plan3d.h"
using namespace obca;

static std::string g_err;

extern "C" {
const char *emu_plan3d_last_error() { return g_err.c_str(); }
int emu_plan3d_limits(int *maxcells, int *maxbox, int *nmax, int *ws_cap) { *maxcells = OBCA_PLAN3D_MAXCELLS; *maxbox = OBCA_PLAN3D_MAXBOX; *nmax = OBCA_PLAN3D_NMAX; *ws_cap = OBCA_PLAN3D_WS_CAP; return 0; }

// The batch calls of include/obca_plan3d.h, instance after instance.  pts: B x pstride.  field (may be NULL): B x ncell floats, the settled cost-to-go arrays.
// N = 0: paths only (B x cap x 3); N > 0: xWS (B x (N+1) x 12) too, the way-points go to paths if it is not NULL (cap must then be OBCA_PLAN3D_WS_CAP).
static int run(int B, int N, const double *starts, const double *goals, int pstride, int nBox, const double *boxes, double clear, const double *room, double res,
               double *paths, int cap, int *counts, int *sweeps, double *xWS, int reverse, float *field) {
    int dims[3];
    const char *bad = pl3::check_args(B, starts, goals, pstride, nBox, boxes, clear, room, res, cap, N, xWS != nullptr, dims);
    if (bad) { g_err = bad; return -1; }
    pl3::Grid G;
    G.nx = dims[0]; G.ny = dims[1]; G.nz = dims[2]; G.ncell = dims[0] * dims[1] * dims[2]; G.nBox = nBox; G.res = res; G.clear = clear;
    for (int i = 0; i < 3; i++) G.room[i] = room[i];
    G.boxes = nullptr;
    pl3::emu_reverse = reverse;
    std::vector<float> lds((size_t)G.ncell + 4);
    std::vector<double> in((size_t)PL3_IN_STRIDE(nBox)), own((size_t)cap * 3);
    for (int i = 0; i < B; i++) {
        for (size_t k = 0; k < lds.size(); k++) lds[k] = 1e30f;      // what a predecessor may have left: the kernel text must not care
        memcpy(in.data(), starts + (size_t)i * pstride, 3 * sizeof(double)); memcpy(in.data() + 3, goals + (size_t)i * pstride, 3 * sizeof(double));
        if (nBox) memcpy(in.data() + 6, boxes + (size_t)i * nBox * 6, (size_t)nBox * 6 * sizeof(double));
        int sw = 0;
        pl3::plan_instance(in.data(), G, lds.data(), paths ? paths + (size_t)i * cap * 3 : own.data(), cap, counts + i, &sw, xWS ? N : 0, xWS ? xWS + (size_t)i * (N + 1) * 12 : nullptr);
        if (sweeps) sweeps[i] = sw;
        if (field) memcpy(field + (size_t)i * G.ncell, lds.data() + 4, (size_t)G.ncell * sizeof(float));
    }
    pl3::emu_reverse = 0;
    return 0;
}

int emu_plan3d_paths_batch(int B, const double *starts, const double *goals, int nBox, const double *boxes, double clear, const double room[3], double res,
                           double *paths, int cap, int *counts, int *sweeps, int reverse, float *field) {
    return run(B, 0, starts, goals, 3, nBox, boxes, clear, room, res, paths, cap, counts, sweeps, nullptr, reverse, field);
}
int emu_plan3d_warm_start_batch(int B, int N, const double *x0, const double *xF, int nBox, const double *boxes, double clear, const double room[3], double res,
                                double *xWS, int *counts, double *paths /* may be NULL: B x OBCA_PLAN3D_WS_CAP x 3 */) {
    return run(B, N, x0, xF, 12, nBox, boxes, clear, room, res, paths, OBCA_PLAN3D_WS_CAP, counts, nullptr, xWS, 0, nullptr);
}
}
