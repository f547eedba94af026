// TEST INFRASTRUCTURE ONLY.  Host build of the quadcopter planner's RESIDENT route (obca_quad_batch_grid_plan_warm_start, include/obca_quad_plan_resident.h):
// obca_amd/csrc/obca_quad_plan_resident.h over obca_plan3d.h compiled with -DOBCA_EMU -- every loop over a workgroup's threads one sequential loop, the barriers nothing --,
// run over problem records as tests/packing.pack_quad_problem packs them, in the order the host layer does it: the shared argument check, -4 / 0 in every count / sweep and
// zeros in the path buffer, then the selected instances one after the other.  tests/test_quad_plan_resident_cpu.py checks the route with it on a machine without a GPU,
// tests/test_gpu_quad_plan_resident.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include "../../obca_amd/csrc/obca_quad_plan_resident.h"
#include "../../include/obca_quad_plan_resident.h"
using namespace obca;

static std::string g_qpr_err;

extern "C" {
const char *emu_qpr_last_error() { return g_qpr_err.c_str(); }
// the record's words (QPH_TS, QPH_R, QPH_X0, QPH_XF, QPH_OB, QPH_TWS, QPH_DWS, QPH_DIST, QPH_SIZE), the skipped code and the threads of a workgroup
int emu_qpr_layout(int *out /* 11 */) {
    const int v[11] = {QPH_TS, QPH_R, QPH_X0, QPH_XF, QPH_OB, QPH_TWS, QPH_DWS, QPH_DIST, QPH_SIZE, OBCA_QUAD_PLAN_SKIPPED, PL3_NT};
    for (int i = 0; i < 11; i++) out[i] = v[i];
    return 0;
}
// obca_quad_batch_grid_plan_warm_start on host memory: prob B x s_prob are the batch's records (rewritten where the count is >= 2), paths B x cap x 3 its path buffer.
// reverse: the nodes of a sweep ascending (0) or descending (1).  lds_fill: what the "LDS" holds before every instance (the text must not care).
int emu_qpr_plan(int B, int N, double *prob, long long s_prob, double clear, const double *room, double res, int cap, const int *sel, int n, const double *timeWS,
                 int reverse, float lds_fill, double *paths, int *counts, int *sweeps) {
    int dims[3];
    if (B < 1 || !prob || !paths || s_prob < QPH_SIZE + (long long)QX * (N + 1) || reverse < 0 || reverse > 1) { g_qpr_err = "bad arguments of the emulation"; return -1; }
    if (const char *bad = qpr::check_args(B, N, clear, room, res, cap, sel, n, timeWS, counts, dims)) { g_qpr_err = bad; return -1; }
    if (!sel) n = B;
    pl3::Grid G;
    G.nx = dims[0]; G.ny = dims[1]; G.nz = dims[2]; G.ncell = dims[0] * dims[1] * dims[2]; G.nBox = QOB; G.res = res; G.clear = clear;
    for (int i = 0; i < 3; i++) G.room[i] = room[i];
    G.boxes = nullptr;
    for (int i = 0; i < B; i++) { counts[i] = OBCA_QUAD_PLAN_SKIPPED; if (sweeps) sweeps[i] = 0; }
    memset(paths, 0, sizeof(double) * 3 * (size_t)cap * B);
    std::vector<float> lds((size_t)G.ncell + 4);
    pl3::emu_reverse = reverse;
    for (int j = 0; j < n; j++) {
        const int i = sel ? sel[j] : j;
        for (size_t k = 0; k < lds.size(); k++) lds[k] = lds_fill;
        int sw = 0;
        qpr::plan_resident_instance(prob + (size_t)i * s_prob, N, G, lds.data(), paths + (size_t)i * cap * 3, cap, counts + i, &sw, timeWS);
        if (sweeps) sweeps[i] = sw;
    }
    pl3::emu_reverse = 0;
    return 0;
}
}
