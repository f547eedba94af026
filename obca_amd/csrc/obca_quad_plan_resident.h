// obca_quad_plan_resident.h -- the resident route of the quadcopter's grid planner (include/obca_quad_plan_resident.h is the ABI): the 3-D grid search of obca_plan3d.h run
// from what an uploaded quadcopter batch holds on the device, its resampled path written straight into the batch's warm start.  Nothing but the selection and two ints per
// instance crosses the bus.
//
// One workgroup of PL3_NT threads per SELECTED instance, the grid in that workgroup's dynamic LDS ((ncell + 4) floats), exactly as obca_plan3d_kernel.  Workgroup j works on
// instance i = sel[j] of the batch's problem records (QPH_* of obca_quad_solver.h, as quad_upload_range packs them):
//   start = prob[QPH_X0 .. +3), goal = prob[QPH_XF .. +3), the QOB = 5 boxes = the 30 doubles at QPH_OB, [xmax,ymax,zmax,-xmin,-ymin,-zmin] each -- the layout `blocked` reads.
// The search is pl3::plan_instance itself (occupancy, in-place relaxation, descent on wave 0), called WITHOUT a warm-start array: it writes the way-points (the rows behind
// the count as zeros), count and sweeps, and leaves the count in its fourth control word.  Step 4 is done here, because an instance without a path (count 0, -1, -2, -3) must
// keep its record to the last bit, where plan_instance would write zeros: only with count >= 2 stage k = 0 .. N gets prob[QPH_SIZE + 12 k + r], rows 0-2 from
// pl3::resample_stage, rows 3-11 zero (what obca_plan3d_warm_start_batch puts into xWS), and QPH_TWS gets the caller's time scale if there is one.  No other header word is
// ever written: QPH_TS, QPH_R, QPH_X0, QPH_XF, QPH_OB, QPH_DWS, QPH_DIST stay.
// A record whose start, goal or boxes are not finite: `blocked` compares, and a NaN passes every comparison as "not blocked" -- so the 36 numbers are tested here first and
// such an instance ends with count -2, no sweeps and its record untouched, alone.
// Every destination word has one writer (stage k belongs to thread k mod PL3_NT; an instance to one workgroup: the host refuses a selection with a duplicate), no atomics,
// and no a * b + c is contracted: obca_plan3d.h switches contraction off at file scope, so this header is included where that is already the rule (behind the parking
// planner's kernel text, last in obca_hip.hip).  The same text compiles for the host with -DOBCA_EMU (tests/emu/quad_plan_resident_emu.cpp): every loop over the threads is one sequential loop.
#pragma once
#include <vector>
#include "obca_quad_solver.h"
#include "obca_plan3d.h"

namespace obca {
namespace qpr {

static_assert(QOB <= OBCA_PLAN3D_MAXBOX && QOB * QL == 30 && QPH_OB + QOB * QL <= QPH_SIZE, "the record's boxes are the planner's: 5 of 6 doubles");
static_assert((OBCA_PLAN3D_MAXCELLS + 4) * sizeof(float) <= 160 * 1024, "the field and its control words must fit the LDS of one workgroup");
static_assert(OBCA_PLAN3D_NMAX == QNMAX, "the warm start's horizon limit is the quadcopter solve's");

// ---------------------------------------------------------------- argument checks (host code; the library and the emulation share them)
// NULL if the arguments are good (then dims are the grid's), else what is wrong.  B, N: the batch's; everything else as the caller gave it.  Touches nothing.
static inline const char *check_args(int B, int N, double clear, const double *room, double res, int cap, const int *sel, int n, const double *timeWS, const int *counts, int dims[3]) {
    if (!counts) return "NULL counts";
    const double origin[3] = {0.0, 0.0, 0.0};      // (the end points and boxes are the records': the kernel tests them, instance by instance)
    if (const char *bad = pl3::check_args(1, origin, origin, 3, 0, nullptr, clear, room, res, cap, N, 1, dims)) return bad;
    if (cap > OBCA_PLAN3D_WS_CAP) return "need cap <= OBCA_PLAN3D_WS_CAP (1024)";
    if (timeWS && !(*timeWS > 0 && *timeWS - *timeWS == 0.0)) return "timeWS must be finite and positive";
    if (sel) {
        if (n < 1 || n > B) return "need 1 <= n <= B with a selection";
        std::vector<char> seen((size_t)B, 0);
        for (int j = 0; j < n; j++) {
            if (sel[j] < 0 || sel[j] >= B) return "an index of sel outside 0 .. B - 1";
            if (seen[sel[j]]) return "an index twice in sel";
            seen[sel[j]] = 1;
        }
    }
    return nullptr;
}

PL3_FN bool all_finite(const double *p, int n) {
    bool ok = true;
    for (int q = 0; q < n; q++) ok = ok && (p[q] - p[q] == 0.0);
    return ok;
}

// prob: the instance's problem record (read: start, goal, boxes; written: the warm start and QPH_TWS, only if the instance has a path); G: the grid, nBox = QOB (boxes are
// set here); lds, path, cap, count, sweeps: plan_instance's; tws: NULL (QPH_TWS stays) or the time scale of the planned instances.
PL3_FN void plan_resident_instance(double *prob, int N, pl3::Grid G, float *lds, double *path, int cap, int *count, int *sweeps, const double *tws) {
    const double *start = prob + QPH_X0, *goal = prob + QPH_XF, *boxes = prob + QPH_OB;
    if (!all_finite(start, 3) || !all_finite(goal, 3) || !all_finite(boxes, QOB * QL)) {      // (every thread decides the same from the same numbers)
#ifdef OBCA_EMU
        for (int q = 0; q < 3 * cap; q++) path[q] = 0.0;
#else
        for (int q = (int)threadIdx.x; q < 3 * cap; q += PL3_NT) path[q] = 0.0;
#endif
        if (PL3_TID0) { *count = -2; if (sweeps) *sweeps = 0; }
        return;
    }
    pl3::plan_instance(start, goal, boxes, G, lds, path, cap, count, sweeps, 0, nullptr);
    const int K = ((const int *)lds)[3];      // written before plan_instance's last barrier, by no one since
    if (K < 2) return;
#ifdef OBCA_EMU
    for (int k = 0; k <= N; k++) {
#else
    for (int k = (int)threadIdx.x; k <= N; k += PL3_NT) {
#endif
        double p[3];
        pl3::resample_stage(path, K, N, k, p);
        double *x = prob + QPH_SIZE + QX * k;
        for (int r = 0; r < QX; r++) x[r] = r < 3 ? p[r] : 0.0;
    }
    if (tws && PL3_TID0) prob[QPH_TWS] = *tws;
}

#ifndef OBCA_EMU
// sel: n distinct indices in 0 .. B - 1 (checked on the host; an index outside is skipped here all the same); paths B x cap x 3, counts and sweeps B, by INSTANCE
__global__ __launch_bounds__(PL3_NT) void obca_quad_plan_resident_kernel(const int *sel, int n, int B, int N, double *prob, size_t s_prob, double clear, double room0, double room1, double room2,
                                                                         double res, int nx, int ny, int nz, double *paths, int cap, int *counts, int *sweeps, int has_tws, double tws) {
    extern __shared__ float qpr_lds[];
    const int j = blockIdx.x;
    if (j >= n) return;
    const int i = sel[j];
    if (i < 0 || i >= B) return;
    pl3::Grid G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.ncell = nx * ny * nz; G.nBox = QOB; G.res = res; G.clear = clear; G.room[0] = room0; G.room[1] = room1; G.room[2] = room2; G.boxes = nullptr;
    plan_resident_instance(prob + (size_t)i * s_prob, N, G, qpr_lds, paths + (size_t)i * cap * 3, cap, counts + i, sweeps + i, has_tws ? &tws : nullptr);
}
#endif

}  // namespace qpr
}  // namespace obca
