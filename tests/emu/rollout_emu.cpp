// TEST INFRASTRUCTURE ONLY.  Host build of the rollout on the continuous vehicle models: obca_amd/csrc/obca_rollout.h compiled with -DOBCA_EMU, where every PAR(lane) region
// is a plain loop over the 64 lanes, SYNC is nothing and the work buffer is the caller's memory.  tests/test_rollout_cpu.py compares it with the numpy statements of
// obca_amd/validate.py on a machine without a GPU, tests/test_gpu_rollout.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include "../../obca_amd/csrc/obca_clearance.h"
#include "../../obca_amd/csrc/obca_rollout.h"
using namespace obca;

static std::string g_ro_err;

extern "C" {
const char *emu_rollout_last_error() { return g_ro_err.c_str(); }
int emu_rollout_sizes(int *out, int *clr, int *smax) { *out = RO_OUT; *clr = RO_CLR; *smax = CL_SMAX; return 0; }
// one instance: prob / z as tests/packing.py packs them (x, u and t of z are read), ts (N + 1) or NULL; vmax: the widest obstacle of the BATCH the instance belongs to;
// rev: deal the clearance items to the lanes backwards; pose 3 x (N S + 1), X (N + 1) x 4: the work buffer's slices
int emu_rollout_parking(int N, const double *prob, const double *z, const double *ts, int vmax, int substeps, int restart, double need, int rev, double *pose, double *X, double *out) {
    if (const char *bad = roll::rollout_check_args(substeps, restart, need)) { g_ro_err = bad; return -1; }
    if (N < 1 || N > OB_NMAX || !prob || !z || !pose || !X || !out) { g_ro_err = "need 1 <= N <= OBCA_NMAX and no NULL argument"; return -1; }
    if (vmax <= 2) roll::rollout_parking_instance<2>(N, prob, z, ts, substeps, restart, need, rev, pose, X, out);
    else if (vmax <= OB_VMID) roll::rollout_parking_instance<OB_VMID>(N, prob, z, ts, substeps, restart, need, rev, pose, X, out);
    else roll::rollout_parking_instance<OB_VMAX>(N, prob, z, ts, substeps, restart, need, rev, pose, X, out);
    return 0;
}
// one instance: prob as tests/packing.py packs it (Ts, R and the boxes are read), x (N + 1) x 12, u N x 4, ts[k * tstride]
int emu_rollout_quad(int N, const double *prob, const double *x, const double *u, const double *ts, int tstride, int substeps, int restart, double need, int rev,
                     double *pose, double *X, double *out) {
    if (const char *bad = roll::rollout_check_args(substeps, restart, need)) { g_ro_err = bad; return -1; }
    if (N < 1 || N > QNMAX || !prob || !x || !u || !ts || !pose || !X || !out) { g_ro_err = "need 1 <= N <= OBCA_QUAD_NMAX and no NULL argument"; return -1; }
    roll::rollout_quad_instance(N, prob, x, u, ts, tstride, substeps, restart, need, rev, pose, X, out);
    return 0;
}
}
