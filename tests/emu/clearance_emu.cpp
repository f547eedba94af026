// TEST INFRASTRUCTURE ONLY.  Host build of the between-node clearance check: obca_amd/csrc/obca_clearance.h compiled with -DOBCA_EMU, where every PAR(lane) region is a plain
// loop over the 64 lanes, SYNC is nothing and the LDS marks are a local array.  tests/test_clearance_cpu.py compares it with the numpy statements of obca_amd/validate.py and
// the oracle's DualMultWS on a machine without a GPU, tests/test_gpu_clearance.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include "../../obca_amd/csrc/obca_clearance.h"
using namespace obca;

static std::string g_cl_err;

extern "C" {
const char *emu_clearance_last_error() { return g_cl_err.c_str(); }
int emu_clearance_sizes(int *out, int *smax, int *npo) { *out = CL_OUT; *smax = CL_SMAX; *npo = CL_NPO; return 0; }
// one instance: prob / z as tests/packing.py packs them (x, u and t of z are read), ts (N + 1) or NULL; vmax: the widest obstacle of the BATCH the instance belongs to
// (the row class, as launch_dualws picks it); rev: deal the items to the lanes backwards
int emu_clearance_parking(int N, const double *prob, const double *z, const double *ts, int vmax, int substeps, double need, int rev, double *out) {
    if (const char *bad = clr::clearance_check_args(substeps, need)) { g_cl_err = bad; return -1; }
    if (N < 1 || N > OB_NMAX || !prob || !z || !out) { g_cl_err = "need 1 <= N <= OBCA_NMAX and no NULL argument"; return -1; }
    if (vmax <= 2) clr::clearance_parking_instance<2>(N, prob, z, ts, substeps, need, rev, out);
    else if (vmax <= OB_VMID) clr::clearance_parking_instance<OB_VMID>(N, prob, z, ts, substeps, need, rev, out);
    else clr::clearance_parking_instance<OB_VMAX>(N, prob, z, ts, substeps, need, rev, out);
    return 0;
}
// one instance: prob as tests/packing.py packs it (Ts, R and the boxes are read), x (N + 1) x 12, ts[k * tstride]
int emu_clearance_quad(int N, const double *prob, const double *x, const double *ts, int tstride, int substeps, double need, int rev, double *out) {
    if (const char *bad = clr::clearance_check_args(substeps, need)) { g_cl_err = bad; return -1; }
    if (N < 1 || N > QNMAX || !prob || !x || !ts || !out) { g_cl_err = "need 1 <= N <= OBCA_QUAD_NMAX and no NULL argument"; return -1; }
    clr::clearance_quad_instance(N, prob, x, ts, tstride, substeps, need, rev, out);
    return 0;
}
}
