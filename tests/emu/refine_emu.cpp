// TEST INFRASTRUCTURE ONLY.  Host build of the refinement of a solved parking instance onto a finer horizon: obca_amd/csrc/obca_refine.h compiled with -DOBCA_EMU, where every
// PAR(lane) region is a plain loop over the 64 lanes and SYNC is nothing.  tests/test_refine_cpu.py compares it with the numpy statement validate.refine_parking on a machine
// without a GPU, tests/test_gpu_refine.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include "../../obca_amd/csrc/obca_refine.h"
using namespace obca;

static std::string g_rf_err;

extern "C" {
const char *emu_refine_last_error() { return g_rf_err.c_str(); }
int emu_refine_sizes(int *maxfactor, int *nmax, int *hdr) { *maxfactor = RF_MAXFACTOR; *nmax = OB_NMAX; *hdr = OB_HDR; return 0; }
// the shared refusals alone
int emu_refine_check_args(int n, int N, int factor, int duals) {
    if (const char *bad = rfn::refine_check_args(n, N, factor, duals)) { g_rf_err = bad; return -1; }
    return 0;
}
// one instance of the host-pointer call: x 4 x (N + 1), u 2 x N, ts (N + 1) or NULL; rev: deal the items to the lanes backwards.  Returns 0, or 1 for a marked instance.
int emu_refine_host(int N, int factor, double Ts, double L, const double *x, const double *u, const double *ts, int rev, double *Tsf, double *xf, double *uf) {
    if (const char *bad = rfn::refine_check_args(1, N, factor, 0)) { g_rf_err = bad; return -1; }
    if (!x || !u || !Tsf || !xf || !uf) { g_rf_err = "NULL argument"; return -1; }
    return rfn::refine_host_instance(N, factor, Ts, L, x, u, ts, rev, Tsf, xf, uf);
}
// one instance of the resident call: prob / z / z0 as tests/packing.py packs them at horizon N, info (8); pd: OB_HDR + 3 (factor N + 1) doubles, zd: zlen doubles.
// The slot's status goes to *status.
int emu_refine_record(int N, int factor, int duals, const double *prob, const double *z, const double *z0, const double *info, int rev, double *pd, double *zd, int zlen, int *status) {
    if (const char *bad = rfn::refine_check_args(1, N, factor, duals)) { g_rf_err = bad; return -1; }
    if (!prob || !z || !z0 || !info || !pd || !zd || !status) { g_rf_err = "NULL argument"; return -1; }
    Lay l; make_layout(N * factor, (int)prob[PH_NOB], (int)prob[PH_M], l);
    if (zlen < l.len) { g_rf_err = "the destination row is shorter than the instance's layout"; return -1; }
    *status = rfn::refine_record(N, factor, duals, prob, z, z0, info, rev, pd, zd, zlen);
    return 0;
}
}
