// TEST INFRASTRUCTURE ONLY.  Host build of the refinement of a solved quadcopter instance onto a finer horizon: obca_amd/csrc/obca_quad_subdivide.h compiled with -DOBCA_EMU,
// where every QPAR(lane) region is a plain loop over the 64 lanes.  tests/test_quad_refine_cpu.py compares it with the numpy statement validate.refine_quad on a machine
// without a GPU, tests/test_gpu_quad_refine.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include "../../obca_amd/csrc/obca_quad_subdivide.h"
using namespace obca;

static std::string g_sd_err;

extern "C" {
const char *emu_quad_subdivide_last_error() { return g_sd_err.c_str(); }
int emu_quad_subdivide_sizes(int *maxfactor, int *nmax, int *hdr) { *maxfactor = QSD_MAXFACTOR; *nmax = QNMAX; *hdr = QPH_SIZE; return 0; }
// the shared refusals alone
int emu_quad_subdivide_check_args(int n, int N, int factor, double margin) {
    if (const char *bad = qsd::subdivide_check_args(n, N, factor, margin)) { g_sd_err = bad; return -1; }
    return 0;
}
// one instance of the host-pointer call: x 12 x (N + 1) stage-contiguous, ts (N + 1) or NULL; rev: deal the items to the lanes backwards.  Returns 0, or 1 for a marked instance.
int emu_quad_subdivide_host(int N, int factor, double Ts, const double *x, const double *ts, int rev, double *Tsf, double *xf) {
    if (const char *bad = qsd::subdivide_check_args(1, N, factor, 0.0)) { g_sd_err = bad; return -1; }
    if (!x || !Tsf || !xf) { g_sd_err = "NULL argument"; return -1; }
    return qsd::subdivide_host_instance(N, factor, Ts, x, ts, rev, Tsf, xf);
}
// one instance of the resident call: prob / z as tests/packing.py packs them at horizon N, info (8); pd: QPH_SIZE + 12 (factor N + 1) doubles.  The slot's status goes to *status.
int emu_quad_subdivide_record(int N, int factor, double margin, const double *prob, const double *z, const double *info, int rev, double *pd, int *status) {
    if (const char *bad = qsd::subdivide_check_args(1, N, factor, margin)) { g_sd_err = bad; return -1; }
    if (!prob || !z || !info || !pd || !status) { g_sd_err = "NULL argument"; return -1; }
    *status = qsd::subdivide_record(N, factor, margin, prob, z, info, rev, pd);
    return 0;
}
}
