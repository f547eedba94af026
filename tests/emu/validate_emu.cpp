// TEST INFRASTRUCTURE ONLY.  Host build of the device-side feasibility checks: obca_amd/csrc/obca_validate.h compiled with -DOBCA_EMU, where every PAR(lane)
// region is a plain loop over the 64 lanes and the wave reductions pair the lanes in the kernel's order.  tests/test_validate_emu_cpu.py compares it with the numpy
// checkers of obca_amd/validate.py on a machine without a GPU.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include "../../obca_amd/csrc/obca_validate.h"
using namespace obca;

extern "C" {
int emu_validate_sizes(int *pv_ncls, int *pv_out, int *qv_ncls, int *qv_out) { *pv_ncls = PV_NCLS; *pv_out = PV_OUT; *qv_ncls = QV_NCLS; *qv_out = QV_OUT; return 0; }
// prob / z: one instance as tests/packing.py packs it; rl (M), ts (N + 1), sl (nOb x (N + 1)) may be NULL, as in the kernel
void emu_validate_parking(int N, const double *prob, const double *z, const double *rl, const double *ts, const double *sl, double tol, double *out) {
    val::validate_parking_instance(N, prob, z, rl, ts, sl, tol, out);
}
void emu_validate_quad(int N, const double *prob, const double *x, const double *u, const double *ts, int tstride, const double *lam, double tol, double *out) {
    val::validate_quad_instance(N, prob, x, u, ts, tstride, lam, tol, out);
}
}
