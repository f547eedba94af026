// TEST INFRASTRUCTURE ONLY.  Host build of the quadcopter receding-horizon shift: obca_amd/csrc/obca_quad_shift.h compiled with -DOBCA_EMU, where the QPAR(lane) region is a
// plain loop over the 64 lanes.  tests/test_quad_shift_cpu.py compares it bit for bit with a numpy statement of the same rules, and the GPU tests build the checker's
// starting point with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include "../../obca_amd/csrc/obca_quad_shift.h"
using namespace obca;

extern "C" {
int emu_quad_shift_sizes(int N, int *prob_len, int *z_len, int *ox, int *ot) {
    quad::QLay l; quad::q_make_layout(N, l);
    *prob_len = QPH_SIZE + QX * (N + 1); *z_len = l.len; *ox = l.x; *ot = l.t;
    return 0;
}
// prob (rw) / z / info: one instance as tests/packing.py packs it; x0_new / xF_new: 12 doubles or NULL, as in the kernel
void emu_quad_shift(int N, int shift, double *prob, const double *z, const double *info, const double *x0_new, const double *xF_new) {
    quad::quad_shift_instance(N, shift, prob, z, info, x0_new, xF_new);
}
}
