// obca_quad_shift.h -- receding-horizon restart of the quadcopter batch (not in the reference): the warm start of the NEXT solve is written into the
// problem record from the LAST solution, one wavefront (64 lanes) per instance, entirely on the device.  q_init_point (obca_quad_solver.h) reads all 12 rows of xWS per stage
// from prob[QPH_SIZE ...] and QPH_TWS / QPH_DWS / QPH_X0 from the header, so rewriting those words is the whole restart: neither interior-point kernel knows about it.
//   quad_shift_instance : last exit flag (info[7]) 1 or 2 -- stage k of the warm start becomes stage min(k + shift, N) of the solution (all 12 rows), TWS = the solution's t,
//                         DWS = 1 (the next solve starts lambda at the closed-form point-to-box duals of the NEW positions; inputs restart at hover and slacks at 1 as
//                         q_init_point always does: carrying u / lambda / s would need another starting point in the kernel);
//                         exit flag 0 -- warm start, TWS and DWS stay what was uploaded, and NOTHING is read from the iterate (it may be non-finite);
//                         every instance -- X0 = x0_new, else stage `shift` of the solution (exit flag 0 without x0_new: unchanged); XF = xF_new if given (a moving goal), and the
//                         tail stages k + shift > N of a shifted warm start then hold xF_new instead of the old terminal stage.  No other header word is touched.
// Source (z, info) and destination (prob) are different buffers and every destination word has one writer: no in-place hazard, no synchronisation.
// The same text compiles for the host (-DOBCA_EMU: QPAR is a loop over the lanes) for tests/emu/quad_shift_emu.cpp.  Nothing here is used by the solve kernels.
#pragma once
#include "obca_quad_solver.h"

namespace obca {
namespace quad {

// prob: problem record (QPH_* header, then xWS 12 x (N + 1)), read and written; z: last solution in the solver's layout; info: the 8 doubles of the last solve;
// x0_new / xF_new: 12 doubles each or nullptr.  Needs 0 <= shift <= N.
OBCA_FN void quad_shift_instance(int N, int shift, double *prob, const double *z, const double *info, const double *x0_new, const double *xF_new) {
    QLay l; q_make_layout(N, l);
    const bool solved = info[7] == 1.0 || info[7] == 2.0;
    QPAR(lane) {
        if (solved) {
            for (int i = lane; i < QX * (N + 1); i += QNT) {
                const int k = i / QX, c = i - k * QX, ks = k + shift;
                prob[QPH_SIZE + i] = (ks > N && xF_new) ? xF_new[c] : z[l.x + QX * (ks < N ? ks : N) + c];
            }
            if (lane == 0) { prob[QPH_TWS] = z[l.t]; prob[QPH_DWS] = 1.0; }
        }
        if (lane < QX) {
            if (x0_new) prob[QPH_X0 + lane] = x0_new[lane];
            else if (solved) prob[QPH_X0 + lane] = z[l.x + QX * shift + lane];
            if (xF_new) prob[QPH_XF + lane] = xF_new[lane];
        }
    }
}

}  // namespace quad
}  // namespace obca
