// obca_shift.h -- receding-horizon restart of the parking batch (not in the reference): the warm start of the NEXT solve is the LAST solution advanced by
// `shift` stages, written on the device, one wavefront (64 lanes) per instance.  The next solve starts from the start iterate z0 and the problem record, so rewriting those
// is the whole restart: neither interior-point kernel knows about it.  With N1 = N + 1, M rows and nOb obstacles of THIS instance (PH_M, PH_NOB of its own record):
//   x        : stage k = 1..N of z0 is stage min(k + shift, N) of the solution (4 words each); stage 0 holds X0 (below)
//   u        : interval k = 0..N-1 is interval min(k + shift, N - 1) of the solution; an interval past the end (k + shift > N - 1) keeps the last steering angle and has
//              acceleration 0: the car stands at the goal
//   lam, mu  : stage k is stage min(k + shift, N) of the solution, M and 4 nOb words per stage -- the instance's own counts, whatever the batch's widest instance has;
//              lambda stays in the solver's scaling (unit-length rows), as the iterate holds it
//   t        : 1, as every start of this project has it (ParkingSignedDist.jl:214)
//   the rest of the primal part (sl -- in ParkingDist the slack of the norm row --, so, ss): 0.  Nothing behind the primal part (l.nprimal) is written: the multipliers of a
//              start are what the upload left there (zeros), and the solve initialises them itself
//   rx,ry,ryaw: word k = 0..N of each is word min(k + shift, N) of the same array: the tracking reference advances with the states
//   X0       : x0_new (the measured state), or without one stage min(shift, N) of the solution
// No other word of the problem record is touched, and of the solution only x, u, lam and mu are read: multipliers, slacks, t and sl of the last iterate are never looked at.
// The exit flag of the last solve is NOT consulted: an unconverged but finite iterate (an iteration limit, a solve cut short on purpose) is a legitimate restart, and a
// non-finite one gives a non-finite start of that instance alone, which its next solve reports with exit flag 0.
// In-place hazard: the reference is read and written in the SAME buffer (prob), and word k is the source of word k - shift that another lane writes.  So every lane first
// copies its advanced words into `tmp` (the direction buffer of the instance: free between two solves), the wavefront synchronises, and only then the words go back.  Everything
// else moves between different buffers (z -> z0, prob), and every destination word has exactly one writer: the lane that is dealt item i of a range.  `rev` deals the items
// to the lanes backwards: the host build's test asks for the same bits.
// The same text compiles for the host (-DOBCA_EMU: PAR is a loop over the lanes, SYNC nothing) for tests/emu/shift_emu.cpp.  Nothing here is used by the solve kernels.
#pragma once
#include "obca_solver.h"

namespace obca {
namespace shf {

// item of lane `lane` in round rd of `rounds`: ascending, or (rev) dealt backwards -- lanes and rounds
OBCA_FN int sh_item(int rd, int rounds, int lane, int rev) { return rev ? (rounds - 1 - rd) * OB_NT + (OB_NT - 1 - lane) : rd * OB_NT + lane; }
#define SH_DEAL(it, n, lane, rev) for (int rounds_ = ((n) + OB_NT - 1) / OB_NT, rd_ = 0, it; rd_ < rounds_; rd_++) if ((it = shf::sh_item(rd_, rounds_, lane, rev)) < (n))
OBCA_FN int sh_min(int a, int b) { return a < b ? a : b; }

// prob: problem record (header | rx | ry | ryaw), read and written; z: last iterate in the solver's layout; z0: start iterate of the next solve; tmp: 3 (N + 1) doubles of
// scratch; x0_new: 4 doubles or nullptr.  Needs N >= 1 and 0 <= shift <= N.
OBCA_FN void shift_instance(int N, int shift, double *prob, const double *z, double *z0, double *tmp, const double *x0_new, int rev) {
    const int nOb = (int)prob[PH_NOB], M = (int)prob[PH_M], N1 = N + 1, W = 4 * nOb;
    Lay l; make_layout(N, nOb, M, l);
    PAR(lane) {
        SH_DEAL(i, 3 * N1, lane, rev) { const int a = i / N1, k = i - a * N1; tmp[i] = prob[OB_HDR + a * N1 + sh_min(k + shift, N)]; }
    }
    SYNC();      // every advanced word of the reference is in tmp before the first one is overwritten
    PAR(lane) {
        SH_DEAL(i, 3 * N1, lane, rev) prob[OB_HDR + i] = tmp[i];
        SH_DEAL(i, 4 * N1, lane, rev) {
            const int k = i / 4, c = i - 4 * k;
            const double v = (k == 0 && x0_new) ? x0_new[c] : z[l.x + 4 * sh_min(k + shift, N) + c];
            z0[l.x + i] = v;
            if (k == 0) prob[PH_X0 + c] = v;      // stage 0 of the warm start holds X0
        }
        SH_DEAL(i, 2 * N, lane, rev) {
            const int k = i / 2, c = i - 2 * k;
            z0[l.u + i] = (c == 1 && k + shift > N - 1) ? 0.0 : z[l.u + 2 * sh_min(k + shift, N - 1) + c];
        }
        if (lane == 0) z0[l.t] = 1.0;
        SH_DEAL(i, M * N1, lane, rev) { const int k = i / M, c = i - k * M; z0[l.lam + i] = z[l.lam + sh_min(k + shift, N) * M + c]; }
        SH_DEAL(i, W * N1, lane, rev) { const int k = i / W, c = i - k * W; z0[l.mu + i] = z[l.mu + sh_min(k + shift, N) * W + c]; }
        SH_DEAL(i, l.nprimal - l.sl, lane, rev) z0[l.sl + i] = 0.0;
    }
}

}  // namespace shf
}  // namespace obca
