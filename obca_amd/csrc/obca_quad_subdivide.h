// obca_quad_subdivide.h -- a solved quadcopter instance on a finer horizon, on the device: the same NLP with N' = r N stages of length Ts / r, started from the solution.  The NLP
// holds the obstacle separation at the nodes only; the clearance kernel finds what is lost between them, and the remedy for a constraint held at the nodes is a finer grid
// (plus, for a box's rounded corner, a small margin on the radius).  One wavefront (64 lanes) per DESTINATION instance; obca_amd/validate.py (refine_quad) is the numpy statement.
// q_init_point (obca_quad_solver.h) reads only xWS, QPH_TWS, QPH_DWS and QPH_X0 of the problem record -- inputs restart at hover, multipliers in closed form --, so the
// refinement rewrites a problem record, as obca_quad_shift.h does.  Write q = k r + s, 0 <= s < r; q = r N is the last node (k = N, s = 0).
//   header   : every word of the source's record bit for bit, except QPH_TS = Ts / r (one fp64 division), QPH_R = R + margin (margin 0: the bits stay), QPH_TWS, QPH_DWS (by status)
//   xWS, status 0 (the source's last exit flag, info[7], is 1 or 2 and x, t of its iterate are finite):
//              s = 0: node k of the solution, bit for bit
//              rows 0-2, s > 0: x_k[i] + keep(tau x_k[6 + i]), tau = (double)s / (double)r * t * Ts with the SOURCE's Ts and the solution's t -- the expression the clearance
//                       kernel evaluates for sample (k, s) at substeps = r; the discretisation is forward Euler, so it is also the partial step: the refined NLP constrains
//                       the very points clearance(substeps = r) looked at
//              rows 3-11, s > 0: x_k[i] + keep((double)s / (double)r * (x_{k+1}[i] - x_k[i]))
//              keep() stops the product from fusing into the sum (the solver's SEAM);  TWS = the solution's t, DWS = 1, as in the shift
//   status 1 : the exit flag is 0, or x / t of the iterate hold a non-finite number (with exit flag 0 NOTHING is read from the iterate): all 12 rows are the linear
//              interpolation, by the formula of rows 3-11, of the source's own uploaded xWS; TWS and DWS stay as uploaded
//   status -1: that xWS is not finite either: xWS = 0, TWS = 1, DWS = 1
// Every destination word has exactly one writer (word i of a range belongs to the lane that is dealt item i); source and destination are different buffers: no
// synchronisation.  `rev` deals the items to the lanes backwards: the host build's test asks for the same bits.  No transcendental is called.
// The same text compiles for the host (-DOBCA_EMU: QPAR is a loop over the lanes) for tests/emu/quad_subdivide_emu.cpp.  Nothing here is used by the solve kernels.
#pragma once
#include "obca_quad_solver.h"

namespace obca {
namespace qsd {

static_assert(QNT == 64, "one wavefront per instance: wred_max reduces over 64 lanes");

#define QSD_MAXFACTOR 32      // largest factor (= OBCA_QUAD_SUBDIVIDE_MAXFACTOR of include/obca_quad_subdivide.h)

OBCA_FN double sd_keep(double x) { SEAM(x); return x; }                      // a product that must not fuse with the sum it enters
OBCA_FN double sd_bad(double v) { return v - v == 0.0 ? 0.0 : 1.0; }         // 1 for NaN and +-inf
// item of lane `lane` in round rd of `rounds`: ascending, or (rev) dealt backwards -- lanes and rounds
OBCA_FN int sd_item(int rd, int rounds, int lane, int rev) { return rev ? (rounds - 1 - rd) * QNT + (QNT - 1 - lane) : rd * QNT + lane; }
#define QSD_DEAL(it, n, lane, rev) for (int rounds_ = ((n) + QNT - 1) / QNT, rd_ = 0, it; rd_ < rounds_; rd_++) if ((it = qsd::sd_item(rd_, rounds_, lane, rev)) < (n))

// the refusals of the entry points, one text for the library and the host build: n instances of horizon N by `factor`, the radius widened by `margin`
static inline const char *subdivide_check_args(int n, int N, int factor, double margin) {
    if (n < 1) return "need n >= 1";
    if (factor < 1 || factor > QSD_MAXFACTOR) return "need 1 <= factor <= 32";
    if (N < 1 || N > QNMAX || factor * N > QNMAX) return "need N >= 1 and factor * N <= OBCA_QUAD_NMAX";
    if (!(margin - margin == 0.0) || margin < 0.0) return "need a finite margin >= 0";
    return nullptr;
}

// 1 if one of the `cnt` doubles at v is NaN or +-inf (wave-uniform)
OBCA_FN double sd_scan(const double *v, int cnt) {
    double b[OBCA_NL];
    QPAR(lane) {
        double a = 0.0;
        for (int i = lane; i < cnt; i += QNT) { const double w = sd_bad(v[i]); a = w > a ? w : a; }
        b[LI(lane)] = a;
    }
    return wred_max(b);
}

// The trajectory.  x: 12 x (N + 1) stage-contiguous; ts[k * tstride] is timeScale[k] (nullptr: 1; tstride 0: one t); euler: rows 0-2 take the partial Euler step, else they
// are interpolated like the rest; xf: 12 x (r N + 1).  Lanes take the words of xf in rounds; consecutive lanes read consecutive words of node k and of node k + 1.
// Needs N >= 1, r >= 1.
OBCA_FN void subdivide_states(int N, int r, double Ts, const double *x, const double *ts, int tstride, bool euler, int rev, double *xf) {
    const int nW = QX * (N * r + 1);
    QPAR(lane) {
        QSD_DEAL(i, nW, lane, rev) {
            const int q = i / QX, c = i - q * QX, k = q / r, s = q - k * r;      // (q = r N: k = N, s = 0)
            const double xk = x[QX * k + c];
            double v = xk;
            if (s) {
                const double f = (double)s / (double)r;
                if (euler && c < 3) { const double tau = f * (ts ? ts[k * tstride] : 1.0) * Ts; v = xk + sd_keep(tau * x[QX * k + 6 + c]); }
                else v = xk + sd_keep(f * (x[QX * (k + 1) + c] - xk));
            }
            xf[i] = v;
        }
    }
}

// One instance of the host-pointer call: Ts' = Ts / r and the trajectory.  A non-finite number among Ts, x, timeScale marks the instance: its outputs are NaN.  Returns 0 / 1.
OBCA_FN int subdivide_host_instance(int N, int r, double Ts, const double *x, const double *ts, int rev, double *Tsf, double *xf) {
    double bad = sd_bad(Ts);
    if (bad == 0.0) bad = sd_scan(x, QX * (N + 1));
    if (bad == 0.0 && ts) bad = sd_scan(ts, N + 1);
    if (bad != 0.0) {
        const double nan_ = __builtin_nan("");
        QPAR(lane) {
            QSD_DEAL(i, QX * (N * r + 1), lane, rev) xf[i] = nan_;
            if (lane == 0) *Tsf = nan_;
        }
        return 1;
    }
    subdivide_states(N, r, Ts, x, ts, 1, true, rev, xf);
    QPAR(lane) { if (lane == 0) *Tsf = Ts / (double)r; }
    return 0;
}

// The resident call.  ps: the source's problem record (QPH_* header, then xWS 12 x (N + 1)), zs: its last iterate, info: the 8 doubles of its last solve; pd: the
// destination's problem record (horizon r N), every word of which is written.  Returns the slot's status.  Needs N >= 1, r >= 1, r N <= QNMAX.
OBCA_FN int subdivide_record(int N, int r, double margin, const double *ps, const double *zs, const double *info, int rev, double *pd) {
    quad::QLay l; quad::q_make_layout(N, l);
    int st = 1;
    if (info[7] == 1.0 || info[7] == 2.0) st = (sd_bad(zs[l.t]) != 0.0 || sd_scan(zs + l.x, QX * (N + 1)) != 0.0) ? 1 : 0;
    if (st && sd_scan(ps + QPH_SIZE, QX * (N + 1)) != 0.0) st = -1;
    const double Ts = ps[QPH_TS], R = ps[QPH_R];
    const double tws = st == 0 ? zs[l.t] : (st < 0 ? 1.0 : ps[QPH_TWS]), dws = st ? (st < 0 ? 1.0 : ps[QPH_DWS]) : 1.0;
    QPAR(lane) {
        QSD_DEAL(i, QPH_SIZE, lane, rev)
            pd[i] = i == QPH_TS ? Ts / (double)r : (i == QPH_R ? (margin != 0.0 ? R + margin : R) : (i == QPH_TWS ? tws : (i == QPH_DWS ? dws : ps[i])));
        if (st < 0) { QSD_DEAL(i, QX * (N * r + 1), lane, rev) pd[QPH_SIZE + i] = 0.0; }
    }
    if (st == 0) subdivide_states(N, r, Ts, zs + l.x, zs + l.t, 0, true, rev, pd + QPH_SIZE);
    else if (st == 1) subdivide_states(N, r, Ts, ps + QPH_SIZE, nullptr, 0, false, rev, pd + QPH_SIZE);
    return st;
}

}  // namespace qsd
}  // namespace obca
