// obca_validate.h -- a-posteriori feasibility checks of returned trajectories on the device: what obca_amd/validate.py computes with numpy, one
// wavefront (64 lanes) per instance.  Lanes take stages and (stage, obstacle) items, every constraint class ends in ONE wave reduction.
//   validate_parking_instance : the 13 classes of validate.parking_constraints_full in the conventions of validate.validate_parking, then `ref_worst`, the
//                               largest "should be <= 0" quantity of the reference's own acceptance test (ParkingConstraints.jl:29-149, quirks as in
//                               validate.parking_constraints_ref and ref_constraints of obca_solver_ipm.h)
//   validate_quad_instance    : the 9 classes of validate.validate_quadcopter (constrSatisfaction.jl:25-204)
// The point comes in the SOLVER's layout (problem header + iterate: unit-length half-space rows, one t) and the classes are reported in the CALLER's units:
// lambda is divided by the row lengths again where its own value is reported (dual_pos); A'lambda and b'lambda do not depend on the row scaling.
// A host-pointer call brings what the iterate cannot hold -- a timeScale per stage, the caller's slack -- in `ts` / `slv`.
// Every maximum propagates NaN (fmax would swallow it), and a non-finite entry anywhere in the point clears both flags.
// Transcendentals are libm's / the device library's sin, cos, tan: the solver's bounded-range versions hold on its own iterates only, a checked trajectory is arbitrary.
// The same text compiles for the host (-DOBCA_EMU: PAR is a loop over the lanes) for tests/emu/validate_emu.cpp.  Nothing here is used by the solve kernels.
#pragma once
#include "obca_solver.h"
#include "obca_quad_solver.h"

namespace obca {
namespace val {

static_assert(OB_NT == 64 && QNT == 64, "one wavefront per instance: wred_max reduces over 64 lanes");

#define PV_NCLS 14     // u_bounds, x_bounds, ts_bounds, ts_chain, dual_pos, start, end, dyn, steer_rate, norm, rot, sep, penetration, ref_worst
#define PV_OUT 16      // doubles per instance: the classes, then ok, ref_ok (0 / 1)
#define QV_NCLS 9      // start, end, u_bounds, x_bounds, dyn, ts_chain, dual_pos, norm, sep
#define QV_OUT 10      // the classes, then ok
#define PV_REF_TOL 5e-5   // ParkingConstraints.jl:133-139
enum { PV_U = 0, PV_X, PV_TSB, PV_TSC, PV_DUAL, PV_START, PV_END, PV_DYN, PV_STEER, PV_NORM, PV_ROT, PV_SEP, PV_PEN, PV_REF, PV_BAD, PV_NACC };
enum { QV_START = 0, QV_END, QV_U, QV_X, QV_DYN, QV_TSC, QV_DUAL, QV_NORM, QV_SEP, QV_BAD, QV_NACC };

OBCA_FN double vmax(double a, double b) { return (b > a || b != b) ? b : a; }      // NaN-propagating, like np.max
OBCA_FN double vbad(double v) { return (v - v == 0.0) ? 0.0 : 1.0; }               // 1 for NaN and +-inf

// ParkingSignedDist.jl:121-139 as validate._dyn states it
OBCA_FN void park_step(double Ts, double L, const double x[4], const double u[2], double ts, double F[4]) {
    const double q = ts * Ts, tn = tan(u[0]);
    const double s = x[3] + q / 2 * u[1];
    const double phi = x[2] + q / 2 * x[3] * tn / L;
    F[0] = x[0] + q * s * cos(phi); F[1] = x[1] + q * s * sin(phi); F[2] = x[2] + q * s * tn / L; F[3] = x[3] + q * u[1];
}

// p: problem header (PH_*), z: iterate in the solver's layout; rl: |a_r| of the M rows as the caller gave them (nullptr: 1);
// ts: the caller's timeScale per stage (N + 1; nullptr: the iterate's single t, 1 with fixTime -- what a download returns);
// slv: the caller's slack, nOb x (N + 1) stage-contiguous (nullptr: the iterate's); out: PV_OUT doubles.  Needs N >= 1.
OBCA_FN void validate_parking_instance(int N, const double *p, const double *z, const double *rl, const double *ts, const double *slv, double tol, double *out) {
    const int nOb = (int)p[PH_NOB], M = (int)p[PH_M], fix = p[PH_FIX] != 0.0, dist = p[PH_DIST] != 0.0;
    Lay l; make_layout(N, nOb, M, l);
    const double Ts = p[PH_TS], L = p[PH_L], off = p[PH_OFF], ninf = -HUGE_VAL;
    const double t1 = fix ? 1.0 : z[l.t], ts0 = ts ? ts[0] : t1;
    double acc[PV_NACC][OBCA_NL];
    PAR(lane) {
        double a[PV_NACC];
#pragma unroll
        for (int i = 0; i < PV_NACC; i++) a[i] = 0.0;      // |.| classes and the ones validate.py starts at 0 (norm, rot, sep); ref_worst holds c4 >= 0
        a[PV_U] = a[PV_X] = a[PV_DUAL] = a[PV_STEER] = a[PV_PEN] = ninf;
        if (!fix) a[PV_TSB] = ninf;
        double refsteer = ninf;
        // multipliers: lambda in the caller's row scaling
        for (int i = lane; i < M * (N + 1); i += OB_NT) { const double v = z[l.lam + i]; a[PV_DUAL] = vmax(a[PV_DUAL], -(rl ? v / rl[i % M] : v)); a[PV_BAD] = vmax(a[PV_BAD], vbad(v)); }
        for (int i = lane; i < 4 * nOb * (N + 1); i += OB_NT) { const double v = z[l.mu + i]; a[PV_DUAL] = vmax(a[PV_DUAL], -v); a[PV_BAD] = vmax(a[PV_BAD], vbad(v)); }
        // stages
        for (int k = lane; k <= N; k += OB_NT) {
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { x[i] = z[l.x + 4 * k + i]; a[PV_BAD] = vmax(a[PV_BAD], vbad(x[i])); }
            const double tc = ts ? ts[k] : t1;            // the caller's timeScale[k]; the full checker runs on 1 with fixTime
            const double tf = fix ? 1.0 : tc;
            a[PV_BAD] = vmax(a[PV_BAD], vbad(tc));
            a[PV_X] = vmax(a[PV_X], vmax(vmax(p[PH_XL] - x[0], x[0] - p[PH_XU]), vmax(p[PH_XL + 1] - x[1], x[1] - p[PH_XU + 1])));
            a[PV_X] = vmax(a[PV_X], vmax(p[PH_XL + 3] - x[3], x[3] - p[PH_XU + 3]));
            if (!fix) a[PV_TSB] = vmax(a[PV_TSB], vmax(OB_TL - tf, tf - OB_TU));
            a[PV_REF] = vmax(a[PV_REF], fabs(tc - 1) - 0.2);                                  // c0[3], :45
            if (k == 0) {
#pragma unroll
                for (int i = 0; i < 4; i++) a[PV_START] = vmax(a[PV_START], fabs(x[i] - p[PH_X0 + i]));
            }
            if (k == N) {
#pragma unroll
                for (int i = 0; i < 4; i++) a[PV_END] = vmax(a[PV_END], fabs(x[i] - p[PH_XF + i]));
            }
            if (k < N) {
                const double u[2] = {z[l.u + 2 * k], z[l.u + 2 * k + 1]};
                a[PV_BAD] = vmax(a[PV_BAD], vmax(vbad(u[0]), vbad(u[1])));
                a[PV_U] = vmax(a[PV_U], vmax(fabs(u[0]) - OB_UU0, fabs(u[1]) - OB_UU1));
                const double tcn = ts ? ts[k + 1] : t1, tfn = fix ? 1.0 : tcn;
                a[PV_TSC] = vmax(a[PV_TSC], fabs(tfn - tf));
                if (!fix) a[PV_REF] = vmax(a[PV_REF], fabs(tcn - tc));                       // c4, :83
                double F[4];
                park_step(Ts, L, x, u, tf, F);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const double r = fabs(z[l.x + 4 * (k + 1) + i] - F[i]);
                    a[PV_DYN] = vmax(a[PV_DYN], r);
                    if (fix || i == 3) a[PV_REF] = vmax(a[PV_REF], r);                        // variable time: only the speed row survives, :76-79
                }
                const double du = fabs(u[0] - (k ? z[l.u + 2 * k - 2] : 0.0));
                a[PV_STEER] = vmax(a[PV_STEER], du / (tf * Ts));
                refsteer = vmax(refsteer, fix ? du / Ts : du / (ts0 * Ts));                   // :88 divides by timeScale[1] only
            }
        }
        // (stage, obstacle) items
        for (int it = lane; it < (N + 1) * nOb; it += OB_NT) {
            const int k = it / nOb, j = it - k * nOb, v = (int)p[PH_VOB + j], r0 = (int)p[PH_ROFF + j];
            double p1 = 0, p2 = 0, beta = 0;
            for (int i = 0; i < v; i++) { const double lm = z[l.lam + k * M + r0 + i]; p1 += p[PH_A + 2 * (r0 + i)] * lm; p2 += p[PH_A + 2 * (r0 + i) + 1] * lm; beta += p[PH_B + r0 + i] * lm; }
            double mu[4];
#pragma unroll
            for (int i = 0; i < 4; i++) mu[i] = z[l.mu + 4 * it + i];
            const double X = z[l.x + 4 * k], Y = z[l.x + 4 * k + 1], psi = z[l.x + 4 * k + 2];
            const double sn = sin(psi), cs = cos(psi);
            const double pp = p1 * p1 + p2 * p2;
            const double r1 = fabs(mu[0] - mu[2] + cs * p1 + sn * p2), r2 = fabs(mu[1] - mu[3] - sn * p1 + cs * p2);
            const double row = -(p[PH_G] * mu[0] + p[PH_G + 1] * mu[1] + p[PH_G + 2] * mu[2] + p[PH_G + 3] * mu[3]) + (X + cs * off) * p1 + (Y + sn * off) * p2 - beta;
            const double sk = dist ? 0.0 : (slv ? slv[it] : z[l.sl + it]);
            a[PV_BAD] = vmax(a[PV_BAD], vbad(sk));
            a[PV_NORM] = vmax(a[PV_NORM], dist ? pp - 1 : fabs(pp - 1));
            a[PV_ROT] = vmax(a[PV_ROT], vmax(r1, r2));
            a[PV_SEP] = vmax(a[PV_SEP], OB_DMIN - (row + sk));
            a[PV_PEN] = vmax(a[PV_PEN], OB_DMIN - row);
            if (j == nOb - 1)                                                                 // c6 is overwritten per obstacle: the LAST one is what the reference tests, without slack (:108-130)
                a[PV_REF] = vmax(a[PV_REF], vmax(vmax(dist ? pp - 1 : fabs(pp) - 1, vmax(r1, r2)), -row + OB_DMIN));
        }
        a[PV_STEER] = a[PV_STEER] - OB_SSB;
        a[PV_REF] = vmax(vmax(vmax(a[PV_REF], refsteer - OB_SSB), vmax(a[PV_U], a[PV_DUAL])), vmax(a[PV_START], a[PV_END]));      // c0[1:2], c0[4:5], c1, c2, c5
#pragma unroll
        for (int i = 0; i < PV_NACC; i++) acc[i][LI(lane)] = a[i];
    }
    double w[PV_NACC];
#pragma unroll
    for (int i = 0; i < PV_NACC; i++) w[i] = wred_max(acc[i]);
    const bool fin = w[PV_BAD] == 0.0;
    bool ok = fin;
#pragma unroll
    for (int i = 0; i < PV_PEN; i++) ok = ok && w[i] <= tol;
    const bool ref_ok = fin && w[PV_REF] <= PV_REF_TOL;
    PAR(lane) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < PV_NCLS; i++) out[i] = w[i];
            out[PV_NCLS] = ok ? 1.0 : 0.0; out[PV_NCLS + 1] = ref_ok ? 1.0 : 0.0;
        }
    }
}

// p: quadcopter problem header (QPH_*); x 12 x (N + 1), u 4 x N, lam 30 x (N + 1) stage-contiguous; ts[k * tstride] is timeScale[k] (tstride 0: one t);
// out: QV_OUT doubles.  Bounds, norm and separation look at stages 1..N only and the gyroscopic terms at stage 1's rates, as constrSatisfaction.jl does.
OBCA_FN void validate_quad_instance(int N, const double *p, const double *x, const double *u, const double *ts, int tstride, const double *lam, double tol, double *out) {
    const double Ts = p[QPH_TS], R = p[QPH_R], ninf = -HUGE_VAL;
    const double xl[QX] = {0, 0, 0, -3, -0.2, -0.2, -1, -1, -1, -1.5, -1, -1.0}, xu[QX] = {10, 10, 5, 3, 0.2, 0.2, 1, 1, 1, 3, 1, 1.0};      // constrSatisfaction.jl:71-98
    const double g0[3] = {x[9], x[10], x[11]};            // x[10], x[11], x[12] with a single index: stage 1 (:151-153)
    double acc[QV_NACC][OBCA_NL];
    PAR(lane) {
        double a[QV_NACC];
#pragma unroll
        for (int i = 0; i < QV_NACC; i++) a[i] = ninf;
        a[QV_START] = a[QV_END] = a[QV_DYN] = a[QV_TSC] = a[QV_BAD] = 0.0;
        for (int k = lane; k <= N; k += QNT) {
            double X[QX];
#pragma unroll
            for (int i = 0; i < QX; i++) { X[i] = x[QX * k + i]; a[QV_BAD] = vmax(a[QV_BAD], vbad(X[i])); }
            const double tk = ts[k * tstride];
            a[QV_BAD] = vmax(a[QV_BAD], vbad(tk));
            for (int i = 0; i < QL * QOB; i++) { const double v = lam[QL * QOB * k + i]; a[QV_DUAL] = vmax(a[QV_DUAL], -v); a[QV_BAD] = vmax(a[QV_BAD], vbad(v)); }
            if (k == 0) {
#pragma unroll
                for (int i = 0; i < QX; i++) a[QV_START] = vmax(a[QV_START], fabs(X[i] - p[QPH_X0 + i]));
            }
            if (k == N) {
#pragma unroll
                for (int i = 0; i < QX; i++) a[QV_END] = vmax(a[QV_END], fabs(X[i] - p[QPH_XF + i]));
                continue;
            }
            double U[QU], usq = 0;
#pragma unroll
            for (int i = 0; i < QU; i++) { U[i] = u[QU * k + i]; a[QV_BAD] = vmax(a[QV_BAD], vbad(U[i])); a[QV_U] = vmax(a[QV_U], vmax(Q_ULO - U[i], U[i] - Q_UHI)); usq += U[i] * U[i]; }
#pragma unroll
            for (int i = 0; i < QX; i++) a[QV_X] = vmax(a[QV_X], vmax(xl[i] - X[i], X[i] - xu[i]));
            a[QV_TSC] = vmax(a[QV_TSC], fabs(ts[(k + 1) * tstride] - tk));
            const double s4 = sin(X[3]), c4 = cos(X[3]), s5 = sin(X[4]), c5 = cos(X[4]), s6 = sin(X[5]), c6 = cos(X[5]);
            const double G[QX] = {X[6], X[7], X[8], c5 * X[9] + s5 * X[11], s5 * s4 / c4 * X[9] + X[10] - c5 * s4 / c4 * X[11], -s5 / c4 * X[9] + c5 / c4 * X[11],
                                  Q_KF / Q_MASS * usq * (s4 * c5 * s6 + s5 * c6), Q_KF / Q_MASS * usq * (-s4 * c5 * c6 + s5 * s6), (Q_KF * usq * c4 * c5 - Q_MASS * Q_GRAV) / Q_MASS,
                                  (Q_ARM * Q_KF * (U[1] * U[1] - U[3] * U[3]) - (Q_I3 - Q_I2) * g0[1] * g0[2]) / Q_I1,
                                  (Q_ARM * Q_KF * (U[2] * U[2] - U[0] * U[0]) - (Q_I1 - Q_I3) * g0[0] * g0[2]) / Q_I2,
                                  (Q_KM * (U[0] * U[0] - U[1] * U[1] + U[2] * U[2] - U[3] * U[3]) - (Q_I2 - Q_I1) * g0[0] * g0[1]) / Q_I3};
#pragma unroll
            for (int i = 0; i < QX; i++) a[QV_DYN] = vmax(a[QV_DYN], fabs(x[QX * (k + 1) + i] - X[i] - tk * Ts * G[i]));
            for (int o = 0; o < QOB; o++) {
                const double *lo = lam + QL * QOB * k + QL * o, *ob = p + QPH_OB + QL * o;
                double nn = 0, sep = 0, bl = 0;
#pragma unroll
                for (int i = 0; i < 3; i++) { const double q = lo[i] - lo[3 + i]; nn += q * q; sep += X[i] * q; bl += ob[i] * lo[i] + ob[3 + i] * lo[3 + i]; }
                a[QV_NORM] = vmax(a[QV_NORM], nn - 1);
                a[QV_SEP] = vmax(a[QV_SEP], -(-bl + sep - R));
            }
        }
#pragma unroll
        for (int i = 0; i < QV_NACC; i++) acc[i][LI(lane)] = a[i];
    }
    double w[QV_NACC];
#pragma unroll
    for (int i = 0; i < QV_NACC; i++) w[i] = wred_max(acc[i]);
    // constrSatisfaction.jl: the bounds fail strictly above 0, the other classes above the tolerance
    const bool ok = w[QV_BAD] == 0.0 && !(w[QV_START] > tol || w[QV_END] > tol || w[QV_U] > 0 || w[QV_X] > 0 || w[QV_DYN] > tol || w[QV_TSC] > tol ||
                                          w[QV_DUAL] > tol || w[QV_NORM] > tol || w[QV_SEP] > tol);
    PAR(lane) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < QV_NCLS; i++) out[i] = w[i];
            out[QV_NCLS] = ok ? 1.0 : 0.0;
        }
    }
}

}  // namespace val
}  // namespace obca
