// obca_rollout.h -- a solved trajectory applied to the CONTINUOUS vehicle model, on the device: validate() and clearance() measure a solution against the NLP's own
// discretisation; here the inputs u_k are held over interval k (length h_k = t_k Ts) and the model the rows discretise is integrated with classical RK4, S equal steps per
// interval.  One wavefront (64 lanes) per instance; obca_amd/validate.py (rollout_parking, rollout_quad, rollout_record) is the numpy statement.
//   models   : parking   x' = v cos psi, y' = v sin psi, psi' = v tan(delta) / L, v' = a (the kinematic bicycle ParkingSignedDist.jl:147-150 steps with the midpoint rule)
//              quadcopter  quad::dyn_g_continuous (obca_quad_model.h): the rigid body QuadcopterSignedDist.jl:138-155 steps with forward Euler, gyroscopic products at the CURRENT rates
//   modes    : chain (restart 0)  X_0 = x[:, 0], X_{k+1} = the state S steps after X_k: the open loop
//              restart (1)        X_{k+1} = the state S steps after the solution's node x[:, k]: the defect of ONE interval, nothing compounds
//   samples  : clearance()'s, q = k S + s and q = N S: (k, s >= 1) is the state after s steps of interval k, (k, 0) is X_k (chain) or the node x[:, k] (restart), the last
//              sample likewise; the clearance of a sample is computed as the clearance check (namespace clr) computes it: dualws_one of the pose with the CL_TOUCH clamp / distance of the point to each box - R
// Phases: 1. finite scan over the lanes  2. integration -- restart: lanes take intervals; chain: ONE lane runs the N S steps (a recurrence in time; the other 63 idle) --
// which leaves the sample poses (3 doubles: x, y, psi / the position) and the node states X in the instance's slices of a device buffer  3. (sample, obstacle) items over
// the lanes, clr::acc_take / clr::write_record and the `hit` marks of the clearance check  4. the deviation maxima X_k - x_k over the nodes k = 1 .. N, NaN-propagating wave
// reductions, ties of the position's node to the smallest.
// Record (RO_OUT doubles): bad, dev_pos, its node, dev_att, dev_vel, dev_rate, the same four at node N, restart, S, 4 x 0, then the CL_OUT clearance record of the samples.
// bad = 1: a non-finite number among what is read (Ts, x, u, the time scale) or a non-finite rolled state -- a number that is not finite, or a quadcopter step across
// cos x[3] = 0 (a pitch through pi/2: the continuous state diverges there, RK4 merely steps over it); then every real-valued field is NaN, the node -1 and the
// clearance part as clr::write_bad leaves it; the node states of such an instance are NaN.
// Transcendentals are libm's / the device library's sin, cos, tan, a plain division where the model divides, as in obca_validate.h: a rolled state is arbitrary.
// The same text compiles for the host (-DOBCA_EMU) for tests/emu/rollout_emu.cpp.  Nothing here is used by the solve kernels.
#pragma once
#include "obca_validate.h"
#ifndef CL_OUT
#error "include the clearance check's kernel text (namespace clr) before this header: its accumulators, record and marks are reused unchanged"
#endif

namespace obca {
namespace roll {
using namespace clr;

#define RO_OUT 40            // doubles per instance (= OBCA_ROLL_OUT of include/obca_rollout.h)
#define RO_CLR 16            // where the clearance record starts
enum { RO_BAD = 0, RO_DPOS, RO_DNODE, RO_DATT, RO_DVEL, RO_DRATE, RO_EPOS, RO_EATT, RO_EVEL, RO_ERATE, RO_RESTART, RO_SUB };
enum { RD_POS = 0, RD_ATT, RD_VEL, RD_RATE, RD_N };
static_assert(RO_CLR + CL_OUT == RO_OUT, "the record ends with the clearance record");

// the refusals of the entry points, one text for the library and the host build
static inline const char *rollout_check_args(int substeps, int restart, double need) {
    if (restart != 0 && restart != 1) return "restart must be 0 (chain) or 1 (restart at every node)";
    return clr::clearance_check_args(substeps, need);
}
// doubles of one instance in the two regions of the work buffer: the sample poses, the node states
OBCA_HD size_t rollout_pose_len(int N, int S) { return 3 * ((size_t)N * S + 1); }
OBCA_HD size_t rollout_state_len(int N, int nx) { return (size_t)nx * (N + 1); }

// the two models: static members (L: the wheel base, the quadcopter ignores it)
#ifdef OBCA_EMU
#define RO_MEMBER OBCA_FN            // (static inline already)
#else
#define RO_MEMBER static OBCA_FN
#endif
struct ParkModel {
    enum { NX = 4, NU = 2 };
    RO_MEMBER void rhs(double L, const double *x, const double *u, double *d) {
        d[0] = x[3] * cos(x[2]); d[1] = x[3] * sin(x[2]); d[2] = x[3] * u[0] / L; d[3] = u[1];      // u[0]: tan(delta), taken once per interval (prep)
    }
    RO_MEMBER void prep(double *u) { u[0] = tan(u[0]); }
    // the tangent of rhs along (dx, du) and of prep (u: prep's result, tan' = 1 + tan^2), for the linearisation of the interval map (obca_track.h)
    RO_MEMBER void jvp(double L, const double *x, const double *u, const double *dx, const double *du, double *d) {
        const double sn = sin(x[2]), cs = cos(x[2]);
        d[0] = dx[3] * cs - x[3] * sn * dx[2]; d[1] = dx[3] * sn + x[3] * cs * dx[2]; d[2] = (dx[3] * u[0] + x[3] * du[0]) / L; d[3] = du[1];
    }
    RO_MEMBER void prep_jvp(const double *u, double *du) { du[0] = (1.0 + u[0] * u[0]) * du[0]; }
    RO_MEMBER double pole(const double *x) { return 1.0; }      // the bicycle has no singular state
    // position, attitude, velocity, body-rate deviation of a rolled state X from the solution's node x
    RO_MEMBER void dev(const double *X, const double *x, double d[RD_N]) {
        const double dx = X[0] - x[0], dy = X[1] - x[1];
        d[RD_POS] = sqrt(dx * dx + dy * dy); d[RD_ATT] = fabs(X[2] - x[2]); d[RD_VEL] = fabs(X[3] - x[3]); d[RD_RATE] = 0.0;
    }
};
struct QuadModel {
    enum { NX = QX, NU = QU };
    RO_MEMBER void rhs(double, const double *x, const double *u, double *d) { quad::dyn_g_continuous(x, u, d); }
    RO_MEMBER void prep(double *u) {}
    RO_MEMBER void jvp(double, const double *x, const double *u, const double *dx, const double *du, double *d) { quad::dyn_g_continuous_jvp(x, u, dx, du, d); }
    RO_MEMBER void prep_jvp(const double *u, double *du) {}
    // the attitude kinematics divide by cos x[3]: where it changes sign within a step the continuous state has diverged (the integral of tan), though RK4 steps across with finite numbers
    RO_MEMBER double pole(const double *x) { return cos(x[3]); }
    RO_MEMBER void dev(const double *X, const double *x, double d[RD_N]) {
        double e[QX];
#pragma unroll
        for (int i = 0; i < QX; i++) e[i] = X[i] - x[i];
        d[RD_POS] = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        d[RD_ATT] = val::vmax(val::vmax(fabs(e[3]), fabs(e[4])), fabs(e[5]));
        d[RD_VEL] = sqrt(e[6] * e[6] + e[7] * e[7] + e[8] * e[8]);
        d[RD_RATE] = val::vmax(val::vmax(fabs(e[9]), fabs(e[10])), fabs(e[11]));
    }
};

// What a caller may put into the chain (obca_track.h: the feedback): start(X) once, on the first state; input(k, X, uk) at the first state X of interval k returns where
// the interval's input is read from (uk: the trajectory's own).  The rollout itself does neither: with NoHook every instantiation below compiles to what it was without the parameter.
#ifdef OBCA_EMU
#define RO_METHOD inline
#else
#define RO_METHOD __device__ __forceinline__
#endif
struct NoHook {
    RO_METHOD void start(double *) {}
    RO_METHOD const double *input(int, const double *, const double *uk) { return uk; }
};

// one classical RK4 step of length h, u held: X <- X + h / 6 (k1 + 2 k2 + 2 k3 + k4)
template <class M>
OBCA_FN void rk4_step(double L, double h, const double *u, double *X) {
    double acc[M::NX], xt[M::NX], k[M::NX];
    M::rhs(L, X, u, k);
#pragma unroll
    for (int i = 0; i < M::NX; i++) { acc[i] = k[i]; xt[i] = X[i] + h / 2 * k[i]; }
    M::rhs(L, xt, u, k);
#pragma unroll
    for (int i = 0; i < M::NX; i++) { acc[i] = acc[i] + 2 * k[i]; xt[i] = X[i] + h / 2 * k[i]; }
    M::rhs(L, xt, u, k);
#pragma unroll
    for (int i = 0; i < M::NX; i++) { acc[i] = acc[i] + 2 * k[i]; xt[i] = X[i] + h * k[i]; }
    M::rhs(L, xt, u, k);
#pragma unroll
    for (int i = 0; i < M::NX; i++) X[i] = X[i] + h / 6 * (acc[i] + k[i]);
}

// Phase 2.  x: NX x (N + 1), u: NU x N stage-contiguous; hk(k): the length of interval k.  pose: 3 x (N S + 1), Xn: NX x (N + 1) of this instance.  Returns in
// bad[LI(lane)] whether the lane met a non-finite state.  All loop bounds are known at launch.
template <class M, class H, class F = NoHook>
OBCA_FN void integrate(double L, int N, int S, int restart, const double *x, const double *u, H &&hk, double *pose, double *Xn, double (&bad)[OBCA_NL], F &&fb = F()) {
    PAR(lane) {
        double b = 0.0;
        const int k0 = restart ? lane : (lane == 0 ? 0 : N), dk = restart ? OB_NT : 1;
        double X[M::NX];
#pragma unroll
        for (int i = 0; i < M::NX; i++) X[i] = x[i];
        fb.start(X);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < M::NX; i++) Xn[i] = X[i];
        }
        for (int k = k0; k < N; k += dk) {
            if (restart) {
#pragma unroll
                for (int i = 0; i < M::NX; i++) X[i] = x[M::NX * k + i];
            }
            double U[M::NU];
            const double *uk = fb.input(k, X, u + M::NU * k);
#pragma unroll
            for (int i = 0; i < M::NU; i++) U[i] = uk[i];
            M::prep(U);
            const double h = hk(k) / (double)S;
            for (int s = 0; s < S; s++) {
#pragma unroll
                for (int i = 0; i < 3; i++) pose[3 * (k * S + s) + i] = X[i];
                const double c0 = M::pole(X);
                rk4_step<M>(L, h, U, X);
                b = val::vmax(b, c0 * M::pole(X) <= 0.0 ? 1.0 : 0.0);      // through the pole: not a state of the continuous model any more
#pragma unroll
                for (int i = 0; i < M::NX; i++) b = val::vmax(b, val::vbad(X[i]));
            }
#pragma unroll
            for (int i = 0; i < M::NX; i++) Xn[M::NX * (k + 1) + i] = X[i];
        }
        if (lane == 0) {      // the last sample: X_N (chain) or the solution's node N (restart)
#pragma unroll
            for (int i = 0; i < 3; i++) pose[3 * N * S + i] = restart ? x[M::NX * N + i] : X[i];
        }
        bad[LI(lane)] = b;
    }
}

OBCA_FN void write_head_bad(int S, int restart, double *out) {
    PAR(lane) {
        if (lane == 0) {
            const double nan_ = __builtin_nan("");
            out[RO_BAD] = 1.0;
            for (int i = RO_DPOS; i <= RO_ERATE; i++) out[i] = nan_;
            out[RO_DNODE] = -1.0; out[RO_RESTART] = (double)restart; out[RO_SUB] = (double)S;
            for (int i = RO_SUB + 1; i < RO_CLR; i++) out[i] = 0.0;
        }
    }
}
// the whole record and the node states of an instance that is not finite
OBCA_FN void write_all_bad(int N, int nx, int S, int restart, double *Xn, double *out) {
    PAR(lane) {
        for (int i = lane; i < nx * (N + 1); i += OB_NT) Xn[i] = __builtin_nan("");
    }
    write_head_bad(S, restart, out);
    clr::write_bad(N * S + 1, out + RO_CLR);
}

// Phase 4: the largest deviations over the nodes 1 .. N and those at node N
template <class M>
OBCA_FN void write_head(int N, int S, int restart, const double *x, const double *Xn, double *out) {
    double mx[RD_N][OBCA_NL], at[OBCA_NL], kk[OBCA_NL];
    PAR(lane) {
        double a[RD_N] = {0.0, 0.0, 0.0, 0.0}, node = HUGE_VAL;      // (deviations are >= 0; the first node a lane sees sets `node`)
        for (int k = 1 + lane; k <= N; k += OB_NT) {
            double d[RD_N];
            M::dev(Xn + M::NX * k, x + M::NX * k, d);
            if (d[RD_POS] > a[RD_POS] || node == HUGE_VAL) { a[RD_POS] = d[RD_POS]; node = (double)k; }      // ascending k: a tie keeps the smaller
#pragma unroll
            for (int i = 1; i < RD_N; i++) a[i] = val::vmax(a[i], d[i]);
        }
#pragma unroll
        for (int i = 0; i < RD_N; i++) mx[i][LI(lane)] = a[i];
        at[LI(lane)] = node;
    }
    double w[RD_N];
#pragma unroll
    for (int i = 0; i < RD_N; i++) w[i] = wred_max(mx[i]);
    PAR(lane) { kk[LI(lane)] = (mx[RD_POS][LI(lane)] == w[RD_POS]) ? at[LI(lane)] : HUGE_VAL; }
    const double node = wred_min(kk);
    PAR(lane) {
        if (lane == 0) {
            double e[RD_N];
            M::dev(Xn + M::NX * N, x + M::NX * N, e);
            out[RO_BAD] = 0.0; out[RO_DPOS] = w[RD_POS]; out[RO_DNODE] = node; out[RO_DATT] = w[RD_ATT]; out[RO_DVEL] = w[RD_VEL]; out[RO_DRATE] = w[RD_RATE];
            out[RO_EPOS] = e[RD_POS]; out[RO_EATT] = e[RD_ATT]; out[RO_EVEL] = e[RD_VEL]; out[RO_ERATE] = e[RD_RATE];
            out[RO_RESTART] = (double)restart; out[RO_SUB] = (double)S;
            for (int i = RO_SUB + 1; i < RO_CLR; i++) out[i] = 0.0;
        }
    }
}

// p: problem header (PH_*: unit-length rows), z: a point in the solver's layout (x, u and t are read); ts: the caller's timeScale per stage (N + 1; nullptr: the point's
// single t, 1 with fixTime); S: sub-steps, 1 .. CL_SMAX; pose / Xn: this instance's slices of the work buffer; out: RO_OUT doubles.  VM: the row class of the batch's
// widest obstacle.  Needs 1 <= N <= OB_NMAX.
template <int VM, class F = NoHook>
OBCA_FN void rollout_parking_instance(int N, const double *p, const double *z, const double *ts, int S, int restart, double need, int rev, double *pose, double *Xn, double *out, F &&fb = F()) {
    CL_LDS unsigned char hit[CL_MAXSAMPLES];
    const int nOb = (int)p[PH_NOB], M = (int)p[PH_M];
    Lay l; make_layout(N, nOb, M, l);
    const double Ts = p[PH_TS], off = p[PH_OFF];
    const double t1 = p[PH_FIX] != 0.0 ? 1.0 : z[l.t];
    const int nS = N * S + 1, nIt = nS * nOb, rounds = (nIt + OB_NT - 1) / OB_NT;
    double acc[CA_N][OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vmax(val::vbad(Ts), ts ? 0.0 : val::vbad(t1)) : 0.0;
        for (int i = lane; i < 4 * (N + 1); i += OB_NT) b = val::vmax(b, val::vbad(z[l.x + i]));
        for (int i = lane; i < 2 * N; i += OB_NT) b = val::vmax(b, val::vbad(z[l.u + i]));
        if (ts) for (int i = lane; i < N + 1; i += OB_NT) b = val::vmax(b, val::vbad(ts[i]));
        acc[CA_BAD][LI(lane)] = b;
        for (int q = lane; q < nS; q += OB_NT) hit[q] = 0;
    }
    if (wred_max(acc[CA_BAD]) != 0.0) { write_all_bad(N, 4, S, restart, Xn, out); return; }
    integrate<ParkModel>(p[PH_L], N, S, restart, z + l.x, z + l.u, [&](int k) { return (ts ? ts[k] : t1) * Ts; }, pose, Xn, acc[CA_BAD], fb);
    if (wred_max(acc[CA_BAD]) != 0.0) { write_all_bad(N, 4, S, restart, Xn, out); return; }
    SYNC();
    PAR(lane) {
        double a[CA_N], g[4];
        clr::acc_init(a);
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = p[PH_G + i];
        for (int r = 0; r < rounds; r++) {
            const int it = clr::cl_item(r, rounds, lane, rev);
            if (it >= nIt) continue;
            const int q = it / nOb, j = it - q * nOb, k = q / S, s = q - k * S;
            const int v = (int)p[PH_VOB + j], r0 = (int)p[PH_ROFF + j];
            double a1[VM], a2[VM], bj[VM];
#pragma unroll
            for (int i = 0; i < VM; i++) { const bool on = i < v; a1[i] = on ? p[PH_A + 2 * (r0 + i)] : 0.0; a2[i] = on ? p[PH_A + 2 * (r0 + i) + 1] : 0.0; bj[i] = on ? p[PH_B + r0 + i] : 0.0; }
            const double X = pose[3 * q], Y = pose[3 * q + 1], psi = pose[3 * q + 2];
            const double sn = sin(psi), cs = cos(psi);
            double lam[VM], mu[4], d;
            dualws_one<VM>(v, a1, a2, bj, g, X + cs * off, Y + sn * off, cs, sn, lam, mu, &d);
            const double c = d < CL_TOUCH ? 0.0 : d;
            clr::acc_take(a, c, q, j, s == 0);
            if (c < need) hit[q] = 1;
        }
#pragma unroll
        for (int i = 0; i < CA_N; i++) acc[i][LI(lane)] = (i == CA_KEY || i == CA_BAD) ? a[i] : -a[i];
    }
    SYNC();
    if (wred_max(acc[CA_BAD]) != 0.0) { write_all_bad(N, 4, S, restart, Xn, out); return; }
    clr::write_record(nS, nOb, acc, hit, out + RO_CLR);
    write_head<ParkModel>(N, S, restart, z + l.x, Xn, out);
}

// p: quadcopter problem header (QPH_*: Ts, R, the boxes as [hi; -lo]); x: 12 x (N + 1), u: 4 x N stage-contiguous; ts[k * tstride] is timeScale[k] (tstride 0: one t).
// Needs 1 <= N <= QNMAX.  fb: see NoHook.
template <class F = NoHook>
OBCA_FN void rollout_quad_instance(int N, const double *p, const double *x, const double *u, const double *ts, int tstride, int S, int restart, double need, int rev,
                                   double *pose, double *Xn, double *out, F &&fb = F()) {
    CL_LDS unsigned char hit[CL_MAXSAMPLES];
    const double Ts = p[QPH_TS], R = p[QPH_R];
    const int nS = N * S + 1, nIt = nS * QOB, rounds = (nIt + QNT - 1) / QNT;
    double acc[CA_N][OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vbad(Ts) : 0.0;
        for (int i = lane; i < QX * (N + 1); i += QNT) b = val::vmax(b, val::vbad(x[i]));
        for (int i = lane; i < QU * N; i += QNT) b = val::vmax(b, val::vbad(u[i]));
        for (int i = lane; i < N + 1; i += QNT) b = val::vmax(b, val::vbad(ts[i * tstride]));
        acc[CA_BAD][LI(lane)] = b;
        for (int q = lane; q < nS; q += QNT) hit[q] = 0;
    }
    if (wred_max(acc[CA_BAD]) != 0.0) { write_all_bad(N, QX, S, restart, Xn, out); return; }
    integrate<QuadModel>(0.0, N, S, restart, x, u, [&](int k) { return ts[k * tstride] * Ts; }, pose, Xn, acc[CA_BAD], fb);
    if (wred_max(acc[CA_BAD]) != 0.0) { write_all_bad(N, QX, S, restart, Xn, out); return; }
    SYNC();
    PAR(lane) {
        double a[CA_N];
        clr::acc_init(a);
        for (int r = 0; r < rounds; r++) {
            const int it = clr::cl_item(r, rounds, lane, rev);
            if (it >= nIt) continue;
            const int q = it / QOB, j = it - q * QOB, k = q / S, s = q - k * S;
            const double *ob = p + QPH_OB + QL * j;
            double d2 = 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double pi = pose[3 * q + i];
                const double lo = -ob[3 + i] - pi, hi = pi - ob[i];
                const double e = lo > 0.0 ? lo : (hi > 0.0 ? hi : 0.0);
                d2 = d2 + clr::cl_keep(e * e);
            }
            const double c = sqrt(d2) - R;
            clr::acc_take(a, c, q, j, s == 0);
            if (c < need) hit[q] = 1;
        }
#pragma unroll
        for (int i = 0; i < CA_N; i++) acc[i][LI(lane)] = (i == CA_KEY || i == CA_BAD) ? a[i] : -a[i];
    }
    SYNC();
    if (wred_max(acc[CA_BAD]) != 0.0) { write_all_bad(N, QX, S, restart, Xn, out); return; }
    clr::write_record(nS, QOB, acc, hit, out + RO_CLR);
    write_head<QuadModel>(N, S, restart, x, Xn, out);
}

}  // namespace roll
}  // namespace obca
