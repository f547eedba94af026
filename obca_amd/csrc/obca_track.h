// obca_track.h -- a solved trajectory TRACKED on the continuous vehicle model, on the device: the rollout (obca_rollout.h) applies the solved inputs open loop; nobody drives
// that way.  Here a time-varying LQR about the trajectory is computed and the closed loop is rolled: u = u_k + K_k (X_k - x_k), evaluated at the nodes and HELD over the
// interval (a zero-order hold, as the inputs themselves); state differences are taken raw, no angle is wrapped.  One wavefront (64 lanes) per instance;
// obca_amd/validate.py (track_gains_parking / track_gains_quad, track_parking / track_quad, track_record) is the numpy statement, in the order of this text.
//   1. linearisation   Phi_k(X, U): the state after S classical RK4 steps of h_k / S from X with U held -- what roll::integrate applies, the parking prep (tan delta, once
//                      per interval) included.  A_k = dPhi_k/dX, B_k = dPhi_k/dU at (x_k, u_k) by forward-mode tangents through the same steps: items are (interval,
//                      direction), NX + NU directions per interval, dealt over the lanes; a lane carries the state and ONE tangent vector, so no lane holds a matrix.
//                      [A_k | B_k], NX x (NX + NU) row-major, goes to the instance's slice of the work buffer.  (The node linearisation I + h f_x of the NLP's forward Euler
//                      is NOT what the plant applies over an interval; gains from it, held over the quadcopter's 0.5 s, are unstable: see validate.track_gains_quad.)
//   2. gains           P_N = diag(qf); k = N - 1 .. 0: G = diag(r) + B'PB, K_k = -G^-1 B'PA by an unpivoted Cholesky of the NU x NU matrix, P <- diag(q) + A'PA + (B'PA)' K_k,
//                      P <- (P + P') / 2.  Sequential in k; within a step the products P [A|B] and [A|B]' P [A|B] are spread over the lanes through LDS (832 doubles for the
//                      quadcopter); every LDS word read has been written by this launch, every loop bound is known at launch.  A pivot that is not finite and positive
//                      marks the instance bad.  K_k, NU x NX row-major, stage after stage, goes to the batch's gain buffer and stays there.
//   3. closed loop     the rollout's chain with two hooks (roll::NoHook): X_0 = x_0 + dx0; per interval U_k = u_k + K_k (X_k - x_k) if `feedback`, clipped to the NLP's own
//                      input bounds if `clamp`.  One lane integrates; the sample clearances and the head of the record are the rollout's own phases.  The hook leaves U_k in
//                      the instance's slice of the work buffer (the applied inputs, NU x N behind [A|B]) and the chain reads it from there, as it reads a trajectory's own
//                      input: with feedback = clamp = 0 and no dx0 the result then equals the rollout kernel's bit for bit (see Feedback::input).
// Record (TK_OUT doubles): the RO_OUT doubles of the chain rollout field for field ([10] = 0), then feedback, clamp, the number of intervals in which an input was
// clipped, the largest |U_k - u_k| over inputs and intervals, its interval (ties: the smallest), |dx0| of the position part, 2 x 0.
// bad = 1: what the rollout calls bad, a dx0 that is not finite, or a pivot as above; then the record is the rollout's bad record, the count and the interval -1, the two
// real fields NaN, and the instance's gains and node states NaN.  An instance is marked alone.
// The same text compiles for the host (-DOBCA_EMU) for tests/emu/track_emu.cpp.  Nothing here is used by the solve kernels.
#pragma once
#ifndef RO_OUT
#error "include the rollout's kernel text (namespace roll) before this header: its models, chain, clearance phase and record are reused unchanged"
#endif

namespace obca {
namespace trk {
using namespace roll;

#define TK_OUT 48            // doubles per instance (= OBCA_TRK_OUT of include/obca_track.h)
enum { TK_FEEDBACK = RO_OUT, TK_CLAMP, TK_SAT, TK_DU, TK_DUNODE, TK_DX0 };
static_assert(TK_DX0 + 3 == TK_OUT, "the record ends with two reserved zeros");

// diagonal weights of one call (parking reads the first 4 / 2 / 4): a kernel argument
struct Weights { double q[QX], r[QU], qf[QX]; };

// the refusals of the entry points, one text for the library and the host build
static inline const char *track_check_args(int substeps, int feedback, int clamp, const double *q, const double *r, const double *qf, int nx, int nu, double need) {
    if (feedback != 0 && feedback != 1) return "feedback must be 0 (open loop) or 1";
    if (clamp != 0 && clamp != 1) return "clamp must be 0 or 1";
    if (!q || !r || !qf) return "the weights q, r and qf must not be NULL";
    for (int i = 0; i < nx; i++) if (!(q[i] - q[i] == 0.0) || q[i] < 0.0 || !(qf[i] - qf[i] == 0.0) || qf[i] < 0.0) return "q and qf need finite entries >= 0";
    for (int i = 0; i < nu; i++) if (!(r[i] - r[i] == 0.0) || !(r[i] > 0.0)) return "r needs finite entries > 0";
    return roll::rollout_check_args(substeps, 0, need);
}
static inline Weights make_weights(const double *q, const double *r, const double *qf, int nx, int nu) {
    Weights w;
    for (int i = 0; i < QX; i++) { w.q[i] = i < nx ? q[i] : 0.0; w.qf[i] = i < nx ? qf[i] : 0.0; }
    for (int i = 0; i < QU; i++) w.r[i] = i < nu ? r[i] : 1.0;
    return w;
}
// doubles of one instance: [A|B] and, behind it, the applied inputs in the work buffer; the gains
OBCA_HD size_t track_ab_len(int N, int nx, int nu) { return (size_t)N * nx * (nx + nu) + (size_t)N * nu; }
OBCA_HD size_t track_gain_len(int N, int nx, int nu) { return (size_t)N * nu * nx; }

// the NLP's own input bounds
template <class M> struct InputBox;
template <> struct InputBox<ParkModel> {
    RO_MEMBER double lo(int a) { return a == 0 ? OB_UL0 : OB_UL1; }
    RO_MEMBER double hi(int a) { return a == 0 ? OB_UU0 : OB_UU1; }
};
template <> struct InputBox<QuadModel> {
    RO_MEMBER double lo(int) { return Q_ULO; }
    RO_MEMBER double hi(int) { return Q_UHI; }
};

// roll::rk4_step with a tangent: (X, T) <- (Phi, dPhi (T, du)) of one step of length h; u as prep left it, du its tangent
template <class M>
OBCA_FN void rk4_step_tan(double L, double h, const double *u, const double *du, double *X, double *T) {
    double acc[M::NX], xt[M::NX], k[M::NX], dacc[M::NX], dxt[M::NX], dk[M::NX];
    M::rhs(L, X, u, k); M::jvp(L, X, u, T, du, dk);
#pragma unroll
    for (int i = 0; i < M::NX; i++) { acc[i] = k[i]; xt[i] = X[i] + h / 2 * k[i]; dacc[i] = dk[i]; dxt[i] = T[i] + h / 2 * dk[i]; }
    M::rhs(L, xt, u, k); M::jvp(L, xt, u, dxt, du, dk);
#pragma unroll
    for (int i = 0; i < M::NX; i++) { acc[i] = acc[i] + 2 * k[i]; xt[i] = X[i] + h / 2 * k[i]; dacc[i] = dacc[i] + 2 * dk[i]; dxt[i] = T[i] + h / 2 * dk[i]; }
    M::rhs(L, xt, u, k); M::jvp(L, xt, u, dxt, du, dk);
#pragma unroll
    for (int i = 0; i < M::NX; i++) { acc[i] = acc[i] + 2 * k[i]; xt[i] = X[i] + h * k[i]; dacc[i] = dacc[i] + 2 * dk[i]; dxt[i] = T[i] + h * dk[i]; }
    M::rhs(L, xt, u, k); M::jvp(L, xt, u, dxt, du, dk);
#pragma unroll
    for (int i = 0; i < M::NX; i++) { X[i] = X[i] + h / 6 * (acc[i] + k[i]); T[i] = T[i] + h / 6 * (dacc[i] + dk[i]); }
}

// Phase 1.  x, u, hk as roll::integrate takes them; AB: N x NX x (NX + NU) of this instance.  Item it = k (NX + NU) + d: column d of [A_k | B_k].
template <class M, class H>
OBCA_FN void linearise(double L, int N, int S, const double *x, const double *u, H &&hk, int rev, double *AB) {
    constexpr int ND = M::NX + M::NU;
    const int nIt = N * ND, rounds = (nIt + OB_NT - 1) / OB_NT;
    PAR(lane) {
        for (int r = 0; r < rounds; r++) {
            const int it = clr::cl_item(r, rounds, lane, rev);
            if (it >= nIt) continue;
            const int k = it / ND, d = it - k * ND;
            double X[M::NX], T[M::NX], U[M::NU], dU[M::NU];
#pragma unroll
            for (int i = 0; i < M::NX; i++) { X[i] = x[M::NX * k + i]; T[i] = i == d ? 1.0 : 0.0; }
#pragma unroll
            for (int i = 0; i < M::NU; i++) { U[i] = u[M::NU * k + i]; dU[i] = M::NX + i == d ? 1.0 : 0.0; }
            M::prep(U); M::prep_jvp(U, dU);
            const double h = hk(k) / (double)S;
            for (int s = 0; s < S; s++) rk4_step_tan<M>(L, h, U, dU, X, T);
#pragma unroll
            for (int i = 0; i < M::NX; i++) AB[(k * M::NX + i) * ND + d] = T[i];
        }
    }
}

// Phase 2.  Returns (to every lane) whether a pivot was not finite and positive.  Begins with a SYNC: the stores of phase 1 have landed.
template <class M>
OBCA_FN double riccati(int N, const Weights &w, const double *AB, double *K) {
    constexpr int NX = M::NX, NU = M::NU, ND = NX + NU;
    CL_LDS double P[NX * NX], Ab[NX * ND], PA[NX * ND], Mm[ND * ND], Ks[NU * NX];
    double bad[OBCA_NL];
    PAR(lane) {
        for (int e = lane; e < NX * NX; e += OB_NT) P[e] = (e / NX == e % NX) ? w.qf[e / NX] : 0.0;
        bad[LI(lane)] = 0.0;
    }
    for (int k = N - 1; k >= 0; k--) {
        SYNC();
        PAR(lane) { for (int e = lane; e < NX * ND; e += OB_NT) Ab[e] = AB[k * NX * ND + e]; }
        SYNC();
        PAR(lane) {      // P [A|B]
            for (int e = lane; e < NX * ND; e += OB_NT) {
                const int i = e / ND, d = e - i * ND;
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NX; j++) s = s + P[i * NX + j] * Ab[j * ND + d];
                PA[e] = s;
            }
        }
        SYNC();
        PAR(lane) {      // [A|B]' P [A|B]: A'PA in the leading NX x NX block, B'PA below it, B'PB in the corner
            for (int e = lane; e < ND * ND; e += OB_NT) {
                const int a = e / ND, b = e - a * ND;
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NX; j++) s = s + Ab[j * ND + a] * PA[j * ND + b];
                Mm[e] = s;
            }
        }
        SYNC();
        PAR(lane) {      // G = diag(r) + B'PB = C C' in every lane (the same numbers); lane j < NX solves column j of G K = -B'PA
            double Cf[NU][NU], b = 0.0;
#pragma unroll
            for (int a = 0; a < NU; a++) {
#pragma unroll
                for (int c = 0; c <= a; c++) {
                    double s = Mm[(NX + a) * ND + NX + c] + (a == c ? w.r[a] : 0.0);
#pragma unroll
                    for (int t = 0; t < c; t++) s = s - Cf[a][t] * Cf[c][t];
                    if (a == c) { b = val::vmax(b, (s > 0.0 && s - s == 0.0) ? 0.0 : 1.0); Cf[a][a] = sqrt(s); }
                    else Cf[a][c] = s / Cf[c][c];
                }
            }
            bad[LI(lane)] = val::vmax(bad[LI(lane)], b);
            if (lane < NX) {
                double y[NU];
#pragma unroll
                for (int a = 0; a < NU; a++) {
                    double s = Mm[(NX + a) * ND + lane];
#pragma unroll
                    for (int t = 0; t < a; t++) s = s - Cf[a][t] * y[t];
                    y[a] = s / Cf[a][a];
                }
#pragma unroll
                for (int a = NU - 1; a >= 0; a--) {
                    double s = y[a];
#pragma unroll
                    for (int t = a + 1; t < NU; t++) s = s - Cf[t][a] * y[t];
                    y[a] = s / Cf[a][a];
                }
#pragma unroll
                for (int a = 0; a < NU; a++) { Ks[a * NX + lane] = -y[a]; K[(k * NU + a) * NX + lane] = -y[a]; }
            }
        }
        SYNC();
        PAR(lane) {      // P <- diag(q) + A'PA + (B'PA)' K, symmetrised: entry (i, j) and its mirror are formed by the same lane
            for (int e = lane; e < NX * NX; e += OB_NT) {
                const int i = e / NX, j = e - i * NX;
                double sij = 0.0, sji = 0.0;
#pragma unroll
                for (int a = 0; a < NU; a++) { sij = sij + Mm[(NX + a) * ND + i] * Ks[a * NX + j]; sji = sji + Mm[(NX + a) * ND + j] * Ks[a * NX + i]; }
                const double qd = i == j ? w.q[i] : 0.0;
                P[e] = 0.5 * (((qd + Mm[i * ND + j]) + sij) + ((qd + Mm[j * ND + i]) + sji));
            }
        }
    }
    SYNC();
    return wred_max(bad);
}

// Phase 3: the two hooks of the chain (roll::NoHook).  Lives in the integrating lane: what it counts is read back by that lane.
template <class M>
struct Feedback {
    const double *x, *K, *dx0;
    double *Ua;
    int feedback, clamp;
    double sat, du, node;
    RO_METHOD void start(double *X) {
        if (dx0) {
#pragma unroll
            for (int i = 0; i < M::NX; i++) X[i] = X[i] + dx0[i];
        }
    }
    // U_k into the instance's slice Ua (NU x N, the applied inputs) of the work buffer; the chain reads it back FROM MEMORY, as it reads a trajectory's own input: the
    // compiler then forms the model's terms in u as it does in the rollout kernel (which terms of u0^2 - u1^2 + u2^2 - u3^2 it fuses depends on where the operands
    // come from), and without feedback, clamp and dx0 the two kernels agree bit for bit
    RO_METHOD const double *input(int k, const double *X, const double *uk) {
        double U[M::NU];
#pragma unroll
        for (int a = 0; a < M::NU; a++) U[a] = uk[a];
        if (feedback) {
            double e[M::NX];
#pragma unroll
            for (int j = 0; j < M::NX; j++) e[j] = X[j] - x[M::NX * k + j];
#pragma unroll
            for (int a = 0; a < M::NU; a++) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < M::NX; j++) s = s + K[(k * M::NU + a) * M::NX + j] * e[j];
                U[a] = U[a] + s;
            }
        }
        double cl = 0.0, d = 0.0;
#pragma unroll
        for (int a = 0; a < M::NU; a++) {
            if (clamp) {
                const double lo = InputBox<M>::lo(a), hi = InputBox<M>::hi(a);
                const double c = U[a] < lo ? lo : (U[a] > hi ? hi : U[a]);
                cl = c != U[a] ? 1.0 : cl;
                U[a] = c;
            }
            d = val::vmax(d, fabs(U[a] - uk[a]));
            Ua[M::NU * k + a] = U[a];
        }
        sat = sat + cl;
        if (d > du) { du = d; node = (double)k; }      // ascending k: a tie keeps the smaller
        int at = M::NU * k;
        OPAQUE(at);      // (the same slot: the load may not be replaced by the values stored above)
        return Ua + at;
    }
};

OBCA_FN void write_tail_bad(int feedback, int clamp, double *out) {
    PAR(lane) {
        if (lane == 0) {
            const double nan_ = __builtin_nan("");
            out[TK_FEEDBACK] = (double)feedback; out[TK_CLAMP] = (double)clamp; out[TK_SAT] = -1.0; out[TK_DU] = nan_; out[TK_DUNODE] = -1.0; out[TK_DX0] = nan_;
            out[TK_DX0 + 1] = out[TK_DX0 + 2] = 0.0;
        }
    }
}
OBCA_FN void write_gains_bad(int n, double *K) {
    PAR(lane) {
        for (int i = lane; i < n; i += OB_NT) K[i] = __builtin_nan("");
    }
}
// after the chain: the tail of the record from what the hooks counted; a chain that came back bad takes the gains with it
template <class M>
OBCA_FN void write_tail(int N, const Feedback<M> &fb, double *K, double *out) {
    SYNC();
    if (out[RO_BAD] != 0.0) { write_gains_bad(N * M::NU * M::NX, K); write_tail_bad(fb.feedback, fb.clamp, out); return; }
    PAR(lane) {
        if (lane == 0) {
            double d[RD_N] = {0.0, 0.0, 0.0, 0.0}, zero[M::NX];
#pragma unroll
            for (int i = 0; i < M::NX; i++) zero[i] = 0.0;
            if (fb.dx0) M::dev(fb.dx0, zero, d);
            out[TK_FEEDBACK] = (double)fb.feedback; out[TK_CLAMP] = (double)fb.clamp; out[TK_SAT] = fb.sat; out[TK_DU] = fb.du; out[TK_DUNODE] = fb.node; out[TK_DX0] = d[RD_POS];
            out[TK_DX0 + 1] = out[TK_DX0 + 2] = 0.0;
        }
    }
}
// whether dx0 (nx doubles or nullptr) holds a number that is not finite, to every lane
OBCA_FN double dx0_bad(const double *dx0, int nx) {
    double b[OBCA_NL];
    PAR(lane) {
        double v = 0.0;
        if (dx0) for (int i = lane; i < nx; i += OB_NT) v = val::vmax(v, val::vbad(dx0[i]));
        b[LI(lane)] = v;
    }
    return wred_max(b);
}

// p, z, ts, S, need, rev, pose, Xn: as roll::rollout_parking_instance takes them; dx0: 4 doubles or nullptr; AB: N x 4 x 6, Ua: 2 x N, K: N x 2 x 4 of this instance; out: TK_OUT doubles.
template <int VM>
OBCA_FN void track_parking_instance(int N, const double *p, const double *z, const double *ts, int S, int feedback, int clamp, const Weights &w, const double *dx0, double need, int rev,
                                    double *AB, double *Ua, double *pose, double *Xn, double *K, double *out) {
    Lay l; make_layout(N, (int)p[PH_NOB], (int)p[PH_M], l);
    const double Ts = p[PH_TS];
    const double t1 = p[PH_FIX] != 0.0 ? 1.0 : z[l.t];
    linearise<ParkModel>(p[PH_L], N, S, z + l.x, z + l.u, [&](int k) { return (ts ? ts[k] : t1) * Ts; }, rev, AB);
    const double bad = val::vmax(riccati<ParkModel>(N, w, AB, K), dx0_bad(dx0, 4));
    if (bad != 0.0) { roll::write_all_bad(N, 4, S, 0, Xn, out); write_gains_bad(N * 2 * 4, K); write_tail_bad(feedback, clamp, out); return; }
    Feedback<ParkModel> fb = {z + l.x, K, dx0, Ua, feedback, clamp, 0.0, -1.0, 0.0};
    roll::rollout_parking_instance<VM>(N, p, z, ts, S, 0, need, rev, pose, Xn, out, fb);
    write_tail<ParkModel>(N, fb, K, out);
}

// p, x, u, ts, tstride, S, need, rev, pose, Xn: as roll::rollout_quad_instance takes them; dx0: 12 doubles or nullptr; AB: N x 12 x 16, Ua: 4 x N, K: N x 4 x 12 of this instance.
OBCA_FN void track_quad_instance(int N, const double *p, const double *x, const double *u, const double *ts, int tstride, int S, int feedback, int clamp, const Weights &w, const double *dx0,
                                 double need, int rev, double *AB, double *Ua, double *pose, double *Xn, double *K, double *out) {
    const double Ts = p[QPH_TS];
    linearise<QuadModel>(0.0, N, S, x, u, [&](int k) { return ts[k * tstride] * Ts; }, rev, AB);
    const double bad = val::vmax(riccati<QuadModel>(N, w, AB, K), dx0_bad(dx0, QX));
    if (bad != 0.0) { roll::write_all_bad(N, QX, S, 0, Xn, out); write_gains_bad(N * QU * QX, K); write_tail_bad(feedback, clamp, out); return; }
    Feedback<QuadModel> fb = {x, K, dx0, Ua, feedback, clamp, 0.0, -1.0, 0.0};
    roll::rollout_quad_instance(N, p, x, u, ts, tstride, S, 0, need, rev, pose, Xn, out, fb);
    write_tail<QuadModel>(N, fb, K, out);
}

}  // namespace trk
}  // namespace obca
