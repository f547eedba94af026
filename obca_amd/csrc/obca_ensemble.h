// obca_ensemble.h -- an ENSEMBLE of closed-loop rollouts about one trajectory, on the device: the track call (obca_track.h) rolls the closed loop from one start offset with
// ONE lane of the wavefront, because the chain is a recurrence in time.  A user who has gains wants the spread of the closed loop over the disturbances they expect: here
// up to 64 members per instance are rolled at once, one member per lane.  One wavefront (64 lanes) per instance, one launch;
// obca_amd/validate.py (ensemble_parking / ensemble_quad, ensemble_record) is the numpy statement.
//   1. finite scan     of what the track call reads (Ts, x, u, the time scale), over the lanes: the rollout's scan
//   2. gains           trk::linearise and trk::riccati, unchanged: K_k depend on the nominal trajectory only, they are computed once and shared by all members
//   3. members         lane m < M: X_0 = x_0 + dx0[m]; per interval the commanded input u_k + K_k (X_k - x_k) if `feedback`, else u_k; the applied input
//                      U_k = commanded + dub[m] (a constant actuator bias), clipped to trk::InputBox if `clamp`; X_{k+1} = S roll::rk4_step of h_k / S with U_k held.
//                      Every sample the member passes (q = k S + s, and q = N S) is measured INLINE by the integrating lane the way the rollout measures it -- parking:
//                      dualws_one<VM> of the pose with the CL_TOUCH clamp; quadcopter: distance of the point to each box - R -- so no buffer of M x (N S + 1) poses exists.
//                      The lane keeps the running minimum (strict <, ascending (q, obstacle): a tie keeps the smaller index), the number of samples under `need`, the
//                      deviations M::dev from the nominal nodes 1 .. N, the clipped intervals and the largest |U_k - u_k|.  A member whose state goes non-finite
//                      integrates on to the end and is marked afterwards.  Lanes m >= M do nothing.
//   4. instance record lane 0 walks the M member records in ascending order (ensemble_reduce): ties go to the smaller member, means are sums in that order -- the host
//                      build and the device add in the same order.  Bad members enter nothing.
// Every loop bound is known at launch; no atomics, no early exit.
// Member record (EN_MEM doubles): bad, dev_pos, its node, end_pos, dev_att, dev_vel, dev_rate, min clearance, its sample, its obstacle, below, saturated intervals, du_max,
// its interval, |dx0[m]| of the position part, 0.  bad = 1: a dx0[m] or dub[m] that is not finite, a rolled state or a clearance that is not finite, a quadcopter step
// across cos x[3] = 0; that member alone is marked: its real fields NaN, its index and count fields -1, its final state NaN.
// Instance record (EN_OUT doubles): bad, M, S, feedback, clamp, members_bad, members_hit (good members with a sample under `need`), members_sat (good members with a
// clipped interval), min over the good members, its member, sample, obstacle, dev_pos max, its member, its node, end_pos max, its member, dev_att, dev_vel, dev_rate,
// du_max, its member, its interval, mean of end_pos, mean of min, below summed, 6 x 0.  bad = 1: what the track call marks for the whole instance (the scan, a Riccati pivot
// that is not finite and positive): every member bad, real fields NaN, indices and counts -1.  Every member bad, the instance not: members_bad = M, the other counts 0,
// real fields NaN, indices -1.
// The same text compiles for the host (-DOBCA_EMU) for tests/emu/ensemble_emu.cpp.  Nothing here is used by the solve, rollout or track kernels.
#pragma once
#ifndef TK_OUT
#error "include the track call's kernel text (namespace trk) before this header: its linearisation, Riccati recursion, weights and input box are reused unchanged"
#endif

namespace obca {
namespace ens {
using namespace trk;

#define EN_MEM 16            // doubles per member (= OBCA_ENS_MEM of include/obca_ensemble.h)
#define EN_OUT 32            // doubles per instance (= OBCA_ENS_OUT)
#define EN_MMAX 64           // most members: one per lane
enum { EM_BAD = 0, EM_DPOS, EM_DNODE, EM_EPOS, EM_DATT, EM_DVEL, EM_DRATE, EM_MIN, EM_SAMPLE, EM_OBST, EM_BELOW, EM_SAT, EM_DU, EM_DUNODE, EM_DX0, EM_RSV };
enum { EO_BAD = 0, EO_M, EO_SUB, EO_FEEDBACK, EO_CLAMP, EO_NBAD, EO_NHIT, EO_NSAT, EO_MIN, EO_MINMEM, EO_SAMPLE, EO_OBST, EO_DPOS, EO_DPOSMEM, EO_DNODE, EO_EPOS, EO_EPOSMEM,
       EO_DATT, EO_DVEL, EO_DRATE, EO_DU, EO_DUMEM, EO_DUNODE, EO_MEANEPOS, EO_MEANMIN, EO_BELOW, EO_RSV };
static_assert(EM_RSV + 1 == EN_MEM && EO_RSV + 6 == EN_OUT && EN_MMAX == OB_NT && EN_MMAX == QNT, "the records end with their reserved zeros; one member per lane");

// the refusals of the entry points, one text for the library and the host build
static inline const char *ensemble_check_args(int substeps, int members, int feedback, int clamp, const double *q, const double *r, const double *qf, int nx, int nu, double need) {
    if (members < 1 || members > EN_MMAX) return "need 1 <= members <= 64";
    return trk::track_check_args(substeps, feedback, clamp, q, r, qf, nx, nu, need);
}
// doubles of one instance: [A|B] in the work buffer (the gains: trk::track_gain_len), the member records, the final states
OBCA_HD size_t ensemble_ab_len(int N, int nx, int nu) { return (size_t)N * nx * (nx + nu); }
OBCA_HD size_t ensemble_mem_len(int M) { return (size_t)M * EN_MEM; }
OBCA_HD size_t ensemble_fin_len(int M, int nx) { return (size_t)M * nx; }

// what the integrating lane keeps of the samples it passes
struct Clear {
    double best, sample, obst, below, bad;
    RO_METHOD void init() { best = HUGE_VAL; sample = obst = -1.0; below = bad = 0.0; }
    RO_METHOD void take(double c, int q, int j) {      // ascending (q, j) and a strict <: a tie keeps the smaller index
        if (c < best) { best = c; sample = (double)q; obst = (double)j; }
        bad = val::vmax(bad, val::vbad(c));
    }
    RO_METHOD void close(double smallest, double need) { below = below + (smallest < need ? 1.0 : 0.0); }      // `below` counts samples, not items
};
// the clearance of one sample to every obstacle, as the rollout's item loop computes it
template <int VM>
struct ParkClear {
    const double *p;
    RO_METHOD void measure(const double *X, int q, double need, Clear &a) const {
        const int nOb = (int)p[PH_NOB];
        const double off = p[PH_OFF];
        double g[4];
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = p[PH_G + i];
        const double sn = sin(X[2]), cs = cos(X[2]);
        double smallest = HUGE_VAL;
        for (int j = 0; j < nOb; j++) {
            const int v = (int)p[PH_VOB + j], r0 = (int)p[PH_ROFF + j];
            double a1[VM], a2[VM], bj[VM];
#pragma unroll
            for (int i = 0; i < VM; i++) { const bool on = i < v; a1[i] = on ? p[PH_A + 2 * (r0 + i)] : 0.0; a2[i] = on ? p[PH_A + 2 * (r0 + i) + 1] : 0.0; bj[i] = on ? p[PH_B + r0 + i] : 0.0; }
            double lam[VM], mu[4], d;
            dualws_one<VM>(v, a1, a2, bj, g, X[0] + cs * off, X[1] + sn * off, cs, sn, lam, mu, &d);
            const double c = d < CL_TOUCH ? 0.0 : d;
            a.take(c, q, j);
            smallest = clr::cl_min(smallest, c);
        }
        a.close(smallest, need);
    }
};
struct QuadClear {
    const double *p;
    RO_METHOD void measure(const double *X, int q, double need, Clear &a) const {
        const double R = p[QPH_R];
        double smallest = HUGE_VAL;
        for (int j = 0; j < QOB; j++) {
            const double *ob = p + QPH_OB + QL * j;
            double d2 = 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double pi = X[i];
                const double lo = -ob[3 + i] - pi, hi = pi - ob[i];
                const double e = lo > 0.0 ? lo : (hi > 0.0 ? hi : 0.0);
                d2 = d2 + clr::cl_keep(e * e);
            }
            const double c = sqrt(d2) - R;
            a.take(c, q, j);
            smallest = clr::cl_min(smallest, c);
        }
        a.close(smallest, need);
    }
};

OBCA_FN void write_member_bad(int nx, double *rec, double *XN) {
    const double nan_ = __builtin_nan("");
    rec[EM_BAD] = 1.0;
    rec[EM_DPOS] = rec[EM_EPOS] = rec[EM_DATT] = rec[EM_DVEL] = rec[EM_DRATE] = rec[EM_MIN] = rec[EM_DU] = rec[EM_DX0] = nan_;
    rec[EM_DNODE] = rec[EM_SAMPLE] = rec[EM_OBST] = rec[EM_BELOW] = rec[EM_SAT] = rec[EM_DUNODE] = -1.0;
    rec[EM_RSV] = 0.0;
    for (int i = 0; i < nx; i++) XN[i] = nan_;
}

// Phase 3, one member in one lane.  x, u, hk as roll::integrate takes them; K: N x NU x NX of the instance; dx0: NX, dub: NU doubles of this member; cm: the clearance of a
// sample; rec: EN_MEM doubles, XN: NX doubles of this member.
template <class M, class H, class C>
OBCA_FN void member(double L, int N, int S, const double *x, const double *u, H &&hk, const double *K, const double *dx0, const double *dub, int feedback, int clamp, double need,
                    const C &cm, double *rec, double *XN) {
    double X[M::NX], bias[M::NU], b = 0.0;
#pragma unroll
    for (int i = 0; i < M::NX; i++) { X[i] = x[i] + dx0[i]; b = val::vmax(b, val::vbad(dx0[i])); }
#pragma unroll
    for (int a = 0; a < M::NU; a++) { bias[a] = dub[a]; b = val::vmax(b, val::vbad(bias[a])); }
    Clear ca; ca.init();
    double mx[RD_N] = {0.0, 0.0, 0.0, 0.0}, d[RD_N] = {0.0, 0.0, 0.0, 0.0}, node = -1.0, sat = 0.0, du = -1.0, dunode = -1.0;
    for (int k = 0; k <= N; k++) {
        const bool last = k == N;      // the last sample, q = N S: X_N is measured, nothing is stepped (ONE call site of the measurement and of the step)
        double U[M::NU], h = 0.0;
#pragma unroll
        for (int a = 0; a < M::NU; a++) U[a] = 0.0;
        if (!last) {
#pragma unroll
            for (int a = 0; a < M::NU; a++) U[a] = u[M::NU * k + a];
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
            double cl = 0.0, dm = 0.0;
#pragma unroll
            for (int a = 0; a < M::NU; a++) {
                U[a] = U[a] + bias[a];
                if (clamp) {
                    const double lo = InputBox<M>::lo(a), hi = InputBox<M>::hi(a);
                    const double c = U[a] < lo ? lo : (U[a] > hi ? hi : U[a]);
                    cl = c != U[a] ? 1.0 : cl;
                    U[a] = c;
                }
                dm = val::vmax(dm, fabs(U[a] - u[M::NU * k + a]));
            }
            sat = sat + cl;
            if (dm > du) { du = dm; dunode = (double)k; }      // ascending k: a tie keeps the smaller
            M::prep(U);
            h = hk(k) / (double)S;
        }
        const int ns = last ? 1 : S;
        for (int s = 0; s < ns; s++) {
            cm.measure(X, k * S + s, need, ca);
            if (!last) {
                const double c0 = M::pole(X);
                rk4_step<M>(L, h, U, X);
                b = val::vmax(b, c0 * M::pole(X) <= 0.0 ? 1.0 : 0.0);      // through the pole: not a state of the continuous model any more
#pragma unroll
                for (int i = 0; i < M::NX; i++) b = val::vmax(b, val::vbad(X[i]));
            }
        }
        if (!last) {
            M::dev(X, x + M::NX * (k + 1), d);
            if (d[RD_POS] > mx[RD_POS] || k == 0) { mx[RD_POS] = d[RD_POS]; node = (double)(k + 1); }      // ascending k: a tie keeps the smaller
#pragma unroll
            for (int i = 1; i < RD_N; i++) mx[i] = val::vmax(mx[i], d[i]);
        }
    }
    b = val::vmax(b, ca.bad);
    if (b != 0.0) { write_member_bad(M::NX, rec, XN); return; }
    double zero[M::NX], d0[RD_N] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < M::NX; i++) zero[i] = 0.0;
    M::dev(dx0, zero, d0);
    rec[EM_BAD] = 0.0; rec[EM_DPOS] = mx[RD_POS]; rec[EM_DNODE] = node; rec[EM_EPOS] = d[RD_POS]; rec[EM_DATT] = mx[RD_ATT]; rec[EM_DVEL] = mx[RD_VEL]; rec[EM_DRATE] = mx[RD_RATE];
    rec[EM_MIN] = ca.best; rec[EM_SAMPLE] = ca.sample; rec[EM_OBST] = ca.obst; rec[EM_BELOW] = ca.below; rec[EM_SAT] = sat; rec[EM_DU] = du; rec[EM_DUNODE] = dunode;
    rec[EM_DX0] = d0[RD_POS]; rec[EM_RSV] = 0.0;
#pragma unroll
    for (int i = 0; i < M::NX; i++) XN[i] = X[i];
}

// Phase 4, one lane: the instance record from the M member records, walked in ascending order.  inst_bad: the whole instance is (the member records are then bad too).
OBCA_FN void ensemble_reduce(int M, int S, int feedback, int clamp, int inst_bad, const double *mem, double *out) {
    const double nan_ = __builtin_nan("");
    double nbad = 0.0, nhit = 0.0, nsat = 0.0, below = 0.0, sume = 0.0, summ = 0.0;
    double mn = HUGE_VAL, mnm = -1.0, mnq = -1.0, mnj = -1.0, dp = -1.0, dpm = -1.0, dpn = -1.0, ep = -1.0, epm = -1.0, da = 0.0, dv = 0.0, dr = 0.0, du = -1.0, dum = -1.0, dun = -1.0;
    for (int m = 0; m < M; m++) {
        const double *r = mem + (size_t)m * EN_MEM;
        if (r[EM_BAD] != 0.0) { nbad = nbad + 1.0; continue; }
        if (r[EM_MIN] < mn) { mn = r[EM_MIN]; mnm = (double)m; mnq = r[EM_SAMPLE]; mnj = r[EM_OBST]; }      // strict comparisons, ascending m: ties go to the smaller member
        if (r[EM_DPOS] > dp) { dp = r[EM_DPOS]; dpm = (double)m; dpn = r[EM_DNODE]; }
        if (r[EM_EPOS] > ep) { ep = r[EM_EPOS]; epm = (double)m; }
        if (r[EM_DU] > du) { du = r[EM_DU]; dum = (double)m; dun = r[EM_DUNODE]; }
        da = val::vmax(da, r[EM_DATT]); dv = val::vmax(dv, r[EM_DVEL]); dr = val::vmax(dr, r[EM_DRATE]);
        nhit = nhit + (r[EM_BELOW] > 0.0 ? 1.0 : 0.0); nsat = nsat + (r[EM_SAT] > 0.0 ? 1.0 : 0.0);
        below = below + r[EM_BELOW]; sume = sume + r[EM_EPOS]; summ = summ + r[EM_MIN];
    }
    const double good = (double)M - nbad;
    const bool none = inst_bad || good == 0.0;
    out[EO_BAD] = inst_bad ? 1.0 : 0.0; out[EO_M] = (double)M; out[EO_SUB] = (double)S; out[EO_FEEDBACK] = (double)feedback; out[EO_CLAMP] = (double)clamp;
    out[EO_NBAD] = inst_bad ? -1.0 : nbad; out[EO_NHIT] = inst_bad ? -1.0 : nhit; out[EO_NSAT] = inst_bad ? -1.0 : nsat; out[EO_BELOW] = inst_bad ? -1.0 : below;
    out[EO_MIN] = none ? nan_ : mn; out[EO_MINMEM] = none ? -1.0 : mnm; out[EO_SAMPLE] = none ? -1.0 : mnq; out[EO_OBST] = none ? -1.0 : mnj;
    out[EO_DPOS] = none ? nan_ : dp; out[EO_DPOSMEM] = none ? -1.0 : dpm; out[EO_DNODE] = none ? -1.0 : dpn;
    out[EO_EPOS] = none ? nan_ : ep; out[EO_EPOSMEM] = none ? -1.0 : epm;
    out[EO_DATT] = none ? nan_ : da; out[EO_DVEL] = none ? nan_ : dv; out[EO_DRATE] = none ? nan_ : dr;
    out[EO_DU] = none ? nan_ : du; out[EO_DUMEM] = none ? -1.0 : dum; out[EO_DUNODE] = none ? -1.0 : dun;
    out[EO_MEANEPOS] = none ? nan_ : sume / good; out[EO_MEANMIN] = none ? nan_ : summ / good;
    for (int i = EO_RSV; i < EN_OUT; i++) out[i] = 0.0;
}
// an instance the track call marks as a whole: every member bad
OBCA_FN void write_instance_bad(int M, int nx, int S, int feedback, int clamp, double *mem, double *fin, double *out) {
    PAR(lane) {
        if (lane < M) write_member_bad(nx, mem + (size_t)lane * EN_MEM, fin + (size_t)lane * nx);
    }
    SYNC();
    PAR(lane) {
        if (lane == 0) ensemble_reduce(M, S, feedback, clamp, 1, mem, out);
    }
}

// p, z, ts, S, need, rev: as trk::track_parking_instance takes them; M: members, 1 .. EN_MMAX; dx0: 4 x M, dub: 2 x M, each member's contiguous; AB: N x 4 x 6, K: N x 2 x 4,
// mem: M x EN_MEM, fin: M x 4 of this instance; out: EN_OUT doubles.  VM: the row class of the batch's widest obstacle.  Needs 1 <= N <= OB_NMAX.
template <int VM>
OBCA_FN void ensemble_parking_instance(int N, const double *p, const double *z, const double *ts, int S, int M, int feedback, int clamp, const Weights &w, const double *dx0,
                                       const double *dub, double need, int rev, double *AB, double *K, double *mem, double *fin, double *out) {
    Lay l; make_layout(N, (int)p[PH_NOB], (int)p[PH_M], l);
    const double Ts = p[PH_TS];
    const double t1 = p[PH_FIX] != 0.0 ? 1.0 : z[l.t];
    double bad[OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vmax(val::vbad(Ts), ts ? 0.0 : val::vbad(t1)) : 0.0;
        for (int i = lane; i < 4 * (N + 1); i += OB_NT) b = val::vmax(b, val::vbad(z[l.x + i]));
        for (int i = lane; i < 2 * N; i += OB_NT) b = val::vmax(b, val::vbad(z[l.u + i]));
        if (ts) for (int i = lane; i < N + 1; i += OB_NT) b = val::vmax(b, val::vbad(ts[i]));
        bad[LI(lane)] = b;
    }
    double ib = wred_max(bad);
    if (ib == 0.0) {
        linearise<ParkModel>(p[PH_L], N, S, z + l.x, z + l.u, [&](int k) { return (ts ? ts[k] : t1) * Ts; }, rev, AB);
        ib = riccati<ParkModel>(N, w, AB, K);
    }
    if (ib != 0.0) { write_instance_bad(M, 4, S, feedback, clamp, mem, fin, out); return; }
    SYNC();      // the gains have landed
    const ParkClear<VM> cm = {p};
    PAR(lane) {
        if (lane < M)
            member<ParkModel>(p[PH_L], N, S, z + l.x, z + l.u, [&](int k) { return (ts ? ts[k] : t1) * Ts; }, K, dx0 + 4 * lane, dub + 2 * lane, feedback, clamp, need, cm,
                              mem + (size_t)lane * EN_MEM, fin + (size_t)lane * 4);
    }
    SYNC();
    PAR(lane) {
        if (lane == 0) ensemble_reduce(M, S, feedback, clamp, 0, mem, out);
    }
}

// p, x, u, ts, tstride, S, need, rev: as trk::track_quad_instance takes them; dx0: 12 x M, dub: 4 x M; AB: N x 12 x 16, K: N x 4 x 12, mem: M x EN_MEM, fin: M x 12.
OBCA_FN void ensemble_quad_instance(int N, const double *p, const double *x, const double *u, const double *ts, int tstride, int S, int M, int feedback, int clamp, const Weights &w,
                                    const double *dx0, const double *dub, double need, int rev, double *AB, double *K, double *mem, double *fin, double *out) {
    const double Ts = p[QPH_TS];
    double bad[OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vbad(Ts) : 0.0;
        for (int i = lane; i < QX * (N + 1); i += QNT) b = val::vmax(b, val::vbad(x[i]));
        for (int i = lane; i < QU * N; i += QNT) b = val::vmax(b, val::vbad(u[i]));
        for (int i = lane; i < N + 1; i += QNT) b = val::vmax(b, val::vbad(ts[i * tstride]));
        bad[LI(lane)] = b;
    }
    double ib = wred_max(bad);
    if (ib == 0.0) {
        linearise<QuadModel>(0.0, N, S, x, u, [&](int k) { return ts[k * tstride] * Ts; }, rev, AB);
        ib = riccati<QuadModel>(N, w, AB, K);
    }
    if (ib != 0.0) { write_instance_bad(M, QX, S, feedback, clamp, mem, fin, out); return; }
    SYNC();      // the gains have landed
    const QuadClear cm = {p};
    PAR(lane) {
        if (lane < M)
            member<QuadModel>(0.0, N, S, x, u, [&](int k) { return ts[k * tstride] * Ts; }, K, dx0 + QX * lane, dub + QU * lane, feedback, clamp, need, cm,
                              mem + (size_t)lane * EN_MEM, fin + (size_t)lane * QX);
    }
    SYNC();
    PAR(lane) {
        if (lane == 0) ensemble_reduce(M, S, feedback, clamp, 0, mem, out);
    }
}

}  // namespace ens
}  // namespace obca
