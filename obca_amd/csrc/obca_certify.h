// obca_certify.h -- a CERTIFICATE of clearance along the whole path of a trajectory, on the device: clearance() (the clearance check's kernel text, namespace clr) looks at S poses per interval and says nothing
// about what lies between them.  Here every (interval, obstacle) pair is walked by conservative advancement: a pose with clearance c clears the stretch of the path on which no
// point of the vehicle can have moved farther than c, and the next sample goes to the end of that stretch.  One wavefront (64 lanes) per instance; obca_amd/validate.py
// (certify_lipschitz_parking, certify_lipschitz_quad, certify_parking, certify_quad, certify_record) is the numpy statement and is normative for everything but the distances.
//   path       : the one clearance() samples.  Interval k = 0 .. N-1 is tau in [0, h_k], h_k = ts_k Ts (ts_k: the caller's timeScale[k]; a resident batch: the solution's single
//                t, 1 with fixTime).  Positions are counted in ticks m = 0 .. G, G = CT_TICKS = 4096: tau = h_k m / G, with m / G exact in fp64 -- host build and device visit the
//                same poses.  parking: val::park_step from node k with u_k over the fraction (m / G) ts_k of Ts (= tau / Ts); quadcopter: p_k + tau v_k, tau = (m / G) ts_k Ts.
//                At m = 0 the pose is the node itself, bit for bit; at m = s G / S with S a power of two it is sample (k, s) of clearance(), bit for bit.  Node N is one
//                further sample per obstacle.  THE CERTIFICATE IS ABOUT THIS PIECEWISE PATH: the end of interval k (m = G) and node k + 1 differ by the dynamics residual of the
//                solve; node k + 1 is checked as the first sample of interval k + 1, the end point of interval k is covered by the stretch in front of it but never sampled.
//   clearance  : what clearance() computes.  parking: dualws_one<VM> of the pose against obstacle j, 0 where it returns less than CL_TOUCH; quadcopter: the distance of the point
//                to box j (0 inside) minus R.  A distance between convex bodies is 1-Lipschitz in the largest displacement of the moving body's points.
//   speed bound: Lambda_k [m per unit tau], constant over the interval, with |h| = |h_k|.
//                parking, v = x_k[3], a = u_k[1], tn = |tan u_k[0]|: V = max(|v|, |v + h a|), Sm = max(|v|, |v + h a / 2|), rho = sqrt((|off| + g_0)^2 + g_1^2) the car point
//                farthest from the reference point (PH_OFF, PH_G of the problem record); Lambda_k = V + |h| Sm |v| tn / (2 L) + rho V tn / L: the first two terms bound
//                |d(X, Y) / dtau| of park_step, the third rho |dpsi / dtau|.  quadcopter: Lambda_k = |v_k|, the Euclidean norm of x_k[6:9].
//   advancement: work items are (interval k, obstacle j), item = k nOb + j, and the nOb items (N, j) of node N (one sample each: their Lambda is 0).  From m = 0:
//                  1. c = clearance of the pose at tick m; c < need: the item is VIOLATED (it goes on)
//                  2. e = c >= need ? c - need + slack : slack
//                  3. Lambda_k |h| == 0 or e >= Lambda_k |h| (G - m) / G: dm = G - m; else dm = clamp(floor(G e / (Lambda_k |h|)), 1, G - m)   (flooring only shortens a step)
//                  4. proven on [m, m + dm]: clearance >= c - Lambda_k |h| dm / G; the item's lb is the smallest of these bounds, its `seen` the smallest c
//                  5. m += dm; done at m == G.  An item still running after max_steps samples is UNDECIDED: lb = -inf.
//   guarantees : every step with c >= need proves >= need - slack ahead of it; so min(need, seen) - slack <= lb <= the true minimum over the path <= seen for a decided item;
//                a decided instance with no violated item has clearance >= need - slack on the whole path.  With `need` above every clearance the call is uniform sampling at
//                spacing slack / Lambda, and seen - slack bounds the true continuous minimum.
// Lanes take the items as clr::cl_item deals them (`rev` deals them backwards): item loops have very unequal lengths (one sample for a far obstacle, tens for a near one), so
// they go round-robin and are not padded.  An item leaves (lb, seen, tick of seen, tick of its first violation, samples) in `work` (LDS on the device, CT_ITEM doubles per
// item); after the items lanes take INTERVALS: the smallest lb and seen over the obstacles go to iv[2 k], iv[2 k + 1] (k = 0 .. N; an undecided item makes lb_k -inf), and
// the instance record is reduced from the items with the tie rules of clearance(): the smallest value first, then the smallest (interval, tick, obstacle).  Nothing depends on
// how the items were dealt.  No atomics.
// Record (CT_OUT doubles): lb, seen, interval / tick / obstacle of seen, violated (intervals with a sample under need; node N counts as one), interval / tick / obstacle of the
// first violation in the order (interval, tick, obstacle) (-1: none), undecided items, samples taken, most samples of one item, the largest Lambda_k, certified, bad, 0.
// bad = 1: a non-finite number among what clearance() scans, a non-finite clearance or a non-finite Lambda_k |h|: then lb, seen, Lambda and every iv entry are NaN, the six
// indices -1, violated = N + 1, undecided = the items, the sample counts 0, certified 0.  Nothing but the finite scan is guaranteed to have run on such an instance.
// Products that must agree to the bit between host build and device are kept out of contraction with clr::cl_keep; the parking distance is an iteration that agrees to 1e-9,
// and tan is libm's / the device library's.  The same text compiles for the host (-DOBCA_EMU) for tests/emu/certify_emu.cpp.  Nothing here is used by any other kernel.
#pragma once
#include "obca_validate.h"
#ifndef CL_OUT
#error "include the clearance check's kernel text (namespace clr) before this header: its dealing of the items, cl_keep, cl_min and CL_TOUCH are reused unchanged"
#endif

namespace obca {
namespace cert {

#define CT_OUT 16            // doubles per instance (= OBCA_CERT_OUT of include/obca_certify.h)
#define CT_TICKS 4096        // G: ticks per interval, a power of two (= OBCA_CERT_TICKS)
#define CT_ITEM 3            // doubles an item leaves in `work`: lb, seen, tick of seen + 8192 (tick of the first violation (G: none) + 8192 samples)
enum { CT_LB = 0, CT_SEEN, CT_SIV, CT_STICK, CT_SOBST, CT_VIOL, CT_VIV, CT_VTICK, CT_VOBST, CT_UNDEC, CT_SAMPLES, CT_MOST, CT_LAMBDA, CT_CERT, CT_BAD, CT_RSV };
enum { CC_LB = 0, CC_SEEN, CC_SKEY, CC_VKEY, CC_NVIOL, CC_UNDEC, CC_TOT, CC_MOST, CC_LAM, CC_BAD, CC_N };      // per-lane accumulators
static_assert((CT_TICKS & (CT_TICKS - 1)) == 0 && CT_TICKS < 8192, "m / G is exact and a tick fits the packing of an item's counts");

// the refusals of the entry points, one text for the library and the host build
static inline const char *certify_check_args(double need, double slack, int max_steps) {
    if (!(need - need == 0.0)) return "need a finite `need`";
    if (!(slack - slack == 0.0) || !(slack > 0.0)) return "need a finite `slack` > 0";
    if (max_steps < 1 || max_steps > CT_TICKS) return "need 1 <= max_steps <= 4096";
    return nullptr;
}
// doubles of `work` for an instance of horizon N with nOb obstacles, and of its interval array
OBCA_HD size_t certify_work_len(int N, int nOb) { return (size_t)CT_ITEM * (size_t)(N + 1) * (size_t)nOb; }
OBCA_HD size_t certify_iv_len(int N) { return (size_t)2 * (size_t)(N + 1); }

// Lambda of a parking interval: x node k, u its input, h = ts_k Ts, rho the farthest car point
OBCA_FN double lipschitz_parking(const double x[4], const double u[2], double h, double L, double rho) {
    const double av = fabs(x[3]), tn = fabs(tan(u[0])), ha = clr::cl_keep(h * u[1]);
    const double V = val::vmax(av, fabs(x[3] + ha)), Sm = val::vmax(av, fabs(x[3] + ha / 2));
    const double t2 = clr::cl_keep(clr::cl_keep(clr::cl_keep(fabs(h) * Sm) * av) * tn) / (2 * L), t3 = clr::cl_keep(clr::cl_keep(rho * V) * tn) / L;
    return (V + t2) + t3;
}
OBCA_FN double car_radius(double off, double g0, double g1) { const double a = fabs(off) + g0; return sqrt(clr::cl_keep(a * a) + clr::cl_keep(g1 * g1)); }
// Lambda of a quadcopter interval: |v_k|
OBCA_FN double lipschitz_quad(const double *xk) { return sqrt((clr::cl_keep(xk[6] * xk[6]) + clr::cl_keep(xk[7] * xk[7])) + clr::cl_keep(xk[8] * xk[8])); }

// the state of one item's walk
struct Walk { double lb, seen; int m, tseen, tviol, steps; };
OBCA_FN void walk_init(Walk &w) { w.lb = HUGE_VAL; w.seen = HUGE_VAL; w.m = 0; w.tseen = 0; w.tviol = CT_TICKS; w.steps = 0; }
// steps 1-5 for the sample c at tick w.m; Lh = Lambda_k |h|.  Returns false when the item is finished (done, or undecided: lb = -inf)
OBCA_FN bool walk_take(Walk &w, double c, double Lh, double need, double slack, int max_steps) {
    const int rem = CT_TICKS - w.m;
    w.steps++;
    if (c < need && w.tviol == CT_TICKS) w.tviol = w.m;
    if (c < w.seen) { w.seen = c; w.tseen = w.m; }
    const double e = c >= need ? (c - need) + slack : slack;
    int dm = rem;
    if (!(Lh == 0.0 || e >= clr::cl_keep(Lh * (double)rem) / CT_TICKS)) {
        const double f = floor((CT_TICKS * e) / Lh);
        dm = f >= 1.0 ? (f < (double)rem ? (int)f : rem) : 1;
    }
    w.lb = clr::cl_min(w.lb, c - clr::cl_keep(Lh * (double)dm) / CT_TICKS);
    w.m += dm;
    if (w.m == CT_TICKS) return false;
    if (w.steps == max_steps) { w.lb = -HUGE_VAL; return false; }
    return true;
}
OBCA_FN void walk_store(const Walk &w, double *item) {
    item[0] = w.lb; item[1] = w.seen; item[2] = (double)w.tseen + 8192.0 * ((double)w.tviol + 8192.0 * (double)w.steps);
}

OBCA_FN void write_bad(int N, int nOb, double *iv, double *out) {
    PAR(lane) {
        const double nan_ = __builtin_nan("");
        for (int i = lane; i < 2 * (N + 1); i += OB_NT) iv[i] = nan_;
        if (lane == 0) {
            out[CT_LB] = out[CT_SEEN] = out[CT_LAMBDA] = nan_;
            out[CT_SIV] = out[CT_STICK] = out[CT_SOBST] = out[CT_VIV] = out[CT_VTICK] = out[CT_VOBST] = -1.0;
            out[CT_VIOL] = (double)(N + 1); out[CT_UNDEC] = (double)((N + 1) * nOb); out[CT_SAMPLES] = out[CT_MOST] = 0.0; out[CT_CERT] = 0.0; out[CT_BAD] = 1.0; out[CT_RSV] = 0.0;
        }
    }
}
// the items of `work` -> the interval array and the instance record.  lam: the lanes' largest Lambda_k; bad: their bad flags
OBCA_FN void write_record(int N, int nOb, const double *work, const double (&lam)[OBCA_NL], const double (&bad)[OBCA_NL], double *iv, double *out) {
    if (wred_max(bad) != 0.0) { write_bad(N, nOb, iv, out); return; }
    double acc[CC_N][OBCA_NL];
    PAR(lane) {
        double a[CC_N];
        a[CC_LB] = a[CC_SEEN] = a[CC_SKEY] = a[CC_VKEY] = HUGE_VAL;
        a[CC_NVIOL] = a[CC_UNDEC] = a[CC_TOT] = a[CC_MOST] = 0.0;
        for (int k = lane; k <= N; k += OB_NT) {
            double lbk = HUGE_VAL, sk = HUGE_VAL;
            bool vk = false;
            for (int j = 0; j < nOb; j++) {
                const double *w = work + (size_t)CT_ITEM * (size_t)(k * nOb + j);
                const long long pk = (long long)w[2];
                const int tseen = (int)(pk & 8191), tviol = (int)((pk >> 13) & 8191), steps = (int)(pk >> 26);
                lbk = clr::cl_min(lbk, w[0]); sk = clr::cl_min(sk, w[1]);
                const double key = ((double)k * CT_TICKS + (double)tseen) * CL_NPO + (double)j;
                if (w[1] < a[CC_SEEN] || (w[1] == a[CC_SEEN] && key < a[CC_SKEY])) { a[CC_SEEN] = w[1]; a[CC_SKEY] = key; }
                if (tviol < CT_TICKS) {
                    const double vkey = ((double)k * CT_TICKS + (double)tviol) * CL_NPO + (double)j;
                    vk = true;
                    if (vkey < a[CC_VKEY]) a[CC_VKEY] = vkey;
                }
                if (w[0] == -HUGE_VAL) a[CC_UNDEC] += 1.0;
                a[CC_TOT] += (double)steps;
                if ((double)steps > a[CC_MOST]) a[CC_MOST] = (double)steps;
            }
            iv[2 * k] = lbk; iv[2 * k + 1] = sk;
            a[CC_LB] = clr::cl_min(a[CC_LB], lbk);
            if (vk) a[CC_NVIOL] += 1.0;
        }
#pragma unroll
        for (int i = 0; i < CC_LAM; i++) acc[i][LI(lane)] = a[i];
    }
    const double lb = wred_min(acc[CC_LB]), seen = wred_min(acc[CC_SEEN]);
    double kk[OBCA_NL];
    PAR(lane) { kk[LI(lane)] = acc[CC_SEEN][LI(lane)] == seen ? acc[CC_SKEY][LI(lane)] : HUGE_VAL; }
    const double skey = wred_min(kk), vkey = wred_min(acc[CC_VKEY]);
    const double nviol = wred_sum(acc[CC_NVIOL]), und = wred_sum(acc[CC_UNDEC]), tot = wred_sum(acc[CC_TOT]), most = wred_max(acc[CC_MOST]), lmax = wred_max(lam);      // (integers below 2^53: the sums are exact in any order)
    PAR(lane) {
        if (lane == 0) {
            const long long sk = (long long)skey, vk = vkey < HUGE_VAL ? (long long)vkey : -1;
            out[CT_LB] = lb; out[CT_SEEN] = seen;
            out[CT_SIV] = (double)(sk / ((long long)CL_NPO * CT_TICKS)); out[CT_STICK] = (double)((sk / CL_NPO) % CT_TICKS); out[CT_SOBST] = (double)(sk % CL_NPO);
            out[CT_VIOL] = nviol;
            out[CT_VIV] = vk < 0 ? -1.0 : (double)(vk / ((long long)CL_NPO * CT_TICKS)); out[CT_VTICK] = vk < 0 ? -1.0 : (double)((vk / CL_NPO) % CT_TICKS); out[CT_VOBST] = vk < 0 ? -1.0 : (double)(vk % CL_NPO);
            out[CT_UNDEC] = und; out[CT_SAMPLES] = tot; out[CT_MOST] = most; out[CT_LAMBDA] = lmax;
            out[CT_CERT] = (nviol == 0.0 && und == 0.0) ? 1.0 : 0.0; out[CT_BAD] = 0.0; out[CT_RSV] = 0.0;
        }
    }
}

// p: problem header (PH_*: unit-length rows), z: a point in the solver's layout (x, u and t are read); ts: the caller's timeScale per stage (N + 1; nullptr: the point's
// single t, 1 with fixTime); work: certify_work_len(N, nOb) doubles (LDS on the device); iv: 2 (N + 1) doubles; out: CT_OUT doubles.  VM: the row class of the batch's widest
// obstacle, as launch_dualws picks it.  Needs 1 <= N <= OB_NMAX and arguments that certify_check_args accepts.
template <int VM>
OBCA_FN void certify_parking_instance(int N, const double *p, const double *z, const double *ts, double need, double slack, int max_steps, int rev, double *work, double *iv, double *out) {
    const int nOb = (int)p[PH_NOB], M = (int)p[PH_M];
    Lay l; make_layout(N, nOb, M, l);
    const double Ts = p[PH_TS], L = p[PH_L], off = p[PH_OFF];
    const double t1 = p[PH_FIX] != 0.0 ? 1.0 : z[l.t];
    const int nIt = (N + 1) * nOb, rounds = (nIt + OB_NT - 1) / OB_NT;
    double bad[OBCA_NL], lam[OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vmax(val::vbad(Ts), ts ? 0.0 : val::vbad(t1)) : 0.0;
        for (int i = lane; i < 4 * (N + 1); i += OB_NT) b = val::vmax(b, val::vbad(z[l.x + i]));
        for (int i = lane; i < 2 * N; i += OB_NT) b = val::vmax(b, val::vbad(z[l.u + i]));
        if (ts) for (int i = lane; i < N + 1; i += OB_NT) b = val::vmax(b, val::vbad(ts[i]));
        bad[LI(lane)] = b;
    }
    if (wred_max(bad) != 0.0) { write_bad(N, nOb, iv, out); return; }
    PAR(lane) {
        double g[4], b = 0.0, lmax = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = p[PH_G + i];
        const double rho = car_radius(off, g[0], g[1]);
        for (int r = 0; r < rounds; r++) {
            const int it = clr::cl_item(r, rounds, lane, rev);
            if (it >= nIt) continue;
            const int k = it / nOb, j = it - k * nOb;
            const int v = (int)p[PH_VOB + j], r0 = (int)p[PH_ROFF + j];
            double a1[VM], a2[VM], bj[VM];
#pragma unroll
            for (int i = 0; i < VM; i++) { const bool on = i < v; a1[i] = on ? p[PH_A + 2 * (r0 + i)] : 0.0; a2[i] = on ? p[PH_A + 2 * (r0 + i) + 1] : 0.0; bj[i] = on ? p[PH_B + r0 + i] : 0.0; }
            double xk[4], u[2] = {0.0, 0.0}, tk = 0.0, Lh = 0.0;
#pragma unroll
            for (int i = 0; i < 4; i++) xk[i] = z[l.x + 4 * k + i];
            if (k < N) {      // (the items of node N take one sample: Lh = 0)
                u[0] = z[l.u + 2 * k]; u[1] = z[l.u + 2 * k + 1];
                tk = ts ? ts[k] : t1;
                const double h = clr::cl_keep(tk * Ts), Lam = lipschitz_parking(xk, u, h, L, rho);
                Lh = clr::cl_keep(Lam * fabs(h));
                lmax = val::vmax(lmax, Lam);
                b = val::vmax(b, val::vbad(Lh));
            }
            Walk w; walk_init(w);
            bool go = b == 0.0;
            while (go) {
                double x[4];
#pragma unroll
                for (int i = 0; i < 4; i++) x[i] = xk[i];
                if (w.m) {
                    double F[4];
                    val::park_step(Ts, L, xk, u, (double)w.m / (double)CT_TICKS * tk, F);
#pragma unroll
                    for (int i = 0; i < 4; i++) x[i] = F[i];
                }
                const double sn = sin(x[2]), cs = cos(x[2]);
                double lm[VM], mu[4], d;
                dualws_one<VM>(v, a1, a2, bj, g, x[0] + cs * off, x[1] + sn * off, cs, sn, lm, mu, &d);
                const double c = d < CL_TOUCH ? 0.0 : d;
                if (val::vbad(c) != 0.0) { b = 1.0; break; }
                go = walk_take(w, c, Lh, need, slack, max_steps);
            }
            walk_store(w, work + (size_t)CT_ITEM * (size_t)it);
        }
        bad[LI(lane)] = b; lam[LI(lane)] = lmax;
    }
    SYNC();
    write_record(N, nOb, work, lam, bad, iv, out);
}

// p: quadcopter problem header (QPH_*: Ts, R, the boxes as [hi; -lo]); x: 12 x (N + 1) stage-contiguous (positions 0-2, velocities 6-8); ts[k * tstride] is timeScale[k]
// (tstride 0: one t); work: certify_work_len(N, QOB) doubles; iv: 2 (N + 1); out: CT_OUT doubles.  Needs 1 <= N <= QNMAX.
OBCA_FN void certify_quad_instance(int N, const double *p, const double *x, const double *ts, int tstride, double need, double slack, int max_steps, int rev, double *work, double *iv, double *out) {
    const double Ts = p[QPH_TS], R = p[QPH_R];
    const int nIt = (N + 1) * QOB, rounds = (nIt + QNT - 1) / QNT;
    double bad[OBCA_NL], lam[OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vbad(Ts) : 0.0;
        for (int i = lane; i < QX * (N + 1); i += QNT) b = val::vmax(b, val::vbad(x[i]));
        for (int i = lane; i < N + 1; i += QNT) b = val::vmax(b, val::vbad(ts[i * tstride]));
        bad[LI(lane)] = b;
    }
    if (wred_max(bad) != 0.0) { write_bad(N, QOB, iv, out); return; }
    PAR(lane) {
        double b = 0.0, lmax = 0.0;
        for (int r = 0; r < rounds; r++) {
            const int it = clr::cl_item(r, rounds, lane, rev);
            if (it >= nIt) continue;
            const int k = it / QOB, j = it - k * QOB;
            const double *ob = p + QPH_OB + QL * j, *xk = x + QX * k;
            double tk = 0.0, Lh = 0.0;
            if (k < N) {
                tk = ts[k * tstride];
                const double h = clr::cl_keep(tk * Ts), Lam = lipschitz_quad(xk);
                Lh = clr::cl_keep(Lam * fabs(h));
                lmax = val::vmax(lmax, Lam);
                b = val::vmax(b, val::vbad(Lh));
            }
            Walk w; walk_init(w);
            bool go = b == 0.0;
            while (go) {
                const double tau = (double)w.m / (double)CT_TICKS * tk * Ts;
                double d2 = 0.0;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const double pi = w.m ? xk[i] + clr::cl_keep(tau * xk[6 + i]) : xk[i];
                    const double lo = -ob[3 + i] - pi, hi = pi - ob[i];
                    const double e = lo > 0.0 ? lo : (hi > 0.0 ? hi : 0.0);
                    d2 = d2 + clr::cl_keep(e * e);
                }
                const double c = sqrt(d2) - R;
                if (val::vbad(c) != 0.0) { b = 1.0; break; }
                go = walk_take(w, c, Lh, need, slack, max_steps);
            }
            walk_store(w, work + (size_t)CT_ITEM * (size_t)it);
        }
        bad[LI(lane)] = b; lam[LI(lane)] = lmax;
    }
    SYNC();
    write_record(N, QOB, work, lam, bad, iv, out);
}

}  // namespace cert
}  // namespace obca
