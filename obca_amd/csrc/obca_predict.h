// obca_predict.h -- clearance of a HELD trajectory against obstacles that MOVE while it is executed, on the device: one wavefront (64 lanes) per instance, one launch.  The
// clearance check between the nodes freezes the scene for the whole horizon; here every sample is measured against the obstacles where they will be when the vehicle gets
// there.  obca_amd/validate.py (predict_parking, predict_quad, predict_record) is the numpy statement: for every sample, move_obstacles by rate * tau, then measure.
//   samples  : those of the clearance check, q = k S + s and q = N S, the same poses.  New is the time a sample is reached: cum[0] = 0, cum[k + 1] = cum[k] + ts_k summed in
//              stage order, tau_q = (cum[k] + (s / S) ts_k) Ts, s / S formed as the clearance check forms it, the product kept from fusing with the sum (cl_keep): host
//              build and device get the same bits of tau.  A resident batch has its one t (1 with fixTime) for every ts_k.
//   parking  : rt holds PR_PIN doubles per obstacle j, [vx, vy, w, cx, cy, g] -- the record of the scene edit's move, read as rates.  At sample q obstacle j is the image
//              the move would make of it with motion (vx tau, vy tau, w tau), pivot (cx, cy) and inflation g tau, row by row in the move's order:
//                a' = R(w tau) a  (w tau == 0: skipped),  b' = ((b + a'.(c + d)) - a.c) + m  (d, w tau and m all 0: skipped)
//              and the clearance of the pose to the moved rows is dualws_one<VM> with the CL_TOUCH rule.  The rows of the record are never written.
//   quadcopter: PR_QIN doubles per box, [vx, vy, vz, g]: word i < 3 is (ob[i] + v_i tau) + g tau, word 3 + i is (ob[3 + i] - v_i tau) + g tau; a word whose two terms are 0
//              keeps its bits.  Clearance = distance of the point to that box - R.
// Whole samples are dealt to the lanes (sample cl_item(round, lane)); a lane walks the obstacles of its sample, so the smallest clearance of a sample is lane-local: it is
// the profile entry, and the lane that owns a sample is the one writer of prof[q] and of the sample's mark.  The sine and cosine of w tau are made per item, only where
// w tau != 0.  Nothing depends on the dealing (`rev` deals backwards; the host build's test asks for the same bits).
// Record (PR_OUT doubles): [0 .. 23] the clearance record, written by clr::write_record from the clr::acc_* accumulators as they are; then
//   [24] first = q of the first sample whose smallest clearance is < need (-1: none)      [25] t_first = its tau in seconds (+inf: none)
//   [26] first_obstacle = the smallest j under need at that sample (-1: none)             [27] t_min = tau of sample [2]
//   [28] horizon = tau of the last sample                                                 [29] moving = obstacles with vx, vy(, vz), w or g != 0 (a pivot alone moves nothing)
//   [30], [31] 0
// first and first_obstacle: one more per-lane accumulator, the smallest key q * CL_NPO + j among the items under need, then one wave minimum.
// bad: what the clearance check calls bad, or a non-finite rate, or a moved word that is not finite.  Then [0 .. 23] are the bad clearance record, [24] = [26] = -1,
// [25] = [27] = [28] = NaN, [29] = 0, and the profile row is NaN.
// Profile (prof != nullptr): the smallest clearance of every sample over the obstacles, N S + 1 doubles per instance.
// LDS: the marks of the clearance check (4 KB) and cum[] (at most 129 doubles), filled once per instance by one lane in stage order.  No atomics: every word of global
// memory and of LDS has one writer.  The same text compiles for the host (-DOBCA_EMU) for tests/emu/predict_emu.cpp.  Nothing here is used by the solve kernels, and no
// existing device function changes.
#pragma once
#if !defined(PV_OUT) || !defined(CL_OUT)
#error "include the validate and the clearance kernel texts (val::vbad, vmax, park_step; clr::acc_*, write_record, cl_keep; dualws_one; the wave reductions) before this header"
#endif

namespace obca {
namespace prd {

#define PR_OUT 32            // doubles per instance (= OBCA_PRD_OUT of include/obca_predict.h)
#define PR_PIN 6             // doubles per parking obstacle: vx, vy, w, cx, cy, g
#define PR_QIN 4             // doubles per box: vx, vy, vz, g
enum { PR_FIRST = CL_OUT, PR_TFIRST, PR_FIRSTOB, PR_TMIN, PR_HORIZON, PR_MOVING, PR_RSV0, PR_RSV1 };
static_assert(PR_RSV1 + 1 == PR_OUT && QNMAX <= OB_NMAX && OB_NT == QNT, "the tail follows the clearance record; cum[] holds every stage of either vehicle");

// timeScale of stage k: the caller's array (stride tstride) or the point's single t
OBCA_FN double pr_ts(const double *ts, int tstride, double t1, int k) { return ts ? ts[(size_t)k * tstride] : t1; }
// the time at which sample (k, s) is reached [s]
OBCA_FN double pr_tau(const double *cum, int k, int s, int S, double tsk, double Ts) { return s ? (cum[k] + clr::cl_keep((double)s / (double)S * tsk)) * Ts : cum[k] * Ts; }
OBCA_FN double pr_tau_of(const double *cum, int q, int S, const double *ts, int tstride, double t1, double Ts) {
    const int k = q / S, s = q - k * S;
    return pr_tau(cum, k, s, S, s ? pr_ts(ts, tstride, t1, k) : 0.0, Ts);
}
// lane 0 sums the stages in stage order
OBCA_FN void pr_fill_cum(double *cum, int N, const double *ts, int tstride, double t1) {
    cum[0] = 0.0;
    for (int k = 0; k < N; k++) cum[k + 1] = cum[k] + pr_ts(ts, tstride, t1, k);
}

// the tail of a bad instance and its profile row; the lanes write the samples they were dealt
OBCA_FN void write_bad_tail(int nS, int rev, double *out, double *prof) {
    const int rounds = (nS + OB_NT - 1) / OB_NT;
    PAR(lane) {
        const double nan_ = __builtin_nan("");
        if (lane == 0) {
            out[PR_FIRST] = out[PR_FIRSTOB] = -1.0; out[PR_TFIRST] = out[PR_TMIN] = out[PR_HORIZON] = nan_; out[PR_MOVING] = out[PR_RSV0] = out[PR_RSV1] = 0.0;
        }
        if (prof) for (int r = 0; r < rounds; r++) { const int q = clr::cl_item(r, rounds, lane, rev); if (q < nS) prof[q] = nan_; }
    }
}
// acc, hit: as clr::write_record takes them; fk: the lanes' smallest key among the items under need (HUGE_VAL: none); mv: the lanes' counts of moving obstacles
OBCA_FN void write_all(int N, int S, int nOb, double (&acc)[clr::CA_N][OBCA_NL], const unsigned char *hit, double (&fk)[OBCA_NL], double (&mv)[OBCA_NL], const double *cum,
                       const double *ts, int tstride, double t1, double Ts, int rev, double *out, double *prof) {
    const int nS = N * S + 1;
    const double isbad = wred_max(acc[clr::CA_BAD]);
    clr::write_record(nS, nOb, acc, hit, out);
    if (isbad != 0.0) { write_bad_tail(nS, rev, out, prof); return; }
    const double key = wred_min(fk), moving = wred_sum(mv);
    PAR(lane) {
        if (lane == 0) {
            const bool none = !(key < HUGE_VAL);
            const int ik = none ? 0 : (int)key, qf = ik / CL_NPO, qm = (int)out[clr::CL_SAMPLE];      // (this lane wrote CL_SAMPLE in write_record)
            out[PR_FIRST] = none ? -1.0 : (double)qf; out[PR_FIRSTOB] = none ? -1.0 : (double)(ik % CL_NPO);
            out[PR_TFIRST] = none ? HUGE_VAL : pr_tau_of(cum, qf, S, ts, tstride, t1, Ts);
            out[PR_TMIN] = pr_tau_of(cum, qm, S, ts, tstride, t1, Ts);
            out[PR_HORIZON] = cum[N] * Ts;
            out[PR_MOVING] = moving; out[PR_RSV0] = out[PR_RSV1] = 0.0;
        }
    }
}

// p: problem header (PH_*: unit-length rows, read only), z: a point in the solver's layout (x, u and t are read); ts: the caller's timeScale per stage (N + 1; nullptr: the
// point's single t, 1 with fixTime); rt: PR_PIN doubles per obstacle; S: sub-steps, 1 .. CL_SMAX; out: PR_OUT doubles; prof: N S + 1 doubles or nullptr.  VM: the row class
// of the batch's widest obstacle.  Needs 1 <= N <= OB_NMAX.
template <int VM>
OBCA_FN void predict_parking_instance(int N, const double *p, const double *z, const double *ts, const double *rt, int S, double need, int rev, double *out, double *prof) {
    CL_LDS unsigned char hit[CL_MAXSAMPLES];
    CL_LDS double cum[OB_NMAX + 1];
    const int nOb = (int)p[PH_NOB], M = (int)p[PH_M];
    Lay l; make_layout(N, nOb, M, l);
    const double Ts = p[PH_TS], L = p[PH_L], off = p[PH_OFF];
    const double t1 = p[PH_FIX] != 0.0 ? 1.0 : z[l.t];
    const int nS = N * S + 1, rounds = (nS + OB_NT - 1) / OB_NT;
    double acc[clr::CA_N][OBCA_NL], fk[OBCA_NL], mv[OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vmax(val::vbad(Ts), ts ? 0.0 : val::vbad(t1)) : 0.0;
        for (int i = lane; i < 4 * (N + 1); i += OB_NT) b = val::vmax(b, val::vbad(z[l.x + i]));
        for (int i = lane; i < 2 * N; i += OB_NT) b = val::vmax(b, val::vbad(z[l.u + i]));
        if (ts) for (int i = lane; i < N + 1; i += OB_NT) b = val::vmax(b, val::vbad(ts[i]));
        for (int i = lane; i < PR_PIN * nOb; i += OB_NT) b = val::vmax(b, val::vbad(rt[i]));
        double m = 0.0;
        for (int j = lane; j < nOb; j += OB_NT) { const double *r = rt + PR_PIN * j; if (r[0] != 0.0 || r[1] != 0.0 || r[2] != 0.0 || r[5] != 0.0) m += 1.0; }
        acc[clr::CA_BAD][LI(lane)] = b; mv[LI(lane)] = m;
        for (int q = lane; q < nS; q += OB_NT) hit[q] = 0;
        if (lane == 0) pr_fill_cum(cum, N, ts, 1, t1);
    }
    if (wred_max(acc[clr::CA_BAD]) != 0.0) { clr::write_bad(nS, out); write_bad_tail(nS, rev, out, prof); return; }
    SYNC();
    PAR(lane) {
        double a[clr::CA_N], g[4], f = HUGE_VAL;
        clr::acc_init(a);
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = p[PH_G + i];
        for (int r = 0; r < rounds; r++) {
            const int q = clr::cl_item(r, rounds, lane, rev);
            if (q >= nS) continue;
            const int k = q / S, s = q - k * S;
            const double tsk = s ? (ts ? ts[k] : t1) : 0.0;
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; i++) x[i] = z[l.x + 4 * k + i];
            if (s) {      // (k < N here: the last sample has s = 0)
                const double u[2] = {z[l.u + 2 * k], z[l.u + 2 * k + 1]};
                double F[4];
                val::park_step(Ts, L, x, u, (double)s / (double)S * tsk, F);
#pragma unroll
                for (int i = 0; i < 4; i++) x[i] = F[i];
            }
            const double sn = sin(x[2]), cs = cos(x[2]), tau = pr_tau(cum, k, s, S, tsk, Ts);
            double cq = HUGE_VAL;
            for (int j = 0; j < nOb; j++) {
                const int v = (int)p[PH_VOB + j], r0 = (int)p[PH_ROFF + j];
                const double *m = rt + PR_PIN * j;
                const double dx = clr::cl_keep(m[0] * tau), dy = clr::cl_keep(m[1] * tau), th = clr::cl_keep(m[2] * tau), cx = m[3], cy = m[4], mg = clr::cl_keep(m[5] * tau);
                const bool tr = th != 0.0, ta = tr || dx != 0.0 || dy != 0.0 || mg != 0.0;
                double rs = 0.0, rc = 1.0;
                if (tr) { rs = sin(th); rc = cos(th); }
                double a1[VM], a2[VM], bj[VM], wb = 0.0;
#pragma unroll
                for (int i = 0; i < VM; i++) {
                    const bool on = i < v;
                    const double o1 = on ? p[PH_A + 2 * (r0 + i)] : 0.0, o2 = on ? p[PH_A + 2 * (r0 + i) + 1] : 0.0, b0 = on ? p[PH_B + r0 + i] : 0.0;
                    double n1 = o1, n2 = o2, nb = b0;
                    if (on && tr) { n1 = rc * o1 - rs * o2; n2 = rs * o1 + rc * o2; }
                    if (on && ta) nb = ((b0 + (n1 * (cx + dx) + n2 * (cy + dy))) - (o1 * cx + o2 * cy)) + mg;
                    a1[i] = n1; a2[i] = n2; bj[i] = nb;
                    wb = val::vmax(wb, val::vmax(val::vbad(n1), val::vmax(val::vbad(n2), val::vbad(nb))));
                }
                double lam[VM], mu[4], d;
                dualws_one<VM>(v, a1, a2, bj, g, x[0] + cs * off, x[1] + sn * off, cs, sn, lam, mu, &d);
                const double c = d < CL_TOUCH ? 0.0 : d;
                clr::acc_take(a, c, q, j, s == 0);
                a[clr::CA_BAD] = val::vmax(a[clr::CA_BAD], wb);
                if (c < need) { const double key = (double)(q * CL_NPO + j); hit[q] = 1; f = key < f ? key : f; }
                cq = clr::cl_min(cq, c);
            }
            if (prof) prof[q] = cq;
        }
#pragma unroll
        for (int i = 0; i < clr::CA_N; i++) acc[i][LI(lane)] = (i == clr::CA_KEY || i == clr::CA_BAD) ? a[i] : -a[i];
        fk[LI(lane)] = f;
    }
    SYNC();
    write_all(N, S, nOb, acc, hit, fk, mv, cum, ts, 1, t1, Ts, rev, out, prof);
}

// p: quadcopter problem header (QPH_*: Ts, R, the boxes as [hi; -lo], read only); x: 12 x (N + 1) stage-contiguous; ts[k * tstride] is timeScale[k] (tstride 0: one t);
// rt: PR_QIN doubles per box; out: PR_OUT doubles; prof: N S + 1 doubles or nullptr.  Needs 1 <= N <= QNMAX.
OBCA_FN void predict_quad_instance(int N, const double *p, const double *x, const double *ts, int tstride, const double *rt, int S, double need, int rev, double *out, double *prof) {
    CL_LDS unsigned char hit[CL_MAXSAMPLES];
    CL_LDS double cum[OB_NMAX + 1];
    const double Ts = p[QPH_TS], R = p[QPH_R];
    const int nS = N * S + 1, rounds = (nS + QNT - 1) / QNT;
    double acc[clr::CA_N][OBCA_NL], fk[OBCA_NL], mv[OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vbad(Ts) : 0.0;
        for (int i = lane; i < QX * (N + 1); i += QNT) b = val::vmax(b, val::vbad(x[i]));
        for (int i = lane; i < N + 1; i += QNT) b = val::vmax(b, val::vbad(ts[(size_t)i * tstride]));
        for (int i = lane; i < PR_QIN * QOB; i += QNT) b = val::vmax(b, val::vbad(rt[i]));
        double m = 0.0;
        for (int j = lane; j < QOB; j += QNT) { const double *r = rt + PR_QIN * j; if (r[0] != 0.0 || r[1] != 0.0 || r[2] != 0.0 || r[3] != 0.0) m += 1.0; }
        acc[clr::CA_BAD][LI(lane)] = b; mv[LI(lane)] = m;
        for (int q = lane; q < nS; q += QNT) hit[q] = 0;
        if (lane == 0) pr_fill_cum(cum, N, ts, tstride, 0.0);
    }
    if (wred_max(acc[clr::CA_BAD]) != 0.0) { clr::write_bad(nS, out); write_bad_tail(nS, rev, out, prof); return; }
    SYNC();
    PAR(lane) {
        double a[clr::CA_N], f = HUGE_VAL;
        clr::acc_init(a);
        for (int r = 0; r < rounds; r++) {
            const int q = clr::cl_item(r, rounds, lane, rev);
            if (q >= nS) continue;
            const int k = q / S, s = q - k * S;
            const double tsk = s ? ts[(size_t)k * tstride] : 0.0;
            const double step = (double)s / (double)S * tsk * Ts, tau = pr_tau(cum, k, s, S, tsk, Ts);
            double pt[3];
#pragma unroll
            for (int i = 0; i < 3; i++) pt[i] = s ? x[QX * k + i] + clr::cl_keep(step * x[QX * k + 6 + i]) : x[QX * k + i];
            double cq = HUGE_VAL;
            for (int j = 0; j < QOB; j++) {
                const double *ob = p + QPH_OB + QL * j, *m = rt + PR_QIN * j;
                const double mg = clr::cl_keep(m[3] * tau);
                double d2 = 0.0, wb = 0.0;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const double dd = clr::cl_keep(m[i] * tau);
                    const bool ta = dd != 0.0 || mg != 0.0;
                    const double hiw = ta ? (ob[i] + dd) + mg : ob[i], low = ta ? (ob[3 + i] - dd) + mg : ob[3 + i];
                    wb = val::vmax(wb, val::vmax(val::vbad(hiw), val::vbad(low)));
                    const double lo = -low - pt[i], hi = pt[i] - hiw;
                    const double far = lo > hi ? lo : hi, e = far > 0.0 ? far : 0.0;      // (a box that g < 0 has turned inside out: the larger of the two, as numpy's maximum)
                    d2 = d2 + clr::cl_keep(e * e);
                }
                const double c = sqrt(d2) - R;
                clr::acc_take(a, c, q, j, s == 0);
                a[clr::CA_BAD] = val::vmax(a[clr::CA_BAD], wb);
                if (c < need) { const double key = (double)(q * CL_NPO + j); hit[q] = 1; f = key < f ? key : f; }
                cq = clr::cl_min(cq, c);
            }
            if (prof) prof[q] = cq;
        }
#pragma unroll
        for (int i = 0; i < clr::CA_N; i++) acc[i][LI(lane)] = (i == clr::CA_KEY || i == clr::CA_BAD) ? a[i] : -a[i];
        fk[LI(lane)] = f;
    }
    SYNC();
    write_all(N, S, QOB, acc, hit, fk, mv, cum, ts, tstride, 0.0, Ts, rev, out, prof);
}

}  // namespace prd
}  // namespace obca
