// obca_clearance.h -- clearance of a trajectory BETWEEN its nodes, on the device: both NLPs hold the obstacle separation at the N + 1 nodes only, and validate() looks at the
// same rows at the same nodes.  Here every interval is sampled S times with the discretisation's own partial step and the distance of every sample to every obstacle is
// computed from scratch -- no multiplier of the solve is trusted.  One wavefront (64 lanes) per instance; obca_amd/validate.py (parking_samples, quad_clearance) is the numpy statement.
//   samples  : q = k S + s, k = 0 .. N-1, s = 0 .. S-1, and q = N S (node N): N S + 1 of them; the node samples are those with s = 0 and the last one
//   parking  : pose of (k, s) = val::park_step from node k with u_k over the step length (s / S) ts_k Ts (ParkingSignedDist.jl:147-150), the node itself, bit for bit, where s is 0;
//              d = dualws_one<VM> of that pose against obstacle j (unit rows, the centre offset of obca_dualws_kernel); c = 0 if d < CL_TOUCH, else d ("touches or overlaps")
//   quadcopter: p_k + tau v_k (QuadcopterSignedDist.jl:138-140), c = Euclidean distance of the point to box j (0 inside) - R
// Lanes take (sample, obstacle) items, item = q nOb + j.  The minimum carries (c, q, j) and ties go to the smallest q, then the smallest j: a lane keeps the
// lexicographically smallest of its items, the wave reduces the value, then the key q * CL_NPO + j among the lanes that hold that value -- the record does not depend on how
// the items are dealt (`rev` deals them backwards; the host build's test asks for the same bits).  `below` counts samples, not items: an item below `need` marks its sample in
// LDS (every writer stores the same 1), the marks are summed after the items.
// Record (CL_OUT doubles): min, min_nodes, sample, obstacle, below, samples, bad, 0, then the smallest c per obstacle (+inf behind the instance's obstacles).
// bad = 1: a non-finite number among what is read (parking: Ts, every x, u and timeScale of the trajectory; quadcopter: Ts, every x and timeScale) or among the c computed
// from them; then min, min_nodes and the per-obstacle entries are NaN, sample and obstacle -1, below = samples.  Nothing but the finite scan runs on such an instance.
// Transcendentals are libm's / the device library's sin, cos, tan, sqrt, as in obca_validate.h.  No product is contracted into a following sum where host build and device are
// expected to agree to the bit (the quadcopter path: cl_keep() puts the solver's SEAM between them); the parking distance is an iteration and agrees to 1e-9.
// The same text compiles for the host (-DOBCA_EMU) for tests/emu/clearance_emu.cpp.  Nothing here is used by the solve kernels.
#pragma once
#include "obca_validate.h"

namespace obca {
namespace clr {

static_assert(OB_NT == 64 && QNT == 64, "one wavefront per instance: the wave reductions run over 64 lanes");

#define CL_OUT 24            // doubles per instance (= OBCA_CLR_OUT of include/obca_clearance.h)
#define CL_SMAX 32           // most sub-steps per interval
#define CL_NPO 16            // per-obstacle entries of the record
#define CL_TOUCH 1e-7        // the path-following of dualws_one ends at a complementarity of 1e-9: a touching or overlapping pose returns noise of that size
#define CL_MAXSAMPLES (OB_NMAX * CL_SMAX + 1)
enum { CL_MIN = 0, CL_MINNODES, CL_SAMPLE, CL_OBST, CL_BELOW, CL_SAMPLES, CL_BAD, CL_RSV, CL_PER };
enum { CA_BEST = 0, CA_KEY, CA_NODES, CA_BAD, CA_PER, CA_N = CA_PER + CL_NPO };      // per-lane accumulators
static_assert(OB_NOBMAX <= CL_NPO && QOB <= CL_NPO && CL_PER + CL_NPO == CL_OUT && QNMAX <= OB_NMAX, "the record holds every obstacle, the marks every sample");
#ifdef OBCA_EMU
#define CL_LDS
#else
#define CL_LDS __shared__
#endif

OBCA_FN double cl_keep(double x) { SEAM(x); return x; }                                  // a product that must not fuse with the sum it enters
OBCA_FN double cl_min(double a, double b) { return (b < a || b != b) ? b : a; }          // NaN-propagating, like np.min

// the refusals of the entry points, one text for the library and the host build
static inline const char *clearance_check_args(int substeps, double need) {
    if (substeps < 1 || substeps > CL_SMAX) return "need 1 <= substeps <= 32";
    if (!(need - need == 0.0)) return "need a finite `need`";
    return nullptr;
}

OBCA_FN void acc_init(double a[CA_N]) {
#pragma unroll
    for (int i = 0; i < CA_N; i++) a[i] = HUGE_VAL;
    a[CA_BAD] = 0.0;
}
// clearance c of item (q, j); node: a node sample
OBCA_FN void acc_take(double a[CA_N], double c, int q, int j, bool node) {
    const double key = (double)(q * CL_NPO + j);
    if (c < a[CA_BEST] || (c == a[CA_BEST] && key < a[CA_KEY])) { a[CA_BEST] = c; a[CA_KEY] = key; }
    if (node) a[CA_NODES] = cl_min(a[CA_NODES], c);
    a[CA_BAD] = val::vmax(a[CA_BAD], val::vbad(c));
#pragma unroll
    for (int i = 0; i < CL_NPO; i++) a[CA_PER + i] = i == j ? cl_min(a[CA_PER + i], c) : a[CA_PER + i];      // (no indexed register array)
}
// item of lane `lane` in round r of `rounds`: ascending, or (rev) dealt backwards -- lanes and rounds
OBCA_FN int cl_item(int r, int rounds, int lane, int rev) { return rev ? (rounds - 1 - r) * OB_NT + (OB_NT - 1 - lane) : r * OB_NT + lane; }

OBCA_FN void write_bad(int nS, double *out) {
    PAR(lane) {
        if (lane == 0) {
            const double nan_ = __builtin_nan("");
            out[CL_MIN] = out[CL_MINNODES] = nan_; out[CL_SAMPLE] = out[CL_OBST] = -1.0; out[CL_BELOW] = out[CL_SAMPLES] = (double)nS; out[CL_BAD] = 1.0; out[CL_RSV] = 0.0;
            for (int i = 0; i < CL_NPO; i++) out[CL_PER + i] = nan_;
        }
    }
}
// acc: the lanes' accumulators, the minima NEGATED (the wave's NaN-propagating reduction is a maximum); hit: the marks of the samples below `need`
OBCA_FN void write_record(int nS, int nOb, double (&acc)[CA_N][OBCA_NL], const unsigned char *hit, double *out) {
    if (wred_max(acc[CA_BAD]) != 0.0) { write_bad(nS, out); return; }
    const double m = -wred_max(acc[CA_BEST]), mn = -wred_max(acc[CA_NODES]);
    double kk[OBCA_NL], cnt[OBCA_NL];
    PAR(lane) {
        kk[LI(lane)] = (-acc[CA_BEST][LI(lane)] == m) ? acc[CA_KEY][LI(lane)] : HUGE_VAL;
        double c = 0.0;
        for (int q = lane; q < nS; q += OB_NT) c += (double)hit[q];
        cnt[LI(lane)] = c;
    }
    const double key = wred_min(kk), below = wred_sum(cnt);      // (integers below 2^53: the sum is exact in any order)
    double per[CL_NPO];
#pragma unroll
    for (int i = 0; i < CL_NPO; i++) per[i] = HUGE_VAL;
    for (int i = 0; i < nOb; i++) per[i] = -wred_max(acc[CA_PER + i]);
    PAR(lane) {
        if (lane == 0) {
            const int ik = (int)key;
            out[CL_MIN] = m; out[CL_MINNODES] = mn; out[CL_SAMPLE] = (double)(ik / CL_NPO); out[CL_OBST] = (double)(ik % CL_NPO);
            out[CL_BELOW] = below; out[CL_SAMPLES] = (double)nS; out[CL_BAD] = 0.0; out[CL_RSV] = 0.0;
            for (int i = 0; i < CL_NPO; i++) out[CL_PER + i] = per[i];
        }
    }
}

// p: problem header (PH_*: unit-length rows), z: a point in the solver's layout (x, u and t are read); ts: the caller's timeScale per stage (N + 1; nullptr: the point's
// single t, 1 with fixTime); S: sub-steps, 1 .. CL_SMAX; out: CL_OUT doubles.  VM: the row class of the batch's widest obstacle, as launch_dualws picks it.  Needs 1 <= N <= OB_NMAX.
template <int VM>
OBCA_FN void clearance_parking_instance(int N, const double *p, const double *z, const double *ts, int S, double need, int rev, double *out) {
    CL_LDS unsigned char hit[CL_MAXSAMPLES];
    const int nOb = (int)p[PH_NOB], M = (int)p[PH_M];
    Lay l; make_layout(N, nOb, M, l);
    const double Ts = p[PH_TS], L = p[PH_L], off = p[PH_OFF];
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
    if (wred_max(acc[CA_BAD]) != 0.0) { write_bad(nS, out); return; }
    SYNC();
    PAR(lane) {
        double a[CA_N], g[4];
        acc_init(a);
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = p[PH_G + i];
        for (int r = 0; r < rounds; r++) {
            const int it = cl_item(r, rounds, lane, rev);
            if (it >= nIt) continue;
            const int q = it / nOb, j = it - q * nOb, k = q / S, s = q - k * S;
            const int v = (int)p[PH_VOB + j], r0 = (int)p[PH_ROFF + j];
            double a1[VM], a2[VM], bj[VM];
#pragma unroll
            for (int i = 0; i < VM; i++) { const bool on = i < v; a1[i] = on ? p[PH_A + 2 * (r0 + i)] : 0.0; a2[i] = on ? p[PH_A + 2 * (r0 + i) + 1] : 0.0; bj[i] = on ? p[PH_B + r0 + i] : 0.0; }
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; i++) x[i] = z[l.x + 4 * k + i];
            if (s) {      // (k < N here: the last sample has s = 0)
                const double u[2] = {z[l.u + 2 * k], z[l.u + 2 * k + 1]};
                double F[4];
                val::park_step(Ts, L, x, u, (double)s / (double)S * (ts ? ts[k] : t1), F);
#pragma unroll
                for (int i = 0; i < 4; i++) x[i] = F[i];
            }
            const double sn = sin(x[2]), cs = cos(x[2]);
            double lam[VM], mu[4], d;
            dualws_one<VM>(v, a1, a2, bj, g, x[0] + cs * off, x[1] + sn * off, cs, sn, lam, mu, &d);
            const double c = d < CL_TOUCH ? 0.0 : d;
            acc_take(a, c, q, j, s == 0);
            if (c < need) hit[q] = 1;
        }
#pragma unroll
        for (int i = 0; i < CA_N; i++) acc[i][LI(lane)] = (i == CA_KEY || i == CA_BAD) ? a[i] : -a[i];
    }
    SYNC();
    write_record(nS, nOb, acc, hit, out);
}

// p: quadcopter problem header (QPH_*: Ts, R, the boxes as [hi; -lo]); x: 12 x (N + 1) stage-contiguous (positions 0-2, velocities 6-8); ts[k * tstride] is timeScale[k]
// (tstride 0: one t); out: CL_OUT doubles, QOB per-obstacle entries.  Needs 1 <= N <= QNMAX.
OBCA_FN void clearance_quad_instance(int N, const double *p, const double *x, const double *ts, int tstride, int S, double need, int rev, double *out) {
    CL_LDS unsigned char hit[CL_MAXSAMPLES];
    const double Ts = p[QPH_TS], R = p[QPH_R];
    const int nS = N * S + 1, nIt = nS * QOB, rounds = (nIt + QNT - 1) / QNT;
    double acc[CA_N][OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vbad(Ts) : 0.0;
        for (int i = lane; i < QX * (N + 1); i += QNT) b = val::vmax(b, val::vbad(x[i]));
        for (int i = lane; i < N + 1; i += QNT) b = val::vmax(b, val::vbad(ts[i * tstride]));
        acc[CA_BAD][LI(lane)] = b;
        for (int q = lane; q < nS; q += QNT) hit[q] = 0;
    }
    if (wred_max(acc[CA_BAD]) != 0.0) { write_bad(nS, out); return; }
    SYNC();
    PAR(lane) {
        double a[CA_N];
        acc_init(a);
        for (int r = 0; r < rounds; r++) {
            const int it = cl_item(r, rounds, lane, rev);
            if (it >= nIt) continue;
            const int q = it / QOB, j = it - q * QOB, k = q / S, s = q - k * S;
            const double tau = (double)s / (double)S * ts[k * tstride] * Ts;
            const double *ob = p + QPH_OB + QL * j;
            double d2 = 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double pi = s ? x[QX * k + i] + cl_keep(tau * x[QX * k + 6 + i]) : x[QX * k + i];
                const double lo = -ob[3 + i] - pi, hi = pi - ob[i];
                const double e = lo > 0.0 ? lo : (hi > 0.0 ? hi : 0.0);
                d2 = d2 + cl_keep(e * e);
            }
            const double c = sqrt(d2) - R;
            acc_take(a, c, q, j, s == 0);
            if (c < need) hit[q] = 1;
        }
#pragma unroll
        for (int i = 0; i < CA_N; i++) acc[i][LI(lane)] = (i == CA_KEY || i == CA_BAD) ? a[i] : -a[i];
    }
    SYNC();
    write_record(nS, QOB, acc, hit, out);
}

}  // namespace clr
}  // namespace obca
