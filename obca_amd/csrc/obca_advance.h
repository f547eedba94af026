// obca_advance.h -- one step of the closed receding-horizon loop, on the device: the PLANT is advanced over the first `shift` intervals of the last solution and the next
// solve is restarted from the state it reached.  solve(), rollout() and shift_warm_start() each do a part; here they run together, one wavefront (64 lanes) per instance,
// one launch, and nothing but the record of the step (AV_OUT doubles) travels.  obca_amd/validate.py (advance_parking, advance_quad, advance_record) is the numpy statement.
// Phases of an instance:
//   1. scan    : a non-finite number among what is read -- Ts, the time scale, X0 of the record, the solution's nodes 0 .. shift and inputs 0 .. shift - 1, the kick
//   2. plant   : roll::integrate in chain mode with a horizon of `shift` (not N) from the RECORD's X0 (the plant's state: what the last advance, or the upload, left there --
//                not the solution's node 0): u_k held over interval k of length t_k Ts, S classical RK4 steps, the rollout's pole test and non-finite handling; ONE lane
//                integrates (a recurrence in time).  It leaves the shift S + 1 sample poses and the node states X_0 .. X_shift in the instance's slices of the work buffer
//   3. kick    : the plant state is X_shift + kick (the process disturbance; no kick: X_shift itself) -- nx doubles per instance that stay on the device (`st`).  It is both
//                the plant's state and the measurement the restart is given
//   4. measure : the driven samples (before the kick) dealt over the lanes as (sample, obstacle) items, their clearance as roll::rollout_*_instance computes it: dualws_one
//                of the pose with the CL_TOUCH clamp / distance of the point to each box - R; clr::acc_take, clr::write_record and the `hit` marks unchanged
//   5. record  : roll::write_head with the horizon `shift`: the deviations of X_k (before the kick: the model mismatch) from the solution's own nodes k = 1 .. shift and at
//                node shift; then the fields of the step.  shift 0: the plant stands, the maxima are 0, the node -1, and "at node shift" is X0 against the solution's node 0
//   6. log     : with a log, the nodes X_1 .. X_shift (the last one after the kick) are appended to the instance's rows
//   7. restart : shf::shift_instance / quad::quad_shift_instance, unchanged, with x0_new = `st` read where phase 3 left it in device memory: every policy of the shift calls
//                holds (parking does not consult the exit flag, a failed quadcopter instance keeps its uploaded start, the tails are padded as those headers describe)
// ORDER: phases 1-6 read the problem record (Ts, X0, XF, the obstacles) and the solution z; phase 7 overwrites words of the record (X0, the reference / the warm start) and,
// for parking, moves reference words in place (the hazard documented in obca_shift.h stays as it is there, with the direction buffer as scratch).  So the wavefront
// synchronises between phase 6 and phase 7: every read of prob and z by the plant and the measurement, and every store to `st`, is complete before the first word of the
// rewrite.  Nothing of phases 1-6 writes into prob, z or z0.
// Record (AV_OUT = RO_OUT doubles): the rollout's head and clearance layout; [10] 0 (chain), [11] S, [12] shift, [13] the driven time sum t_k Ts, [14] the position distance of
// the plant state (after the kick) to the goal the next solve has (XF of the record, xF_new where given), [15] the nodes logged so far including this step's, -1 without a log.
// bad = 1 marks ONE instance: a non-finite number in phase 1, a rolled state that is not finite or a quadcopter step across cos x[3] = 0, a kicked state or a clearance that is
// not finite.  Its record is filled as the rollout fills a bad one (real fields NaN, indices -1; [13], [14] NaN, [12], [15] as above), `st` is NaN, and NOTHING else of it is
// written: problem record, start iterate and log rows keep their bits (phases 6 and 7 do not run).
// A parking instance without obstacles has nothing to measure: min and min_nodes +inf, sample and obstacle -1, below 0.
// No feedback acts inside the step: in this loop the re-solve IS the feedback; obca_track.h is the tool between two re-solves.
// The same text compiles for the host (-DOBCA_EMU) for tests/emu/advance_emu.cpp.  Nothing here is used by the solve kernels, and no existing device function changes.
#pragma once
#ifndef RO_OUT
#error "include the rollout's kernel text (namespace roll, behind the clearance check's) before this header: its integrator, models and record are reused unchanged"
#endif
#ifndef SH_DEAL
#error "include the two shift texts (obca_shift.h, obca_quad_shift.h) before this header: the restart runs through their device functions unchanged"
#endif

namespace obca {
namespace adv {
using namespace roll;

#define AV_OUT 40            // doubles per instance (= OBCA_ADV_OUT of include/obca_advance.h)
enum { AV_SHIFT = 12, AV_TIME, AV_GOAL, AV_LOGGED };
static_assert(AV_OUT == RO_OUT && AV_LOGGED < RO_CLR, "the record is the rollout's, with the four reserved fields of the head in use");

// the refusals of the entry points, one text for the library and the host build
static inline const char *advance_check_args(int N, int shift, int substeps, double need) {
    if (shift < 0 || shift > N) return "shift out of range 0..N";
    if (substeps < 1 || substeps > CL_SMAX) return "need 1 <= substeps <= 32";
    if (!(need - need == 0.0)) return "need a finite `need`";
    return nullptr;
}
// doubles of one instance in the two regions of the work buffer: the sample poses, the node states -- of `shift` intervals
OBCA_HD size_t advance_pose_len(int shift, int S) { return rollout_pose_len(shift, S); }
OBCA_HD size_t advance_state_len(int shift, int nx) { return rollout_state_len(shift, nx); }

// the record and the plant state of an instance that is not finite
OBCA_FN void advance_bad(int shift, int nx, int S, double logged, double *Xn, double *st, double *out) {
    write_all_bad(shift, nx, S, 0, Xn, out);
    PAR(lane) {
        if (lane < nx) st[lane] = __builtin_nan("");
        if (lane == 0) { out[AV_SHIFT] = (double)shift; out[AV_TIME] = out[AV_GOAL] = __builtin_nan(""); out[AV_LOGGED] = logged; }
    }
}
// Phase 3: st <- X_shift + kick; bad: the sum is not finite
template <class M>
OBCA_FN void kick_state(int shift, const double *Xn, const double *kick, double *st, double (&bad)[OBCA_NL]) {
    PAR(lane) {
        double b = 0.0;
        if (lane < M::NX) {
            const double v = kick ? Xn[M::NX * shift + lane] + kick[lane] : Xn[M::NX * shift + lane];
            st[lane] = v; b = val::vbad(v);
        }
        bad[LI(lane)] = b;
    }
}
// Phases 5 (the fields of the step; write_head has run) and 6.  hsum: the driven time; xF: the goal's state (positions first, npos of them); log: this step's rows or nullptr
template <class M>
OBCA_FN void step_fields(int shift, int npos, double hsum, const double *xF, const double *Xn, const double *st, double logged, double *log, int rev, double *out) {
    SYNC();      // `st` of phase 3 is read by other lanes than wrote it
    PAR(lane) {
        if (lane == 0) {
            double d2 = 0.0;
            for (int i = 0; i < npos; i++) { const double e = st[i] - xF[i]; d2 = d2 + clr::cl_keep(e * e); }
            if (shift == 0) out[RO_DNODE] = -1.0;      // (no node 1 .. shift: write_head found none)
            out[AV_SHIFT] = (double)shift; out[AV_TIME] = hsum; out[AV_GOAL] = sqrt(d2); out[AV_LOGGED] = logged;
        }
        if (log) {
            SH_DEAL(i, M::NX * shift, lane, rev) { const int k = i / M::NX + 1, c = i - (k - 1) * M::NX; log[i] = k == shift ? st[c] : Xn[M::NX * k + c]; }
        }
    }
}

// prob: problem record (header | rx | ry | ryaw), read, then rewritten by the restart; z: the last solution in the solver's layout; z0: start iterate of the next solve; tmp:
// 3 (N + 1) doubles of scratch (the direction buffer); kick: 4 doubles or nullptr; pose / Xn: this instance's slices of the work buffer (advance_pose_len, advance_state_len);
// st: 4 doubles, the plant state; log: where this step's 4 x shift doubles go, or nullptr; logged: field [15]; out: AV_OUT doubles.  VM: the row class of the batch's widest
// obstacle.  Needs 1 <= N <= OB_NMAX, 0 <= shift <= N, 1 <= S <= CL_SMAX.
template <int VM>
OBCA_FN void advance_parking_instance(int N, int shift, double *prob, const double *z, double *z0, double *tmp, int S, const double *kick, double need, int rev,
                                      double *pose, double *Xn, double *st, double *log, double logged, double *out) {
    CL_LDS unsigned char hit[CL_MAXSAMPLES];
    const double *p = prob;
    const int nOb = (int)p[PH_NOB], M = (int)p[PH_M];
    Lay l; make_layout(N, nOb, M, l);
    const double Ts = p[PH_TS], off = p[PH_OFF];
    const double t1 = p[PH_FIX] != 0.0 ? 1.0 : z[l.t];
    const int nS = shift * S + 1, nIt = nS * nOb, rounds = (nIt + OB_NT - 1) / OB_NT;
    double acc[CA_N][OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vmax(val::vbad(Ts), val::vbad(t1)) : 0.0;
        if (lane < 4) b = val::vmax(b, val::vmax(val::vbad(p[PH_X0 + lane]), kick ? val::vbad(kick[lane]) : 0.0));
        for (int i = lane; i < 4 * (shift + 1); i += OB_NT) b = val::vmax(b, val::vbad(z[l.x + i]));
        for (int i = lane; i < 2 * shift; i += OB_NT) b = val::vmax(b, val::vbad(z[l.u + i]));
        acc[CA_BAD][LI(lane)] = b;
        for (int q = lane; q < nS; q += OB_NT) hit[q] = 0;
    }
    if (wred_max(acc[CA_BAD]) != 0.0) { advance_bad(shift, 4, S, logged, Xn, st, out); return; }
    integrate<ParkModel>(p[PH_L], shift, S, 0, p + PH_X0, z + l.u, [&](int) { return t1 * Ts; }, pose, Xn, acc[CA_BAD]);      // (chain mode reads the start only: the record's X0)
    if (wred_max(acc[CA_BAD]) != 0.0) { advance_bad(shift, 4, S, logged, Xn, st, out); return; }
    SYNC();
    kick_state<ParkModel>(shift, Xn, kick, st, acc[CA_BAD]);
    if (wred_max(acc[CA_BAD]) != 0.0) { advance_bad(shift, 4, S, logged, Xn, st, out); return; }
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
    if (wred_max(acc[CA_BAD]) != 0.0) { advance_bad(shift, 4, S, logged, Xn, st, out); return; }
    if (nOb > 0) clr::write_record(nS, nOb, acc, hit, out + RO_CLR);
    else {      // nothing to measure
        PAR(lane) {
            if (lane == 0) {
                double *o = out + RO_CLR;
                o[CL_MIN] = o[CL_MINNODES] = HUGE_VAL; o[CL_SAMPLE] = o[CL_OBST] = -1.0; o[CL_BELOW] = 0.0; o[CL_SAMPLES] = (double)nS; o[CL_BAD] = 0.0; o[CL_RSV] = 0.0;
                for (int i = 0; i < CL_NPO; i++) o[CL_PER + i] = HUGE_VAL;
            }
        }
    }
    write_head<ParkModel>(shift, S, 0, z + l.x, Xn, out);
    step_fields<ParkModel>(shift, 2, (double)shift * (t1 * Ts), p + PH_XF, Xn, st, logged, log, rev, out);
    SYNC();      // ORDER (see the head of this file): every read of prob and z above, and `st`, before the rewrite below
    shf::shift_instance(N, shift, prob, z, z0, tmp, st, rev);
}

// prob: quadcopter problem record (QPH_* header, then xWS), read, then rewritten by the restart; z: the last solution in the solver's layout (x, u and its one t are
// read); info: the 8 doubles of the last solve; kick / xF_new: 12 doubles each or nullptr; the rest as advance_parking_instance.  Needs 1 <= N <= QNMAX, 0 <= shift <= N.
OBCA_FN void advance_quad_instance(int N, int shift, double *prob, const double *z, const double *info, int S, const double *kick, const double *xF_new, double need, int rev,
                                   double *pose, double *Xn, double *st, double *log, double logged, double *out) {
    CL_LDS unsigned char hit[CL_MAXSAMPLES];
    const double *p = prob;
    quad::QLay l; quad::q_make_layout(N, l);
    const double *x = z + l.x, *u = z + l.u;
    const double Ts = p[QPH_TS], R = p[QPH_R], t1 = z[l.t];
    const int nS = shift * S + 1, nIt = nS * QOB, rounds = (nIt + QNT - 1) / QNT;
    double acc[CA_N][OBCA_NL];
    PAR(lane) {
        double b = lane == 0 ? val::vmax(val::vbad(Ts), val::vbad(t1)) : 0.0;
        if (lane < QX) b = val::vmax(b, val::vmax(val::vbad(p[QPH_X0 + lane]), kick ? val::vbad(kick[lane]) : 0.0));
        for (int i = lane; i < QX * (shift + 1); i += QNT) b = val::vmax(b, val::vbad(x[i]));
        for (int i = lane; i < QU * shift; i += QNT) b = val::vmax(b, val::vbad(u[i]));
        acc[CA_BAD][LI(lane)] = b;
        for (int q = lane; q < nS; q += QNT) hit[q] = 0;
    }
    if (wred_max(acc[CA_BAD]) != 0.0) { advance_bad(shift, QX, S, logged, Xn, st, out); return; }
    integrate<QuadModel>(0.0, shift, S, 0, p + QPH_X0, u, [&](int) { return t1 * Ts; }, pose, Xn, acc[CA_BAD]);      // (chain mode reads the start only: the record's X0)
    if (wred_max(acc[CA_BAD]) != 0.0) { advance_bad(shift, QX, S, logged, Xn, st, out); return; }
    SYNC();
    kick_state<QuadModel>(shift, Xn, kick, st, acc[CA_BAD]);
    if (wred_max(acc[CA_BAD]) != 0.0) { advance_bad(shift, QX, S, logged, Xn, st, out); return; }
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
    if (wred_max(acc[CA_BAD]) != 0.0) { advance_bad(shift, QX, S, logged, Xn, st, out); return; }
    clr::write_record(nS, QOB, acc, hit, out + RO_CLR);
    write_head<QuadModel>(shift, S, 0, x, Xn, out);
    step_fields<QuadModel>(shift, 3, (double)shift * (t1 * Ts), xF_new ? xF_new : p + QPH_XF, Xn, st, logged, log, rev, out);
    SYNC();      // ORDER (see the head of this file): every read of prob and z above, and `st`, before the rewrite below
    quad::quad_shift_instance(N, shift, prob, z, info, st, xF_new);
}

}  // namespace adv
}  // namespace obca
