// obca_scene_edit.h -- the obstacles of a resident batch moved and inflated in place, on the device: one wavefront (64 lanes) per instance, one launch.  Everything
// downstream -- both interior-point kernels, DualMultWS, validate, clearance, certify, rollout, track, ensemble, advance, refine, the planners' packing -- reads the obstacle
// set from the instance's problem record (PH_A, PH_B / QPH_OB), so editing those words is the whole change of scene: no other kernel knows about it, and the start iterate,
// the last solution, its multipliers, the plant state and the advance log stay as they are.  obca_amd/validate.py (move_obstacles_parking, move_obstacles_quad) is the numpy
// statement: the same operations in the same order.
// Parking.  Obstacle j = {p : A p <= b} (unit-length rows, as the upload left them) becomes its image under p' = R(dth)(p - c) + c + d and then grows by m.  Row by row:
//   a' = R(dth) a            (dth == 0: the rotation is skipped and the two words of `a` are not stored)
//   b' = ((b + a'.(c + d)) - a.c) + m      with a'.(c + d) = a1' (cx + dx) + a2' (cy + dy) and a.c = a1 cx + a2 cy, evaluated in this order
// The rows stay unit length (a rotation; a few ulp of drift per turn, nothing renormalises).  An obstacle whose motion and inflation are all zero keeps every bit.
//   in : 6 doubles per obstacle j of the instance, [dx, dy, dth, cx, cy, m] at in[6 j]
// Quadcopter.  Box j is [ub(3), -lb(3)] at QPH_OB + 6 j: word i < 3 becomes (ob[i] + d_i) + m, word 3 + i becomes (ob[3 + i] - d_i) + m; R is not touched.
//   in : 4 doubles per box j, [dx, dy, dz, m] at in[4 j]
// The lanes are dealt the rows (parking: M <= OB_MMAX = 64, one round; quadcopter: the 30 words); a lane finds its row's obstacle from PH_ROFF.  The lanes below nOb each
// take ONE obstacle's parameters, check them and make its one sin and one cos; the row lanes fetch them from that lane (a lane exchange, no LDS).
// ORDER: all or nothing per instance.  (1) every lane computes its new words into registers, (2) ONE wave reduction over "a parameter or a result is not finite",
// (3) only then the words are stored.  An instance with a non-finite parameter or result keeps every bit of its record and reports status 1, the others 0.  Every word has
// one writer, the lane of its row, and that lane alone has read it: no synchronisation is needed beyond the reduction.  Row counts, offsets, the formulation flag and every
// other header word are never written.
// `rev` deals rows and obstacles to the lanes backwards: the host build's test asks for the same bits.
// The same text compiles for the host (-DOBCA_EMU) for tests/emu/scene_edit_emu.cpp.  Nothing here is used by the solve kernels, and no existing device function changes.
#pragma once
#ifndef PV_OUT
#error "include the validate kernel text (namespace val: vbad, vmax; behind it both solvers' records and the wave reductions) before this header"
#endif

namespace obca {
namespace sed {

#define SE_PIN 6             // doubles per parking obstacle: dx, dy, dth, cx, cy, m
#define SE_QIN 4             // doubles per box: dx, dy, dz, m
static_assert(OB_MMAX <= OB_NT && OB_NOBMAX <= OB_NT && QOB * QL <= QNT, "one round: a lane per row / per word, a lane per obstacle");

// the value lane `src` holds of a per-lane variable (all 64 lanes take part)
#ifdef OBCA_EMU
#define SE_FROM_LANE(x, src) ((x)[src])
#else
#define SE_FROM_LANE(x, src) __shfl((x)[0], (src), 64)
#endif

// prob: the instance's problem record (PH_* header; only PH_A and PH_B words are written); in: SE_PIN doubles per obstacle; status: 1 double, 0 moved / 1 left as it was
OBCA_FN void move_parking_instance(double *prob, const double *in, int rev, double *status) {
    const double *p = prob;
    const int nOb = (int)p[PH_NOB], M = (int)p[PH_M];
    double sn[OBCA_NL], cs[OBCA_NL], bad[OBCA_NL];
    PAR(lane) {      // one obstacle per lane: its parameters checked, its sine and cosine
        const int j = rev ? OB_NT - 1 - lane : lane;
        double s = 0.0, c = 1.0, b = 0.0;
        if (j < nOb) {
#pragma unroll
            for (int i = 0; i < SE_PIN; i++) b = val::vmax(b, val::vbad(in[SE_PIN * j + i]));
            const double th = in[SE_PIN * j + 2];
            if (th != 0.0) { s = sin(th); c = cos(th); }
        }
        sn[LI(lane)] = s; cs[LI(lane)] = c; bad[LI(lane)] = b;
    }
    double na1[OBCA_NL], na2[OBCA_NL], nb[OBCA_NL];
    int rot[OBCA_NL], any[OBCA_NL];
    PAR(lane) {      // one row per lane: the new words into registers
        const int r = rev ? OB_NT - 1 - lane : lane;
        const bool on = r < M;
        int j = 0;
        for (int q = 1; q < nOb; q++) if (on && r >= (int)p[PH_ROFF + q]) j = q;
        const int src = rev ? OB_NT - 1 - j : j;
        const double s = SE_FROM_LANE(sn, src), c = SE_FROM_LANE(cs, src);
        double a1 = 0.0, a2 = 0.0, b = 0.0, b0 = 0.0;
        int tr = 0, ta = 0;
        if (on) {
            const double *m = in + SE_PIN * j;
            const double dx = m[0], dy = m[1], th = m[2], cx = m[3], cy = m[4], mg = m[5];
            const double o1 = p[PH_A + 2 * r], o2 = p[PH_A + 2 * r + 1];
            a1 = o1; a2 = o2; b = b0 = p[PH_B + r];
            tr = th != 0.0; ta = tr || dx != 0.0 || dy != 0.0 || mg != 0.0;
            if (tr) { a1 = c * o1 - s * o2; a2 = s * o1 + c * o2; }
            if (ta) b = ((b0 + (a1 * (cx + dx) + a2 * (cy + dy))) - (o1 * cx + o2 * cy)) + mg;
        }
        na1[LI(lane)] = a1; na2[LI(lane)] = a2; nb[LI(lane)] = b; rot[LI(lane)] = tr; any[LI(lane)] = ta;
        bad[LI(lane)] = val::vmax(bad[LI(lane)], val::vmax(val::vbad(a1), val::vmax(val::vbad(a2), val::vbad(b))));
    }
    const double isbad = wred_max(bad);
    PAR(lane) {      // ORDER: nothing has been stored before the reduction above
        const int r = rev ? OB_NT - 1 - lane : lane;
        if (isbad == 0.0 && r < M) {
            if (rot[LI(lane)]) { prob[PH_A + 2 * r] = na1[LI(lane)]; prob[PH_A + 2 * r + 1] = na2[LI(lane)]; }
            if (any[LI(lane)]) prob[PH_B + r] = nb[LI(lane)];
        }
        if (r == 0) status[0] = isbad != 0.0 ? 1.0 : 0.0;
    }
}

// prob: the instance's quadcopter record (only the QOB * QL words at QPH_OB are written); in: SE_QIN doubles per box; status: 1 double
OBCA_FN void move_quad_instance(double *prob, const double *in, int rev, double *status) {
    const double *p = prob;
    double nw[OBCA_NL], bad[OBCA_NL];
    int any[OBCA_NL];
    PAR(lane) {
        const int w = rev ? QNT - 1 - lane : lane;
        double v = 0.0, b = 0.0;
        int ta = 0;
        if (w < QOB * SE_QIN) b = val::vbad(in[w]);
        if (w < QOB * QL) {
            const int j = w / QL, i = w - QL * j;
            const double d = in[SE_QIN * j + (i < 3 ? i : i - 3)], mg = in[SE_QIN * j + 3], o = p[QPH_OB + w];
            ta = d != 0.0 || mg != 0.0;
            v = ta ? (i < 3 ? o + d : o - d) + mg : o;
            b = val::vmax(b, val::vbad(v));
        }
        nw[LI(lane)] = v; any[LI(lane)] = ta; bad[LI(lane)] = b;
    }
    const double isbad = wred_max(bad);
    PAR(lane) {      // ORDER: nothing has been stored before the reduction above
        const int w = rev ? QNT - 1 - lane : lane;
        if (isbad == 0.0 && w < QOB * QL && any[LI(lane)]) prob[QPH_OB + w] = nw[LI(lane)];
        if (w == 0) status[0] = isbad != 0.0 ? 1.0 : 0.0;
    }
}

}  // namespace sed
}  // namespace obca
