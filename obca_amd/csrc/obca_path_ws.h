// obca_path_ws.h -- the warm start of a parking solve from a planner path, on the device: what planner.path_to_warm_start (and velo_smooth behind it) computes with numpy
// per instance, one wavefront (64 lanes) per instance.  In: the nodes (x, y, yaw) and directions of a Hybrid A* path as obca_plan_hybrid_astar_batch2 writes them.  Out: Ts,
// xWS 4 x (N + 1), uWS 2 x N in the orientation the solve takes -- host arrays, or the words of a resident batch's problem record and start iterate (path_ws_record).
//   path_ws_count_status : -1 no path (count < 2), -2 more nodes than the caller's rows or than PW_MAXNODES
//   path_ws_instance     : -3 a non-finite pose, -4 the path length is not positive (and finite); else 0 and the outputs.  Nothing is written unless it returns 0.
// Arithmetic.  The two running sums -- the unwrap corrections of the yaw and the arc length -- are formed by ONE lane in node order (numpy's cumsum); everything else is per
// node or per stage and independent of the lane count.  No product is contracted into a following sum: pw_keep() puts the solver's SEAM between them, so the host build
// (tests/emu/path_ws_emu.cpp, -DOBCA_EMU: PAR is a loop over the lanes, SYNC nothing, the LDS arrays plain locals) and the device agree bit for bit on everything except
// the steering angle, whose atan is the one libm / device-library call of this text (sqrt is an instruction on both sides; floor, fmod and round are written out).
// Every output word has one writer (stage k belongs to lane k mod 64); no index leaves 0 .. nodes-1, 0 .. N, 0 .. N-1.  Nothing here is used by the solve kernels.
#pragma once
#include "obca_solver.h"

namespace obca {
namespace pw {

#define PW_MAXNODES 1024      // nodes of the longest path (= OBCA_PATH_WS_MAXNODES of include/obca_path_ws.h): two fp64 words each in LDS
#define PW_PAD 19             // veloSmooth.jl:31-41: 19 leading ...
#define PW_TAIL 21            // ... and 21 trailing zeros around the speed profile
#ifdef OBCA_EMU
#define PW_LDS
#else
#define PW_LDS __shared__
#endif

static_assert(OB_NT == 64, "one wavefront per instance: wred_max reduces over 64 lanes");

OBCA_FN double pw_keep(double x) { SEAM(x); return x; }                       // a product that must not fuse with the sum it enters
OBCA_FN double pw_bad(double v) { return (v - v == 0.0) ? 0.0 : 1.0; }         // 1 for NaN and +-inf
OBCA_FN double pw_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }
OBCA_FN double pw_clip(double v, double b) { const double lo = v > -b ? v : -b; return lo < b ? lo : b; }
OBCA_FN double pw_floor(double q) {
    if (!(q > -4.5e15 && q < 4.5e15)) return q;      // no fraction bits left (or not finite)
    const double f = (double)(long long)q;
    return f > q ? f - 1.0 : f;
}
// np.mod(a, b), b > 0: the remainder with the sign of b
OBCA_FN double pw_mod(double a, double b) {
    const double r = a - pw_keep(pw_floor(a / b) * b);
    return r < 0.0 ? r + b : r;
}
// Python's round() of q >= 0 (half to even), capped where the ramps it sizes have long left the padded profile
OBCA_FN long long pw_round_even(double q) {
    if (!(q < 1e15)) return 1000000000000000LL;
    const double f = (double)(long long)q, r = q - f;
    const long long n = (long long)f;
    return r > 0.5 ? n + 1 : (r == 0.5 ? n + (n & 1) : n);
}
// np.linspace(0, v1, acc + 1)[i] and np.linspace(-v1, v1, 2 acc + 1)[i]
OBCA_FN double pw_ramp(long long i, long long acc, double v1) { return acc == 0 ? 0.0 : (i == acc ? v1 : pw_keep((double)i * (v1 / (double)acc))); }
OBCA_FN double pw_full(long long i, long long acc, double v1) { return acc == 0 ? -v1 : (i == 2 * acc ? v1 : pw_keep((double)i * ((v1 + v1) / (double)(2 * acc))) + (-v1)); }

OBCA_HD int path_ws_count_status(int count, int cap) { return count < 2 ? -1 : ((count > cap || count > PW_MAXNODES) ? -2 : 0); }

// the refusals of the two batch calls, one text for the library and the host build (L of a resident batch lives on the device: its call passes 1)
static inline const char *path_ws_check_args(int B, int N, int cap, double v_nom, double L, double a_max, bool pointers) {
    if (B < 1) return "need B >= 1";
    if (N < 1 || N > OB_NMAX) return "need 1 <= N <= OBCA_NMAX";
    if (cap < 2) return "need cap >= 2";
    if (!(v_nom > 0) || !(v_nom - v_nom == 0.0) || !(L > 0) || !(L - L == 0.0)) return "need v_nom and L positive and finite";
    if (!(a_max >= 0) || !(a_max - a_max == 0.0)) return "need a_max >= 0 and finite";
    if (!pointers) return "NULL argument";
    return nullptr;
}

// One instance.  path: nodes x 3 (x, y, yaw), dir: nodes; xF: 4 doubles (the goal replaces the last pose, planner.py:165) or nullptr; Ts: 1, xWS: 4 x (N + 1), uWS: 2 x N.
// a_max > 0: the speed profile goes through velo_smooth.  Needs 2 <= nodes <= PW_MAXNODES, 1 <= N <= OB_NMAX, v_nom, L > 0.
OBCA_FN int path_ws_instance(int N, int nodes, const double *path, const int *dir, const double *xF, double v_nom, double L, double a_max, double *Ts, double *xWS, double *uWS) {
    PW_LDS double yw[PW_MAXNODES], cum[PW_MAXNODES];      // unwrapped yaw and running arc length of the nodes
    PW_LDS double syaw[OB_NMAX + 1], sd[OB_NMAX + 1], sv[OB_NMAX + 1], vex[OB_NMAX + 2 + PW_PAD + PW_TAIL];      // per stage: yaw, direction, speed; the padded raw profile (1-based)
    const double PI = 3.141592653589793, TWO_PI = 2.0 * PI;
    const int last = nodes - 1;
    double bad[OBCA_NL];
    PAR(lane) {
        double b = 0.0;
        for (int i = lane; i < 3 * nodes; i += OB_NT) b = b > pw_bad(path[i]) ? b : pw_bad(path[i]);
        if (xF && lane < 3) b = b > pw_bad(xF[lane]) ? b : pw_bad(xF[lane]);
        bad[LI(lane)] = b;
    }
    if (wred_max(bad) != 0.0) return -3;
    // per node: the unwrap correction (np.unwrap: ph_correct) and the length of the segment that ends in it
    PAR(lane) {
        for (int i = lane; i < nodes; i += OB_NT) {
            if (i == 0) { yw[0] = 0.0; cum[0] = 0.0; continue; }
            const double dd = path[3 * i + 2] - path[3 * i - 1];
            double m = pw_mod(dd + PI, TWO_PI) - PI;
            if (m == -PI && dd > 0.0) m = PI;
            yw[i] = fabs(dd) < PI ? 0.0 : m - dd;
            const bool g = xF && i == last;
            const double dx = (g ? xF[0] : path[3 * i]) - path[3 * i - 3], dy = (g ? xF[1] : path[3 * i + 1]) - path[3 * i - 2];
            cum[i] = sqrt(pw_keep(dx * dx) + pw_keep(dy * dy));
        }
    }
    SYNC();
    PAR(lane) {
        if (lane == 0) {      // the two running sums, in node order
            double c = 0.0, t = 0.0;
            for (int i = 1; i < nodes; i++) { c = c + yw[i]; yw[i] = c; t = t + cum[i]; cum[i] = t; }
        }
    }
    SYNC();
    PAR(lane) {
        for (int i = lane; i < nodes; i += OB_NT) yw[i] = path[3 * i + 2] + yw[i];
    }
    SYNC();
    PAR(lane) {
        if (lane == 0 && xF) yw[last] = yw[last - 1] + (pw_mod(xF[2] - yw[last - 1] + PI, TWO_PI) - PI);
    }
    SYNC();
    const double tot = cum[last];
    if (!(tot > 0.0) || !(tot - tot == 0.0)) return -4;
    const double step = tot / (double)N, Tsv = tot / ((double)N * v_nom);
    // per stage: the pose at arc length s_k (np.interp) and the direction of the node the left-sided search finds
    PAR(lane) {
        for (int k = lane; k <= N; k += OB_NT) {
            const double s = k == N ? tot : pw_keep((double)k * step);
            int lo = 0, hi = last;
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (cum[mid] <= s) lo = mid; else hi = mid - 1; }      // the last node with cum <= s
            const int j = lo;
            double P[3];
            if (j >= last || cum[j] == s) {
                const bool g = xF && j == last;
                P[0] = g ? xF[0] : path[3 * j]; P[1] = g ? xF[1] : path[3 * j + 1]; P[2] = yw[j];
            } else {
                const bool g = xF && j + 1 == last;
                const double w = s - cum[j], h = cum[j + 1] - cum[j];
                const double x0 = path[3 * j], y0 = path[3 * j + 1], x1 = g ? xF[0] : path[3 * j + 3], y1 = g ? xF[1] : path[3 * j + 4];
                P[0] = pw_keep((x1 - x0) / h * w) + x0; P[1] = pw_keep((y1 - y0) / h * w) + y0; P[2] = pw_keep((yw[j + 1] - yw[j]) / h * w) + yw[j];
            }
            lo = 0; hi = last;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (cum[mid] >= s) hi = mid; else lo = mid + 1; }          // the first node with cum >= s
            const int idx = lo < 1 ? 1 : lo;
            xWS[4 * k] = P[0]; xWS[4 * k + 1] = P[1]; xWS[4 * k + 2] = P[2];
            syaw[k] = P[2]; sd[k] = (double)dir[idx];
        }
    }
    SYNC();
    const int n = N + 1;
    PAR(lane) {
        if (a_max > 0.0) {      // the raw speed of every interval between its pads
            for (int i = lane + 1; i <= n + PW_PAD + PW_TAIL; i += OB_NT) { const int q = i - PW_PAD - 1; vex[i] = (q >= 0 && q < N) ? sd[q + 1] * v_nom : 0.0; }
        } else {
            for (int k = lane; k <= N; k += OB_NT) sv[k] = (k == 0 || k == N || sd[k] != sd[k + 1]) ? 0.0 : sd[k] * v_nom;
        }
    }
    SYNC();
    if (a_max > 0.0) {
        // velo_smooth: every jump of the padded profile writes a ramp into one of four candidate rows, in ascending jump order, later writes winning; lane by lane the
        // value each row ends with at the lane's own sample, then the sign rule
        PAR(lane) {
            const double v1 = fabs(vex[PW_PAD + 1]), cut1 = 0.25 * v1, cut2 = 1.25 * v1;
            const long long acc = pw_round_even(v1 / a_max / Tsv);
            for (int k = lane; k <= N; k += OB_NT) {
                const long long p = PW_PAD + 1 + k;
                const double raw = vex[p];
                double bar[4] = {raw, raw, raw, raw};
                bool up_first = true, dn_first = true;
                for (int kk = 1; kk <= n + PW_PAD + PW_TAIL - 1; kk++) {
                    const double dv = vex[kk + 1] - vex[kk];
                    if (dv > cut1 && dv < cut2) {                     // rise by v_nom: start from rest, or come to rest from reverse
                        const int ke = (up_first && kk == PW_PAD) ? kk + 1 : kk;
                        up_first = false;
                        if (vex[ke] > cut1 || vex[ke + 1] > cut1) { const long long i = p - ke; if (i >= 0 && i <= acc) bar[0] = pw_ramp(i, acc, v1); }
                        else if (vex[ke] < -cut1 || vex[ke + 1] < -cut1) { const long long i = p - (ke - acc + 1); if (i >= 0 && i <= acc) bar[0] = pw_ramp(i, acc, v1) - v1; }
                    }
                    if (dv > -cut2 && dv < -cut1) {                   // fall by v_nom: come to rest, or start in reverse
                        const int ke = (dn_first && kk == PW_PAD) ? kk + 1 : kk;
                        dn_first = false;
                        if (vex[ke] > cut1 || vex[ke + 1] > cut1) { const long long i = p - (ke - acc + 1); if (i >= 0 && i <= acc) bar[1] = v1 - pw_ramp(i, acc, v1); }
                        else if (vex[ke] < -cut1 || vex[ke + 1] < -cut1) { const long long i = p - ke; if (i >= 0 && i <= acc) bar[1] = -pw_ramp(i, acc, v1); }
                    }
                    if (dv > cut2) { const long long i = p - (kk - acc); if (i >= 0 && i <= 2 * acc) bar[2] = pw_full(i, acc, v1); }      // reverse -> forward
                    if (dv < -cut2) { const long long i = p - (kk - acc); if (i >= 0 && i <= 2 * acc) bar[3] = -pw_full(i, acc, v1); }    // forward -> reverse
                }
                double out = 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) {      // a candidate of the wrong sign falls back to the raw profile
                    const double c = bar[r] == 0.0 ? 0.0 : (pw_sign(raw) != pw_sign(bar[r]) ? raw : bar[r]);
                    out = r == 0 ? c : (raw > 0.0 ? (c < out ? c : out) : (c > out ? c : out));
                }
                sv[k] = out;
            }
        }
        SYNC();
    }
    PAR(lane) {
        for (int k = lane; k <= N; k += OB_NT) {
            xWS[4 * k + 3] = sv[k];
            if (k == N) continue;
            const double s0 = pw_keep((double)k * step), s1 = k + 1 == N ? tot : pw_keep((double)(k + 1) * step), ds = s1 - s0;
            const double dsv = (ds > 1e-9 ? ds : 1e-9) * (sd[k + 1] == 0.0 ? 1.0 : sd[k + 1]);
            uWS[2 * k] = pw_clip(atan(L * (syaw[k + 1] - syaw[k]) / dsv), 0.6);
            uWS[2 * k + 1] = pw_clip((sv[k + 1] - sv[k]) / Tsv, 0.4);
        }
        if (lane == 0) *Ts = Tsv;
    }
    return 0;
}

// an instance of the host-pointer call that has no warm start: its outputs are zeros
OBCA_FN void path_ws_zero(int N, double *Ts, double *xWS, double *uWS) {
    PAR(lane) {
        for (int i = lane; i < 4 * (N + 1); i += OB_NT) xWS[i] = 0.0;
        for (int i = lane; i < 2 * N; i += OB_NT) uWS[i] = 0.0;
        if (lane == 0) *Ts = 0.0;
    }
}

// The resident call: the warm start goes into the instance's problem record p (PH_TS; rx, ry, ryaw behind OB_HDR) and its start iterate z0 (x, u, t = 1, zeros from the
// multipliers to the end of the row: the next solve runs DualMultWS as after an upload without duals).  L is the record's, the goal -- with use_xF -- too.  An instance
// whose status is negative keeps its record and its iterate as uploaded.  zlen: doubles of z0's row.
OBCA_FN int path_ws_record(int N, int count, int cap, const double *path, const int *dir, int use_xF, double v_nom, double a_max, double *p, double *z0, int zlen) {
    int st = path_ws_count_status(count, cap);
    if (st) return st;
    Lay l; make_layout(N, 0, 0, l);      // x, u, t come first in every instance's layout
    double xF[4];
#pragma unroll
    for (int i = 0; i < 4; i++) xF[i] = p[PH_XF + i];
    st = path_ws_instance(N, count, path, dir, use_xF ? xF : nullptr, v_nom, p[PH_L], a_max, p + PH_TS, z0 + l.x, z0 + l.u);
    if (st) return st;
    PAR(lane) {
        for (int k = lane; k <= N; k += OB_NT) {      // the lane that wrote stage k reads it back
            p[OB_HDR + k] = z0[l.x + 4 * k]; p[OB_HDR + (N + 1) + k] = z0[l.x + 4 * k + 1]; p[OB_HDR + 2 * (N + 1) + k] = z0[l.x + 4 * k + 2];
        }
        if (lane == 0) z0[l.t] = 1.0;
        for (int i = l.lam + lane; i < zlen; i += OB_NT) z0[i] = 0.0;
    }
    return 0;
}

}  // namespace pw
}  // namespace obca
