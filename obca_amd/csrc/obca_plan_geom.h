// obca_plan_geom.h -- what the two parking planners share, stated ONCE: the car rectangle against a field of convex obstacles, the disc of the holonomic map against the
// same field, an obstacle's rows as a polygon, the Reeds-Shepp curves and the option defaults.  Two users include it: the host search (obca_planner.cpp, plain host C++)
// and the device search's kernel text, which also compiles for the host under -DOBCA_EMU and carries it to the resident route's packing.  Both searches and every build of
// them must agree to the last bit, so none of this is written a second time anywhere.
// The device user includes this header BEHIND its `#pragma clang fp contract(off)`: no a * b + c below may become an fma.  No other header of csrc/ includes it.
// Left to each search, on purpose: wrap() (the device's is bounded, the host's takes any yaw), the integration of a motion primitive, the holonomic map, the search loops.
#pragma once
#include <math.h>
#include <vector>

// HY_FN: a function of the search (device only in a device build); HY_HD: one the host code of a device build calls as well; HY_MEMBER: a member function of the search's.
// Plain host C++ knows one kind.
#if defined(OBCA_EMU) || !defined(__HIPCC__)
#define HY_FN static inline
#define HY_HD static inline
#define HY_MEMBER
#else
#define HY_FN __device__ __forceinline__
#define HY_HD __host__ __device__ static inline
#define HY_MEMBER __device__ __forceinline__
#endif
#define HY_PI 3.14159265358979323846
// the options of a search (include/obca_plan.h: OBCA_PLAN_NOPTS doubles) where the caller sets none
#define HY_DEFAULT_OPTS {0.25, 7.5, 0.6, 0.6, 2, 0.1, 0.3, 8.0, 1.5, 2.0, 0.3, 400000, 1.0, 0.2, 1.0, 0.0, 0.0, 7.5}

namespace obca {
namespace geom {

struct P2 { double x, y; };
// An obstacle field as the tests below read it, a view of arrays someone else owns.  Obstacle j: rows off[j] .. off[j] + v[j] of A (x 2) and b, A p <= b; rn = 1 / |a_i| of
// every row (0 for a zero row) and nrm = |a_i| = hypot(A0, A1) (read by disc_collides only); the obstacle as a polygon (polygon, below): vertices voff[j] .. voff[j + 1]
// of vert (x 2).
struct Field { int nOb; const int *v, *off, *voff; const double *A, *b, *rn, *vert; const double *nrm = nullptr; };

// The smaller / larger of two numbers.  The two forms part only where an argument is not a number.  The device search refuses a start, a goal or a row that is not finite
// at its door (make_params) and never meets one; its form hands a NaN second argument on.  The host search refuses none and keeps the answer of std::min / std::max (the
// first argument), by which a pose that is not a number, or one beside a row that is none, is tested as it has always been: such a pose touches the first obstacle.
#if defined(OBCA_EMU) || defined(__HIPCC__)
HY_HD double min2(double a, double b) { return a < b ? a : b; }
HY_HD double max2(double a, double b) { return a > b ? a : b; }
#else
HY_HD double min2(double a, double b) { return b < a ? b : a; }
HY_HD double max2(double a, double b) { return a < b ? b : a; }
#endif

// convex polygon clipped by the half-plane a.p <= bb (Sutherland-Hodgman); returns the number of vertices left (at most n + 1).  (HY_HD: polygon() calls it from host code.)
HY_HD int clip(const P2 *in, int n, double ax, double ay, double bb, P2 *out) {
    int m = 0;
    for (int i = 0; i < n; i++) {
        const P2 p = in[i], q = in[i + 1 == n ? 0 : i + 1];
        const double dp = ax * p.x + ay * p.y - bb, dq = ax * q.x + ay * q.y - bb;
        if (dp <= 0) out[m++] = p;
        if ((dp < 0 && dq > 0) || (dp > 0 && dq < 0)) { const double t = dp / (dp - dq); out[m].x = p.x + t * (q.x - p.x); out[m].y = p.y + t * (q.y - p.y); m++; }
    }
    return m;
}
// One obstacle as a polygon: its `rows` half-planes (A x 2, b) cut from the square of half side far_, so an unbounded obstacle ends far outside the bounds.  pa, pb: scratch
// of 4 + rows + 1 vertices each (every half-plane adds at most one vertex to a convex polygon); the n vertices are in the one returned.
HY_HD const P2 *polygon(const double *A, const double *b, int rows, double far_, P2 *pa, P2 *pb, int &n) {
    pa[0].x = far_; pa[0].y = far_; pa[1].x = -far_; pa[1].y = far_; pa[2].x = -far_; pa[2].y = -far_; pa[3].x = far_; pa[3].y = -far_;
    n = 4; P2 *cur = pa, *nxt = pb;
    for (int i = 0; i < rows && n > 0; i++) { n = clip(cur, n, A[2 * i], A[2 * i + 1], b[i], nxt); P2 *t = cur; cur = nxt; nxt = t; }
    return cur;
}
// the same, the vertices appended to `vert` (x, y, x, y, ...)
static inline void append_polygon(const double *A, const double *b, int rows, double far_, P2 *pa, P2 *pb, std::vector<double> &vert) {
    int n; const P2 *poly = polygon(A, b, rows, far_, pa, pb, n);
    for (int i = 0; i < n; i++) { vert.push_back(poly[i].x); vert.push_back(poly[i].y); }
}
static inline double host_far(const double *XYbounds) { return 1e3 + max2(max2(fabs(XYbounds[0]), fabs(XYbounds[1])), max2(fabs(XYbounds[2]), fabs(XYbounds[3]))); }

// Does the (inflated) car rectangle at the pose overlap an obstacle?  c, s = cos, sin of the heading.  P carries the bounds of the rear-axle position (xmin, xmax, ymin,
// ymax), the inflation `margin` and ego[4] = front, left, rear, right extents from the rear axle.  The answer is DEFINED by the clipped overlap area (car cut by every
// half-plane of the obstacle, area > 1e-9); nearly every call is settled before that by the separating-axis tests of a rectangle against a convex polygon, which agree with
// it: a row all four corners violate (the clip would leave nothing), a car side every vertex of the obstacle lies beyond, or a corner deep inside every row.
// S: the clip scratch, made from P where a clip starts: a and b, 4 + (most rows of an obstacle) + 1 vertices each -- two local arrays in the device search, which caps the
// rows (declared here, inside the loop, they live for one clip only: handed in as pointers they cost the kernel three times the private memory), pointers to the carrier's
// heap buffers in the host search, which takes obstacles with any number of rows.
template <class S, class C> HY_FN bool collides_cs(const C &P, const Field &w, double x, double y, double c, double s) {
    if (x < P.xmin || x > P.xmax || y < P.ymin || y > P.ymax) return true;
    const double m = P.margin;
    const double f = P.ego[0] + m, l = P.ego[1] + m, r = P.ego[2] + m, rt = P.ego[3] + m;
    const P2 car[4] = {{x + f * c - l * s, y + f * s + l * c}, {x - r * c - l * s, y - r * s + l * c}, {x - r * c + rt * s, y - r * s - rt * c}, {x + f * c + rt * s, y + f * s - rt * c}};
    for (int j = 0; j < w.nOb; j++) {
        bool apart = false; double deep[4] = {1e300, 1e300, 1e300, 1e300};      // deep[q]: how far corner q is inside the obstacle (least over its rows)
        for (int i = 0; i < w.v[j]; i++) {
            const int rix = w.off[j] + i; const double ax = w.A[2 * rix], ay = w.A[2 * rix + 1], bb = w.b[rix];
            const double d0 = ax * car[0].x + ay * car[0].y - bb, d1 = ax * car[1].x + ay * car[1].y - bb, d2 = ax * car[2].x + ay * car[2].y - bb, d3 = ax * car[3].x + ay * car[3].y - bb;
            if (d0 > 0 && d1 > 0 && d2 > 0 && d3 > 0) { apart = true; break; }
            const double n_ = w.rn[rix];
            deep[0] = min2(deep[0], -d0 * n_); deep[1] = min2(deep[1], -d1 * n_); deep[2] = min2(deep[2], -d2 * n_); deep[3] = min2(deep[3], -d3 * n_);
        }
        if (apart) continue;
        if (max2(max2(deep[0], deep[1]), max2(deep[2], deep[3])) > 1e-3) return true;      // a quarter disc of radius 1e-3 around that corner is overlap: area > 7e-7
        {   // the car's own sides: in its frame the obstacle's vertices are (u, v_); a side with every vertex beyond it (by more than a rounding margin) separates
            const int v0 = w.voff[j], v1 = w.voff[j + 1];
            double umin = 1e300, umax = -1e300, wmin = 1e300, wmax = -1e300;
            for (int q = v0; q < v1; q++) {
                const double dx = w.vert[2 * q] - x, dy = w.vert[2 * q + 1] - y, u = c * dx + s * dy, v_ = -s * dx + c * dy;
                umin = min2(umin, u); umax = max2(umax, u); wmin = min2(wmin, v_); wmax = max2(wmax, v_);
            }
            if (v1 > v0 && (umin > f + 1e-7 || umax < -r - 1e-7 || wmin > l + 1e-7 || wmax < -rt - 1e-7)) continue;
        }
        S buf(P);
        int n = 4; for (int i = 0; i < 4; i++) buf.a[i] = car[i];
        P2 *cur = buf.a, *nxt = buf.b;
        for (int i = 0; i < w.v[j] && n > 0; i++) {
            const int rix = w.off[j] + i;
            n = clip(cur, n, w.A[2 * rix], w.A[2 * rix + 1], w.b[rix], nxt);
            P2 *t = cur; cur = nxt; nxt = t;
        }
        if (n >= 3) {   // non-degenerate overlap
            double area = 0; for (int i = 0; i < n; i++) { const P2 p = cur[i], q = cur[i + 1 == n ? 0 : i + 1]; area += p.x * q.y - q.x * p.y; }
            if (fabs(area) > 1e-9) return true;
        }
    }
    return false;
}

// Does a disc of radius rad at (x, y) touch an obstacle (the blocked cells of the holonomic map)?  The distance of the point to the convex set, conservative via the most
// violated row.  A row's slack is divided by its norm as stored in F.nrm: no libm here, so the host's map, the device's and the one a search makes itself are one byte string.
HY_HD bool disc_collides(const Field &F, double x, double y, double rad) {
    for (int j = 0; j < F.nOb; j++) {
        double worst = -1e300;
        for (int i = 0; i < F.v[j]; i++) { const int r = F.off[j] + i; const double e = (F.A[2 * r] * x + F.A[2 * r + 1] * y - F.b[r]) / F.nrm[r]; worst = e > worst ? e : worst; }
        if (worst < rad) {   // inside the rad-offset of every half-plane: within rad of the set unless near a corner (then slightly conservative)
            if (worst <= 0) return true;
            // corner case: exact distance to the set is >= worst; test the rounded corner with the violated rows
            int cnt = 0; double d2 = 0;
            for (int i = 0; i < F.v[j]; i++) { const int r = F.off[j] + i; const double e = (F.A[2 * r] * x + F.A[2 * r + 1] * y - F.b[r]) / F.nrm[r]; if (e > 0) { d2 += e * e; cnt++; } }
            if (cnt <= 1 || d2 < rad * rad) return true;
        }
    }
    return false;
}

// ---------------------------------------------------------------- Reeds-Shepp curves (the only code of the device search that calls libm)
// Shortest path of a car that drives forwards and backwards with a bounded turning radius (Reeds & Shepp 1990), in the normalised problem (unit radius, start at the origin
// with heading 0): the 48 candidate words are generated from the closed-form families CSC, CCC, CCCC, CCSC, CCSCC and the time-flip / reflection / backwards symmetries,
// the shortest is kept.  Stands where hybrid_a_star.jl:262-300 calls reeds_shepp.calc_shortest_path (reeds_shepp.jl).  A path is at most five segments of type 0 S
// (signed length), 1 L or 2 R (arc, signed angle).
struct RsPath { char type[5]; double len[5]; int n; double total; };
// One mirror image of the query, (x, y, phi), with what the families share: sin / cos of phi, the two centre offsets (xi, eta) = (x -+ sin phi, y - 1 +- cos phi) and
// their polar forms: (xm, em, rm, tm) for LSL, LRL, LRSL; (xp, ep, rp, tp) for LSR, LRLR, LRSR, LRSLR.  A family is a few lines on top of these; evaluating the 44 family
// calls of a query from scratch costs ~200 libm calls, from here ~50.
struct Pre { double x, y, phi, sp, cp, xm, em, rm, tm, xp, ep, rp, tp; };
#define HY_ZERO 1e-12
HY_FN double mod2pi(double x) { double v = fabs(x) < 2 * HY_PI ? x : fmod(x, 2 * HY_PI); if (v < -HY_PI) v += 2 * HY_PI; else if (v > HY_PI) v -= 2 * HY_PI; return v; }      // (fmod returns such an x itself)
HY_FN void tau_omega(double u, double v, double xi, double eta, double phi, double &tau, double &omega) {
    const double delta = mod2pi(u - v), A = sin(u) - sin(delta), B = cos(u) - cos(delta) - 1.0;
    const double t1 = atan2(eta * A - xi * B, xi * A + eta * B), t2 = 2.0 * (cos(delta) - cos(v) - cos(u)) + 3.0;
    tau = t2 < 0 ? mod2pi(t1 + HY_PI) : mod2pi(t1);
    omega = mod2pi(tau - u + v - phi);
}
HY_FN Pre make_pre(double x, double y, double phi, double sp, double cp, bool polar_p) {
    Pre q; q.x = x; q.y = y; q.phi = phi; q.sp = sp; q.cp = cp;
    q.xm = x - sp; q.em = y - 1.0 + cp; q.rm = hypot(q.xm, q.em); q.tm = atan2(q.em, q.xm);
    q.xp = x + sp; q.ep = y - 1.0 - cp; q.rp = hypot(q.xp, q.ep); q.tp = polar_p && q.rp >= 2.0 ? atan2(q.ep, q.xp) : 0;      // (the angle: LSR only, which needs rp >= 2)
    return q;
}
// the families by number: 0 LpSpLp, 1 LpSpRp, 2 LpRmL, 3 LpRupLumRm, 4 LpRumLumRp, 5 LpRmSmLm, 6 LpRmSmRm, 7 LpRmSLmRp
HY_FN bool family(int fam, const Pre &q, double &t, double &u, double &v) {
    switch (fam) {
    case 0: u = q.rm; t = q.tm; if (t >= -HY_ZERO) { v = mod2pi(q.phi - t); if (v >= -HY_ZERO) return true; } return false;
    case 1: { double u1 = q.rp; const double t1 = q.tp; u1 *= u1;
              if (u1 >= 4.0) { u = sqrt(u1 - 4.0); const double th = atan2(2.0, u); t = mod2pi(t1 + th); v = mod2pi(t - q.phi); return t >= -HY_ZERO && v >= -HY_ZERO; } return false; }
    case 2: { const double u1 = q.rm, th = q.tm;
              if (u1 <= 4.0) { u = -2.0 * asin(0.25 * u1); t = mod2pi(th + 0.5 * u + HY_PI); v = mod2pi(q.phi - t + u); return t >= -HY_ZERO && u <= HY_ZERO; } return false; }
    case 3: { const double rho = 0.25 * (2.0 + q.rp);
              if (rho <= 1.0) { u = acos(rho); tau_omega(u, -u, q.xp, q.ep, q.phi, t, v); return t >= -HY_ZERO && v <= HY_ZERO; } return false; }
    case 4: { const double rho = (20.0 - q.xp * q.xp - q.ep * q.ep) / 16.0;
              if (rho >= 0 && rho <= 1) { u = -acos(rho); if (u >= -0.5 * HY_PI) { tau_omega(u, u, q.xp, q.ep, q.phi, t, v); return t >= -HY_ZERO && v >= -HY_ZERO; } } return false; }
    case 5: { const double rho = q.rm, th = q.tm;
              if (rho >= 2.0) { const double r = sqrt(rho * rho - 4.0); u = 2.0 - r; t = mod2pi(th + atan2(r, -2.0)); v = mod2pi(q.phi - 0.5 * HY_PI - t); return t >= -HY_ZERO && u <= HY_ZERO && v <= HY_ZERO; } return false; }
    case 6: { const double rho = q.rp;                                       // polar form of (-eta, xi): the same radius, the angle atan2(xi, -eta) -- negative (a reject) for xi < 0
              if (rho >= 2.0 && !(q.xp < -1e-9 * (1.0 + fabs(q.ep)))) { t = atan2(q.xp, -q.ep); u = 2.0 - rho; v = mod2pi(t + 0.5 * HY_PI - q.phi); return t >= -HY_ZERO && u <= HY_ZERO && v <= HY_ZERO; } return false; }
    default: { const double xi = q.xp, eta = q.ep, rho = q.rp;
              if (rho >= 2.0) { u = 4.0 - sqrt(rho * rho - 4.0);
                  if (u <= HY_ZERO) { t = mod2pi(atan2((4.0 - u) * xi - 2.0 * eta, -2.0 * xi + (u - 4.0) * eta)); v = mod2pi(t - q.phi); return t >= -HY_ZERO && v >= -HY_ZERO; } } return false; }
    }
}
// how (t, u, v) become the segment lengths: 0 t u v, 1 v u t, 2 t u -u v, 3 t u u v, 4 t -pi/2 u v, 5 v u -pi/2 t, 6 t -pi/2 u -pi/2 v
HY_FN void fill(int how, double t, double u, double v, double *l) {
    const double q = -0.5 * HY_PI;
    switch (how) {
    case 0: l[0] = t; l[1] = u; l[2] = v; break;
    case 1: l[0] = v; l[1] = u; l[2] = t; break;
    case 2: l[0] = t; l[1] = u; l[2] = -u; l[3] = v; break;
    case 3: l[0] = t; l[1] = u; l[2] = u; l[3] = v; break;
    case 4: l[0] = t; l[1] = q; l[2] = u; l[3] = v; break;
    case 5: l[0] = v; l[1] = u; l[2] = q; l[3] = t; break;
    default: l[0] = t; l[1] = q; l[2] = u; l[3] = q; l[4] = v; break;
    }
}
// word: the n segment types packed two bits each (0 S, 1 L, 2 R); mirror: L <-> R
HY_FN void offer(RsPath &best, int word, bool mirror, int n, const double *len, bool neg) {
    double tot = 0; for (int i = 0; i < n; i++) tot += fabs(len[i]);
    if (tot < best.total) {
        best.n = n; best.total = tot;
        for (int i = 0; i < n; i++) { const int ty = (word >> (2 * i)) & 3; best.type[i] = (char)(ty == 0 ? 0 : (mirror ? 3 - ty : ty)); best.len[i] = neg ? -len[i] : len[i]; }
    }
}
// every family is tried on (x, y, phi), its time flip (-x, y, -phi: all lengths negated), its reflection (x, -y, -phi: L <-> R) and both: q[0..3]
HY_FN void four(RsPath &best, int fam, const Pre *q, int word, int n, int how) {
    double t, u, v, len[5];
    for (int k = 0; k < 4; k++)
        if (family(fam, q[k], t, u, v)) { fill(how, t, u, v, len); offer(best, word, k >= 2, n, len, (k & 1) != 0); }
}
#define HY_WORD(a, b, c, d, e) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6) | ((e) << 8))
HY_FN RsPath rs_shortest(double x, double y, double phi) {
    RsPath best; best.n = 0; best.total = 1e300;
    for (int i = 0; i < 5; i++) { best.type[i] = 0; best.len[i] = 0.0; }
    const double sp = sin(phi), cp = cos(phi);                  // (sin, cos of -phi are -sp, cp: libm's sin is odd and its cos even to the last bit)
    const double xb = x * cp + y * sp, yb = x * sp - y * cp;    // the same word driven backwards
    const Pre q[4] = {make_pre(x, y, phi, sp, cp, true), make_pre(-x, y, -phi, -sp, cp, true), make_pre(x, -y, -phi, -sp, cp, true), make_pre(-x, -y, phi, sp, cp, true)};
    const Pre qb[4] = {make_pre(xb, yb, phi, sp, cp, false), make_pre(-xb, yb, -phi, -sp, cp, false), make_pre(xb, -yb, -phi, -sp, cp, false), make_pre(-xb, -yb, phi, sp, cp, false)};
    enum { S = 0, L = 1, R = 2 };
    four(best, 0, q, HY_WORD(L, S, L, 0, 0), 3, 0);
    four(best, 1, q, HY_WORD(L, S, R, 0, 0), 3, 0);
    four(best, 2, q, HY_WORD(L, R, L, 0, 0), 3, 0);
    four(best, 2, qb, HY_WORD(L, R, L, 0, 0), 3, 1);
    four(best, 3, q, HY_WORD(L, R, L, R, 0), 4, 2);
    four(best, 4, q, HY_WORD(L, R, L, R, 0), 4, 3);
    four(best, 5, q, HY_WORD(L, R, S, L, 0), 4, 4);
    four(best, 6, q, HY_WORD(L, R, S, R, 0), 4, 4);
    four(best, 5, qb, HY_WORD(L, S, R, L, 0), 4, 5);
    four(best, 6, qb, HY_WORD(R, S, R, L, 0), 4, 5);
    four(best, 7, q, HY_WORD(L, R, S, L, R), 5, 6);
    return best;
}
// advance a pose along one segment (type ty) by the signed amount s (unit radius); sy, cy: sin, cos of `yaw` on entry and on exit -- a walk along a path asks libm for
// each angle once
HY_FN void advance_sc(int ty, double s, double &x, double &y, double &yaw, double &sy, double &cy) {
    if (ty == 0) { x += s * cy; y += s * sy; }
    else { const double k = ty == 1 ? 1.0 : -1.0, y1 = yaw + k * s, s1 = sin(y1), c1 = cos(y1); x += k * (s1 - sy); y += -k * (c1 - cy); yaw = y1; sy = s1; cy = c1; }
}

}  // namespace geom
}  // namespace obca
