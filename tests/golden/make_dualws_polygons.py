"""Writes tests/golden/dualws_polygons.npz: (pose, convex obstacle) problems of DualMultWS with the exact distance of the car rectangle to the obstacle.

    python tests/golden/make_dualws_polygons.py [--check]      (--check: compute everything, write nothing)

Every distance is computed twice from the H-rep the file stores -- by tests/polygon_distance.py (numpy fp64: separating axes, vertex-edge distances) and here with mpmath
at 40 digits by another route (vertices inside the other polygon, crossing edges, segment-segment distances) -- and the file is written only if the two agree to
1e-13 max(1, d) on every case.  No solver, no iteration of the project takes part.  Fixed seed; the families are listed in families() below.

Arrays (n cases): A (n, 8, 2) and b (n, 8) padded with zeros, v (n,) rows, pose (n, 3) = X, Y, psi, d (n,), family (n,), name (n,), ego (4,).
No exact gap lies in (8e-8, 1.2e-7): the clearance record's threshold CL_TOUCH = 1e-7 -+ the tolerance of the tests."""
import os
import sys
import numpy as np
import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import polygon_distance as PD      # noqa: E402
from obca_amd import scenarios as S      # noqa: E402

mp.mp.dps = 40
EGO = S.EGO
GAPS = (1e-6, 1e-4, 1e-2, 0.3, 2.0, 5.0, 10.0, 20.0, 40.0)
ASPECTS = (1.0, 0.3, 3.0, 0.05, 8.0)
WEDGES = (("wedge_9.8cm", 10.84), ("wedge_37cm", 14.84), ("wedge_82cm", 22.84))


# ---------------------------------------------------------------- H-rep of a counter-clockwise polygon
def hrep(P, scaled=False):
    """rows of the edges P[i] -> P[i + 1], outward normals: of unit length, or of the edge's length (scaled)"""
    P = np.asarray(P, float); d = np.roll(P, -1, axis=0) - P
    n = np.stack([d[:, 1], -d[:, 0]], axis=1)
    if not scaled:
        n = n / np.hypot(n[:, 0], n[:, 1])[:, None]
    return n, (n * P).sum(axis=1)


def regular(n, radius, aspect, rot):
    """a regular n-gon of the given radius, stretched by `aspect` along x, then turned by `rot`"""
    t = 2 * np.pi * np.arange(n) / n + 0.3
    P = np.stack([aspect * radius * np.cos(t), radius * np.sin(t)], axis=1)
    c, s = np.cos(rot), np.sin(rot)
    return P @ np.array([[c, s], [-s, c]])


def place(P, pose, theta, gap):
    """P moved along the direction theta from the car's centre until its exact distance to the car is `gap` (bisection on the shift)"""
    _, off = PD.car_geometry(EGO)
    c0 = np.array([pose[0] + off * np.cos(pose[2]), pose[1] + off * np.sin(pose[2])]); u = np.array([np.cos(theta), np.sin(theta)])
    dist = lambda t: PD.polygon_distance(*pose, EGO, *hrep(P + c0 + t * u))
    lo, hi = 0.0, 200.0
    assert dist(lo) < gap < dist(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if dist(mid) < gap:
            lo = mid
        else:
            hi = mid
    return P + c0 + hi * u


# ---------------------------------------------------------------- the second computation: mpmath, by another route
def _mp_vertices(A, b):
    A = [[mp.mpf(float(x)) for x in r] for r in A]; b = [mp.mpf(float(x)) for x in b]
    if len(b) <= 2:
        A += [[mp.mpf(1), mp.mpf(0)], [mp.mpf(-1), mp.mpf(0)], [mp.mpf(0), mp.mpf(1)], [mp.mpf(0), mp.mpf(-1)]]; b += [mp.mpf(PD.BOX)] * 4
    pts = []
    for i in range(len(b)):
        for j in range(i + 1, len(b)):
            det = A[i][0] * A[j][1] - A[i][1] * A[j][0]
            if abs(det) <= mp.mpf(10) ** -25 * mp.hypot(*A[i]) * mp.hypot(*A[j]):
                continue
            p = ((b[i] * A[j][1] - A[i][1] * b[j]) / det, (A[i][0] * b[j] - b[i] * A[j][0]) / det)
            if all((A[k][0] * p[0] + A[k][1] * p[1] - b[k]) / mp.hypot(*A[k]) <= mp.mpf(10) ** -25 for k in range(len(b))):
                if all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) > mp.mpf(10) ** -20 for q in pts):
                    pts.append(p)
    c = (sum(p[0] for p in pts) / len(pts), sum(p[1] for p in pts) / len(pts))
    return sorted(pts, key=lambda p: mp.atan2(p[1] - c[1], p[0] - c[0]))


def _mp_point_segment(p, a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    t = ((p[0] - a[0]) * dx + (p[1] - a[1]) * dy) / (dx * dx + dy * dy)
    t = min(max(t, mp.mpf(0)), mp.mpf(1))
    return mp.hypot(p[0] - a[0] - t * dx, p[1] - a[1] - t * dy)


def _mp_inside(p, Q):
    """p in the closed counter-clockwise polygon Q"""
    n = len(Q)
    return all((Q[(i + 1) % n][0] - Q[i][0]) * (p[1] - Q[i][1]) - (Q[(i + 1) % n][1] - Q[i][1]) * (p[0] - Q[i][0]) >= 0 for i in range(n))


def _mp_cross(a, b, c, d):
    """the open segments a-b and c-d cross properly"""
    o = lambda p, q, r: (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])
    return o(a, b, c) * o(a, b, d) < 0 and o(c, d, a) * o(c, d, b) < 0


def mp_distance(pose, A, b):
    X, Y, psi = (mp.mpf(float(x)) for x in pose); ego = [mp.mpf(float(x)) for x in EGO]
    hl, hw, off = (ego[0] + ego[2]) / 2, (ego[1] + ego[3]) / 2, (ego[0] + ego[2]) / 2 - ego[2]
    # the heading enters as the fp64 cosine and sine the project's code forms: the rectangle of THOSE numbers is the one every implementation sees
    cs, sn = mp.mpf(float(np.cos(float(pose[2])))), mp.mpf(float(np.sin(float(pose[2]))))
    e = (X + cs * off, Y + sn * off)
    car = [(e[0] + sx * hl * cs - sy * hw * sn, e[1] + sx * hl * sn + sy * hw * cs) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    ob = _mp_vertices(A, b)
    if any(_mp_inside(p, ob) for p in car) or any(_mp_inside(p, car) for p in ob):
        return mp.mpf(0)
    ec = [(car[i], car[(i + 1) % 4]) for i in range(4)]; eo = [(ob[i], ob[(i + 1) % len(ob)]) for i in range(len(ob))]
    if any(_mp_cross(*s, *t) for s in ec for t in eo):
        return mp.mpf(0)
    return min(min(_mp_point_segment(p, *t) for p in car for t in eo), min(_mp_point_segment(p, *s) for p in ob for s in ec))


# ---------------------------------------------------------------- the families
def families():
    rng = np.random.default_rng(20261019)
    out = []      # (family, name, pose, A, b)

    def add(family, name, pose, A, b):
        out.append((family, name, np.array(pose, float), np.array(A, float).reshape(-1, 2), np.array(b, float).ravel()))

    # 1. regular and stretched polygons, 3 .. 8 rows, placed at the nine gaps; each once with unit rows, once with rows of the edges' lengths
    for n in range(3, 9):
        for asp in ASPECTS:
            for gap in GAPS:
                radius = rng.uniform(0.2, 4.0); pose = (rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-np.pi, np.pi))
                P = place(regular(n, radius, asp, rng.uniform(0, 2 * np.pi)), pose, rng.uniform(0, 2 * np.pi), gap)
                assert np.ptp(P, axis=0).max() <= 64.0
                fam = "regular" if asp == 1.0 else "stretched"
                for scaled in (False, True):
                    add(fam, "%s_n%d_a%g_gap%g_%s" % (fam, n, asp, gap, "edge" if scaled else "unit"), pose, *hrep(P, scaled))
    # 2. the three wedges: a long thin triangle pointing at the car from a few metres
    for name, tip in WEDGES:
        add("wedge", name, (0.0, 0.0, 1.0), *hrep([(tip, 0.0), (tip + 30.0, -1.0), (tip + 30.0, 1.0)]))
    # 3. axis-aligned boxes against the car at multiples of pi / 2: face to face (parallel edges) and corner to corner
    for psi, pn in ((0.0, "0"), (np.pi / 2, "pi/2"), (-np.pi / 2, "-pi/2"), (np.pi, "pi"), (7 * np.pi, "7pi")):
        pose = (1.5, 2.25, psi); R = PD.car_rectangle(*pose, EGO); xm, ym = R[:, 0].max(), R[:, 1].max()
        for gap in (0.0, 1e-8, 1e-6, 1e-3, 0.05, 1.0):
            x0 = xm + gap; y0 = ym - 0.75
            add("box", "box_face_psi%s_gap%g" % (pn, gap), pose, *hrep([(x0, y0), (x0 + 2, y0), (x0 + 2, y0 + 2), (x0, y0 + 2)]))
            x0, y0 = xm + gap / np.sqrt(2), ym + gap / np.sqrt(2)
            add("box", "box_corner_psi%s_gap%g" % (pn, gap), pose, *hrep([(x0, y0), (x0 + 2, y0), (x0 + 2, y0 + 1.5), (x0, y0 + 1.5)]))
    # 4. overlaps
    pose = (0.5, -0.25, 0.4); _, off = PD.car_geometry(EGO); c = np.array([pose[0] + off * np.cos(0.4), pose[1] + off * np.sin(0.4)])
    add("overlap", "overlap_deep_box", pose, *hrep(np.array([(0, -1.5), (3, -1.5), (3, 1.5), (0, 1.5)]) + c))
    add("overlap", "overlap_car_inside_30m_hexagon", pose, *hrep(regular(6, 30.0, 1.0, 0.2) + c + (3.0, -2.0)))
    add("overlap", "overlap_10cm_pentagon_inside_car", pose, *hrep(regular(5, 0.05, 1.0, 0.1) + c + (0.4, 0.2)))
    add("overlap", "overlap_corner_in_triangle", pose, *hrep(regular(3, 2.0, 1.0, 1.0) + PD.car_rectangle(*pose, EGO)[0]))
    # 5. small and thin obstacles
    for gap in (1e-4, 0.3, 2.0):
        pose = (rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-np.pi, np.pi))
        add("small", "small_1mm_square_gap%g" % gap, pose, *hrep(place(regular(4, 0.0005 * np.sqrt(2), 1.0, rng.uniform(0, 1)), pose, rng.uniform(0, 6), gap)))
        sl = np.array([(-1.0, -0.001), (1.0, -0.001), (1.0, 0.001), (-1.0, 0.001)]); r = rng.uniform(0, np.pi); cr, sr = np.cos(r), np.sin(r)
        add("small", "sliver_1e-3_gap%g" % gap, pose, *hrep(place(sl @ np.array([[cr, sr], [-sr, cr]]), pose, rng.uniform(0, 6), gap)))
    # 6. unbounded obstacles: half-planes, and the obstacles of the shipped scenarios (quadrants of 2 rows, half-planes of 1)
    for i in range(12):
        t = rng.uniform(0, 2 * np.pi); a = np.array([np.cos(t), np.sin(t)]) * (1.0 if i % 2 else rng.uniform(0.2, 30)); pose = (rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-np.pi, np.pi))
        gap = (-1.0, 1e-6, 0.02, 0.7, 6.0, 35.0)[i // 2]
        add("halfplane", "halfplane_%d_gap%g" % (i, gap), pose, a[None, :], [(PD.car_rectangle(*pose, EGO) @ a).min() - gap * np.hypot(*a)])
    for sn, sc in (("backwards", S.BACKWARDS), ("parallel", S.PARALLEL)):
        A, b, v = S.scenario_hrep(sc); r0 = 0
        for j, vj in enumerate(v):
            for q in range(6):
                pose = (rng.uniform(-10, 10), rng.uniform(5.5, 10), rng.uniform(-np.pi, np.pi))
                add("scenario", "%s_obstacle%d_pose%d" % (sn, j, q), pose, A[r0:r0 + vj], b[r0:r0 + vj])
            r0 += vj
    return out


def main(check_only):
    cases = families(); n = len(cases)
    A = np.zeros((n, 8, 2)); b = np.zeros((n, 8)); v = np.zeros(n, np.int32); pose = np.zeros((n, 3)); d = np.zeros(n); worst = 0.0
    for i, (fam, name, ps, Ai, bi) in enumerate(cases):
        vi = len(bi); assert 1 <= vi <= 8
        A[i, :vi] = Ai; b[i, :vi] = bi; v[i] = vi; pose[i] = ps
        d[i] = PD.polygon_distance(*ps, EGO, Ai, bi)
        dm = mp_distance(ps, Ai, bi)
        err = float(abs(mp.mpf(d[i]) - dm)); worst = max(worst, err / max(1.0, d[i]))
        if err > 1e-13 * max(1.0, d[i]):
            sys.exit("refused: %s numpy %.17g mpmath %s differ by %.3g" % (name, d[i], mp.nstr(dm, 20), err))
        if 8e-8 < d[i] < 1.2e-7:
            sys.exit("refused: %s has an exact gap of %.3g, inside the clearance threshold's window" % (name, d[i]))
    fams = np.array([c[0] for c in cases]); names = np.array([c[1] for c in cases])
    assert len(set(names.tolist())) == n
    print("%d cases; numpy and mpmath agree to %.3g max(1, d); per family: %s" % (n, worst, {f: int((fams == f).sum()) for f in sorted(set(fams.tolist()))}))
    if not check_only:
        np.savez_compressed(os.path.join(HERE, "dualws_polygons.npz"), A=A, b=b, v=v, pose=pose, d=d, family=fams, name=names, ego=np.asarray(EGO, float))


if __name__ == "__main__":
    main("--check" in sys.argv[1:])
