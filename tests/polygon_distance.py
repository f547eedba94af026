"""Exact distance between the car rectangle and a convex obstacle given as half-planes, in plain numpy fp64: the independent answer the DualMultWS tests are held against
(tests/test_dualws_geometry_cpu.py, tests/test_gpu_dualws_geometry.py; the expected values of tests/golden/dualws_polygons.npz are computed here and a second time
with mpmath at 40 digits by tests/golden/make_dualws_polygons.py).  Nothing here iterates: vertices from pairs of rows, a separating-axis test, point-segment distances.

  car       {e + R(psi) y : |y_1| <= L_ev / 2, |y_2| <= W_ev / 2},  e = (X, Y) + off (cos psi, sin psi),  off = (ego[0] + ego[2]) / 2 - ego[2]      (the centre of dualmult_ws)
  obstacle  {p : A p <= b}; one of 1 or 2 rows is unbounded and is cut with the box |p_i| <= BOX for this reference only
  distance  0 if no row of the obstacle and no side of the car separates the two (they touch or overlap), else the smallest distance of a vertex of one to an edge of the other

certificate(): the conditions under which multipliers (lam, mu) prove that the distance is at least d (weak duality of DualMultWS.jl:52-73)."""
import numpy as np

BOX = 1e3


def car_geometry(ego):
    """(g, off): the half sizes [L_ev/2, W_ev/2, L_ev/2, W_ev/2] and the offset of the rectangle's centre from the rear axle along the heading"""
    ego = np.asarray(ego, float).ravel()
    L_ev, W_ev = ego[0] + ego[2], ego[1] + ego[3]
    return np.array([L_ev / 2, W_ev / 2, L_ev / 2, W_ev / 2]), (ego[0] + ego[2]) / 2 - ego[2]


def car_rectangle(X, Y, psi, ego):
    """(4, 2) corners, counter-clockwise"""
    g, off = car_geometry(ego)
    cs, sn = np.cos(psi), np.sin(psi)
    e = np.array([X + cs * off, Y + sn * off])
    u, w = np.array([cs, sn]), np.array([-sn, cs])
    return np.array([e + g[0] * u + g[1] * w, e - g[0] * u + g[1] * w, e - g[0] * u - g[1] * w, e + g[0] * u - g[1] * w])


def _rows(A, b):
    A = np.asarray(A, float).reshape(-1, 2); b = np.asarray(b, float).ravel()
    if len(b) <= 2:
        A = np.vstack([A, [[1, 0], [-1, 0], [0, 1], [0, -1]]]); b = np.r_[b, [BOX] * 4]
    return A, b


def hrep_vertices(A, b):
    """(n, 2) vertices, counter-clockwise, of {p : A p <= b}: every intersection of two rows that satisfies all rows, duplicates (redundant rows) merged.  1 or 2 rows are cut
    with the box first."""
    A, b = _rows(A, b)
    nr = np.hypot(A[:, 0], A[:, 1])
    pts = []
    for i in range(len(b)):
        for j in range(i + 1, len(b)):
            det = A[i, 0] * A[j, 1] - A[i, 1] * A[j, 0]
            if abs(det) <= 1e-12 * nr[i] * nr[j]:
                continue
            p = np.array([(b[i] * A[j, 1] - A[i, 1] * b[j]) / det, (A[i, 0] * b[j] - b[i] * A[j, 0]) / det])
            if ((A @ p - b) / nr <= 1e-9 * max(1.0, np.abs(p).max())).all():
                pts.append(p)
    assert len(pts) >= 3, "the half-planes bound no polygon"
    pts = np.array(pts); keep = []
    for k, p in enumerate(pts):
        if all(np.abs(p - pts[m]).max() > 1e-9 * max(1.0, np.abs(p).max()) for m in keep):
            keep.append(k)
    pts = pts[keep]; c = pts.mean(axis=0)
    return pts[np.argsort(np.arctan2(pts[:, 1] - c[1], pts[:, 0] - c[0]))]


def _point_segments(P, Q):
    """smallest distance of the points P (m, 2) to the edges of the closed polygon Q (n, 2)"""
    a = Q; d = np.roll(Q, -1, axis=0) - Q
    w = P[:, None, :] - a[None, :, :]
    t = np.clip((w * d[None]).sum(-1) / (d * d).sum(-1)[None], 0.0, 1.0)
    r = w - t[..., None] * d[None]
    return np.sqrt((r * r).sum(-1)).min()


def _points_rows(P, A, b, V):
    """smallest distance of the points P (m, 2) to the edges of the polygon A p <= b with vertices V: over an edge's interior the distance is the row's own residual
    (a'p - b) / |a| -- the far ends of a long edge, known only to 1e-16 of their size, do not enter --, beyond its ends the distance to the end"""
    best = np.inf
    for a, bi in zip(A, b):
        nr = np.hypot(a[0], a[1]); t = np.array([-a[1], a[0]]) / nr
        on = V[np.abs(V @ a - bi) / nr <= 1e-9 * np.maximum(1.0, np.abs(V).max(axis=1))]
        if len(on) < 2:
            continue      # a redundant row carries no edge
        s = on @ t; lo, hi = on[np.argmin(s)], on[np.argmax(s)]
        for p in P:
            sp = p @ t
            best = min(best, abs(p @ a - bi) / nr if s.min() <= sp <= s.max() else np.hypot(*(p - (lo if sp < s.min() else hi))))
    return best


def polygon_distance(X, Y, psi, ego, A, b):
    """distance of the car at pose (X, Y, psi) to the obstacle A p <= b; 0 if they touch or overlap"""
    A = np.asarray(A, float).reshape(-1, 2); b = np.asarray(b, float).ravel()
    car = car_rectangle(X, Y, psi, ego); ob = hrep_vertices(A, b)
    # separating axes: a row of the obstacle (its support is b itself) or a side of the car
    sep = (((car @ A.T).min(axis=0) - b) / np.hypot(A[:, 0], A[:, 1])).max()
    for i in range(2):
        n = car[i] - car[i + 1]; n = n / np.hypot(n[0], n[1])
        pc, po = car @ n, ob @ n
        sep = max(sep, po.min() - pc.max(), pc.min() - po.max())
    if sep <= 0:
        return 0.0
    return float(min(_points_rows(car, *_rows(A, b), ob), _point_segments(ob, car)))


def certificate(X, Y, psi, ego, A, b, lam, mu, d):
    """The dual certificate of DualMultWS for a returned (lam, mu, d), with A, b and lam in the caller's row scaling.  Returns a dict of the four violations, each
    divided by its bound: all <= 1 means the multipliers prove distance >= d.
      sign        -min(lam, mu) against 0 (reported as is: must be <= 0)
      norm        |A' lam| - 1                        against 1e-12
      equality    |G' mu + R' A' lam|_inf             against 1e-12 max(1, |lam|_1)
      objective   |-g' mu + (A e - b)' lam - d|       against 1e-12 max(1, d)"""
    A = np.asarray(A, float).reshape(-1, 2); b = np.asarray(b, float).ravel(); lam = np.asarray(lam, float).ravel(); mu = np.asarray(mu, float).ravel()
    g, off = car_geometry(ego); cs, sn = np.cos(psi), np.sin(psi)
    e = np.array([X + cs * off, Y + sn * off])
    p = A.T @ lam
    rp = np.array([cs * p[0] + sn * p[1], -sn * p[0] + cs * p[1]])      # R' A' lam
    eq = np.array([mu[0] - mu[2], mu[1] - mu[3]]) + rp
    obj = -g @ mu + (A @ e - b) @ lam
    return dict(sign=float(-min(lam.min(), mu.min())), norm=float((np.hypot(p[0], p[1]) - 1) / 1e-12),
                equality=float(np.abs(eq).max() / (1e-12 * max(1.0, np.abs(lam).sum()))), objective=float(abs(obj - d) / (1e-12 * max(1.0, d))))


def certificate_ok(c):
    return c["sign"] <= 0 and c["norm"] <= 1 and c["equality"] <= 1 and c["objective"] <= 1
