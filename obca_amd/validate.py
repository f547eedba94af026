"""
A-posteriori feasibility checkers for returned trajectories -- the public validate() API.  Pure numpy,
no GPU, no oracle: they look only at a solution.

parking_constraints_ref : restatement of /root/reference/AutonomousParking/ParkingConstraints.jl:29-149 VERBATIM, including its
    quirks: in variable-time mode all four dynamics residuals are written to c3[0,i] (only the last, the speed
    row, survives, :76-79); c6 is overwritten per obstacle so only the LAST obstacle is checked (:108-130); the c6[3] row
    ignores the slack (:127-128); the steering-rate check divides by timeScale[0] only (:88).  It is the reference's own
    acceptance test (tolerance 5e-5, :133-139) and decides exitflag after failed attempts (ParkingSignedDist.jl:278-283, ParkingDist.jl).
parking_constraints_ref_worst : the maximum that parking_constraints_ref thresholds (the device-side check reports it as `ref_worst`).
parking_constraints_full : a correct checker of every constraint class of ParkingSignedDist.jl:100-207 (with the slack),
    returning the individual maxima.
validate_parking : (ok, violations) of one returned parking solution; validate_quadcopter: restatement of
    /root/reference/QuadcopterNavigation/constrSatisfaction.jl:25-204 (tolerance 1e-3; single-index gyroscopic quirk included).
parking_samples, quad_clearance, clearance_record : the numpy statement of the between-node clearance check (obca_amd/csrc/obca_clearance.h, Batch.clearance):
    the sample poses of a parking trajectory, the clearance record of a quadcopter trajectory, and the record of any (samples, obstacles) table of clearances.
refine_parking : the numpy statement of the refinement of a solved parking instance onto a finer horizon (obca_amd/csrc/obca_refine.h, Batch.refine).
refine_quad : the same for a solved quadcopter instance (obca_amd/csrc/obca_quad_subdivide.h, QuadBatch.refine).
rollout_parking, rollout_quad, rollout_record : the numpy statement of the rollout of a solution on the continuous vehicle models (obca_amd/csrc/obca_rollout.h,
    Batch.rollout, QuadBatch.rollout): held inputs, classical RK4, the rolled node states, the sample poses and the record of deviations and clearances.
track_gains_parking, track_gains_quad, track_parking, track_quad, track_record : the numpy statement of the closed-loop rollout (obca_amd/csrc/obca_track.h, Batch.track,
    QuadBatch.track): the interval map's derivatives by forward-mode tangents, the Riccati recursion, the held TVLQR feedback on the continuous models and its record.
certify_lipschitz_parking, certify_lipschitz_quad, certify_parking, certify_quad, certify_record : the numpy statement of the clearance certificate (obca_amd/csrc/obca_certify.h,
    Batch.certify, QuadBatch.certify): the speed bound of an interval, conservative advancement of every (interval, obstacle) item with a distance the caller passes, and the record.
Shapes follow the reference: x (4,N+1), u (2,N), l (M,N+1), n (4nOb,N+1), timeScale (N+1,) .
"""
import math
import numpy as np

DMIN = 0.05


def _geom(ego):
    ego = np.asarray(ego, float).ravel()
    W_ev, L_ev = ego[1] + ego[3], ego[0] + ego[2]
    return np.array([L_ev / 2, W_ev / 2, L_ev / 2, W_ev / 2]), (ego[0] + ego[2]) / 2 - ego[2]


def _dyn(x, u, ts, Ts, L):
    q = ts * Ts
    s = x[3] + q / 2 * u[1]
    phi = x[2] + q / 2 * x[3] * np.tan(u[0]) / L
    return np.array([x[0] + q * s * np.cos(phi), x[1] + q * s * np.sin(phi), x[2] + q * s * np.tan(u[0]) / L, x[3] + q * u[1]])


def _parking_ref_classes(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd):
    """the seven quantities ParkingConstraints.jl:133-139 compares with 5e-5"""
    x0 = np.ravel(x0); xF = np.ravel(xF); vOb = [int(v) for v in np.ravel(vOb)]
    A = np.asarray(A, float).reshape(-1, 2); b = np.ravel(b)
    timeScale = np.ravel(timeScale)
    c0 = np.zeros(5)
    c0[0] = np.max(np.abs(u[0, :])) - 0.6
    c0[1] = np.max(np.abs(u[1, :])) - 0.4
    c0[2] = np.max(np.abs(timeScale - 1)) - 0.2
    c0[3] = -np.min(l)
    c0[4] = -np.min(n)
    c1 = np.abs(x[:, 0] - x0)
    c2 = np.abs(x[:, N] - xF)
    c3 = np.zeros((4, N))
    for i in range(N):
        if fixTime == 1:
            c3[:, i] = x[:, i + 1] - _dyn(x[:, i], u[:, i], 1.0, Ts, L)
        else:
            r = x[:, i + 1] - _dyn(x[:, i], u[:, i], timeScale[i], Ts, L)
            c3[0, i] = r[3]          # ParkingConstraints.jl:76-79: every row is stored in c3[1,i]; the last assignment wins
    if fixTime == 1:
        c5 = np.max(np.abs(np.diff(np.concatenate([[0.0], u[0, :]]))) / Ts) - 0.6
        c4 = 0.0
    else:
        c4 = np.max(np.abs(np.diff(timeScale)))
        c5 = np.max(np.abs(np.diff(np.concatenate([[0.0], u[0, :]]))) / (timeScale[0] * Ts)) - 0.6
    g, off = _geom(ego)
    c6 = np.zeros((4, N + 1))
    for i in range(N + 1):
        r0 = 0
        for j in range(nOb):
            Aj = A[r0:r0 + vOb[j]]; bj = b[r0:r0 + vOb[j]]; lj = l[r0:r0 + vOb[j], i]; nj = n[4 * j:4 * j + 4, i]
            r0 += vOb[j]
            p = Aj.T @ lj
            cs, sn = np.cos(x[2, i]), np.sin(x[2, i])
            if sd == 1:
                c6[0, i] = abs(p[0] ** 2 + p[1] ** 2) - 1
            else:
                c6[0, i] = p[0] ** 2 + p[1] ** 2 - 1
            c6[1, i] = abs(nj[0] - nj[2] + cs * p[0] + sn * p[1])
            c6[2, i] = abs(nj[1] - nj[3] - sn * p[0] + cs * p[1])
            c6[3, i] = -(-g @ nj + (x[0, i] + cs * off) * p[0] + (x[1, i] + sn * off) * p[1] - bj @ lj) + DMIN
    return [np.max(c0), np.max(c1), np.max(c2), np.max(np.abs(c3)), c4, c5, np.max(c6)]


def parking_constraints_ref(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd):
    e = [c <= 5e-5 for c in _parking_ref_classes(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd)]
    return 1 if sum(e) == 7 else 0


def parking_constraints_ref_worst(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd):
    """the largest of the quantities parking_constraints_ref compares with 5e-5 (NaN if any of them is): what the device-side check reports as `ref_worst`"""
    return float(np.max(np.array(_parking_ref_classes(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd), float)))


VIOL_NAMES = ("u_bounds", "x_bounds", "ts_bounds", "ts_chain", "dual_pos", "start", "end", "dyn", "steer_rate", "norm", "rot", "sep", "penetration", "ref_worst")
QUAD_VIOL_NAMES = ("start", "end", "u_bounds", "x_bounds", "dyn", "ts_chain", "dual_pos", "norm", "sep")


def parking_constraints_full(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sl=None):
    """max violation of each constraint class (all <= tol means feasible).  sl (nOb,N+1) is the parking slack (if None the
    obstacle row is evaluated with the best slack, i.e. the row is reported as the required slack)."""
    x0 = np.ravel(x0); xF = np.ravel(xF); vOb = [int(v) for v in np.ravel(vOb)]
    A = np.asarray(A, float).reshape(-1, 2); b = np.ravel(b); XYb = np.ravel(XYbounds)
    ts = np.ones(N + 1) if fixTime else np.ravel(timeScale)
    out = {}
    out["u_bounds"] = max(np.max(np.abs(u[0])) - 0.6, np.max(np.abs(u[1])) - 0.4)
    out["x_bounds"] = max(np.max(XYb[0] - x[0]), np.max(x[0] - XYb[1]), np.max(XYb[2] - x[1]), np.max(x[1] - XYb[3]),
                          np.max(-1 - x[3]), np.max(x[3] - 2))
    out["ts_bounds"] = max(np.max(0.8 - ts), np.max(ts - 1.2)) if not fixTime else 0.0
    out["ts_chain"] = np.max(np.abs(np.diff(ts)))
    out["dual_pos"] = max(-np.min(l), -np.min(n))
    out["start"] = np.max(np.abs(x[:, 0] - x0)); out["end"] = np.max(np.abs(x[:, N] - xF))
    out["dyn"] = max(np.max(np.abs(x[:, i + 1] - _dyn(x[:, i], u[:, i], ts[i], Ts, L))) for i in range(N))
    du = np.diff(np.concatenate([[0.0], u[0]]))
    out["steer_rate"] = np.max(np.abs(du) / (ts[:N] * Ts)) - 0.6
    g, off = _geom(ego)
    cn = ce = cd = 0.0
    need = np.zeros((nOb, N + 1))
    for i in range(N + 1):
        r0 = 0
        cs, sn = np.cos(x[2, i]), np.sin(x[2, i])
        for j in range(nOb):
            Aj = A[r0:r0 + vOb[j]]; bj = b[r0:r0 + vOb[j]]; lj = l[r0:r0 + vOb[j], i]; nj = n[4 * j:4 * j + 4, i]
            r0 += vOb[j]
            p = Aj.T @ lj
            cn = max(cn, abs(p @ p - 1))
            ce = max(ce, abs(nj[0] - nj[2] + cs * p[0] + sn * p[1]), abs(nj[1] - nj[3] - sn * p[0] + cs * p[1]))
            row = -g @ nj + (x[0, i] + cs * off) * p[0] + (x[1, i] + sn * off) * p[1] - bj @ lj
            need[j, i] = DMIN - row
            if sl is not None:
                cd = max(cd, DMIN - (row + sl[j, i]))
    out["norm"] = cn; out["rot"] = ce
    out["sep"] = cd if sl is not None else 0.0
    out["penetration"] = float(np.max(need))      # >0 : the trajectory needs positive slack somewhere (min-penetration mode)
    return out


def feasible(viol, tol=5e-5):
    return all(v <= tol for k, v in viol.items() if k != "penetration")


def validate_parking(x0, xF, N, Ts, L, ego, XYbounds, vOb, A, b, xp, up, timeScale, lp, np_, sl=None, fixTime=0, tol=5e-5, dist=False):
    """(ok, violations).  dist=False: min-penetration solution (every row with its slack, |A'lam| == 1); dist=True: collision-free
    solution (|A'lam| <= 1, separation rows without slack)."""
    nOb = len(np.ravel(vOb)); ts = np.broadcast_to(np.ravel(timeScale), (N + 1,)) if np.size(timeScale) > 1 else np.full(N + 1, float(timeScale))
    v = parking_constraints_full(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, xp, up, lp, np_, ts, fixTime,
                                 np.zeros((nOb, N + 1)) if (dist or sl is None) else sl)
    if dist:
        Am = np.asarray(A, float).reshape(-1, 2); r0 = 0; worst = 0.0
        for vj in [int(q) for q in np.ravel(vOb)]:
            p = Am[r0:r0 + vj].T @ lp[r0:r0 + vj]; worst = max(worst, float(np.max((p ** 2).sum(0) - 1))); r0 += vj
        v["norm"] = worst
    return feasible(v, tol), v


_Q = dict(mass=0.5, g=9.81, kF=0.0611, kM=0.0015, I=(3.9e-3, 4.4e-3, 4.9e-3), arm=0.225)
_QXL = np.array([0, 0, 0, -3, -0.2, -0.2, -1, -1, -1, -1.5, -1, -1.0]); _QXU = np.array([10, 10, 5, 3, 0.2, 0.2, 1, 1, 1, 3, 1, 1.0])


def validate_quadcopter(x, u, timeScale, x0, xF, Ts, lam, ob, R, tol=1e-3):
    """constrSatisfaction(x,u,timeScale,x0,xF,Ts,lambda,ob1..ob5,R): x (12,N+1), u (4,N), lam (30,N+1), ob (5,6).  Returns (ok, worst)."""
    x = np.asarray(x, float); u = np.asarray(u, float); lam = np.asarray(lam, float); ob = np.asarray(ob, float).reshape(5, 6)
    N = x.shape[1] - 1; ts = np.broadcast_to(np.ravel(timeScale), (N + 1,)); q = _Q; w = {}
    w["start"] = np.abs(x[:, 0] - np.ravel(x0)).max(); w["end"] = np.abs(x[:, -1] - np.ravel(xF)).max()
    w["u_bounds"] = max((1.2 - u).max(), (u - 7.8).max()); w["x_bounds"] = max((_QXL[:, None] - x[:, :N]).max(), (x[:, :N] - _QXU[:, None]).max())
    X = x[:, :N]; U = (u ** 2).sum(0); s4, c4, s5, c5, s6, c6 = np.sin(X[3]), np.cos(X[3]), np.sin(X[4]), np.cos(X[4]), np.sin(X[5]), np.cos(X[5])
    g0 = x[9:12, 0]                                   # x[10], x[11], x[12] with a single index = stage 1
    G = np.stack([X[6], X[7], X[8], c5 * X[9] + s5 * X[11], s5 * s4 / c4 * X[9] + X[10] - c5 * s4 / c4 * X[11], -s5 / c4 * X[9] + c5 / c4 * X[11],
                  q["kF"] / q["mass"] * U * (s4 * c5 * s6 + s5 * c6), q["kF"] / q["mass"] * U * (-s4 * c5 * c6 + s5 * s6),
                  (q["kF"] * U * c4 * c5 - q["mass"] * q["g"]) / q["mass"],
                  (q["arm"] * q["kF"] * (u[1] ** 2 - u[3] ** 2) - (q["I"][2] - q["I"][1]) * g0[1] * g0[2]) / q["I"][0],
                  (q["arm"] * q["kF"] * (u[2] ** 2 - u[0] ** 2) - (q["I"][0] - q["I"][2]) * g0[0] * g0[2]) / q["I"][1],
                  (q["kM"] * (u[0] ** 2 - u[1] ** 2 + u[2] ** 2 - u[3] ** 2) - (q["I"][1] - q["I"][0]) * g0[0] * g0[1]) / q["I"][2]])
    w["dyn"] = np.abs(x[:, 1:] - X - ts[:N] * Ts * G).max(); w["ts_chain"] = np.abs(np.diff(ts)).max()
    w["dual_pos"] = -lam.min()
    L5 = lam.reshape(5, 6, N + 1)[:, :, :N]; qv = L5[:, :3] - L5[:, 3:]
    w["norm"] = ((qv ** 2).sum(1) - 1).max()
    sep = -(ob[:, :, None] * L5).sum(1) + (x[None, :3, :N] * qv).sum(1) - R
    w["sep"] = -sep.min()
    bad = w["start"] > tol or w["end"] > tol or w["u_bounds"] > 0 or w["x_bounds"] > 0 or w["dyn"] > tol or w["ts_chain"] > tol or \
        w["dual_pos"] > tol or w["norm"] > tol or w["sep"] > tol
    return (not bad), w


# ---------------------------------------------------------------- clearance between the nodes (obca_amd/csrc/obca_clearance.h)
CLR_OUT = 24          # doubles of a record: min, min_nodes, sample, obstacle, below, samples, bad, 0, then 16 per-obstacle minima
CLR_TOUCH = 1e-7      # a parking distance below this counts as 0: "touches or overlaps"


def _stage_scale(timeScale, N):
    return np.array(np.broadcast_to(np.ravel(np.asarray(timeScale, float)), (N + 1,)), float)


def parking_samples(x, u, timeScale, Ts, L, substeps):
    """(N S + 1, 3) poses (x, y, yaw) of the samples q = k S + s of a parking trajectory x (4,N+1), u (2,N): sub-step s of interval k is the discretisation's own step
    (ParkingSignedDist.jl:147-150, `_dyn`) from node k with u_k over (s / S) timeScale[k] Ts; s = 0 and the last sample are the nodes themselves."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = x.shape[1] - 1; S = int(substeps); ts = _stage_scale(timeScale, N)
    out = np.zeros((N * S + 1, 3))
    for k in range(N):
        out[k * S] = x[:3, k]
        for s in range(1, S):
            out[k * S + s] = _dyn(x[:, k], u[:, k], s / S * ts[k], Ts, L)[:3]
    out[N * S] = x[:3, N]
    return out


def refine_parking(x, u, timeScale, Ts, L, factor, ref=None, lam=None, mu=None):
    """A parking trajectory x (4,N+1), u (2,N) on the horizon N' = r N, r = factor: the start of the same NLP on a grid of step Ts / r (obca_amd/csrc/obca_refine.h is
    the device's text of this statement).  With q = k r + s, 0 <= s < r, and q = r N the last node:
      x'[q] = x[k] at s = 0, else the discretisation's own step `_dyn` from node k with u_k over (s / r) timeScale[k] Ts -- the pose parking_samples(..., substeps=r) gives for
              sample q, so the refined NLP constrains the very poses the clearance check sampled;  x'[r N] = x[N]
      u'[q] = u[k] (zero-order hold);  Ts' = Ts / r
      ref'[q] = ref[k] + (s / r)(ref[k+1] - ref[k]) for the rows of `ref` (3,N+1: rx, ry, ryaw), ref[k] itself at s = 0
      lam'[q], mu'[q] = the columns q // r of lam (M,N+1) and mu (4nOb,N+1), the last node takes N
    timeScale: a scalar or (N+1,).  Returns dict(x (4,rN+1), u (2,rN), Ts, ref, lam, mu) -- None where nothing was given."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = x.shape[1] - 1; r = int(factor); ts = _stage_scale(timeScale, N)
    assert r >= 1 and u.shape == (2, N) and x.shape[0] == 4
    Nf = N * r; xf = np.zeros((4, Nf + 1)); uf = np.zeros((2, Nf)); k_of = np.minimum(np.arange(Nf + 1) // r, N)
    for q in range(Nf + 1):
        k, s = divmod(q, r)
        xf[:, q] = _dyn(x[:, k], u[:, k], s / r * ts[k], Ts, L) if s else x[:, k]
        if q < Nf:
            uf[:, q] = u[:, k]
    out = dict(x=xf, u=uf, Ts=Ts / r, ref=None, lam=None, mu=None)
    if ref is not None:
        ref = np.asarray(ref, float).reshape(3, N + 1); rf = np.zeros((3, Nf + 1))
        for q in range(Nf + 1):
            k, s = divmod(q, r)
            rf[:, q] = ref[:, k] + (s / r) * (ref[:, k + 1] - ref[:, k]) if s else ref[:, k]
        out["ref"] = rf
    for name, a in (("lam", lam), ("mu", mu)):
        if a is not None:
            out[name] = np.asarray(a, float)[:, k_of].copy()
    return out


def refine_quad(x, timeScale, Ts, factor, euler=True):
    """A quadcopter trajectory x (12,N+1) on the horizon N' = r N, r = factor: the warm start of the same NLP on a grid of step Ts / r (obca_amd/csrc/obca_quad_subdivide.h is
    the device's text of this statement).  With q = k r + s, 0 <= s < r, and q = r N the last node:
      x'[q] = x[k] at s = 0;  x'[r N] = x[N]
      rows 0-2 at s > 0: p_k + (s / r) timeScale[k] Ts v_k -- the point quad_clearance(..., substeps=r) gives for sample q (the discretisation is forward Euler: it is also
              the partial step), so the refined NLP constrains the very points the clearance check sampled;  euler=False: interpolated like the other rows
      rows 3-11 at s > 0: x[k] + (s / r)(x[k+1] - x[k])
    timeScale: a scalar or (N+1,).  Returns dict(x (12,rN+1), Ts = Ts / r)."""
    x = np.asarray(x, float); N = x.shape[1] - 1; r = int(factor); ts = _stage_scale(timeScale, N)
    assert r >= 1 and x.shape[0] == 12
    Nf = N * r; xf = np.zeros((12, Nf + 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Nf + 1):
            k, s = divmod(q, r)
            if not s:
                xf[:, q] = x[:, k]
                continue
            xf[:, q] = x[:, k] + (s / r) * (x[:, k + 1] - x[:, k])
            if euler:
                xf[:3, q] = x[:3, k] + s / r * ts[k] * Ts * x[6:9, k]
    return dict(x=xf, Ts=Ts / r)


def clearance_record(c, substeps, need, finite=True):
    """the record of a table c (N S + 1, nOb) of clearances: ties of the minimum go to the smallest sample, then the smallest obstacle; `below` counts the samples whose
    smallest clearance is < need.  Not finite (an input was not, or an entry of c is not): NaN / -1 / below = samples."""
    c = np.asarray(c, float); nS, nOb = c.shape; S = int(substeps)
    r = np.zeros(CLR_OUT); r[5] = nS; r[8:] = np.inf
    if not (finite and np.isfinite(c).all()):
        r[[0, 1]] = np.nan; r[[2, 3]] = -1; r[4] = nS; r[6] = 1; r[8:] = np.nan
        return r
    q, j = np.unravel_index(np.argmin(c), c.shape)      # the first minimum in row-major order: smallest sample, then smallest obstacle
    nodes = np.r_[np.arange(0, nS - 1, S), nS - 1]
    r[0] = c[q, j]; r[1] = c[nodes].min(); r[2] = q; r[3] = j; r[4] = int((c.min(axis=1) < need).sum()); r[8:8 + nOb] = c.min(axis=0)
    return r


def quad_clearance(x, timeScale, Ts, ob, R, substeps, need=0.0):
    """the clearance record of a quadcopter trajectory x (12,N+1): sample (k, s) is the point p_k + (s / S) timeScale[k] Ts v_k (QuadcopterSignedDist.jl:138-140), its
    clearance to box j (ob (5,6) as [hi; -lo]) the Euclidean distance to the box (0 inside) minus R."""
    x = np.asarray(x, float); N = x.shape[1] - 1; S = int(substeps); ts = _stage_scale(timeScale, N); ob = np.asarray(ob, float).reshape(5, 6)
    finite = bool(np.isfinite(x).all() and np.isfinite(ts).all() and np.isfinite(Ts))
    c = np.zeros((N * S + 1, 5))
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(N * S + 1):
            k, s = divmod(q, S)
            pt = x[:3, k] + s / S * ts[k] * Ts * x[6:9, k] if s else x[:3, k]
            for j in range(5):
                e = np.maximum(np.maximum(-ob[j, 3:] - pt, pt - ob[j, :3]), 0.0)
                c[q, j] = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) - R
    return clearance_record(c, S, need, finite)


# ---------------------------------------------------------------- rollout on the continuous models (obca_amd/csrc/obca_rollout.h)
ROLL_OUT = 40         # doubles of a record: bad, dev_pos, dev_node, dev_att, dev_vel, dev_rate, the same four at node N, restart, S, 4 x 0, then the CLR_OUT clearance record
_QC = dict(m=0.5, g=9.81, kF=0.0611, kM=0.0015, arm=0.225, I1=3.9e-3, I2=4.4e-3, I3=4.9e-3)      # QuadcopterSignedDist.jl:51-62 (obca_quad_model.h)


def _park_rhs(x, u, L):
    """the kinematic bicycle; u[0] is tan(delta)"""
    return [x[3] * math.cos(x[2]), x[3] * math.sin(x[2]), x[3] * u[0] / L, u[1]]


def _quad_rhs(x, u, _=None):
    """the rigid body QuadcopterSignedDist.jl:138-155 discretises, gyroscopic products at the CURRENT rates (quad::dyn_g_continuous, term by term)"""
    q = _QC; s4, c4, s5, c5, s6, c6 = math.sin(x[3]), math.cos(x[3]), math.sin(x[4]), math.cos(x[4]), math.sin(x[5]), math.cos(x[5])
    usq = u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]
    return [x[6], x[7], x[8],
            c5 * x[9] + s5 * x[11], s5 * s4 / c4 * x[9] + x[10] - c5 * s4 / c4 * x[11], -s5 / c4 * x[9] + c5 / c4 * x[11],
            q["kF"] / q["m"] * usq * (s4 * c5 * s6 + s5 * c6), q["kF"] / q["m"] * usq * (-s4 * c5 * c6 + s5 * s6), (q["kF"] * usq * c4 * c5 - q["m"] * q["g"]) / q["m"],
            (q["arm"] * q["kF"] * (u[1] * u[1] - u[3] * u[3]) - (q["I3"] - q["I2"]) * x[10] * x[11]) / q["I1"],
            (q["arm"] * q["kF"] * (u[2] * u[2] - u[0] * u[0]) - (q["I1"] - q["I3"]) * x[9] * x[11]) / q["I2"],
            (q["kM"] * (u[0] * u[0] - u[1] * u[1] + u[2] * u[2] - u[3] * u[3]) - (q["I2"] - q["I1"]) * x[9] * x[10]) / q["I3"]]


def _rk4(f, X, u, h, L):
    """one classical RK4 step, in the order of roll::rk4_step"""
    n = len(X)
    k = f(X, u, L); acc = list(k); xt = [X[i] + h / 2 * k[i] for i in range(n)]
    k = f(xt, u, L); acc = [acc[i] + 2 * k[i] for i in range(n)]; xt = [X[i] + h / 2 * k[i] for i in range(n)]
    k = f(xt, u, L); acc = [acc[i] + 2 * k[i] for i in range(n)]; xt = [X[i] + h * k[i] for i in range(n)]
    k = f(xt, u, L)
    return [X[i] + h / 6 * (acc[i] + k[i]) for i in range(n)]


def _rollout(f, prep, x, u, timeScale, Ts, L, substeps, restart, pole=None):
    x = np.asarray(x, float); u = np.asarray(u, float); nx, N1 = x.shape; N = N1 - 1; S = int(substeps); ts = _stage_scale(timeScale, N)
    X = np.zeros((nx, N + 1)); P = np.zeros((N * S + 1, 3)); X[:, 0] = x[:, 0]
    cur = [float(v) for v in x[:, 0]]; bad = False
    for k in range(N):
        if restart:
            cur = [float(v) for v in x[:, k]]
        U = prep([float(v) for v in u[:, k]]); h = float(ts[k]) * float(Ts) / S
        for s in range(S):
            P[k * S + s] = cur[:3]
            try:
                new = _rk4(f, cur, U, h, L)
                if pole is not None and math.cos(cur[pole]) * math.cos(new[pole]) <= 0.0:      # a step across the pole of the attitude kinematics: the continuous state has diverged
                    bad = True
            except (OverflowError, ValueError, ZeroDivisionError):      # (Python's math raises where C returns inf / NaN)
                new = [math.nan] * nx
            cur = new
        X[:, k + 1] = cur
    P[N * S] = x[:3, N] if restart else cur[:3]
    if bad or not np.isfinite(X).all():
        X[:] = np.nan
    return X, P


def rollout_parking(x, u, timeScale, Ts, L, substeps=8, restart=False):
    """A parking trajectory x (4,N+1), u (2,N) on the continuous kinematic bicycle x' = v cos psi, y' = v sin psi, psi' = v tan(delta) / L, v' = a: u_k held over interval k
    of length timeScale[k] Ts, classical RK4 with `substeps` equal steps per interval.  restart False: the open loop from x[:, 0] (chain); True: every interval starts at the
    solution's own node (the defect of one interval).  Returns (X (4,N+1) the rolled node states, samples (N S + 1, 3) the poses (x, y, psi) of the samples q = k S + s of
    parking_samples: the state after s steps of interval k; s = 0 and the last one are X_k (chain) or the nodes (restart))."""
    return _rollout(_park_rhs, lambda U: [math.tan(U[0]), U[1]], x, u, timeScale, Ts, float(L), substeps, restart)


def rollout_quad(x, u, timeScale, Ts, substeps=8, restart=False):
    """The same for a quadcopter trajectory x (12,N+1), u (4,N) on the rigid body that QuadcopterSignedDist.jl:138-155 steps with forward Euler (gyroscopic products at the
    current rates).  Returns (X (12,N+1), samples (N S + 1, 3) positions).  A step across cos x[3] = 0 (a pitch through pi/2: the continuous state diverges there), like
    a number that is not finite, makes all of X NaN."""
    return _rollout(_quad_rhs, lambda U: U, x, u, timeScale, Ts, None, substeps, restart, pole=3)


def quad_point_clearance(points, ob, R):
    """(n, 5) clearances of points (n, 3) to the boxes ob (5,6) as [hi; -lo]: Euclidean distance (0 inside) - R, as quad_clearance computes them"""
    ob = np.asarray(ob, float).reshape(5, 6); c = np.zeros((len(points), 5))
    with np.errstate(invalid="ignore", over="ignore"):
        for q, pt in enumerate(np.asarray(points, float)):
            for j in range(5):
                e = np.maximum(np.maximum(-ob[j, 3:] - pt, pt - ob[j, :3]), 0.0)
                c[q, j] = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) - R
    return c


def rollout_record(x, X, c, substeps, restart, need, finite=True):
    """the ROLL_OUT doubles of a rollout: x the solution (nx,N+1), X the rolled node states, c (N S + 1, nOb) the clearances of the samples.  [1] the largest position
    deviation |P(X_k) - P(x_k)|_2 over k = 1..N, [2] its node (ties: the smallest), [3] attitude (parking |d psi|; quadcopter max-abs over states 4-6), [4] velocity (parking
    |d v|; quadcopter Euclidean over states 7-9), [5] body rates (quadcopter max-abs over states 10-12; parking 0), [6..9] the same at node N, [10] restart, [11] S,
    [16..39] clearance_record(c).  Not finite (`finite` False, or a rolled state or a clearance is not): bad = 1, the real-valued fields NaN, the node -1."""
    x = np.asarray(x, float); X = np.asarray(X, float); nx = x.shape[0]; S = int(substeps)
    r = np.zeros(ROLL_OUT); r[10] = int(bool(restart)); r[11] = S
    finite = bool(finite and np.isfinite(X).all() and np.isfinite(np.asarray(c, float)).all())
    r[16:] = clearance_record(c, S, need, finite)
    if not finite:
        r[0] = 1; r[1:10] = np.nan; r[2] = -1
        return r
    e = X[:, 1:] - x[:, 1:]
    if nx == 4:
        d = np.array([np.sqrt(e[0] * e[0] + e[1] * e[1]), np.abs(e[2]), np.abs(e[3]), np.zeros(e.shape[1])])
    else:
        d = np.array([np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]), np.abs(e[3:6]).max(axis=0), np.sqrt(e[6] * e[6] + e[7] * e[7] + e[8] * e[8]), np.abs(e[9:12]).max(axis=0)])
    r[1] = d[0].max(); r[2] = 1 + int(np.argmax(d[0])); r[3:6] = d[1:].max(axis=1); r[6:10] = d[:, -1]
    return r


# ---------------------------------------------------------------- one step of the closed receding-horizon loop (obca_amd/csrc/obca_advance.h)
ADV_OUT = 40          # doubles of a record: the ROLL_OUT layout with [10] 0, [11] S, [12] shift, [13] the driven time, [14] the distance to the goal, [15] the nodes logged


def _advance(roll, nx, x, u, t, Ts, shift, substeps, x0, kick):
    x = np.asarray(x, float); shift = int(shift)
    xs = np.array(x[:, :shift + 1], float); xs[:, 0] = np.asarray(x0, float).reshape(nx)      # the chain starts at the record's X0, not at the solution's node 0
    X, P = roll(xs, np.asarray(u, float)[:, :shift], float(t), Ts, substeps)
    st = X[:, shift] + np.asarray(kick, float).reshape(nx) if kick is not None else X[:, shift].copy()
    ok = bool(np.isfinite(X).all() and np.isfinite(st).all() and np.isfinite(x[:, :shift + 1]).all() and np.isfinite(np.asarray(u, float)[:, :shift]).all()
              and np.isfinite(xs[:, 0]).all() and np.isfinite(float(t) * float(Ts)))
    return X, P, (st if ok else np.full(nx, np.nan)), ok


def advance_parking(x, u, t, Ts, L, shift, substeps=8, x0=None, kick=None):
    """The plant of one closed-loop step: _rollout (rollout_parking's chain) truncated to the first `shift` intervals of the solution x (4,N+1), u (2,N) with its one time
    scale t, started at x0 (the record's X0; None: the solution's node 0).  Returns (X (4, shift+1) the driven node states BEFORE the kick, samples (shift S + 1, 3), state
    (4,) = X[:, shift] + kick, ok); not ok (a number that is not finite among what is read or rolled): state is NaN."""
    x = np.asarray(x, float)
    return _advance(lambda a, b, c, d, e: rollout_parking(a, b, c, d, L, e, False), 4, x, u, t, Ts, shift, substeps, x[:, 0] if x0 is None else x0, kick)


def advance_quad(x, u, t, Ts, shift, substeps=8, x0=None, kick=None):
    """the same for a quadcopter solution x (12,N+1), u (4,N): rollout_quad's chain over `shift` intervals (a step across cos x[3] = 0 is not ok)"""
    x = np.asarray(x, float)
    return _advance(lambda a, b, c, d, e: rollout_quad(a, b, c, d, e, False), 12, x, u, t, Ts, shift, substeps, x[:, 0] if x0 is None else x0, kick)


def advance_record(x, X, c, state, xF, shift, substeps, need, step_time, logged=-1, ok=True):
    """the ADV_OUT doubles of a step: rollout_record of the solution's nodes 0 .. shift against the driven states X (before the kick) with the clearances c (shift S + 1,
    nOb) of the driven samples, then [10] 0, [11] S, [12] shift, [13] shift * step_time (step_time = t Ts), [14] the position distance (2 coordinates for nx = 4, else 3) of
    `state` to xF, [15] logged.  shift 0: the maxima are 0, the node -1, [6..9] compare X_0 with the solution's node 0.  No obstacle (c has no column): min and min_nodes
    +inf, sample and obstacle -1.  Not ok: as a bad rollout record, [13] and [14] NaN."""
    x = np.asarray(x, float)[:, :shift + 1]; X = np.asarray(X, float); c = np.asarray(c, float); nx = x.shape[0]; S = int(substeps); npos = 2 if nx == 4 else 3
    ok = bool(ok and np.isfinite(X).all() and np.isfinite(c).all() and np.isfinite(state).all())
    if not ok:
        r = rollout_record(x, np.full_like(X, np.nan), np.full((shift * S + 1, max(1, c.shape[1])), np.nan), S, False, need, False)
        r[13] = r[14] = np.nan
    else:
        r = np.zeros(ROLL_OUT); r[11] = S
        if c.shape[1]:
            r[16:] = clearance_record(c, S, need, True)
        else:
            r[16:] = 0.0; r[[16, 17]] = np.inf; r[[18, 19]] = -1; r[21] = shift * S + 1; r[24:] = np.inf
        xx = x if shift else np.c_[x, x]; XX = X if shift else np.c_[X, X]      # (shift 0: node 0 stands in for "node shift")
        h = rollout_record(xx, XX, np.zeros((xx.shape[1] * S - S + 1, 1)), S, False, need, True)
        r[:10] = h[:10]
        if not shift:
            r[1] = r[3] = r[4] = r[5] = 0.0; r[2] = -1
        e = np.asarray(state, float)[:npos] - np.asarray(xF, float)[:npos]
        r[13] = shift * step_time; r[14] = np.sqrt(sum(float(v) * float(v) for v in e))
    r[10] = 0; r[12] = shift; r[15] = logged
    return r


# ---------------------------------------------------------------- the obstacles of a resident batch moved and inflated in place (obca_amd/csrc/obca_scene_edit.h)
def move_obstacles_parking(A, b, vOb, motion=None, pivot=None, inflate=None):
    """One instance's unit-length rows A (M,2), b (M,) with the row counts vOb after its obstacles have moved: obstacle j = {p : A p <= b} becomes its image under
    p' = R(dth)(p - c) + c + d, then grows by m -- motion (nOb,3) = (dx, dy, dth), pivot (nOb,2) = (cx, cy), inflate (nOb,) = m; None: zeros.  Row by row, the kernel's
    operations in the kernel's order: a' = (cos a1 - sin a2, sin a1 + cos a2) where dth != 0 (else `a` itself, bit for bit), b' = ((b + (a1' (cx + dx) + a2' (cy + dy))) -
    (a1 cx + a2 cy)) + m where any of dx, dy, dth, m is not 0 (else b itself).  Returns (A', b', ok); not ok (a non-finite parameter or result): A, b are returned as
    they came, all or nothing."""
    A = np.array(A, float).reshape(-1, 2); b = np.array(b, float).ravel(); v = np.asarray(vOb, np.int64).ravel(); n = len(v)
    mo = np.zeros((n, 3)) if motion is None else np.asarray(motion, float).reshape(n, 3)
    pv = np.zeros((n, 2)) if pivot is None else np.asarray(pivot, float).reshape(n, 2)
    mg = np.zeros(n) if inflate is None else np.asarray(inflate, float).reshape(n)
    A2, b2 = A.copy(), b.copy(); r = 0
    for j in range(n):
        dx, dy, th = (float(t) for t in mo[j]); cx, cy = (float(t) for t in pv[j]); m = float(mg[j])
        rot = th != 0.0; any_ = rot or dx != 0.0 or dy != 0.0 or m != 0.0
        with np.errstate(invalid="ignore"):      # (an infinite angle: NaN, reported as not ok)
            s, c = (float(np.sin(th)), float(np.cos(th))) if rot else (0.0, 1.0)
        for _ in range(int(v[j])):
            o1, o2 = float(A[r, 0]), float(A[r, 1]); a1, a2 = o1, o2
            if rot:
                a1 = c * o1 - s * o2; a2 = s * o1 + c * o2
                A2[r] = a1, a2
            if any_:
                b2[r] = ((float(b[r]) + (a1 * (cx + dx) + a2 * (cy + dy))) - (o1 * cx + o2 * cy)) + m
            r += 1
    ok = bool(np.isfinite(mo).all() and np.isfinite(pv).all() and np.isfinite(mg).all() and np.isfinite(A2).all() and np.isfinite(b2).all())
    return (A2, b2, True) if ok else (A, b, False)


def move_obstacles_quad(ob, motion=None, inflate=None):
    """One instance's five boxes ob (5,6) = [ub(3), -lb(3)] after a motion (5,3) = (dx, dy, dz) and an inflation (5,) per box (None: zeros): word i < 3 becomes
    (ob[i] + d_i) + m, word 3 + i becomes (ob[3 + i] - d_i) + m, a word whose d_i and m are both 0 keeps its bits.  Returns (ob', ok); not ok: ob as it came."""
    ob = np.array(ob, float).reshape(5, 6)
    d = np.zeros((5, 3)) if motion is None else np.asarray(motion, float).reshape(5, 3)
    m = np.zeros(5) if inflate is None else np.asarray(inflate, float).reshape(5)
    dd = np.c_[d, -d]; mm = np.repeat(m[:, None], 6, 1)
    with np.errstate(invalid="ignore"):
        out = np.where((dd != 0.0) | (mm != 0.0), (ob + dd) + mm, ob)
    ok = bool(np.isfinite(d).all() and np.isfinite(m).all() and np.isfinite(out).all())
    return (out, True) if ok else (ob, False)


# ---------------------------------------------------------------- clearance of a held plan against obstacles that move (obca_amd/csrc/obca_predict.h)
PRD_OUT = 32          # doubles of a record: the CLR_OUT clearance record, first, t_first, first_obstacle, t_min, horizon, moving, 2 x 0


def predict_times(timeScale, Ts, N, substeps):
    """tau (N S + 1,): the time [s] at which sample q = k S + s of a trajectory is reached -- cum[0] = 0, cum[k+1] = cum[k] + timeScale[k] summed in stage order,
    tau_q = (cum[k] + (s / S) timeScale[k]) Ts, cum[k] Ts at s = 0 and for the last sample."""
    S = int(substeps); ts = _stage_scale(timeScale, N); cum = np.zeros(N + 1)
    for k in range(N):
        cum[k + 1] = cum[k] + ts[k]
    tau = np.zeros(N * S + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(N * S + 1):
            k, s = divmod(q, S)
            tau[q] = (cum[k] + (s / S) * ts[k]) * Ts if s else cum[k] * Ts
    return tau


def predict_parking(x, u, timeScale, Ts, L, vOb, A, b, rates, dist, substeps):
    """The clearance table of a parking trajectory x (4,N+1), u (2,N) against obstacles that MOVE while it is driven: rates (nOb,6) = [vx, vy, w, cx, cy, g] per obstacle.
    Sample q is the pose parking_samples gives; the scene it is measured in is the one move_obstacles_parking makes of the unit-length rows A (M,2), b (M,) with motion
    (vx, vy, w) tau_q, pivot (cx, cy) and inflation g tau_q -- "clearance() in the scene move_obstacles would have made at that time".  dist(pose, A_j, b_j): the distance
    of the car at pose (x, y, yaw) to the polygon with rows A_j, b_j (an exact polygon distance, the host build's DualMultWS); below CLR_TOUCH it counts as 0.
    Returns (c (N S + 1, nOb), tau (N S + 1,), finite); not finite (a number of the trajectory, a rate or a moved row is not): c is NaN."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = x.shape[1] - 1; S = int(substeps); ts = _stage_scale(timeScale, N)
    v = np.asarray(vOb, np.int64).ravel(); n = len(v); A = np.asarray(A, float).reshape(-1, 2); b = np.asarray(b, float).ravel(); rt = np.asarray(rates, float).reshape(n, 6)
    tau = predict_times(ts, Ts, N, S); c = np.full((N * S + 1, n), np.nan)
    if not (np.isfinite(x).all() and np.isfinite(u).all() and np.isfinite(ts).all() and np.isfinite(Ts) and np.isfinite(rt).all()):
        return c, tau, False
    poses = parking_samples(x, u, ts, Ts, L, S); r0 = np.concatenate([[0], np.cumsum(v)])
    for q in range(N * S + 1):
        with np.errstate(invalid="ignore", over="ignore"):
            A2, b2, ok = move_obstacles_parking(A, b, v, rt[:, :3] * tau[q], rt[:, 3:5], rt[:, 5] * tau[q])
        if not ok:
            return np.full_like(c, np.nan), tau, False
        for j in range(n):
            d = dist(poses[q], A2[r0[j]:r0[j + 1]], b2[r0[j]:r0[j + 1]])
            c[q, j] = 0.0 if d < CLR_TOUCH else d
    return c, tau, True


def predict_quad(x, timeScale, Ts, ob, R, rates, substeps):
    """the same for a quadcopter trajectory x (12,N+1): rates (5,4) = [vx, vy, vz, g] per box; sample q is the point quad_clearance measures, the boxes are those
    move_obstacles_quad makes of ob (5,6) with motion (vx, vy, vz) tau_q and inflation g tau_q.  Returns (c (N S + 1, 5), tau, finite)."""
    x = np.asarray(x, float); N = x.shape[1] - 1; S = int(substeps); ts = _stage_scale(timeScale, N); ob = np.asarray(ob, float).reshape(5, 6)
    rt = np.asarray(rates, float).reshape(5, 4); tau = predict_times(ts, Ts, N, S); c = np.full((N * S + 1, 5), np.nan)
    if not (np.isfinite(x).all() and np.isfinite(ts).all() and np.isfinite(Ts) and np.isfinite(rt).all()):
        return c, tau, False
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(N * S + 1):
            k, s = divmod(q, S)
            pt = x[:3, k] + s / S * ts[k] * Ts * x[6:9, k] if s else x[:3, k]
            ob2, ok = move_obstacles_quad(ob, rt[:, :3] * tau[q], rt[:, 3] * tau[q])
            if not ok:
                return np.full_like(c, np.nan), tau, False
            c[q] = quad_point_clearance(pt[None, :], ob2, R)[0]
    return c, tau, True


def predict_record(c, tau, rates, substeps, need, finite=True):
    """(record (PRD_OUT,), profile (N S + 1,)) of a table c of predicted clearances with the sample times tau: [0..23] clearance_record(c); [24] first = the first sample
    whose smallest clearance is < need (-1: none), [25] t_first = its tau (+inf: none), [26] first_obstacle = the smallest j under need at that sample (-1), [27] t_min =
    tau of sample [2], [28] horizon = tau of the last sample, [29] moving = the obstacles with a velocity, a turn rate or a growth rate that is not 0 (a pivot alone moves
    nothing), [30], [31] 0; profile = the smallest clearance of every sample.  Not finite: the bad clearance record, [24] = [26] = -1, [25] = [27] = [28] = NaN, [29] = 0,
    profile NaN."""
    c = np.asarray(c, float); tau = np.asarray(tau, float); rt = np.asarray(rates, float); r = np.zeros(PRD_OUT)
    r[:CLR_OUT] = clearance_record(c, substeps, need, finite)
    if r[6]:
        r[[24, 26]] = -1; r[[25, 27, 28]] = np.nan
        return r, np.full(c.shape[0], np.nan)
    prof = c.min(axis=1); under = np.flatnonzero(prof < need)
    if len(under):
        q = int(under[0]); r[24] = q; r[25] = tau[q]; r[26] = int(np.flatnonzero(c[q] < need)[0])
    else:
        r[24] = r[26] = -1; r[25] = np.inf
    r[27] = tau[int(r[2])]; r[28] = tau[-1]
    r[29] = int((np.delete(rt, [3, 4], axis=1) != 0).any(axis=1).sum()) if rt.shape[1] == 6 else int((rt != 0).any(axis=1).sum())
    return r, prof


# ---------------------------------------------------------------- closed-loop rollout: TVLQR gains about a trajectory (obca_amd/csrc/obca_track.h)
TRK_OUT = 48          # doubles of a record: the ROLL_OUT doubles of the chain, feedback, clamp, saturated, du_max, du_node, dx0_pos, 2 x 0
# Default weights: the values the first prototype ran with.  UNTUNED.
TRACK_Q_PARKING = (10.0, 10.0, 10.0, 1.0); TRACK_R_PARKING = (1.0, 1.0); TRACK_QF_PARKING = tuple(10.0 * v for v in TRACK_Q_PARKING)
TRACK_Q_QUAD = (10.0, 10.0, 10.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.1, 0.1, 0.1); TRACK_R_QUAD = (0.1, 0.1, 0.1, 0.1); TRACK_QF_QUAD = tuple(10.0 * v for v in TRACK_Q_QUAD)
_PARK_UBOX = ((-0.6, 0.6), (-0.4, 0.4)); _QUAD_UBOX = ((1.2, 7.8),) * 4      # the NLP's own input bounds (OB_UL0 .. OB_UU1; Q_ULO, Q_UHI)


def _park_jvp(x, u, dx, du, L):
    """the tangent of _park_rhs along (dx, du): ParkModel::jvp, term by term.  dx, du: one row per component, a row holds all directions"""
    sn, cs = math.sin(x[2]), math.cos(x[2])
    return [dx[3] * cs - x[3] * sn * dx[2], dx[3] * sn + x[3] * cs * dx[2], (dx[3] * u[0] + x[3] * du[0]) / L, du[1] + 0.0]


def _quad_jvp(x, u, dx, du, _=None):
    """the tangent of _quad_rhs along (dx, du): quad::dyn_g_continuous_jvp, term by term"""
    q = _QC; s4, c4, s5, c5, s6, c6 = math.sin(x[3]), math.cos(x[3]), math.sin(x[4]), math.cos(x[4]), math.sin(x[5]), math.cos(x[5])
    usq = u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]
    dusq = 2.0 * (u[0] * du[0] + u[1] * du[1] + u[2] * du[2] + u[3] * du[3])
    tn = s4 / c4; sc = 1.0 / (c4 * c4); a = q["kF"] / q["m"]
    return [dx[6] + 0.0, dx[7] + 0.0, dx[8] + 0.0,
            (c5 * x[11] - s5 * x[9]) * dx[4] + c5 * dx[9] + s5 * dx[11],
            (s5 * x[9] - c5 * x[11]) * sc * dx[3] + (c5 * x[9] + s5 * x[11]) * tn * dx[4] + s5 * tn * dx[9] + dx[10] - c5 * tn * dx[11],
            (c5 * x[11] - s5 * x[9]) * tn / c4 * dx[3] - (c5 * x[9] + s5 * x[11]) / c4 * dx[4] - s5 / c4 * dx[9] + c5 / c4 * dx[11],
            a * (dusq * (s4 * c5 * s6 + s5 * c6) + usq * (c4 * c5 * s6 * dx[3] + (c5 * c6 - s4 * s5 * s6) * dx[4] + (s4 * c5 * c6 - s5 * s6) * dx[5])),
            a * (dusq * (s5 * s6 - s4 * c5 * c6) + usq * ((s4 * s5 * c6 + c5 * s6) * dx[4] - c4 * c5 * c6 * dx[3] + (s4 * c5 * s6 + s5 * c6) * dx[5])),
            a * (dusq * c4 * c5 - usq * (s4 * c5 * dx[3] + c4 * s5 * dx[4])),
            (q["arm"] * q["kF"] * 2.0 * (u[1] * du[1] - u[3] * du[3]) - (q["I3"] - q["I2"]) * (dx[10] * x[11] + x[10] * dx[11])) / q["I1"],
            (q["arm"] * q["kF"] * 2.0 * (u[2] * du[2] - u[0] * du[0]) - (q["I1"] - q["I3"]) * (dx[9] * x[11] + x[9] * dx[11])) / q["I2"],
            (q["kM"] * 2.0 * (u[0] * du[0] - u[1] * du[1] + u[2] * du[2] - u[3] * du[3]) - (q["I2"] - q["I1"]) * (dx[9] * x[10] + x[9] * dx[10])) / q["I3"]]


def _rk4_tan(f, jvp, X, T, u, du, h, L):
    """one classical RK4 step with its tangent, in the order of trk::rk4_step_tan"""
    n = len(X)
    k = f(X, u, L); dk = jvp(X, u, T, du, L); acc = list(k); dacc = list(dk)
    xt = [X[i] + h / 2 * k[i] for i in range(n)]; dxt = [T[i] + h / 2 * dk[i] for i in range(n)]
    k = f(xt, u, L); dk = jvp(xt, u, dxt, du, L); acc = [acc[i] + 2 * k[i] for i in range(n)]; dacc = [dacc[i] + 2 * dk[i] for i in range(n)]
    xt = [X[i] + h / 2 * k[i] for i in range(n)]; dxt = [T[i] + h / 2 * dk[i] for i in range(n)]
    k = f(xt, u, L); dk = jvp(xt, u, dxt, du, L); acc = [acc[i] + 2 * k[i] for i in range(n)]; dacc = [dacc[i] + 2 * dk[i] for i in range(n)]
    xt = [X[i] + h * k[i] for i in range(n)]; dxt = [T[i] + h * dk[i] for i in range(n)]
    k = f(xt, u, L); dk = jvp(xt, u, dxt, du, L)
    return [X[i] + h / 6 * (acc[i] + k[i]) for i in range(n)], [T[i] + h / 6 * (dacc[i] + dk[i]) for i in range(n)]


def _linearise(f, jvp, parking, x, u, timeScale, Ts, L, substeps):
    """[A_k | B_k] (N, nx, nx + nu): the derivative of the interval map (S RK4 steps of h_k / S, the input held) at (x_k, u_k), by forward-mode tangents through the steps"""
    x = np.asarray(x, float); u = np.asarray(u, float); nx, N1 = x.shape; N = N1 - 1; nu = u.shape[0]; nd = nx + nu; S = int(substeps); ts = _stage_scale(timeScale, N)
    AB = np.zeros((N, nx, nd))
    for k in range(N):
        X = [float(v) for v in x[:, k]]; U = [float(v) for v in u[:, k]]; E = np.eye(nd)
        T = [E[i].copy() for i in range(nx)]; dU = [E[nx + a].copy() for a in range(nu)]
        try:
            if parking:      # prep: tan(delta) once per interval, and its tangent 1 + tan^2
                U[0] = math.tan(U[0]); dU[0] = (1.0 + U[0] * U[0]) * dU[0]
            h = float(ts[k]) * float(Ts) / S
            for _ in range(S):
                X, T = _rk4_tan(f, jvp, X, T, U, dU, h, L)
            AB[k] = np.array(T)
        except (OverflowError, ValueError, ZeroDivisionError):      # (Python's math raises where C returns inf / NaN)
            AB[k] = np.nan
    return AB


def _riccati(AB, nx, q, r, qf):
    """K (N, nu, nx), P_0 and whether every pivot was finite and positive: P_N = diag(qf); G = diag(r) + B'PB = C C' (unpivoted), K_k = -G^-1 B'PA,
    P <- diag(q) + A'PA + (B'PA)' K_k, P <- (P + P') / 2"""
    N, _, nd = AB.shape; nu = nd - nx; P = np.diag(np.asarray(qf, float)); K = np.zeros((N, nu, nx)); ok = True
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(N - 1, -1, -1):
            M = AB[k].T @ (P @ AB[k]); H = M[nx:, :nx]; C = np.zeros((nu, nu))
            for a in range(nu):
                for c in range(a + 1):
                    s = M[nx + a, nx + c] + (r[a] if a == c else 0.0)
                    for t in range(c):
                        s = s - C[a, t] * C[c, t]
                    if a == c:
                        ok = ok and bool(s > 0.0 and np.isfinite(s)); C[a, a] = np.sqrt(s)
                    else:
                        C[a, c] = s / C[c, c]
            y = [None] * nu
            for a in range(nu):
                s = H[a].copy()
                for t in range(a):
                    s = s - C[a, t] * y[t]
                y[a] = s / C[a, a]
            for a in range(nu - 1, -1, -1):
                s = y[a]
                for t in range(a + 1, nu):
                    s = s - C[t, a] * y[t]
                y[a] = s / C[a, a]
            K[k] = -np.array(y)
            Pn = (np.diag(np.asarray(q, float)) + M[:nx, :nx]) + H.T @ K[k]
            P = 0.5 * (Pn + Pn.T)
    if not ok:
        K[:] = np.nan
    return K, P, ok


def _weights(nx, Q, R, Qf):
    park = nx == 4
    q = np.asarray(TRACK_Q_PARKING if park else TRACK_Q_QUAD, float) if Q is None else np.broadcast_to(np.asarray(Q, float), (nx,)).copy()
    nu = 2 if park else 4
    r = np.asarray(TRACK_R_PARKING if park else TRACK_R_QUAD, float) if R is None else np.broadcast_to(np.asarray(R, float), (nu,)).copy()
    qf = 10.0 * q if Qf is None else np.broadcast_to(np.asarray(Qf, float), (nx,)).copy()
    return q, r, qf


def track_gains_parking(x, u, timeScale, Ts, L, substeps=8, Q=None, R=None, Qf=None):
    """Time-varying LQR gains about a parking trajectory x (4,N+1), u (2,N): (A (N,4,4), B (N,4,2), K (N,2,4), P_0 (4,4)).  A_k, B_k are the derivatives of the map the
    plant applies over interval k -- `substeps` RK4 steps of the bicycle with the input held, rollout_parking's step -- at (x_k, u_k), with respect to the state and to
    (delta, a) (the steering column carries sec^2 delta); K from the backward Riccati recursion with diagonal weights Q (4), R (2), Qf (4) (defaults TRACK_*_PARKING).
    Convention: u = u_k + K_k (X_k - x_k).  K is NaN if a pivot of R + B'PB was not finite and positive."""
    q, r, qf = _weights(4, Q, R, Qf)
    AB = _linearise(_park_rhs, _park_jvp, True, x, u, timeScale, Ts, float(L), substeps)
    K, P0, _ = _riccati(AB, 4, q, r, qf)
    return AB[:, :, :4].copy(), AB[:, :, 4:].copy(), K, P0


def track_gains_quad(x, u, timeScale, Ts, substeps=8, Q=None, R=None, Qf=None):
    """The same about a quadcopter trajectory x (12,N+1), u (4,N): (A (N,12,12), B (N,12,4), K (N,4,12), P_0), defaults TRACK_*_QUAD.
    Gains from the NLP's own node linearisation A = I + h f_x, B = h f_u (forward Euler) are NOT offered: the feedback is held over the interval, 0.5 s on the fixture of
    make_quad_batch(4, 20), and the attitude loop those gains close is much faster than that -- held over the interval map they make the closed loop of all four fixture
    instances leave every bound within the horizon (non-finite states), while the gains of the interval map itself track all seven fixture trajectories."""
    q, r, qf = _weights(12, Q, R, Qf)
    AB = _linearise(_quad_rhs, _quad_jvp, False, x, u, timeScale, Ts, None, substeps)
    K, P0, _ = _riccati(AB, 12, q, r, qf)
    return AB[:, :, :12].copy(), AB[:, :, 12:].copy(), K, P0


def _track(f, parking, x, u, timeScale, Ts, L, substeps, K, dx0, feedback, clamp, pole=None):
    """the chain of _rollout with the input formed per interval: X_0 = x_0 + dx0, U_k = u_k + K_k (X_k - x_k) if feedback, clipped to the input box if clamp"""
    x = np.asarray(x, float); u = np.asarray(u, float); nx, N1 = x.shape; N = N1 - 1; nu = u.shape[0]; S = int(substeps); ts = _stage_scale(timeScale, N)
    box = _PARK_UBOX if parking else _QUAD_UBOX
    X = np.zeros((nx, N + 1)); P = np.zeros((N * S + 1, 3)); Ua = np.zeros((nu, N)); clipped = np.zeros(N, bool)
    cur = [float(v) for v in x[:, 0]]; bad = False
    if dx0 is not None:
        cur = [cur[i] + float(dx0[i]) for i in range(nx)]
    X[:, 0] = cur
    for k in range(N):
        U = [float(v) for v in u[:, k]]
        if feedback:
            e = [cur[j] - float(x[j, k]) for j in range(nx)]
            for a in range(nu):
                s = 0.0
                for j in range(nx):
                    s = s + float(K[k, a, j]) * e[j]
                U[a] = U[a] + s
        if clamp:
            for a in range(nu):
                c = box[a][0] if U[a] < box[a][0] else (box[a][1] if U[a] > box[a][1] else U[a])
                clipped[k] |= c != U[a]
                U[a] = c
        Ua[:, k] = U
        h = float(ts[k]) * float(Ts) / S
        try:
            if parking:
                U = [math.tan(U[0]), U[1]]
        except (OverflowError, ValueError):
            U = [math.nan, U[1]]
        for s_ in range(S):
            P[k * S + s_] = cur[:3]
            try:
                new = _rk4(f, cur, U, h, L)
                if pole is not None and math.cos(cur[pole]) * math.cos(new[pole]) <= 0.0:
                    bad = True
            except (OverflowError, ValueError, ZeroDivisionError):
                new = [math.nan] * nx
            cur = new
        X[:, k + 1] = cur
    P[N * S] = cur[:3]
    if bad or not np.isfinite(X).all():
        X[:] = np.nan
    return X, P, Ua, clipped


def _track_model(parking, x, u, timeScale, Ts, L, substeps, dx0, Q, R, Qf, feedback, clamp):
    x = np.asarray(x, float); u = np.asarray(u, float); nx = x.shape[0]
    q, r, qf = _weights(nx, Q, R, Qf)
    AB = _linearise(_park_rhs if parking else _quad_rhs, _park_jvp if parking else _quad_jvp, parking, x, u, timeScale, Ts, L, substeps)
    K, P0, ok = _riccati(AB, nx, q, r, qf)
    ok = ok and (dx0 is None or bool(np.isfinite(np.asarray(dx0, float)).all()))
    if ok:
        X, P, Ua, clipped = _track(_park_rhs if parking else _quad_rhs, parking, x, u, timeScale, Ts, L, substeps, K, dx0, feedback, clamp, None if parking else 3)
        ok = bool(np.isfinite(X).all())
    if not ok:
        N = u.shape[1]
        X = np.full(x.shape, np.nan); P = np.full((N * int(substeps) + 1, 3), np.nan); Ua = np.full(u.shape, np.nan); clipped = np.zeros(N, bool); K = np.full(K.shape, np.nan)
    return X, P, dict(AB=AB, K=K, P0=P0, U=Ua, clipped=clipped, feedback=bool(feedback), clamp=bool(clamp), dx0=None if dx0 is None else np.asarray(dx0, float), finite=ok)


def track_parking(x, u, timeScale, Ts, L, substeps=8, dx0=None, Q=None, R=None, Qf=None, feedback=True, clamp=True):
    """A parking trajectory tracked on the continuous bicycle by the held TVLQR feedback of track_gains_parking: X_0 = x[:, 0] + dx0, per interval
    U_k = u_k + K_k (X_k - x_k) (feedback), clipped to |delta| <= 0.6, |a| <= 0.4 (clamp), X_{k+1} = `substeps` RK4 steps from X_k with U_k held.  The feedback is
    evaluated at the nodes and held; state differences are raw, no angle is wrapped.  Returns (X (4,N+1), samples (N S + 1, 3) as rollout_parking, info): info has AB
    (N,4,6), K, P0, U (2,N) the applied inputs, clipped (N,) bool, feedback, clamp, dx0, finite.  Not finite (a number that is not finite, a bad pivot): X, samples, U, K NaN."""
    return _track_model(True, x, u, timeScale, Ts, float(L), substeps, dx0, Q, R, Qf, feedback, clamp)


def track_quad(x, u, timeScale, Ts, substeps=8, dx0=None, Q=None, R=None, Qf=None, feedback=True, clamp=True):
    """The same for a quadcopter trajectory on the rigid body of rollout_quad, rotor speeds clipped to 1.2 .. 7.8.  A step across cos x[3] = 0 counts as not finite."""
    return _track_model(False, x, u, timeScale, Ts, None, substeps, dx0, Q, R, Qf, feedback, clamp)


def track_record(x, u, X, c, substeps, need, info):
    """the TRK_OUT doubles of a tracked trajectory: [0..39] rollout_record of the chain (x the trajectory, X the tracked node states, c (N S + 1, nOb) the clearances of the
    samples), [40] feedback, [41] clamp, [42] the number of intervals in which an input was clipped, [43] the largest |U_k - u_k| over inputs and intervals, [44] its interval
    (ties: the smallest), [45] |dx0| of the position part, [46], [47] 0.  Not finite: [42] = [44] = -1, [43] = [45] = NaN."""
    x = np.asarray(x, float); u = np.asarray(u, float); nx = x.shape[0]
    r = np.zeros(TRK_OUT); r[40] = int(info["feedback"]); r[41] = int(info["clamp"])
    finite = bool(info["finite"] and np.isfinite(np.asarray(c, float)).all())
    r[:ROLL_OUT] = rollout_record(x, X, c, substeps, False, need, finite)
    if not finite:
        r[42] = r[44] = -1; r[43] = r[45] = np.nan
        return r
    d = np.abs(info["U"] - u).max(axis=0)
    r[42] = int(info["clipped"].sum()); r[43] = d.max(); r[44] = int(np.argmax(d))
    if info["dx0"] is not None:
        p = info["dx0"][:2 if nx == 4 else 3]
        r[45] = np.sqrt(p[0] * p[0] + p[1] * p[1]) if nx == 4 else np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    return r


# ---------------------------------------------------------------- closed-loop ensemble: disturbed tracked rollouts about one trajectory (obca_amd/csrc/obca_ensemble.h)
ENS_MEM = 16          # doubles of a member record: bad, dev_pos, its node, end_pos, dev_att, dev_vel, dev_rate, min, its sample, its obstacle, below, saturated, du_max, its interval, dx0_pos, 0
ENS_OUT = 32          # doubles of an instance record: see ensemble_record
ENS_MMAX = 64         # most members: one per lane


def _ensemble_biased(f, parking, x, u, timeScale, Ts, L, substeps, K, dx0, dub, feedback, clamp, pole=None):
    """_track with a constant input bias, in the order of ens::member: commanded U_k = u_k + K_k (X_k - x_k) if feedback; applied U_k = commanded + dub, clipped if clamp"""
    x = np.asarray(x, float); u = np.asarray(u, float); nx, N1 = x.shape; N = N1 - 1; nu = u.shape[0]; S = int(substeps); ts = _stage_scale(timeScale, N)
    box = _PARK_UBOX if parking else _QUAD_UBOX
    X = np.zeros((nx, N + 1)); P = np.zeros((N * S + 1, 3)); Ua = np.zeros((nu, N)); clipped = np.zeros(N, bool)
    cur = [float(x[i, 0]) + float(dx0[i]) for i in range(nx)]; bad = False
    X[:, 0] = cur
    for k in range(N):
        U = [float(v) for v in u[:, k]]
        if feedback:
            e = [cur[j] - float(x[j, k]) for j in range(nx)]
            for a in range(nu):
                s = 0.0
                for j in range(nx):
                    s = s + float(K[k, a, j]) * e[j]
                U[a] = U[a] + s
        for a in range(nu):
            U[a] = U[a] + float(dub[a])
            if clamp:
                c = box[a][0] if U[a] < box[a][0] else (box[a][1] if U[a] > box[a][1] else U[a])
                clipped[k] |= c != U[a]
                U[a] = c
        Ua[:, k] = U
        h = float(ts[k]) * float(Ts) / S
        try:
            if parking:
                U = [math.tan(U[0]), U[1]]
        except (OverflowError, ValueError):
            U = [math.nan, U[1]]
        for s_ in range(S):
            P[k * S + s_] = cur[:3]
            try:
                new = _rk4(f, cur, U, h, L)
                if pole is not None and math.cos(cur[pole]) * math.cos(new[pole]) <= 0.0:
                    bad = True
            except (OverflowError, ValueError, ZeroDivisionError):
                new = [math.nan] * nx
            cur = new
        X[:, k + 1] = cur
    P[N * S] = cur[:3]
    if bad or not np.isfinite(X).all():
        X[:] = np.nan
    return X, P, Ua, clipped


def _ensemble_model(parking, x, u, timeScale, Ts, L, members, substeps, dx0, dub, Q, R, Qf, feedback, clamp):
    x = np.asarray(x, float); u = np.asarray(u, float); nx = x.shape[0]; nu = u.shape[0]; N = u.shape[1]; M = int(members); S = int(substeps)
    if not 1 <= M <= ENS_MMAX:
        raise ValueError("need 1 <= members <= 64")
    dx0 = np.zeros((M, nx)) if dx0 is None else np.asarray(dx0, float).reshape(M, nx)
    dub = np.zeros((M, nu)) if dub is None else np.asarray(dub, float).reshape(M, nu)
    f, jvp = (_park_rhs, _park_jvp) if parking else (_quad_rhs, _quad_jvp)
    q, r, qf = _weights(nx, Q, R, Qf)
    AB = _linearise(f, jvp, parking, x, u, timeScale, Ts, L, S)
    K, _, ok = _riccati(AB, nx, q, r, qf)
    ok = bool(ok and np.isfinite(x).all() and np.isfinite(u).all() and np.isfinite(_stage_scale(timeScale, N)).all() and np.isfinite(Ts))
    out = []
    for m in range(M):
        if not ok:
            X = np.full(x.shape, np.nan); P = np.full((N * S + 1, 3), np.nan)
            info = dict(AB=AB, K=np.full(K.shape, np.nan), U=np.full(u.shape, np.nan), clipped=np.zeros(N, bool), feedback=bool(feedback), clamp=bool(clamp), dx0=dx0[m], finite=False)
        elif not np.any(dub[m]):      # a zero bias: the track statement itself, with this member's offset
            X, P, info = (track_parking(x, u, timeScale, Ts, L, S, dx0[m], Q, R, Qf, feedback, clamp) if parking
                          else track_quad(x, u, timeScale, Ts, S, dx0[m], Q, R, Qf, feedback, clamp))
        else:
            fin = bool(np.isfinite(dx0[m]).all() and np.isfinite(dub[m]).all())
            if fin:
                X, P, Ua, clipped = _ensemble_biased(f, parking, x, u, timeScale, Ts, L, S, K, dx0[m], dub[m], feedback, clamp, None if parking else 3)
                fin = bool(np.isfinite(X).all())
            if not fin:
                X = np.full(x.shape, np.nan); P = np.full((N * S + 1, 3), np.nan); Ua = np.full(u.shape, np.nan); clipped = np.zeros(N, bool)
            info = dict(AB=AB, K=K, U=Ua, clipped=clipped, feedback=bool(feedback), clamp=bool(clamp), dx0=dx0[m], finite=fin)
        out.append((X, P, info))
    return out, ok


def ensemble_parking(x, u, timeScale, Ts, L, members, substeps=8, dx0=None, dub=None, Q=None, R=None, Qf=None, feedback=True, clamp=True):
    """`members` (1 .. 64) closed loops about a parking trajectory x (4,N+1), u (2,N): member m starts at x[:, 0] + dx0[m] (dx0 (M,4) or None = zeros) and applies
    clip(u_k + K_k (X_k - x_k) + dub[m]) (dub (M,2) a constant input bias per member, or None = zeros).  With a zero dub[m] member m IS track_parking with dx0[m]; a
    non-zero bias is restated beside it (_ensemble_biased).  Returns (list of (X (4,N+1), samples (N S + 1, 3), info) per member as track_parking returns them, instance_ok):
    instance_ok False -- a non-finite number in the trajectory, Ts or the time scale, or a bad Riccati pivot -- makes every member not finite."""
    return _ensemble_model(True, x, u, timeScale, Ts, float(L), members, substeps, dx0, dub, Q, R, Qf, feedback, clamp)


def ensemble_quad(x, u, timeScale, Ts, members, substeps=8, dx0=None, dub=None, Q=None, R=None, Qf=None, feedback=True, clamp=True):
    """The same about a quadcopter trajectory x (12,N+1), u (4,N): dx0 (M,12), dub (M,4), track_quad for a zero bias."""
    return _ensemble_model(False, x, u, timeScale, Ts, None, members, substeps, dx0, dub, Q, R, Qf, feedback, clamp)


def ensemble_member_record(x, u, X, c, substeps, need, info):
    """the ENS_MEM doubles of one member from what track_record makes of it (c (N S + 1, nOb) the clearances of its samples): [0] bad, [1] dev_pos, [2] its node, [3] end_pos,
    [4] dev_att, [5] dev_vel, [6] dev_rate, [7] min, [8] its sample, [9] its obstacle, [10] below, [11] saturated, [12] du_max, [13] its interval, [14] dx0_pos, [15] 0.
    Not finite: real fields NaN, indices and counts -1."""
    t = track_record(x, u, X, c, substeps, need, info)
    if t[0] != 0:
        return np.array([1, np.nan, -1, np.nan, np.nan, np.nan, np.nan, np.nan, -1, -1, -1, -1, np.nan, -1, np.nan, 0])
    return np.array([0, t[1], t[2], t[6], t[3], t[4], t[5], t[16], t[18], t[19], t[20], t[42], t[43], t[44], t[45], 0])


def ensemble_record(mem, substeps, feedback, clamp, instance_ok=True):
    """the ENS_OUT doubles of an instance from its member records (M, ENS_MEM), walked in ascending member order as ens::ensemble_reduce walks them: [0] bad, [1] M, [2] S,
    [3] feedback, [4] clamp, [5] members_bad, [6] members_hit (good members with a sample under need), [7] members_sat, [8] min over the good members, [9] its member,
    [10] its sample, [11] its obstacle, [12] dev_pos max, [13] its member, [14] its node, [15] end_pos max, [16] its member, [17] dev_att, [18] dev_vel, [19] dev_rate,
    [20] du_max, [21] its member, [22] its interval, [23] mean of end_pos, [24] mean of min, [25] below summed, [26..31] 0.  Ties go to the smaller member; bad members
    enter nothing.  instance_ok False: counts -1; no good member: real fields NaN, indices -1."""
    mem = np.asarray(mem, float).reshape(-1, ENS_MEM); M = len(mem)
    r = np.zeros(ENS_OUT); r[0] = 0 if instance_ok else 1; r[1] = M; r[2] = int(substeps); r[3] = int(bool(feedback)); r[4] = int(bool(clamp))
    good = [m for m in range(M) if mem[m, 0] == 0]
    r[5] = M - len(good); r[6] = sum(1 for m in good if mem[m, 10] > 0); r[7] = sum(1 for m in good if mem[m, 11] > 0); r[25] = sum(mem[m, 10] for m in good)
    if not instance_ok:
        r[[5, 6, 7, 25]] = -1
    if not instance_ok or not good:
        r[[8, 12, 15, 17, 18, 19, 20, 23, 24]] = np.nan; r[[9, 10, 11, 13, 14, 16, 21, 22]] = -1
        return r
    g = mem[good]
    a = int(np.argmin(g[:, 7])); r[8:12] = [g[a, 7], good[a], g[a, 8], g[a, 9]]      # (argmin / argmax: the first, the smaller member)
    a = int(np.argmax(g[:, 1])); r[12:15] = [g[a, 1], good[a], g[a, 2]]
    a = int(np.argmax(g[:, 3])); r[15:17] = [g[a, 3], good[a]]
    r[17:20] = g[:, 4:7].max(axis=0)
    a = int(np.argmax(g[:, 12])); r[20:23] = [g[a, 12], good[a], g[a, 13]]
    se = sm = 0.0
    for m in good:      # one sum in ascending member order, as the kernel text adds
        se = se + mem[m, 3]; sm = sm + mem[m, 7]
    r[23] = se / len(good); r[24] = sm / len(good)
    return r


# ---------------------------------------------------------------- clearance certified along the whole path (obca_amd/csrc/obca_certify.h)
CERT_OUT = 16         # doubles of a record: see certify_record
CERT_TICKS = 4096     # G: an interval is tau = h_k m / G, m = 0 .. G


def certify_lipschitz_parking(xk, uk, h, L, ego):
    """Lambda of one parking interval [m per unit tau]: no point of the car moves faster along park_step from node xk (4,) with uk (2,) over tau in [0, h].  With v = xk[3],
    a = uk[1], tn = |tan uk[0]|: V = max(|v|, |v + h a|), Sm = max(|v|, |v + h a / 2|), rho the car point farthest from the reference point;
    Lambda = V + |h| Sm |v| tn / (2 L) + rho V tn / L (|d(X, Y) / dtau| <= the first two terms, rho |dpsi / dtau| <= the third)."""
    g, off = _geom(ego)
    a0 = abs(off) + g[0]; rho = np.sqrt(a0 * a0 + g[1] * g[1])
    v = float(xk[3]); av = abs(v); tn = abs(np.tan(float(uk[0]))); ha = h * float(uk[1])
    V = max(av, abs(v + ha)); Sm = max(av, abs(v + ha / 2))
    return (V + abs(h) * Sm * av * tn / (2 * L)) + rho * V * tn / L


def certify_lipschitz_quad(xk):
    """Lambda of one quadcopter interval: |v_k|, the Euclidean norm of xk[6:9]"""
    return float(np.sqrt((xk[6] * xk[6] + xk[7] * xk[7]) + xk[8] * xk[8]))


def _certify_walk(clear, Lh, need, slack, max_steps):
    """conservative advancement of one (interval, obstacle) item: clear(m) is the clearance at tick m, Lh = Lambda |h|.  Returns (lb, seen, tick of seen, tick of the first
    violation or G, samples): every sample c proves c - Lh dm / G on the dm ticks it advances by; an item still running after max_steps samples has lb = -inf."""
    G = CERT_TICKS; m = 0; lb = seen = np.inf; tseen = 0; tviol = G; steps = 0
    while True:
        c = float(clear(m)); steps += 1
        if not np.isfinite(c):
            return np.nan, np.nan, -1, -1, steps
        rem = G - m
        if c < need and tviol == G:
            tviol = m
        if c < seen:
            seen, tseen = c, m
        e = (c - need) + slack if c >= need else slack
        if Lh == 0.0 or e >= Lh * rem / G:
            dm = rem
        else:
            f = math.floor(G * e / Lh)
            dm = min(f, rem) if f >= 1 else 1
        lb = min(lb, c - Lh * dm / G)
        m += dm
        if m == G:
            return lb, seen, tseen, tviol, steps
        if steps == max_steps:
            return -np.inf, seen, tseen, tviol, steps


def certify_parking(x, u, timeScale, Ts, L, ego, nOb, dist, need=DMIN, slack=0.01, max_steps=CERT_TICKS):
    """The item table of a parking trajectory x (4,N+1), u (2,N): items (N+1, nOb, 5) = (lb, seen, tick of seen, tick of the first violation or G, samples) per
    (interval, obstacle) -- interval N is node N, one sample --, and lam (N,) the Lambda_k.  dist(pose, j): the distance of the car at pose (x, y, yaw) to obstacle j (the
    oracle's DualMultWS, an exact polygon distance, the host build's own); below CLR_TOUCH it counts as 0.  The pose at tick m of interval k is `_dyn` from node k with u_k
    over (m / G) timeScale[k] of Ts, the node itself at m = 0."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = x.shape[1] - 1; ts = _stage_scale(timeScale, N); G = CERT_TICKS
    items = np.zeros((N + 1, nOb, 5)); lam = np.zeros(N)
    for k in range(N + 1):
        Lh = 0.0
        if k < N:
            h = ts[k] * Ts
            lam[k] = certify_lipschitz_parking(x[:, k], u[:, k], h, L, ego); Lh = lam[k] * abs(h)
        for j in range(nOb):
            def clear(m, k=k, j=j):
                pose = _dyn(x[:, k], u[:, k], m / G * ts[k], Ts, L)[:3] if m else x[:3, k]
                d = dist(pose, j)
                return 0.0 if d < CLR_TOUCH else d
            items[k, j] = _certify_walk(clear, Lh, need, slack, max_steps) if np.isfinite(Lh) else (np.nan, np.nan, -1, -1, 0)
    return items, lam


def certify_quad(x, timeScale, Ts, ob, R, need=0.0, slack=0.01, max_steps=CERT_TICKS):
    """the same for a quadcopter trajectory x (12,N+1): the point at tick m of interval k is p_k + (m / G) timeScale[k] Ts v_k, its clearance to box j (ob (5,6) as [hi; -lo])
    the Euclidean distance to the box (0 inside) minus R.  Returns items (N+1, 5, 5), lam (N,)."""
    x = np.asarray(x, float); N = x.shape[1] - 1; ts = _stage_scale(timeScale, N); ob = np.asarray(ob, float).reshape(5, 6); G = CERT_TICKS
    items = np.zeros((N + 1, 5, 5)); lam = np.zeros(N)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(N + 1):
            Lh = 0.0
            if k < N:
                lam[k] = certify_lipschitz_quad(x[:, k]); Lh = lam[k] * abs(ts[k] * Ts)
            for j in range(5):
                def clear(m, k=k, j=j):
                    pt = x[:3, k] + m / G * ts[k] * Ts * x[6:9, k] if m else x[:3, k]
                    e = np.maximum(np.maximum(-ob[j, 3:] - pt, pt - ob[j, :3]), 0.0)
                    return np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) - R
                items[k, j] = _certify_walk(clear, Lh, need, slack, max_steps) if np.isfinite(Lh) else (np.nan, np.nan, -1, -1, 0)
    return items, lam


def certify_record(items, lam, finite=True):
    """(record (CERT_OUT,), intervals (N+1, 2)) of an item table: intervals[k] = (the smallest lb, the smallest seen) over the obstacles.  Record: [0] lb, [1] seen, [2-4]
    interval, tick, obstacle of seen (ties: the smallest interval, then tick, then obstacle), [5] violated = intervals with a sample under need (node N counts as one), [6-8]
    interval, tick, obstacle of the first violation in that order (-1: none), [9] undecided items, [10] samples taken, [11] most samples of one item, [12] the largest
    Lambda_k, [13] certified, [14] bad, [15] 0.  Not finite (an input, a clearance or a Lambda_k |h| was not): NaN / -1, violated = N + 1, undecided = the items, counts 0."""
    items = np.asarray(items, float); N1, nOb, _ = items.shape; G = CERT_TICKS
    r = np.zeros(CERT_OUT)
    if not (finite and np.isfinite(lam).all() and not np.isnan(items[:, :, :2]).any()):
        r[[0, 1, 12]] = np.nan; r[[2, 3, 4, 6, 7, 8]] = -1; r[5] = N1; r[9] = N1 * nOb; r[14] = 1
        return r, np.full((N1, 2), np.nan)
    iv = np.stack([items[:, :, 0].min(axis=1), items[:, :, 1].min(axis=1)], axis=1)
    seen = items[:, :, 1].min()
    skey = min((k, int(items[k, j, 2]), j) for k in range(N1) for j in range(nOb) if items[k, j, 1] == seen)
    vkeys = [(k, int(items[k, j, 3]), j) for k in range(N1) for j in range(nOb) if items[k, j, 3] < G]
    r[0] = iv[:, 0].min(); r[1] = seen; r[2:5] = skey
    r[5] = len({k for k, _, _ in vkeys}); r[6:9] = min(vkeys) if vkeys else (-1, -1, -1)
    r[9] = int((items[:, :, 0] == -np.inf).sum()); r[10] = items[:, :, 4].sum(); r[11] = items[:, :, 4].max(); r[12] = max(0.0, float(np.max(lam))) if len(lam) else 0.0
    r[13] = 1.0 if r[5] == 0 and r[9] == 0 else 0.0
    return r, iv
