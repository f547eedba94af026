"""
Generates tests/golden/rollout_cases.npz (run from the repo root:  python tests/golden/make_rollout_cases.py): solved trajectories for the rollout on the continuous
vehicle models (obca_amd/csrc/obca_rollout.h), with the CPU oracles at their default options, numpy and scipy only.

  make_quad_batch(4, 20), QuadcopterSignedDist                  -> quad_x (4,12,21), quad_u (4,4,20), quad_t (4,), quad_exitflag
  make_batch(BACKWARDS, 8, 30), instances 0-2, ParkingSignedDist -> park_x (3,4,31), park_u (3,2,30), park_ts (3,31), park_exitflag
  the numpy records (validate.rollout_record) in both modes at 8 sub-steps: quadcopter with validate.quad_point_clearance, parking with the oracle's DualMultWS
  distance of every sample pose and the 1e-7 clamp     -> quad_rec, park_rec (instance, mode, 40)
  node states of the open loop (chain mode) from scipy.integrate.solve_ivp (DOP853, rtol 1e-13, atol 1e-15, interval by interval, u_k held): an integrator that
  shares no code with the statement -- its right-hand sides are written again below, with numpy          -> quad_ivp (4,12,21), park_ivp (3,4,31)

The script prints the gap between the discretisation and the continuous model and asserts that the fixture shows one: the quadcopter's one-interval position defect
(restart mode) is above 0.05 m on every instance, the open loop of parking instance 2 drifts more than 1 cm.  It also prints what the gyroscopic products at the current
rates change against the products frozen at stage 1 (the NLP's rows).
"""
import os
import sys
import numpy as np
from scipy.integrate import solve_ivp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)
from obca_amd import scenarios as S, validate as V   # noqa: E402
import oracle as O                                   # noqa: E402
import oracle_quad as Q                              # noqa: E402
OUT = os.path.dirname(os.path.abspath(__file__))
SUBSTEPS = 8


def quad_f(t, x, u, gyro=None):
    """the rigid body, vectorised with numpy (gyro: the three rates frozen, as the NLP's rows have them; None: the current ones)"""
    m, g, kF, kM, arm, I1, I2, I3 = 0.5, 9.81, 0.0611, 0.0015, 0.225, 3.9e-3, 4.4e-3, 4.9e-3
    s, c = np.sin(x[3:6]), np.cos(x[3:6]); w = x[9:12] if gyro is None else gyro; T = kF * np.sum(u ** 2)
    return np.array([x[6], x[7], x[8],
                     c[1] * x[9] + s[1] * x[11], np.tan(x[3]) * (s[1] * x[9] - c[1] * x[11]) + x[10], (-s[1] * x[9] + c[1] * x[11]) / c[0],
                     T / m * (s[0] * c[1] * s[2] + s[1] * c[2]), T / m * (-s[0] * c[1] * c[2] + s[1] * s[2]), T / m * c[0] * c[1] - g,
                     (arm * kF * (u[1] ** 2 - u[3] ** 2) - (I3 - I2) * w[1] * w[2]) / I1, (arm * kF * (u[2] ** 2 - u[0] ** 2) - (I1 - I3) * w[0] * w[2]) / I2,
                     (kM * (u[0] ** 2 - u[1] ** 2 + u[2] ** 2 - u[3] ** 2) - (I2 - I1) * w[0] * w[1]) / I3])


def park_f(t, x, u, L):
    return np.array([x[3] * np.cos(x[2]), x[3] * np.sin(x[2]), x[3] * np.tan(u[0]) / L, u[1]])


def ivp_chain(f, x0, u, h, *args):
    X = np.zeros((len(x0), u.shape[1] + 1)); X[:, 0] = x0
    for k in range(u.shape[1]):
        X[:, k + 1] = solve_ivp(f, (0.0, h[k]), X[:, k], method="DOP853", rtol=1e-13, atol=1e-15, args=(u[:, k],) + args).y[:, -1]
    return X


def main():
    out = {}
    bt = S.make_quad_batch(4, 20); N = 20
    sol = [Q.quadcopter_signed_dist_full(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], bt["timeWS"]) for i in range(4)]
    rec = np.zeros((4, 2, V.ROLL_OUT)); ivp = []
    for i, s in enumerate(sol):
        for mode in (0, 1):
            X, P = V.rollout_quad(s["xp"], s["up"], s["t"], bt["Ts"], SUBSTEPS, mode)
            rec[i, mode] = V.rollout_record(s["xp"], X, V.quad_point_clearance(P, bt["ob"], bt["R"]), SUBSTEPS, mode, 0.0)
        h = np.full(N, s["t"] * bt["Ts"]); ivp.append(ivp_chain(quad_f, s["xp"][:, 0], s["up"], h))
        frozen = ivp_chain(quad_f, s["xp"][:, 0], s["up"], h, s["xp"][9:12, 0])
        print("quadcopter %d: exit flag %d, interval %.3f s; one interval: %.3f m, %.3f rad, %.3f m/s; open loop: %.3f m worst (node %d), %.3f m at the end; "
              "gyroscopic products current against frozen: %.2e m" % (i, s["exitflag"], h[0], rec[i, 1, 1], rec[i, 1, 3], rec[i, 1, 4], rec[i, 0, 1], rec[i, 0, 2], rec[i, 0, 6],
                                                                      np.linalg.norm(ivp[-1][:3] - frozen[:3], axis=0).max()))
    assert (rec[:, 1, 1] > 0.05).all() and (rec[:, :, 0] == 0).all(), rec[:, :, :2]
    out.update(quad_x=np.array([s["xp"] for s in sol]), quad_u=np.array([s["up"] for s in sol]), quad_t=np.array([s["t"] for s in sol]),
               quad_exitflag=np.array([s["exitflag"] for s in sol]), quad_rec=rec, quad_ivp=np.array(ivp))

    bw = S.make_batch(S.BACKWARDS, 8, 30); N = 30
    px, pu, pt, pe, pivp = [], [], [], [], []; rec = np.zeros((3, 2, V.ROLL_OUT))
    for i in range(3):
        xWS = bw["xWS"][i].copy(); xWS[0] = bw["x0"][i]
        r = O.parking_signed_dist(bw["x0"][i], bw["xF"][i], N, bw["Ts"][i], bw["L"], bw["ego"], bw["XYbounds"], bw["vOb"], bw["A"], bw["b"], xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, bw["uWS"][i])
        x, u, ts = r["xp"], r["up"], np.asarray(r["timeScale"], float)
        for mode in (0, 1):
            X, P = V.rollout_parking(x, u, ts, bw["Ts"][i], bw["L"], SUBSTEPS, mode)
            _, _, d = O.dualmult_ws(len(P) - 1, bw["vOb"], bw["A"], bw["b"], P[:, 0].copy(), P[:, 1].copy(), P[:, 2].copy(), bw["ego"])
            rec[i, mode] = V.rollout_record(x, X, np.where(d < V.CLR_TOUCH, 0.0, d), SUBSTEPS, mode, V.DMIN)
        pivp.append(ivp_chain(park_f, x[:, 0], u, ts[:N] * bw["Ts"][i], bw["L"]))
        px.append(x); pu.append(u); pt.append(ts); pe.append(r["exitflag"])
        print("parking %d: exit flag %d, interval %.3f s; one interval: %.2f mm, yaw %.1e, speed %.1e; open loop: %.2f cm worst (node %d); clearance of the rolled "
              "samples %.4f (at the solution's nodes %.4f)" % (i, r["exitflag"], ts[0] * bw["Ts"][i], 1e3 * rec[i, 1, 1], rec[i, 1, 3], rec[i, 1, 4], 1e2 * rec[i, 0, 1], rec[i, 0, 2],
                                                               rec[i, 0, 16], rec[i, 1, 17]))
    assert rec[2, 0, 1] > 0.01 and (rec[:, :, 0] == 0).all(), rec[:, :, :2]
    out.update(park_x=np.array(px), park_u=np.array(pu), park_ts=np.array(pt), park_exitflag=np.array(pe), park_rec=rec, park_ivp=np.array(pivp))
    np.savez_compressed(os.path.join(OUT, "rollout_cases.npz"), substeps=SUBSTEPS, **out)


if __name__ == "__main__":
    main()
