"""
Generates tests/golden/refine_cases.npz (run from the repo root:  python tests/golden/make_refine_cases.py): what refining a solved parking batch onto a finer horizon buys,
with the structured C oracle and numpy only.

  make_batch(BACKWARDS, 8, 30), instances 0 .. 5, ParkingSignedDist, solved at N = 30 by the oracle at its default options  -> x, u, t, lam, mu, exit flag, iterations
  their refinement x 2 by validate.refine_parking (Ts / 2, interpolated reference, refined x, held u, carried lam / mu)        -> fx, fu, fref, flam, fmu
  the oracle's N = 60 solutions from those starts
      ws    : DualMultWS duals (none handed over), default options
      carry : the carried multipliers, default options with mu_init = bound_push = bound_frac = 1e-4 (what api.warm_restart_opts() sets)
  and the clearance record (numpy validate.parking_samples, the oracle's DualMultWS distance per pose, the 1e-7 clamp; need = 0.05) of the coarse solution at 8 sub-steps
  and of both fine solutions at 4: the same sample density.

The script prints one line per instance and the two iteration sums; tests/test_refine_cpu.py pins them.
"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
from obca_amd import scenarios as S, validate as V   # noqa: E402
import oracle as O                                   # noqa: E402
OUT = os.path.dirname(os.path.abspath(__file__))
N, FACTOR, INSTANCES, S_COARSE, S_FINE = 30, 2, 6, 8, 4


def record(bt, x, u, ts, Ts, substeps):
    poses = V.parking_samples(x, u, ts, Ts, bt["L"], substeps)
    _, _, d = O.dualmult_ws(len(poses) - 1, bt["vOb"], bt["A"], bt["b"], poses[:, 0].copy(), poses[:, 1].copy(), poses[:, 2].copy(), bt["ego"])
    return V.clearance_record(np.where(d < V.CLR_TOUCH, 0.0, d), substeps, V.DMIN)


def main():
    bt = S.make_batch(S.BACKWARDS, 8, N); Nf = N * FACTOR
    warm = O.default_opts(); warm.mu_init = warm.bound_push = warm.bound_frac = 1e-4
    keys = ("x", "u", "t", "lam", "mu", "exitflag", "iters", "rec", "fx", "fu", "fref", "flam", "fmu", "fTs") + tuple(m + "_" + k for m in ("ws", "carry") for k in ("x", "u", "t", "exitflag", "iters", "rec"))
    out = {k: [] for k in keys}
    for i in range(INSTANCES):
        xWS = bt["xWS"][i].copy(); xWS[0] = bt["x0"][i]; Ts = float(bt["Ts"][i])
        common = (bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"])
        r = O.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, Ts, *common, xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, bt["uWS"][i])
        t = float(r["timeScale"][0])
        f = V.refine_parking(r["xp"], r["up"], t, Ts, bt["L"], FACTOR, ref=xWS[:, :3].T, lam=r["lp"], mu=r["np"])
        for k, v in (("x", r["xp"]), ("u", r["up"]), ("t", t), ("lam", r["lp"]), ("mu", r["np"]), ("exitflag", r["exitflag"]), ("iters", r["iters"]), ("rec", record(bt, r["xp"], r["up"], t, Ts, S_COARSE)),
                     ("fx", f["x"]), ("fu", f["u"]), ("fref", f["ref"]), ("flam", f["lam"]), ("fmu", f["mu"]), ("fTs", f["Ts"])):
            out[k].append(v)
        line = "instance %d  N=%d: exitflag %d, %d iterations, t %.4f, min %.6g, min_nodes %.6g, below %d" % (i, N, r["exitflag"], r["iters"], t, out["rec"][-1][0], out["rec"][-1][1], out["rec"][-1][4])
        for mode, duals, opts in (("ws", (None, None), None), ("carry", (f["lam"].T, f["mu"].T), warm)):
            q = O.parking_signed_dist(bt["x0"][i], bt["xF"][i], Nf, f["Ts"], *common, f["ref"][0], f["ref"][1], f["ref"][2], 0, f["x"].T, f["u"].T, *duals, opts=opts)
            tq = float(q["timeScale"][0]); rec = record(bt, q["xp"], q["up"], tq, f["Ts"], S_FINE)
            for k, v in (("x", q["xp"]), ("u", q["up"]), ("t", tq), ("exitflag", q["exitflag"]), ("iters", q["iters"]), ("rec", rec)):
                out[mode + "_" + k].append(v)
            line += "  | N=%d %s: exitflag %d, %d iterations, t %.4f, min %.6g, min_nodes %.6g, below %d" % (Nf, mode, q["exitflag"], q["iters"], tq, rec[0], rec[1], rec[4])
        print(line)
    print("iterations of the N = %d solves, instances 0 .. %d: DualMultWS start %d, carried multipliers %d" % (Nf, INSTANCES - 1, sum(out["ws_iters"]), sum(out["carry_iters"])))
    np.savez_compressed(os.path.join(OUT, "refine_cases.npz"), N=N, factor=FACTOR, substeps_coarse=S_COARSE, substeps_fine=S_FINE, Ts=bt["Ts"][:INSTANCES], **{k: np.array(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
