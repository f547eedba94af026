"""What the receding-horizon restart of the resident quadcopter batch (QuadBatch.shift_warm_start) buys on the device, against a cold solve and against the route it
replaces (download, shift in numpy, upload), for scenarios.make_quad_batch instances at N = 60.

    python tools/quad_mpc_rate.py [--out profiles/quad_mpc_restart.json] [--batches 256 1024] [--shifts 1 4] [--steps 20] [--repeats 3]

Per (batch, shift, option set) an entry records: iterations (mean, max) and interior-point kernel time of the cold solve and of the restart from the shifted solution with
obca_amd.quad_warm_restart_opts; the wall time of shift_warm_start (stream synchronisation included, minimum of `repeats`); the wall time of download + numpy shift + upload for
the same batch; and a closed loop of `steps` steps in which the measured state -- the predicted one plus a seeded disturbance of +-0.02 on positions and velocities -- comes back
through x0_new: kernel time and wall time (shift + solve + sync) per step and the share of instances that converged (exit flag 1).  The download that builds the next measured
state stands in for the plant and is not part of the step's wall time."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import obca_amd as OA                       # noqa: E402
from obca_amd import scenarios as S         # noqa: E402


def host_route(b, q, N, shift):
    """the route the device call replaces: download the solution, advance it with numpy, upload the new problem (host packing, H2D copy and a sync inside upload)"""
    t0 = time.perf_counter()
    out = b.download()
    x = np.transpose(out["xp"], (0, 2, 1))
    xws = x[:, np.minimum(np.arange(N + 1) + shift, N)]
    b.upload(x[:, shift], q["xF"], q["Ts"], q["R"], q["ob"], xws, out["timeScale"][:, 0], dual_ws=True)
    return (time.perf_counter() - t0) * 1e3


def entry(ctx, q, B, N, shift, reference, steps, repeats, seed):
    cold = OA.quadcopter_ipopt_opts() if reference else OA.quadcopter_default_opts()
    warm = OA.quad_warm_restart_opts(reference=reference)
    b = OA.QuadBatch(ctx, B, N)

    def fresh():
        b.upload(q["x0"], q["xF"], q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"], dual_ws=True)
        b.solve(opts=cold)
    fresh(); cold_ms = b.kernel_ms(); o1 = b.download()
    shift_ms = None
    for _ in range(repeats):
        t0 = time.perf_counter(); b.shift_warm_start(shift); dt = (time.perf_counter() - t0) * 1e3
        shift_ms = dt if shift_ms is None else min(shift_ms, dt)
        b.solve(opts=warm); warm_ms = b.kernel_ms(); o2 = b.download()
        fresh()
    host_ms = None
    for _ in range(repeats):
        dt = host_route(b, q, N, shift); host_ms = dt if host_ms is None else min(host_ms, dt)
        fresh()
    # closed loop
    out = b.download(); rng = np.random.default_rng(seed)
    x0 = q["x0"].copy(); kern, wall, conv, its = [], [], [], []
    for _ in range(steps):
        good = out["exitflag"] == 1
        x0 = np.where(good[:, None], out["xp"][:, :, shift], x0)
        x0[:, :3] += rng.uniform(-0.02, 0.02, (B, 3)); x0[:, 6:9] += rng.uniform(-0.02, 0.02, (B, 3))
        t0 = time.perf_counter(); b.shift_warm_start(shift, x0_new=x0); b.solve(opts=warm); wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(b.kernel_ms()); out = b.download()
        conv.append(float((out["exitflag"] == 1).mean())); its.append(float(out["iters"].mean()))
    b.close()
    ok1, ok2 = o1["exitflag"] == 1, o2["exitflag"] == 1
    return dict(batch=B, N=N, shift=shift, options="reference" if reference else "throughput",
                cold_iters_mean=float(o1["iters"].mean()), cold_iters_max=int(o1["iters"].max()), cold_converged=float(ok1.mean()), cold_ipm_ms=cold_ms,
                restart_iters_mean=float(o2["iters"].mean()), restart_iters_max=int(o2["iters"].max()), restart_converged=float(ok2.mean()), restart_ipm_ms=warm_ms,
                shift_warm_start_wall_ms=shift_ms, download_numpy_shift_upload_wall_ms=host_ms,
                loop_steps=steps, loop_ipm_ms=kern, loop_wall_ms=wall, loop_converged=conv, loop_iters_mean=its, repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_mpc_restart.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024]); ap.add_argument("--shifts", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--horizon", type=int, default=60); ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--seed", type=int, default=20260925)
    a = ap.parse_args()
    ctx = OA.Context(0)
    res = dict(device=ctx.name(), workload="quadcopter, 5 boxes, N = %d, scenarios.make_quad_batch (jittered end points, way-point warm starts)" % a.horizon, entries=[])
    for B in a.batches:
        q = S.make_quad_batch(B, a.horizon)
        for shift in a.shifts:
            for reference in (False, True):
                e = entry(ctx, q, B, a.horizon, shift, reference, a.steps, a.repeats, a.seed)
                res["entries"].append(e)
                print("B %d shift %d %s: iterations %.1f -> %.1f, ipm %.1f -> %.1f ms, shift %.3f ms against %.1f ms on the host route; loop %.1f ms / step, %.3f converged"
                      % (B, shift, e["options"], e["cold_iters_mean"], e["restart_iters_mean"], e["cold_ipm_ms"], e["restart_ipm_ms"], e["shift_warm_start_wall_ms"],
                         e["download_numpy_shift_upload_wall_ms"], float(np.mean(e["loop_wall_ms"])), float(np.mean(e["loop_converged"]))), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
