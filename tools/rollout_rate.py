"""Cost of the rollout on the continuous vehicle models (Batch.rollout / QuadBatch.rollout, include/obca_rollout.h: one wavefront per instance) beside the solve it follows
and against doing the same on the host, and what the rolled state does to a receding-horizon loop.

    python tools/rollout_rate.py [--out profiles/rollout_device_vs_host.json] [--batches 1024 16384] [--quad-batches 256 1024] [--substeps 1 8 32] [--host-sample 64]
                                 [--repeats 5] [--diffs FILE] [--closed-loop] [--no-rates]

Config 2 (backwards parking, N = 80; 1 024 planned instances, repeated for the larger batch) and make_quad_batch(B, 60): per batch size, number of sub-steps and mode
(chain / restart) the kernel's time from HIP events and the wall time of rollout() (kernel + 40 doubles per instance down), medians of `repeats` after one warm-up call,
beside ipm_ms of the same batch's solve; the wall time of rollout_states(); the deviations found.  In chain mode ONE lane of the wavefront integrates (a recurrence in
time), in restart mode the lanes take intervals: the two kernel times side by side are the measured cost of the 63 idle lanes.  The host route -- download() and the numpy
statement (validate.rollout_parking / rollout_quad, the sample clearances left out) at 8 sub-steps -- is timed on `host_sample` instances on one core and scaled.
--diffs: the file tests/test_gpu_rollout.py leaves its largest device-to-host-build differences in (OBCA_ROLLOUT_DIFFS); copied into the profile.
--closed-loop: 10 steps of solve -> rollout(chain) -> rollout_states()[:, shift] -> shift_warm_start(shift, x0_new=...) -> solve at B = 256, N = 60, shift 4 with
quad_warm_restart_opts(reference=True) and max_iter capped at 200: solved counts and iterations per step with the rolled state as the plant, against the same loop fed
the predicted state (x0_new = None)."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import obca_amd                                                     # noqa: E402
from obca_amd import scenarios as S, validate as V                  # noqa: E402


def timed(fn, kernel_ms, repeats):
    """one warm-up call, then medians of wall and kernel time over `repeats` calls"""
    fn(); wall = []; kern = []; r = None
    for _ in range(repeats):
        t0 = time.perf_counter(); r = fn(); wall.append((time.perf_counter() - t0) * 1e3); kern.append(kernel_ms())
    return float(np.median(wall)), float(np.median(kern)), r


def entries(b, cfg, B, N, ipm_ms, solved, substeps, repeats, host):
    out = []
    for S_ in substeps:
        for restart in (False, True):
            wall_ms, kernel_ms, r = timed(lambda: b.rollout(S_, restart), b.rollout_ms, repeats)
            t0 = time.perf_counter(); b.rollout_states(); states_ms = (time.perf_counter() - t0) * 1e3
            fin = r["finite"]
            e = dict(config=cfg, B=B, N=N, substeps=S_, mode="restart" if restart else "chain", kernel_ms=kernel_ms, rollout_wall_ms=wall_ms, states_download_wall_ms=states_ms,
                     ipm_ms=ipm_ms, kernel_over_ipm=kernel_ms / ipm_ms, solved=solved, finite=int(fin.sum()),
                     dev_pos_median=float(np.median(r["dev_pos"][fin])) if fin.any() else None, dev_pos_max=float(r["dev_pos"][fin].max()) if fin.any() else None,
                     clearance_min_smallest=float(r["clearance"]["min"][fin].min()) if fin.any() else None)
            if S_ == 8 and host is not None:
                e.update(host(restart))
            out.append(e); print(json.dumps(e), flush=True)
    return out


def parking_entries(ctx, B, substeps, repeats, host_sample):
    N = 80; base = S.make_batch(S.BACKWARDS, min(B, 1024), N); sel = np.arange(B) % len(base["Ts"])
    bt = dict(base, x0=base["x0"][sel], xF=base["xF"][sel], Ts=base["Ts"][sel], xWS=base["xWS"][sel], uWS=base["uWS"][sel])
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = obca_amd.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    b.solve(); ipm_ms, _ = b.kernel_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    m = min(host_sample, B)

    def host(restart):
        t0 = time.perf_counter(); o = b.download(); down_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for i in range(m):
            V.rollout_parking(o["xp"][i], o["up"][i], o["timeScale"][i], bt["Ts"][i], bt["L"], 8, restart)
        return dict(host_download_wall_ms=down_ms, host_numpy_loop_wall_ms=(time.perf_counter() - t0) * 1e3 / m * B, host_loop_sampled_on=m)
    out = entries(b, 2, B, N, ipm_ms, solved, substeps, repeats, host if m > 0 else None)
    b.close()
    return out


def quad_entries(ctx, B, substeps, repeats, host_sample):
    N = 60; bt = S.make_quad_batch(B, N)
    b = obca_amd.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    b.solve(); ipm_ms = b.kernel_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    m = min(host_sample, B)

    def host(restart):
        t0 = time.perf_counter(); o = b.download(); down_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for i in range(m):
            V.rollout_quad(o["xp"][i], o["up"][i], o["timeScale"][i], bt["Ts"], 8, restart)
        return dict(host_download_wall_ms=down_ms, host_numpy_loop_wall_ms=(time.perf_counter() - t0) * 1e3 / m * B, host_loop_sampled_on=m)
    out = entries(b, "quad60", B, N, ipm_ms, solved, substeps, repeats, host if m > 0 else None)
    b.close()
    return out


def closed_loop(ctx, B=256, N=60, shift=4, steps=10, max_iter=200):
    """the rolled state as the plant of a receding-horizon loop, beside the loop that is fed its own prediction"""
    bt = S.make_quad_batch(B, N); out = {}
    for plant in ("rollout", "predicted"):
        b = obca_amd.QuadBatch(ctx, B, N)
        b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
        o = obca_amd.quadcopter_ipopt_opts(); o.max_iter = max_iter
        b.solve(opts=o)
        w = obca_amd.quad_warm_restart_opts(reference=True); w.max_iter = max_iter
        log = []
        for step in range(steps):
            sol = b.download(); ok = sol["exitflag"] == 1
            e = dict(step=step, solved=int(ok.sum()), iterations_median=float(np.median(sol["iters"])), iterations_max=int(sol["iters"].max()), ipm_ms=b.kernel_ms())
            if plant == "rollout":
                r = b.rollout(8, False); x_new = b.rollout_states()[:, shift]
                lost = ~np.isfinite(x_new).all(axis=1)
                x_new[lost] = sol["xp"][lost, :, shift]      # (an instance that is not finite -- a failed solve -- goes on from its prediction)
                e.update(rollout_kernel_ms=b.rollout_ms(), plant_off_prediction_median_m=float(np.median(np.linalg.norm(x_new[:, :3] - sol["xp"][:, :3, shift], axis=1))), not_finite=int(lost.sum()),
                         clearance_min_smallest=float(np.nanmin(r["clearance"]["min"])))
                b.shift_warm_start(shift, x0_new=x_new)
            else:
                b.shift_warm_start(shift)
            b.solve(opts=w)
            log.append(e); print(plant, json.dumps(e), flush=True)
        b.close()
        out[plant] = log
    return dict(B=B, N=N, shift=shift, steps=steps, max_iter=max_iter, substeps=8, loops=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 16384])
    ap.add_argument("--quad-batches", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--substeps", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--diffs", default=None)
    ap.add_argument("--closed-loop", action="store_true")
    ap.add_argument("--no-rates", action="store_true")
    a = ap.parse_args()
    ctx = obca_amd.Context(0)
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec.update(device=ctx.name(), what="tools/rollout_rate.py: rollout on the continuous vehicle models on the device, beside the solve of the same batch and the host route")
    if a.diffs and os.path.exists(a.diffs):
        rec["device_vs_host_build"] = dict(json.load(open(a.diffs)), what="largest relative |device - host build| and |resident - host-pointer call| over tests/test_gpu_rollout.py")
    if not a.no_rates:
        rec["entries"] = []
        for B in a.batches:
            rec["entries"] += parking_entries(ctx, B, a.substeps, a.repeats, a.host_sample)
        for B in a.quad_batches:
            rec["entries"] += quad_entries(ctx, B, a.substeps, a.repeats, a.host_sample)
    if a.closed_loop:
        rec["closed_loop"] = closed_loop(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
