"""Cost and effect of refining a solved parking batch onto a finer horizon on the device (Batch.refine, include/obca_refine.h: one wavefront per destination instance), against
doing the same through the host: download() + a validate.refine_parking loop + upload() of a new batch.

    python tools/refine_rate.py [--out profiles/refine_device_vs_host.json] [--batches 1024 16384] [--factors 2 3] [--host-sample 64] [--repeats 5] [--effect-batch 256] [--diffs FILE]

Kernel and call time: backwards parking at N = 40 (1 024 planned instances, repeated for the larger batch), refined by 2 (N = 80) and 3 (N = 120): the kernel's time from HIP
events and the wall time of refine() into an existing batch (minimum of `repeats`), with and without carried multipliers.  Host route: download() timed, the numpy loop timed
on `host_sample` instances on one core and scaled, upload() of the fine batch timed.  Iterations and ipm_ms of the fine solve: cold from the planner's start at r N; refined,
duals=False; refined, duals=True with warm_restart_opts().  Clearance: minimum and `below` before (8 sub-steps) and after (8 / r sub-steps: the same sample density) on
make_corridor_batch(B, 40, seed=11, clearance=(0.0, 0.2)) and make_batch(BACKWARDS, B, 30), B = `effect_batch`.  --diffs: the file tests/test_gpu_refine.py leaves its
largest differences in (OBCA_REFINE_DIFFS); they are copied into the profile as "largest_differences"."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import obca_amd                                                     # noqa: E402
from obca_amd import scenarios as S, validate as V                  # noqa: E402


def timed(fn, repeats):
    best = None; r = None
    for _ in range(repeats):
        t0 = time.perf_counter(); r = fn(); dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, r


def tiled(base, B):
    sel = np.arange(B) % len(base["Ts"])
    return dict(base, x0=base["x0"][sel], xF=base["xF"][sel], Ts=base["Ts"][sel], xWS=base["xWS"][sel], uWS=base["uWS"][sel])


def upload(ctx, bt, B, N, Ts=None, ref=None, xWS=None, uWS=None):
    x = bt["xWS"].copy() if xWS is None else xWS
    if xWS is None:
        x[:, 0, :] = bt["x0"]
    ref = x[:, :, :3] if ref is None else ref
    b = obca_amd.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"] if Ts is None else Ts, bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], ref[:, :, 0], ref[:, :, 1], ref[:, :, 2], 0, x, bt["uWS"] if uWS is None else uWS)
    return b, x


def solve_stats(b, opts=None):
    b.solve(opts); o = b.download()
    return dict(ipm_ms=b.kernel_ms()[0], dualws_ms=b.kernel_ms()[1], solved=int((o["exitflag"] == 1).sum()), iterations_mean=float(o["iters"].mean()), iterations_max=int(o["iters"].max()))


def rate_entries(ctx, B, N, r, repeats, host_sample):
    bt = tiled(S.make_batch(S.BACKWARDS, min(B, 1024), N), B)
    b, xWS = upload(ctx, bt, B, N)
    coarse = solve_stats(b)
    dst = obca_amd.Batch(ctx, B, r * N)
    e = dict(B=B, N=N, factor=r, coarse=coarse)
    for duals in (False, True):
        b.refine(r, duals=duals, into=dst)
        wall_ms, (_, st) = timed(lambda: b.refine(r, duals=duals, into=dst), repeats)
        key = "duals" if duals else "no_duals"
        e["refine_kernel_ms_" + key] = dst.refine_ms(); e["refine_wall_ms_" + key] = wall_ms; e["status_0_" + key] = int((st == 0).sum())
        e["fine_solve_refined_" + key] = solve_stats(dst, obca_amd.warm_restart_opts() if duals else None)
    # the host route: down, numpy, up
    t0 = time.perf_counter(); o = b.download(); e["host_download_wall_ms"] = (time.perf_counter() - t0) * 1e3
    m = min(host_sample, B); t0 = time.perf_counter()
    fs = [V.refine_parking(o["xp"][i], o["up"][i], o["timeScale"][i], bt["Ts"][i], bt["L"], r, ref=xWS[i, :, :3].T) for i in range(m)]
    e["host_numpy_loop_wall_ms"] = (time.perf_counter() - t0) * 1e3 / m * B; e["host_loop_sampled_on"] = m
    fx = np.stack([fs[i % m]["x"].T for i in range(B)]); fu = np.stack([fs[i % m]["u"].T for i in range(B)]); fr = np.stack([fs[i % m]["ref"].T for i in range(B)])
    t0 = time.perf_counter(); hb, _ = upload(ctx, bt, B, r * N, Ts=bt["Ts"] / r, ref=fr, xWS=fx, uWS=fu); hb.sync(); e["host_upload_wall_ms"] = (time.perf_counter() - t0) * 1e3
    hb.close()
    # cold: the planner's start at r N
    cold_bt = tiled(S.make_batch(S.BACKWARDS, min(B, 1024), r * N), B)
    cb, _ = upload(ctx, cold_bt, B, r * N); e["fine_solve_cold_planner_start"] = solve_stats(cb); cb.close()
    b.close(); dst.close()
    return e


def effect_entry(ctx, name, bt, N, r):
    B = len(bt["Ts"])
    b, _ = upload(ctx, bt, B, N)
    b.solve(); o1 = b.download(); ok = o1["exitflag"] == 1
    c1 = b.clearance(substeps=8)
    select = ok & (c1["below"] > 0)
    e = dict(scenario=name, B=B, N=N, factor=r, solved=int(ok.sum()), selected=int(select.sum()))
    if select.any():
        d, st = b.refine(r, select)
        d.solve(); o2 = d.download(); c2 = d.clearance(substeps=max(1, 8 // r)); ok2 = o2["exitflag"] == 1
        e.update(status_0=int((st == 0).sum()), fine_solved=int(ok2.sum()), min_before=float(c1["min"][select].min()), below_before=int(c1["below"][select].sum()),
                 min_after=float(c2["min"][ok2].min()) if ok2.any() else None, below_after=int(c2["below"][ok2].sum()), instances_still_below=int((c2["below"][ok2] > 0).sum()),
                 min_nodes_after=float(c2["min_nodes"][ok2].min()) if ok2.any() else None, refine_kernel_ms=d.refine_ms(), fine_ipm_ms=d.kernel_ms()[0])
        d.close()
    b.close()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--factors", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--effect-batch", type=int, default=256)
    ap.add_argument("--diffs", default=None)
    a = ap.parse_args()
    ctx = obca_amd.Context(0)
    rec = dict(device=ctx.name(), what="tools/refine_rate.py: solved parking batches refined onto a finer horizon on the device, beside the host route and the solves around it", entries=[], effect=[])
    if a.diffs and os.path.exists(a.diffs):
        rec["largest_differences"] = dict(json.load(open(a.diffs)), what="largest |device - host build|, |device - numpy| and |resident pipeline - oracle| over tests/test_gpu_refine.py")
    for B in a.batches:
        for r in a.factors:
            e = rate_entries(ctx, B, 40, r, a.repeats, a.host_sample)
            rec["entries"].append(e); print(json.dumps(e), flush=True)
    for name, bt, N in (("corridor", S.make_corridor_batch(a.effect_batch, 40, seed=11, clearance=(0.0, 0.2)), 40), ("backwards", S.make_batch(S.BACKWARDS, a.effect_batch, 30), 30)):
        e = effect_entry(ctx, name, bt, N, 2)
        rec["effect"].append(e); print(json.dumps(e), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
