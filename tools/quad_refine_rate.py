"""Cost and effect of refining a solved quadcopter batch onto a finer horizon on the device (QuadBatch.refine, include/obca_quad_subdivide.h: one wavefront per destination
instance), against doing the same through the host: download() + a validate.refine_quad loop + upload() of a new batch.

    python tools/quad_refine_rate.py [--out profiles/quad_refine_device_vs_host.json] [--batches 256 1024] [--margins 0 0.005] [--host-sample 64] [--repeats 5]

make_quad_batch(B, 60) solved at the throughput defaults, refined by 2 (N = 120) with each margin: the kernel's time from HIP events (refine_ms) and the wall time of refine()
into an existing batch (minimum of `repeats`).  Host route for the same selection: download() timed, the numpy loop timed on `host_sample` instances on one core and scaled,
upload() of the fine batch timed.  Iterations and ipm_ms of the fine solve from the refined start -- cold options and quad_warm_restart_opts() -- against a cold
make_quad_batch(B, 120) solve, with both option sets (throughput defaults; the reference's IPOPT switches).  Clearance: `below` and the minimum before (8 samples per coarse
interval, need 0) and after (4 per fine interval, need = -margin: against the true radius) over the instances that solved."""
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

N, R = 60, 2


def timed(fn, repeats):
    best = None; r = None
    for _ in range(repeats):
        t0 = time.perf_counter(); r = fn(); dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, r


def upload(ctx, bt, B, n, **kw):
    b = obca_amd.QuadBatch(ctx, B, n)
    a = dict(bt, **kw)
    b.upload(a["x0"], a["xF"], a["Ts"], a["R"], a["ob"], a["xWS"], a["timeWS"])
    return b


def solve_stats(b, opts=None):
    b.solve(opts); o = b.download()
    return dict(ipm_ms=b.kernel_ms(), solved=int((o["exitflag"] == 1).sum()), iterations_mean=float(o["iters"].mean()), iterations_max=int(o["iters"].max())), o


def option_sets():
    return (("throughput", obca_amd.quadcopter_default_opts(), obca_amd.quad_warm_restart_opts()), ("reference", obca_amd.quadcopter_ipopt_opts(), obca_amd.quad_warm_restart_opts(reference=True)))


def entry(ctx, B, margin, repeats, host_sample, cold):
    bt = S.make_quad_batch(B, N)
    b = upload(ctx, bt, B, N)
    coarse, o1 = solve_stats(b)
    c1 = b.clearance(8); ok1 = o1["exitflag"] == 1
    dst = obca_amd.QuadBatch(ctx, B, R * N)
    b.refine(R, margin=margin, into=dst)
    wall_ms, (_, st) = timed(lambda: b.refine(R, margin=margin, into=dst), repeats)
    e = dict(B=B, N=N, factor=R, margin=margin, coarse=coarse, refine_kernel_ms=dst.refine_ms(), refine_wall_ms=wall_ms, status_0=int((st == 0).sum()),
             below_before=int(c1["below"][ok1].sum()), instances_below_before=int((c1["below"][ok1] > 0).sum()), min_before=float(c1["min"][ok1].min()), fine_solve={}, fine_solve_cold=cold)
    for name, plain, warm in option_sets():
        for key, opts in (("refined_start_cold_options", plain), ("refined_start_warm_restart_options", warm)):
            b.refine(R, margin=margin, into=dst)
            s, o2 = solve_stats(dst, opts)
            c2 = dst.clearance(8 // R, need=-margin); ok2 = o2["exitflag"] == 1
            s.update(below_after=int(c2["below"][ok2].sum()), instances_below_after=int((c2["below"][ok2] > 0).sum()), min_after_against_true_R=float(c2["min"][ok2].min() + margin) if ok2.any() else None)
            e["fine_solve"][name + "_" + key] = s
    # the host route: down, numpy, up
    t0 = time.perf_counter(); o = b.download(); e["host_download_wall_ms"] = (time.perf_counter() - t0) * 1e3
    m = min(host_sample, B); t0 = time.perf_counter()
    fs = [V.refine_quad(o["xp"][i], o["timeScale"][i, 0], bt["Ts"], R)["x"] for i in range(m)]
    e["host_numpy_loop_wall_ms"] = (time.perf_counter() - t0) * 1e3 / m * B; e["host_loop_sampled_on"] = m
    fx = np.stack([fs[i % m].T for i in range(B)])
    t0 = time.perf_counter(); hb = upload(ctx, bt, B, R * N, Ts=bt["Ts"] / R, R=bt["R"] + margin, xWS=fx, timeWS=o["timeScale"][:, 0]); hb.sync(); e["host_upload_wall_ms"] = (time.perf_counter() - t0) * 1e3
    e["host_route_wall_ms"] = e["host_download_wall_ms"] + e["host_numpy_loop_wall_ms"] + e["host_upload_wall_ms"]
    for q in (hb, b, dst):
        q.close()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_refine_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--margins", type=float, nargs="+", default=[0.0, 0.005])
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    ctx = obca_amd.Context(0)
    rec = dict(device=ctx.name(), what="tools/quad_refine_rate.py: solved quadcopter batches refined onto a finer horizon on the device, beside the host route and the solves around it", entries=[])
    for B in a.batches:
        cb = upload(ctx, S.make_quad_batch(B, R * N), B, R * N)
        cold = {name: solve_stats(cb, plain)[0] for name, plain, _ in option_sets()}      # the way-point warm start at r N, once per batch size
        cb.close()
        for margin in a.margins:
            e = entry(ctx, B, margin, a.repeats, a.host_sample, cold)
            rec["entries"].append(e); print(json.dumps(e), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(rec, open(a.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
