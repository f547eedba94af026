"""Cost of turning planner paths into parking warm starts: the device calls (planner.path_to_warm_start_many, Batch.set_path_warm_start: one wavefront per instance,
include/obca_path_ws.h) against the numpy loop over planner.path_to_warm_start, with the interior-point kernel of the same batch beside them.

    python tools/path_ws_rate.py [--out profiles/path_ws_device_vs_host.json] [--batches 1024 16384] [--host-sample 128] [--repeats 5]

Per a_max (0: plain conversion, 0.3: with velo_smooth) and batch size at N = 80: the kernel's time from HIP events, the wall time of both calls (packing, transfers, kernel,
download; minimum of `repeats`), the wall time of the numpy loop (measured on `host_sample` instances and scaled; one core) and the interior-point kernel's time of a solve
started from that warm start.  The paths are 128 planned ones of the backwards scenario, repeated.  An entry "device_vs_host_build" that tests/test_gpu_path_ws.py has left
in the file is kept."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import obca_amd                                                     # noqa: E402
from obca_amd import scenarios as S, planner as PL                  # noqa: E402

N = 80


def planned(n=128, seed=7):
    sc = S.BACKWARDS
    x0, xF = S.sample_poses(sc, n, np.random.default_rng(seed))
    A, b, vrows = S.scenario_hrep(sc)
    _, _, paths, dirs, cnt, _ = PL._hybrid_astar_dense(x0[:, :3], xF[:, :3], vrows, A, b, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, PL.effective_cpus(), 1024, dict(PL.SCENARIO_OPTS[sc["name"]][0]))
    ok = np.flatnonzero(cnt >= 2)
    return dict(paths=paths[ok], dirs=dirs[ok], cnt=cnt[ok], x0=x0[ok], xF=xF[ok], A=A, b=b, vOb=vrows)


def timed(fn, repeats):
    best = None; r = None
    for _ in range(repeats):
        t0 = time.perf_counter(); r = fn(); dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, r


def entry(ctx, p, B, smooth, repeats, host_sample):
    sel = np.arange(B) % len(p["cnt"])
    paths = np.ascontiguousarray(p["paths"][sel]); dirs = np.ascontiguousarray(p["dirs"][sel]); cnt = np.ascontiguousarray(p["cnt"][sel]); xF = np.ascontiguousarray(p["xF"][sel])
    PL.path_to_warm_start_many(paths, dirs, cnt, N, xF, smooth=smooth, device=ctx)
    host_call_ms, (Ts, xWS, uWS, ok) = timed(lambda: PL.path_to_warm_start_many(paths, dirs, cnt, N, xF, smooth=smooth, device=ctx), repeats)
    b = obca_amd.Batch(ctx, B, N)
    b.upload(p["x0"][sel], xF, np.ones(B), S.L_WHEELBASE, S.EGO, S.XYBOUNDS, p["vOb"], p["A"], p["b"], *np.zeros((3, B, N + 1)), 0, None, None)
    b.set_path_warm_start(paths, dirs, cnt, smooth=smooth)
    resident_ms, st = timed(lambda: b.set_path_warm_start(paths, dirs, cnt, smooth=smooth), repeats)
    kernel_ms = b.path_ws_ms()
    b.solve(); b.sync(); ipm_ms = b.kernel_ms()[0]; solved = int((b.download()["exitflag"] == 1).sum()); b.close()
    m = min(host_sample, B)
    t0 = time.perf_counter()
    for i in range(m):
        PL.path_to_warm_start(paths[i, :cnt[i]], dirs[i, :cnt[i]], N, xF[i], smooth=smooth)
    numpy_ms = (time.perf_counter() - t0) * 1e3 / m * B
    return dict(B=B, N=N, a_max=0.3 if smooth else 0.0, nodes_mean=float(cnt.mean()), nodes_max=int(cnt.max()), written=int((st == 0).sum()),
                kernel_ms=kernel_ms, host_pointer_call_wall_ms=host_call_ms, resident_call_wall_ms=resident_ms, numpy_loop_wall_ms=numpy_ms, numpy_loop_sampled_on=m,
                ipm_kernel_ms=ipm_ms, solved=solved, instances_per_s_kernel=B / kernel_ms * 1e3, instances_per_s_resident_call=B / resident_ms * 1e3,
                instances_per_s_numpy=B / numpy_ms * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_ws_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--host-sample", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    ctx = obca_amd.Context(0)
    p = planned()
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec.update(device=ctx.name(), what="tools/path_ws_rate.py: planner paths -> parking warm starts, device calls against the numpy loop (N = 80)", entries=[])
    for smooth in (False, True):
        for B in a.batches:
            e = entry(ctx, p, B, smooth, a.repeats, a.host_sample)
            rec["entries"].append(e); print(json.dumps(e), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
