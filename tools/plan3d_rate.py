"""Cost of planning the quadcopter's warm starts: the batch planner on the device (planner.quad_warm_start_many: one workgroup per search, the grid in LDS) against the
host loop over obca_plan_astar3d (scenarios.plan_quad_batch), with the interior-point solve of the same batch beside them.

    python tools/plan3d_rate.py [--out profiles/plan3d_device_vs_host.json] [--batches 256 1024] [--host-sample 64] [--variants]

Every entry records the plan kernel's time from HIP events, the wall time of the whole call (packing, transfers, kernel; minimum of `repeats`), plans per second of both
routes on this box (the host loop measured on `host_sample` instances and scaled; one core), the sweeps of the relaxation, and the quadcopter IPM kernel's time for the same
batch at N = 60.  --variants: the A/B of the thread counts and cell-to-thread maps (obca_plan3d.h: -DPL3_NT, -DPL3_MAP), each built into obca_amd/csrc/variants/ if it is
not there yet (build them where the compiler is cheap: `python tools/plan3d_rate.py --build-only`)."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from obca_amd import buildflags, scenarios as S, planner as PL     # noqa: E402

VARIANTS = [(nt, mp) for nt in (1024, 512, 256) for mp in (0, 1)]      # (threads per workgroup, map: 0 = node c to thread c mod NT, 1 = a contiguous run of nodes per thread)


def variant_path(nt, mp):
    return os.path.join(ROOT, "obca_amd", "csrc", "variants", "libobca_plan3d_nt%d_map%d.so" % (nt, mp))


def build_variants():
    for nt, mp in VARIANTS:
        buildflags.build("plan3d", out=variant_path(nt, mp), flags=["-DPL3_NT=%d" % nt, "-DPL3_MAP=%d" % mp])


def use_library(path):
    """point the front end at another build of the library (a fresh context with it)"""
    for h in PL._ctx3d.values():
        PL._lib3d.obca_plan3d_destroy(h)
    PL._LIB3D = path; PL._lib3d = None; PL._ctx3d.clear()


def endpoints(B, seed=20260925):
    """B end-point pairs that have a path (instance 0 the shipped one), as make_quad_batch(random_endpoints=True) draws them -- planned on the device"""
    q = S.make_quad_batch(B, 60, seed=seed, random_endpoints=True, device=0)
    return q["x0"], q["xF"]


def timed(fn, repeats):
    best = None; r = None
    for _ in range(repeats):
        t0 = time.perf_counter(); r = fn(); dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, r


def device_entry(x0, xF, N, repeats):
    PL.quad_warm_start_many(x0, xF, N)
    wall_ms, (xws, ok, _) = timed(lambda: PL.quad_warm_start_many(x0, xF, N, with_ms=True), repeats)
    kms = min(PL.quad_warm_start_many(x0, xF, N, with_ms=True)[2] for _ in range(repeats))
    _, cnt, sw, pms = PL.plan3d_paths(x0[:, :3], xF[:, :3])
    return dict(plan_kernel_ms=kms, paths_only_kernel_ms=pms, plan_wall_ms=wall_ms, plans_per_s_kernel=len(x0) / kms * 1e3, plans_per_s_wall=len(x0) / wall_ms * 1e3,
                sweeps_mean=float(sw.mean()), sweeps_max=int(sw.max()), way_points_mean=float(cnt.mean()), way_points_max=int(cnt.max()), planned=int(ok.sum())), xws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan3d_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024]); ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=64); ap.add_argument("--variants", action="store_true"); ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    if a.build_only:
        build_variants(); return
    import obca_amd as OA
    N = 60; ctx = OA.Context(0); default_lib = PL._LIB3D
    res = dict(device=ctx.name(), N=N, grid="41 x 41 x 21 nodes (room 10 x 10 x 5 m, res 0.25), five boxes, clear 0.4", threads_per_workgroup=1024, cell_map="node c -> thread c mod 1024", entries=[])
    for B in a.batches:
        x0, xF = endpoints(B)
        e, xws = device_entry(x0, xF, N, a.repeats)
        n = min(a.host_sample, B); t0 = time.perf_counter()
        S.plan_quad_batch(x0[:n].copy(), xF[:n].copy(), N, np.random.default_rng(0))
        host_ms = (time.perf_counter() - t0) * 1e3
        qb = OA.QuadBatch(ctx, B, N)
        qb.upload(x0, xF, S.quad_sample_time(N), S.QUAD_R, S.QUAD_OB, xws, 1.0)
        qb.solve(opts=OA.quadcopter_ipopt_opts()); ipm_ms = qb.kernel_ms(); out = qb.download(); v = qb.validate(); qb.close()
        e.update(batch=B, host_loop_ms_per_plan=host_ms / n, host_loop_plans_per_s=n / host_ms * 1e3, host_sample=n, ipm_kernel_ms_same_batch=ipm_ms,
                 solved_and_valid_from_device_plans=int(((out["exitflag"] == 1) & v["ok"]).sum()), repeats=a.repeats)
        res["entries"].append(e)
    if a.variants:
        build_variants(); res["variants"] = []
        for nt, mp in VARIANTS:
            use_library(variant_path(nt, mp))
            for B in a.batches:
                x0, xF = endpoints(B)
                e, _ = device_entry(x0, xF, N, a.repeats)
                res["variants"].append(dict(threads=nt, cell_map=mp, batch=B, plan_kernel_ms=e["plan_kernel_ms"], plan_wall_ms=e["plan_wall_ms"], sweeps_mean=e["sweeps_mean"], sweeps_max=e["sweeps_max"]))
        use_library(default_lib)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
