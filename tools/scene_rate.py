"""Rate of the parking planner on the device in PER-INSTANCE obstacle fields (obca_scene_astar_batch, include/obca_plan_scenes.h) against the only host route such a batch
has -- one planner.hybrid_astar per instance, here on a pool of threads -- and beside the interior-point solve of the same batch.

    python tools/scene_rate.py [--out profiles/scene_plan_device_vs_host.json] [--batches 1024 4096] [--slots 256] [--threads 16] [--repeats 3] [--host-sample 256]

The inputs are scenarios.make_scene_batch's (scene_inputs: the backwards poses, 1-3 boxes on the road per instance).  Per batch size: one warm-up call (allocates the
slots), then `repeats` timed calls -- the search kernel by HIP events of the call's own and the whole call by the wall clock, each with its spread --, rounds and expansions
(mean / max), the counts by return code.  The host route plans `host-sample` of the same instances.  ipm_ms: DualMultWS + interior point of the same batch at N = 80 from
the device plans' warm starts, by the batch's own events.  An entry is appended to --out as soon as it is measured (a run per batch size adds to the same file).  No rate
is a pass criterion."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import obca_amd
from obca_amd import api, planner as PL, scenarios as S


def spread(v):
    v = np.asarray(v, float)
    return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()), runs=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/scene_plan_device_vs_host.json")
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=256)
    ap.add_argument("--max-nodes", type=int, default=1 << 19)
    ap.add_argument("--no-ipm", action="store_true")
    a = ap.parse_args()
    ctx = api._ctx(0)
    out = json.load(open(a.out)) if os.path.exists(a.out) else dict(device=ctx.name(), bucket_width=api.HYBRID_DEFAULT_WIDTH, max_nodes=a.max_nodes, host_threads=a.threads, entries=[])
    kw, v_nom = PL.SCENARIO_OPTS["backwards"]
    o = dict(PL.DEFAULT_OPTS); o.update(kw); opts = np.array([o[k] for k in PL.DEFAULT_OPTS], float)
    for B in a.batches:
        _, x0, xF, fields = S.scene_inputs(B)
        vl, Al, bl = [f[0] for f in fields], [f[1] for f in fields], [f[2] for f in fields]
        m = min(a.host_sample, B)

        def one(i):
            try:
                return PL.hybrid_astar(x0[i, :3], xF[i, :3], vl[i], Al[i], bl[i], **kw)
            except ValueError:
                return None
        ths = []
        with ThreadPoolExecutor(a.threads) as pool:
            for _ in range(a.repeats + 1):      # the first pass warms up (library load, thread start) and is not counted
                t0 = time.perf_counter(); h = list(pool.map(one, range(m))); ths.append(time.perf_counter() - t0)
        th = float(np.median(ths[1:]))
        host = dict(sample=m, wall_s=spread(ths[1:]), plans_per_s=m / th, expansions_mean=float(np.mean([r[2] for r in h if r is not None])), no_path=sum(r is None for r in h))
        api.hybrid_configure(slots=a.slots, max_nodes=a.max_nodes)
        args = (x0, xF, vl, Al, bl, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, opts, None, 1024)
        api.scene_astar_batch(*args)      # warm-up: the slots are allocated and cleared here
        kms, wall = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter(); paths, dirs, cnt, nexp, rounds = api.scene_astar_batch(*args); wall.append(time.perf_counter() - t0); kms.append(api.scene_ms())
        e = dict(B=B, slots=a.slots, obstacles_mean=float(np.mean([len(v) for v in vl])), rows_mean=float(np.mean([int(np.sum(v)) for v in vl])),
                 kernel_ms=spread(kms), call_wall_ms=spread(np.array(wall) * 1e3), plans_per_s_kernel=B / (np.median(kms) * 1e-3), plans_per_s_call=B / np.median(wall),
                 host=host, ratio_to_host_call=B / np.median(wall) / host["plans_per_s"],
                 rounds_mean=float(rounds.mean()), rounds_max=int(rounds.max()), expansions_mean=float(nexp.mean()), expansions_max=int(nexp.max()),
                 counts={str(k): int((cnt == k).sum()) for k in (0, -1, -2, -3)}, with_path=int((cnt > 0).sum()))
        if not a.no_ipm:
            N = 80
            Ts, xWS, uWS, ok = PL.path_to_warm_start_many(paths, dirs, cnt, N, xF, v_nom=v_nom, device=ctx)
            sel = np.flatnonzero(ok); n = len(sel)
            x = xWS[sel].copy(); x[:, 0, :] = x0[sel]
            b = obca_amd.Batch(ctx, n, N)
            b.upload(x0[sel], xF[sel], Ts[sel], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, [vl[i] for i in sel], [Al[i] for i in sel], [bl[i] for i in sel], x[:, :, 0], x[:, :, 1], x[:, :, 2], 0, x, uWS[sel])
            b.solve(); so = b.download()
            e.update(ipm_ms=b.kernel_ms()[0], dualws_ms=b.kernel_ms()[1], ipm_instances=n, ipm_solved=int((so["exitflag"] == 1).sum()), ipm_iterations_mean=float(so["iters"].mean()),
                     ipm_iterations_max=int(so["iters"].max()))
            b.close()
        out["entries"].append(e)
        print(json.dumps(e), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
