"""Rate of the parking planner on the device (obca_hybrid_astar_batch, include/obca_plan_device.h) against the host planner (obca_plan_hybrid_astar_batch2) on the same
machine, and beside the interior-point solve of the same batch.

    python tools/hybrid_rate.py [--out profiles/hybrid_device_vs_host.json] [--batches 1024 4096] [--slots 64 128 256] [--threads 16] [--repeats 3] [--host-sample 256]

Per config (2: backwards, 3: parallel with goal jitter), batch size and slot count: one warm-up call (allocates the slots), then `repeats` timed calls -- the search kernel by
HIP events and the whole call by the wall clock, each with its spread (min / median / max) --, rounds and expansions (mean / max), the counts by return code.  The host planner
runs `host-sample` of the same poses on `threads` threads (the rest of the batch would only repeat the distribution), one warm-up call and `repeats` timed ones.  ipm_ms: DualMultWS + interior point of the same
poses at N = 80 from the device plans' warm starts, by the batch's own events.  No rate is a pass criterion."""
import argparse
import json
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import obca_amd
from obca_amd import api, planner as PL, scenarios as S


def spread(v):
    v = np.asarray(v, float)
    return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()), runs=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/hybrid_device_vs_host.json")
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--slots", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=256)
    ap.add_argument("--max-nodes", type=int, default=1 << 19)
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--no-ipm", action="store_true")
    a = ap.parse_args()
    ctx = api._ctx(0)
    out = dict(device=ctx.name(), bucket_width=api.HYBRID_DEFAULT_WIDTH, max_nodes=a.max_nodes, host_threads=a.threads, entries=[])
    for cfg in a.configs:
        sc = S.BACKWARDS if cfg == 2 else S.PARALLEL; name = sc["name"]
        kw, v_nom = PL.SCENARIO_OPTS[name]
        Ah, bh, vrows = S.scenario_hrep(sc); opts = PL._search_args(vrows, Ah, bh, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, kw)[7]
        for B in a.batches:
            x0, xF = S.sample_poses(sc, B, np.random.default_rng(3), goal_jitter=(cfg == 3))
            m = min(a.host_sample, B)
            ths = []
            for _ in range(a.repeats + 1):      # the first call warms up (library load, thread start, page faults of the cell tables) and is not counted
                t0 = time.perf_counter(); h = PL._hybrid_astar_dense(x0[:m], xF[:m], vrows, Ah, bh, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, a.threads, 1024, kw); ths.append(time.perf_counter() - t0)
            th = float(np.median(ths[1:]))
            host = dict(sample=m, wall_s=spread(ths[1:]), plans_per_s=m / th, expansions_mean=float(h[5].mean()), expansions_max=int(h[5].max()), no_path=int((h[4] <= 0).sum()))
            for slots in a.slots:
                api.hybrid_configure(slots=slots, max_nodes=a.max_nodes)
                args = (x0, xF, vrows, Ah, bh, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, opts, None, 1024)
                api.hybrid_astar_batch(*args)      # warm-up: the slots are allocated and cleared here
                kms, wall = [], []
                for _ in range(a.repeats):
                    t0 = time.perf_counter(); paths, dirs, cnt, nexp, rounds = api.hybrid_astar_batch(*args); wall.append(time.perf_counter() - t0); kms.append(api.hybrid_ms())
                e = dict(config=cfg, scenario=name, B=B, slots=slots, kernel_ms=spread(kms), call_wall_ms=spread(np.array(wall) * 1e3),
                         plans_per_s_kernel=B / (np.median(kms) * 1e-3), plans_per_s_call=B / np.median(wall), host=host,
                         ratio_to_host_call=B / np.median(wall) / host["plans_per_s"],
                         rounds_mean=float(rounds.mean()), rounds_max=int(rounds.max()), expansions_mean=float(nexp.mean()), expansions_max=int(nexp.max()),
                         counts={str(k): int((cnt == k).sum()) for k in (0, -1, -2, -3)}, with_path=int((cnt > 0).sum()))
                if not a.no_ipm and slots == a.slots[-1]:
                    N = 80
                    Ts, xWS, uWS, ok = PL.path_to_warm_start_many(paths, dirs, cnt, N, xF, v_nom=v_nom, device=ctx)
                    sel = np.flatnonzero(ok); n = len(sel)
                    x = xWS[sel].copy(); x[:, 0, :] = x0[sel]
                    b = obca_amd.Batch(ctx, n, N)
                    b.upload(x0[sel], xF[sel], Ts[sel], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, vrows, Ah, bh, x[:, :, 0], x[:, :, 1], x[:, :, 2], 0, x, uWS[sel])
                    b.solve(); o = b.download()
                    e.update(ipm_ms=b.kernel_ms()[0], dualws_ms=b.kernel_ms()[1], ipm_instances=n, ipm_solved=int((o["exitflag"] == 1).sum()), ipm_iterations_mean=float(o["iters"].mean()))
                    b.close()
                out["entries"].append(e)
                print(json.dumps(e), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
