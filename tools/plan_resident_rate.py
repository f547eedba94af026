"""Wall time of the two routes from an UPLOADED batch to its planned warm start (include/obca_plan_resident.h):

    resident   : Batch.plan_warm_start -- packing, search and warm start on the device, four ints per instance down
    round trip : api.scene_astar_batch (poses and fields up, paths down) + Batch.set_path_warm_start (paths up again) on the same uploaded batch

    python tools/plan_resident_rate.py [--out profiles/plan_resident_vs_round_trip.json] [--batches 1024 4096] [--slots 256] [--repeats 3] [--horizon 80]

The inputs are scenarios.scene_inputs' (the backwards poses, 1-3 boxes on the road per instance), as tools/scene_rate.py takes them.  Per batch size: one warm-up call of
each route (allocates the slots and the staging), then `repeats` timed calls of each, alternating -- wall clock around the Python call, the three kernel times of plan_ms(),
scene_ms() and path_ws_ms() of the round trip, each with its spread -- and the bytes each route moves over the bus, COMPUTED from the sizes of the arrays the calls send and
fetch (the library's staging layout), not counted on the bus: every entry says so.  The search is the same kernel on both routes: the
two search times should agree within the spread profiles/scene_plan_device_vs_host.json records for it.  An entry is appended to --out as soon as it is measured.  No
number is a pass criterion."""
import argparse
import json
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import obca_amd
from obca_amd import api, planner as PL, scenarios as S


PARAMS_BYTES = 1288      # sizeof(hy::Params) of obca_amd/csrc/obca_hybrid.h, the one block the resident call sends (obca_hip.hip asserts the number where it sends it)


def spread(v):
    v = np.asarray(v, float)
    return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()), runs=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/plan_resident_vs_round_trip.json")
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=80)
    ap.add_argument("--max-nodes", type=int, default=1 << 19)
    a = ap.parse_args()
    ctx = api._ctx(0); N = a.horizon; cap = 1024
    out = json.load(open(a.out)) if os.path.exists(a.out) else dict(device=ctx.name(), bucket_width=api.HYBRID_DEFAULT_WIDTH, max_nodes=a.max_nodes, horizon=N, cap=cap, entries=[])
    kw, v_nom = PL.SCENARIO_OPTS["backwards"]
    o = dict(PL.DEFAULT_OPTS); o.update(kw); opts = np.array([o[k] for k in PL.DEFAULT_OPTS], float)
    for B in a.batches:
        _, x0, xF, fields = S.scene_inputs(B)
        vl, Al, bl = [f[0] for f in fields], [f[1] for f in fields], [f[2] for f in fields]
        rows = int(sum(int(np.sum(v)) for v in vl)); obstacles = int(sum(len(v) for v in vl))
        api.hybrid_configure(slots=a.slots, max_nodes=a.max_nodes)
        z = np.zeros((B, N + 1))
        b = obca_amd.Batch(ctx, B, N)
        b.upload(x0, xF, np.full(B, 0.6), S.L_WHEELBASE, S.EGO, S.XYBOUNDS, vl, Al, bl, z, z, z, 0, None, None)

        def resident():
            t0 = time.perf_counter(); r = b.plan_warm_start(v_nom=v_nom, cap=cap, **kw); return (time.perf_counter() - t0) * 1e3, r

        def round_trip():
            t0 = time.perf_counter()
            paths, dirs, cnt, nexp, rounds = api.scene_astar_batch(x0, xF, vl, Al, bl, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, opts, None, cap)
            t1 = time.perf_counter()
            st = b.set_path_warm_start(paths, dirs, cnt, v_nom=v_nom)
            return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, (cnt, st, nexp, rounds)
        resident(); round_trip()      # warm-up: slots, staging, pinned mirrors
        res = dict(wall=[], pack=[], search=[], ws=[]); rt = dict(wall=[], search_call=[], search=[], ws=[])
        for _ in range(a.repeats):
            w, r = resident(); ms = b.plan_ms()
            res["wall"].append(w); res["pack"].append(ms[0]); res["search"].append(ms[1]); res["ws"].append(ms[2])
            w, w1, q = round_trip()
            rt["wall"].append(w); rt["search_call"].append(w1); rt["search"].append(api.scene_ms()); rt["ws"].append(b.path_ws_ms())
        usable = int(((q[0] >= 2) & (q[0] <= cap)).sum()); longest = int(q[0].max())
        e = dict(B=B, slots=a.slots, obstacles_mean=obstacles / B, rows_mean=rows / B,
                 resident=dict(wall_ms=spread(res["wall"]), pack_ms=spread(res["pack"]), search_ms=spread(res["search"]), ws_ms=spread(res["ws"]),
                               bytes_up=PARAMS_BYTES, bytes_down=4 * 4 * B),      # up: the search's parameter block; down: counts, expansions, rounds, status
                 round_trip=dict(wall_ms=spread(rt["wall"]), search_call_wall_ms=spread(rt["search_call"]), search_ms=spread(rt["search"]), ws_ms=spread(rt["ws"]),
                                 # up: poses 2 x B x 3 doubles, rows 3 doubles each, counts; then the paths' rows below the longest count, their dirs and counts
                                 bytes_up=int(B * 48 + rows * 24 + (obstacles + B) * 4 + B * longest * 28 + B * 4),
                                 bytes_down=int(B * cap * 28 + 3 * 4 * B + 4 * B)),
                 bytes="computed from the sizes of the arrays each call sends and fetches (the staging layout of obca_hip.hip; the parameter block: %d bytes, sizeof hy::Params), not measured" % PARAMS_BYTES,
                 wall_ratio_round_trip_over_resident=float(np.median(rt["wall"]) / np.median(res["wall"])),
                 same_counts=bool(np.array_equal(r[0], q[0])), same_status=bool(np.array_equal(r[1], q[1])), instances_differing_in_counts=int((r[0] != q[0]).sum()),
                 with_path=usable, counts={str(k): int((r[0] == k).sum()) for k in (0, -1, -2, -3)}, status_written=int((r[1] == 0).sum()),
                 rounds_mean=float(r[3].mean()), rounds_max=int(r[3].max()), expansions_mean=float(r[2].mean()), expansions_max=int(r[2].max()))
        b.close()
        out["entries"].append(e)
        print(json.dumps(e), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
