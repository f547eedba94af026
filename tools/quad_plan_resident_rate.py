"""Wall time of the two routes from the end points of a quadcopter batch to a batch that is uploaded WITH its planned warm start (include/obca_quad_plan_resident.h):

    resident   : QuadBatch.plan_warm_start on the uploaded batch -- the search and the resampling on the device, two ints per instance down
    round trip : planner.quad_warm_start_many (x0, xF, boxes up to the planner's own context, xWS down) + QuadBatch.upload (the same xWS up again)

    python tools/quad_plan_resident_rate.py [--out profiles/quad_plan_resident_vs_round_trip.json] [--batches 256 1024] [--repeats 3] [--horizon 60]

The end points are scenarios.make_quad_batch(B, N, random_endpoints=True)'s (every instance has a path; instance 0 is the shipped one), the boxes the shipped five.  Per
batch size: one warm-up call of each route (contexts, buffers, the LDS attribute), then `repeats` timed calls of each, alternating -- wall clock around the Python calls,
the kernel time of plan_ms() and of quad_warm_start_many(with_ms=True), each as minimum / median / maximum -- and the bytes each route moves over the bus, COMPUTED from
the sizes of the arrays the calls send and fetch, not counted on the bus: every entry says so.  The resident route plans a batch that is ALREADY uploaded (the case of a
replan); what that upload costs is recorded beside it (upload_before_resident_wall_ms).  Then the batch is solved from the resident start (ipm_ms, exit flags).
The search is the same kernel text on both routes.  An entry is appended to --out as soon as it is measured.  No number is a pass criterion."""
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
    ap.add_argument("--out", default="profiles/quad_plan_resident_vs_round_trip.json")
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=60)
    a = ap.parse_args()
    ctx = api._ctx(0); N = a.horizon; cap = PL.PLAN3D_WS_CAP
    out = json.load(open(a.out)) if os.path.exists(a.out) else dict(device=ctx.name(), horizon=N, cap=cap, clear=0.4, res=0.25, room=list(PL.QUAD_ROOM), entries=[])
    for B in a.batches:
        q = S.make_quad_batch(B, N, random_endpoints=True, device=0)
        x0, xF = q["x0"], q["xF"]; Ts = S.quad_sample_time(N)
        zeros = np.zeros((B, N + 1, 12))
        qb = obca_amd.QuadBatch(ctx, B, N)
        qb.upload(x0, xF, Ts, S.QUAD_R, S.QUAD_OB, zeros, 1.0)      # what the resident route starts from: a batch that holds the problem, no start yet
        t0 = time.perf_counter(); qb.upload(x0, xF, Ts, S.QUAD_R, S.QUAD_OB, zeros, 1.0); first_upload = (time.perf_counter() - t0) * 1e3      # (the second one: buffers exist)
        other = obca_amd.QuadBatch(ctx, B, N)                        # the round trip uploads into a batch of its own

        def resident():
            t0 = time.perf_counter(); r = qb.plan_warm_start(timeWS=1.0); return (time.perf_counter() - t0) * 1e3, r

        def round_trip():
            t0 = time.perf_counter()
            xws, ok, kms = PL.quad_warm_start_many(x0, xF, N, with_ms=True)
            t1 = time.perf_counter()
            other.upload(x0, xF, Ts, S.QUAD_R, S.QUAD_OB, xws, 1.0)
            return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, kms, xws, ok
        resident(); round_trip()      # warm-up
        res = dict(wall=[], kernel=[]); rt = dict(wall=[], plan_wall=[], upload_wall=[], kernel=[])
        for _ in range(a.repeats):
            w, (cnt, sw) = resident()
            res["wall"].append(w); res["kernel"].append(qb.plan_ms())
            w, w1, w2, kms, xws, ok = round_trip()
            rt["wall"].append(w); rt["plan_wall"].append(w1); rt["upload_wall"].append(w2); rt["kernel"].append(kms)
        same = bool(np.array_equal(qb.warm_start()[0][ok], xws[ok]) and np.array_equal(cnt >= 2, ok))
        qb.solve(); ipm_ms = qb.kernel_ms(); ef = qb.download()["exitflag"]
        nws = B * (N + 1) * 12 * 8
        e = dict(B=B, N=N,
                 upload_before_resident_wall_ms=first_upload,      # a batch planned for the FIRST time needs this upload too; a replanned one (failed solves, moved end points) does not
                 resident=dict(wall_ms=spread(res["wall"]), kernel_ms=spread(res["kernel"]),
                               bytes_up=4 * B + 2 * 4 * B, bytes_down=2 * 4 * B),      # up: the selection and the preset counts and sweeps; down: counts and sweeps
                 round_trip=dict(wall_ms=spread(rt["wall"]), plan_wall_ms=spread(rt["plan_wall"]), upload_wall_ms=spread(rt["upload_wall"]), kernel_ms=spread(rt["kernel"]),
                                 # planner: start, goal and five boxes per instance up, xWS and counts + sweeps down; upload: the whole problem record per instance up
                                 bytes_up=int(B * 36 * 8 + B * (64 + (N + 1) * 12) * 8), bytes_down=int(nws + 2 * 4 * B)),
                 bytes="computed from the sizes of the arrays each call sends and fetches (the staging layouts of obca_hip.hip and obca_plan3d.hip), not measured",
                 wall_ratio_round_trip_over_resident=float(np.median(rt["wall"]) / np.median(res["wall"])),
                 same_warm_start=same, with_path=int((cnt >= 2).sum()), way_points_mean=float(cnt[cnt >= 2].mean()), way_points_max=int(cnt.max()),
                 sweeps_mean=float(sw.mean()), sweeps_max=int(sw.max()),
                 ipm_ms=ipm_ms, solved=int((ef == 1).sum()), failed=int((ef == 0).sum()))
        qb.close(); other.close()
        out["entries"].append(e)
        print(json.dumps(e), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
