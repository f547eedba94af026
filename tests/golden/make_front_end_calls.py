"""
Generates tests/golden/front_end_calls.json: what the Python front end built on top of the first ABI -- the planner routes of obca_amd.planner, the device search wrappers,
the timers, the refines and the resident planners of obca_amd.api -- hands to the C ABI, call by call and argument by argument, and what it returns.

The method is make_abi_calls.py's, and its stand-in, encoder and digest are imported from there.  Two things differ: the stand-in also takes the place of the HOST planner
library (planner._lib), so that no byte depends on a libm or a compiler, and it answers what the routes branch on: the counts of a search (a queue per call: -1 "longer than
cap", 0 "no path", -3 "outgrew its slot"), the return value of the single-instance search, the status of the device resampling, the cap a plan download reports.  The paths it
writes are straight lines along x with yaw 0 and the goals of the driver lie on that line with yaw 0, so that numpy's resampling of a re-searched path (path_to_warm_start)
is additions, multiplications and divisions only.

The record is the contract of the front end: it is produced by the code BEFORE a change of obca_amd/api.py or obca_amd/planner.py and compared with the code as it stands by
tests/test_front_end_cpu.py; it is never regenerated from the code under test.

Run from the repo root (a second):  python tests/golden/make_front_end_calls.py
"""
import json
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_abi_calls import B, N, StandIn, _array, declared, digest, seq      # noqa: E402 -- one stand-in, one encoder

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "front_end_calls.json")
HEADERS = ("obca_path_ws.h", "obca_clearance.h", "obca_refine.h", "obca_quad_subdivide.h", "obca_plan_device.h", "obca_plan_scenes.h", "obca_plan_resident.h",
           "obca_plan_resident_check.h", "obca_quad_plan_resident.h")      # the headers bound since abi_calls.json was recorded: every function of theirs is driven
SUPPORT = ("obca_hip.h", "obca_plan.h", "obca_plan3d.h")      # contexts and batches, the host planner, the quadcopter's grid planner: what the driven routes call besides
# name -> position of the counts array of a search
SEARCHES = {"obca_plan_hybrid_astar_batch2": 15, "obca_hybrid_astar_batch": 17, "obca_scene_astar_batch": 17, "obca_plan3d_paths_batch": 11}


def _line(paths, dirs):
    """a straight path along x at y = 1 with yaw 0, driven forwards: node k at x = k / 2"""
    paths[..., 0] = 0.5 * np.arange(paths.shape[-2]); paths[..., 1] = 1.0; paths[..., 2] = 0.0; dirs[...] = 1


class FrontEndStandIn(StandIn):
    """make_abi_calls' stand-in with the answers the planner routes branch on"""

    def __init__(self):
        super().__init__()
        self.sig = declared(HEADERS + SUPPORT)
        self.counts = []       # the counts the next searches answer, one list per call; without one every instance has a path of 3 nodes
        self.singles = []      # the return values of the next single-instance searches; without one 3

    def _call(self, name, args):
        rc = super()._call(name, args)
        if rc != 0 or name.endswith("last_error"):
            return rc
        if name in SEARCHES:
            cnt = _array(args[SEARCHES[name]]); cnt[:] = self.counts.pop(0) if self.counts else 3
            if name != "obca_plan3d_paths_batch":
                _line(_array(args[SEARCHES[name] - 3]), _array(args[SEARCHES[name] - 2]))
        elif name == "obca_plan_hybrid_astar2":
            _line(_array(args[11]), _array(args[12]))
            return self.singles.pop(0) if self.singles else 3
        elif name == "obca_parking_path_warm_start_batch":      # status: written where the instance has a path
            _array(args[14])[:] = np.where(_array(args[5]) >= 2, 0, -1)
        elif name in ("obca_batch_plan_download", "obca_quad_batch_grid_plan_download") and args[1] is None:
            return 4      # the cap of the last plan
        return rc


def drive(lib, opened):
    """every entry point of the front end through every branch that differs between its copies; returns [(label, digest of what it returned)]"""
    import obca_amd as OA
    from obca_amd import api, planner as PL, scenarios as S
    ret = []

    def run(label, f, *a, **kw):
        r = f(*a, **kw)
        ret.append([label, digest(r)])
        return r

    def raises(label, f, *a, fails=None, **kw):      # an exception, its type and its text; `fails`: the C call that answers -1
        lib.fail = fails
        try:
            f(*a, **kw)
            ret.append([label, None])
        except Exception as e:      # noqa: BLE001 -- type and text are what is recorded
            ret.append([label, [type(e).__name__, str(e)]])
        lib.fail = None

    def timer(label, f, *a):      # the values as well: the stand-in's are exact
        ret.append([label + " values", digest(np.asarray(run(label, f, *a), float))])

    def searches(label, f, *a, runs=("long", "none", "both long"), **kw):
        answers = {"long": ([[-1, 3]], [3]), "none": ([[0, -3]], []), "both long": ([[-1, -1], [0, 3]], [-2, 0])}      # (counts per search call, single-instance returns)
        for tag in runs:
            lib.counts, lib.singles = [list(c) for c in answers[tag][0]], list(answers[tag][1])
            run(f"{label}: {tag}", f, *a, **kw)
        lib.counts, lib.singles = [], []
    N1 = N + 1
    cx = OA.Context(1); opened.append(cx)

    # ---- the parking planner routes
    sc = S.BACKWARDS
    A, b, vrows = S.scenario_hrep(sc)
    x0 = np.array([[-2.0, 1.0, 0.0, 0.0], [-1.5, 1.0, 0.25, 0.0]]); xF = np.array([[4.0, 1.0, 0.0, 0.0], [5.0, 1.0, 0.0, 0.0]])      # goals on the stand-in's line, yaw 0
    more = dict(L=2.5, cap=16, xy_res=0.5)
    searches("hybrid_astar_many host", PL.hybrid_astar_many, x0, xF, vrows, A, b, threads=2, xy_res=0.5)
    searches("hybrid_astar_many device", PL.hybrid_astar_many, x0, xF, vrows, A, b, device=0, bucket_width=0.25, cap=8, max_steer=0.5)
    searches("hybrid_astar_many context", PL.hybrid_astar_many, x0, xF, vrows, A, b, S.EGO, 2.5, [-16.0, 16.0, 0.0, 12.0], device=cx, runs=("long",))
    searches("warm_start_many host", PL.warm_start_many, sc, x0, xF, N, workers=2, runs=("long", "none"), **more)      # (hybrid_astar_many's host route, driven above)
    searches("warm_start_many device, host search", PL.warm_start_many, sc, x0, xF, N, workers=2, device=0, **more)
    searches("warm_start_many device search", PL.warm_start_many, sc, x0, xF, N, device=0, search="device", bucket_width=0.25, **more)
    searches("warm_start_many parallel smooth context", PL.warm_start_many, S.PARALLEL, x0, xF, N, smooth=True, device=cx, search="device", runs=("long",))
    run("warm_start_many empty", PL.warm_start_many, sc, np.zeros((0, 4)), np.zeros((0, 4)), N, device=0, search="device")
    raises("warm_start_many search", PL.warm_start_many, None, x0, xF, N, search="gpu")      # (no scenario: the check comes first)
    raises("warm_start_many search needs a device", PL.warm_start_many, None, x0, xF, N, search="device")
    lists = dict(vOb=[[3, 4], [4]], A=[seq((7, 2), -1.0), seq((4, 2), 0.5)], b=[seq((7,), 2.0), seq((4,), 5.0)])
    shared = dict(vOb=[3, 4], A=seq((7, 2), -1.0), b=seq((7,), 2.0))
    for tag, ob, runs in (("lists", lists, ("long", "none", "both long")), ("shared", shared, ("long", "none"))):      # (the copies differ in the fields of the second call)
        searches(f"scene_astar_many {tag}", PL.scene_astar_many, x0, xF, ob["vOb"], ob["A"], ob["b"], device=0, bucket_width=0.25, cap=8, max_steer=0.5, runs=runs[:2])
        searches(f"scene_warm_start_many {tag}", PL.scene_warm_start_many, x0, xF, N, ob["vOb"], ob["A"], ob["b"], device=0, v_nom=0.25, runs=runs, **more)
    searches("scene_astar_many context", PL.scene_astar_many, x0, xF, lists["vOb"], lists["A"], lists["b"], S.EGO, 2.5, [-16.0, 16.0, 0.0, 12.0], device=cx, runs=("long",))
    searches("scene_warm_start_many smooth context", PL.scene_warm_start_many, x0, xF, N, lists["vOb"], lists["A"], lists["b"], device=cx, smooth=True, ego=[3.5, 1.0, 1.0, 1.0],
             XYbounds=[-16.0, 16.0, 0.0, 12.0], runs=("long",))
    run("scene_warm_start_many empty", PL.scene_warm_start_many, np.zeros((0, 4)), np.zeros((0, 4)), N, lists["vOb"], lists["A"], lists["b"])

    # ---- the device search wrappers and the context-level timers
    opts = np.array([PL.DEFAULT_OPTS[k] for k in PL.DEFAULT_OPTS], float)
    run("hybrid_astar_batch", api.hybrid_astar_batch, x0, xF, shared["vOb"], shared["A"], shared["b"], S.EGO, 2.75, S.XYBOUNDS)
    run("hybrid_astar_batch opts", api.hybrid_astar_batch, x0, xF, shared["vOb"], shared["A"], shared["b"], S.EGO, 2.75, S.XYBOUNDS, opts, 0.5, 4, cx)
    run("scene_astar_batch", api.scene_astar_batch, x0, xF, lists["vOb"], lists["A"], lists["b"], S.EGO, 2.75, S.XYBOUNDS)
    run("scene_astar_batch opts", api.scene_astar_batch, x0, xF, shared["vOb"], shared["A"], shared["b"], S.EGO, 2.75, S.XYBOUNDS, opts, 0.5, 4, cx)
    raises("hybrid_astar_batch refused", api.hybrid_astar_batch, x0, xF, shared["vOb"], shared["A"], shared["b"], S.EGO, 2.75, S.XYBOUNDS, fails="obca_hybrid_astar_batch")
    raises("scene_astar_batch refused", api.scene_astar_batch, x0, xF, shared["vOb"], shared["A"], shared["b"], S.EGO, 2.75, S.XYBOUNDS, fails="obca_scene_astar_batch")
    run("hybrid_configure", api.hybrid_configure, 4, 1024, 64, device=cx)
    timer("hybrid_ms", api.hybrid_ms, 0); timer("scene_ms", api.scene_ms, cx)
    raises("hybrid_ms refused", api.hybrid_ms, cx, fails="obca_hybrid_ms"); raises("scene_ms refused", api.scene_ms, 0, fails="obca_scene_astar_ms")

    # ---- the parking batch: timers, the resident planner, refine
    ego, XYb, L = [3.5, 1.0, 1.0, 1.0], [-15.0, 15.0, 1.0, 10.0], 2.75
    p0, pF = seq((B, 4), -2.0), seq((B, 4), 1.0)
    rx, ry, ryaw = seq((B, N1), 0.25), seq((B, N1), 3.0), seq((B, N1), -0.5)
    xWS, uWS = seq((B, N1, 4), 0.5), seq((B, N, 2), -1.0)
    bt = OA.Batch(cx, B, N); opened.append(bt)
    bt.upload(p0, pF, 0.5, L, ego, XYb, lists["vOb"], lists["A"], lists["b"], rx, ry, ryaw, 0, xWS, uWS)
    for t in ("validate_ms", "clearance_ms", "path_ws_ms", "refine_ms", "plan_ms", "kernel_ms"):
        timer(t, getattr(bt, t))
    raises("plan_ms refused", bt.plan_ms, fails="obca_batch_plan_ms")
    paths, dirs = np.zeros((B, 4, 3)), np.zeros((B, 4), np.int32); _line(paths, dirs)
    run("set_path_warm_start", bt.set_path_warm_start, paths, dirs, [3, 0], v_nom=0.25, smooth=True, use_xF=False)
    run("clearance", bt.clearance, 2, 0.25)
    run("plan_warm_start", bt.plan_warm_start)
    run("plan_warm_start options", bt.plan_warm_start, 0.25, 16, 0.25, True, False, xy_res=0.5, max_steer=0.5)
    run("plan_paths", bt.plan_paths); run("plan_block", bt.plan_block)
    raises("plan_paths refused", bt.plan_paths, fails="obca_batch_plan_download")
    given = OA.Batch(cx, 3, 2 * N); opened.append(given)
    for tag, sel in (("all", None), ("mask", np.array([False, True])), ("indices", [1, 0, 1])):
        dst, st = run(f"refine {tag}", bt.refine, 2, sel, duals=tag == "mask")
        run(f"refine {tag}: records", lambda: (dst.B, dst.capacity, dst.N, dst.nObs, dst.Ms, dst.vflat)); dst.close()
        dst, st = run(f"refine {tag} into", bt.refine, 2, sel, True, given)
        run(f"refine {tag} into: records", lambda: (dst is given, dst.B, dst.capacity, dst.N, dst.nObs, dst.Ms, dst.vflat))
    raises("refine refused", bt.refine, 3, fails="obca_batch_refine_into")                    # the fresh destination is destroyed ...
    raises("refine into refused", bt.refine, 2, into=given, fails="obca_batch_refine_into")   # ... a given one is not
    raises("refine empty", bt.refine, 2, np.array([False, False])); raises("refine empty indices", bt.refine, 2, [])
    raises("refine index", bt.refine, 2, [0, 2]); raises("refine negative index", bt.refine, 2, [-1]); raises("refine index into", bt.refine, 2, [2], into=given)
    raises("refine factor", bt.refine, api.REFINE_MAXFACTOR + 1); raises("refine factor 0", bt.refine, 0)
    run("refine factor into", bt.refine, api.REFINE_MAXFACTOR + 1, into=given)      # (with a given batch the library is the one that checks the factor)
    timer("refine_ms of the destination", given.refine_ms)
    given.close(); bt.close()
    x, u = seq((B, 4, N1), 0.0), seq((B, 2, N), 1.0)
    run("parking_refine_batch", api.parking_refine_batch, N, 0.5, L, x, u)
    run("parking_refine_batch ts", api.parking_refine_batch, N, np.array([0.5, 0.75]), L, x, u, timeScale=seq((B, N1), 1.0), factor=3, device=cx)
    run("parking_clearance_batch", api.parking_clearance_batch, N, 0.5, L, ego, lists["vOb"], lists["A"], lists["b"], x, u, timeScale=1.25, substeps=2, need=0.25, device=cx)
    run("parking_clearance_batch shared", api.parking_clearance_batch, N, 0.5, L, ego, shared["vOb"], shared["A"], shared["b"], x, u)
    run("path_to_warm_start_many", PL.path_to_warm_start_many, paths, dirs, np.array([3, 0], np.int32), N, device=cx)
    raises("path_to_warm_start_many shapes", PL.path_to_warm_start_many, paths[:, :, :2], dirs, [3, 0], N, device=cx)

    # ---- the quadcopter batch: timers, the resident planner, refine
    R = 0.25
    q0, qF = seq((B, 12), 0.0), seq((B, 12), 4.0)
    ob1, obB = seq((5, 6), 1.0), seq((B, 5, 6), 2.0)
    qWS = seq((B, N1, 12), 0.5)
    qb = OA.QuadBatch(cx, B, N); opened.append(qb)
    qb.upload(q0, qF, 0.5, R, ob1, qWS, 1.0)
    for t in ("validate_ms", "clearance_ms", "plan_ms", "refine_ms", "kernel_ms"):
        timer("quad " + t, getattr(qb, t))
    raises("quad kernel_ms refused", qb.kernel_ms, fails="obca_quad_batch_kernel_ms")
    run("quad clearance", qb.clearance, 2, 0.25)
    for tag, sel in (("all", None), ("mask", np.array([False, True])), ("indices", [1, 0])):
        run(f"quad plan_warm_start {tag}", qb.plan_warm_start, select=sel, **({} if sel is None else dict(clear=0.5, room=(8.0, 8.0, 4.0), res=0.5, cap=64, timeWS=1.25)))
    run("quad plan_warm_start outside", qb.plan_warm_start, select=[5])      # (no range check here: the library refuses a bad index)
    raises("quad plan_warm_start empty", qb.plan_warm_start, select=np.array([False, False]))
    raises("quad plan_warm_start refused", qb.plan_warm_start, select=[5], fails="obca_quad_batch_grid_plan_warm_start")
    run("quad plan_paths", qb.plan_paths); run("quad warm_start", qb.warm_start)
    raises("quad plan_paths refused", qb.plan_paths, fails="obca_quad_batch_grid_plan_download")
    qgiven = OA.QuadBatch(cx, 3, 2 * N); opened.append(qgiven)
    for tag, sel in (("all", None), ("mask", np.array([False, True])), ("indices", [1, 0, 1])):
        dst, st = run(f"quad refine {tag}", qb.refine, 2, sel, margin=0.25 if tag == "mask" else 0.0)
        run(f"quad refine {tag}: records", lambda: (dst.B, dst.capacity, dst.N)); dst.close()
        dst, st = run(f"quad refine {tag} into", qb.refine, 2, sel, 0.5, qgiven)
        run(f"quad refine {tag} into: records", lambda: (dst is qgiven, dst.B, dst.capacity, dst.N))
    raises("quad refine refused", qb.refine, 3, fails="obca_quad_batch_subdivide_into")
    raises("quad refine into refused", qb.refine, 2, into=qgiven, fails="obca_quad_batch_subdivide_into")
    raises("quad refine empty", qb.refine, 2, np.array([False, False])); raises("quad refine index", qb.refine, 2, [0, 2]); raises("quad refine index into", qb.refine, 2, [-1], into=qgiven)
    raises("quad refine factor", qb.refine, api.QUAD_SUBDIVIDE_MAXFACTOR + 1); raises("quad refine factor 0", qb.refine, 0)
    run("quad refine factor into", qb.refine, api.QUAD_SUBDIVIDE_MAXFACTOR + 1, into=qgiven)
    timer("quad refine_ms of the destination", qgiven.refine_ms)
    qgiven.close(); qb.close()
    qx = seq((B, 12, N1), 0.0)
    run("quadcopter_refine_batch", api.quadcopter_refine_batch, qx, None, 0.5)
    run("quadcopter_refine_batch ts", api.quadcopter_refine_batch, qx, np.array([1.0, 1.5]), np.array([0.5, 0.75]), factor=3, device=cx)
    run("quadcopter_clearance_batch", api.quadcopter_clearance_batch, qx, None, 0.5, ob1, R)
    run("quadcopter_clearance_batch ts", api.quadcopter_clearance_batch, qx, seq((B, N1), 1.0), np.array([0.5, 0.75]), obB, R, substeps=2, need=0.25, device=cx)

    # ---- the quadcopter's grid planner with its long-path second call
    lib.counts = [[-1, 3]]
    run("astar3d_many", PL.astar3d_many, q0, qF, boxes=obB[:, :2], clear=0.5, room=(8.0, 8.0, 4.0), res=0.5, device=1)
    lib.counts = [[1, 0]]
    run("astar3d_many none", PL.astar3d_many, q0, qF)
    lib.counts = [[-1, -3], [2]]
    raises("astar3d_many unsettled", PL.astar3d_many, q0, qF)
    lib.counts = []

    cx.close()
    for c in api._default_ctx.values():      # the cached contexts of the `device=` arguments: closed here, not when the collector gets to them
        c.close()
    return ret


def record():
    """(stand-in after the drive, what the Python calls returned); the package's libraries are put back afterwards"""
    from obca_amd import api, planner as PL
    lib = FrontEndStandIn()
    saved = (api._lib, api._default_ctx, PL._lib, PL._lib3d, PL._ctx3d)
    api._lib, api._default_ctx, PL._lib, PL._lib3d, PL._ctx3d = lib, {}, lib, lib, {}
    opened = []
    try:
        ret = drive(lib, opened)
    finally:
        for o in opened + list(api._default_ctx.values()):      # (after a failure: nothing that holds a stand-in handle may reach the real library's destroy)
            o.close()
        api._lib, api._default_ctx, PL._lib, PL._lib3d, PL._ctx3d = saved
    return lib, ret


def main():
    lib, ret = record()
    with open(OUT, "w") as f:
        json.dump(dict(B=B, N=N, calls=lib.calls, returns=ret), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, len(lib.calls), "calls of", len({c[0] for c in lib.calls}), "entry points,", len(ret), "Python calls")


if __name__ == "__main__":
    main()
