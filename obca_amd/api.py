"""
ctypes binding of libobca_hip.so and the Python mirror of the reference's entry points for the signed-distance path:

    ParkingSignedDist(x0,xF,N,Ts,L,ego,XYbounds,nOb,vOb,A,b,rx,ry,ryaw,fixTime,xWS,uWS)
        -> xp (4,N+1), up (2,N), timeScale, exitflag, time, lp (M,N+1), np (4nOb,N+1)
        same positional arguments, shapes and exit-flag meaning as
        /root/reference/AutonomousParking/ParkingSignedDist.jl:29,297-313
    DualMultWS(N,nOb,vOb,A,b,rx,ry,ryaw, ego) -> lp (N+1,M), np (N+1,4nOb)
        /root/reference/AutonomousParking/DualMultWS.jl:29,81-84 (the reference reads `ego` from global scope, :39-45)

    QuadcopterSignedDist(x0,xF,N,Ts,R,ob1,ob2,ob3,ob4,ob5,xWS,uWS,timeWS)
        -> xp (12,N+1), up (4,N), timeScale, exitflag, time, lp (30,N+1), status string
        /root/reference/QuadcopterNavigation/QuadcopterSignedDist.jl:25,298

plus batched variants (leading batch dimension) that keep everything resident on the GPU between upload and download.
"""
import ctypes as C
import numbers
import os
import time
import numpy as np
from . import buildflags, cabi, planner
from .cabi import Opts      # `typedef struct obca_opts` of include/obca_hip.h, read from the header
from .validate import (VIOL_NAMES, QUAD_VIOL_NAMES, DMIN, CLR_OUT, ROLL_OUT, TRK_OUT, TRACK_Q_PARKING, TRACK_R_PARKING, TRACK_QF_PARKING, TRACK_Q_QUAD, TRACK_R_QUAD,
                       TRACK_QF_QUAD, ENS_MEM, ENS_OUT, ENS_MMAX, CERT_OUT, CERT_TICKS, ADV_OUT, PRD_OUT)

_LIBPATH = os.environ.get("OBCA_HIP_LIBRARY") or buildflags.PIECES["hip"].out   # override: diagnostic builds
_lib = None


class ObcaError(RuntimeError):
    pass


def library_path():
    return _LIBPATH


def build_library(force=False):
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    return buildflags.build("hip", force, out=_LIBPATH)      # the flags (warnings are errors), the dependency rule and why: obca_amd/buildflags.py


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIBPATH):
        raise ObcaError(f"{_LIBPATH} is missing: build it with obca_amd.build_library() / __graft_entry__.build(); "
                        "there is no CPU fallback")
    # The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and serialises the launches that share one: with more than four
    # batches in flight the extra streams bought nothing (rounds 3-6: 4 / 8 / 12 streams gave the same rate).  16 queues: +6 % on config 2, +8 % on config 3 with 16
    # batches in flight (profiles/r06_hw_queues.txt).  Read by the runtime at its first call in the process; a value the caller has set stays.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    _lib = cabi.bind(C.CDLL(_LIBPATH), "obca_hip.h")      # every prototype of the header: the call sites below pass numbers and prepared arrays
    cabi.bind(_lib, "obca_path_ws.h")                     # the warm start from planner paths: the same library, a header of its own
    cabi.bind(_lib, "obca_clearance.h")                   # the clearance between the nodes: likewise
    cabi.bind(_lib, "obca_refine.h")                      # solved batches on a finer horizon: likewise
    cabi.bind(_lib, "obca_quad_subdivide.h")              # ... and solved quadcopter batches
    cabi.bind(_lib, "obca_plan_device.h")                 # the parking planner on the device
    cabi.bind(_lib, "obca_plan_scenes.h")                 # ... in per-instance obstacle fields
    cabi.bind(_lib, "obca_plan_resident.h")               # ... from the records of an uploaded batch
    cabi.bind(_lib, "obca_plan_resident_check.h")         # ... and the diagnostic that hands out what its packing kernel wrote
    cabi.bind(_lib, "obca_quad_plan_resident.h")          # the quadcopter's grid planner from the records of an uploaded batch
    cabi.bind(_lib, "obca_rollout.h")                     # solved batches applied to the continuous vehicle models
    cabi.bind(_lib, "obca_track.h")                       # ... and tracked on them by a time-varying LQR
    cabi.bind(_lib, "obca_ensemble.h")                    # ... from a spread of start offsets and input biases at once
    cabi.bind(_lib, "obca_advance.h")                     # the closed loop: the plant advanced under a solution and the next solve restarted from where it got
    cabi.bind(_lib, "obca_scene_edit.h")                  # the obstacles of a resident batch moved and inflated in place
    cabi.bind(_lib, "obca_certify.h")                     # the clearance certified along the whole path
    cabi.bind(_lib, "obca_predict.h")                     # the clearance of a held plan against obstacles that move
    return _lib


EXPORTS = ["obca_create", "obca_create_multi", "obca_device_count", "obca_visible_device_count", "obca_destroy", "obca_last_error", "obca_default_opts", "obca_reference_opts", "obca_device_name",
           "obca_dualmult_ws_batch", "obca_parking_signed_dist_batch", "obca_parking_dist_batch", "obca_batch_create", "obca_batch_destroy",
           "obca_batch_set_formulation", "obca_batch_shift_warm_start",
           "obca_batch_upload", "obca_batch_solve", "obca_batch_sync", "obca_batch_kernel_ms", "obca_batch_last_schedule", "obca_batch_download",
           "obca_batch_scratch_bytes", "obca_batch_validate", "obca_batch_validate_ms", "obca_parking_constraints_batch",
           "obca_quad_batch_validate", "obca_quad_batch_validate_ms", "obca_quadcopter_constr_satisfaction_batch",
           "obca_quadcopter_default_opts", "obca_quadcopter_reference_opts", "obca_quadcopter_signed_dist_batch", "obca_quadcopter_dist_batch", "obca_quad_batch_create", "obca_quad_batch_destroy",
           "obca_quad_batch_upload", "obca_quad_batch_solve", "obca_quad_batch_sync", "obca_quad_batch_shift_warm_start", "obca_quad_batch_kernel_ms",
           "obca_quad_batch_download", "obca_quad_batch_scratch_bytes"]
# include/obca_path_ws.h: warm starts from planner paths on the device (planner.path_to_warm_start_many, Batch.set_path_warm_start)
PATH_WS_EXPORTS = ["obca_parking_path_warm_start_batch", "obca_batch_set_path_warm_start", "obca_batch_path_ws_ms"]
PATH_WS_MAXNODES = 1024      # OBCA_PATH_WS_MAXNODES
# include/obca_clearance.h: clearance of trajectories between their nodes (Batch.clearance, QuadBatch.clearance, parking_clearance_batch, quadcopter_clearance_batch)
CLEARANCE_EXPORTS = ["obca_batch_clearance", "obca_batch_clearance_ms", "obca_parking_clearance_batch", "obca_quad_batch_clearance", "obca_quad_batch_clearance_ms",
                     "obca_quadcopter_clearance_batch"]
# include/obca_refine.h: solved parking batches on a finer horizon (Batch.refine, parking_refine_batch)
REFINE_EXPORTS = ["obca_batch_refine_into", "obca_batch_refine_ms", "obca_parking_refine_batch"]
REFINE_MAXFACTOR = 32      # OBCA_REFINE_MAXFACTOR
# include/obca_quad_subdivide.h: solved quadcopter batches on a finer horizon (QuadBatch.refine, quadcopter_refine_batch)
QUAD_SUBDIVIDE_EXPORTS = ["obca_quad_batch_subdivide_into", "obca_quad_batch_subdivide_ms", "obca_quadcopter_subdivide_batch"]
QUAD_SUBDIVIDE_MAXFACTOR = 32      # OBCA_QUAD_SUBDIVIDE_MAXFACTOR
# include/obca_plan_device.h: the parking planner on the device (planner.hybrid_astar_many(device=...), planner.warm_start_many(search="device"), hybrid_configure, hybrid_ms)
PLAN_DEVICE_EXPORTS = ["obca_hybrid_configure", "obca_hybrid_astar_batch", "obca_hybrid_ms"]
HYBRID_MAXMAP, HYBRID_MAXCELLS, HYBRID_MAXSLOTS, HYBRID_MAXNODES, HYBRID_DEFAULT_WIDTH = 35000, 6000000, 256, 1 << 20, 0.2      # the limits of include/obca_plan_device.h
HYBRID_STATUS = {0: "no path", -1: "more nodes than cap", -2: "the start or goal pose collides", -3: "a sizing limit of the slot was hit (node pool, chunk pool)"}
# include/obca_plan_scenes.h: the same planner, every search in the obstacle field of its own instance (scene_astar_batch, scene_ms, planner.scene_astar_many,
# planner.scene_warm_start_many, scenarios.make_scene_batch(device=...)); slots, pools and status codes are the shared-field planner's
SCENE_EXPORTS = ["obca_scene_astar_batch", "obca_scene_astar_ms"]
# include/obca_plan_resident.h: the same search from what an uploaded batch holds, its paths straight into the batch's warm start (Batch.plan_warm_start, plan_ms, plan_paths)
PLAN_RESIDENT_EXPORTS = ["obca_batch_plan_warm_start", "obca_batch_plan_ms", "obca_batch_plan_download"]
PLAN_RESIDENT_CHECK_EXPORTS = ["obca_batch_packed_block"]      # include/obca_plan_resident_check.h: a diagnostic (Batch.plan_block)
# include/obca_quad_plan_resident.h: the quadcopter's 3-D grid search from what an uploaded batch holds, its resampled path straight into the batch's warm start
# (QuadBatch.plan_warm_start, plan_ms, plan_paths), and the read-back of the start a batch will solve from (QuadBatch.warm_start)
QUAD_PLAN_RESIDENT_EXPORTS = ["obca_quad_batch_grid_plan_warm_start", "obca_quad_batch_grid_plan_ms", "obca_quad_batch_grid_plan_download", "obca_quad_batch_start_download"]
QUAD_PLAN_SKIPPED = -4      # OBCA_QUAD_PLAN_SKIPPED
# include/obca_rollout.h: solutions and trajectories on the continuous vehicle models (Batch.rollout, QuadBatch.rollout, rollout_states, rollout_ms, parking_rollout_batch,
# quadcopter_rollout_batch)
ROLLOUT_EXPORTS = ["obca_batch_rollout", "obca_batch_rollout_ms", "obca_batch_rollout_states", "obca_parking_rollout_batch", "obca_quad_batch_rollout",
                   "obca_quad_batch_rollout_ms", "obca_quad_batch_rollout_states", "obca_quadcopter_rollout_batch"]
# include/obca_track.h: TVLQR gains about solutions and trajectories and the closed loop on the continuous vehicle models (Batch.track, QuadBatch.track, track_states,
# track_gains, track_ms, parking_track_batch, quadcopter_track_batch)
TRACK_EXPORTS = ["obca_batch_track", "obca_batch_track_ms", "obca_batch_track_states", "obca_batch_track_gains", "obca_parking_track_batch", "obca_quad_batch_track",
                 "obca_quad_batch_track_ms", "obca_quad_batch_track_states", "obca_quad_batch_track_gains", "obca_quadcopter_track_batch"]
# include/obca_ensemble.h: up to 64 disturbed closed loops about every solution or trajectory at once, one member per lane (Batch.ensemble, QuadBatch.ensemble,
# ensemble_members, ensemble_final, ensemble_ms, parking_ensemble_batch, quadcopter_ensemble_batch)
ENSEMBLE_EXPORTS = ["obca_batch_ensemble", "obca_batch_ensemble_ms", "obca_batch_ensemble_members", "obca_batch_ensemble_final", "obca_parking_ensemble_batch",
                    "obca_quad_batch_ensemble", "obca_quad_batch_ensemble_ms", "obca_quad_batch_ensemble_members", "obca_quad_batch_ensemble_final", "obca_quadcopter_ensemble_batch"]
# include/obca_advance.h: one step of the closed receding-horizon loop on the device (Batch.advance, QuadBatch.advance, advance_state, advance_log, advance_log_states,
# advance_ms)
ADVANCE_EXPORTS = ["obca_batch_advance", "obca_batch_advance_ms", "obca_batch_advance_state", "obca_batch_advance_log", "obca_batch_advance_log_states",
                   "obca_quad_batch_advance", "obca_quad_batch_advance_ms", "obca_quad_batch_advance_state", "obca_quad_batch_advance_log", "obca_quad_batch_advance_log_states"]
# include/obca_scene_edit.h: the obstacles of a resident batch moved and inflated on the device (Batch.move_obstacles, QuadBatch.move_obstacles, obstacles, move_obstacles_ms)
SCENE_EDIT_EXPORTS = ["obca_batch_move_obstacles", "obca_batch_move_obstacles_ms", "obca_batch_obstacles_download",
                      "obca_quad_batch_move_obstacles", "obca_quad_batch_move_obstacles_ms", "obca_quad_batch_obstacles_download"]
# include/obca_certify.h: the clearance of solutions and trajectories certified along the whole path by conservative advancement (Batch.certify, QuadBatch.certify,
# certify_intervals, certify_ms, parking_certify_batch, quadcopter_certify_batch)
CERTIFY_EXPORTS = ["obca_batch_certify", "obca_batch_certify_ms", "obca_batch_certify_intervals", "obca_parking_certify_batch", "obca_quad_batch_certify",
                   "obca_quad_batch_certify_ms", "obca_quad_batch_certify_intervals", "obca_quadcopter_certify_batch"]
# include/obca_predict.h: the clearance of held solutions and trajectories against obstacles that move at given rates (Batch.predict_clearance, QuadBatch.predict_clearance,
# predict_profile, predict_clearance_ms, parking_predict_batch, quadcopter_predict_batch)
PREDICT_EXPORTS = ["obca_batch_predict_clearance", "obca_batch_predict_clearance_ms", "obca_batch_predict_profile", "obca_parking_predict_batch",
                   "obca_quad_batch_predict_clearance", "obca_quad_batch_predict_clearance_ms", "obca_quad_batch_predict_profile", "obca_quadcopter_predict_batch"]
QUAD_PLAN_STATUS = {0: "no path", -1: "more way-points than cap", -2: "the start or goal point is blocked, or a coordinate of the record is not finite",
                    -3: "the relaxation hit its sweep bound", -4: "not selected"}
QUAD_REFINE_STATUS = {0: "refined from the solution", 1: "interpolated from the uploaded warm start (the last solve failed, or its iterate is not finite)",
                      -1: "zero warm start (the uploaded one is not finite either)"}
REFINE_STATUS = {0: "refined from the solution", 1: "refined from the start iterate (the last solve failed, or its iterate is not finite)", -1: "zero start (the start iterate is not finite either)"}
PATH_WS_STATUS = {0: "written", -1: "no path", -2: "more nodes than rows, or than PATH_WS_MAXNODES", -3: "a non-finite pose", -4: "the path length is not positive"}


def selftest(device=0, repeats=4, opts=None):
    """Does this GPU return the same bits for the same inputs, whatever ran on it before?  The config-2 bench batch (1 024 instances, N = 80: every SIMD of the chip holds one) is
    solved `repeats` times as one device-resident batch and every download is compared bit for bit with the first; then a kernel leaves a large finite pattern in the LDS of every
    CU (obca_amd.diag.leave_pattern, libobca_diag.so) and the batch is solved once more.  Returns a dict: `differing` = (instance, run) pairs that differ, `after_pattern` = instances that differ
    after the pattern, `pattern_units` = per device (compute units the pattern kernel ran on, units that got the four workgroups which cover their whole LDS), `instances`, `runs`, `solved`, `device`.  Both counts are 0: the kernels contain no atomics and no order-dependent reductions, and read nothing they have not
    written (DESIGN.md sections 3 and 11 -- until the end of round 5 the multiplier sums of the parking kernels' termination test were read from LDS unwritten, and results changed with what other
    kernels had left there, e.g. when another process shared the GPU)."""
    from . import scenarios as S
    N, B = 80, 1024
    bt = S.make_batch(S.BACKWARDS, B, N)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    ctx = device if isinstance(device, Context) else Context(device)
    b = Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])

    def differing(o, ref):
        return int(((o["info"] != ref["info"]).any(axis=1) | (np.abs(o["xp"] - ref["xp"]).reshape(B, -1).max(axis=1) > 0)).sum())
    ref = None; bad = 0
    for _ in range(max(2, repeats)):
        b.solve(opts=opts); o = b.download()
        if ref is None:
            ref = o; continue
        bad += differing(o, ref)
    from . import diag
    reach = diag.leave_pattern(ctx, 4, 1e30)      # (a diagnostic library of its own: libobca_diag.so)
    b.solve(opts=opts); after = differing(b.download(), ref)
    name = ctx.name()
    b.close()
    if not isinstance(device, Context):
        ctx.close()
    return dict(differing=bad, after_pattern=after, pattern_units=reach, instances=B, runs=max(2, repeats), solved=int((ref["exitflag"] == 1).sum()), device=name)


def warm_restart_opts():
    """options for a solve that starts from a (shifted) previous solution: small initial barrier and bound push, so the interior point
    does not first walk away from the active bounds (16 instead of 47 iterations on the config-2 batch)"""
    o = default_opts(); o.mu_init = 1e-4; o.bound_push = 1e-4; o.bound_frac = 1e-4
    return o


def _opts(fn):
    """an option record filled by one of the library's four obca_*_opts"""
    o = Opts()
    getattr(_load(), fn)(C.byref(o))
    return o


def default_opts():
    return _opts("obca_default_opts")


def ipopt_opts():
    """the reference's IPOPT configuration as far as the kernels carry it: default options + second-order correction (IPOPT's default max_soc = 4), recalc_y = "yes"
    (ParkingSignedDist.jl:41), IPOPT's least-squares initial multipliers, and the block feasibility restoration that stands in for IPOPT's restoration phase (restoration = 1)"""
    return _opts("obca_reference_opts")


def _in(a, dtype=np.float64):
    """an input as the ABI takes it: C-contiguous float64 (or int32); None stays NULL"""
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _ref(opts):
    return C.byref(opts) if opts is not None else None


def _per_instance(v, B):
    """a scalar or (B,) values -> (B,)"""
    return _in(np.broadcast_to(np.asarray(v, float), (B,)))


def _time_scale(timeScale, B, N1):
    """a scalar, (B,) or (B, N+1) values -> (B, N+1)"""
    ts = np.asarray(timeScale, float)
    return _in(np.broadcast_to(ts.reshape(B, 1) if ts.ndim == 1 and ts.size == B else ts, (B, N1)))


def _boxes(ob, B):
    """the quadcopter's five boxes, one shared set (5,6) or (B,5,6) -> (B, 30)"""
    ob = np.asarray(ob, float)
    return _in(np.broadcast_to(ob.reshape(-1, 30) if ob.size != 30 else ob.reshape(1, 30), (B, 30)))


def _blocks(flat, rows, N1):
    """the ABI's packed per-instance blocks -> a list of (N+1, rows_i) views"""
    ends = np.cumsum(rows) * N1
    return [flat[e - r * N1:e].reshape(N1, r) for e, r in zip(ends.tolist(), np.asarray(rows).tolist())]


def _verdict(B, names, call, ref_ok=False):
    """the outputs of a validate entry point, `call(ok, [ref_ok,] viol)`, and the dict they are returned in"""
    ok = np.zeros(B, np.int32); rok = [np.zeros(B, np.int32)] if ref_ok else []; viol = np.zeros((B, len(names)))
    call(ok, *rok, viol)
    return dict(ok=ok.astype(bool), **({"ref_ok": rok[0].astype(bool)} if ref_ok else {}), viol=viol, names=names)


def _clearance(B, substeps, nOb, call):
    """the records of a clearance entry point, `call(out)` with out (B, CLR_OUT), and the dict they are returned in: min, min_nodes (B,); sample q = stage * substeps + substep of
    the minimum, obstacle (-1 where not finite); below = samples whose smallest clearance is < need, samples = N substeps + 1; per_obstacle (B, nOb) (+inf behind an
    instance's own obstacles); finite (B,) bool -- False: a non-finite number in the trajectory, the values of that instance are NaN"""
    rec = np.zeros((B, CLR_OUT))
    call(rec)
    return _clearance_dict(rec, substeps, nOb)


def _clearance_dict(rec, substeps, nOb):
    """the dict of _clearance from records (B, CLR_OUT)"""
    q = rec[:, 2].astype(np.int64); S = int(substeps)
    return dict(min=rec[:, 0], min_nodes=rec[:, 1], sample=q, stage=np.where(q >= 0, q // S, -1), substep=np.where(q >= 0, q % S, -1), obstacle=rec[:, 3].astype(np.int64),
                below=rec[:, 4].astype(np.int64), samples=rec[:, 5].astype(np.int64), per_obstacle=rec[:, 8:8 + int(nOb)], finite=rec[:, 6] == 0)


def _certify(B, call):
    """the records of a certify entry point, `call(out)` with out (B, CERT_OUT), and the dict they are returned in: lb (B,) the PROVEN lower bound of the clearance over the
    whole path (-inf: an item was left undecided), seen the smallest clearance sampled, at `interval`, `tick` (of CERT_TICKS per interval; interval N is node N) and
    `obstacle`; violated = intervals with a sample under need, first_violation (B, 3) = (interval, tick, obstacle) of the first one, -1 where none; undecided items;
    samples taken in total and samples_max in one item; lipschitz = the largest speed bound of an interval; certified (B,) bool: clearance >= need - slack everywhere on
    the path; finite (B,) bool -- False: a non-finite number in the trajectory, the values of that instance are NaN"""
    rec = np.zeros((B, CERT_OUT))
    call(rec)
    return _certify_dict(rec)


def _certify_dict(rec):
    """the dict of _certify from records (B, CERT_OUT)"""
    i64 = lambda a: a.astype(np.int64)
    return dict(lb=rec[:, 0], seen=rec[:, 1], interval=i64(rec[:, 2]), tick=i64(rec[:, 3]), obstacle=i64(rec[:, 4]), violated=i64(rec[:, 5]), first_violation=i64(rec[:, 6:9]),
                undecided=i64(rec[:, 9]), samples=i64(rec[:, 10]), samples_max=i64(rec[:, 11]), lipschitz=rec[:, 12], certified=rec[:, 13] != 0, finite=rec[:, 14] == 0)


def _rollout(B, substeps, nOb, call):
    """the records of a rollout entry point, `call(out)` with out (B, ROLL_OUT), and the dict they are returned in: dev_pos (B,) the largest position deviation of the rolled
    node states from the trajectory's own over the nodes 1..N, dev_node its node (-1 where not finite); dev_att, dev_vel, dev_rate likewise for attitude, velocity and body
    rates; end_pos, end_att, end_vel, end_rate the same at node N; restart, substeps as the call had them; finite (B,) bool -- False: a non-finite number in the trajectory
    or among the rolled states, the values of that instance are NaN; clearance: the dict of _clearance for the rolled samples"""
    rec = np.zeros((B, ROLL_OUT))
    call(rec)
    return _rollout_dict(rec, substeps, nOb)


def _rollout_dict(rec, substeps, nOb):
    """the dict of _rollout from records (B, ROLL_OUT)"""
    return dict(dev_pos=rec[:, 1], dev_node=rec[:, 2].astype(np.int64), dev_att=rec[:, 3], dev_vel=rec[:, 4], dev_rate=rec[:, 5], end_pos=rec[:, 6], end_att=rec[:, 7],
                end_vel=rec[:, 8], end_rate=rec[:, 9], restart=rec[:, 10] != 0, substeps=rec[:, 11].astype(np.int64), finite=rec[:, 0] == 0,
                clearance=_clearance_dict(rec[:, 16:], substeps, nOb))


def _per_obstacle(v, nObs, width):
    """a parameter of Batch.move_obstacles as the ABI takes it, (nOb_total, width) (width 0: (nOb_total,)) in upload order: one value ((width,) / a scalar) goes to every
    obstacle, B rows go over each instance's obstacles, nOb_total rows are taken as they are; None stays NULL"""
    if v is None:
        return None
    a = np.asarray(v, float); B, nt = len(nObs), int(np.sum(nObs)); tail = (width,) if width else ()
    if a.shape == tail:
        return _in(np.broadcast_to(a, (nt,) + tail))
    if a.shape == (nt,) + tail:
        return _in(a)
    if a.shape == (B,) + tail:
        return _in(np.repeat(a, np.asarray(nObs, np.int64), axis=0))
    raise ValueError("move_obstacles: need a value of shape %s, (B,)+ it or (nOb_total,) + it, got %s" % (tail, a.shape))


def _per_box(v, B, width):
    """the same for QuadBatch.move_obstacles, 5 boxes per instance: (width,) / a scalar, (5,) + it, (B,) + it (B != 5) or (B, 5) + it -> (B, 5) + it"""
    if v is None:
        return None
    a = np.asarray(v, float); tail = (width,) if width else ()
    if a.shape == (B,) + tail and B != 5:
        a = a.reshape((B, 1) + tail)
    return _in(np.broadcast_to(a, (B, 5) + tail))


def _parking_rates(nObs, rates, pivot, grow):
    """the rate records of Batch.predict_clearance as the ABI takes them, (nOb_total, 6) = [vx, vy, w, cx, cy, g] per obstacle in upload order: each of the three
    parameters goes through _per_obstacle, as move_obstacles packs its motion, pivot and inflate; None: zeros"""
    out = np.zeros((int(np.sum(nObs)), 6))
    for v, cols, width in ((rates, slice(0, 3), 3), (pivot, slice(3, 5), 2), (grow, 5, 0)):
        a = _per_obstacle(v, nObs, width)
        if a is not None:
            out[:, cols] = a
    return out


def _quad_rates(B, rates, grow):
    """the same for QuadBatch.predict_clearance through _per_box: (B, 5, 4) = [vx, vy, vz, g] per box"""
    out = np.zeros((B, 5, 4))
    for v, cols, width in ((rates, slice(0, 3), 3), (grow, 3, 0)):
        a = _per_box(v, B, width)
        if a is not None:
            out[:, :, cols] = a
    return out


def _predict(B, substeps, nOb, call):
    """the records of a predict entry point, `call(out)` with out (B, PRD_OUT), and the dict they are returned in: the dict of _clearance for the samples measured against
    the obstacles where they will be when the vehicle reaches them, and first (B,) the first sample whose smallest clearance is < need (-1: none), t_first its time in
    seconds (+inf: none; finite: an instance to re-solve now), first_obstacle (-1: none), t_min the time of `sample`, horizon the time of the last sample, moving the
    obstacles with a rate that is not 0.  finite False: a non-finite number in the trajectory or the rates, or a moved row that is not finite -- the times are NaN"""
    rec = np.zeros((B, PRD_OUT))
    call(rec)
    return dict(_clearance_dict(rec, substeps, nOb), first=rec[:, 24].astype(np.int64), t_first=rec[:, 25], first_obstacle=rec[:, 26].astype(np.int64), t_min=rec[:, 27],
                horizon=rec[:, 28], moving=rec[:, 29].astype(np.int64))


def _advance(B, substeps, nOb, call):
    """the records of an advance entry point, `call(out)` with out (B, ADV_OUT), and the dict they are returned in: the dict of _rollout for the driven intervals --
    dev_* the deviations of the plant from the solution's own nodes 1..shift (the model mismatch the next solve absorbs), end_* at node `shift`, `clearance` of the driven
    samples; finite False marks an instance that was NOT advanced and not restarted (its values are NaN) -- and shift, driven_time (sum t_k Ts), goal_dist (the position
    distance of the new plant state to the goal of the next solve), logged (the nodes in the log after the call, -1 without one)"""
    rec = np.zeros((B, ADV_OUT))
    call(rec)
    return dict(_rollout_dict(rec, substeps, nOb), shift=rec[:, 12].astype(np.int64), driven_time=rec[:, 13], goal_dist=rec[:, 14], logged=rec[:, 15].astype(np.int64))


def _track(B, substeps, nOb, call):
    """the records of a track entry point, `call(out)` with out (B, TRK_OUT), and the dict they are returned in: the dict of _rollout for the tracked chain (deviations of
    the tracked node states from the trajectory's own, `clearance` of the driven samples; finite False: a non-finite number in the trajectory, in dx0 or among the tracked
    states, or a pivot of the Riccati recursion that was not finite and positive -- the values of that instance are NaN), and saturated (B,) the number of intervals in
    which an input was clipped, du_max the largest |U_k - u_k| over inputs and intervals, du_node its interval, dx0_pos |dx0| of the position part, feedback, clamp as the
    call had them"""
    rec = np.zeros((B, TRK_OUT))
    call(rec)
    return dict(_rollout_dict(rec[:, :ROLL_OUT], substeps, nOb), saturated=rec[:, 42].astype(np.int64), du_max=rec[:, 43], du_node=rec[:, 44].astype(np.int64), dx0_pos=rec[:, 45],
                feedback=rec[:, 40] != 0, clamp=rec[:, 41] != 0)


def _ensemble(B, call):
    """the records of an ensemble entry point, `call(out)` with out (B, ENS_OUT), and the dict they are returned in: finite (B,) bool -- False: what track() marks for the
    whole instance, every member is bad and the values are NaN / -1 --; members, substeps, feedback, clamp as the call had them; members_bad, members_hit (good members
    with a sample whose clearance is < need), members_sat (good members with a clipped interval); min the smallest clearance over the good members, min_member,
    min_sample, min_obstacle where; dev_pos the largest position deviation from the nominal nodes 1..N, dev_pos_member, dev_node; end_pos the largest at node N,
    end_pos_member; dev_att, dev_vel, dev_rate; du_max the largest |U_k - u_k|, du_member, du_node; end_pos_mean and min_mean over the good members; below the samples
    under need, summed over the good members.  Ties go to the smaller member."""
    rec = np.zeros((B, ENS_OUT))
    call(rec)
    i = lambda c: rec[:, c].astype(np.int64)      # noqa: E731
    return dict(finite=rec[:, 0] == 0, members=i(1), substeps=i(2), feedback=rec[:, 3] != 0, clamp=rec[:, 4] != 0, members_bad=i(5), members_hit=i(6), members_sat=i(7),
                min=rec[:, 8], min_member=i(9), min_sample=i(10), min_obstacle=i(11), dev_pos=rec[:, 12], dev_pos_member=i(13), dev_node=i(14), end_pos=rec[:, 15],
                end_pos_member=i(16), dev_att=rec[:, 17], dev_vel=rec[:, 18], dev_rate=rec[:, 19], du_max=rec[:, 20], du_member=i(21), du_node=i(22), end_pos_mean=rec[:, 23],
                min_mean=rec[:, 24], below=i(25))


def _ensemble_rows(a, B, M, n, what):
    """None, (M, n) for every instance or (B, M, n): the ABI's n x M x B, each member's n contiguous"""
    if a is None:
        return None
    a = np.asarray(a, float)
    if a.shape not in ((M, n), (B, M, n)):
        raise ObcaError(f"{what} must be ({M},{n}) or ({B},{M},{n}); got {a.shape}")
    return _in(np.broadcast_to(a, (B, M, n)))


def ensemble_offsets(B, M, sigma, seed=0):
    """(B, M, len(sigma)) rows drawn from N(0, diag(sigma^2)) with numpy's default_rng(seed) -- there is no random number generator on the device --, member 0 exactly
    zero: member 0 of an ensemble() is then the nominal closed loop.  For the dx0 (sigma of length nx) or the dub (length nu) of ensemble()."""
    sigma = np.atleast_1d(np.asarray(sigma, float))
    d = np.random.default_rng(seed).standard_normal((int(B), int(M), sigma.size)) * sigma
    d[:, 0] = 0.0
    return d


def _track_weights(nx, nu, Q, R, Qf, defaults):
    """diagonal weights as the ABI takes them: None -> the named defaults (Qf: 10 Q); a scalar is repeated"""
    q = _in(np.broadcast_to(np.asarray(defaults[0] if Q is None else Q, float), (nx,)))
    r = _in(np.broadcast_to(np.asarray(defaults[1] if R is None else R, float), (nu,)))
    qf = _in(np.broadcast_to(np.asarray((defaults[2] if Q is None else 10.0 * q) if Qf is None else Qf, float), (nx,)))
    return q, r, qf


def _track_dx0(dx0, B, nx):
    """None, (nx,) for every instance or (B, nx)"""
    return None if dx0 is None else _in(np.broadcast_to(np.asarray(dx0, float), (B, nx)))


class _Handle:
    """an opaque handle of the library (`_h`) and the call that destroys it (`_destroy`)"""

    def close(self):
        if self._h:
            getattr(_load(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """One device (`device=k`), an explicit list (`devices=[...]`) or every visible device (`devices="all"`): the host-pointer entry points
    of a multi-device context shard their batch over the devices through a work queue (include/obca_hip.h, obca_create_multi)."""
    _destroy = "obca_destroy"

    def __init__(self, device=0, devices=None):
        lib = _load()
        self._h = C.c_void_p()
        if devices is None:
            rc = lib.obca_create(C.byref(self._h), int(device))
            self.devices = [int(device)]
        else:
            lst = [] if isinstance(devices, str) else [int(d) for d in devices]
            arr = (C.c_int * max(1, len(lst)))(*lst)
            rc = lib.obca_create_multi(C.byref(self._h), arr if lst else None, len(lst))
            self.devices = lst
        if rc != 0:
            raise ObcaError("obca_create failed: " + (lib.obca_last_error(None) or b"").decode())
        if devices is not None:
            self.devices = list(range(lib.obca_device_count(self._h))) if not self.devices else self.devices
        self.device = self.devices[0]

    def device_count(self):
        return int(_load().obca_device_count(self._h))

    def _check(self, rc, what):
        if rc != 0:
            raise ObcaError(f"{what} failed ({rc}): " + (_load().obca_last_error(self._h) or b"").decode())

    def name(self):
        buf = C.create_string_buffer(256)
        _load().obca_device_name(self._h, buf, 256)
        return buf.value.decode()


_default_ctx = {}


def _ctx(device=0):
    """cached context of one device index, of a tuple of indices, or of "all" visible devices"""
    if isinstance(device, Context):
        return device
    if isinstance(device, numbers.Integral):          # np.int64 local ranks, torch scalars' .item(), ...
        device = int(device)
    key = device if isinstance(device, (int, str)) else tuple(int(d) for d in device)
    if key not in _default_ctx:
        _default_ctx[key] = Context(device) if isinstance(key, int) else Context(devices=device)
    return _default_ctx[key]


def _norm_obstacles(B, vOb, A, b):
    """Accept one shared obstacle set (vOb 1-D, A (M,2)) or per-instance lists; return packed per-instance arrays."""
    if isinstance(vOb, (list, tuple)) and len(vOb) == B and np.ndim(vOb[0]) >= 1:
        nObs = np.array([len(np.ravel(v)) for v in vOb], np.int32)
        vflat = np.concatenate([np.ravel(v) for v in vOb]).astype(np.int32)
        Aflat = np.concatenate([np.asarray(a, float).reshape(-1, 2) for a in A])
        bflat = np.concatenate([np.ravel(np.asarray(x, float)) for x in b])
        return nObs, vflat, Aflat, bflat
    v = np.ravel(np.asarray(vOb)).astype(np.int32)
    M = int(v.sum())
    A = np.asarray(A, float).reshape(M, 2); b = np.ravel(np.asarray(b, float))
    return np.full(B, len(v), np.int32), np.tile(v, B), np.tile(A, (B, 1)), np.tile(b, B)


def _selection(select):
    """the instances `select` of a batch as the ABI takes them: a boolean mask or an index array -> int32 indices; None stays None, and the caller says what "all" means"""
    if select is None:
        return None
    sel = np.asarray(select)
    return np.flatnonzero(sel).astype(np.int32) if sel.dtype == bool else np.ascontiguousarray(sel, np.int32).ravel()


def _path_arrays(paths, dirs, counts, B):
    """the planner's dense output as the ABI takes it: paths (B, cap, 3) float64, dirs (B, cap) int32, counts (B,) int32 -- arrays of that kind pass unconverted"""
    paths = _in(paths); dirs = _in(dirs, np.int32); counts = _in(counts, np.int32)
    if paths.ndim != 3 or paths.shape[0] != B or paths.shape[2] != 3 or dirs.shape != paths.shape[:2] or counts.shape != (B,):
        raise ObcaError(f"paths must be (B, cap, 3), dirs (B, cap), counts (B,) with B = {B}; got {paths.shape}, {dirs.shape}, {counts.shape}")
    return paths, dirs, counts, int(paths.shape[1])


def _warm_start(xWS, uWS, B, N):
    """xWS (B, >= N+1, 4), uWS (B, >= N, 2) cut to the horizon -- checked here, because the C side reads N+1 / N rows through raw pointers"""
    xWS = np.asarray(xWS, float).reshape(B, -1, 4); uWS = np.asarray(uWS, float).reshape(B, -1, 2)
    if xWS.shape[1] < N + 1 or uWS.shape[1] < N:
        raise ObcaError(f"warm start too short: xWS has {xWS.shape[1]} stages (need N+1 = {N + 1}), uWS {uWS.shape[1]} (need N = {N})")
    return xWS[:, :N + 1], uWS[:, :N]


def _dual_start(lWS, nWS, Mt, nt, N):
    """optional dual warm start, packed per instance ((N+1) x M_i, (N+1) x 4 nOb_i blocks); sizes checked before raw pointers go to C"""
    if lWS is None or nWS is None:
        return None, None
    if not isinstance(lWS, np.ndarray):
        lWS = np.concatenate([np.ravel(x) for x in lWS])
    if not isinstance(nWS, np.ndarray):
        nWS = np.concatenate([np.ravel(x) for x in nWS])
    if lWS.size != Mt * (N + 1) or nWS.size != 4 * nt * (N + 1):
        raise ObcaError(f"dual warm start has the wrong size: lWS {lWS.size} (need {Mt * (N + 1)}), nWS {nWS.size} (need {4 * nt * (N + 1)})")
    return lWS, nWS


def _problem(B, Ts, L, ego, XYbounds, fixTime, x0, xF, vOb, A, b):
    """what the three parking entry points share: (nOb per instance, rows per instance, the arguments Ts .. b in the order of include/obca_hip.h)"""
    nObs, vflat, Aflat, bflat = _norm_obstacles(B, vOb, A, b)
    return nObs, _row_counts(nObs, vflat), (_per_instance(Ts, B), L, _in(ego), _in(XYbounds), int(fixTime), _in(np.reshape(x0, (B, 4))), _in(np.reshape(xF, (B, 4))),
                                            _in(nObs, np.int32), _in(vflat, np.int32), _in(Aflat), _in(bflat))


def _row_counts(nObs, vflat):
    """half-space rows per instance: segment sums of vflat (one numpy call -- a Python loop over 16 384 instances cost a third of the wrapper's time)"""
    nObs = np.asarray(nObs, np.int64)
    csum = np.concatenate([[0], np.cumsum(np.asarray(vflat, np.int64))])
    ends = np.cumsum(nObs)
    return csum[ends] - csum[ends - nObs]


class _DeviceBatch(_Handle):
    """What Batch and QuadBatch share: the handle and the calls of the C ABI that differ only in their prefix (`_c`: obca_batch / obca_quad_batch)."""
    _destroy = property(lambda self: f"{self._c}_destroy")

    def __init__(self, ctx, B, N):
        self.ctx, self.B, self.N = ctx, int(B), int(N)
        self.capacity = self.B      # (B is the number of instances the batch holds: a refine into it may leave fewer)
        self._h = C.c_void_p()
        self._call("create", ctx._h, self.B, self.N, C.byref(self._h), handle=False)

    def _call(self, name, *args, handle=True):
        """obca_[quad_]batch_<name>(handle, *args); a non-zero status raises ObcaError with the library's message"""
        fn = f"{self._c}_{name}"
        self.ctx._check(getattr(_load(), fn)(*((self._h,) if handle else ()), *args), fn)

    def solve(self, opts=None, sync=True):
        self._call("solve", _ref(opts))
        if sync:
            self.sync()

    def sync(self):
        self._call("sync")

    def phase_cycles(self):
        """(B,16) per-phase shader-cycle counters of the last solve: exists in the profiling build only (OBCA_HIP_LIBRARY=.../libobca_hip_prof.so, tools/phase_profile.py)."""
        out = np.zeros((self.B, 16))
        if not hasattr(_load(), f"{self._c}_debug_phase_cycles"):
            raise ObcaError("phase_cycles(): the loaded library is not the -DOBCA_PROFILE build")
        self._call("debug_phase_cycles", out)
        return out

    def scratch_bytes(self):
        v = C.c_longlong(0)
        getattr(_load(), f"{self._c}_scratch_bytes")(self._h, C.byref(v))
        return v.value

    def _floats(self, name, n=1):
        """what obca_[quad_]batch_<name> writes through its n `float *`: HIP-event durations [ms]; one number for n = 1, else a tuple"""
        v = [C.c_float(0) for _ in range(n)]
        self._call(name, *map(C.byref, v))
        return v[0].value if n == 1 else tuple(x.value for x in v)

    def validate_ms(self):
        """HIP-event duration of the last validate kernel"""
        return self._floats("validate_ms")

    def clearance_ms(self):
        """HIP-event duration of the last clearance kernel"""
        return self._floats("clearance_ms")

    def _certify(self, need, slack, max_steps):
        return _certify(self.B, lambda out: self._call("certify", float(need), float(slack), int(max_steps), out))

    def certify_intervals(self):
        """[lb_k, seen_k] of the last certify(), fetched from the device: (B, N+1, 2) -- per interval (row N: node N) the proven bound and the smallest sampled clearance over
        the obstacles; lb_k = -inf where an item of the interval was left undecided, NaN for an instance that was not finite.  They describe the scene
        certify() ran in: a later move_obstacles() does not change them."""
        iv = np.zeros((self.B, self.N + 1, 2))
        self._call("certify_intervals", iv)
        return iv

    def certify_ms(self):
        """HIP-event duration of the last certify kernel"""
        return self._floats("certify_ms")

    def _rollout(self, nOb, substeps, restart, need):
        return _rollout(self.B, substeps, nOb, lambda out: self._call("rollout", int(substeps), int(restart), float(need), out))

    def rollout_states(self):
        """The node states of the last rollout(), fetched from the device: (B, N+1, nx), nx = 4 (parking) or 12 (quadcopter); NaN for an instance that was not finite.
        rollout_states()[:, shift] of a chain-mode rollout is the state the vehicle reaches after `shift` intervals: the x0_new of shift_warm_start(shift, x0_new=...).
        The states do not depend on the obstacles; the clearances rollout() returned with them describe the scene it ran in, whatever move_obstacles() did later."""
        X = np.zeros((self.B, self.N + 1, self._nx))
        self._call("rollout_states", X)
        return X

    def rollout_ms(self):
        """HIP-event duration of the last rollout kernel"""
        return self._floats("rollout_ms")

    def _advance(self, nOb, shift, substeps, need, *rows):
        """what Batch.advance and QuadBatch.advance share: `rows` (the kick, for the quadcopter xF_new) are None or (B, nx) / (nx,)"""
        a = [None if r is None else _in(np.broadcast_to(np.asarray(r, float), (self.B, self._nx))) for r in rows]
        return _advance(self.B, substeps, nOb, lambda out: self._call("advance", int(shift), int(substeps), *a, float(need), out))

    def advance_state(self):
        """The plant state the last advance() left on the device: (B, nx), after the kick; NaN for an instance that was not finite.  It is X0 of the instance's problem
        record now: the next advance() starts the plant there."""
        X = np.zeros((self.B, self._nx))
        self._call("advance_state", X)
        return X

    def advance_log(self, capacity):
        """Keep the node states every advance() drives through ON THE DEVICE: room for `capacity` nodes per instance (0: free the log).  The log starts empty, an upload
        empties it, and an advance() that would not fit is refused before it does anything."""
        self._call("advance_log", int(capacity))

    def advance_log_states(self):
        """The log, fetched from the device: (B, nodes, nx) -- per advance() its `shift` nodes, the last one after the kick; the rows of a step in which an instance was
        not finite hold what was there before (zeros in a fresh log)."""
        n = np.zeros(1, np.int32)
        self._call("advance_log_states", None, n)
        X = np.zeros((self.B, int(n[0]), self._nx))
        if n[0]:
            self._call("advance_log_states", X, n)
        return X

    def advance_ms(self):
        """HIP-event duration of the last advance kernel"""
        return self._floats("advance_ms")

    def move_obstacles_ms(self):
        """HIP-event duration of the last move_obstacles kernel"""
        return self._floats("move_obstacles_ms")

    def _predict(self, nOb, rates, substeps, need, profile):
        r = _predict(self.B, substeps, nOb, lambda out: self._call("predict_clearance", _in(rates).reshape(-1), int(substeps), float(need), int(bool(profile)), out))
        if profile:
            self._predict_S = int(substeps)
        return r

    def predict_profile(self):
        """The clearance-over-time profile of the last predict_clearance(profile=True), fetched from the device: (B, N substeps + 1) -- per sample the smallest predicted
        clearance over the obstacles; a row of NaN for an instance that was not finite.  Sample q is reached at the time the numpy statement
        obca_amd.validate.predict_times gives.  The buffer costs 8 B (N substeps + 1) bytes of device memory and stays with the batch."""
        S = getattr(self, "_predict_S", 0)
        out = np.zeros((self.B, self.N * S + 1))
        self._call("predict_profile", out.reshape(-1), out.size if S else 0)
        return out

    def predict_clearance_ms(self):
        """HIP-event duration of the last predict_clearance kernel"""
        return self._floats("predict_clearance_ms")

    def _track(self, nOb, defaults, substeps, dx0, Q, R, Qf, feedback, clamp, need):
        q, r, qf = _track_weights(self._nx, self._nu, Q, R, Qf, defaults)
        return _track(self.B, substeps, nOb, lambda out: self._call("track", int(substeps), int(feedback), int(clamp), q, r, qf, _track_dx0(dx0, self.B, self._nx), float(need), out))

    def track_states(self):
        """The node states of the last track(), fetched from the device: (B, N+1, nx); NaN for an instance that was not finite.  track_states()[:, shift] is the state the
        vehicle reaches after `shift` intervals under the feedback: the x0_new of shift_warm_start(shift, x0_new=...).  rollout_states() of an earlier rollout stays valid."""
        X = np.zeros((self.B, self.N + 1, self._nx))
        self._call("track_states", X)
        return X

    def track_gains(self):
        """The gains of the last track(), fetched from the device: (B, N, nu, nx), u = u_k + K[k] (X_k - x_k); NaN for an instance that was not finite."""
        K = np.zeros((self.B, self.N, self._nu, self._nx))
        self._call("track_gains", K)
        return K

    def track_ms(self):
        """HIP-event duration of the last track kernel"""
        return self._floats("track_ms")

    def _ensemble(self, defaults, members, substeps, dx0, dub, Q, R, Qf, feedback, clamp, need):
        q, r, qf = _track_weights(self._nx, self._nu, Q, R, Qf, defaults); M = int(members)
        if not 1 <= M <= ENS_MMAX:
            raise ObcaError(f"need 1 <= members <= {ENS_MMAX}")
        d0 = _ensemble_rows(dx0, self.B, M, self._nx, "dx0"); db = _ensemble_rows(dub, self.B, M, self._nu, "dub")
        r_ = _ensemble(self.B, lambda out: self._call("ensemble", int(substeps), M, int(feedback), int(clamp), q, r, qf, d0, db, float(need), out))
        self._ens_members = M
        return r_

    def ensemble_members(self):
        """The member records of the last ensemble(), fetched from the device: (B, M, 16) -- bad, dev_pos, its node, end_pos, dev_att, dev_vel, dev_rate, min clearance,
        its sample, its obstacle, below, saturated intervals, du_max, its interval, |dx0| of the position part, 0; a bad member's real fields are NaN, its indices -1."""
        mem = np.zeros((self.B, getattr(self, "_ens_members", 1), ENS_MEM))
        self._call("ensemble_members", mem)
        return mem

    def ensemble_final(self):
        """The final states X_N of the members of the last ensemble(), fetched from the device: (B, M, nx); NaN for a bad member."""
        fin = np.zeros((self.B, getattr(self, "_ens_members", 1), self._nx))
        self._call("ensemble_final", fin)
        return fin

    def ensemble_ms(self):
        """HIP-event duration of the last ensemble kernel"""
        return self._floats("ensemble_ms")

    def _refine_into(self, entry, limit, extra, select, factor, into):
        """What Batch.refine and QuadBatch.refine share: the selection (None: all) checked against the batch, the factor against `limit`, the destination (`into`, or a new
        batch of this kind, closed again if the call fails) and the call of `entry` with its one own argument `extra`.  Returns (destination, selection, status)."""
        sel = _selection(select)
        sel = np.arange(self.B, dtype=np.int32) if sel is None else sel
        n = int(sel.size); factor = int(factor)
        if n < 1:
            raise ObcaError("refine: the selection is empty")
        if sel.min() < 0 or sel.max() >= self.B:
            raise ObcaError(f"refine: an index outside 0 .. {self.B - 1}")
        if into is None and not (1 <= factor <= limit):
            raise ObcaError(f"refine: need 1 <= factor <= {limit}")
        dst = into if into is not None else type(self)(self.ctx, n, factor * self.N)
        st = np.zeros(n, np.int32)
        try:
            self.ctx._check(getattr(_load(), entry)(dst._h, self._h, factor, extra, sel, n, st), entry)
        except ObcaError:
            if into is None:
                dst.close()
            raise
        dst.B = n
        return dst, sel, st


class Batch(_DeviceBatch):
    """Device-resident batch: upload once, solve (repeatedly), download."""
    _c = "obca_batch"
    _nx = 4
    _nu = 2

    def upload(self, x0, xF, Ts, L, ego, XYbounds, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS, lWS=None, nWS=None, dist=False):
        """lWS/nWS, when given, are packed per instance as (N+1, M_i) / (N+1, 4 nOb_i) row-major blocks (= the reference's
        column-major l (M x N+1) and n (4nOb x N+1))."""
        self._call("set_formulation", bool(dist))
        B = self.B = self.capacity; N = self.N      # (an upload fills the batch)
        self.nObs, self.Ms, prob = _problem(B, Ts, L, ego, XYbounds, fixTime, x0, xF, vOb, A, b)
        self.vflat = prob[8]
        lWS, nWS = _dual_start(lWS, nWS, int(self.Ms.sum()), int(self.nObs.sum()), N)
        ws = (None, None) if xWS is None and uWS is None else _warm_start(xWS, uWS, B, N)      # (both None: zeros, for a start that set_path_warm_start writes on the device)
        self._call("upload", *prob, *(_in(np.reshape(r, (B, N + 1))) for r in (rx, ry, ryaw)), *(_in(w) for w in ws), _in(lWS), _in(nWS))

    def set_path_warm_start(self, paths, dirs, counts, v_nom=0.5, smooth=False, use_xF=True):
        """The warm start of planner.path_to_warm_start, computed ON THE DEVICE from the planner's dense arrays (obca_batch_set_path_warm_start; paths (B, cap, 3), dirs
        (B, cap), counts (B,) as obca_plan_hybrid_astar_batch2 writes them) and written into the uploaded batch: Ts, the tracking reference, the x / u start, t = 1; the
        next solve runs DualMultWS.  use_xF: the uploaded goal replaces the last pose; smooth: the speed profile goes through velo_smooth at 0.3 m/s^2.  Returns the status
        per instance (PATH_WS_STATUS; an instance with a negative one keeps what was uploaded)."""
        paths, dirs, counts, cap = _path_arrays(paths, dirs, counts, self.B)
        st = np.zeros(self.B, np.int32)
        self._call("set_path_warm_start", paths, dirs, counts, cap, bool(use_xF), float(v_nom), 0.3 if smooth else 0.0, st)
        return st

    def path_ws_ms(self):
        """HIP-event duration of the last set_path_warm_start kernel"""
        return self._floats("path_ws_ms")

    def plan_warm_start(self, bucket_width=None, cap=1024, v_nom=0.5, smooth=False, use_xF=True, **planner_options):
        """The resident route (obca_batch_plan_warm_start): every instance of the uploaded batch is planned ON THE DEVICE in its own obstacle field -- put together there
        from the record the upload left: x0, xF, the unit rows, the uploaded ego, L and XYbounds -- by scene_astar_batch's search, and set_path_warm_start's kernel writes
        the warm start from the paths where they lie.  No path, no field and no pose crosses the bus.  planner_options: the search options by name, as
        planner.scene_astar_many takes them (planner.DEFAULT_OPTS); bucket_width, cap: scene_astar_batch's (cap <= PATH_WS_MAXNODES); v_nom, smooth, use_xF:
        set_path_warm_start's.  Returns (counts, status, expansions, rounds), (B,) int32 each: counts as scene_astar_batch (HYBRID_STATUS), status as set_path_warm_start
        (PATH_WS_STATUS; an instance with a negative one keeps what was uploaded)."""
        opts = planner._opts_array(planner_options)
        cnt, st, nexp, rounds = (np.zeros(self.B, np.int32) for _ in range(4))
        self._call("plan_warm_start", opts, len(opts), 0.0 if bucket_width is None else float(bucket_width), int(cap), bool(use_xF), float(v_nom), 0.3 if smooth else 0.0,
                   cnt, st, nexp, rounds)
        return cnt, st, nexp, rounds

    def plan_ms(self):
        """HIP-event durations (pack, search, ws) of the three kernels of the last plan_warm_start [ms]"""
        return self._floats("plan_ms", 3)

    def plan_paths(self):
        """What the last plan_warm_start planned, for plots and tests: (paths (B, cap, 3), dirs (B, cap), inst (B, 10) -- the instance records the packing kernel wrote:
        start x, y, yaw, sin, cos, goal x, y, yaw, sin, cos).  They lie in the context's planner staging: an ObcaError once another planner call of the context has run."""
        cap = _load().obca_batch_plan_download(self._h, None, None, 0, None)      # (no array: the call answers with the last plan's cap, whoever made the plan)
        if cap < 2:
            self.ctx._check(cap, "obca_batch_plan_download")
        paths = np.zeros((self.B, cap, 3)); dirs = np.zeros((self.B, cap), np.int32); inst = np.zeros((self.B, 10))
        self._call("plan_download", paths, dirs, cap, inst)
        return paths, dirs, inst

    def plan_block(self):
        """DIAGNOSTIC (obca_batch_packed_block): what the packing kernel of the last plan_warm_start wrote on the device, as the search read it -- (block, dims): the bytes of
        the packed block (layout: obca_amd/csrc/obca_plan_resident.h) and dict(B, nObMax, MMax, slot_allocs, io_allocs), the last two counting how often the context's planner
        has allocated its slots and its staging block so far."""
        d = np.zeros(6, np.int32)
        self._call("packed_block", None, 0, d)
        block = np.zeros(int(d[3]))
        self._call("packed_block", block, len(block), d)
        return block.view(np.uint8), dict(B=int(d[0]), nObMax=int(d[1]), MMax=int(d[2]), slot_allocs=int(d[4]), io_allocs=int(d[5]))

    def shift_warm_start(self, shift, x0_new=None):
        """receding-horizon restart: the next solve starts from the last solution advanced by `shift` stages (kept on the device), from x0_new (B,4; the measured state;
        None: stage `shift` of the solution).  The exit flag of the last solve is not consulted.  ObcaError if nothing has been solved since the last upload or shift, if shift
        is outside 0..N, or if x0_new holds a non-finite entry; the batch is then as it was."""
        self._call("shift_warm_start", int(shift), _in(np.reshape(x0_new, (self.B, 4))) if x0_new is not None else None)

    def kernel_ms(self):
        """(ipm_ms, dualws_ms) of the last solve, measured with HIP events on the launch stream."""
        return self._floats("kernel_ms", 2)

    def last_schedule(self):
        """(ipm launches, slice passes) of the last solve: (1, 0) single launch, (2, q) the two-launch schedule with a q-pass first slice"""
        a, b = C.c_int(0), C.c_int(0)
        self._call("last_schedule", C.byref(a), C.byref(b))
        return a.value, b.value

    def download(self):
        B, N = self.B, self.N
        Mt, nt = int(self.Ms.sum()), int(self.nObs.sum())
        xp = np.zeros((B, N + 1, 4)); up = np.zeros((B, N, 2)); ts = np.zeros((B, N + 1)); ef = np.zeros(B, np.int32)
        lp = np.zeros(Mt * (N + 1)); npp = np.zeros(4 * nt * (N + 1)); sl = np.zeros(nt * (N + 1)); info = np.zeros((B, 8))
        self._call("download", xp, up, ts, ef, lp, npp, sl, info)
        return _unpack_parking(B, N, self.nObs, self.Ms, xp, up, ts, ef, lp, npp, sl, info)

    def validate(self, tol=5e-5):
        """A-posteriori check of the last solution ON THE DEVICE (obca_batch_validate; the numpy statement is obca_amd.validate.validate_parking /
        parking_constraints_ref_worst): dict(ok (B,) bool -- every class except penetration <= tol --, ref_ok (B,) bool -- the reference's own test at 5e-5 --,
        viol (B, 14) in the order of `names` = VIOL_NAMES).  Only these 16 numbers per instance are downloaded."""
        return _verdict(self.B, VIOL_NAMES, lambda *out: self._call("validate", tol, *out), ref_ok=True)

    def rollout(self, substeps=8, restart=False, need=DMIN):
        """The last solution applied to the CONTINUOUS kinematic bicycle, ON THE DEVICE (obca_batch_rollout; the numpy statement is obca_amd.validate.rollout_parking +
        rollout_record): u_k held over interval k, classical RK4 with `substeps` steps per interval.  restart=False: the open loop from the solution's first node;
        True: every interval starts at the solution's own node -- the defect of one interval.  validate() and clearance() measure against the NLP's midpoint rule; this
        is what the car does.  Returns the dict of _rollout: deviations of the rolled node states from the solution's, and `clearance`, the dict of clearance() for the
        rolled samples (need: its `need`).  The rolled states stay on the device: rollout_states()."""
        return self._rollout(int(self.nObs.max()), substeps, restart, need)

    def advance(self, shift, substeps=8, kick=None, need=DMIN):
        """One step of the closed receding-horizon loop, ON THE DEVICE in one launch (obca_batch_advance; the numpy statement is obca_amd.validate.advance_parking +
        advance_record): the continuous bicycle of rollout() is driven from the record's X0 over the first `shift` intervals of the last solution, `kick` ((4,) or (B,4);
        the process disturbance) is added to the state it reaches, and the next solve is restarted exactly as shift_warm_start(shift, x0_new=<that state>) restarts it --
        the state never leaves the device.  Returns the dict of _advance.  The batch counts as unsolved afterwards: solve() again, that re-solve is the feedback of this
        loop (track() is the tool between two re-solves).  advance_state(), advance_log(), advance_log_states(), advance_ms()."""
        return self._advance(int(self.nObs.max()), shift, substeps, need, kick)

    def track(self, substeps=8, dx0=None, Q=None, R=None, Qf=None, feedback=True, clamp=True, need=DMIN):
        """The last solution TRACKED on the continuous kinematic bicycle by a time-varying LQR about it, ON THE DEVICE (obca_batch_track; the numpy statement is
        obca_amd.validate.track_parking + track_record): the gains come from the derivative of the map the plant applies over an interval (`substeps` RK4 steps, the input
        held) and a backward Riccati recursion with diagonal weights Q (4), R (2), Qf (4) -- defaults TRACK_Q_PARKING, TRACK_R_PARKING, 10 Q; untuned --, the loop starts at
        x0 + dx0 (dx0: (4,) or (B,4)), applies u_k + K_k (X_k - x_k) held over interval k (feedback=False: u_k) and clips it to |delta| <= 0.6, |a| <= 0.4 (clamp).  Returns the
        dict of _track: the deviations and the clearance of the driven path as rollout() reports them, and saturated, du_max, du_node, dx0_pos, feedback, clamp.  States and
        gains stay on the device: track_states(), track_gains()."""
        return self._track(int(self.nObs.max()), (TRACK_Q_PARKING, TRACK_R_PARKING, TRACK_QF_PARKING), substeps, dx0, Q, R, Qf, feedback, clamp, need)

    def ensemble(self, members=64, substeps=8, dx0=None, dub=None, Q=None, R=None, Qf=None, feedback=True, clamp=True, need=DMIN):
        """`members` (1 .. 64) disturbed closed loops about the last solution at once, ON THE DEVICE (obca_batch_ensemble; the numpy statement is
        obca_amd.validate.ensemble_parking + ensemble_record): the gains of track() -- computed once per instance --, member m started at the solution's first state +
        dx0[m] (dx0 (M,4) for every instance or (B,M,4); None: zeros) and driven by clip(u_k + K_k (X_k - x_k) + dub[m]) (dub (M,2) or (B,M,2), a constant actuator bias
        per member; None: zeros).  One member per lane of the instance's wavefront: 64 members cost one launch, where 64 track() calls recompute the same gains 64 times
        with 63 lanes idle.  Every sample a member passes is measured against the obstacles as rollout() measures it.  Returns the dict of _ensemble: over the members of an
        instance, how far the vehicle strays and how close it comes -- the distribution a refine(margin=...) is chosen from.  ensemble_offsets() draws dx0 / dub.  Member
        records and final states stay on the device: ensemble_members(), ensemble_final()."""
        return self._ensemble((TRACK_Q_PARKING, TRACK_R_PARKING, TRACK_QF_PARKING), members, substeps, dx0, dub, Q, R, Qf, feedback, clamp, need)

    def clearance(self, substeps=8, need=DMIN):
        """Clearance of the last solution BETWEEN its nodes, ON THE DEVICE (obca_batch_clearance; the numpy statement is obca_amd.validate.parking_samples + a DualMultWS
        distance per pose): every interval is sampled `substeps` times with the discretisation's own partial step and the car's distance to every obstacle computed anew,
        0 = touches or overlaps.  validate() looks at the nodes only; a solution can pass it and cut a corner in between.  Returns the dict of _clearance; only 24 numbers
        per instance are downloaded."""
        return _clearance(self.B, substeps, int(self.nObs.max()), lambda out: self._call("clearance", int(substeps), float(need), out))

    def certify(self, need=DMIN, slack=0.01, max_steps=CERT_TICKS):
        """A CERTIFICATE for the clearance of the last solution along its WHOLE path, ON THE DEVICE (obca_batch_certify; the numpy statement is
        obca_amd.validate.certify_parking + certify_record): clearance() samples `substeps` poses per interval and says nothing about what lies between them.  Here every
        (interval, obstacle) pair is walked by conservative advancement -- a pose with clearance c clears the stretch on which no point of the car moves farther than c, the
        next sample goes to its end --, so samples go where the path is close to an obstacle and a far obstacle costs one.  certified: clearance >= need - slack everywhere
        on the path the discretisation's own partial step draws between the nodes; otherwise a sample under `need` was found (violated, first_violation) or an item ran out
        of max_steps (undecided).  Returns the dict of _certify; 16 numbers per instance are downloaded, certify_intervals() fetches the per-interval bounds."""
        return self._certify(need, slack, max_steps)

    def predict_clearance(self, rates=None, pivot=None, grow=None, substeps=8, need=DMIN, profile=False):
        """Clearance of the last solution against obstacles that MOVE while it is driven, ON THE DEVICE (obca_batch_predict_clearance; the numpy statement is
        obca_amd.validate.predict_parking + predict_record).  clearance() holds the scene as it stands now for the whole horizon; here sample q, reached at the time
        tau_q = (sum of the t_k before its interval + (s / S) t_k) Ts, is measured against the scene move_obstacles(rates * tau_q, pivot, grow * tau_q) WOULD make --
        nothing is written to the batch.  rates: (vx, vy, w) per second as (3,), (B,3) or (nOb_total,3); pivot: (cx, cy) as move_obstacles takes it; grow: g metres per
        second of margin (prediction uncertainty that widens with time) as a scalar, (B,) or (nOb_total,); None: zeros.  Returns the dict of _predict: the dict of
        clearance() and first / t_first (the first sample under `need` and its time: an instance with a finite t_first is one to re-solve now), first_obstacle, t_min,
        horizon, moving.  With all rates 0 it is clearance().  inflate = rate x horizon can be checked here before a refine() pays for it; after advance() and
        move_obstacles() the same call answers for the new step.  profile=True keeps the smallest clearance of every sample on the device: predict_profile()."""
        return self._predict(int(self.nObs.max()), _parking_rates(self.nObs, rates, pivot, grow), substeps, need, profile)

    def move_obstacles(self, motion=None, pivot=None, inflate=None):
        """The obstacles of the uploaded batch MOVED AND INFLATED IN PLACE, ON THE DEVICE (obca_batch_move_obstacles; the numpy statement is
        obca_amd.validate.move_obstacles_parking): obstacle j = {p : A p <= b} becomes its image under p' = R(dth)(p - c) + c + d and then grows by m metres (m < 0
        shrinks it).  motion: (dx, dy, dth) as (3,) for every obstacle, (B,3) over each instance's obstacles or (nOb_total,3) packed in upload order; pivot: (cx, cy) as
        (2,), (B,2) or (nOb_total,2), None: the world origin; inflate: m as a scalar, (B,) or (nOb_total,).  The batch may be solved or not, and stays what it was: the
        solved state, the start iterate, the last solution and its multipliers, the plant state and the advance log are not touched, so shift_warm_start() / advance()
        and a solve with warm_restart_opts() restart in the moved scene, validate() / clearance() / certify() of the held solution answer "is my plan still clear in the
        scene as it is now", plan_warm_start() replans in the moved field, and refine() + move_obstacles(inflate=m) on the result is the parking margin.  What earlier
        calls computed and kept -- certify_intervals(), rollout_states(), track_states(), ensemble_members(), plan_paths() -- describes the scene it was computed in.
        Returns status (B,) int32: 0 moved; 1 marks an instance with a non-finite motion, pivot, inflation or result, ALONE -- its record keeps every bit.  With dth == 0
        the words of A keep their bits; an obstacle with nothing to do keeps every bit.  obstacles(), move_obstacles_ms()."""
        st = np.zeros(self.B, np.int32)
        self._call("move_obstacles", _per_obstacle(motion, self.nObs, 3), _per_obstacle(pivot, self.nObs, 2), _per_obstacle(inflate, self.nObs, 0), st)
        return st

    def obstacles(self):
        """The obstacle rows as the device holds them now: (A (M_total,2), b (M_total,)) packed as upload() takes them.  They are the UNIT-LENGTH rows of the problem
        records -- not scaled back by the row lengths upload() divided out (the same half-planes; download() still returns lambda in the caller's scaling)."""
        Mt = int(self.Ms.sum())
        A = np.zeros((Mt, 2)); b = np.zeros(Mt)
        self._call("obstacles_download", A, b)
        return A, b

    def refine(self, factor=2, select=None, duals=False, into=None):
        """The solved instances `select` (an index array or a boolean mask over this batch's instances; None: all, duplicates allowed) on the horizon factor * N, ON THE
        DEVICE (obca_batch_refine_into; the numpy statement is obca_amd.validate.refine_parking): the same NLP with Ts / factor, the tracking reference interpolated, and
        as start the solution itself -- its nodes, between them the poses clearance(substeps=factor) sampled, u held, t = 1.  duals=False: the next solve runs DualMultWS;
        duals=True: stage q starts from the multipliers of stage q // factor (solve with warm_restart_opts(): about 0.55 of the iterations on the oracle; the default is the
        safer one).  into: a Batch of this context with horizon factor * N and room for the selection; None: a new one.  Returns (batch, status) with status (n,) int32,
        REFINE_STATUS: 0 refined from the solution, 1 from the start iterate (the last solve failed or left non-finite numbers), -1 zero start.  The result is uploaded, not
        solved; only `status` crosses the bus."""
        dst, sel, st = self._refine_into("obca_batch_refine_into", REFINE_MAXFACTOR, int(duals), select, factor, into)
        dst.nObs = self.nObs[sel]; dst.Ms = self.Ms[sel]
        ends = np.cumsum(self.nObs); dst.vflat = np.concatenate([self.vflat[ends[i] - self.nObs[i]:ends[i]] for i in sel.tolist()])
        return dst, st

    def refine_ms(self):
        """HIP-event duration of the last refine kernel that wrote into THIS batch (the destination of refine)"""
        return self._floats("refine_ms")


def hybrid_configure(slots=0, max_nodes=0, max_chunks=0, device=0):
    """the slots of the device planner of a context (obca_hybrid_configure): searches in flight, nodes and bucket chunks per search; 0 = the default"""
    ctx = _ctx(device)
    ctx._check(_load().obca_hybrid_configure(ctx._h, int(slots), int(max_nodes), int(max_chunks)), "obca_hybrid_configure")


def parking_rollout_batch(N, Ts, L, ego, vOb, A, b, x, u, timeScale=None, substeps=8, restart=False, need=DMIN, device=0, states=True):
    """Batch.rollout for arbitrary trajectories (obca_parking_rollout_batch): the arguments of parking_clearance_batch, then the mode.  Returns the dict of Batch.rollout,
    with `states` (B, N+1, 4), the rolled node states, unless states=False."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = int(N); B = x.shape[0]
    if x.shape != (B, 4, N + 1) or u.shape != (B, 2, N):
        raise ObcaError(f"x must be (B,4,N+1) and u (B,2,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    nObs, vflat, Aflat, bflat = _norm_obstacles(B, vOb, A, b)
    ins = (_per_instance(Ts, B), L, _in(ego), _in(nObs, np.int32), _in(vflat, np.int32), _in(Aflat), _in(bflat), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))),
           None if timeScale is None else _time_scale(timeScale, B, N + 1), int(substeps), int(restart), float(need))
    X = np.zeros((B, N + 1, 4)) if states else None
    r = _rollout(B, substeps, int(nObs.max()), lambda out: ctx._check(_load().obca_parking_rollout_batch(ctx._h, B, N, *ins, out, X), "obca_parking_rollout_batch"))
    return dict(r, **({"states": X} if states else {}))


def parking_track_batch(N, Ts, L, ego, vOb, A, b, x, u, timeScale=None, substeps=8, dx0=None, Q=None, R=None, Qf=None, feedback=True, clamp=True, need=DMIN, device=0,
                        states=True, gains=True):
    """Batch.track for arbitrary trajectories (obca_parking_track_batch): the arguments of parking_rollout_batch, then those of Batch.track.  Returns the dict of
    Batch.track, with `states` (B, N+1, 4) and `gains` (B, N, 2, 4) unless states=False / gains=False."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = int(N); B = x.shape[0]
    if x.shape != (B, 4, N + 1) or u.shape != (B, 2, N):
        raise ObcaError(f"x must be (B,4,N+1) and u (B,2,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    nObs, vflat, Aflat, bflat = _norm_obstacles(B, vOb, A, b)
    q, r, qf = _track_weights(4, 2, Q, R, Qf, (TRACK_Q_PARKING, TRACK_R_PARKING, TRACK_QF_PARKING))
    ins = (_per_instance(Ts, B), L, _in(ego), _in(nObs, np.int32), _in(vflat, np.int32), _in(Aflat), _in(bflat), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))),
           None if timeScale is None else _time_scale(timeScale, B, N + 1), int(substeps), int(feedback), int(clamp), q, r, qf, _track_dx0(dx0, B, 4), float(need))
    X = np.zeros((B, N + 1, 4)) if states else None; K = np.zeros((B, N, 2, 4)) if gains else None
    t = _track(B, substeps, int(nObs.max()), lambda out: ctx._check(_load().obca_parking_track_batch(ctx._h, B, N, *ins, out, X, K), "obca_parking_track_batch"))
    return dict(t, **({"states": X} if states else {}), **({"gains": K} if gains else {}))


def _ensemble_host(B, M, nx, call, members, final):
    """what the two host-pointer ensemble calls share: the outputs, `call(out, mem, fin)`, and the dict"""
    mem = np.zeros((B, M, ENS_MEM)) if members else None; fin = np.zeros((B, M, nx)) if final else None
    r = _ensemble(B, lambda out: call(out, mem, fin))
    return dict(r, **({"member_records": mem} if members else {}), **({"final": fin} if final else {}))


def parking_ensemble_batch(N, Ts, L, ego, vOb, A, b, x, u, timeScale=None, members=64, substeps=8, dx0=None, dub=None, Q=None, R=None, Qf=None, feedback=True, clamp=True,
                           need=DMIN, device=0, member_records=True, final=True):
    """Batch.ensemble for arbitrary trajectories (obca_parking_ensemble_batch): the arguments of parking_track_batch up to timeScale, then those of Batch.ensemble.  Returns
    the dict of Batch.ensemble, with `member_records` (B, M, 16) and `final` (B, M, 4) unless switched off."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = int(N); B = x.shape[0]; M = int(members)
    if x.shape != (B, 4, N + 1) or u.shape != (B, 2, N):
        raise ObcaError(f"x must be (B,4,N+1) and u (B,2,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    nObs, vflat, Aflat, bflat = _norm_obstacles(B, vOb, A, b)
    q, r, qf = _track_weights(4, 2, Q, R, Qf, (TRACK_Q_PARKING, TRACK_R_PARKING, TRACK_QF_PARKING))
    Mc = min(max(M, 1), ENS_MMAX)      # (a count the library refuses still needs arrays of some shape)
    ins = (_per_instance(Ts, B), L, _in(ego), _in(nObs, np.int32), _in(vflat, np.int32), _in(Aflat), _in(bflat), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))),
           None if timeScale is None else _time_scale(timeScale, B, N + 1), int(substeps), M, int(feedback), int(clamp), q, r, qf, _ensemble_rows(dx0, B, Mc, 4, "dx0"),
           _ensemble_rows(dub, B, Mc, 2, "dub"), float(need))
    return _ensemble_host(B, Mc, 4, lambda out, mem, fin: ctx._check(_load().obca_parking_ensemble_batch(ctx._h, B, N, *ins, out, mem, fin), "obca_parking_ensemble_batch"),
                          member_records, final)


def _context_ms(entry, device):
    """the HIP-event duration [ms] that `entry` reports for the context of `device`"""
    ctx = _ctx(device); a = C.c_float(0)
    ctx._check(getattr(_load(), entry)(ctx._h, C.byref(a)), entry)
    return a.value


def hybrid_ms(device=0):
    """HIP-event duration of the last search kernel of the context's device planner [ms]"""
    return _context_ms("obca_hybrid_ms", device)


def _astar_batch(entry, field, starts, goals, ego, L, XYbounds, opts, bucket_width, cap, device):
    """what hybrid_astar_batch and scene_astar_batch share; `field`: the obstacle arguments as `entry` takes them, marshalled"""
    s = np.ascontiguousarray(np.asarray(starts, float)[:, :3]); g = np.ascontiguousarray(np.asarray(goals, float)[:, :3]); B = len(s); cap = int(cap)
    o = None if opts is None else np.ascontiguousarray(opts, float)
    paths = np.zeros((B, max(cap, 0), 3)); dirs = np.zeros((B, max(cap, 0)), np.int32); cnt = np.zeros(B, np.int32); nexp = np.zeros(B, np.int32); rounds = np.zeros(B, np.int32)
    ctx = _ctx(device)
    rc = getattr(_load(), entry)(ctx._h, B, s, g, *field, _in(ego), float(L), _in(XYbounds), o, 0 if o is None else len(o),
                                 0.0 if bucket_width is None else float(bucket_width), paths, dirs, cap, cnt, nexp, rounds)
    ctx._check(rc, entry)
    return paths, dirs, cnt, nexp, rounds


def hybrid_astar_batch(starts, goals, vOb, A, b, ego, L, XYbounds, opts=None, bucket_width=None, cap=1024, device=0):
    """obca_hybrid_astar_batch as it is: B Hybrid A* searches in one obstacle field on the GPU, one workgroup each.  starts, goals (B, >= 3); opts: the option array of
    obca_plan.h or None.  Returns (paths (B, cap, 3), dirs (B, cap), counts (B,), expansions (B,), rounds (B,)); counts as the host planner's, -3: HYBRID_STATUS."""
    vOb = np.ascontiguousarray(vOb, np.int32)
    return _astar_batch("obca_hybrid_astar_batch", (len(vOb), vOb, _in(A), _in(b)), starts, goals, ego, L, XYbounds, opts, bucket_width, cap, device)


def scene_ms(device=0):
    """HIP-event duration of the last per-instance search kernel (scene_astar_batch) of the context's device planner [ms]; hybrid_ms keeps the shared-field one"""
    return _context_ms("obca_scene_astar_ms", device)


def scene_astar_batch(starts, goals, vOb, A, b, ego, L, XYbounds, opts=None, bucket_width=None, cap=1024, device=0):
    """obca_scene_astar_batch: B Hybrid A* searches on the GPU, one workgroup each, every search in the obstacle field of ITS OWN instance.  vOb, A, b: per-instance lists
    (taken as they are) or one field (broadcast), as everywhere here (_norm_obstacles); an instance without obstacles is a free field inside XYbounds.  The rest is
    hybrid_astar_batch's: starts, goals (B, >= 3), opts, the slots of hybrid_configure, the return value (paths (B, cap, 3), dirs (B, cap), counts (B,), expansions (B,),
    rounds (B,)) and the counts codes (HYBRID_STATUS; -2: the pose collides with the instance's own field)."""
    nObs, vflat, Aflat, bflat = _norm_obstacles(len(starts), vOb, A, b)
    return _astar_batch("obca_scene_astar_batch", (_in(nObs, np.int32), _in(vflat, np.int32), _in(Aflat), _in(bflat)), starts, goals, ego, L, XYbounds, opts, bucket_width, cap, device)


def parking_refine_batch(N, Ts, L, x, u, timeScale=None, factor=2, device=0):
    """The primal part of Batch.refine for arbitrary trajectories (obca_parking_refine_batch): x (B,4,N+1), u (B,2,N) -- the shapes the solve calls return --, timeScale scalar,
    (B,), (B,N+1) or None (= 1), used per stage as in parking_clearance_batch.  Returns dict(Ts (B,) = Ts / factor, x (B,4,factor N+1), u (B,2,factor N)); an instance with a
    non-finite number among its inputs comes back as NaN."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = int(N); B = x.shape[0]; r = int(factor)
    if x.shape != (B, 4, N + 1) or u.shape != (B, 2, N):
        raise ObcaError(f"x must be (B,4,N+1) and u (B,2,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    Nf = N * max(r, 0); Tsf = np.zeros(B); xf = np.zeros((B, Nf + 1, 4)); uf = np.zeros((B, Nf, 2))
    rc = _load().obca_parking_refine_batch(ctx._h, B, N, r, _per_instance(Ts, B), float(L), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))),
                                           None if timeScale is None else _time_scale(timeScale, B, N + 1), Tsf, xf, uf)
    ctx._check(rc, "obca_parking_refine_batch")
    return dict(Ts=Tsf, x=np.transpose(xf, (0, 2, 1)), u=np.transpose(uf, (0, 2, 1)))


def parking_signed_dist_batch(x0, xF, N, Ts, L, ego, XYbounds, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS, lWS=None, nWS=None,
                              opts=None, device=0, dist=False, buffers=None):
    """Batched ParkingSignedDist through the host-pointer entry point obca_parking_(signed_)dist_batch (what the Julia shim calls):
    x0,xF (B,4); rx,ry,ryaw (B,N+1); xWS (B,N+1,4); uWS (B,>=N,2); Ts scalar or (B,).
    Obstacles: one shared set (vOb 1-D, A (M,2), b (M,)) or per-instance lists.  lWS/nWS=None runs DualMultWS on the GPU.
    `device`: an index, a list of indices or "all" (the batch is then sharded over the devices, obca_create_multi), or a Context.
    `buffers`: a dict the caller keeps between calls; the output arrays live in it and are written again by the next call of the same shape (a
    16 384-instance call returns 280 MB: fresh arrays cost a page fault per 4 KB inside the C call, tools/pcie_rate.py measures both)."""
    x0 = np.reshape(x0, (-1, 4)); B = x0.shape[0]
    ctx = _ctx(device)
    nObs, Ms, prob = _problem(B, Ts, L, ego, XYbounds, fixTime, x0, xF, vOb, A, b)
    Mt, nt = int(Ms.sum()), int(nObs.sum())
    lWS, nWS = _dual_start(lWS, nWS, Mt, nt, N)
    ins = (*prob, *(_in(np.reshape(r, (B, N + 1))) for r in (rx, ry, ryaw)), *(_in(w) for w in _warm_start(xWS, uWS, B, N)), _in(lWS), _in(nWS), _ref(opts))
    shapes = dict(xp=(B, N + 1, 4), up=(B, N, 2), ts=(B, N + 1), ef=(B,), lp=(Mt * (N + 1),), npp=(4 * nt * (N + 1),), sl=(nt * (N + 1),), info=(B, 8))      # in the ABI's order
    bufs = buffers if buffers is not None else {}
    for k, shp in shapes.items():
        if k not in bufs or bufs[k].shape != shp:
            bufs[k] = np.zeros(shp, np.int32 if k == "ef" else float) if k in ("ef", "sl", "info") else np.empty(shp)
    xp, up, ts, ef, lp, npp, sl, info = (bufs[k] for k in shapes)
    name = "obca_parking_dist_batch" if dist else "obca_parking_signed_dist_batch"      # the same arguments but for `slp`, which the dist entry point does not have
    fn = getattr(_load(), name)
    t0 = time.perf_counter()
    rc = fn(ctx._h, B, int(N), *ins, xp, up, ts, ef, lp, npp, *(() if dist else (sl,)), info)
    dt = time.perf_counter() - t0
    ctx._check(rc, name)
    out = _unpack_parking(B, N, nObs, Ms, xp, up, ts, ef, lp, npp, sl, info)
    out["time"] = dt
    return out


def _unpack_parking(B, N, nObs, Ms, xp, up, ts, ef, lp, npp, sl, info):
    """C-ABI output arrays -> the reference's shapes: xp (B,4,N+1), up (B,2,N), per-instance lp (M,N+1) / np (4nOb,N+1) / sl (nOb,N+1): lists for ragged obstacle sets, (B, ., N+1) arrays for uniform ones"""
    if len(set(Ms.tolist())) == 1 and len(set(nObs.tolist())) == 1:          # uniform obstacle sets: one reshape, views per instance
        m, n = int(Ms[0]), int(nObs[0])
        L3 = lp.reshape(B, N + 1, m).transpose(0, 2, 1); N3 = npp.reshape(B, N + 1, 4 * n).transpose(0, 2, 1); S3 = sl.reshape(B, N + 1, n).transpose(0, 2, 1)
        lps, nps, sls = L3, N3, S3                                             # (B, M, N+1) views: lp[i] is instance i's (M, N+1) array, as in the ragged case -- no 3 x B Python objects
    else:
        lps, nps, sls = ([x.T for x in _blocks(a, rows, N + 1)] for a, rows in ((lp, Ms), (npp, 4 * nObs), (sl, nObs)))
    return dict(xp=np.transpose(xp, (0, 2, 1)), up=np.transpose(up, (0, 2, 1)), timeScale=ts, exitflag=ef,
                lp=lps, np=nps, sl=sls, info=info, iters=info[:, 1].astype(int), obj=info[:, 2], status=info[:, 0].astype(int))


def _parking_one(dist, x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS, opts, device):
    """one instance through the batched call, returned as the reference's 7-tuple"""
    assert int(nOb) == len(np.ravel(vOb))
    opts = ipopt_opts() if opts is None else opts
    r = parking_signed_dist_batch(np.reshape(x0, (1, 4)), np.reshape(xF, (1, 4)), N, Ts, L, ego, XYbounds, vOb, A, b,
                                  np.reshape(np.ravel(rx)[:N + 1], (1, -1)), np.reshape(np.ravel(ry)[:N + 1], (1, -1)),
                                  np.reshape(np.ravel(ryaw)[:N + 1], (1, -1)), fixTime, np.asarray(xWS, float)[None, :N + 1],
                                  np.asarray(uWS, float)[None, :N], opts=opts, device=device, dist=dist)
    ts = np.ones((1, N + 1)) if fixTime else r["timeScale"][0]          # ParkingSignedDist.jl:304-308
    return r["xp"][0], r["up"][0], ts, int(r["exitflag"][0]), r["time"], r["lp"][0], r["np"][0]


def ParkingSignedDist(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS, opts=None, device=0):
    """Drop-in for ParkingSignedDist.jl:29 (one instance).  Returns (xp, up, timeScalep, exitflag, time, lp, np).
    opts=None runs the reference's IPOPT configuration (ipopt_opts(): recalc_y = "yes" as ParkingSignedDist.jl:41 sets it, IPOPT's default second-order correction and
    least-squares initial multipliers); pass default_opts() for the library's throughput defaults (include/obca_hip.h says what the difference costs and changes)."""
    return _parking_one(False, x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS, opts, device)


def ParkingDist(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS, opts=None, device=0):
    """Drop-in for ParkingDist.jl:29 (the collision-free sibling of ParkingSignedDist): same arguments, same 7-tuple.  opts=None: the reference's IPOPT configuration
    (ParkingDist.jl:41 sets recalc_y = "yes" as well), see ParkingSignedDist."""
    return _parking_one(True, x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS, opts, device)


def _pack_cols(a, B, rows, N1, what):
    """per-instance (rows_i, N+1) arrays (a list, or one (B, rows, N+1) array) -> the C ABI's packed stage-contiguous blocks"""
    out = np.concatenate([np.ascontiguousarray(np.asarray(a[i], float).T).ravel() for i in range(B)])
    if out.size != int(np.sum(rows)) * N1:
        raise ObcaError(f"{what} has the wrong size: {out.size} (need {int(np.sum(rows)) * N1})")
    return out


def parking_constraints_batch(x0, xF, N, Ts, L, ego, XYbounds, vOb, A, b, x, u, timeScale, l, n, sl=None, fixTime=0, dist=False, tol=5e-5, device=0):
    """Batched ParkingConstraints on the device for arbitrary trajectories (obca_parking_constraints_batch): x (B,4,N+1), u (B,2,N), l / n / sl per instance
    (M_i,N+1) / (4nOb_i,N+1) / (nOb_i,N+1) -- the shapes the solve calls return --, timeScale scalar, (B,) or (B,N+1) (it may vary over the stages).
    Obstacles and `device` as in parking_signed_dist_batch.  Returns dict(ok, ref_ok, viol (B,14), names) like Batch.validate; sl=None: zeros."""
    x0 = np.reshape(x0, (-1, 4)); B = x0.shape[0]; N = int(N)
    ctx = _ctx(device)
    nObs, Ms, prob = _problem(B, Ts, L, ego, XYbounds, fixTime, x0, xF, vOb, A, b)
    x = np.asarray(x, float); u = np.asarray(u, float)
    if x.shape != (B, 4, N + 1) or u.shape != (B, 2, N):
        raise ObcaError(f"x must be (B,4,N+1) and u (B,2,N); got {x.shape}, {u.shape}")
    ins = (*prob, bool(dist), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))), _time_scale(timeScale, B, N + 1), _pack_cols(l, B, Ms, N + 1, "l"),
           _pack_cols(n, B, 4 * nObs, N + 1, "n"), _pack_cols(sl, B, nObs, N + 1, "sl") if sl is not None else None, tol)
    return _verdict(B, VIOL_NAMES, lambda *out: ctx._check(_load().obca_parking_constraints_batch(ctx._h, B, N, *ins, *out), "obca_parking_constraints_batch"), ref_ok=True)


def parking_certify_batch(N, Ts, L, ego, vOb, A, b, x, u, timeScale=None, need=DMIN, slack=0.01, max_steps=CERT_TICKS, device=0, intervals=True):
    """Batch.certify for arbitrary trajectories (obca_parking_certify_batch): the arguments of parking_clearance_batch up to timeScale, then those of Batch.certify.  Returns
    the dict of Batch.certify, with `intervals` (B, N+1, 2) unless switched off."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = int(N); B = x.shape[0]
    if x.shape != (B, 4, N + 1) or u.shape != (B, 2, N):
        raise ObcaError(f"x must be (B,4,N+1) and u (B,2,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    nObs, vflat, Aflat, bflat = _norm_obstacles(B, vOb, A, b)
    ins = (_per_instance(Ts, B), L, _in(ego), _in(nObs, np.int32), _in(vflat, np.int32), _in(Aflat), _in(bflat), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))),
           None if timeScale is None else _time_scale(timeScale, B, N + 1), float(need), float(slack), int(max_steps))
    iv = np.zeros((B, N + 1, 2)) if intervals else None
    r = _certify(B, lambda out: ctx._check(_load().obca_parking_certify_batch(ctx._h, B, N, *ins, out, iv), "obca_parking_certify_batch"))
    return dict(r, intervals=iv) if intervals else r


def parking_clearance_batch(N, Ts, L, ego, vOb, A, b, x, u, timeScale=None, substeps=8, need=DMIN, device=0):
    """Batch.clearance for arbitrary trajectories (obca_parking_clearance_batch): x (B,4,N+1), u (B,2,N) -- the shapes the solve calls return --, timeScale scalar, (B,),
    (B,N+1) or None (= 1).  The arguments are those of parking_constraints_batch, in its order, that the check reads: no start, goal, bounds or multipliers.  Obstacles and
    `device` as in parking_signed_dist_batch.  Returns the dict of Batch.clearance."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = int(N); B = x.shape[0]
    if x.shape != (B, 4, N + 1) or u.shape != (B, 2, N):
        raise ObcaError(f"x must be (B,4,N+1) and u (B,2,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    nObs, vflat, Aflat, bflat = _norm_obstacles(B, vOb, A, b)
    ins = (_per_instance(Ts, B), L, _in(ego), _in(nObs, np.int32), _in(vflat, np.int32), _in(Aflat), _in(bflat), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))),
           None if timeScale is None else _time_scale(timeScale, B, N + 1), int(substeps), float(need))
    return _clearance(B, substeps, int(nObs.max()), lambda out: ctx._check(_load().obca_parking_clearance_batch(ctx._h, B, N, *ins, out), "obca_parking_clearance_batch"))


def parking_predict_batch(N, Ts, L, ego, vOb, A, b, x, u, timeScale=None, rates=None, pivot=None, grow=None, substeps=8, need=DMIN, device=0, profile=False):
    """Batch.predict_clearance for arbitrary trajectories (obca_parking_predict_batch): the arguments of parking_clearance_batch up to timeScale, then those of
    Batch.predict_clearance.  Returns its dict, with `profile` (B, N substeps + 1) if asked for."""
    x = np.asarray(x, float); u = np.asarray(u, float); N = int(N); B = x.shape[0]
    if x.shape != (B, 4, N + 1) or u.shape != (B, 2, N):
        raise ObcaError(f"x must be (B,4,N+1) and u (B,2,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    nObs, vflat, Aflat, bflat = _norm_obstacles(B, vOb, A, b)
    ins = (_per_instance(Ts, B), L, _in(ego), _in(nObs, np.int32), _in(vflat, np.int32), _in(Aflat), _in(bflat), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))),
           None if timeScale is None else _time_scale(timeScale, B, N + 1), int(substeps), float(need))
    rt = _parking_rates(nObs, rates, pivot, grow).reshape(-1); pr = np.zeros((B, N * max(int(substeps), 0) + 1)) if profile else None
    r = _predict(B, substeps, int(nObs.max()), lambda out: ctx._check(_load().obca_parking_predict_batch(ctx._h, B, N, *ins, out, rt, None if pr is None else pr.reshape(-1)),
                                                                     "obca_parking_predict_batch"))
    return dict(r, profile=pr) if profile else r


def ParkingConstraints(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd, device=0):
    """Drop-in for ParkingConstraints.jl:29 (one instance): 1 if the reference's own acceptance test passes at 5e-5, else 0 (sd = 1: signed-distance formulation)."""
    assert int(nOb) == len(np.ravel(vOb))
    r = parking_constraints_batch(np.reshape(x0, (1, 4)), np.reshape(xF, (1, 4)), N, Ts, L, ego, XYbounds, vOb, A, b, np.asarray(x, float)[None], np.asarray(u, float)[None],
                                  np.reshape(np.broadcast_to(np.ravel(np.asarray(timeScale, float)), (N + 1,)), (1, N + 1)), [l], [n], None, fixTime, dist=not int(sd), device=device)
    return int(r["ref_ok"][0])


def dualmult_ws_batch(N, vOb, A, b, rx, ry, ryaw, ego, device=0):
    """Batched DualMultWS: rx,ry,ryaw (B,N+1) -> lWS list of (N+1,M), nWS list of (N+1,4nOb), d list of (N+1,nOb)."""
    rx = np.atleast_2d(np.asarray(rx, float)); B = rx.shape[0]
    ctx = _ctx(device)
    nObs, vflat, Aflat, bflat = _norm_obstacles(B, vOb, A, b)
    Ms = _row_counts(nObs, vflat)
    Mt, nt = int(Ms.sum()), int(nObs.sum())
    lw = np.zeros(Mt * (N + 1)); nw = np.zeros(4 * nt * (N + 1)); dd = np.zeros(nt * (N + 1))
    rc = _load().obca_dualmult_ws_batch(ctx._h, B, N, _in(ego), _in(nObs, np.int32), _in(vflat, np.int32), _in(Aflat), _in(bflat), _in(rx), _in(np.atleast_2d(ry)),
                                        _in(np.atleast_2d(ryaw)), lw, nw, dd)
    ctx._check(rc, "obca_dualmult_ws_batch")
    return tuple([x.copy() for x in _blocks(a, rows, N + 1)] for a, rows in ((lw, Ms), (nw, 4 * nObs), (dd, nObs)))


def DualMultWS(N, nOb, vOb, A, b, rx, ry, ryaw, ego, device=0):
    """Drop-in for DualMultWS.jl:29 -> (lp (N+1,M), np (N+1,4nOb)); `ego` is explicit (the reference uses a global)."""
    assert int(nOb) == len(np.ravel(vOb))
    ls, ns, _ = dualmult_ws_batch(N, vOb, A, b, np.ravel(rx)[None, :N + 1], np.ravel(ry)[None, :N + 1],
                                  np.ravel(ryaw)[None, :N + 1], ego, device)
    return ls[0], ns[0]


# ---------------------------------------------------------------- quadcopter path (QuadcopterSignedDist.jl)
def quadcopter_default_opts():
    return _opts("obca_quadcopter_default_opts")


def quadcopter_ipopt_opts():
    """the reference's IPOPT configuration of the quadcopter call as far as the kernel carries it (obca_quadcopter_reference_opts: max_soc = 4, least-squares
    initial multipliers, gradient-based objective scaling; recalc_y = "no" as QuadcopterSignedDist.jl:29 sets it): the default of the drop-ins QuadcopterSignedDist / QuadcopterDist"""
    return _opts("obca_quadcopter_reference_opts")


def quad_warm_restart_opts(reference=False):
    """options for a quadcopter solve that starts from QuadBatch.shift_warm_start: the quadcopter defaults (reference=True: the reference's IPOPT switches,
    quadcopter_ipopt_opts()) with a small initial barrier and bound push, mu_init = bound_push = bound_frac = 1e-4, so that the interior point does not first walk
    away from the previous solution.  What the restart buys, measured on the CPU checker under oracle/ (states advanced by `shift`, tail = the terminal
    stage, timeWS = the previous t, closed-form duals) on scenarios.make_quad_batch instances (the device: tools/quad_mpc_rate.py, profiles/quad_mpc_restart.json):

        N, shift, formulation           option set        iterations cold -> shifted restart            ratio
        60, 4, SignedDist (4 inst.)     throughput        108, 108, 107, 70 -> 43, 46, 44, 25           0.40
        60, 4, SignedDist (4 inst.)     reference         72, 73, 75, 77 -> 60, 50, 57, 60              0.76
        30, 3, SignedDist (6 inst.)     throughput / ref  sums 490 -> 285 / 713 -> 350                  0.58 / 0.49
        30, 3, Dist (6 inst.)           throughput / ref  sums 349 -> 301 / 458 -> 275                  0.86 / 0.60

    Every restart ended with exit flag 1 (shift = 0 and shift = N at N = 33 and 60 included); a 12-step closed loop at N = 60 (shift 2, +-0.02 disturbances on position and
    velocity per step) stayed solvable at 25-66 iterations per step against 97 cold.  The restart is not uniformly cheaper: at N = 20 one instance went from 61 to 77
    iterations, and with the COLD values of the three options a restart is often slower than a cold solve -- use these options with it.  In a closed loop with disturbed
    measured states (one MI355X, 20 steps, +-0.02 per step) reference=True kept every instance solvable; the throughput set lost 1-6 % of the instances of a step, and a lost
    instance runs into max_iter = 3 000: prefer reference=True there and cap max_iter."""
    o = quadcopter_ipopt_opts() if reference else quadcopter_default_opts()
    o.mu_init = 1e-4; o.bound_push = 1e-4; o.bound_frac = 1e-4
    return o


def _unpack_quad(T, xp, up, ts, ef, lp, sl, info):
    """C-ABI output arrays -> the reference's shapes, T = the transposition of the stage-contiguous ones (a copy for the resident batch, a view for the host-pointer call)"""
    return dict(xp=T(xp), up=T(up), timeScale=ts, exitflag=ef, lp=T(lp), slack=T(sl), info=info, iters=info[:, 1].astype(int), obj=info[:, 2], status=info[:, 0].astype(int))


class QuadBatch(_DeviceBatch):
    """Device-resident batch of quadcopter signed-distance NLPs (obca_quad_batch_* in include/obca_hip.h)."""
    _c = "obca_quad_batch"
    _nx = 12
    _nu = 4

    def upload(self, x0, xF, Ts, R, ob, xWS, timeWS, dual_ws=True, dist=False):
        B = self.B = self.capacity; N = self.N      # (an upload fills the batch)
        xw = _in(np.asarray(xWS, float)[:, :N + 1]); assert xw.shape == (B, N + 1, 12)
        self._call("upload", _per_instance(Ts, B), R, _in(np.reshape(x0, (B, 12))), _in(np.reshape(xF, (B, 12))), _boxes(ob, B), xw, _per_instance(timeWS, B), bool(dual_ws), bool(dist))

    def shift_warm_start(self, shift, x0_new=None, xF_new=None):
        """receding-horizon restart on the device (obca_quad_batch_shift_warm_start): the next solve starts from the last solution advanced by `shift` stages -- all 12 states,
        timeWS = the last t, closed-form duals --, from x0_new (B,12; the measured state; None: stage `shift` of the solution) towards xF_new (B,12; a moving goal; None: unchanged).
        An instance whose last solve failed keeps its uploaded warm start.  Solve with quad_warm_restart_opts()."""
        self._call("shift_warm_start", int(shift), *(_in(np.reshape(a, (self.B, 12))) if a is not None else None for a in (x0_new, xF_new)))

    def plan_warm_start(self, clear=0.4, room=planner.QUAD_ROOM, res=0.25, cap=planner.PLAN3D_WS_CAP, select=None, timeWS=None):
        """The resident route (obca_quad_batch_grid_plan_warm_start): the instances `select` (an index array without duplicates or a boolean mask over the batch; None: all)
        are planned ON THE DEVICE from the x0, xF and boxes the upload left there -- planner.quad_warm_start_many's search, one workgroup per instance, the defaults
        (planner.QUAD_ROOM, planner.PLAN3D_WS_CAP) its own -- and the path, resampled at N + 1 uniform arc lengths, becomes the instance's warm start (rows 3-11 zero).
        timeWS: None (every instance keeps its time scale) or one number > 0 for the planned instances.  Returns (counts, sweeps), (B,) int32 each: counts as
        planner.plan3d_paths (QUAD_PLAN_STATUS: >= 2 way-points, 0, -1, -2, -3) and -4 for an instance that was not selected; an instance with a count below 2 keeps
        its uploaded record to the last bit.  The batch counts as unsolved afterwards."""
        sel = _selection(select); n = 0 if sel is None else int(sel.size)      # (all: NULL, 0; no range check here: the library refuses a bad index)
        if sel is not None and n < 1:
            raise ObcaError("plan_warm_start: the selection is empty")
        cnt = np.zeros(self.B, np.int32); sw = np.zeros(self.B, np.int32)
        self._call("grid_plan_warm_start", float(clear), np.ascontiguousarray(room, float), float(res), int(cap), sel, n,
                   None if timeWS is None else np.array([timeWS], float), cnt, sw)
        return cnt, sw

    def plan_ms(self):
        """HIP-event duration of the last plan_warm_start's kernel [ms]"""
        return self._floats("grid_plan_ms")

    def plan_paths(self):
        """The way-points of the last plan_warm_start, for plots and tests: (B, cap, 3) -- start point, grid nodes, goal point; the rows behind an instance's count, and all
        rows of an instance the call skipped, are zero."""
        cap = _load().obca_quad_batch_grid_plan_download(self._h, None, 0)      # (no array: the call answers with the last plan's cap)
        if cap < 2:
            self.ctx._check(cap, "obca_quad_batch_grid_plan_download")
        paths = np.zeros((self.B, cap, 3))
        self._call("grid_plan_download", paths, cap)
        return paths

    def warm_start(self):
        """The start the next solve begins from, read from the records on the device (obca_quad_batch_start_download): (xWS (B, N+1, 12), timeWS (B,)).  Works on every
        uploaded batch: after upload, plan_warm_start, shift_warm_start, and on the batch refine() returned."""
        xws = np.zeros((self.B, self.N + 1, 12)); tws = np.zeros(self.B)
        self._call("start_download", xws, tws)
        return xws, tws

    def kernel_ms(self):
        return self._floats("kernel_ms")

    def download(self):
        B, N = self.B, self.N
        xp = np.zeros((B, N + 1, 12)); up = np.zeros((B, N, 4)); ts = np.zeros((B, N + 1)); ef = np.zeros(B, np.int32)
        lp = np.zeros((B, N + 1, 30)); sl = np.zeros((B, N + 1, 5)); info = np.zeros((B, 8))
        self._call("download", xp, up, ts, ef, lp, sl, info)
        return _unpack_quad(lambda a: np.transpose(a, (0, 2, 1)).copy(), xp, up, ts, ef, lp, sl, info)

    def validate(self, tol=1e-3):
        """constrSatisfaction on the last solution, on the device (obca_quad_batch_validate): dict(ok (B,) bool, viol (B, 9) in the order of `names` = QUAD_VIOL_NAMES)"""
        return _verdict(self.B, QUAD_VIOL_NAMES, lambda *out: self._call("validate", tol, *out))

    def rollout(self, substeps=8, restart=False, need=0.0):
        """The last solution applied to the continuous rigid body, on the device (obca_quad_batch_rollout; numpy: obca_amd.validate.rollout_quad + rollout_record): the
        rotor speeds held over every interval, classical RK4 with `substeps` steps per interval, the gyroscopic products at the current rates.  The NLP's rows are forward
        Euler: restart=True shows what one interval of it is off by, restart=False where the open loop ends up.  Returns the dict of Batch.rollout, 5 obstacles."""
        return self._rollout(5, substeps, restart, need)

    def advance(self, shift, substeps=8, kick=None, xF_new=None, need=0.0):
        """One step of the closed receding-horizon loop on the device (obca_quad_batch_advance; numpy: obca_amd.validate.advance_quad + advance_record): Batch.advance
        on the continuous rigid body with kick (12,) or (B,12), restarted as shift_warm_start(shift, x0_new=<the plant state>, xF_new) restarts (xF_new: (12,) or (B,12),
        a moving goal).  Solve with quad_warm_restart_opts()."""
        return self._advance(5, shift, substeps, need, kick, xF_new)

    def move_obstacles(self, motion=None, inflate=None):
        """The five boxes of every instance moved and inflated in place, on the device (obca_quad_batch_move_obstacles; numpy: obca_amd.validate.move_obstacles_quad):
        Batch.move_obstacles for axis-aligned boxes -- motion (dx, dy, dz) as (3,), (5,3), (B,3) or (B,5,3), inflate m as a scalar, (5,), (B,) or (B,5); a box
        [ub, -lb] becomes [ub + d + m, -(lb + d) + m]; R is not touched.  Returns status (B,) int32 (1: non-finite, that instance keeps every bit).  Results earlier
        calls kept (certify_intervals(), rollout_states(), ...) describe the scene they were computed in."""
        st = np.zeros(self.B, np.int32)
        self._call("move_obstacles", _per_box(motion, self.B, 3), _per_box(inflate, self.B, 0), st)
        return st

    def obstacles(self):
        """The boxes as the device holds them now: (B, 5, 6), [ub(3), -lb(3)] per box"""
        ob = np.zeros((self.B, 5, 6))
        self._call("obstacles_download", ob)
        return ob

    def track(self, substeps=8, dx0=None, Q=None, R=None, Qf=None, feedback=True, clamp=True, need=0.0):
        """The last solution tracked on the continuous rigid body by a time-varying LQR about it, on the device (obca_quad_batch_track; numpy:
        obca_amd.validate.track_quad + track_record): Batch.track with Q (12), R (4), Qf (12) -- defaults TRACK_Q_QUAD, TRACK_R_QUAD, 10 Q; untuned --, dx0 (12,) or (B,12),
        rotor speeds clipped to 1.2 .. 7.8.  The NLP's rows are forward Euler, so the solution is not a trajectory of the continuous model and the feedback cannot make it
        one: what remains is of the size of one interval's defect (rollout(restart=True)).  Returns the dict of Batch.track, 5 obstacles."""
        return self._track(5, (TRACK_Q_QUAD, TRACK_R_QUAD, TRACK_QF_QUAD), substeps, dx0, Q, R, Qf, feedback, clamp, need)

    def ensemble(self, members=64, substeps=8, dx0=None, dub=None, Q=None, R=None, Qf=None, feedback=True, clamp=True, need=0.0):
        """`members` disturbed closed loops about the last solution at once, on the device (obca_quad_batch_ensemble; numpy: obca_amd.validate.ensemble_quad +
        ensemble_record): Batch.ensemble with dx0 (M,12) or (B,M,12), dub (M,4) or (B,M,4) rotor-speed biases, the weights of QuadBatch.track."""
        return self._ensemble((TRACK_Q_QUAD, TRACK_R_QUAD, TRACK_QF_QUAD), members, substeps, dx0, dub, Q, R, Qf, feedback, clamp, need)

    def clearance(self, substeps=8, need=0.0):
        """Clearance of the last solution between its nodes, on the device (obca_quad_batch_clearance; numpy: obca_amd.validate.quad_clearance): the straight segment of every
        interval is sampled `substeps` times, clearance = distance of the point to a box - R (-R inside the box).  Returns the dict of Batch.clearance, 5 obstacles."""
        return _clearance(self.B, substeps, 5, lambda out: self._call("clearance", int(substeps), float(need), out))

    def certify(self, need=0.0, slack=0.01, max_steps=CERT_TICKS):
        """A certificate for the clearance of the last solution along its whole path, on the device (obca_quad_batch_certify; numpy: obca_amd.validate.certify_quad +
        certify_record): Batch.certify on the straight segment of every interval, speed bound |v_k|, clearance = distance of the point to a box - R."""
        return self._certify(need, slack, max_steps)

    def predict_clearance(self, rates=None, grow=None, substeps=8, need=0.0, profile=False):
        """Clearance of the last solution against boxes that move while it is flown, on the device (obca_quad_batch_predict_clearance; numpy:
        obca_amd.validate.predict_quad + predict_record): Batch.predict_clearance for axis-aligned boxes -- rates (vx, vy, vz) per second as (3,), (5,3), (B,3) or
        (B,5,3), grow g per second as a scalar, (5,), (B,) or (B,5); sample q is measured against the boxes move_obstacles(rates * tau_q, grow * tau_q) would make."""
        return self._predict(5, _quad_rates(self.B, rates, grow), substeps, need, profile)

    def refine(self, factor=2, select=None, margin=0.0, into=None):
        """The solved instances `select` (an index array or a boolean mask over this batch's instances; None: all, duplicates allowed) on the horizon factor * N, ON THE
        DEVICE (obca_quad_batch_subdivide_into; the numpy statement is obca_amd.validate.refine_quad): the same NLP with Ts / factor and the radius R + margin, and as
        warm start the solution itself -- its nodes, between them the points clearance(substeps=factor) sampled (the forward-Euler partial step) and the other nine states
        interpolated; timeWS = the solution's t, closed-form duals, as shift_warm_start leaves them.  A finer grid shrinks the cut between the nodes roughly with the square of
        the step; the chord across a box's rounded corner still sags inside, and a small margin (0.005 at N = 60 x 2, 0.02 at N = 20 x 4 on make_quad_batch) closes it.
        validate() and clearance() of the result use R + margin: clearance against the TRUE radius is clearance(need=-margin).  into: a QuadBatch of this context with
        horizon factor * N and room for the selection; None: a new one.  Returns (batch, status) with status (n,) int32, QUAD_REFINE_STATUS: 0 refined from the solution,
        1 interpolated from the uploaded warm start (the last solve failed or left non-finite numbers), -1 zero warm start.  The result is uploaded, not solved; only the
        selection and `status` cross the bus."""
        dst, _, st = self._refine_into("obca_quad_batch_subdivide_into", QUAD_SUBDIVIDE_MAXFACTOR, float(margin), select, factor, into)
        return dst, st

    def refine_ms(self):
        """HIP-event duration of the last refine kernel that wrote into THIS batch (the destination of refine)"""
        return self._floats("subdivide_ms")


def quadcopter_refine_batch(x, timeScale, Ts, factor=2, device=0):
    """The trajectory part of QuadBatch.refine for arbitrary trajectories (obca_quadcopter_subdivide_batch): x (B,12,N+1), timeScale scalar, (B,), (B,N+1) or None (= 1), used
    per stage -- the arguments of quadcopter_clearance_batch that the call reads.  Returns dict(Ts (B,) = Ts / factor, x (B,12,factor N+1)); an instance with a non-finite
    number among its inputs comes back as NaN."""
    x = np.asarray(x, float); B, _, N1 = x.shape; N = N1 - 1; r = int(factor)
    if x.shape != (B, 12, N1):
        raise ObcaError(f"x must be (B,12,N+1); got {x.shape}")
    ctx = _ctx(device)
    Tsf = np.zeros(B); xf = np.zeros((B, N * max(r, 0) + 1, 12))
    rc = _load().obca_quadcopter_subdivide_batch(ctx._h, B, N, r, _per_instance(Ts, B), _in(np.transpose(x, (0, 2, 1))),
                                                 None if timeScale is None else _time_scale(timeScale, B, N1), Tsf, xf)
    ctx._check(rc, "obca_quadcopter_subdivide_batch")
    return dict(Ts=Tsf, x=np.transpose(xf, (0, 2, 1)))


def quadcopter_signed_dist_batch(x0, xF, N, Ts, R, ob, xWS, timeWS, dual_ws=True, opts=None, device=0, dist=False):
    """Batched QuadcopterSignedDist / QuadcopterDist through the host-pointer entry points (what the Julia shim calls):
    x0,xF (B,12); ob (5,6) shared or (B,5,6); xWS (B,N+1,12); Ts, timeWS scalar or (B,).  `device` as in parking_signed_dist_batch."""
    x0 = _in(np.reshape(x0, (-1, 12))); B = x0.shape[0]
    ctx = _ctx(device)
    xw = _in(np.asarray(xWS, float)[:, :N + 1]); assert xw.shape == (B, N + 1, 12)
    ins = (_per_instance(Ts, B), R, x0, _in(np.reshape(xF, (B, 12))), _boxes(ob, B), xw, None, _per_instance(timeWS, B), bool(dual_ws), _ref(opts))      # (uWS: ignored, NULL)
    xp = np.empty((B, N + 1, 12)); up = np.empty((B, N, 4)); ts = np.empty((B, N + 1)); ef = np.zeros(B, np.int32)
    lp = np.empty((B, N + 1, 30)); sl = np.zeros((B, N + 1, 5)); info = np.zeros((B, 8))
    name = "obca_quadcopter_dist_batch" if dist else "obca_quadcopter_signed_dist_batch"      # the same arguments but for `slack`, which the dist entry point does not have
    fn = getattr(_load(), name)
    t0 = time.perf_counter()
    rc = fn(ctx._h, B, int(N), *ins, xp, up, ts, ef, lp, *(() if dist else (sl,)), info)
    dt = time.perf_counter() - t0
    ctx._check(rc, name)
    return dict(_unpack_quad(lambda a: np.transpose(a, (0, 2, 1)), xp, up, ts, ef, lp, sl, info), time=dt)


def quadcopter_constr_satisfaction_batch(x, u, timeScale, x0, xF, Ts, lam, ob, R, tol=1e-3, device=0):
    """Batched constrSatisfaction on the device for arbitrary trajectories (obca_quadcopter_constr_satisfaction_batch): x (B,12,N+1), u (B,4,N), lam (B,30,N+1) -- the
    shapes quadcopter_signed_dist_batch returns --, timeScale scalar, (B,) or (B,N+1); x0, xF (B,12) or (12,); ob (5,6) shared or (B,5,6).  Returns dict(ok, viol (B,9), names)."""
    x = np.asarray(x, float); B, _, N1 = x.shape; N = N1 - 1
    u = np.asarray(u, float); lam = np.asarray(lam, float)
    if x.shape != (B, 12, N1) or u.shape != (B, 4, N) or lam.shape != (B, 30, N1):
        raise ObcaError(f"x must be (B,12,N+1), u (B,4,N), lam (B,30,N+1); got {x.shape}, {u.shape}, {lam.shape}")
    ctx = _ctx(device)
    ins = (_per_instance(Ts, B), R, *(_in(np.broadcast_to(np.reshape(a, (-1, 12)), (B, 12))) for a in (x0, xF)), _boxes(ob, B),
           _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))), _time_scale(timeScale, B, N1), _in(np.transpose(lam, (0, 2, 1))), tol)
    return _verdict(B, QUAD_VIOL_NAMES, lambda *out: ctx._check(_load().obca_quadcopter_constr_satisfaction_batch(ctx._h, B, N, *ins, *out),
                                                                "obca_quadcopter_constr_satisfaction_batch"))


def quadcopter_clearance_batch(x, timeScale, Ts, ob, R, substeps=8, need=0.0, device=0):
    """QuadBatch.clearance for arbitrary trajectories (obca_quadcopter_clearance_batch): x (B,12,N+1), timeScale scalar, (B,), (B,N+1) or None (= 1), ob (5,6) shared or
    (B,5,6) -- the arguments of quadcopter_constr_satisfaction_batch, in its order, that the check reads."""
    x = np.asarray(x, float); B, _, N1 = x.shape
    if x.shape != (B, 12, N1):
        raise ObcaError(f"x must be (B,12,N+1); got {x.shape}")
    ctx = _ctx(device)
    ins = (_per_instance(Ts, B), R, _boxes(ob, B), _in(np.transpose(x, (0, 2, 1))), _time_scale(1.0 if timeScale is None else timeScale, B, N1), int(substeps), float(need))
    return _clearance(B, substeps, 5, lambda out: ctx._check(_load().obca_quadcopter_clearance_batch(ctx._h, B, N1 - 1, *ins, out), "obca_quadcopter_clearance_batch"))


def quadcopter_predict_batch(x, timeScale, Ts, ob, R, rates=None, grow=None, substeps=8, need=0.0, device=0, profile=False):
    """QuadBatch.predict_clearance for arbitrary trajectories (obca_quadcopter_predict_batch): the arguments of quadcopter_clearance_batch up to R, then those of
    QuadBatch.predict_clearance.  Returns its dict, with `profile` (B, N substeps + 1) if asked for."""
    x = np.asarray(x, float); B, _, N1 = x.shape
    if x.shape != (B, 12, N1):
        raise ObcaError(f"x must be (B,12,N+1); got {x.shape}")
    ctx = _ctx(device)
    ins = (_per_instance(Ts, B), R, _boxes(ob, B), _in(np.transpose(x, (0, 2, 1))), _time_scale(1.0 if timeScale is None else timeScale, B, N1), int(substeps), float(need))
    rt = _quad_rates(B, rates, grow).reshape(-1); pr = np.zeros((B, (N1 - 1) * max(int(substeps), 0) + 1)) if profile else None
    r = _predict(B, substeps, 5, lambda out: ctx._check(_load().obca_quadcopter_predict_batch(ctx._h, B, N1 - 1, *ins, out, rt, None if pr is None else pr.reshape(-1)),
                                                        "obca_quadcopter_predict_batch"))
    return dict(r, profile=pr) if profile else r


def quadcopter_certify_batch(x, timeScale, Ts, ob, R, need=0.0, slack=0.01, max_steps=CERT_TICKS, device=0, intervals=True):
    """QuadBatch.certify for arbitrary trajectories (obca_quadcopter_certify_batch): the arguments of quadcopter_clearance_batch up to R, then those of QuadBatch.certify.
    Returns the dict of QuadBatch.certify, with `intervals` (B, N+1, 2) unless switched off."""
    x = np.asarray(x, float); B, _, N1 = x.shape
    if x.shape != (B, 12, N1):
        raise ObcaError(f"x must be (B,12,N+1); got {x.shape}")
    ctx = _ctx(device)
    ins = (_per_instance(Ts, B), R, _boxes(ob, B), _in(np.transpose(x, (0, 2, 1))), _time_scale(1.0 if timeScale is None else timeScale, B, N1), float(need), float(slack), int(max_steps))
    iv = np.zeros((B, N1, 2)) if intervals else None
    r = _certify(B, lambda out: ctx._check(_load().obca_quadcopter_certify_batch(ctx._h, B, N1 - 1, *ins, out, iv), "obca_quadcopter_certify_batch"))
    return dict(r, intervals=iv) if intervals else r


def quadcopter_rollout_batch(x, u, timeScale, Ts, ob, R, substeps=8, restart=False, need=0.0, device=0, states=True):
    """QuadBatch.rollout for arbitrary trajectories (obca_quadcopter_rollout_batch): x (B,12,N+1), u (B,4,N), timeScale scalar, (B,), (B,N+1) or None (= 1), ob (5,6)
    shared or (B,5,6).  Returns the dict of QuadBatch.rollout, with `states` (B, N+1, 12) unless states=False."""
    x = np.asarray(x, float); u = np.asarray(u, float); B, _, N1 = x.shape
    if x.shape != (B, 12, N1) or u.shape != (B, 4, N1 - 1):
        raise ObcaError(f"x must be (B,12,N+1) and u (B,4,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    ins = (_per_instance(Ts, B), R, _boxes(ob, B), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))), _time_scale(1.0 if timeScale is None else timeScale, B, N1),
           int(substeps), int(restart), float(need))
    X = np.zeros((B, N1, 12)) if states else None
    r = _rollout(B, substeps, 5, lambda out: ctx._check(_load().obca_quadcopter_rollout_batch(ctx._h, B, N1 - 1, *ins, out, X), "obca_quadcopter_rollout_batch"))
    return dict(r, **({"states": X} if states else {}))


def quadcopter_track_batch(x, u, timeScale, Ts, ob, R, substeps=8, dx0=None, Q=None, R_=None, Qf=None, feedback=True, clamp=True, need=0.0, device=0, states=True, gains=True):
    """QuadBatch.track for arbitrary trajectories (obca_quadcopter_track_batch): the arguments of quadcopter_rollout_batch (R: the vehicle's radius), then those of
    QuadBatch.track with the input weights as R_.  Returns the dict of QuadBatch.track, with `states` (B, N+1, 12) and `gains` (B, N, 4, 12) unless switched off."""
    x = np.asarray(x, float); u = np.asarray(u, float); B, _, N1 = x.shape
    if x.shape != (B, 12, N1) or u.shape != (B, 4, N1 - 1):
        raise ObcaError(f"x must be (B,12,N+1) and u (B,4,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    q, r, qf = _track_weights(12, 4, Q, R_, Qf, (TRACK_Q_QUAD, TRACK_R_QUAD, TRACK_QF_QUAD))
    ins = (_per_instance(Ts, B), R, _boxes(ob, B), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))), _time_scale(1.0 if timeScale is None else timeScale, B, N1),
           int(substeps), int(feedback), int(clamp), q, r, qf, _track_dx0(dx0, B, 12), float(need))
    X = np.zeros((B, N1, 12)) if states else None; K = np.zeros((B, N1 - 1, 4, 12)) if gains else None
    t = _track(B, substeps, 5, lambda out: ctx._check(_load().obca_quadcopter_track_batch(ctx._h, B, N1 - 1, *ins, out, X, K), "obca_quadcopter_track_batch"))
    return dict(t, **({"states": X} if states else {}), **({"gains": K} if gains else {}))


def quadcopter_ensemble_batch(x, u, timeScale, Ts, ob, R, members=64, substeps=8, dx0=None, dub=None, Q=None, R_=None, Qf=None, feedback=True, clamp=True, need=0.0, device=0,
                              member_records=True, final=True):
    """QuadBatch.ensemble for arbitrary trajectories (obca_quadcopter_ensemble_batch): the arguments of quadcopter_track_batch up to timeScale (R: the vehicle's radius), then
    those of QuadBatch.ensemble with the input weights as R_.  Returns the dict of QuadBatch.ensemble, with `member_records` (B, M, 16) and `final` (B, M, 12) unless switched off."""
    x = np.asarray(x, float); u = np.asarray(u, float); B, _, N1 = x.shape; M = int(members)
    if x.shape != (B, 12, N1) or u.shape != (B, 4, N1 - 1):
        raise ObcaError(f"x must be (B,12,N+1) and u (B,4,N); got {x.shape}, {u.shape}")
    ctx = _ctx(device)
    q, r, qf = _track_weights(12, 4, Q, R_, Qf, (TRACK_Q_QUAD, TRACK_R_QUAD, TRACK_QF_QUAD))
    Mc = min(max(M, 1), ENS_MMAX)
    ins = (_per_instance(Ts, B), R, _boxes(ob, B), _in(np.transpose(x, (0, 2, 1))), _in(np.transpose(u, (0, 2, 1))), _time_scale(1.0 if timeScale is None else timeScale, B, N1),
           int(substeps), M, int(feedback), int(clamp), q, r, qf, _ensemble_rows(dx0, B, Mc, 12, "dx0"), _ensemble_rows(dub, B, Mc, 4, "dub"), float(need))
    return _ensemble_host(B, Mc, 12, lambda out, mem, fin: ctx._check(_load().obca_quadcopter_ensemble_batch(ctx._h, B, N1 - 1, *ins, out, mem, fin), "obca_quadcopter_ensemble_batch"),
                          member_records, final)


def constrSatisfaction(x, u, timeScale, x0, xF, Ts, lam, ob1, ob2, ob3, ob4, ob5, R, device=0):
    """Drop-in for constrSatisfaction.jl:25 (one instance): True / False at the reference's tolerance 1e-3."""
    ob = np.stack([np.ravel(o)[:6] for o in (ob1, ob2, ob3, ob4, ob5)])
    x = np.asarray(x, float)
    r = quadcopter_constr_satisfaction_batch(x[None], np.asarray(u, float)[None], np.reshape(np.broadcast_to(np.ravel(np.asarray(timeScale, float)), (x.shape[1],)), (1, -1)),
                                             x0, xF, Ts, np.asarray(lam, float)[None], ob, R, device=device)
    return bool(r["ok"][0])


_QUAD_STATUS = {0: "Optimal", 1: "UserLimit", 2: "Error"}


def _quadcopter_one(dist, x0, xF, N, Ts, R, obs, xWS, timeWS, opts, device, dual_ws):
    """one instance through the batched call, returned as the reference's 7-tuple"""
    ob = np.stack([np.ravel(o)[:6] for o in obs])
    opts = quadcopter_ipopt_opts() if opts is None else opts      # the drop-in runs the reference's IPOPT configuration; the batched calls default to the throughput options
    r = quadcopter_signed_dist_batch(np.reshape(x0, (1, 12)), np.reshape(xF, (1, 12)), N, Ts, R, ob, np.asarray(xWS, float)[None, :N + 1],
                                     timeWS, dual_ws, opts, device, dist=dist)
    return r["xp"][0], r["up"][0], r["timeScale"][0], int(r["exitflag"][0]), r["time"], r["lp"][0], _QUAD_STATUS[int(r["status"][0])]


def QuadcopterSignedDist(x0, xF, N, Ts, R, ob1, ob2, ob3, ob4, ob5, xWS, uWS, timeWS, opts=None, device=0, dual_ws=True):
    """Drop-in for QuadcopterSignedDist.jl:25 (one instance; xWS is (N+1,12) here, the reference's is 12 x (N+1) column-major,
    i.e. the same memory).  Returns (xp, up, timeScalep, exitflag, time, lp, status) like :298; uWS is ignored like :202."""
    return _quadcopter_one(False, x0, xF, N, Ts, R, (ob1, ob2, ob3, ob4, ob5), xWS, timeWS, opts, device, dual_ws)


def QuadcopterDist(x0, xF, N, Ts, R, ob1, ob2, ob3, ob4, ob5, xWS, uWS, timeWS, opts=None, device=0, dual_ws=True):
    """Drop-in for QuadcopterDist.jl:25 (the collision-free sibling: no slack variable): same arguments and 7-tuple as QuadcopterSignedDist."""
    return _quadcopter_one(True, x0, xF, N, Ts, R, (ob1, ob2, ob3, ob4, ob5), xWS, timeWS, opts, device, dual_ws)
