"""The host layer around the kernels, where the rest of the GPU suite does not pin it (run with -m gpu): the texts of the lifecycle errors both batch families
raise, and the cached batch of a context's worker lane when calls of other shapes replace it -- every result bit for bit what a fresh device-resident batch gives,
for the solves and for the validate entry points that then run on the replaced batch; the timers of the staged calls before their first call; the staging of a
context's refine, subdivide and path-warm-start calls when it grows and is used again, a refine destination used twice, and the planner's memory under both of its entry
points -- each against the same call on a fresh context, bit for bit.  Every shape is tiny."""
import re
import numpy as np
import pytest
import hybrid_common as H
import path_ws_common as K
import scenes_common as SC
from obca_amd import api, planner as PL, scenarios as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.Context(0).close()      # fails loudly if the HIP library / device is missing
    return obca_amd


@pytest.fixture()
def ctx(OA):
    c = OA.Context(0)                # a context of its own per test: its lanes start without a cached batch
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_bits(a, b, keys, what):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and _bits(x) == _bits(y), (what, k)


def _parking_args(bt, N):
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    return (bt["x0"], bt["xF"]), (bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])


def test_lifecycle_errors_keep_their_texts(OA, ctx):
    """the expected texts are those of obca_batch_solve / quad_solve / obca_[quad_]batch_validate_ms in the C ABI's source before the two families shared a core"""
    B = 2
    pb = OA.Batch(ctx, B, 4); qb = OA.QuadBatch(ctx, B, 4)
    with pytest.raises(OA.ObcaError, match=re.escape("obca_batch_solve: nothing uploaded")):
        pb.solve()
    with pytest.raises(OA.ObcaError, match=re.escape("obca_quad_batch_solve: nothing uploaded")):
        qb.solve()
    with pytest.raises(OA.ObcaError, match=re.escape("obca_batch_validate_ms: no validate call has run on this batch")):
        pb.validate_ms()
    with pytest.raises(OA.ObcaError, match=re.escape("obca_quad_batch_validate_ms: no validate call has run on this batch")):
        qb.validate_ms()
    q = S.make_quad_batch(B, 4)
    qb.upload(q["x0"], q["xF"], q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"])
    o = OA.quadcopter_default_opts(); o.recalc_y = 1
    with pytest.raises(OA.ObcaError, match=re.escape("quadcopter solve: recalc_y is a switch of the parking kernels only")):
        qb.solve(opts=o)
    with pytest.raises(OA.ObcaError, match=re.escape("obca_quad_batch_validate_ms: no validate call has run on this batch")):      # (an upload is no validate)
        qb.validate_ms()
    (x0, xF), rest = _parking_args(S.make_batch(S.BACKWARDS, B, 4, seed=5), 4)
    pb.upload(x0, xF, *rest)
    with pytest.raises(OA.ObcaError, match=re.escape("obca_batch_validate_ms: no validate call has run on this batch")):
        pb.validate_ms()
    pb.close(); qb.close()


PARK_KEYS = ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info")
QUAD_KEYS = ("xp", "up", "timeScale", "exitflag", "lp", "slack", "info")


def test_parking_slot_batch_replacement_is_bit_neutral(OA, ctx):
    """(B, N) = (3, 8), (5, 10), (3, 8) through the host-pointer entry of ONE context: its lane's cached batch is created, replaced by a larger one of another horizon,
    replaced again; every result equals a fresh resident Batch's, and the host-pointer validate on the batch replaced last equals that Batch's resident validate()"""
    fresh = OA.Context(0)
    outs = []
    for B, N in ((3, 8), (5, 10), (3, 8)):
        bt = S.make_batch(S.BACKWARDS, B, N, seed=11)
        (x0, xF), rest = _parking_args(bt, N)
        out = OA.parking_signed_dist_batch(x0, xF, N, *rest, device=ctx)
        b = OA.Batch(fresh, B, N)
        b.upload(x0, xF, *rest); b.solve()
        ref = b.download(); val = b.validate(); b.close()
        _same_bits(out, ref, PARK_KEYS, "parking host-pointer call against a resident batch, B=%d N=%d" % (B, N))
        outs.append(out)
    _same_bits(outs[0], outs[2], PARK_KEYS, "first against third parking call")
    assert np.isfinite(out["xp"]).all() and (out["iters"] > 0).all()
    host = OA.parking_constraints_batch(x0, xF, N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], out["xp"], out["up"], out["timeScale"],
                                        out["lp"], out["np"], out["sl"], device=ctx)
    _same_bits(host, val, ("ok", "ref_ok", "viol"), "parking_constraints_batch against Batch.validate")
    fresh.close()


def test_quadcopter_slot_batch_replacement_is_bit_neutral(OA, ctx):
    """the same walk for the quadcopter family: (B, N) = (2, 8), (3, 10), (2, 8)"""
    fresh = OA.Context(0)
    outs = []
    for B, N in ((2, 8), (3, 10), (2, 8)):
        q = S.make_quad_batch(B, N)
        out = OA.quadcopter_signed_dist_batch(q["x0"], q["xF"], N, q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"], device=ctx)
        b = OA.QuadBatch(fresh, B, N)
        b.upload(q["x0"], q["xF"], q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"]); b.solve()
        ref = b.download(); val = b.validate(); b.close()
        _same_bits(out, ref, QUAD_KEYS, "quadcopter host-pointer call against a resident batch, B=%d N=%d" % (B, N))
        outs.append(out)
    _same_bits(outs[0], outs[2], QUAD_KEYS, "first against third quadcopter call")
    assert np.isfinite(out["xp"]).all() and (out["iters"] > 0).all()
    host = OA.quadcopter_constr_satisfaction_batch(out["xp"], out["up"], out["timeScale"], q["x0"], q["xF"], q["Ts"], out["lp"], q["ob"], q["R"], device=ctx)
    _same_bits(host, val, ("ok", "viol"), "quadcopter_constr_satisfaction_batch against QuadBatch.validate")
    fresh.close()


def test_timers_refuse_before_their_first_call(OA, ctx):
    """the texts are those of obca_batch_path_ws_ms, obca_batch_refine_ms, obca_quad_batch_subdivide_ms, obca_hybrid_ms and obca_scene_astar_ms in the C ABI's source before
    the event pairs became one type"""
    pb = OA.Batch(ctx, 2, 4); qb = OA.QuadBatch(ctx, 2, 4)
    for call, text in ((pb.path_ws_ms, "obca_batch_path_ws_ms: no path warm start has run on this batch"),
                       (pb.refine_ms, "obca_batch_refine_ms: no refine call has written into this batch"),
                       (qb.refine_ms, "obca_quad_batch_subdivide_ms: no subdivide call has written into this batch"),
                       (lambda: api.hybrid_ms(device=ctx), "obca_hybrid_ms: no search has run on this context"),
                       (lambda: api.scene_ms(device=ctx), "obca_scene_astar_ms: no per-instance search has run on this context")):
        with pytest.raises(OA.ObcaError, match=re.escape(text)):
            call()
    pb.close(); qb.close()


def _short_paths(B, seed, cap=12):
    """B planner-like paths of 4, 5, ... nodes (every other one with a direction switch) in the planner's dense arrays; rows beyond a count hold NaN / 9"""
    rng = np.random.default_rng(seed)
    paths = np.full((B, cap, 3), np.nan); dirs = np.full((B, cap), 9, np.int32); cnt = np.zeros(B, np.int32); xF = np.zeros((B, 4))
    for i in range(B):
        P, D = K.make_path(rng, 4 + i, switch_at=(2,) if i % 2 else ())
        cnt[i] = len(P); paths[i, :len(P)] = P; dirs[i, :len(P)] = D; xF[i, :3] = P[-1]
    return paths, dirs, cnt, xF


def _staged_calls(B, N, device):
    """the three host-pointer calls that stage through a block of the context, on arrays that (B, N) determines: dict of their outputs"""
    rng = np.random.default_rng(100 * B + N)
    x = rng.normal(size=(B, 4, N + 1)); u = rng.normal(size=(B, 2, N)); ts = rng.uniform(0.5, 1.5, (B, N + 1)); xq = rng.normal(size=(B, 12, N + 1))
    pr = api.parking_refine_batch(N, 0.3, S.L_WHEELBASE, x, u, ts, factor=2, device=device)
    qr = api.quadcopter_refine_batch(xq, ts, 0.25, factor=2, device=device)
    paths, dirs, cnt, xF = _short_paths(B, 100 * B + N)
    Ts, xWS, uWS, ok = PL.path_to_warm_start_many(paths, dirs, cnt, N, xF, device=device)
    assert ok.all()
    return dict(pr_Ts=pr["Ts"], pr_x=pr["x"], pr_u=pr["u"], qr_Ts=qr["Ts"], qr_x=qr["x"], ws_Ts=Ts, ws_x=xWS, ws_u=uWS)


def test_staging_that_grows_and_is_reused_changes_no_bit(OA, ctx):
    """(B, N) = (2, 4), (5, 6), (2, 4) through parking_refine_batch, quadcopter_refine_batch and path_to_warm_start_many of ONE context: each staging block is created, replaced
    by a larger one and used again below its size; every result equals that of a context that has run nothing else"""
    outs = []
    for B, N in ((2, 4), (5, 6), (2, 4)):
        out = _staged_calls(B, N, ctx)
        fresh = OA.Context(0)
        ref = _staged_calls(B, N, fresh)
        fresh.close()
        _same_bits(out, ref, tuple(ref), "staged calls against a fresh context, B=%d N=%d" % (B, N))
        assert all(np.isfinite(v).all() for v in out.values())
        outs.append(out)
    _same_bits(outs[0], outs[2], tuple(outs[0]), "first against third staged calls")


def _refine_twice(src, make_dst, keys):
    """n = 3, then n = 2 (a permutation with a gap) out of the solved `src` into ONE destination, each time against a destination of its own: status, and the download after a
    solve -- what the destination's records determine"""
    dst = make_dst()
    for sel in ((0, 1, 2), (2, 0)):
        d, st = src.refine(2, select=list(sel), into=dst)
        assert d is dst and d.B == len(sel) and dst.refine_ms() > 0
        dst.solve(); got = dst.download()
        own = make_dst()
        _, st_own = src.refine(2, select=list(sel), into=own)
        own.solve(); ref = own.download(); own.close()
        assert _bits(st) == _bits(st_own), sel
        _same_bits(got, ref, keys, "reused refine destination, selection %s" % (sel,))
    dst.close()


def test_refine_destinations_are_reused(OA, ctx):
    """Batch.refine(into=) and QuadBatch.refine(into=) twice into one destination, B = 3, N = 4 -> 8"""
    B, N = 3, 4
    (x0, xF), rest = _parking_args(S.make_batch(S.BACKWARDS, B, N, seed=5), N)
    pb = OA.Batch(ctx, B, N); pb.upload(x0, xF, *rest); pb.solve()
    _refine_twice(pb, lambda: OA.Batch(ctx, B, 2 * N), PARK_KEYS)
    pb.close()
    q = S.make_quad_batch(B, N)
    qb = OA.QuadBatch(ctx, B, N); qb.upload(q["x0"], q["xF"], q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"]); qb.solve()
    _refine_twice(qb, lambda: OA.QuadBatch(ctx, B, 2 * N), QUAD_KEYS)
    qb.close()


def test_planner_memory_is_shared_by_both_entry_points(OA, ctx):
    """ONE context, analytic expansion off: a shared-field call (B = 2, 1 slot), a per-instance call (B = 3, 2 slots: the slots grow), a smaller node pool and a shared-field
    call (the slots are reallocated), a per-instance call with twice the path capacity (the staging block grows).  All five arrays of every call equal the same call on a
    fresh context; the shared-field timer keeps its value across the per-instance calls"""
    sc, x0, xF, kw = H.poses("backwards", 33)
    o = H.opts_array(dict(kw, analytic=0.0))
    v, A, b = SC.shared_field()
    fields = SC.lists(SC.scenes()[3][:3])

    def shared(c, cap=H.CAP):
        return api.hybrid_astar_batch(x0[:2], xF[:2], v, A, b, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, o, None, cap, device=c)

    def own(c, cap=H.CAP):
        return api.scene_astar_batch(x0[:3], xF[:3], *fields, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, o, None, cap, device=c)

    steps = ((dict(slots=1, max_nodes=H.NODES), shared, H.CAP), (dict(slots=2, max_nodes=H.NODES), own, H.CAP), (dict(max_nodes=6000), shared, H.CAP), (dict(max_nodes=6000), own, 2 * H.CAP))
    t_shared = None
    for i, (conf, call, cap) in enumerate(steps):
        api.hybrid_configure(device=ctx, **conf)
        got = call(ctx, cap)
        fresh = OA.Context(0)
        api.hybrid_configure(device=fresh, **conf)
        ref = call(fresh, cap)
        fresh.close()
        _same_bits(dict(zip(H.FIELDS, got)), dict(zip(H.FIELDS, ref)), H.FIELDS, "planner call %d against a fresh context" % i)
        if call is shared:
            t_shared = api.hybrid_ms(device=ctx)
            assert t_shared > 0
        else:      # (the runtime converts the same pair of event timestamps anew at every query: "the same" is within a microsecond, as in tests/test_gpu_scenes.py)
            assert api.scene_ms(device=ctx) > 0 and abs(api.hybrid_ms(device=ctx) - t_shared) <= 1e-3
        if i == 1:      # (with the large pool every scene has a path: tests/test_gpu_scenes.py)
            assert (got[2] >= 2).all()
