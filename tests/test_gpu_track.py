"""Closed-loop rollout on the device (include/obca_track.h) against the host build of the same kernel text (tests/emu/track_emu.cpp): the host-pointer entry points on the
fixture's solved trajectories and on synthetic ones at the horizons where the kernel takes another path; equality with the merged rollout where nothing is fed back; the
resident calls after a solve; the fixture tiled over several chunks; a foreign pattern in LDS; the refusals.  Trajectories: tests/rollout_common.py; comparison rules and
tolerances: tests/track_common.py.  The largest differences seen are printed (tools/track_rate.py copies them into its profile)."""
import json
import os
import numpy as np
import pytest
import rollout_common as R
import track_common as T
from obca_amd import scenarios as S, validate as V
from test_gpu_rollout import record as rollout_record, flat, upload_parking

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.build_library()
    return obca_amd


def record(r, i):
    """row i of a returned dict, back in the layout of the C record"""
    out = np.zeros(V.TRK_OUT); out[:40] = rollout_record(r, i); out[10] = 0.0
    out[40], out[41], out[42], out[43], out[44], out[45] = r["feedback"][i], r["clamp"][i], r["saturated"][i], r["du_max"][i], r["du_node"][i], r["dx0_pos"][i]
    return out


def quad_call(OA, cases, S_, fb=True, cl=True, dx0=None, need=0.0, **kw):
    return OA.quadcopter_track_batch(np.stack([c["x"] for c in cases]), np.stack([c["u"] for c in cases]), np.stack([c["ts"] for c in cases]), [c["Ts"] for c in cases],
                                     cases[0]["ob"], cases[0]["R"], S_, dx0, feedback=fb, clamp=cl, need=need, **kw)


def parking_call(OA, cases, S_, fb=True, cl=True, dx0=None, need=V.DMIN, **kw):
    c0 = cases[0]
    return OA.parking_track_batch(c0["N"], [c["Ts"] for c in cases], c0["L"], c0["ego"], [c["vOb"] for c in cases], [c["A"] for c in cases], [c["b"] for c in cases],
                                  np.stack([c["x"] for c in cases]), np.stack([c["u"] for c in cases]), np.stack([c["ts"] for c in cases]), S_, dx0, feedback=fb, clamp=cl, need=need, **kw)


def against_host_build(r, hosts, key, what):
    """every instance of a device result against the host build's (record, X, poses, K, AB) of the same trajectory: 1e-9 max(1, |value|) on record, states and gains (gains
    relative to the instance's largest); flags and sizes equal; an index or a count may move only where the values it separates agree within the bound"""
    for i, h in enumerate(hosts):
        dev = record(r, i); X = r["states"][i].T; K = r["gains"][i]
        WORST[key] = max(WORST.get(key, 0.0), R.worst(dev[T.REAL], h[0][T.REAL]), R.worst(X, h[1]), T.gain_gap(K, h[3]))
        T.check((dev, X, None, K), (h[0], h[1], None, h[3]), T.TOL_DEV, "%s instance %d" % (what, i), exact_idx=False)
        if not np.array_equal(dev[T.EXACT], h[0][T.EXACT]):
            assert abs(dev[20] - h[0][20]) <= 1 and abs(dev[42] - h[0][42]) <= 1 and R.close(dev[[1, 16, 43]], h[0][[1, 16, 43]], T.TOL_DEV), (what, i, dev[T.EXACT], h[0][T.EXACT])


# ---------------------------------------------------------------- 1. host-pointer entries against the host build
@pytest.mark.parametrize("fb", [1, 0])
@pytest.mark.parametrize("S_", [1, 8])
@pytest.mark.parametrize("N", [2, 20, 65, 128])
def test_quadcopter_host_pointer_call_matches_the_host_build(OA, N, S_, fb):
    cases = R.quad_cases(N)[:2]; dx0 = T.DX0_QUAD * (1.0 if N == 20 else 0.1)
    r = quad_call(OA, cases, S_, fb, True, dx0)
    assert r["states"].shape == (2, N + 1, 12) and r["gains"].shape == (2, N, 4, 12) and r["finite"].all() and (r["substeps"] == S_).all() and (r["feedback"] == bool(fb)).all()
    against_host_build(r, [T.emu_quad(c, S_, fb, 1, dx0) for c in cases], "quad_device_vs_host_build", "quad N=%d S=%d feedback=%d" % (N, S_, fb))
    print("largest quadcopter difference device - host build so far: %.3g" % WORST["quad_device_vs_host_build"])


@pytest.mark.parametrize("fb", [1, 0])
@pytest.mark.parametrize("S_", [1, 8])
@pytest.mark.parametrize("N", [1, 30, 65, 128])
def test_parking_host_pointer_call_matches_the_host_build(OA, N, S_, fb):
    cases = R.parking_cases(N)[:2]
    r = parking_call(OA, cases, S_, fb, True, T.DX0_PARK)
    assert r["states"].shape == (2, N + 1, 4) and r["gains"].shape == (2, N, 2, 4) and r["finite"].all() and (r["clearance"]["samples"] == N * S_ + 1).all()
    against_host_build(r, [T.emu_parking(c, S_, fb, 1, T.DX0_PARK) for c in cases], "parking_device_vs_host_build", "parking N=%d S=%d feedback=%d" % (N, S_, fb))
    print("largest parking difference device - host build so far: %.3g" % WORST["parking_device_vs_host_build"])


# ---------------------------------------------------------------- 2. equality with the merged rollout
@pytest.mark.parametrize("S_", [1, 8])
def test_without_feedback_clamp_and_offset_it_is_the_chain_rollout_on_the_device(OA, S_):
    q = R.golden_quad(); t = quad_call(OA, q, S_, False, False, None)
    r = OA.quadcopter_rollout_batch(np.stack([c["x"] for c in q]), np.stack([c["u"] for c in q]), np.stack([c["ts"] for c in q]), [c["Ts"] for c in q], q[0]["ob"], q[0]["R"], S_, False, 0.0)
    for i in range(4):
        assert np.array_equal(record(t, i)[:40], rollout_record(r, i)) and record(t, i)[40:].tolist() == [0] * 8
    assert np.array_equal(t["states"], r["states"])
    p = R.golden_parking(); c0 = p[0]; t = parking_call(OA, p, S_, False, False, None)
    r = OA.parking_rollout_batch(c0["N"], [c["Ts"] for c in p], c0["L"], c0["ego"], [c["vOb"] for c in p], [c["A"] for c in p], [c["b"] for c in p],
                                 np.stack([c["x"] for c in p]), np.stack([c["u"] for c in p]), np.stack([c["ts"] for c in p]), S_, False, V.DMIN)
    for i in range(3):
        assert np.array_equal(record(t, i)[:40], rollout_record(r, i))
    assert np.array_equal(t["states"], r["states"])


# ---------------------------------------------------------------- 3. resident
def tflat(r):
    return {k: np.asarray(v, float) for k, v in flat(r).items()}


def resident_checks(OA, b, ctx, host_call, keys, N, nx, nu, dx0):
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.track(8)
    with pytest.raises(OA.ObcaError, match="no track call has run"):
        b.track_states()
    with pytest.raises(OA.ObcaError, match="no track call has run"):
        b.track_gains()
    b.solve(); before = b.download()
    assert (before["exitflag"] == 1).any()
    b.rollout(8, False); Xr = b.rollout_states()
    out = {}
    for d in (None, dx0):
        r = tflat(b.track(8, d)); X = b.track_states(); K = b.track_gains()
        assert b.track_ms() > 0 and X.shape == (b.B, N + 1, nx) and K.shape == (b.B, N, nu, nx)
        h = host_call(before, d); hs = h.pop("states"); hk = h.pop("gains"); h = tflat(h)
        for k in r:
            assert np.array_equal(r[k], h[k], equal_nan=True), (k, r[k], h[k])
        assert np.array_equal(X, hs, equal_nan=True) and np.array_equal(K, hk, equal_nan=True)
        out[d is not None] = (r, X, K)
    after = b.download()
    for k in keys:
        assert np.array_equal(before[k], after[k], equal_nan=True), k      # the iterate is read, nothing is written
    assert np.array_equal(b.rollout_states(), Xr, equal_nan=True)           # the rollout's node states have a buffer of their own
    # what another kernel left in LDS changes nothing
    from obca_amd import diag
    diag.leave_pattern(ctx, 4, 1e30)
    r2 = tflat(b.track(8, dx0)); X2 = b.track_states(); K2 = b.track_gains()
    assert all(np.array_equal(r2[k], out[True][0][k], equal_nan=True) for k in r2) and np.array_equal(X2, out[True][1], equal_nan=True) and np.array_equal(K2, out[True][2], equal_nan=True)
    for kw, msg in ((dict(substeps=0), "substeps"), (dict(substeps=33), "substeps"), (dict(need=np.nan), "finite `need`"), (dict(Q=-1.0), "q and qf need finite entries >= 0"),
                    (dict(Qf=np.nan), "q and qf need finite entries >= 0"), (dict(R=0.0), "r needs finite entries > 0")):
        with pytest.raises(OA.ObcaError, match=msg):
            b.track(**kw)
    return before, out


def test_resident_quadcopter_track(OA):
    B, N = 4, 20; bt = S.make_quad_batch(B, N); ctx = OA.Context(0)
    b = OA.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    before, out = resident_checks(OA, b, ctx, lambda o, d: OA.quadcopter_track_batch(o["xp"], o["up"], o["timeScale"], bt["Ts"], bt["ob"], bt["R"], 8, d),
                                  ("xp", "up", "timeScale", "exitflag", "lp", "slack", "info"), N, 12, 4, T.DX0_QUAD)
    ok = before["exitflag"] == 1
    r = out[False][0]; op = b.rollout(8, False)
    print("resident quadcopter, N = 20: dev_pos closed %s m, open %s m" % (np.round(r["dev_pos"], 3), np.round(op["dev_pos"], 3)))
    assert r["finite"][ok].all() and (r["dev_pos"][ok] < op["dev_pos"][ok]).all()
    b.close(); ctx.close()


def test_resident_parking_track(OA):
    B, N = 8, 30; bt = S.make_batch(S.BACKWARDS, B, N); ctx = OA.Context(0)
    b = upload_parking(OA, ctx, bt)
    before, out = resident_checks(OA, b, ctx, lambda o, d: OA.parking_track_batch(N, bt["Ts"], bt["L"], bt["ego"], bt["vOb"], bt["A"], bt["b"], o["xp"], o["up"], o["timeScale"], 8, d),
                                  ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info"), N, 4, 2, T.DX0_PARK)
    ok = before["exitflag"] == 1
    r = out[False][0]; op = b.rollout(8, False)
    print("resident parking, N = 30: end_pos closed %s m, open %s m" % (np.round(r["end_pos"], 5), np.round(op["end_pos"], 5)))
    assert r["finite"][ok].all() and (r["end_pos"][ok] < op["end_pos"][ok]).all()
    b.close(); ctx.close()


# ---------------------------------------------------------------- 4. tiling
def test_fixture_tiled_over_several_chunks(OA, monkeypatch):
    """260 instances in chunks of 100: every instance lands in its own rows of out, X and K, whichever chunk and slot ran it; a NaN marks its instance alone"""
    monkeypatch.setenv("OBCA_CHUNK", "100")
    q = R.golden_quad(); tiled = [q[i % 4] for i in range(260)]; dx0 = np.stack([T.DX0_QUAD * (1 + i % 4) / 4 for i in range(260)])
    hosts = [T.emu_quad(c, 8, 1, 1, dx0[i]) for i, c in enumerate(q)]
    r = quad_call(OA, tiled, 8, True, True, dx0)
    against_host_build(r, [hosts[i % 4] for i in range(260)], "quad_device_vs_host_build", "quad tiled")
    for i in range(4, 260):      # the same trajectory gives the same bits wherever it runs
        assert np.array_equal(record(r, i), record(r, i % 4)) and np.array_equal(r["states"][i], r["states"][i % 4]) and np.array_equal(r["gains"][i], r["gains"][i % 4])
    bad = [dict(c) for c in tiled]; bad[137] = dict(bad[137], u=bad[137]["u"].copy()); bad[137]["u"][2, 7] = np.nan
    rb = quad_call(OA, bad, 8, True, True, dx0)
    assert (~rb["finite"]).nonzero()[0].tolist() == [137] and np.isnan(rb["states"][137]).all() and np.isnan(rb["gains"][137]).all() and np.isnan(rb["du_max"][137])
    assert rb["saturated"][137] == -1 and rb["du_node"][137] == -1 and rb["dev_node"][137] == -1
    assert all(np.array_equal(record(rb, i), record(r, i)) and np.array_equal(rb["states"][i], r["states"][i]) and np.array_equal(rb["gains"][i], r["gains"][i]) for i in range(260) if i != 137)
    p = R.golden_parking(); tiled = [p[i % 3] for i in range(260)]
    hosts = [T.emu_parking(c, 8, 1, 1, T.DX0_PARK) for c in p]
    r = parking_call(OA, tiled, 8, True, True, T.DX0_PARK)
    against_host_build(r, [hosts[i % 3] for i in range(260)], "parking_device_vs_host_build", "parking tiled")
    for i in range(3, 260):
        assert np.array_equal(record(r, i), record(r, i % 3)) and np.array_equal(r["states"][i], r["states"][i % 3]) and np.array_equal(r["gains"][i], r["gains"][i % 3])


def test_bad_instances_and_the_refusals_of_the_host_pointer_calls(OA):
    q = R.golden_quad(); dx0 = np.tile(T.DX0_QUAD, (3, 1)); dx0[1, 4] = np.nan
    r = quad_call(OA, q[:3], 8, True, True, dx0); good = quad_call(OA, q[:3], 8, True, True, np.tile(T.DX0_QUAD, (3, 1)))
    assert r["finite"].tolist() == [True, False, True] and np.isnan(r["states"][1]).all() and np.isnan(r["gains"][1]).all()
    for i in (0, 2):
        assert np.array_equal(record(r, i), record(good, i)) and np.array_equal(r["states"][i], good["states"][i]) and np.array_equal(r["gains"][i], good["gains"][i])
    assert np.array_equal(record(r, 1), T.emu_quad(q[1], 8, 1, 1, dx0[1])[0], equal_nan=True)
    for kw, msg in ((dict(S_=0), "substeps"), (dict(need=np.inf), "finite `need`"), (dict(fb=2), "feedback must be 0"), (dict(cl=-1), "clamp must be 0 or 1")):
        with pytest.raises(OA.ObcaError, match=msg):
            quad_call(OA, q, **{"S_": 8, **kw})
        with pytest.raises(OA.ObcaError, match=msg):
            parking_call(OA, R.golden_parking(), **{"S_": 8, **kw})
    with pytest.raises(OA.ObcaError, match="r needs finite entries > 0"):
        quad_call(OA, q, 8, R_=[0.1, 0.1, -0.1, 0.1])
    t = quad_call(OA, q, 8, states=False, gains=False)
    assert "states" not in t and "gains" not in t


def test_largest_differences_are_on_record():
    """the figures tools/track_rate.py copies into profiles/track_device_vs_host.json (OBCA_TRACK_DIFFS names the file they are left in)"""
    print("device against host build:", WORST)
    path = os.environ.get("OBCA_TRACK_DIFFS")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f)
