"""Rollout on the continuous vehicle models on the device (include/obca_rollout.h) against the host build of the same kernel text (tests/emu/rollout_emu.cpp): the
host-pointer entry points on the fixture's solved trajectories, on synthetic ones at the horizons where the kernel takes another path, and on the fixture tiled over
several chunks; the resident calls after a solve; a foreign pattern in LDS; the refusals.  Trajectories, comparison rules and tolerances: tests/rollout_common.py.
The largest differences seen are printed (tools/rollout_rate.py copies them into its profile)."""
import json
import os
import numpy as np
import pytest
import rollout_common as R
from obca_amd import scenarios as S, validate as V

pytestmark = pytest.mark.gpu
WORST = {}
KEYS = ("dev_pos", "dev_att", "dev_vel", "dev_rate", "end_pos", "end_att", "end_vel", "end_rate")


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.build_library()
    return obca_amd


def record(r, i):
    """row i of a returned dict, back in the layout of the C record"""
    out = np.zeros(V.ROLL_OUT); c = r["clearance"]; out[24:] = np.inf
    out[0] = 0.0 if r["finite"][i] else 1.0; out[2] = r["dev_node"][i]; out[10] = r["restart"][i]; out[11] = r["substeps"][i]
    out[[1, 3, 4, 5, 6, 7, 8, 9]] = [r[k][i] for k in KEYS]
    out[16], out[17], out[18], out[19], out[20], out[21], out[22] = c["min"][i], c["min_nodes"][i], c["sample"][i], c["obstacle"][i], c["below"][i], c["samples"][i], 0.0 if c["finite"][i] else 1.0
    po = c["per_obstacle"][i]; out[24:24 + len(po)] = po
    if out[22]:
        out[24:] = np.nan      # (a record that is not finite has no +inf behind the instance's obstacles)
    return out


def quad_call(OA, cases, S_, restart, need=0.0, device=0):
    return OA.quadcopter_rollout_batch(np.stack([c["x"] for c in cases]), np.stack([c["u"] for c in cases]), np.stack([c["ts"] for c in cases]), [c["Ts"] for c in cases],
                                       cases[0]["ob"], cases[0]["R"], S_, restart, need, device=device)


def parking_call(OA, cases, S_, restart, need=V.DMIN, device=0):
    c0 = cases[0]
    return OA.parking_rollout_batch(c0["N"], [c["Ts"] for c in cases], c0["L"], c0["ego"], [c["vOb"] for c in cases], [c["A"] for c in cases], [c["b"] for c in cases],
                                    np.stack([c["x"] for c in cases]), np.stack([c["u"] for c in cases]), np.stack([c["ts"] for c in cases]), S_, restart, need, device=device)


def against_host_build(r, hosts, key, what):
    """every instance of a device result against the host build's (record, X) of the same trajectory: 1e-9 max(1, |value|); flags, sizes and counts of samples equal"""
    for i, (hrec, hX) in enumerate(hosts):
        dev = record(r, i)
        WORST[key] = max(WORST.get(key, 0.0), R.worst(dev[R.REAL], hrec[R.REAL]), R.worst(r["states"][i].T, hX))
        R.check_record(dev, hrec, R.TOL_DEV, "%s instance %d" % (what, i), exact_idx=False)
        assert R.close(r["states"][i].T, hX, R.TOL_DEV), (what, i)
        if not np.array_equal(dev[R.EXACT], hrec[R.EXACT]):      # an index or a count may move only where the values it separates agree within the bound
            assert abs(dev[20] - hrec[20]) <= 1 and R.close(dev[[1, 16]], hrec[[1, 16]], R.TOL_DEV), (what, i, dev[R.EXACT], hrec[R.EXACT])


# ---------------------------------------------------------------- 1. host-pointer entries against the host build
@pytest.mark.parametrize("restart", R.MODES)
@pytest.mark.parametrize("S_", [1, 8])
@pytest.mark.parametrize("N", [20, 65, 128])
def test_quadcopter_host_pointer_call_matches_the_host_build(OA, N, S_, restart):
    cases = R.quad_cases(N)
    r = quad_call(OA, cases, S_, restart)
    assert r["states"].shape == (len(cases), N + 1, 12) and r["finite"].all() and (r["substeps"] == S_).all() and (r["restart"] == bool(restart)).all()
    against_host_build(r, [R.emu_quad(c, S_, restart)[:2] for c in cases], "quad_device_vs_host_build", "quad N=%d S=%d restart=%d" % (N, S_, restart))
    print("largest quadcopter difference device - host build so far: %.3g" % WORST["quad_device_vs_host_build"])


@pytest.mark.parametrize("restart", R.MODES)
@pytest.mark.parametrize("S_", [1, 8])
@pytest.mark.parametrize("N", [30, 65, 128])
def test_parking_host_pointer_call_matches_the_host_build(OA, N, S_, restart):
    cases = R.parking_cases(N)
    r = parking_call(OA, cases, S_, restart)
    assert r["states"].shape == (len(cases), N + 1, 4) and r["finite"].all() and (r["clearance"]["samples"] == N * S_ + 1).all()
    against_host_build(r, [R.emu_parking(c, S_, restart)[:2] for c in cases], "parking_device_vs_host_build", "parking N=%d S=%d restart=%d" % (N, S_, restart))
    print("largest parking difference device - host build so far: %.3g" % WORST["parking_device_vs_host_build"])


@pytest.mark.parametrize("restart", R.MODES)
def test_fixture_tiled_over_several_chunks(OA, restart, monkeypatch):
    """260 instances in chunks of 100: every instance lands in its own row of `out` and of X, whichever chunk and slot ran it; a NaN marks its instance alone"""
    monkeypatch.setenv("OBCA_CHUNK", "100")
    q = R.golden_quad(); tiled = [q[i % 4] for i in range(260)]
    hosts = [R.emu_quad(c, 8, restart)[:2] for c in q]
    r = quad_call(OA, tiled, 8, restart)
    against_host_build(r, [hosts[i % 4] for i in range(260)], "quad_device_vs_host_build", "quad tiled restart=%d" % restart)
    for i in range(4, 260):      # the same trajectory gives the same bits wherever it runs
        assert np.array_equal(record(r, i), record(r, i % 4)) and np.array_equal(r["states"][i], r["states"][i % 4])
    bad = [dict(c) for c in tiled]; bad[137] = dict(bad[137], u=bad[137]["u"].copy()); bad[137]["u"][2, 7] = np.nan
    rb = quad_call(OA, bad, 8, restart)
    assert (~rb["finite"]).nonzero()[0].tolist() == [137] and np.isnan(rb["states"][137]).all() and np.isnan(rb["dev_pos"][137]) and rb["dev_node"][137] == -1
    assert not rb["clearance"]["finite"][137] and rb["clearance"]["sample"][137] == -1
    assert all(np.array_equal(record(rb, i), record(r, i)) and np.array_equal(rb["states"][i], r["states"][i]) for i in range(260) if i != 137)
    p = R.golden_parking(); tiled = [p[i % 3] for i in range(260)]
    hosts = [R.emu_parking(c, 8, restart)[:2] for c in p]
    r = parking_call(OA, tiled, 8, restart)
    against_host_build(r, [hosts[i % 3] for i in range(260)], "parking_device_vs_host_build", "parking tiled restart=%d" % restart)
    for i in range(3, 260):
        assert np.array_equal(record(r, i), record(r, i % 3)) and np.array_equal(r["states"][i], r["states"][i % 3])


def test_a_pitch_through_half_pi_and_the_refusals_of_the_host_pointer_calls(OA):
    q = R.golden_quad(); N = 20
    u = np.full((4, N), 4.48); u[1] += 1.0; u[3] -= 1.0
    cases = [q[0], dict(q[1], u=u), q[2]]
    r = quad_call(OA, cases, 8, 0); good = quad_call(OA, q[:3], 8, 0)
    assert r["finite"].tolist() == [True, False, True] and np.isnan(r["states"][1]).all() and np.isnan(r["end_pos"][1]) and r["clearance"]["below"][1] == 8 * N + 1
    for i in (0, 2):
        assert np.array_equal(record(r, i), record(good, i)) and np.array_equal(r["states"][i], good["states"][i])
    assert np.array_equal(record(r, 1), R.emu_quad(cases[1], 8, 0)[0], equal_nan=True)
    for S_, restart, need, msg in ((0, 0, 0.0, "substeps"), (33, 1, 0.0, "substeps"), (8, 2, 0.0, "restart must be 0"), (8, 0, np.nan, "finite `need`")):
        with pytest.raises(OA.ObcaError, match=msg):
            quad_call(OA, q, S_, restart, need)
        with pytest.raises(OA.ObcaError, match=msg):
            parking_call(OA, R.golden_parking(), S_, restart, V.DMIN if need == 0.0 else need)
    assert "states" not in OA.quadcopter_rollout_batch(np.stack([c["x"] for c in q]), np.stack([c["u"] for c in q]), q[0]["ts"][0], q[0]["Ts"], q[0]["ob"], q[0]["R"], states=False)


# ---------------------------------------------------------------- 2. resident
def upload_parking(OA, ctx, bt):
    B, N = len(bt["Ts"]), bt["N"]
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    return b


def flat(r):
    return {**{k: v for k, v in r.items() if k != "clearance"}, **{"clearance_" + k: v for k, v in r["clearance"].items()}}


def resident_checks(OA, b, ctx, host_call, keys, N, nx, key):
    """what both resident tests assert: refusals, both modes against the host-pointer call on download(), nothing written, the pattern, the states"""
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.rollout(8)
    with pytest.raises(OA.ObcaError, match="no rollout has run"):
        b.rollout_states()
    b.solve(); before = b.download()
    assert (before["exitflag"] == 1).any()
    out = {}
    for restart in (False, True):
        r = flat(b.rollout(8, restart)); X = b.rollout_states()
        assert b.rollout_ms() > 0 and X.shape == (b.B, N + 1, nx)
        h = host_call(before, restart); hs = h.pop("states"); h = flat(h)
        bits = True
        for k in r:
            a, c = np.asarray(r[k], float), np.asarray(h[k], float)
            assert R.close(a, c, 1e-12), (k, restart, a, c)
            bits = bits and np.array_equal(a, c, equal_nan=True)
        assert R.close(X, hs, 1e-12)
        WORST[key] = max(WORST.get(key, 0.0), R.worst(X, hs), *(R.worst(r[k], h[k]) for k in r))
        print("resident against host-pointer call, restart=%d: bit-equal %s, largest difference %.3g" % (restart, bits and np.array_equal(X, hs, equal_nan=True), WORST[key]))
        out[restart] = (r, X)
    after = b.download()
    for k in keys:
        assert np.array_equal(before[k], after[k], equal_nan=True), k      # the iterate is read, nothing is written
    # what another kernel left in LDS changes nothing
    from obca_amd import diag
    diag.leave_pattern(ctx, 4, 1e30)
    r2 = flat(b.rollout(8, True)); X2 = b.rollout_states()
    assert all(np.array_equal(np.asarray(r2[k], float), np.asarray(out[True][0][k], float), equal_nan=True) for k in r2) and np.array_equal(X2, out[True][1], equal_nan=True)
    for S_, restart, msg in ((0, 0, "substeps"), (33, 0, "substeps"), (8, 2, "restart must be 0")):
        with pytest.raises(OA.ObcaError, match=msg):
            b.rollout(S_, restart)
    b.solve(); again = b.download()
    for k in keys:
        assert np.array_equal(before[k], again[k], equal_nan=True), k      # a second solve is unchanged
    return before, out


def test_resident_quadcopter_rollout(OA):
    B, N = 4, 20; bt = S.make_quad_batch(B, N); ctx = OA.Context(0)
    b = OA.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    before, out = resident_checks(OA, b, ctx, lambda o, restart: OA.quadcopter_rollout_batch(o["xp"], o["up"], o["timeScale"], bt["Ts"], bt["ob"], bt["R"], 8, restart, 0.0),
                                  ("xp", "up", "timeScale", "exitflag", "lp", "slack", "info"), N, 12, "quad_resident_vs_host_pointer")
    ok = before["exitflag"] == 1
    r, _ = out[True]
    assert r["finite"][ok].all() and (r["dev_pos"][ok] > 0.05).all()      # forward Euler over 0.5 s: one interval is decimetres off
    print("resident quadcopter, N = 20: one interval %s m, open loop %s m" % (np.round(r["dev_pos"], 3), np.round(out[False][0]["dev_pos"], 3)))
    for i in np.flatnonzero(ok)[:2]:      # ... and the numpy statement on the downloaded solution
        X, P = V.rollout_quad(before["xp"][i], before["up"][i], before["timeScale"][i], bt["Ts"], 8, True)
        ref = V.rollout_record(before["xp"][i], X, V.quad_point_clearance(P, bt["ob"], bt["R"]), 8, True, 0.0)
        assert R.close([r[k][i] for k in KEYS], ref[[1, 3, 4, 5, 6, 7, 8, 9]], R.TOL_DEV) and r["dev_node"][i] == ref[2]
    # the plant of a receding horizon: the state the vehicle reaches after two intervals is where the next solve starts
    b.rollout(8, False); x2 = b.rollout_states()[:, 2]
    x2[~ok] = before["xp"][~ok, :, 2]
    b.shift_warm_start(2, x0_new=x2)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.rollout(8)
    b.solve(opts=OA.quad_warm_restart_opts()); nxt = b.download()
    print("stage 0 of the next solve against the rolled state: %.3g" % np.abs(nxt["xp"][:, :, 0] - x2).max())
    assert np.abs(nxt["xp"][:, :, 0] - x2).max() <= 1e-6
    b.close(); ctx.close()


def test_resident_parking_rollout(OA):
    B, N = 4, 30; bt = S.make_batch(S.BACKWARDS, B, N); ctx = OA.Context(0)
    b = upload_parking(OA, ctx, bt)
    before, out = resident_checks(OA, b, ctx, lambda o, restart: OA.parking_rollout_batch(N, bt["Ts"], bt["L"], bt["ego"], bt["vOb"], bt["A"], bt["b"], o["xp"], o["up"], o["timeScale"], 8, restart, V.DMIN),
                                  ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info"), N, 4, "parking_resident_vs_host_pointer")
    ok = before["exitflag"] == 1
    r, _ = out[True]
    assert r["finite"][ok].all() and (r["dev_att"][ok] < 1e-4).all() and (r["dev_rate"] == 0).all()      # the midpoint rule is exact in yaw and speed up to the solve's residual
    assert np.array_equal(r["clearance_min_nodes"], flat({"clearance": b.clearance(8)})["clearance_min_nodes"])      # restart mode keeps the solution's nodes as node samples
    print("resident parking, N = 30: one interval %s m, open loop %s m" % (np.round(r["dev_pos"], 5), np.round(out[False][0]["dev_pos"], 5)))
    b.rollout(8, False); x2 = b.rollout_states()[:, 2]
    b.shift_warm_start(2, x0_new=x2)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.rollout(8)
    b.solve(); nxt = b.download()
    print("stage 0 of the next solve against the rolled state: %.3g" % np.abs(nxt["xp"][:, :, 0] - x2).max())
    assert np.abs(nxt["xp"][:, :, 0] - x2).max() <= 1e-6
    b.close(); ctx.close()


def test_largest_differences_are_on_record():
    """the figures tools/rollout_rate.py copies into profiles/rollout_device_vs_host.json (OBCA_ROLLOUT_DIFFS names the file they are left in)"""
    print("device against host build / resident against host-pointer call:", WORST)
    path = os.environ.get("OBCA_ROLLOUT_DIFFS")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f)
