"""Clearance between the nodes on the device (include/obca_clearance.h) against the host build of the same kernel text (tests/emu/clearance_emu.cpp): the host-pointer entry
points on trajectories that were never solved, the solved golden cases that touch an obstacle between their nodes, and the resident calls after a solve.
Trajectories, comparison rules and tolerances: tests/clearance_common.py.  The largest differences seen are printed (tools/clearance_rate.py writes them to the profile)."""
import os
import numpy as np
import pytest
import clearance_common as K
from obca_amd import scenarios as S, validate as V

pytestmark = pytest.mark.gpu
NEED = V.DMIN
WORST = {}


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.build_library()
    return obca_amd


def parking_call(OA, batch, S_, need=NEED, device=0):
    B = len(batch)
    return OA.parking_clearance_batch(batch[0]["N"], [c["Ts"] for c in batch], batch[0]["L"], batch[0]["ego"], [c["vOb"] for c in batch], [c["A"] for c in batch], [c["b"] for c in batch],
                                      np.stack([c["x"] for c in batch]), np.stack([c["u"] for c in batch]), np.stack([c["ts"] for c in batch]), S_, need, device=device), B


def record(r, i):
    """row i of a returned dict, back in the layout of the C record"""
    out = np.zeros(V.CLR_OUT); out[8:] = np.inf
    out[0], out[1], out[2], out[3], out[4], out[5], out[6] = r["min"][i], r["min_nodes"][i], r["sample"][i], r["obstacle"][i], r["below"][i], r["samples"][i], 0.0 if r["finite"][i] else 1.0
    po = r["per_obstacle"][i]; out[8:8 + len(po)] = po
    return out


# ---------------------------------------------------------------- 1. host-pointer entries, no solve
@pytest.mark.parametrize("N,S_", K.SHAPES[1:])
def test_parking_host_pointer_call_matches_the_host_build(OA, N, S_):
    for bi, batch in enumerate(K.parking_cases(N, 12)):
        vm = K.vmax_of(batch)
        r, B = parking_call(OA, batch, S_)
        assert r["per_obstacle"].shape == (B, max(len(c["vOb"]) for c in batch)) and (r["stage"] == r["sample"] // S_).all() and (r["substep"] == r["sample"] % S_).all()
        for i, c in enumerate(batch):
            K.check_against_host_build(record(r, i), K.emu_parking(c, S_, NEED, vmax=vm), K.TOL_PARK, len(c["vOb"]), "N=%d S=%d batch %d instance %d" % (N, S_, bi, i),
                                       table=lambda c=c: K.ref_parking_table(c, S_), substeps=S_, need=NEED, worst=WORST, key="parking_device_vs_host_build")
    print("largest parking difference device - host build so far: %.3g" % WORST["parking_device_vs_host_build"])


def test_parking_host_pointer_call_in_chunks_and_without_time_scale(OA, monkeypatch):
    N, S_ = 7, 4; batch = K.parking_cases(N, 12)[2]
    whole, B = parking_call(OA, batch, S_)
    monkeypatch.setenv("OBCA_CHUNK", "5")      # three chunks on three lanes: every instance lands in its own row of `out`
    parts, _ = parking_call(OA, batch, S_)
    monkeypatch.delenv("OBCA_CHUNK")
    for k in whole:
        assert np.array_equal(whole[k], parts[k], equal_nan=True), k
    r1 = OA.parking_clearance_batch(N, [c["Ts"] for c in batch], batch[0]["L"], batch[0]["ego"], [c["vOb"] for c in batch], [c["A"] for c in batch], [c["b"] for c in batch],
                                    np.stack([c["x"] for c in batch]), np.stack([c["u"] for c in batch]), None, S_, NEED)
    for k in whole:      # (this batch's timeScale is 1)
        assert np.array_equal(whole[k], r1[k], equal_nan=True), k
    for S_bad, need in ((0, 0.05), (33, 0.05), (8, np.nan), (8, np.inf)):
        with pytest.raises(OA.ObcaError, match="substeps|need"):
            parking_call(OA, batch, S_bad, need)
    # non-finite input marks its instance and no other
    bad = [dict(c) for c in batch]
    bad[2] = dict(bad[2], x=bad[2]["x"].copy()); bad[2]["x"][1, 3] = np.nan
    bad[5] = dict(bad[5], u=bad[5]["u"].copy()); bad[5]["u"][0, 2] = np.inf
    bad[9] = dict(bad[9], ts=bad[9]["ts"].copy()); bad[9]["ts"][4] = np.nan
    rb, _ = parking_call(OA, bad, S_)
    assert (~rb["finite"]).nonzero()[0].tolist() == [2, 5, 9]
    for i in range(B):
        if i in (2, 5, 9):
            assert np.isnan(rb["min"][i]) and np.isnan(rb["min_nodes"][i]) and np.isnan(rb["per_obstacle"][i]).all() and rb["sample"][i] == rb["obstacle"][i] == rb["stage"][i] == -1
            assert rb["below"][i] == rb["samples"][i] == N * S_ + 1
        else:
            assert np.array_equal(record(rb, i), record(whole, i))


@pytest.mark.parametrize("N,S_", K.QUAD_SHAPES + ((7, 1), (2, 32), (60, 4)))
def test_quadcopter_host_pointer_call_matches_the_host_build(OA, N, S_):
    cases = K.quad_cases(N)
    for need in (0.0, 0.3):
        r = OA.quadcopter_clearance_batch(np.stack([c["x"] for c in cases]), np.stack([c["ts"] for c in cases]), cases[0]["Ts"], cases[0]["ob"], cases[0]["R"], S_, need)
        for i, c in enumerate(cases):
            K.check_against_host_build(record(r, i), K.emu_quad(c, S_, need), K.TOL_QUAD, 5, "quad N=%d S=%d instance %d" % (N, S_, i), worst=WORST, key="quad_device_vs_host_build")
    x = np.stack([c["x"] for c in cases]); x[1, 7, 0] = np.nan
    rb = OA.quadcopter_clearance_batch(x, np.stack([c["ts"] for c in cases]), cases[0]["Ts"], cases[0]["ob"], cases[0]["R"], S_, 0.3)
    assert rb["finite"].tolist() == [i != 1 for i in range(len(cases))] and np.isnan(rb["min"][1]) and rb["sample"][1] == -1
    assert all(np.array_equal(record(rb, i), record(r, i)) for i in range(len(cases)) if i != 1)
    print("largest quadcopter difference device - host build so far: %.3g" % WORST["quad_device_vs_host_build"])


def test_golden_cases_give_the_same_verdicts_on_the_device(OA):
    from test_clearance_cpu import golden_case
    for name, nodes in (("corridor_sd", 0.0551111), ("corridor_dist", 0.0501531)):
        c = golden_case(name)
        r, _ = parking_call(OA, [c], 8)
        assert r["finite"][0] and r["min_nodes"][0] >= 0.05 - 1e-6 and abs(r["min_nodes"][0] - nodes) < 1e-6 and r["min"][0] == 0.0
        assert (r["stage"][0], r["substep"][0], r["obstacle"][0]) == (13, 2, 3) and r["below"][0] >= 1 and r["samples"][0] == 641
    c = golden_case("backwards30")
    r, _ = parking_call(OA, [c], 8)
    assert r["min"][0] < r["min_nodes"][0] - 0.02 and abs(r["min"][0] - 0.024412) < 1e-6 and (r["sample"][0], r["obstacle"][0], r["below"][0]) == (164, 2, 7)


# ---------------------------------------------------------------- 2. resident
def upload_parking(OA, ctx, bt, x0=None):
    B, N = len(bt["Ts"]), bt["N"]
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"] if x0 is None else x0
    b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"] if x0 is None else x0, bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    return b


def same(a, b, rows=None):
    return all(np.array_equal(np.asarray(a[k])[rows] if rows is not None else a[k], np.asarray(b[k])[rows] if rows is not None else b[k], equal_nan=True) for k in a)


def test_resident_parking_clearance(OA):
    B, N = 16, 30; bt = S.make_batch(S.BACKWARDS, B, N); ctx = OA.Context(0)
    b = upload_parking(OA, ctx, bt)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.clearance(8)
    b.solve(opts=OA.ipopt_opts()); before = b.download()
    r = b.clearance(8)
    assert b.clearance_ms() > 0
    after = b.download()
    for k in ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info"):
        assert np.array_equal(before[k], after[k], equal_nan=True), k      # the iterate is read, nothing is written
    assert (before["exitflag"] == 1).all() and r["finite"].all() and (r["samples"] == 8 * N + 1).all() and (r["min"] <= r["min_nodes"]).all()
    print("resident parking, N = 30, 8 sub-steps: min_nodes %.4f .. %.4f, min %.4f .. %.4f" % (r["min_nodes"].min(), r["min_nodes"].max(), r["min"].min(), r["min"].max()))
    # the host-pointer call on the downloaded solution sees the same numbers: <= 1e-12, bits expected (the same packing code)
    h = OA.parking_clearance_batch(N, bt["Ts"], bt["L"], bt["ego"], bt["vOb"], bt["A"], bt["b"], before["xp"], before["up"], before["timeScale"], 8, NEED)
    for k in ("min", "min_nodes", "per_obstacle"):
        d = float(np.abs(r[k] - h[k]).max()); WORST["resident_vs_host_pointer"] = max(WORST.get("resident_vs_host_pointer", 0.0), d)
        assert d <= 1e-12, (k, d)
    for k in ("sample", "obstacle", "below", "samples", "finite"):
        assert np.array_equal(r[k], h[k]), k
    print("resident against host-pointer call: largest difference %.3g" % WORST["resident_vs_host_pointer"])
    # S = 1: the per-obstacle minima of DualMultWS's own d at the downloaded poses, after the clamp
    r1 = b.clearance(1)
    _, _, ds = OA.dualmult_ws_batch(N, bt["vOb"], bt["A"], bt["b"], before["xp"][:, 0, :], before["xp"][:, 1, :], before["xp"][:, 2, :], bt["ego"])
    dmin = np.stack([np.where(d < V.CLR_TOUCH, 0.0, d).min(axis=0) for d in ds])
    assert np.abs(r1["per_obstacle"] - dmin).max() <= 1e-9 and np.array_equal(r1["min"], r1["min_nodes"]) and np.array_equal(r1["min_nodes"], r["min_nodes"])
    for S_bad, need in ((0, 0.05), (33, 0.05), (8, np.nan)):
        with pytest.raises(OA.ObcaError, match="substeps|need"):
            b.clearance(S_bad, need)
    # a context that lists the device twice: the same bits
    ctx2 = OA.Context(devices=[0, 0]); b2 = upload_parking(OA, ctx2, bt); b2.solve(opts=OA.ipopt_opts())
    assert same(b2.clearance(8), r)
    assert same(OA.parking_clearance_batch(N, bt["Ts"], bt["L"], bt["ego"], bt["vOb"], bt["A"], bt["b"], before["xp"], before["up"], before["timeScale"], 8, NEED, device=ctx2), h)
    b2.close(); ctx2.close()
    # after a shift the batch holds a warm start, not a solution
    b.shift_warm_start(2)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.clearance(8)
    b.close()
    # an instance whose solve fails with a non-finite iterate (a NaN in its start): finite False there, the others as before
    x0 = bt["x0"].copy(); x0[3, 0] = np.nan
    b3 = upload_parking(OA, ctx, bt, x0=x0); b3.solve(opts=OA.ipopt_opts()); o3 = b3.download(); r3 = b3.clearance(8)
    assert o3["exitflag"][3] == 0 and not np.isfinite(o3["xp"][3]).all()
    assert not r3["finite"][3] and np.isnan(r3["min"][3]) and r3["sample"][3] == -1 and r3["below"][3] == r3["samples"][3]
    keep = np.arange(B) != 3
    assert same(r3, r, keep)
    b3.close(); ctx.close()


def test_resident_quadcopter_clearance(OA):
    B, N = 16, 20; bt = S.make_quad_batch(B, N); ctx = OA.Context(0)
    b = OA.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.clearance(8)
    b.solve(); before = b.download()
    r = b.clearance(8)
    assert b.clearance_ms() > 0
    after = b.download()
    for k in ("xp", "up", "timeScale", "exitflag", "lp", "slack", "info"):
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    ok = before["exitflag"] == 1
    assert ok.any() and r["finite"][ok].all() and (r["samples"] == 8 * N + 1).all() and (r["min"][ok] <= r["min_nodes"][ok]).all() and (r["min"][ok] >= -bt["R"]).all()
    print("resident quadcopter, N = 20, 8 sub-steps: min_nodes %.4f .. %.4f, min %.4f .. %.4f" % (r["min_nodes"][ok].min(), r["min_nodes"][ok].max(), r["min"][ok].min(), r["min"][ok].max()))
    h = OA.quadcopter_clearance_batch(before["xp"], before["timeScale"], bt["Ts"], bt["ob"], bt["R"], 8, 0.0)
    for k in ("min", "min_nodes", "per_obstacle"):
        assert np.allclose(r[k], h[k], rtol=0, atol=1e-12, equal_nan=True), k
    for k in ("sample", "obstacle", "below", "samples", "finite"):
        assert np.array_equal(r[k], h[k]), k
    for i in np.flatnonzero(ok)[:4]:      # ... and the numpy statement on the downloaded solution
        ref = V.quad_clearance(before["xp"][i], before["timeScale"][i], bt["Ts"], bt["ob"], bt["R"], 8)
        assert abs(r["min"][i] - ref[0]) <= K.TOL_QUAD and abs(r["min_nodes"][i] - ref[1]) <= K.TOL_QUAD and (r["sample"][i], r["obstacle"][i], r["below"][i]) == tuple(ref[2:5])
    ctx2 = OA.Context(devices=[0, 0]); b2 = OA.QuadBatch(ctx2, B, N)
    b2.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"]); b2.solve()
    assert same(b2.clearance(8), r) and same(OA.quadcopter_clearance_batch(before["xp"], before["timeScale"], bt["Ts"], bt["ob"], bt["R"], 8, 0.0, device=ctx2), h)
    b2.close(); ctx2.close()
    b.shift_warm_start(2)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.clearance(8)
    b.close(); ctx.close()


def test_largest_differences_are_on_record():
    """the figures tools/clearance_rate.py copies into profiles/clearance_device_vs_host.json (OBCA_CLEARANCE_DIFFS names the file they are left in)"""
    print("device against host build / resident against host-pointer call:", WORST)
    path = os.environ.get("OBCA_CLEARANCE_DIFFS")
    if path:
        import json
        with open(path, "w") as f:
            json.dump(WORST, f)
