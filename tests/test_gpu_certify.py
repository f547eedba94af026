"""Clearance certificate on the device (include/obca_certify.h) against the host build of the same kernel text (tests/emu/certify_emu.cpp): the host-pointer entry points on
the synthetic and solved trajectories of the CPU suite, the resident calls after a solve, the device's own sampling as a witness, the quadcopter segment that a sampling
misses, and that a certify call leaves everything else of a batch alone.  Cases, comparison rules and tolerances: tests/certify_common.py.  The largest differences seen are
printed (tools/certify_rate.py writes them to the profile)."""
import os
import numpy as np
import pytest
import certify_common as K
from obca_amd import scenarios as S, validate as V

pytestmark = pytest.mark.gpu
G = V.CERT_TICKS
WORST = {}
PAIRS = ((V.DMIN, 0.01), (0.02, 0.002))


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.build_library()
    return obca_amd


def record(r, i):
    """row i of a returned dict, back in the layout of the C record"""
    return np.array([r["lb"][i], r["seen"][i], r["interval"][i], r["tick"][i], r["obstacle"][i], r["violated"][i], *r["first_violation"][i], r["undecided"][i], r["samples"][i],
                     r["samples_max"][i], r["lipschitz"][i], 1.0 if r["certified"][i] else 0.0, 0.0 if r["finite"][i] else 1.0, 0.0], float)


def parking_call(OA, batch, need=V.DMIN, slack=0.01, max_steps=G, ts=True, device=0):
    return OA.parking_certify_batch(batch[0]["N"], [c["Ts"] for c in batch], batch[0]["L"], batch[0]["ego"], [c["vOb"] for c in batch], [c["A"] for c in batch], [c["b"] for c in batch],
                                    np.stack([c["x"] for c in batch]), np.stack([c["u"] for c in batch]), np.stack([c["ts"] for c in batch]) if ts else None, need, slack, max_steps,
                                    device=device)


def quad_call(OA, cases, need=0.0, slack=0.01, max_steps=G, device=0):
    return OA.quadcopter_certify_batch(np.stack([c["x"] for c in cases]), np.stack([c["ts"] for c in cases]), cases[0]["Ts"], np.stack([c["ob"] for c in cases]), cases[0]["R"],
                                       need, slack, max_steps, device=device)


def same(a, b, rows=None):
    return all(np.array_equal(np.asarray(a[k])[rows] if rows is not None else a[k], np.asarray(b[k])[rows] if rows is not None else b[k], equal_nan=True) for k in a)


# ---------------------------------------------------------------- 6. device against host build: host-pointer entries
@pytest.mark.parametrize("N", (1, 2, 3))
def test_parking_host_pointer_call_matches_the_host_build_on_short_horizons(OA, N):
    """fewer items than lanes: 6, 9, 12"""
    batch = [K.synthetic_parking(kind, N) for kind in K.SYNTHETIC]
    for need, slack in PAIRS + ((0.3, 0.05),):
        r = parking_call(OA, batch, need, slack)
        assert r["intervals"].shape == (4, N + 1, 2)
        for i, c in enumerate(batch):
            host, hiv, _ = K.emu_parking(c, need, slack, vmax=max(K.vmax_of(b) for b in batch))
            K.check_device_parking(record(r, i), r["intervals"][i], host, hiv, "%s need %g slack %g" % (c["name"], need, slack), WORST)
    one = parking_call(OA, batch, V.DMIN, 0.01, max_steps=1)      # the near items run out of steps, on the device as in the host build
    for i, c in enumerate(batch):
        host, hiv, _ = K.emu_parking(c, V.DMIN, 0.01, max_steps=1)
        K.check_device_parking(record(one, i), one["intervals"][i], host, hiv, c["name"] + " max_steps 1")
    assert one["undecided"][0] > 0 and one["lb"][0] == -np.inf and not one["certified"][0] and one["certified"][3]      # (the car at rest needs one sample per item)


@pytest.mark.parametrize("name", ["backwards30", "corridor_sd", "corridor_dist"])
def test_parking_host_pointer_call_matches_the_host_build_on_solved_trajectories(OA, name):
    """N = 30 with 3 obstacles: 93 items, two rounds; N = 80 with 5: 405 items, seven rounds, 4- and 3-row obstacles"""
    c = K.golden_parking(name)
    for need, slack in PAIRS:
        r = parking_call(OA, [c], need, slack)
        host, hiv, _ = K.emu_parking(c, need, slack)
        K.check_device_parking(record(r, 0), r["intervals"][0], host, hiv, "%s need %g slack %g" % (name, need, slack), WORST)
    if name != "backwards30":      # the certificate finds what the nodes do not show
        r = parking_call(OA, [c], 0.05, 0.01)
        assert not r["certified"][0] and r["first_violation"][0, 0] == 13 and r["first_violation"][0, 2] == 3 and r["seen"][0] == 0.0 and r["intervals"][0, 13, 1] == 0.0
    print("largest parking difference device - host build so far: %.3g" % WORST["parking_value"])


def test_parking_host_pointer_call_in_chunks_marks_bad_instances_alone_and_refuses(OA, monkeypatch):
    batch = [K.synthetic_parking(kind, 3) for kind in K.SYNTHETIC] * 3
    whole = parking_call(OA, batch)
    monkeypatch.setenv("OBCA_CHUNK", "5")      # three chunks: every instance lands in its own rows of `out` and `iv`
    parts = parking_call(OA, batch)
    monkeypatch.delenv("OBCA_CHUNK")
    assert same(whole, parts)
    flat = [dict(c, ts=np.ones(4)) for c in batch]
    assert same(parking_call(OA, flat), parking_call(OA, flat, ts=False))      # no timeScale: 1
    short = OA.parking_certify_batch(3, [c["Ts"] for c in batch], batch[0]["L"], batch[0]["ego"], [c["vOb"] for c in batch], [c["A"] for c in batch], [c["b"] for c in batch],
                                     np.stack([c["x"] for c in batch]), np.stack([c["u"] for c in batch]), np.stack([c["ts"] for c in batch]), intervals=False)
    assert "intervals" not in short and same(short, whole)
    bad = [dict(c) for c in batch]
    bad[2] = dict(bad[2], x=bad[2]["x"].copy()); bad[2]["x"][1, 3] = np.nan
    bad[5] = dict(bad[5], u=bad[5]["u"].copy()); bad[5]["u"][0, 2] = np.inf
    bad[9] = dict(bad[9], ts=bad[9]["ts"].copy()); bad[9]["ts"][1] = np.nan
    rb = parking_call(OA, bad)
    assert (~rb["finite"]).nonzero()[0].tolist() == [2, 5, 9]
    want = V.certify_record(np.zeros((4, 3, 5)), np.zeros(3), finite=False)[0]
    for i in range(len(batch)):
        if i in (2, 5, 9):
            assert np.array_equal(record(rb, i), want, equal_nan=True) and np.isnan(rb["intervals"][i]).all()
        else:
            assert np.array_equal(record(rb, i), record(whole, i)) and np.array_equal(rb["intervals"][i], whole["intervals"][i])
    for kw, msg in ((dict(need=np.nan), "need"), (dict(need=np.inf), "need"), (dict(slack=0.0), "slack"), (dict(slack=-1.0), "slack"), (dict(slack=np.nan), "slack"),
                    (dict(max_steps=0), "max_steps"), (dict(max_steps=G + 1), "max_steps")):
        with pytest.raises(OA.ObcaError, match=msg):
            parking_call(OA, batch, **kw)


def test_quadcopter_host_pointer_call_is_the_host_build_bit_for_bit(OA):
    full = K.golden_quads()
    for cases in (full, [K.cut_quad(c, 3) for c in full], [K.cut_quad(c, 2) for c in full], [K.slip_quad()]):
        for need, slack in ((0.0, 0.01), (0.03, 0.005), (-0.3, 0.05)):
            r = quad_call(OA, cases, need, slack)
            for i, c in enumerate(cases):
                host, hiv, _ = K.emu_quad(c, need, slack)
                assert np.array_equal(record(r, i), host) and np.array_equal(r["intervals"][i], hiv), (c["name"], need, slack, record(r, i), host)
    tick = quad_call(OA, [K.slip_quad()], 1e3, 1e-9)      # a floor of zero: tick by tick, G samples per moving item
    host, hiv, _ = K.emu_quad(K.slip_quad(), 1e3, 1e-9)
    assert np.array_equal(record(tick, 0), host) and np.array_equal(tick["intervals"][0], hiv) and tick["samples_max"][0] == G and tick["undecided"][0] == 0
    assert quad_call(OA, [K.slip_quad()], 1e3, 1e-9, max_steps=G - 1)["undecided"][0] == 10
    x = np.stack([c["x"] for c in full]); x[1, 7, 0] = np.nan
    rb = OA.quadcopter_certify_batch(x, np.stack([c["ts"] for c in full]), full[0]["Ts"], full[0]["ob"], full[0]["R"])
    ok = quad_call(OA, full)
    assert rb["finite"].tolist() == [True, False, True, True] and np.isnan(rb["lb"][1]) and rb["interval"][1] == -1 and np.isnan(rb["intervals"][1]).all()
    assert all(np.array_equal(record(rb, i), record(ok, i)) and np.array_equal(rb["intervals"][i], ok["intervals"][i]) for i in (0, 2, 3))
    for kw, msg in ((dict(need=np.nan), "need"), (dict(slack=0.0), "slack"), (dict(max_steps=0), "max_steps")):
        with pytest.raises(OA.ObcaError, match=msg):
            quad_call(OA, full, **kw)


def test_quadcopter_slips_past_a_box_between_two_samples_on_the_device(OA):
    """issue 3(b) / 8: clearance(8) is clean at need = 0.03, certify is violated in interval 0"""
    c = K.slip_quad()
    clr = OA.quadcopter_clearance_batch(c["x"][None], c["ts"][None], c["Ts"], c["ob"], c["R"], 8, 0.03)
    assert clr["below"][0] == 0 and abs(clr["min"][0] - 0.0379) < 1e-4 and clr["finite"][0]
    r = quad_call(OA, [c], 0.03, 0.005)
    assert not r["certified"][0] and r["violated"][0] == 1 and r["first_violation"][0, 0] == 0 and r["first_violation"][0, 2] == 0 and r["seen"][0] < 0.03
    assert abs(r["seen"][0] - 0.02) < 1e-12 and G // 2 < r["first_violation"][0, 1] < 5 * G // 8 and r["interval"][0] == 0


# ---------------------------------------------------------------- 6 / 7 / 9. resident
def upload_parking(OA, ctx, bt):
    B, N = len(bt["Ts"]), bt["N"]
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    return b


def test_resident_parking_certify(OA):
    B, N = 16, 30; bt = S.make_batch(S.BACKWARDS, B, N); ctx = OA.Context(0)
    b = upload_parking(OA, ctx, bt)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.certify()
    b.solve(); before = b.download()
    with pytest.raises(OA.ObcaError, match="certify"):
        b.certify_intervals()
    with pytest.raises(OA.ObcaError, match="certify"):
        b.certify_ms()
    val0, clr0 = b.validate(), b.clearance(8)
    val_ms = b.validate_ms()
    per = isinstance(bt["vOb"], list)
    for need, slack in PAIRS:
        r = b.certify(need, slack); iv = b.certify_intervals()
        assert b.certify_ms() > 0 and iv.shape == (B, N + 1, 2) and r["finite"].all() and (before["exitflag"] == 1).all()
        # the host build on the downloaded solution
        for i in range(B):
            c = dict(N=N, Ts=float(bt["Ts"][i]), L=bt["L"], ego=bt["ego"], vOb=np.asarray(bt["vOb"][i] if per else bt["vOb"], np.int32), A=np.asarray(bt["A"][i] if per else bt["A"], float),
                     b=np.asarray(bt["b"][i] if per else bt["b"], float), x=before["xp"][i], u=before["up"][i], ts=V._stage_scale(before["timeScale"][i], N))
            host, hiv, _ = K.emu_parking(c, need, slack)
            K.check_device_parking(record(r, i), iv[i], host, hiv, "resident instance %d need %g slack %g" % (i, need, slack), WORST)
        # the host-pointer call on download() gives the same bits
        h = OA.parking_certify_batch(N, bt["Ts"], bt["L"], bt["ego"], bt["vOb"], bt["A"], bt["b"], before["xp"], before["up"], before["timeScale"], need, slack)
        assert same({k: v for k, v in h.items() if k != "intervals"}, r) and np.array_equal(h["intervals"], iv)
        # the device's own sampling is a witness: no sample lies under the proven bound, and a certified instance has none under need - slack
        c32 = b.clearance(32, need - slack)
        assert (r["lb"] <= c32["min"] + 1e-9).all() and (iv[:, :, 0].min(axis=1) == r["lb"]).all()
        assert (c32["below"][r["certified"]] == 0).all() and (np.minimum(need, r["seen"]) - slack <= r["lb"] + 1e-15).all() and (r["lb"] <= r["seen"]).all()
        print("resident parking, N = 30, need %g slack %g: certified %d of %d, lb %.4f .. %.4f, seen %.4f .. %.4f, clearance(32) min %.4f .. %.4f, samples per item %.2f (max %d), kernel %.3f ms" % (
            need, slack, r["certified"].sum(), B, r["lb"].min(), r["lb"].max(), r["seen"].min(), r["seen"].max(), c32["min"].min(), c32["min"].max(),
            r["samples"].mean() / ((N + 1) * 3), r["samples_max"].max(), b.certify_ms()))
    # nothing else moved: the iterate, validate's and clearance's results and their timers' state
    after = b.download()
    for k in ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info"):
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    assert abs(b.validate_ms() - val_ms) <= 1e-3 * val_ms      # (certify has events of its own: validate's still hold the time of its last call; two readings of one pair differ in the last digits)
    val1, clr1 = b.validate(), b.clearance(8)
    assert all(np.array_equal(val0[k], val1[k], equal_nan=True) for k in ("ok", "ref_ok", "viol")) and same(clr0, clr1)
    # after a shift the batch holds a warm start, not a solution
    b.shift_warm_start(2)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.certify()
    b.close(); ctx.close()


def test_resident_quadcopter_certify(OA):
    B, N = 4, 20; bt = S.make_quad_batch(B, N); ctx = OA.Context(0)
    b = OA.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.certify()
    b.solve(); before = b.download()
    with pytest.raises(OA.ObcaError, match="certify"):
        b.certify_intervals()
    val0, clr0 = b.validate(), b.clearance(8)
    val_ms = b.validate_ms()
    for need, slack in ((0.0, 0.01), (-0.05, 0.005)):
        r = b.certify(need, slack); iv = b.certify_intervals()
        assert b.certify_ms() > 0 and iv.shape == (B, N + 1, 2)
        for i in np.flatnonzero(r["finite"]):
            c = dict(N=N, Ts=float(bt["Ts"]), R=float(bt["R"]), ob=np.asarray(bt["ob"], float).reshape(5, 6), x=before["xp"][i], ts=V._stage_scale(before["timeScale"][i], N), name="resident%d" % i)
            host, hiv, _ = K.emu_quad(c, need, slack)
            assert np.array_equal(record(r, i), host) and np.array_equal(iv[i], hiv), (i, need, slack, record(r, i), host)
        h = OA.quadcopter_certify_batch(before["xp"], before["timeScale"], bt["Ts"], bt["ob"], bt["R"], need, slack)
        assert same({k: v for k, v in h.items() if k != "intervals"}, r) and np.array_equal(h["intervals"], iv, equal_nan=True)
        c32 = b.clearance(32, need - slack); f = r["finite"]
        assert f.any() and (r["lb"][f] <= c32["min"][f] + 1e-9).all() and (c32["below"][r["certified"]] == 0).all()
        print("resident quadcopter, N = 20, need %g slack %g: certified %d of %d, lb %s, seen %s, clearance(32) min %s, kernel %.3f ms" % (
            need, slack, r["certified"].sum(), B, r["lb"], r["seen"], c32["min"], b.certify_ms()))
    after = b.download()
    for k in ("xp", "up", "timeScale", "exitflag", "lp", "slack", "info"):
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    assert abs(b.validate_ms() - val_ms) <= 1e-3 * val_ms
    val1, clr1 = b.validate(), b.clearance(8)
    assert all(np.array_equal(val0[k], val1[k], equal_nan=True) for k in ("ok", "viol")) and same(clr0, clr1)
    b.close(); ctx.close()


def test_largest_differences_are_on_record():
    """the figures tools/certify_rate.py copies into profiles/certify_device_vs_host.json (OBCA_CERTIFY_DIFFS names the file they are left in)"""
    print("device against host build:", WORST)
    path = os.environ.get("OBCA_CERTIFY_DIFFS")
    if path:
        import json
        with open(path, "w") as f:
            json.dump(WORST, f)
