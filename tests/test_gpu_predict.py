"""Clearance of a held plan against obstacles that move, on the device (include/obca_predict.h) through the C ABI: against the host build of the same kernel text
(tests/emu/predict_emu.cpp) fed the device's own download() and obstacles(), resident against host-pointer; zero rates against clearance(); a Galilean change of frame for
the quadcopter; consistency with move_obstacles() + clearance(); the staleness story of the drifting kerb; refusals.  Bounds: tests/predict_common.py.  The largest
differences seen are printed."""
import numpy as np
import pytest
import predict_common as K
import scene_edit_common as E
from obca_amd import scenarios as S, validate as V

pytestmark = pytest.mark.gpu
B_PARK, N_PARK, B_QUAD, N_QUAD = 8, 30, 4, 20


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.build_library()
    return obca_amd


@pytest.fixture(scope="module")
def ctx(OA):
    c = OA.Context(0)
    yield c
    c.close()


def upload(OA, ctx, bt):
    B, N = len(bt["Ts"]), bt["N"]
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    return b


@pytest.fixture(scope="module")
def park(OA, ctx):
    """make_batch(BACKWARDS, 8, 30) solved with default options: (batch dict, Batch, download)"""
    bt = S.make_batch(S.BACKWARDS, B_PARK, N_PARK); b = upload(OA, ctx, bt); b.solve(); o = b.download()
    assert (o["exitflag"] == 1).all()
    yield bt, b, o
    b.close()


@pytest.fixture(scope="module")
def quad(OA, ctx):
    bt = S.make_quad_batch(B_QUAD, N_QUAD); b = OA.QuadBatch(ctx, B_QUAD, N_QUAD)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"]); b.solve(OA.quadcopter_default_opts()); o = b.download()
    yield bt, b, o
    b.close()


def park_case(bt, o, i, vOb, A, b):
    return dict(N=bt["N"], Ts=float(bt["Ts"][i]), L=bt["L"], ego=bt["ego"], vOb=np.asarray(vOb, np.int32), A=np.asarray(A, float), b=np.asarray(b, float),
                x=np.ascontiguousarray(o["xp"][i]), u=np.ascontiguousarray(o["up"][i]), ts=np.ascontiguousarray(o["timeScale"][i]))


def quad_case(bt, o, i, ob):
    return dict(N=N_QUAD, Ts=float(np.ravel(bt["Ts"])[0]), R=bt["R"], ob=np.asarray(ob, float), x=np.ascontiguousarray(o["xp"][i]), ts=np.ascontiguousarray(o["timeScale"][i]))


def record(r, i):
    """instance i of the dict of a predict call, as the 32 doubles of its record (per_obstacle padded with +inf as the device pads it)"""
    per = np.full(16, np.inf); per[:r["per_obstacle"].shape[1]] = r["per_obstacle"][i]
    return np.r_[r["min"][i], r["min_nodes"][i], r["sample"][i], r["obstacle"][i], r["below"][i], r["samples"][i], float(not r["finite"][i]), 0.0, per,
                 r["first"][i], r["t_first"][i], r["first_obstacle"][i], r["t_min"][i], r["horizon"][i], r["moving"][i], 0.0, 0.0]


# ---------------------------------------------------------------- 1. device against host build
@pytest.mark.parametrize("S_", [1, 8])
def test_ragged_parking_batch_matches_the_host_build(OA, ctx, S_):
    """the five instances of the scene-edit tests (1 x 3 rows, 16 x 4, 8 + 3, the shipped scene twice, the last with a NaN in its rates) solved with default options;
    the host build is fed the device's own download() and obstacles(): values within 1e-9 max(1, |value|), every index, count and tau equal; the resident call bit-equal
    to the host-pointer call on download(); the profile likewise"""
    bt = E.ragged_batch(); b = upload(OA, ctx, bt); b.solve(); o = b.download(); A, bb = b.obstacles()
    nObs = [len(v) for v in bt["vOb"]]; Ms = [int(np.sum(v)) for v in bt["vOb"]]; oo = np.r_[0, np.cumsum(nObs)]; ro = np.r_[0, np.cumsum(Ms)]
    rng = np.random.default_rng(7); nt = sum(nObs)
    rates = np.c_[rng.uniform(-0.08, 0.08, (nt, 2)), rng.uniform(-0.05, 0.05, nt)]; pivot = rng.uniform(-3, 3, (nt, 2)); grow = rng.uniform(-0.002, 0.01, nt)
    rates[oo[4] + 1, 1] = np.nan; rates[3] = 0.0; grow[3] = 0.0
    r = b.predict_clearance(rates, pivot, grow, substeps=S_, profile=True); prof = b.predict_profile()
    assert b.predict_clearance_ms() > 0 and prof.shape == (5, bt["N"] * S_ + 1)
    A2, bb2 = b.obstacles()
    assert E.same(A, A2) and E.same(bb, bb2)      # nothing is written to the records
    worst = {}
    for i in range(5):
        c = park_case(bt, o, i, bt["vOb"][i], A[ro[i]:ro[i + 1]], bb[ro[i]:ro[i + 1]])
        rt = np.c_[rates, pivot, grow][oo[i]:oo[i + 1]]
        host, hprof = K.emu_parking(c, rt, S_, V.DMIN, vmax=8)
        K.check_parking(record(r, i), prof[i], host, hprof, K.TOL_DEV, "S=%d instance %d" % (S_, i), worst)
    print("device against host build, ragged parking batch, S=%d: %s" % (S_, worst))
    assert not r["finite"][4] and r["finite"][:4].all() and np.isnan(prof[4]).all() and r["moving"][:4].tolist() == [1, 15, 2, 3]
    h = OA.parking_predict_batch(bt["N"], bt["Ts"], bt["L"], bt["ego"], bt["vOb"], bt["A"], bt["b"], o["xp"], o["up"], o["timeScale"], rates, pivot, grow, substeps=S_, profile=True)
    for i in range(5):
        assert np.array_equal(record(r, i), record(h, i), equal_nan=True), i
    assert np.array_equal(prof, h["profile"], equal_nan=True)
    b.close()


@pytest.mark.parametrize("S_", [1, 8])
def test_quadcopter_batch_matches_the_host_build_bit_for_bit(OA, quad, S_):
    bt, b, o = quad; ob = b.obstacles()
    rng = np.random.default_rng(8); rates = rng.uniform(-0.3, 0.3, (B_QUAD, 5, 3)); grow = rng.uniform(-0.01, 0.03, (B_QUAD, 5)); rates[1, 2] = 0.0; grow[1, 2] = 0.0
    r = b.predict_clearance(rates, grow, substeps=S_, need=0.3, profile=True); prof = b.predict_profile()
    assert b.predict_clearance_ms() > 0 and E.same(b.obstacles(), ob)
    for i in range(B_QUAD):
        host, hprof = K.emu_quad(quad_case(bt, o, i, ob[i]), np.c_[rates[i], grow[i]], S_, 0.3)
        assert np.array_equal(record(r, i), host, equal_nan=True) and np.array_equal(prof[i], hprof, equal_nan=True), (i, record(r, i), host)
    h = OA.quadcopter_predict_batch(o["xp"], o["timeScale"], bt["Ts"], bt["ob"], bt["R"], rates, grow, substeps=S_, need=0.3, profile=True)
    for i in range(B_QUAD):
        assert np.array_equal(record(r, i), record(h, i), equal_nan=True), i
    assert np.array_equal(prof, h["profile"], equal_nan=True) and r["moving"].tolist() == [5, 4, 5, 5]
    bad = rates.copy(); bad[2, 4, 0] = np.inf
    r2 = b.predict_clearance(bad, grow, substeps=S_, need=0.3, profile=True); prof2 = b.predict_profile()
    assert r2["finite"].tolist() == [True, True, False, True] and np.isnan(prof2[2]).all() and np.isnan(r2["t_min"][2]) and r2["first"][2] == -1
    for i in (0, 1, 3):
        assert np.array_equal(record(r2, i), record(r, i)) and np.array_equal(prof2[i], prof[i])


# ---------------------------------------------------------------- 2. zero rates
def test_zero_rates_are_clearance_and_nothing_is_written(OA, park, quad):
    bt, b, o = park; A, bb = b.obstacles()
    for S_ in (1, 8):
        c = b.clearance(S_); r = b.predict_clearance(substeps=S_)
        assert np.array_equal(r["sample"], c["sample"]) and np.array_equal(r["obstacle"], c["obstacle"]) and np.array_equal(r["below"], c["below"]) and np.array_equal(r["samples"], c["samples"])
        d = max(np.abs(r["min"] - c["min"]).max(), np.abs(r["min_nodes"] - c["min_nodes"]).max(), np.abs(r["per_obstacle"] - c["per_obstacle"]).max())
        print("parking, zero rates against clearance(), S=%d: largest difference %.3g, bit-equal: %s" % (S_, d, d == 0.0))
        assert d <= K.TOL_DEV and not r["moving"].any() and r["finite"].all()
        assert np.array_equal(np.isfinite(r["t_first"]), c["below"] > 0) and np.array_equal(r["first"] >= 0, c["below"] > 0)
    A2, bb2 = b.obstacles()
    assert E.same(A, A2) and E.same(bb, bb2)
    bq, q, _ = quad; ob = q.obstacles()
    for S_ in (1, 8):
        c = q.clearance(S_, need=0.3); r = q.predict_clearance(substeps=S_, need=0.3)
        for k in ("min", "min_nodes", "sample", "obstacle", "below", "samples", "per_obstacle", "finite"):
            assert np.array_equal(r[k], c[k]), (S_, k)
    assert E.same(q.obstacles(), ob)


# ---------------------------------------------------------------- 3. a Galilean change of frame
def test_quadcopter_boxes_with_one_velocity_are_a_moving_frame(OA, quad):
    """all five boxes move with the same velocity v: the clearances are those of quadcopter_clearance_batch on the trajectory seen from the boxes, p_k - v cum_k Ts and
    v_k - v (cum_k = k t for the batch's one t).  Values within 1e-12 absolute: a dozen operations on numbers of size <= 10."""
    bt, b, o = quad; v = np.array([0.11, -0.07, 0.05])
    r = b.predict_clearance(v, substeps=8, need=0.3)
    x = o["xp"].copy(); Ts = float(np.ravel(bt["Ts"])[0])
    for i in range(B_QUAD):
        cum = np.r_[0.0, np.cumsum(o["timeScale"][i][:N_QUAD])]
        x[i, :3] -= v[:, None] * (cum * Ts)[None, :]; x[i, 6:9] -= v[:, None]
    c = OA.quadcopter_clearance_batch(x, o["timeScale"], bt["Ts"], bt["ob"], bt["R"], substeps=8, need=0.3)
    d = max(np.abs(r["min"] - c["min"]).max(), np.abs(r["min_nodes"] - c["min_nodes"]).max(), np.abs(r["per_obstacle"] - c["per_obstacle"]).max())
    print("Galilean check, largest difference %.3g" % d)
    assert d <= 1e-12 and (r["moving"] == 5).all() and r["finite"].all() and np.abs(r["horizon"] - N_QUAD * o["timeScale"][:, 0] * Ts).max() <= 1e-12


# ---------------------------------------------------------------- 4. consistency with move_obstacles
def test_the_scene_at_t_min_is_the_one_move_obstacles_makes(OA, ctx, park):
    """the record's t_min, then move_obstacles(rate * t_min, pivot, grow * t_min) on a second upload of the same solved problem and clearance(S) there: its entry for
    obstacle [3] is <= the predicted minimum + 1e-9 (the sample of the minimum is among its samples, in the same scene); entry [2] of the profile IS the minimum"""
    bt, b, o = park; S_ = 8
    rate = np.array([[0.002, 0.0, 0.0003], [-0.001, 0.0005, 0.0], [0.0, -0.0005, -0.0001]]); pivot = np.array([[-1.3, 5.0], [0.0, 0.0], [4.0, 11.0]]); grow = np.array([0.0003, 0.0, 0.0003])
    r = b.predict_clearance(np.tile(rate, (B_PARK, 1)), np.tile(pivot, (B_PARK, 1)), np.tile(grow, B_PARK), substeps=S_, profile=True); prof = b.predict_profile()
    assert r["finite"].all() and (r["moving"] == 3).all() and (r["min"] > 0).any()      # (not every minimum is a contact: the comparison below says something)
    assert np.array_equal(prof[np.arange(B_PARK), r["sample"]], r["min"]) and np.array_equal(prof.min(axis=1), r["min"])
    b2 = upload(OA, ctx, bt); b2.solve(); o2 = b2.download()
    assert E.same(o2["xp"], o["xp"]) and E.same(o2["up"], o["up"])      # the same solved problem, to the bit
    tm = np.repeat(r["t_min"], 3)
    assert not b2.move_obstacles(np.tile(rate, (B_PARK, 1)) * tm[:, None], np.tile(pivot, (B_PARK, 1)), np.tile(grow, B_PARK) * tm).any()
    c = b2.clearance(S_)
    at = c["per_obstacle"][np.arange(B_PARK), r["obstacle"]]
    print("clearance() in the scene moved to t_min, obstacle of the predicted minimum: %s; predicted: %s" % (np.round(at, 6).tolist(), np.round(r["min"], 6).tolist()))
    assert (at <= r["min"] + 1e-9).all()
    b2.close()


# ---------------------------------------------------------------- 5. the staleness story
def test_a_drifting_kerb_is_seen_before_it_arrives(OA, ctx, park):
    """the left kerb of the scene-edit test moves onto the paths at 0.215 m per horizon.  The instances with a finite t_first are the numpy statement's (the host build's
    own distance on the rows numpy moved; no sample within 1e-6 of the need), a superset of those clearance() flags in the unmoved scene; and for each of them clearance()
    after move_obstacles() to the time t_first has min < need.  (Measured: the same set as in the unmoved scene -- the kerb arrives after the car has passed it, the
    instances it would reach at its full 0.215 m are clear while it is still on its way; what changes is WHEN: t_first is the answer clearance() cannot give.)"""
    bt, b, o = park; S_ = 8; need = V.DMIN
    still = b.predict_clearance(substeps=S_); hz = still["horizon"]
    rate = np.zeros((B_PARK, 3, 3)); rate[:, 0, 0] = 0.215 / hz
    r = b.predict_clearance(rate.reshape(-1, 3), substeps=S_, need=need)
    flagged = np.isfinite(r["t_first"]); now = b.clearance(S_, need=need)["below"] > 0
    want = []
    for i in range(B_PARK):
        c = park_case(bt, o, i, bt["vOb"], bt["A"], bt["b"])
        rec, rprof, _, tau = K.ref_parking(c, np.c_[rate[i], np.zeros((3, 3))], S_, need)
        assert np.abs(rprof - need).min() > 1e-6, i      # (no sample sits on the threshold: the comparison below is not a matter of rounding)
        want.append(bool(np.isfinite(rec[25])))
        if want[-1]:
            assert r["first"][i] == rec[24] and r["t_first"][i] == rec[25] and r["first_obstacle"][i] == rec[26], (i, record(r, i)[24:], rec[24:])
    print("finite t_first: %s (numpy statement %s); flagged by clearance() in the unmoved scene: %s; t_first %s of horizons %s" %
          (flagged.tolist(), want, now.tolist(), np.round(r["t_first"], 3).tolist(), np.round(hz, 3).tolist()))
    assert flagged.tolist() == want and (flagged | ~now).all() and flagged.any() and (r["moving"] == 1).all()
    b2 = upload(OA, ctx, bt); b2.solve()
    t = np.where(flagged, r["t_first"], 0.0)
    assert not b2.move_obstacles((rate * t[:, None, None]).reshape(-1, 3)).any()
    moved = b2.clearance(S_, need=need)
    assert (moved["min"][flagged] < need).all()
    b2.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals(OA, ctx, park, quad):
    from obca_amd import api
    bt = S.make_batch(S.BACKWARDS, 2, 6); b = upload(OA, ctx, bt)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.predict_clearance()
    with pytest.raises(OA.ObcaError, match="predict"):
        b.predict_clearance_ms()
    with pytest.raises(OA.ObcaError, match="profile"):
        b.predict_profile()
    b.solve()
    for S_ in (0, 33):
        with pytest.raises(OA.ObcaError, match="substeps"):
            b.predict_clearance(substeps=S_)
    out = np.zeros((2, 32))
    assert api._load().obca_batch_predict_clearance(b._h, None, 8, 0.05, 0, out) == -1 and b"NULL" in api._load().obca_last_error(ctx._h)
    b.predict_clearance()
    with pytest.raises(OA.ObcaError, match="profile"):      # a call that kept none
        b.predict_profile()
    assert b.predict_clearance_ms() > 0
    b.predict_clearance(substeps=2, profile=True)
    small = np.zeros(5)
    assert api._load().obca_batch_predict_profile(b._h, small, small.size) == -1 and b"capacity" in api._load().obca_last_error(ctx._h)
    assert b.predict_profile().shape == (2, 13)
    b.predict_clearance(substeps=4, profile=True)      # a later call that needs more: the buffer grows
    assert b.predict_profile().shape == (2, 25)
    b.close()
    _, q, _ = quad
    qn = OA.QuadBatch(ctx, 2, 4)
    with pytest.raises(OA.ObcaError):
        qn.predict_clearance()
    with pytest.raises(OA.ObcaError, match="predict"):
        qn.predict_clearance_ms()
    qn.close()
    for S_ in (0, 33):
        with pytest.raises(OA.ObcaError, match="substeps"):
            q.predict_clearance(substeps=S_)
    assert api._load().obca_quad_batch_predict_clearance(q._h, None, 8, 0.0, 0, np.zeros((B_QUAD, 32))) == -1
