"""The obstacles of a resident batch moved and inflated in place on the device (include/obca_scene_edit.h) through the C ABI: against the host build of the same kernel
text (tests/emu/scene_edit_emu.cpp) on the ragged batch of the CPU tests and on the quadcopter batch; a solve after a move against the solve of a fresh upload of the rows
read back; the warm restart across a move, judged by the CPU oracle started from tests/shift_common.py's statement of the shift in the host-moved scene; clearance() of a
held solution as a staleness query; refine() + move_obstacles(inflate=m) as the parking margin.  Bounds: tests/scene_edit_common.py; trajectories: TOL_X of
tests/test_gpu_parity.py.  The largest differences seen are printed."""
import numpy as np
import pytest
import packing as P
import clearance_common as K
import scene_edit_common as E
import shift_common as SC
from obca_amd import scenarios as S, validate as V
from test_gpu_parity import TOL_X

pytestmark = pytest.mark.gpu
B_PARK, N_PARK = 8, 30
TOL_D = 2e-8      # the duality gap DualMultWS leaves (tests/test_dualws_geometry_cpu.py)


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


@pytest.fixture(scope="module")
def park():
    return S.make_batch(S.BACKWARDS, B_PARK, N_PARK)


def upload(OA, ctx, bt, rows=None):
    """the batch uploaded as the solve calls of the sibling tests upload it; rows: (A, b) in place of the batch's own"""
    B, N = len(bt["Ts"]), bt["N"]
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    A, bb = (bt["A"], bt["b"]) if rows is None else rows
    b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], A, bb, xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    return b, xWS


def records_of(A, b, vObs):
    """parking records (B, OB_HDR) that hold the unit rows A, b of instances with the row counts vObs: what the host build is fed"""
    out = np.zeros((len(vObs), P.OB_HDR)); r = 0
    for i, v in enumerate(vObs):
        v = np.asarray(v, int); m = int(v.sum())
        out[i, P.PH["NOB"]] = len(v); out[i, P.PH["M"]] = m; out[i, P.PH["VOB"]:P.PH["VOB"] + len(v)] = v; out[i, P.PH["ROFF"]:P.PH["ROFF"] + len(v) + 1] = np.r_[0, np.cumsum(v)]
        out[i, P.PH["A"]:P.PH["A"] + 2 * m] = A[r:r + m].reshape(-1); out[i, P.PH["B"]:P.PH["B"] + m] = b[r:r + m]; r += m
    return out


def case(bt, o, i, rows=None, N=None, Ts=None):
    """instance i of the download o as a case of tests/clearance_common.py, against the rows (A, b) of the whole batch (every instance holds the same three obstacles)"""
    A, b = (bt["A"], bt["b"]) if rows is None else rows
    return dict(N=N or bt["N"], Ts=float(bt["Ts"][i] if Ts is None else Ts), L=bt["L"], ego=bt["ego"], vOb=np.asarray(bt["vOb"], np.int32), A=np.asarray(A, float), b=np.asarray(b, float),
                x=o["xp"][i], u=o["up"][i], ts=o["timeScale"][i])


# ---------------------------------------------------------------- 1. device against host build
def test_ragged_parking_batch_matches_the_host_build(OA, ctx):
    """the five instances of the CPU test (1 x 3 rows, 16 x 4, 8 + 3, the shipped scene twice, the last with a NaN in its motion): rows within 1e-9 max(1, |value|) of the
    host build fed the device's own rows, status equal, the NaN instance bit for bit what it was; obstacles() returns what upload() packed, and a fresh upload of the rows
    read back holds them again (to the ulp: an upload divides by a row length that is 1 to the last bit or two)"""
    bt = E.ragged_batch(); b, _ = upload(OA, ctx, bt)
    with pytest.raises(OA.ObcaError, match="move"):
        b.move_obstacles_ms()
    A0, b0 = b.obstacles()
    Ap, bp, v = E.rows_of(E.pack_ragged(bt))
    assert E.same(A0, Ap) and E.same(b0, bp)
    motion, pivot, inflate = E.ragged_motion()
    st = b.move_obstacles(motion, pivot, inflate)
    A1, b1 = b.obstacles()
    assert b.move_obstacles_ms() > 0
    host, hst = E.emu_move_parking(records_of(A0, b0, bt["vOb"]), motion, pivot, inflate)
    Ah, bh, _ = E.rows_of(host)
    w = max(E.worst(A1, Ah), E.worst(b1, bh)); print("device against host build, ragged parking batch: %.3g" % w)
    assert st.tolist() == hst.tolist() == [0, 0, 0, 0, 1] and w <= E.TOL_DEV
    assert E.same(A1[-12:], A0[-12:]) and E.same(b1[-12:], b0[-12:]) and not E.same(A1[:-12], A0[:-12])
    assert np.abs(np.hypot(A1[:, 0], A1[:, 1]) - 1.0).max() <= 4 * np.finfo(float).eps
    # nothing to do: no bit changes; a translation: no bit of A
    assert not b.move_obstacles().any() and not b.move_obstacles(np.zeros(3), [1.0, 2.0], 0.0).any()
    A2, b2 = b.obstacles()
    assert E.same(A2, A1) and E.same(b2, b1)
    assert not b.move_obstacles([0.1, -0.2, 0.0]).any()
    A3, b3 = b.obstacles()
    assert E.same(A3, A1) and np.abs(b3 - (b1 + A1 @ np.array([0.1, -0.2]))).max() <= 1e-13
    # per-instance values go over each instance's obstacles
    per = np.arange(5.0) * 0.01
    b.move_obstacles(inflate=per); A4, b4 = b.obstacles()
    assert E.same(A4, A3) and np.abs(b4 - (b3 + np.repeat(per, [3, 64, 11, 12, 12]))).max() <= 1e-15
    b2nd, _ = upload(OA, ctx, dict(bt), rows=(np.split(A4, np.cumsum([3, 64, 11, 12])), np.split(b4, np.cumsum([3, 64, 11, 12]))))
    A5, b5 = b2nd.obstacles()
    assert np.abs(A5 - A4).max() <= 4 * np.finfo(float).eps and E.worst(b5, b4) <= 4 * np.finfo(float).eps
    b.close(); b2nd.close()


def test_quadcopter_batch_matches_the_host_build_bit_for_bit(OA, ctx):
    Bq, Nq = 4, 20; bt = S.make_quad_batch(Bq, Nq); b = OA.QuadBatch(ctx, Bq, Nq)
    with pytest.raises(OA.ObcaError, match="uploaded"):
        b.move_obstacles([0.1, 0, 0])
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    # the checks of a held solution read the moved boxes: boxes shrunk by 5 cm are nowhere closer than they were
    b.solve(OA.quadcopter_default_opts()); c0 = b.clearance(8); held = b.download()
    assert not b.move_obstacles(inflate=-0.05).any()
    c1 = b.clearance(8); fin = c0["finite"] & c1["finite"]
    print("quadcopter clearance of the held solution: %s, boxes shrunk by 0.05: %s" % (np.round(c0["min"], 4).tolist(), np.round(c1["min"], 4).tolist()))
    assert fin.any() and (c1["min"][fin] >= c0["min"][fin]).all() and (c1["min"][fin] > c0["min"][fin]).any() and E.same(b.download()["xp"], held["xp"])
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    ob0 = b.obstacles(); ws0 = b.warm_start()
    assert ob0.shape == (Bq, 5, 6) and E.same(ob0, np.broadcast_to(np.asarray(bt["ob"], float).reshape(-1, 5, 6), (Bq, 5, 6)))
    rng = np.random.default_rng(4); motion = rng.uniform(-0.3, 0.3, (Bq, 5, 3)); inflate = rng.uniform(-0.02, 0.1, (Bq, 5)); motion[2, 1, 2] = np.nan
    st = b.move_obstacles(motion, inflate); ob1 = b.obstacles()
    rec = np.zeros((Bq, P.QPH_SIZE)); rec[:, P.QPH_OB:P.QPH_OB + 30] = ob0.reshape(Bq, 30)
    host, hst = E.emu_move_quad(rec, motion, inflate)
    assert st.tolist() == hst.tolist() == [0, 0, 1, 0] and E.same(ob1.reshape(Bq, 30), host[:, P.QPH_OB:P.QPH_OB + 30]) and E.same(ob1[2], ob0[2]) and b.move_obstacles_ms() > 0
    ws1 = b.warm_start()
    assert E.same(ws0[0], ws1[0]) and E.same(ws0[1], ws1[1])      # the warm start behind the header keeps its bits
    assert not b.move_obstacles().any() and E.same(b.obstacles(), ob1)
    b.move_obstacles([0.5, 0.0, -0.25], 0.05)
    d = np.array([0.5, 0.0, -0.25, -0.5, 0.0, 0.25])
    assert E.same(b.obstacles(), (ob1 + d) + 0.05)
    b.close()


# ---------------------------------------------------------------- 2. the same solve as a fresh upload
def test_solve_after_a_move_is_the_solve_of_a_fresh_upload(OA, ctx, park):
    """upload, move (a kerb turned by 5 mrad about its corner and pushed 5 cm, the far wall 3 cm down, two inflations), solve -- against an upload of the rows read back,
    solved from the same start: exit flags and iteration counts equal, trajectories within TOL_X of tests/test_gpu_parity.py"""
    bt = park; b, _ = upload(OA, ctx, bt)
    motion = np.array([[0.05, 0.02, 0.005], [0, 0, 0], [0, -0.03, 0]]); pivot = np.array([[-1.3, 5.0], [0, 0], [0, 0]]); inflate = np.array([0.01, 0.0, 0.02])
    st = b.move_obstacles(np.tile(motion, (B_PARK, 1)), np.tile(pivot, (B_PARK, 1)), np.tile(inflate, B_PARK))
    assert not st.any()
    A, bb = b.obstacles()
    assert E.same(A.reshape(B_PARK, -1), np.tile(A[:5].reshape(1, -1), (B_PARK, 1)))      # every instance holds the same moved scene
    Aref, bref, ok = V.move_obstacles_parking(bt["A"], bt["b"], bt["vOb"], motion, pivot, inflate)
    assert ok and max(E.worst(A[:5], Aref), E.worst(bb[:5], bref)) <= E.TOL_DEV
    b.solve(); o1 = b.download()
    f, _ = upload(OA, ctx, bt, rows=(A[:5], bb[:5])); f.solve(); o2 = f.download()
    dx = float(max(np.abs(o1["xp"] - o2["xp"]).max(), np.abs(o1["up"] - o2["up"]).max()))
    print("move + solve against fresh upload + solve: exit flags %s, iterations %s / %s, largest trajectory difference %.3g" % (o1["exitflag"].tolist(), o1["iters"].tolist(), o2["iters"].tolist(), dx))
    assert (o1["exitflag"] == 1).all() and np.array_equal(o1["exitflag"], o2["exitflag"]) and np.array_equal(o1["iters"], o2["iters"]) and dx < TOL_X
    # ... and it is not the solve of the unmoved scene
    u, _ = upload(OA, ctx, bt); u.solve(); o3 = u.download()
    assert np.abs(o1["xp"] - o3["xp"]).max() > 1e-3
    b.close(); f.close(); u.close()


# ---------------------------------------------------------------- 3. the restart survives
def test_warm_restart_across_a_move_follows_the_oracle(OA, ctx, oracle, park):
    """solve; advance(2); the left kerb drifts 5 cm towards the slot and the road ((0.03, 0.04)); solve with warm_restart_opts().  The move leaves the plant state, the
    held solution and the restart where advance() put them; the solve is accepted, validate() is ok against the moved field, and the CPU oracle started from the shift
    statement of the device's own download, in the scene moved by the numpy statement, takes the same exit flags and iteration counts on all 8 (checked on the CPU
    beforehand: the oracle solves all 8, 13 - 17 iterations)."""
    bt = park; N, shift = N_PARK, 2; b, xWS = upload(OA, ctx, bt)
    b.solve(); prev = b.download()
    assert (prev["exitflag"] == 1).all()
    r = b.advance(shift); st0 = b.advance_state(); held = b.download()
    assert r["finite"].all()
    motion = np.zeros((3, 3)); motion[0] = [0.03, 0.04, 0.0]
    assert not b.move_obstacles(np.tile(motion, (B_PARK, 1))).any()
    assert E.same(b.advance_state(), st0) and E.same(b.download()["xp"], held["xp"]) and E.same(b.download()["up"], held["up"])
    b.solve(OA.warm_restart_opts()); cur = b.download(); val = b.validate()
    A1, b1, ok = V.move_obstacles_parking(bt["A"], bt["b"], bt["vOb"], motion)
    Ad, bd = b.obstacles()
    assert ok and E.same(Ad[:5], A1) and E.same(bd[:5], b1)      # a translation: additions and products only, the bits of the numpy statement
    oo = oracle.default_opts(); w = OA.warm_restart_opts(); oo.mu_init = w.mu_init; oo.bound_push = w.bound_push; oo.bound_frac = w.bound_frac
    worst = 0.0
    for i in range(B_PARK):
        sp = SC.shifted_problem(N, shift, prev, i, xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], st0[i])
        q = oracle.parking_signed_dist(sp["x0"], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], A1, b1, sp["rx"], sp["ry"], sp["ryaw"], 0,
                                       sp["xWS"], sp["uWS"], sp["lWS"], sp["nWS"], opts=oo)
        what = "instance %d: device exit flag %d, %d iterations; oracle %d, %d" % (i, cur["exitflag"][i], cur["iters"][i], q["exitflag"], q["iters"])
        print(what)
        assert q["exitflag"] == 1 and cur["exitflag"][i] == q["exitflag"] and cur["iters"][i] == q["iters"], what
        dx = float(max(np.abs(cur["xp"][i] - q["xp"]).max(), np.abs(cur["up"][i] - q["up"]).max())); worst = max(worst, dx)
        assert dx < TOL_X and np.array_equal(cur["xp"][i][:, 0], st0[i]), (what, dx)
    print("warm restart across the move, device - oracle: %.3g; cold %s iterations, restart %s" % (worst, prev["iters"].tolist(), cur["iters"].tolist()))
    assert val["ok"].all() and cur["iters"].mean() < prev["iters"].mean()
    b.close()


# ---------------------------------------------------------------- 4. the staleness query
def test_clearance_of_the_held_solution_answers_for_the_moved_scene(OA, ctx, park):
    """on a solved batch the left kerb moves 0.215 m towards the path (the paths keep 0.25 - 0.28 m to it): clearance() flags exactly the instances the numpy statement
    -- validate.parking_samples of the downloaded solution, the oracle's DualMultWS distance to the host-moved rows -- flags; on the CPU oracle's solutions these are
    {0, 2, 3, 4, 5, 6, 7} after the move against {0, 2, 3, 5, 6} before, no sample within 1e-4 of the need."""
    bt = park; b, _ = upload(OA, ctx, bt); b.solve(); o = b.download()
    before = b.clearance(8)
    motion = np.zeros((3, 3)); motion[0] = [0.215, 0.0, 0.0]
    assert not b.move_obstacles(np.tile(motion, (B_PARK, 1))).any()
    after = b.clearance(8); o2 = b.download()
    assert E.same(o["xp"], o2["xp"]) and np.array_equal(o["exitflag"], o2["exitflag"])      # the held solution is what it was
    A1, b1, ok = V.move_obstacles_parking(bt["A"], bt["b"], bt["vOb"], motion)
    flags = []
    for i in range(B_PARK):
        rowmin = K.ref_parking_table(case(bt, o, i, rows=(A1, b1)), 8).min(axis=1)
        assert np.abs(rowmin - V.DMIN).min() > 1e-6, i      # (no sample sits on the threshold: the comparison below is not a matter of rounding)
        flags.append(int((rowmin < V.DMIN).sum()))
        assert abs(after["min"][i] - rowmin.min()) <= 1e-6
    print("samples under %.2f before the move %s, after %s, numpy statement %s" % (V.DMIN, before["below"].tolist(), after["below"].tolist(), flags))
    assert np.array_equal(after["below"] > 0, np.array(flags) > 0) and np.array_equal(after["below"], flags)
    assert not np.array_equal(after["below"] > 0, before["below"] > 0) and 0 < (after["below"] > 0).sum() < B_PARK
    b.close()


# ---------------------------------------------------------------- 5. the parking margin
def test_refine_then_inflate_is_a_margin_against_the_true_obstacles(OA, ctx, park):
    """the instances clearance() flags are refined (factor 2), the destination's obstacles inflated by m = 0.03, the fine problems solved: clearance(need=DMIN) of the result
    is measured against the inflated rows, and against the original rows (numpy statement) the smallest clearance is at least m larger, within 2e-8"""
    bt = park; m = 0.03; b, _ = upload(OA, ctx, bt); b.solve()
    c1 = b.clearance(8); sel = np.flatnonzero(c1["below"] > 0)
    assert 0 < len(sel) < B_PARK
    d, st = b.refine(2, select=sel)
    assert (st == 0).all() and not d.move_obstacles(inflate=m).any()
    Ai, bi = d.obstacles(); A0, b0 = b.obstacles()
    assert E.same(Ai[:5], A0[:5]) and np.abs(bi[:5] - (b0[:5] + m)).max() <= 1e-15
    d.solve(); o = d.download(); c2 = d.clearance(4, need=V.DMIN)
    assert (o["exitflag"] == 1).all(), o["exitflag"]
    for j, i in enumerate(sel):
        cs = dict(case(bt, o, j, N=2 * N_PARK, Ts=bt["Ts"][i] / 2))
        t_true = K.ref_parking_table(cs, 4).min(); t_infl = K.ref_parking_table(dict(cs, A=Ai[:5], b=bi[:5]), 4).min()
        print("instance %d: smallest clearance against the inflated rows %.6f (device %.6f), against the original rows %.6f: %.3g beyond m" % (i, t_infl, c2["min"][j], t_true, t_true - t_infl - m))
        assert abs(c2["min"][j] - t_infl) <= 1e-6 and c2["min"][j] > 0
        assert t_true >= c2["min"][j] + m - TOL_D and t_true >= t_infl + m - TOL_D
    b.close(); d.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_batch_as_it_was(OA, ctx, park):
    from obca_amd import api
    b = OA.Batch(ctx, B_PARK, N_PARK); st = np.zeros(B_PARK, np.int32); A = np.zeros((40, 2)); bb = np.zeros(40)
    assert api._load().obca_batch_move_obstacles(b._h, None, None, None, st) == -1 and api._load().obca_batch_obstacles_download(b._h, A, bb) == -1      # nothing uploaded
    b.close()
    b, _ = upload(OA, ctx, park)
    assert api._load().obca_batch_move_obstacles(b._h, None, None, None, None) == -1 and api._load().obca_batch_obstacles_download(b._h, None, None) == -1      # NULL arguments
    with pytest.raises(ValueError):
        b.move_obstacles(np.zeros((5, 3)))
    A, bb = b.obstacles()
    assert E.same(A[:5], np.asarray(park["A"], float)) and E.same(bb[:5], np.asarray(park["b"], float))
    b.close()
