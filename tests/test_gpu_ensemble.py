"""Closed-loop ensemble on the device (include/obca_ensemble.h) against the host build of the same kernel text (tests/emu/ensemble_emu.cpp) on the cases of
tests/test_ensemble_cpu.py; against the device's own track call, member by member; the resident calls after a solve; more instances than one chunk and more workgroups than
CUs with all 64 lanes live; bad members, bad instances and the refusals.  Cases, comparison rules and tolerances: tests/ensemble_common.py.  The largest differences seen
are printed (tools/ensemble_rate.py copies them into its profile)."""
import json
import os
import numpy as np
import pytest
import rollout_common as R
import ensemble_common as E
from obca_amd import scenarios as S, validate as V
from test_gpu_rollout import upload_parking

pytestmark = pytest.mark.gpu
WORST = {}
INT = dict(members=1, substeps=2, members_bad=5, members_hit=6, members_sat=7, min_member=9, min_sample=10, min_obstacle=11, dev_pos_member=13, dev_node=14, end_pos_member=16,
           du_member=21, du_node=22, below=25)
REAL = dict(min=8, dev_pos=12, end_pos=15, dev_att=17, dev_vel=18, dev_rate=19, du_max=20, end_pos_mean=23, min_mean=24)


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.build_library()
    return obca_amd


def record(r, i):
    """row i of a returned dict, back in the layout of the C record"""
    out = np.zeros(V.ENS_OUT); out[0] = 0.0 if r["finite"][i] else 1.0; out[3] = r["feedback"][i]; out[4] = r["clamp"][i]
    for k, j in {**INT, **REAL}.items():
        out[j] = r[k][i]
    return out


def dev(r, i):
    return record(r, i), r["member_records"][i], r["final"][i]


def quad_call(OA, cases, S_, M, dx0=None, dub=None, fb=True, cl=True, need=0.0, **kw):
    return OA.quadcopter_ensemble_batch(np.stack([c["x"] for c in cases]), np.stack([c["u"] for c in cases]), np.stack([c["ts"] for c in cases]), [c["Ts"] for c in cases],
                                        cases[0]["ob"], cases[0]["R"], M, S_, dx0, dub, feedback=fb, clamp=cl, need=need, **kw)


def parking_call(OA, cases, S_, M, dx0=None, dub=None, fb=True, cl=True, need=V.DMIN, **kw):
    c0 = cases[0]
    return OA.parking_ensemble_batch(c0["N"], [c["Ts"] for c in cases], c0["L"], c0["ego"], [c["vOb"] for c in cases], [c["A"] for c in cases], [c["b"] for c in cases],
                                     np.stack([c["x"] for c in cases]), np.stack([c["u"] for c in cases]), np.stack([c["ts"] for c in cases]), M, S_, dx0, dub, feedback=fb, clamp=cl,
                                     need=need, **kw)


def calls(kind):
    return (parking_call, E.emu_parking) if kind == "parking" else (quad_call, E.emu_quad)


# ---------------------------------------------------------------- 1. host-pointer entries against the host build
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_host_pointer_call_matches_the_host_build(OA, case):
    """the inputs of tests/test_ensemble_cpu.py (its numpy side asserts that they are separated): real fields within 1e-9 max(1, |value|), index and count fields equal"""
    kind = case[0]; c, S_, M, dx0, need = E.case_inputs(case); call, emu = calls(kind)
    if kind == "quad" and c["N"] < 2:      # the quadcopter's host-pointer calls need N >= 2, as its track call: the host build covers N = 1
        with pytest.raises(OA.ObcaError, match="2<=N<=OBCA_QUAD_NMAX"):
            call(OA, [c], S_, M, dx0, need=need)
        return
    r = call(OA, [c], S_, M, dx0, need=need)
    assert r["member_records"].shape == (1, M, 16) and r["final"].shape == (1, M, c["x"].shape[0]) and r["finite"].all() and r["members"][0] == M and r["substeps"][0] == S_
    host = emu(c, S_, M, dx0, need=need)
    key = kind + "_device_vs_host_build"; WORST[key] = max(WORST.get(key, 0.0), E.worst(dev(r, 0), host))
    print("largest difference device - host build so far:", WORST)
    E.check(dev(r, 0), host, E.TOL_DEV, E.case_id(case))


def test_a_bias_on_the_device_matches_the_host_build(OA):
    for kind, cases, dub in (("parking", R.golden_parking(), np.array([[0.0, 0.0], [0.05, -0.03], [9.0, -9.0]])), ("quad", R.golden_quad(), np.array([np.zeros(4), [0.02, -0.02, 0.01, 0.0], [9.0, 9.0, 9.0, 9.0]]))):
        call, emu = calls(kind); full = cases[1] if kind == "parking" else cases[0]; dx0 = E.offsets(3, E.SIGMA_PARK if kind == "parking" else E.SIGMA_QUAD, 3)
        for fb in (True, False):
            c = full if fb else E.cut(full, 3)      # (open loop the quadcopter is unstable: over the full horizon a biased member ends 200 m away and rounding grows with it)
            r = call(OA, [c], 2, 3, dx0, dub, fb=fb); host = emu(c, 2, 3, dx0, dub, fb=int(fb), need=V.DMIN if kind == "parking" else 0.0)
            key = kind + "_device_vs_host_build"; WORST[key] = max(WORST.get(key, 0.0), E.worst(dev(r, 0), host))
            got = dev(r, 0)
            assert R.close(got[1][:, E.MEM_REAL], host[1][:, E.MEM_REAL], E.TOL_DEV) and R.close(got[2], host[2], E.TOL_DEV) and np.array_equal(got[1][:, [0, 11, 15]], host[1][:, [0, 11, 15]]), (kind, fb)
            assert np.array_equal(got[0][[0, 1, 2, 3, 4, 5, 7]], host[0][[0, 1, 2, 3, 4, 5, 7]])
            if not fb:
                assert got[1][2, 0] == 0 and got[1][2, 11] == c["N"]      # the bias beyond the box: clipped in every interval


# ---------------------------------------------------------------- 2. against the device's own track call
@pytest.mark.parametrize("M", [3, 64])
def test_every_member_is_the_device_track_call_with_its_offset(OA, M):
    """member m against parking_track_batch / quadcopter_track_batch with dx0[m] (the trajectory tiled M times, one offset each): field by field within 1e-9, indices equal,
    the final state X[:, N] of that call.  Not bit-equality: which products the compiler fuses depends on where the operands come from (obca_track.h)."""
    for kind in ("parking", "quad"):
        case = [k for k in E.CASES if k[0] == kind and k[4] == M and k[2] > 3][0]; c, S_, _, dx0, need = E.case_inputs(case); call, _ = calls(kind)
        r = call(OA, [c], S_, M, dx0, need=need); mem, fin = r["member_records"][0], r["final"][0]
        tiled = [c] * M
        if kind == "parking":
            t = OA.parking_track_batch(c["N"], [c["Ts"]] * M, c["L"], c["ego"], [c["vOb"]] * M, [c["A"]] * M, [c["b"]] * M, np.stack([c["x"]] * M), np.stack([c["u"]] * M),
                                       np.stack([c["ts"]] * M), S_, dx0, need=need)
        else:
            t = OA.quadcopter_track_batch(np.stack([c["x"]] * M), np.stack([c["u"]] * M), np.stack([c["ts"]] * M), [c["Ts"]] * M, c["ob"], c["R"], S_, dx0, need=need)
        assert t["finite"].all() and len(tiled) == M
        real = np.stack([t["dev_pos"], t["end_pos"], t["dev_att"], t["dev_vel"], t["dev_rate"], t["clearance"]["min"], t["du_max"], t["dx0_pos"]], 1)
        idx = np.stack([np.zeros(M), t["dev_node"], t["clearance"]["sample"], t["clearance"]["obstacle"], t["clearance"]["below"], t["saturated"], t["du_node"]], 1)
        key = kind + "_ensemble_vs_device_track"; WORST[key] = max(WORST.get(key, 0.0), R.worst(mem[:, E.MEM_REAL], real), R.worst(fin, t["states"][:, -1]))
        assert R.close(mem[:, E.MEM_REAL], real, E.TOL_DEV), (kind, M)
        assert np.array_equal(mem[:, [0, 2, 8, 9, 10, 11, 13]], idx), (kind, M, mem[:, [0, 2, 8, 9, 10, 11, 13]], idx)
        assert R.close(fin, t["states"][:, -1], E.TOL_DEV), (kind, M)
    print("largest difference ensemble - device track so far:", WORST)


# ---------------------------------------------------------------- 3. resident
def resident_checks(OA, b, ctx, host_call, keys, nx, nu, sig):
    M = 5; dx0 = OA.ensemble_offsets(b.B, M, sig, seed=2); dub = OA.ensemble_offsets(b.B, M, np.full(nu, 0.01), seed=3)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.ensemble(M, 8)
    with pytest.raises(OA.ObcaError, match="no ensemble call has run"):
        b.ensemble_members()
    with pytest.raises(OA.ObcaError, match="no ensemble call has run"):
        b.ensemble_final()
    b.solve(); before = b.download()
    assert (before["exitflag"] == 1).any()
    b.rollout(8, False); Xr = b.rollout_states(); b.track(8); Xt = b.track_states(); Kt = b.track_gains()
    out = []
    for d, u in ((None, None), (dx0, dub), (dx0[0], None)):      # (the last: one table of offsets for every instance)
        r = b.ensemble(M, 8, d, u); mem = b.ensemble_members(); fin = b.ensemble_final()
        assert b.ensemble_ms() > 0 and mem.shape == (b.B, M, 16) and fin.shape == (b.B, M, nx)
        h = host_call(before, M, d, u); hm = h.pop("member_records"); hf = h.pop("final")
        for k in r:
            assert np.array_equal(r[k], h[k], equal_nan=True), (k, r[k], h[k])      # bit for bit: the same kernel on the same numbers
        assert np.array_equal(mem, hm, equal_nan=True) and np.array_equal(fin, hf, equal_nan=True)
        out.append((r, mem, fin))
    after = b.download()
    for k in keys:
        assert np.array_equal(before[k], after[k], equal_nan=True), k      # the iterate is read, nothing is written
    assert np.array_equal(b.rollout_states(), Xr, equal_nan=True) and np.array_equal(b.track_states(), Xt, equal_nan=True) and np.array_equal(b.track_gains(), Kt, equal_nan=True)
    ok = before["exitflag"] == 1; r0, mem0, _ = out[0]
    assert r0["finite"][ok].all() and (r0["members_bad"][ok] == 0).all()
    assert all(np.array_equal(mem0[i, m], mem0[i, 0]) for i in np.nonzero(ok)[0] for m in range(M))      # without offsets every lane carries the nominal closed loop
    # what another kernel left in LDS changes nothing
    from obca_amd import diag
    diag.leave_pattern(ctx, 4, 1e30)
    r2 = b.ensemble(M, 8, dx0, dub)
    assert all(np.array_equal(r2[k], out[1][0][k], equal_nan=True) for k in r2) and np.array_equal(b.ensemble_members(), out[1][1], equal_nan=True)
    for kw, msg in ((dict(members=0), "members"), (dict(members=65), "members"), (dict(substeps=0), "substeps"), (dict(need=np.nan), "finite `need`"), (dict(R=0.0), "r needs finite entries > 0")):
        with pytest.raises(OA.ObcaError, match=msg):
            b.ensemble(**kw)
    return before, out


def test_resident_quadcopter_ensemble(OA):
    B, N = 4, 20; bt = S.make_quad_batch(B, N); ctx = OA.Context(0)
    b = OA.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    resident_checks(OA, b, ctx, lambda o, M, d, u: OA.quadcopter_ensemble_batch(o["xp"], o["up"], o["timeScale"], bt["Ts"], bt["ob"], bt["R"], M, 8, d, u),
                    ("xp", "up", "timeScale", "exitflag", "lp", "slack", "info"), 12, 4, E.SIGMA_QUAD)
    b.close(); ctx.close()


def test_resident_parking_ensemble(OA):
    B, N = 8, 30; bt = S.make_batch(S.BACKWARDS, B, N); ctx = OA.Context(0)
    b = upload_parking(OA, ctx, bt)
    resident_checks(OA, b, ctx, lambda o, M, d, u: OA.parking_ensemble_batch(N, bt["Ts"], bt["L"], bt["ego"], bt["vOb"], bt["A"], bt["b"], o["xp"], o["up"], o["timeScale"], M, 8, d, u),
                    ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info"), 4, 2, E.SIGMA_PARK)
    b.close(); ctx.close()


# ---------------------------------------------------------------- 4. chunks, 5. lanes and rounds
def test_260_instances_of_64_members_over_chunks_and_rounds(OA, monkeypatch):
    """B = 260, M = 64: more workgroups than CUs, all lanes live -- the parking call in one chunk, the quadcopter call in chunks of 100 over the slots.  Every instance
    lands in its own rows of out, mem and fin and repeats the bits of the first instances; a NaN in a trajectory marks its instance alone, one in an offset its member"""
    p = R.golden_parking(); tiled = [p[i % 3] for i in range(260)]; dx0 = np.stack([E.offsets(64, E.SIGMA_PARK, i % 3) for i in range(260)])
    r = parking_call(OA, tiled, 2, 64, dx0)
    for i in range(3):
        host = E.emu_parking(p[i], 2, 64, dx0[i], need=V.DMIN)
        assert R.close(r["member_records"][i][:, E.MEM_REAL], host[1][:, E.MEM_REAL], E.TOL_DEV) and R.close(r["final"][i], host[2], E.TOL_DEV) and r["members_bad"][i] == 0
    for i in range(3, 260):
        assert np.array_equal(record(r, i), record(r, i % 3)) and np.array_equal(r["member_records"][i], r["member_records"][i % 3]) and np.array_equal(r["final"][i], r["final"][i % 3])
    monkeypatch.setenv("OBCA_CHUNK", "100")
    q = R.golden_quad(); tiled = [q[i % 4] for i in range(260)]; dx0 = np.stack([E.offsets(64, E.SIGMA_QUAD, i % 4) for i in range(260)])
    r = quad_call(OA, tiled, 2, 64, dx0)
    for i in range(4):
        host = E.emu_quad(q[i], 2, 64, dx0[i], need=0.0)
        assert R.close(r["member_records"][i][:, E.MEM_REAL], host[1][:, E.MEM_REAL], E.TOL_DEV) and R.close(r["final"][i], host[2], E.TOL_DEV) and r["members_bad"][i] == 0
    for i in range(4, 260):
        assert np.array_equal(record(r, i), record(r, i % 4)) and np.array_equal(r["member_records"][i], r["member_records"][i % 4]) and np.array_equal(r["final"][i], r["final"][i % 4])
    bad = [dict(c) for c in tiled]; bad[137] = dict(bad[137], u=bad[137]["u"].copy()); bad[137]["u"][2, 7] = np.nan
    d = dx0.copy(); d[201, 63, 4] = np.nan; d[0, 0, 0] = np.inf
    rb = quad_call(OA, bad, 2, 64, d)
    assert (~rb["finite"]).nonzero()[0].tolist() == [137] and np.isnan(rb["final"][137]).all() and (rb["member_records"][137][:, 0] == 1).all() and rb["members_bad"][137] == -1
    assert rb["members_bad"][201] == 1 and rb["members_bad"][0] == 1 and rb["member_records"][201][63, 0] == 1 and rb["member_records"][0][0, 0] == 1 and np.isnan(rb["final"][201][63]).all()
    assert np.array_equal(rb["member_records"][201][:63], r["member_records"][201][:63]) and np.array_equal(rb["member_records"][0][1:], r["member_records"][0][1:])
    assert np.array_equal(record(rb, 201), V.ensemble_record(rb["member_records"][201], 2, 1, 1, True), equal_nan=True)
    same = [i for i in range(260) if i not in (0, 137, 201)]
    assert all(np.array_equal(record(rb, i), record(r, i)) and np.array_equal(rb["member_records"][i], r["member_records"][i]) and np.array_equal(rb["final"][i], r["final"][i]) for i in same)


def test_refusals_of_the_host_pointer_calls(OA):
    q = R.golden_quad(); p = R.golden_parking()
    for kw, msg in ((dict(M=0), "need 1 <= members <= 64"), (dict(M=65), "need 1 <= members <= 64"), (dict(S_=0), "substeps"), (dict(need=np.inf), "finite `need`"),
                    (dict(fb=2), "feedback must be 0"), (dict(cl=-1), "clamp must be 0 or 1")):
        with pytest.raises(OA.ObcaError, match=msg):
            quad_call(OA, q, **{"S_": 8, "M": 3, **kw})
        with pytest.raises(OA.ObcaError, match=msg):
            parking_call(OA, p, **{"S_": 8, "M": 3, **kw})
    with pytest.raises(OA.ObcaError, match="dx0 must be"):
        quad_call(OA, q, 8, 3, np.zeros((2, 12)))
    t = quad_call(OA, q, 8, 3, member_records=False, final=False)
    assert "member_records" not in t and "final" not in t and t["finite"].all()


def test_largest_differences_are_on_record():
    """the figures tools/ensemble_rate.py copies into profiles/ensemble_device_vs_host.json (OBCA_ENSEMBLE_DIFFS names the file they are left in)"""
    print("device against host build / device track:", WORST)
    path = os.environ.get("OBCA_ENSEMBLE_DIFFS")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f)
