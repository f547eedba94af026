"""Closed-loop ensemble (obca_amd/csrc/obca_ensemble.h): the kernel text compiled for the host (tests/emu/ensemble_emu.cpp) against the numpy statement
(obca_amd/validate.py: with a zero bias every member IS validate.track_parking / track_quad with that member's offset), on the fixture's trajectories and on horizons cut to
N = 1 and N = 3; the reduction rules on a hand-made member table; isolation of bad members and bad instances; the input bias; refusals, the public surface, the build rule
and the Julia shim.  No GPU.  Cases, comparison rules and tolerances: tests/ensemble_common.py."""
import ctypes as C
import inspect
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import rollout_common as R
import track_common as T
import ensemble_common as E
from obca_amd import validate as V

WORST = {}


# ---------------------------------------------------------------- 1. the host build against the statement
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_host_build_matches_numpy(case):
    """real fields within 3.1e-10 max(1, |value|) (track_common.TOL_HOST), index and count fields equal; the numpy side is asserted to be separated first"""
    kind = case[0]; c, S_, M, dx0, need = E.case_inputs(case)
    emu, ref, tref = (E.emu_parking, E.ref_parking, T.ref_parking) if kind == "parking" else (E.emu_quad, E.ref_quad, T.ref_quad)
    want = ref(c, S_, M, dx0, need=need)
    assert E.separated(want, need), case
    assert (want[1][:, 0] == 0).all() and want[0][0] == 0 and want[0][5] == 0 and 0 < want[0][6] and (M == 1 or want[0][6] < M), want[0]
    assert np.array_equal(dx0[0], np.zeros(dx0.shape[1])) and want[1][0, 14] == 0      # member 0 is the nominal closed loop
    got = emu(c, S_, M, dx0, need=need)
    WORST[kind] = max(WORST.get(kind, 0.0), E.worst(got, want))
    print("largest difference host build - numpy so far:", WORST)
    E.check(got, want, E.TOL_HOST, E.case_id(case))
    assert got[0][:5].tolist() == [0, M, S_, 1, 1] and got[0][26:].tolist() == [0] * 6
    # the yardstick itself, spelled out for the first and the last member: the record of validate.track_* with that member's offset
    for m in sorted({0, M - 1}):
        t = tref(c, S_, 1, 1, dx0[m], need=need)[0]
        assert R.close(got[1][m, E.MEM_REAL], t[[1, 6, 3, 4, 5, 16, 43, 45]], E.TOL_HOST), (case, m)
        assert np.array_equal(got[1][m, [0, 2, 8, 9, 10, 11, 13]], t[[0, 2, 18, 19, 20, 42, 44]]), (case, m)
        assert R.close(got[2][m], tref(c, S_, 1, 1, dx0[m], need=need)[1][:, -1], E.TOL_HOST)
    back = emu(c, S_, M, dx0, need=need, rev=1)      # the lane order of the linearisation gives the same bits
    assert all(np.array_equal(a, b) for a, b in zip(got, back))


def test_members_share_nothing():
    """member m of an ensemble of 64 is, bit for bit, member 0 of an ensemble of one with the same offset: lanes share the gains and nothing else"""
    for kind, emu in (("parking", E.emu_parking), ("quad", E.emu_quad)):
        case = [k for k in E.CASES if k[0] == kind and k[4] == 64][0]; c, S_, M, dx0, need = E.case_inputs(case)
        all_ = emu(c, S_, M, dx0, need=need)
        for m in (0, 1, 37, 63):
            one = emu(c, S_, 1, dx0[m:m + 1], need=need)
            assert np.array_equal(one[1][0], all_[1][m]) and np.array_equal(one[2][0], all_[2][m]), (kind, m)


# ---------------------------------------------------------------- 2. the reduction rules
def _member(**kw):
    r = np.array([0, 0.5, 7, 0.2, 0.1, 0.3, 0.0, 0.4, 11, 1, 0, 0, 0.05, 3, 0.1, 0], float)
    for k, v in kw.items():
        r[dict(bad=0, dev_pos=1, dev_node=2, end_pos=3, dev_att=4, dev_vel=5, dev_rate=6, min=7, sample=8, obst=9, below=10, sat=11, du=12, du_node=13)[k]] = v
    return r


BAD_MEMBER = np.array([1, np.nan, -1, np.nan, np.nan, np.nan, np.nan, np.nan, -1, -1, -1, -1, np.nan, -1, np.nan, 0])


def test_reduction_rules_on_a_hand_made_table():
    mem = np.stack([_member(), _member(min=0.3, sample=5, obst=2, below=2, dev_pos=0.9, dev_node=4), BAD_MEMBER, _member(min=0.3, sample=9, obst=0, below=1, dev_pos=0.9, dev_node=8, sat=3),
                    _member(end_pos=0.7, du=0.25, du_node=6, dev_att=0.6), _member(end_pos=0.7, du=0.25, du_node=2, dev_vel=0.8, dev_rate=0.05)])
    out = E.emu_reduce(mem, 4, 1, 0, 0)
    assert np.array_equal(out, V.ensemble_record(mem, 4, 1, 0, True), equal_nan=True)
    assert out[:8].tolist() == [0, 6, 4, 1, 0, 1, 2, 1]                              # one bad; members 1 and 3 have samples under need; member 3 saturated
    assert out[8:12].tolist() == [0.3, 1, 5, 2]                                      # the tie of the minimum goes to member 1, not 3
    assert out[12:17].tolist() == [0.9, 1, 4, 0.7, 4]                                # dev_pos: member 1 before 3; end_pos: member 4 before 5
    assert out[17:23].tolist() == [0.6, 0.8, 0.05, 0.25, 4, 6] and out[25] == 3      # du_max: member 4 before 5
    good = [0, 1, 3, 4, 5]; se = sm = 0.0
    for m in good:
        se += mem[m, 3]; sm += mem[m, 7]
    assert out[23] == se / 5 and out[24] == sm / 5 and out[26:].tolist() == [0] * 6  # the bad member enters no mean
    # every member bad, the instance not
    allbad = np.stack([BAD_MEMBER] * 3); out = E.emu_reduce(allbad, 2, 0, 1, 0)
    exp = np.r_[0, 3, 2, 0, 1, 3, 0, 0, np.nan, -1, -1, -1, np.nan, -1, -1, np.nan, -1, np.nan, np.nan, np.nan, np.nan, -1, -1, np.nan, np.nan, 0, np.zeros(6)]
    assert np.array_equal(out, exp, equal_nan=True) and np.array_equal(V.ensemble_record(allbad, 2, 0, 1, True), exp, equal_nan=True)
    # the instance bad
    out = E.emu_reduce(allbad, 2, 1, 1, 1)
    exp = np.r_[1, 3, 2, 1, 1, -1, -1, -1, np.nan, -1, -1, -1, np.nan, -1, -1, np.nan, -1, np.nan, np.nan, np.nan, np.nan, -1, -1, np.nan, np.nan, -1, np.zeros(6)]
    assert np.array_equal(out, exp, equal_nan=True) and np.array_equal(V.ensemble_record(allbad, 2, 1, 1, False), exp, equal_nan=True)
    one = E.emu_reduce(_member()[None], 1, 1, 1, 0)      # a single member is its own minimum, maximum and mean
    assert one[[8, 9, 12, 13, 15, 16, 20, 21, 23, 24]].tolist() == [0.4, 0, 0.5, 0, 0.2, 0, 0.05, 0, 0.2, 0.4]


# ---------------------------------------------------------------- 3. isolation
def test_a_bad_offset_marks_its_member_alone():
    for kind, emu, ref in (("parking", E.emu_parking, E.ref_parking), ("quad", E.emu_quad, E.ref_quad)):
        case = [k for k in E.CASES if k[0] == kind and k[4] == 64 and k[2] > 3][0]; c, S_, M, dx0, need = E.case_inputs(case)
        good = emu(c, S_, M, dx0, need=need)
        d = dx0.copy(); d[5, 2] = np.nan; b = np.zeros((M, 2 if kind == "parking" else 4)); b[40, 1] = np.inf
        got = emu(c, S_, M, d, b, need=need)
        for m in range(M):
            if m in (5, 40):
                assert np.array_equal(got[1][m], BAD_MEMBER, equal_nan=True) and np.isnan(got[2][m]).all(), (kind, m)
            else:
                assert np.array_equal(got[1][m], good[1][m]) and np.array_equal(got[2][m], good[2][m]), (kind, m)
        assert got[0][0] == 0 and got[0][5] == 2
        assert np.array_equal(got[0], V.ensemble_record(got[1], S_, 1, 1, True), equal_nan=True)      # the bad members enter no extremum and no mean
        small = [0, 5, 40]; want = ref(c, S_, 3, d[small], b[small], need=need); sub = emu(c, S_, 3, d[small], b[small], need=need)
        E.check(sub, want, E.TOL_HOST, kind + " with bad members")


def assert_instance_bad(got, M, S_, fb, cl):
    exp = np.r_[1, M, S_, fb, cl, -1, -1, -1, np.nan, -1, -1, -1, np.nan, -1, -1, np.nan, -1, np.nan, np.nan, np.nan, np.nan, -1, -1, np.nan, np.nan, -1, np.zeros(6)]
    assert np.array_equal(got[0], exp, equal_nan=True), got[0]
    assert all(np.array_equal(r, BAD_MEMBER, equal_nan=True) for r in got[1]) and np.isnan(got[2]).all()


def test_a_bad_trajectory_marks_its_instance_and_no_other():
    q = R.golden_quad(); dq = E.offsets(3, E.SIGMA_QUAD, 1); good = [E.emu_quad(c, 2, 3, dq) for c in q]
    u = np.array(q[1]["u"]); u[1, 3] = np.nan
    assert_instance_bad(E.emu_quad(dict(q[1], u=u), 2, 3, dq), 3, 2, 1, 1)
    want = E.ref_quad(dict(q[1], u=u), 2, 3, dq)
    assert np.array_equal(want[0], E.emu_quad(dict(q[1], u=u), 2, 3, dq)[0], equal_nan=True)
    xn = np.array(q[1]["x"]); xn[0, 20] = np.inf      # the last node enters no gain: the scan finds it
    assert_instance_bad(E.emu_quad(dict(q[1], x=xn), 2, 3, dq, fb=0, cl=0), 3, 2, 0, 0)
    assert_instance_bad(E.emu_quad(dict(q[2], ts=np.full(21, np.nan)), 1, 64), 64, 1, 1, 1)
    for c, g in zip(q, good):      # (instances share nothing: the neighbours come back bit for bit)
        assert all(np.array_equal(a, b) for a, b in zip(E.emu_quad(c, 2, 3, dq), g))
    p = R.golden_parking(); dp_ = E.offsets(3, E.SIGMA_PARK, 1); good = [E.emu_parking(c, 2, 3, dp_) for c in p]
    u = np.array(p[2]["u"]); u[0, 29] = np.nan
    assert_instance_bad(E.emu_parking(dict(p[2], u=u), 2, 3, dp_), 3, 2, 1, 1)
    assert_instance_bad(E.emu_parking(dict(p[0], Ts=np.nan), 1, 1, fb=0), 1, 1, 0, 1)
    assert np.array_equal(E.ref_parking(dict(p[0], Ts=np.nan), 1, 1, fb=0)[0], E.emu_parking(dict(p[0], Ts=np.nan), 1, 1, fb=0)[0], equal_nan=True)
    for c, g in zip(p, good):
        assert all(np.array_equal(a, b) for a, b in zip(E.emu_parking(c, 2, 3, dp_), g))


def test_a_quadcopter_member_across_the_pole_is_bad_alone():
    """feedback off, member 1 with a pitch rate of 3 rad/s: cos x[3] changes sign within a step; its neighbours are untouched"""
    c = R.golden_quad()[0]; dx0 = np.zeros((3, 12)); dx0[1, 9] = 3.0; dx0[2, 0] = 0.05
    got = E.emu_quad(c, 8, 3, dx0, fb=0, cl=0); want = E.ref_quad(c, 8, 3, dx0, fb=0, cl=0)
    assert got[1][:, 0].tolist() == [0, 1, 0] and np.array_equal(got[1][1], BAD_MEMBER, equal_nan=True) and np.isnan(got[2][1]).all() and got[0][0] == 0 and got[0][5] == 1
    X, _, info = V.track_quad(c["x"], c["u"], c["ts"], c["Ts"], 8, dx0[1], feedback=False, clamp=False)
    assert not info["finite"] and np.isfinite(dx0).all()
    E.check(got, want, E.TOL_HOST, "pole")
    alone = E.emu_quad(c, 8, 2, dx0[[0, 2]], fb=0, cl=0)
    assert np.array_equal(alone[1], got[1][[0, 2]]) and np.array_equal(alone[2], got[2][[0, 2]])


# ---------------------------------------------------------------- 4. the input bias
def test_a_bias_beyond_the_box_sits_on_the_bound():
    """clamp on, feedback off (the commanded input is u_k, inside the box), dub = +2 / -2 on every input: the applied input is the upper / lower bound in every interval"""
    for kind, emu, cases, lo, hi, roll in (("parking", E.emu_parking, R.golden_parking(), np.array([-0.6, -0.4]), np.array([0.6, 0.4]), None), ("quad", E.emu_quad, R.golden_quad(), np.full(4, 1.2), np.full(4, 7.8), None)):
        c = E.cut(cases[0], 3); N = 3; nu = len(lo); dub = np.stack([np.full(nu, 9.0), np.full(nu, -9.0), np.zeros(nu)])
        got = emu(c, 2, 3, None, dub, fb=0, cl=1)
        assert got[1][:, 0].tolist() == [0, 0, 0] and got[1][:, 11].tolist() == [N, N, 0], got[1]
        for m, bound in ((0, hi), (1, lo)):
            dist = np.abs(bound[:, None] - c["u"]).max(axis=0)
            assert got[1][m, 12] == dist.max() and got[1][m, 13] == int(np.argmax(dist)), (kind, m)
            ub = np.repeat(bound[:, None], N, axis=1)      # the same plant with the bound as its input, open loop
            Xb = (V.rollout_parking(c["x"], ub, c["ts"], c["Ts"], c["L"], 2)[0] if kind == "parking" else V.rollout_quad(c["x"], ub, c["ts"], c["Ts"], 2)[0])
            assert R.close(got[2][m], Xb[:, -1], E.TOL_HOST), (kind, m)
        assert got[0][7] == 2 and got[0][20] == got[1][:2, 12].max()
    # a bias inside the box, the loop closed: the restated numpy chain
    for kind, emu, ref, cases, dub in (("parking", E.emu_parking, E.ref_parking, R.golden_parking(), np.array([[0.0, 0.0], [0.05, -0.03], [-0.2, 0.1]])),
                                       ("quad", E.emu_quad, E.ref_quad, R.golden_quad(), np.array([np.zeros(4), [0.02, -0.02, 0.01, 0.0], [-0.03, 0.02, 0.02, -0.01]]))):
        for c, S_ in ((cases[1], 2), (E.cut(cases[0], 3), 1)):
            dx0 = E.offsets(3, E.SIGMA_PARK if kind == "parking" else E.SIGMA_QUAD, 3)
            for cl in (1, 0):
                got = emu(c, S_, 3, dx0, dub, cl=cl); want = ref(c, S_, 3, dx0, dub, cl=cl)
                assert np.array_equal(got[1][:, 0], want[1][:, 0]) and (got[1][:, 0] == 0).all() and got[1][1, 12] > 0, (kind, S_, cl, got[1][:, 0], want[1][:, 0])
                WORST[kind] = max(WORST.get(kind, 0.0), E.worst(got, want))
                assert R.close(got[1][:, E.MEM_REAL], want[1][:, E.MEM_REAL], E.TOL_HOST) and R.close(got[2], want[2], E.TOL_HOST), (kind, S_, cl)
                assert np.array_equal(got[1][:, [0, 11, 15]], want[1][:, [0, 11, 15]])
    print("largest difference host build - numpy so far:", WORST)


def test_without_feedback_clamp_offset_and_bias_every_member_is_the_chain_rollout():
    for kind, emu, cases in (("parking", E.emu_parking, R.golden_parking()), ("quad", E.emu_quad, R.golden_quad())):
        for c in cases[:2]:
            for S_ in (1, 2):
                got = emu(c, S_, 3, None, None, fb=0, cl=0)
                ro = (R.ref_parking(c, S_, 0, V.DMIN) if kind == "parking" else R.ref_quad(c, S_, 0, 0.0)); rec, X = ro[0], ro[1]
                for m in range(3):
                    r = got[1][m]
                    assert R.close(r[[1, 3, 4, 5, 6, 7]], rec[[1, 6, 3, 4, 5, 16]], E.TOL_HOST) and r[[0, 2, 8, 9, 10]].tolist() == rec[[0, 2, 18, 19, 20]].tolist(), (kind, S_, m)
                    assert r[11:].tolist() == [0, 0, 0, 0, 0] and R.close(got[2][m], X[:, -1], E.TOL_HOST)
                    assert np.array_equal(r, got[1][0])      # equal inputs, equal bits in every lane


# ---------------------------------------------------------------- 5. refusals
def test_argument_errors():
    lib = E.emu(); out = np.zeros(32); w = np.zeros(4096); z = np.zeros(8192); prob = np.zeros(4096); dp = E.dp
    q4, r2, q12, r4 = np.ones(4), np.ones(2), np.ones(12), np.ones(4)

    def park(S_=8, M=3, fb=1, cl=1, r=r2, need=0.05, N=30):
        return lib.emu_ensemble_parking(N, dp(prob), dp(z), None, 2, S_, M, fb, cl, dp(q4), E._opt(r), dp(q4), None, None, need, 0, dp(w), dp(w), dp(out))

    def quad(S_=8, M=3, fb=1, cl=1, r=r4, need=0.0, N=5):
        return lib.emu_ensemble_quad(N, dp(prob), dp(z), dp(z), dp(z), 1, S_, M, fb, cl, dp(q12), E._opt(r), dp(q12), None, None, need, 0, dp(w), dp(w), dp(out))
    cases = [(dict(M=0), b"need 1 <= members <= 64"), (dict(M=65), b"need 1 <= members <= 64"), (dict(M=-1), b"need 1 <= members <= 64"),
             (dict(S_=0), b"need 1 <= substeps <= 32"), (dict(S_=33), b"need 1 <= substeps <= 32"), (dict(need=np.nan), b"need a finite `need`"),
             (dict(fb=2), b"feedback must be 0 (open loop) or 1"), (dict(cl=2), b"clamp must be 0 or 1"), (dict(r=None), b"must not be NULL")]
    for kw, msg in cases:
        assert park(**kw) == -1 and msg in lib.emu_ensemble_last_error(), kw
        assert quad(**kw) == -1 and msg in lib.emu_ensemble_last_error(), kw
    assert park(r=np.array([1.0, 0.0])) == -1 and b"r needs finite entries > 0" in lib.emu_ensemble_last_error()
    for N in (0, 129):
        assert park(N=N) == -1 and quad(N=N) == -1
    assert (out == 0).all()
    assert lib.emu_ensemble_reduce(0, 1, 1, 1, 0, dp(w), dp(out)) == -1 and lib.emu_ensemble_reduce(65, 1, 1, 1, 0, dp(w), dp(out)) == -1
    with pytest.raises(ValueError, match="members"):
        V.ensemble_quad(np.zeros((12, 3)), np.zeros((4, 2)), 1.0, 0.1, 65)
    # the library's own refusals: one text per cause and entry point
    hip = open(os.path.join(ROOT, "obca_amd", "csrc", "obca_hip.hip")).read()
    for e, dims in (("obca_batch_ensemble", "4"), ("obca_quad_batch_ensemble", "QX")):
        assert '"%s: NULL argument"' % e in hip and '"%s: nothing has been solved since the last upload or shift"' % e in hip
        assert '"%s_ms: no ensemble call has run on this batch"' % e in hip
        assert 'ensemble_fetch(bt, %s, false, mem, "%s_members")' % (dims, e) in hip and 'ensemble_fetch(bt, %s, true, fin, "%s_final")' % (dims, e) in hip
    assert '": no ensemble call has run on this batch since it was last filled"' in hip
    assert '"obca_parking_ensemble_batch: need B>=1, 1<=N<=OBCA_NMAX"' in hip and '"obca_quadcopter_ensemble_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"' in hip
    assert hip.count("ens::ensemble_check_args(substeps, members, feedback, clamp, q, r, qf, ") == 4
    # a NULL batch is refused with no device touched
    from obca_amd import api
    lib = api._load(); f = C.c_float(0); q, r = np.ones(12), np.ones(4)
    assert lib.obca_batch_ensemble(None, 8, 3, 1, 1, q[:4], r[:2], q[:4], None, None, 0.05, np.zeros(32)) == -1
    assert lib.obca_quad_batch_ensemble(None, 8, 3, 1, 1, q, r, q, None, None, 0.0, np.zeros(32)) == -1
    assert lib.obca_batch_ensemble_ms(None, C.byref(f)) == -1 and lib.obca_quad_batch_ensemble_ms(None, C.byref(f)) == -1
    assert lib.obca_batch_ensemble_members(None, np.zeros(1)) == -1 and lib.obca_quad_batch_ensemble_final(None, np.zeros(1)) == -1
    assert lib.obca_batch_ensemble_final(None, np.zeros(1)) == -1 and lib.obca_quad_batch_ensemble_members(None, np.zeros(1)) == -1
    with pytest.raises((TypeError, C.ArgumentError)):      # out as int32
        lib.obca_batch_ensemble(None, 8, 3, 1, 1, q[:4], r[:2], q[:4], None, None, 0.05, np.zeros(32, np.int32))


# ---------------------------------------------------------------- 6. the public surface, the build rule, the Julia shim
FORBIDDEN = ("track", "rollout", "plan", "refine", "hybrid", "scene", "subdivide", "clearance", "path_ws", "start_download")


def test_header_exports_python_and_julia_agree():
    import obca_amd
    from obca_amd import api, cabi, planner as PL
    import test_hybrid_cpu as TH
    import test_julia_shim_cpu as J
    protos = cabi.prototypes("obca_ensemble.h")
    assert sorted(protos) == sorted(api.ENSEMBLE_EXPORTS) and len(protos) == 10 and "obca_ensemble.h" in cabi.__doc__
    others = (set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS) | set(api.REFINE_EXPORTS) | set(api.QUAD_SUBDIVIDE_EXPORTS) | set(api.PLAN_DEVICE_EXPORTS)
              | set(api.SCENE_EXPORTS) | set(api.PLAN_RESIDENT_EXPORTS) | set(api.PLAN_RESIDENT_CHECK_EXPORTS) | set(api.QUAD_PLAN_RESIDENT_EXPORTS) | set(api.ROLLOUT_EXPORTS)
              | set(api.TRACK_EXPORTS) | set(PL.PLAN3D_EXPORTS))
    assert not set(api.ENSEMBLE_EXPORTS) & others
    assert not any(set(protos) & set(cabi.prototypes(h)) for h in ("obca_hip.h", "obca_rollout.h", "obca_track.h"))
    assert [len(protos[n][1]) for n in api.ENSEMBLE_EXPORTS] == [12, 2, 2, 2, 26, 12, 2, 2, 2, 22]
    # no name of the header falls under a filter by which an older test picks ITS entry points out of the library's symbols
    assert not any(w in s for s in api.ENSEMBLE_EXPORTS for w in FORBIDDEN)
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {s for s in exported if "ensemble" in s} == set(api.ENSEMBLE_EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "obca_ensemble.h")).read()
    assert re.search(r"#define OBCA_ENS_MEM 16\b", hdr) and re.search(r"#define OBCA_ENS_OUT 32\b", hdr) and re.search(r"#define OBCA_ENS_MMAX 64\b", hdr)
    txt = open(os.path.join(ROOT, "obca_amd", "csrc", "obca_ensemble.h")).read()
    assert re.search(r"#define EN_MEM 16\b", txt) and re.search(r"#define EN_OUT 32\b", txt) and re.search(r"#define EN_MMAX 64\b", txt)
    assert (V.ENS_MEM, V.ENS_OUT, V.ENS_MMAX) == (16, 32, 64)
    for f_ in ("parking_ensemble_batch", "quadcopter_ensemble_batch", "ensemble_offsets"):
        assert hasattr(obca_amd, f_) and f_ in obca_amd.__all__
    for cls, need in ((obca_amd.Batch, V.DMIN), (obca_amd.QuadBatch, 0.0)):
        sig = inspect.signature(cls.ensemble).parameters
        assert list(sig) == ["self", "members", "substeps", "dx0", "dub", "Q", "R", "Qf", "feedback", "clamp", "need"]
        assert [sig[n].default for n in list(sig)[1:]] == [64, 8, None, None, None, None, None, True, True, need]
        assert all(callable(getattr(cls, m)) for m in ("ensemble_members", "ensemble_final", "ensemble_ms")) and "ensemble_members" in vars(api._DeviceBatch)
    for fn in (obca_amd.parking_ensemble_batch, obca_amd.quadcopter_ensemble_batch):
        sig = inspect.signature(fn).parameters
        assert sig["members"].default == 64 and sig["substeps"].default == 8 and sig["dx0"].default is None and sig["dub"].default is None
    # ensemble_offsets: numpy only, seeded, member 0 exactly zero, the stated spread
    sig = inspect.signature(obca_amd.ensemble_offsets).parameters
    assert list(sig) == ["B", "M", "sigma", "seed"] and sig["seed"].default == 0
    d = obca_amd.ensemble_offsets(50, 64, [0.1, 0.0, 2.0], seed=3)
    assert d.shape == (50, 64, 3) and (d[:, 0] == 0).all() and (d[:, :, 1] == 0).all() and np.array_equal(d, obca_amd.ensemble_offsets(50, 64, [0.1, 0.0, 2.0], 3))
    assert not np.array_equal(d, obca_amd.ensemble_offsets(50, 64, [0.1, 0.0, 2.0], 4))
    s = d[:, 1:].reshape(-1, 3).std(axis=0)      # 3150 draws: the sample deviation lies within 5 % of sigma (4 standard errors are 5 %)
    assert abs(s[0] - 0.1) < 0.005 and abs(s[2] - 2.0) < 0.1
    src_fn = inspect.getsource(api.ensemble_offsets)
    assert "torch" not in src_fn and "_load" not in src_fn
    # every ccall of the shim against the header, parameter by parameter; a library constant of its own
    kinds = TH._kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCAEnsemble.jl")).read()
    assert re.search(r"^const ENS = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), ENS\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
        assert m.group(2) == "Cint"
    assert {n for n, _ in calls} == set(kinds) == set(api.ENSEMBLE_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])
    assert src.count("ccall(") == len(calls) + 1 and "ccall((:obca_last_error, LIB)" in src


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu"); name = "ensemble_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_ensemble_emu.so")
    deps = {os.path.realpath(d) for d in BF.dependencies(p.sources)}
    todo = [os.path.realpath(s) for s in p.sources]; seen = set()
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        assert f in deps, f
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', open(f).read(), flags=re.M):
            assert os.path.exists(os.path.join(os.path.dirname(f), inc)), (f, inc)
            todo.append(os.path.realpath(os.path.join(os.path.dirname(f), inc)))
    csrc = os.path.join(ROOT, "obca_amd", "csrc")
    for h in ("obca_ensemble.h", "obca_track.h", "obca_rollout.h", "obca_clearance.h", "obca_quad_model.h", "obca_model.h"):
        assert os.path.realpath(os.path.join(csrc, h)) in seen, h
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_ensemble_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/ensemble_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # nothing in csrc includes the kernel text but the one line of the library, behind the track call's; the text includes nothing itself
    for f in os.listdir(csrc):
        if f.endswith((".h", ".hip", ".cpp")) and f != "obca_hip.hip":
            assert not re.search(r'#\s*include\s*"obca_ensemble.h"', open(os.path.join(csrc, f)).read()), f
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    assert hip.count('#include "obca_ensemble.h"') == 1 and '#include "obca_track.h"\n#include "obca_ensemble.h"' in hip
    raw = open(os.path.join(csrc, "obca_ensemble.h")).read(); txt = re.sub(r"//.*", "", raw)
    assert "#include" not in txt and '#error "include the track call' in raw
    # the loop bounds are known at launch: no while, no early exit out of a loop, no atomics; the gains are the track call's own functions
    assert not re.search(r"\bwhile\b|\bbreak\b|\bgoto\b|atomic", txt)
    assert txt.count("linearise<") == 2 and txt.count("riccati<") == 2 and "rk4_step<M>" in txt and "dualws_one<VM>" in txt and "InputBox<M>" in txt
