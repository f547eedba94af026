"""Clearance of a held plan against obstacles that move, without a GPU: the kernel text of obca_amd/csrc/obca_predict.h compiled for the host (tests/emu/predict_emu.cpp)
against the numpy statement (validate.predict_parking / predict_quad + predict_record: move_obstacles by rate * tau per sample, then measure) on solved trajectories in
scenes at both limits of the header and in every row class, in both dealing orders; zero rates against the clearance host build; the per-sample clearances against
polygons whose VERTICES were moved with plain numpy, through the exact distance of tests/polygon_distance.py; analytic cases; bad inputs; the public surface, the build
rule and the Julia shim.  tests/predict_common.py has the cases and the tolerances."""
import inspect
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import clearance_common as CK
import polygon_distance as PD
import predict_common as K
import scene_edit_common as E
from obca_amd import validate as V

TOL_D = 2e-8      # tests/test_dualws_geometry_cpu.py: the duality gap DualMultWS leaves, at every distance
NEED = V.DMIN


# ---------------------------------------------------------------- 1. host build against the statement
@pytest.mark.parametrize("N,S_", K.PARK_SHAPES)
def test_parking_record_and_profile_match_the_statement(N, S_):
    """(N, S) = (1, 1): the first interval alone, cum[0]; (2, 32), (30, 8), (128, 32): 65, 241 and 4 097 samples -- one more than a round of 64 lanes, the last sample with
    cum[N] and no interval behind it.  Scenes: 1 x 3 rows, 16 x 4 (both limits of the header), 8 + 3, 3 x 4 and the shipped 2 + 2 + 1: the row classes 4, 4, 8, 4 and 2.
    tau (t_first, t_min, horizon), indices and counts equal; clearances within 3.1e-10 max(1, |value|) (measured on x86-64: <= 5.4e-15); both dealing orders the same bits."""
    worst = {}; classes = set()
    for sc in range(len(K.scenes())):
        if N == 128 and sc in (0, 3):      # (the largest shape in the scenes at the limits and in the classes 2 and 8: the row class 4 is the 16 x 4 scene's)
            continue
        c = K.parking_case(N, sc, source=sc); rt = K.parking_rates(c, seed=sc); what = "N=%d S=%d scene %d" % (N, S_, sc)
        vm = int(c["vOb"].max()); classes.add(2 if vm <= 2 else 4 if vm <= 4 else 8)
        rec, prof = K.emu_parking(c, rt, S_, NEED)
        ref, rprof, table, tau = K.ref_parking(c, rt, S_, NEED)
        K.check_parking(rec, prof, ref, rprof, K.TOL_HOST, what, worst)
        assert rec[5] == N * S_ + 1 and rec[28] == tau[-1] and rec[29] == (len(c["vOb"]) - (len(c["vOb"]) > 1)) and (S_ > 1 or rec[0] == rec[1]), what
        rev, rprof2 = K.emu_parking(c, rt, S_, NEED, rev=1)
        assert K.same(rev, rec) and K.same(rprof2, prof), what
        if sc == 4:      # through the row class of a wider batch: the same record within the iteration's bound, the same indices
            wide, _ = K.emu_parking(c, rt, S_, NEED, vmax=8)
            K.check_parking(wide, None, rec, None, CK.TOL_PARK, what + " class 8")
        if N == 30:      # one t, as a resident batch holds it, is every stage's timeScale
            one = dict(c, ts=np.full(N + 1, c["ts"][0]))
            assert K.same(K.emu_parking(one, rt, S_, NEED, resident=True)[0], K.emu_parking(one, rt, S_, NEED)[0]), what
    print("parking host build against the statement, N=%d S=%d: %s" % (N, S_, worst))
    assert classes == {2, 4, 8}


@pytest.mark.parametrize("N,S_", K.QUAD_SHAPES)
def test_quadcopter_record_and_profile_match_the_statement_bit_for_bit(N, S_):
    for src in range(len(K.quad_sources())):
        c = K.quad_case(N, src); rt = K.quad_rates(src)
        for need in (0.0, 0.4):
            rec, prof = K.emu_quad(c, rt, S_, need); ref, rprof, _, tau = K.ref_quad(c, rt, S_, need)
            assert K.same(rec, ref) and K.same(prof, rprof), (N, S_, src, need, rec, ref)
            rev, rprof2 = K.emu_quad(c, rt, S_, need, rev=1)
            assert K.same(rev, rec) and K.same(rprof2, prof)
            assert rec[29] == 4 and rec[28] == tau[-1] and rec[5] == N * S_ + 1
        one = dict(c, ts=np.full(N + 1, c["ts"][0]))      # one t, as a resident batch holds it
        assert K.same(K.emu_quad(dict(one, ts=one["ts"][:1].copy()), rt, S_, tstride=0)[0], K.emu_quad(one, rt, S_)[0])


def test_times_are_summed_in_stage_order_and_reach_every_edge():
    """tau of the statement itself: cum[0] = 0 for the whole first interval, cum[N] for the last sample, the sub-step term on top of cum[k]"""
    ts = np.array([1.0, 0.5, 2.0, 7.0]); tau = V.predict_times(ts, 0.25, 3, 4)
    assert tau.shape == (13,) and tau[0] == 0.0 and tau[4] == 0.25 and tau[8] == 0.375 and tau[12] == 0.875      # (ts[3] belongs to no interval)
    assert tau[1] == (0.25 * 1.0) * 0.25 and tau[6] == (1.0 + 0.5 * 0.5) * 0.25 and tau[11] == (1.5 + 0.75 * 2.0) * 0.25 and (np.diff(tau) > 0).all()
    assert V.predict_times(1.0, 0.5, 1, 1).tolist() == [0.0, 0.5]
    # the record's times are these, bit for bit, in the host build too
    c = K.parking_case(5, 4); rt = K.parking_rates(c); rec, prof = K.emu_parking(c, rt, 3, 10.0)
    tau = V.predict_times(c["ts"], c["Ts"], 5, 3)
    assert rec[24] == 0 and rec[25] == 0.0 and rec[27] == tau[int(rec[2])] and rec[28] == tau[15] and rec[4] == 16


# ---------------------------------------------------------------- 2. all-zero rates: the clearance check
def test_zero_rates_are_the_clearance_record_bit_for_bit():
    seen = set()
    for N, S_, sc, need in ((5, 3, 1, 0.05), (30, 8, 4, 0.05), (30, 8, 4, 0.2), (30, 8, 2, 4.0), (2, 32, 0, 7.0)):
        c = K.parking_case(N, sc, source=sc); zero = np.zeros((len(c["vOb"]), 6)); zero[:, 3:5] = 2.5      # (a pivot alone moves nothing)
        for rev in (0, 1):
            rec, prof = K.emu_parking(c, zero, S_, need, rev=rev); clr = CK.emu_parking(c, S_, need)
            assert K.same(rec[:24], clr) and prof.min() == clr[0] and rec[29] == 0 and rec[30] == rec[31] == 0, (N, S_, sc)
            under = np.flatnonzero(prof < need); tau = V.predict_times(c["ts"], c["Ts"], N, S_)
            assert len(under) == clr[4] and rec[27] == tau[int(clr[2])] and rec[28] == tau[-1]
            seen.add(len(under) > 0)
            if len(under):
                assert rec[24] == under[0] and rec[25] == tau[under[0]] and rec[26] >= 0
            else:
                assert rec[24] == rec[26] == -1 and rec[25] == np.inf
    assert seen == {True, False}      # both: an instance with samples under `need` and one without
    for N, S_ in K.QUAD_SHAPES:
        c = K.quad_case(N, 2)
        for need in (0.0, 0.5):
            rec, prof = K.emu_quad(c, np.zeros((5, 4)), S_, need); clr = CK.emu_quad(c, S_, need)
            assert K.same(rec[:24], clr) and prof.min() == clr[0] and rec[29] == 0 and (prof < need).sum() == clr[4]


# ---------------------------------------------------------------- 3. against geometry that shares no code with the kernel
POLYGONS = (E.regular_polygon(3, (4.0, 12.5), 1.1, 0.3), E.regular_polygon(8, (-5.0, 13.0), 1.5, 0.1), E.box(1.3, 20.0, -5.0, 5.0), E.regular_polygon(5, (-3.0, 2.0), 0.8, 0.7))


@pytest.mark.parametrize("kind", ["translation", "rotation", "both about a pivot off the obstacle"])
def test_node_clearances_against_polygons_whose_vertices_were_moved(kind):
    """S = 1, one obstacle per instance: the profile IS the clearance of every node.  The polygon's vertices are moved to tau_k by p' = R(w tau)(p - c) + c + v tau with plain
    numpy; the exact distance of the car's rectangle to that polygon (tests/polygon_distance.py) agrees within 2e-8.  Sign, rotation sense, pivot and the time of every
    node are pinned by geometry.  (g is left out: an offset polygon is not the disc sum.)"""
    worst = 0.0; n = 0
    for i, V0 in enumerate(POLYGONS):
        A, b = E.polygon_hrep(V0); N = 30
        c = dict(K.parking_case(N, 0, source=i), vOb=np.array([len(b)], np.int32), A=A, b=b)
        centre = V0.mean(axis=0)
        v, w, piv = {"translation": ((0.07, -0.05), 0.0, (0.0, 0.0)), "rotation": ((0.0, 0.0), 0.04, tuple(centre)),
                     "both about a pivot off the obstacle": ((-0.04, 0.06), -0.03, tuple(centre + (3.0, -2.0)))}[kind]
        rt = np.array([[v[0], v[1], w, piv[0], piv[1], 0.0]])
        rec, prof = K.emu_parking(c, rt, 1, NEED); tau = V.predict_times(c["ts"], c["Ts"], N, 1)
        assert rec[6] == 0 and rec[29] == 1 and tau[-1] > 10
        for k in range(N + 1):
            A1, b1 = E.polygon_hrep(E.move_vertices(V0, np.asarray(v) * tau[k], w * tau[k], np.asarray(piv)))
            want = PD.polygon_distance(*c["x"][:3, k], c["ego"], A1, b1)
            if prof[k] == 0.0:
                assert want <= V.CLR_TOUCH + TOL_D, (kind, i, k, want)
            else:
                assert abs(prof[k] - want) <= TOL_D, (kind, i, k, prof[k], want)
                worst = max(worst, abs(prof[k] - want)); n += 1
    print("%s: %d node clearances, largest |host build - exact distance to the moved vertices| %.3g" % (kind, n, worst))
    assert n >= 60


# ---------------------------------------------------------------- 4. analytic cases
def _hover(N=30):
    ob = np.tile([-50.0, -50, -50, 51, 51, 51], (5, 1)); ob[2] = [5.0, 1.5, 1.5, -4.0, -0.5, -0.5]      # box 2: x in [4, 5], y, z in [0.5, 1.5]; the others far away
    x = np.zeros((12, N + 1)); x[:3] = np.array([1.0, 1.0, 1.0])[:, None]
    return dict(N=N, Ts=0.5, R=0.25, ob=ob, x=x, ts=1 + 0.1 * np.sin(np.arange(N + 1.0)))


def test_hovering_quadcopter_and_an_approaching_or_growing_box():
    c = _hover(); S_ = 4; tau = V.predict_times(c["ts"], c["Ts"], c["N"], S_); gap0 = 3.0
    for rate, speed in ((np.array([-0.2, 0, 0, 0.0]), 0.2), (np.array([0, 0, 0, 0.15]), 0.15), (np.array([-0.1, 0, 0, 0.05]), 0.15)):
        rt = np.zeros((5, 4)); rt[2] = rate; need = 1.0
        rec, prof = K.emu_quad(c, rt, S_, need)
        want = np.maximum(gap0 - speed * tau, 0.0) - c["R"]      # (the box reaches the point before the horizon ends: -R inside)
        assert np.abs(prof - want).max() <= 1e-12 and rec[29] == 1 and rec[3] == 2 and rec[2] == np.argmin(want) and abs(rec[0] - want.min()) <= 1e-12
        q = int(np.flatnonzero(want < need)[0])
        assert abs(want[q] - need) > 1e-9 and (rec[24], rec[25], rec[26]) == (q, tau[q], 2.0) and rec[4] == len(tau) - q and rec[27] == tau[np.argmin(want)] and rec[28] == tau[-1]
    rec, prof = K.emu_quad(c, np.zeros((5, 4)), S_, 1.0)
    assert (prof == gap0 - c["R"]).all() and rec[24] == -1 and rec[25] == np.inf and rec[2] == 0 and rec[27] == 0.0


def test_standing_car_and_an_approaching_or_growing_wall():
    N = 30; ego = np.array([3.7, 1.0, 1.0, 1.0]); A, b = E.polygon_hrep(E.box(6.0, 8.0, -5.0, 5.0)); gap0 = 6.0 - 3.7
    c = dict(N=N, Ts=1.0, L=2.7, ego=ego, vOb=np.array([4], np.int32), A=A, b=b, x=np.zeros((4, N + 1)), u=np.zeros((2, N)), ts=np.ones(N + 1))
    tau = V.predict_times(c["ts"], c["Ts"], N, 2)
    assert tau[-1] == 30.0
    for rate in ((-0.1, 0, 0, 0, 0, 0.0), (0, 0, 0, 0, 0, 0.1), (-0.06, 0, 0, 1.0, 2.0, 0.04)):
        need = 0.07      # (the samples are 0.05 apart in clearance: none lies at the bound)
        rec, prof = K.emu_parking(c, np.array([rate]), 2, need)
        want = np.maximum(gap0 - 0.1 * tau, 0.0)
        assert np.abs(prof - want).max() <= TOL_D and (prof[want == 0.0] == 0.0).all() and (want == 0.0).sum() >= 10, (rate, np.abs(prof - want).max())
        q = int(np.flatnonzero(want < need)[0])
        assert abs(want[q] - need) > 1e-6 and (rec[24], rec[25], rec[26]) == (q, tau[q], 0.0) and rec[0] == 0.0 and rec[1] == 0.0 and rec[29] == 1
        assert rec[2] == np.flatnonzero(prof == 0.0)[0] and rec[27] == tau[int(rec[2])]


# ---------------------------------------------------------------- 5. bad inputs
BAD_RECORD = np.r_[np.nan, np.nan, -1, -1, 0, 0, 1, 0, np.full(16, np.nan), -1, np.nan, -1, np.nan, np.nan, 0, 0, 0]


def assert_bad(rec, prof, nS):
    exp = BAD_RECORD.copy(); exp[4] = exp[5] = nS
    assert np.array_equal(rec, exp, equal_nan=True) and prof.shape == (nS,) and np.isnan(prof).all(), (rec, prof)


def test_bad_inputs_mark_their_instance_alone():
    N, S_ = 7, 4; nS = N * S_ + 1
    cases = [K.parking_case(N, sc, source=sc) for sc in (2, 3, 4)]; rates = [K.parking_rates(c, seed=i) for i, c in enumerate(cases)]
    good = [K.emu_parking(c, r, S_, NEED, vmax=8) for c, r in zip(cases, rates)]

    def neighbours_keep_their_bits():
        for c, r, g in zip(cases, rates, good):      # (instances share nothing: the others come back bit for bit)
            rec, prof = K.emu_parking(c, r, S_, NEED, vmax=8)
            assert K.same(rec, g[0]) and K.same(prof, g[1])
    c = cases[1]
    for col, val in ((0, np.nan), (2, np.inf), (4, np.nan), (5, -np.inf)):
        rt = rates[1].copy(); rt[2, col] = val
        for rev in (0, 1):
            assert_bad(*K.emu_parking(c, rt, S_, NEED, vmax=8, rev=rev), nS)
        ref, rprof, _, _ = K.ref_parking(c, rt, S_, NEED)
        assert_bad(ref, rprof, nS)
        neighbours_keep_their_bits()
    for field, idx, val in (("x", (0, 3), np.nan), ("x", (3, N), np.inf), ("u", (1, 2), np.inf), ("ts", (4,), np.nan), ("ts", (N,), np.nan)):
        a = np.array(c[field], float); a[idx] = val
        assert_bad(*K.emu_parking(dict(c, **{field: a}), rates[1], S_, NEED, vmax=8), nS)
        assert_bad(*K.ref_parking(dict(c, **{field: a}), rates[1], S_, NEED)[:2], nS)
    assert_bad(*K.emu_parking(dict(c, Ts=np.inf), rates[1], S_, NEED, vmax=8), nS)
    assert_bad(*K.ref_parking(dict(c, Ts=np.inf), rates[1], S_, NEED)[:2], nS)
    rt = rates[1].copy(); rt[0, 0] = 1.7e308; rt[0, 3] = 1.7e308      # finite rates, a moved row that is not
    assert_bad(*K.emu_parking(c, rt, S_, NEED, vmax=8), nS)
    assert_bad(*K.ref_parking(c, rt, S_, NEED)[:2], nS)
    neighbours_keep_their_bits()
    q = K.quad_case(7, 1); qr = K.quad_rates(1); qgood = K.emu_quad(q, qr, 4)
    for what in ("rate", "x", "ts", "Ts", "overflow"):
        qq = dict(q); rt = qr.copy()
        if what == "rate":
            rt[4, 3] = np.nan
        elif what == "overflow":
            rt[1, 0] = 1e308; qq["ts"] = q["ts"] * 100.0
        elif what == "Ts":
            qq["Ts"] = np.inf
        else:
            a = np.array(q[what], float); a[(1, 3) if what == "x" else (2,)] = np.nan; qq[what] = a
        assert_bad(*K.emu_quad(qq, rt, 4), 29)
        assert_bad(*K.ref_quad(qq, rt, 4)[:2], 29)
        assert K.same(K.emu_quad(q, qr, 4)[0], qgood[0])


def test_argument_errors():
    lib = K.emu(); out = np.zeros(32); z = np.zeros(4096); prob = np.zeros(4096)
    for S_, need, msg in ((0, 0.05, b"substeps"), (33, 0.05, b"substeps"), (8, np.nan, b"need"), (8, np.inf, b"need")):
        assert lib.emu_predict_parking(5, K.dp(prob), K.dp(z), None, K.dp(z), 2, S_, need, 0, K.dp(out), None) == -1 and msg in lib.emu_predict_last_error()
        assert lib.emu_predict_quad(5, K.dp(prob), K.dp(z), K.dp(z), 1, K.dp(z), S_, need, 0, K.dp(out), None) == -1 and msg in lib.emu_predict_last_error()
    assert lib.emu_predict_parking(5, K.dp(prob), K.dp(z), None, None, 2, 8, 0.05, 0, K.dp(out), None) == -1 and b"NULL" in lib.emu_predict_last_error()
    assert (out == 0).all()
    c = K.parking_case(5, 4); rec, prof = K.emu_parking(c, K.parking_rates(c), 32, profile=False)
    assert prof is None and rec[5] == 161


# ---------------------------------------------------------------- 6. the front end's packing, the public surface, the build rule, the Julia shim
def test_front_end_packs_rates_through_the_helpers_of_move_obstacles():
    from obca_amd import api
    nObs = np.array([1, 16, 2, 3, 3]); nt = 25
    assert np.array_equal(api._parking_rates(nObs, None, None, None), np.zeros((nt, 6)))
    r = api._parking_rates(nObs, [1, 2, 3], np.arange(10.0).reshape(5, 2), 0.5)
    assert r.shape == (nt, 6) and (r[:, :3] == [1, 2, 3]).all() and np.array_equal(r[:, 3:5], np.repeat(np.arange(10.0).reshape(5, 2), nObs, axis=0)) and (r[:, 5] == 0.5).all()
    assert np.array_equal(api._parking_rates(nObs, np.arange(75.0).reshape(25, 3), None, np.arange(25.0))[:, [0, 5]], np.c_[np.arange(0, 75.0, 3), np.arange(25.0)])
    q = api._quad_rates(4, [1, 2, 3], np.arange(4.0))
    assert q.shape == (4, 5, 4) and (q[:, :, :3] == [1, 2, 3]).all() and q[:, 0, 3].tolist() == [0, 1, 2, 3] and np.array_equal(api._quad_rates(4, None, None), np.zeros((4, 5, 4)))
    src = inspect.getsource(api._parking_rates) + inspect.getsource(api._quad_rates)
    assert src.count("_per_obstacle(") == 1 and src.count("_per_box(") == 1      # the one helper each, no second packing


def test_header_exports_python_and_julia_agree():
    import obca_amd
    from obca_amd import api, cabi, planner as PL
    import test_hybrid_cpu as TH
    import test_julia_shim_cpu as J
    protos = cabi.prototypes("obca_predict.h")
    assert sorted(protos) == sorted(api.PREDICT_EXPORTS) and len(protos) == 8 and "obca_predict.h" in cabi.__doc__
    others = set()
    for name in dir(api):
        if name.endswith("EXPORTS") and name != "PREDICT_EXPORTS":
            others |= set(getattr(api, name))
    assert len(others) > 100 and not set(api.PREDICT_EXPORTS) & (others | set(PL.PLAN3D_EXPORTS))
    assert [len(protos[n][1]) for n in api.PREDICT_EXPORTS] == [6, 2, 3, 18, 6, 2, 3, 13]
    # the host-pointer calls take the arguments of the clearance calls, then rates and profile
    clr = cabi.prototypes("obca_clearance.h")
    for mine, theirs in (("obca_parking_predict_batch", "obca_parking_clearance_batch"), ("obca_quadcopter_predict_batch", "obca_quadcopter_clearance_batch")):
        assert len(protos[mine][1]) == len(clr[theirs][1]) + 2
    # no name of the header falls under a filter by which an older test picks ITS entry points out of the library's symbols
    assert not any(w in s for s in api.PREDICT_EXPORTS for w in ("track", "rollout", "plan", "refine", "hybrid", "scene", "subdivide", "path_ws", "start_download", "ensemble",
                                                                 "certify", "shift", "advance", "obstacles"))
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {s for s in exported if "predict" in s} == set(api.PREDICT_EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "obca_predict.h")).read()
    assert re.search(r"#define OBCA_PRD_OUT 32\b", hdr) and re.search(r"#define OBCA_PRD_PIN 6\b", hdr) and re.search(r"#define OBCA_PRD_QIN 4\b", hdr) and V.PRD_OUT == 32
    assert "8 B (N S + 1) bytes" in hdr      # what the profile costs stands in the header
    for f in ("parking_predict_batch", "quadcopter_predict_batch"):
        assert hasattr(obca_amd, f) and f in obca_amd.__all__
    sig = inspect.signature(obca_amd.Batch.predict_clearance).parameters
    assert list(sig) == ["self", "rates", "pivot", "grow", "substeps", "need", "profile"] and (sig["substeps"].default, sig["need"].default, sig["profile"].default) == (8, 0.05, False)
    sig = inspect.signature(obca_amd.QuadBatch.predict_clearance).parameters
    assert list(sig) == ["self", "rates", "grow", "substeps", "need", "profile"] and (sig["substeps"].default, sig["need"].default, sig["profile"].default) == (8, 0.0, False)
    assert all(m in vars(api._DeviceBatch) for m in ("predict_profile", "predict_clearance_ms"))
    for f in (V.predict_parking, V.predict_quad):      # the statement stands on move_obstacles and the samples of the clearance check
        assert "move_obstacles_" in inspect.getsource(f)
    assert "parking_samples(" in inspect.getsource(V.predict_parking) and "quad_point_clearance(" in inspect.getsource(V.predict_quad) and "clearance_record(" in inspect.getsource(V.predict_record)
    # every ccall of the shim against the header, parameter by parameter; a library constant of its own
    kinds = TH._kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCAPredict.jl")).read()
    assert re.search(r"^const PRD = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), PRD\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
        assert m.group(2) == "Cint"
    assert {n for n, _ in calls} == set(kinds) == set(api.PREDICT_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])
    assert src.count("ccall(") == len(calls) + 1 and "ccall((:obca_last_error, LIB)" in src


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu"); name = "predict_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_predict_emu.so")
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
    for h in ("obca_predict.h", "obca_clearance.h", "obca_validate.h", "obca_solver.h", "obca_quad_solver.h", "obca_model.h"):
        assert os.path.realpath(os.path.join(csrc, h)) in seen, h
    assert os.path.realpath(os.path.join(ROOT, "include", "obca_predict.h")) in deps
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_predict_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/predict_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # nothing in csrc includes the kernel text but the one line of the library, and it comes behind its prerequisites
    for f in os.listdir(csrc):
        if f.endswith((".h", ".hip", ".cpp")) and f != "obca_hip.hip":
            assert not re.search(r'#\s*include\s*"obca_predict.h"', open(os.path.join(csrc, f)).read()), f
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    assert hip.count('#include "obca_predict.h"') == 1 and hip.count('#include "../../include/obca_predict.h"') == 1
    assert hip.index('#include "obca_validate.h"') < hip.index('#include "obca_clearance.h"') < hip.index('#include "obca_predict.h"')
    # the kernel header includes nothing and demands its prerequisites; no atomics, no loops that wait; the first 24 fields come out of the clearance text's own writers
    raw = open(os.path.join(csrc, "obca_predict.h")).read(); txt = re.sub(r"//.*", "", raw)
    assert "#include" not in txt and '#error "include the validate and the clearance kernel texts' in raw
    assert not re.search(r"\bwhile\b|\bgoto\b|atomic", txt)
    assert txt.count("clr::write_record(") == 1 and txt.count("clr::acc_take(") == 2 and txt.count("clr::acc_init(") == 2 and txt.count("dualws_one<VM>(") == 1
    assert txt.count("sin(") == 2 and txt.count("cos(") == 2 and "if (tr) { rs = sin(th); rc = cos(th); }" in txt      # the pose's, and the turn's only where w tau != 0
    # the kernels of the library read the records and the iterate: every pointer but the record and the profile is const
    for k in re.findall(r"void (obca_predict_\w+_kernel)\(([^)]*)\)", hip):
        assert [a.strip() for a in k[1].split(",") if "*" in a and "const" not in a] == ["double *out", "double *prof"], k
