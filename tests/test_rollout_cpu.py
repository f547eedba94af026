"""Rollout on the continuous vehicle models (obca_amd/csrc/obca_rollout.h): the numpy statement (obca_amd/validate.py) against an integrator that shares no code with it
(scipy's DOP853, stored in tests/golden/rollout_cases.npz) and against the closed form of the bicycle's yaw and speed; the kernel text compiled for the host
(tests/emu/rollout_emu.cpp) against the numpy statement, against the clearance emulation, dealt forwards and backwards, on non-finite input; the pinned figures of the
fixture; the public surface and the host build as a piece of the build rule.  No GPU.  Trajectories, comparison rules and tolerances: tests/rollout_common.py."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import clearance_common as K
import rollout_common as R
from obca_amd import validate as V


# ---------------------------------------------------------------- 1. the statement against independent mathematics
def test_numpy_statement_converges_with_fourth_order_to_dop853():
    """chain mode at 2, 4, 8 sub-steps against the DOP853 node states (rtol 1e-13): the error falls by 2^4 per doubling -- [12, 20] asserted, 15.98 .. 16.00 measured"""
    g = R.golden()
    for i, c in enumerate(R.golden_quad()[:2]):
        e = [np.abs(V.rollout_quad(c["x"], c["u"], c["ts"], c["Ts"], S_, False)[0] - g["quad_ivp"][i]).max() for S_ in (2, 4, 8)]
        print("quadcopter %d: errors %s, ratios %.3f %.3f" % (i, e, e[0] / e[1], e[1] / e[2]))
        assert 12 <= e[0] / e[1] <= 20 and 12 <= e[1] / e[2] <= 20 and e[2] < 1e-4, e
    for i, c in enumerate(R.golden_parking()):
        e = [np.abs(V.rollout_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], S_, False)[0][:2] - g["park_ivp"][i][:2]).max() for S_ in (2, 4, 8)]
        print("parking %d (x, y): errors %s, ratios %.3f %.3f" % (i, e, e[0] / e[1], e[1] / e[2]))
        assert 12 <= e[0] / e[1] <= 20 and 12 <= e[1] / e[2] <= 20 and e[2] < 1e-8, e


@pytest.mark.parametrize("S_", [1, 8])
def test_parking_yaw_and_speed_have_their_closed_form(S_):
    """psi' = v tan(delta) / L with v' = a is a quadratic in time: RK4 is exact for it whatever the step"""
    for c in R.golden_parking() + R.synthetic_parking(65):
        X, _ = V.rollout_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], S_, True)
        h = c["ts"][:-1] * c["Ts"]; v0, a = c["x"][3, :-1], c["u"][1]
        psi = c["x"][2, :-1] + np.tan(c["u"][0]) / c["L"] * (v0 * h + a * h * h / 2)
        assert np.abs(X[2, 1:] - psi).max() <= 1e-12 and np.abs(X[3, 1:] - (v0 + a * h)).max() <= 1e-12
        rec, Xe, _ = R.emu_parking(c, S_, 1)
        assert np.abs(Xe[2, 1:] - psi).max() <= 1e-12 and np.abs(Xe[3, 1:] - (v0 + a * h)).max() <= 1e-12 and rec[5] == 0 and rec[9] == 0


# ---------------------------------------------------------------- 2. the host build against the statement
WORST = {}


@pytest.mark.parametrize("restart", R.MODES)
@pytest.mark.parametrize("S_", [1, 8, 32])
@pytest.mark.parametrize("N", [2, 20, 65, 128])
def test_quadcopter_host_build_matches_numpy(N, S_, restart):
    for i, c in enumerate(R.quad_cases(N)):
        rec, X, P = R.emu_quad(c, S_, restart); ref, Xr, Pr = R.ref_quad(c, S_, restart)
        what = "quad N=%d S=%d restart=%d instance %d" % (N, S_, restart, i)
        R.check_record(rec, ref, R.TOL_HOST, what)
        assert R.close(X, Xr, R.TOL_HOST) and R.close(P, Pr, R.TOL_HOST) and rec[0] == 0 and rec[21] == N * S_ + 1 and (rec[10], rec[11]) == (restart, S_), what
        assert np.array_equal(X[:, 0], c["x"][:, 0]) and np.array_equal(P[::S_][:-1] if not restart else P[::S_], (X[:3].T[:-1] if not restart else c["x"][:3].T)), what
        WORST["quad"] = max(WORST.get("quad", 0.0), R.worst(rec[R.REAL], ref[R.REAL]), R.worst(X, Xr))
        one = c["ts"][:1].copy()      # one t, as a resident batch holds it
        if np.ptp(c["ts"]) == 0:
            assert np.array_equal(R.emu_quad(dict(c, ts=one), S_, restart, tstride=0)[0], rec), what
    print("largest difference host build - numpy so far:", WORST)


@pytest.mark.parametrize("restart", R.MODES)
@pytest.mark.parametrize("S_", [1, 8, 32])
@pytest.mark.parametrize("N", [1, 30, 65, 128])
def test_parking_host_build_matches_numpy(N, S_, restart):
    for i, c in enumerate(R.parking_cases(N)[:1 if N * S_ > 1024 else None]):
        rec, X, P = R.emu_parking(c, S_, restart); ref, Xr, Pr = R.ref_parking(c, S_, restart)
        what = "parking N=%d S=%d restart=%d instance %d" % (N, S_, restart, i)
        R.check_record(rec, ref, R.TOL_HOST, what)
        assert R.close(X, Xr, R.TOL_HOST) and R.close(P, Pr, R.TOL_HOST) and rec[0] == 0 and rec[21] == N * S_ + 1 and (rec[10], rec[11]) == (restart, S_), what
        WORST["parking"] = max(WORST.get("parking", 0.0), R.worst(rec[R.REAL], ref[R.REAL]), R.worst(X, Xr))
        if np.ptp(c["ts"]) == 0:
            assert np.array_equal(R.emu_parking(c, S_, restart, resident=True)[0], rec), what
    print("largest difference host build - numpy so far:", WORST)


def test_chain_and_restart_agree_on_the_first_interval_and_differ_after_it():
    c = R.golden_quad()[0]
    (rc, Xc, Pc), (rr, Xr, Pr) = R.emu_quad(c, 8, 0), R.emu_quad(c, 8, 1)
    assert np.array_equal(Xc[:, :2], Xr[:, :2]) and np.array_equal(Pc[:8], Pr[:8]) and not np.array_equal(Xc[:, 2], Xr[:, 2])
    assert rc[1] > rr[1] > 0.05 and rc[6] > 0 and rr[2] >= 1      # the open loop compounds what one interval is off by


# ---------------------------------------------------------------- 3. order independence, agreement with the clearance check
@pytest.mark.parametrize("restart", R.MODES)
def test_record_does_not_depend_on_how_items_are_dealt_to_the_lanes(restart):
    for c in R.golden_quad()[:2] + R.synthetic_quad(65)[:1]:
        for need in (0.0, 0.3):
            assert np.array_equal(R.emu_quad(c, 8, restart, need, rev=0)[0], R.emu_quad(c, 8, restart, need, rev=1)[0])
    for c in R.golden_parking()[:2] + R.synthetic_parking(65)[:1]:
        for need in (V.DMIN, 0.2):
            assert np.array_equal(R.emu_parking(c, 8, restart, need, rev=0)[0], R.emu_parking(c, 8, restart, need, rev=1)[0])


def test_restart_mode_sees_at_the_nodes_what_the_clearance_check_sees():
    """restart mode leaves the solution's own nodes as node samples: min_nodes, and at one sub-step the whole clearance record, equal the clearance emulation's bit for bit"""
    for c in R.golden_parking() + R.synthetic_parking(65):
        for S_ in (1, 8):
            rec = R.emu_parking(c, S_, 1)[0]; clr = K.emu_parking(c, S_, V.DMIN)
            assert rec[17] == clr[1] == K.emu_parking(c, 1, V.DMIN)[0], (S_, rec[16:24], clr[:8])
        node = R.emu_parking(c, 1, 1)[0][16:]; clr1 = K.emu_parking(c, 1, V.DMIN)
        assert np.array_equal(node, clr1), (node, clr1)      # every sample is a node: the per-obstacle minima over the nodes too
    for c in R.golden_quad() + R.synthetic_quad(65):
        for S_ in (1, 8):
            assert R.emu_quad(c, S_, 1)[0][17] == K.emu_quad(c, S_)[1]
        assert np.array_equal(R.emu_quad(c, 1, 1)[0][16:], K.emu_quad(c, 1))


# ---------------------------------------------------------------- 4. non-finite input
def assert_bad(rec, X, nS, restart, S_):
    exp = np.r_[1, np.nan, -1, np.full(7, np.nan), restart, S_, 0, 0, 0, 0, np.nan, np.nan, -1, -1, nS, nS, 1, 0, np.full(16, np.nan)]
    assert np.array_equal(rec, exp, equal_nan=True), rec
    assert np.isnan(X).all()


@pytest.mark.parametrize("restart", R.MODES)
def test_non_finite_input_marks_its_instance_and_no_other(restart):
    q = R.golden_quad(); good = [R.emu_quad(c, 4, restart)[0] for c in q]
    for field, idx, v in (("u", (1, 3), np.nan), ("u", (0, 19), np.inf), ("x", (7, 0), np.nan), ("ts", (2,), np.nan)):
        a = np.array(q[1][field], float); a[idx] = v
        bad = dict(q[1], **{field: a})
        rec, X, _ = R.emu_quad(bad, 4, restart)
        assert_bad(rec, X, 81, restart, 4)
        ref = R.ref_quad(bad, 4, restart)[0]
        assert np.array_equal(rec, ref, equal_nan=True), (field, rec, ref)
        for c, g in zip(q, good):      # (instances share nothing: the others come back bit for bit)
            assert np.array_equal(R.emu_quad(c, 4, restart)[0], g)
    p = R.golden_parking(); good = [R.emu_parking(c, 4, restart)[0] for c in p]
    for field, idx, v in (("u", (1, 2), np.nan), ("u", (0, 29), -np.inf), ("x", (3, 30), np.inf), ("ts", (4,), np.nan)):
        a = np.array(p[2][field], float); a[idx] = v
        rec, X, _ = R.emu_parking(dict(p[2], **{field: a}), 4, restart)
        assert_bad(rec, X, 121, restart, 4)
        for c, g in zip(p, good):
            assert np.array_equal(R.emu_parking(c, 4, restart)[0], g)
    rec, X, _ = R.emu_parking(dict(p[0], Ts=np.nan), 4, restart)
    assert_bad(rec, X, 121, restart, 4)


@pytest.mark.parametrize("restart", R.MODES)
def test_a_pitch_driven_through_half_pi_marks_its_instance(restart):
    """Rotor speeds inside their bounds that roll the vehicle over: x[3] passes pi/2, where the attitude kinematics divide by cos x[3] = 0 and the continuous state
    diverges.  RK4 steps across the pole with finite numbers (the largest state stays below 1e4 here), so the step itself is tested for a sign change of cos x[3]."""
    c = R.golden_quad()[0]; N = c["N"]
    u = np.full((4, N), 4.48); u[1] += 1.0; u[3] -= 1.0
    x = c["x"].copy()
    if restart:      # one interval from a node that stands just short of the pole, turning towards it
        x[3, 5] = np.pi / 2 - 0.05; x[9, 5] = 1.0
    over = dict(c, u=u, x=x)
    rec, X, _ = R.emu_quad(over, 8, restart)
    assert_bad(rec, X, 8 * N + 1, restart, 8)
    Xn, _ = V.rollout_quad(over["x"], u, c["ts"], c["Ts"], 8, restart)
    assert np.isnan(Xn).all() and np.array_equal(rec, R.ref_quad(over, 8, restart)[0], equal_nan=True)
    assert R.emu_quad(c, 8, restart)[0][0] == 0      # the solution itself stays clear of it
    # overflow: finite inputs, a rolled state that is not
    huge = dict(c, u=np.full((4, N), 1e160))
    assert_bad(*R.emu_quad(huge, 8, restart)[:2], 8 * N + 1, restart, 8)


# ---------------------------------------------------------------- 5. the fixture
def test_fixture_figures_are_pinned():
    """what tests/golden/make_rollout_cases.py printed: the one-interval defect of forward Euler and of the midpoint rule, and where the open loop ends up"""
    g = R.golden()
    assert int(g["substeps"]) == 8 and (g["quad_exitflag"] == 1).all() and (g["park_exitflag"] == 1).all()
    q, p = g["quad_rec"], g["park_rec"]
    assert np.abs(q[:, 1, 1] - [0.2689825, 0.3801814, 0.2588306, 0.3429215]).max() < 5e-7 and (q[:, 1, 1] > 0.05).all()      # restart: one interval of 0.5 s
    assert np.abs(q[:, 0, 1] - [2.008382, 1.1669699, 1.4353404, 1.1229677]).max() < 5e-7 and q[:, 0, 2].tolist() == [18, 17, 13, 18]      # chain
    assert np.abs(p[:, 1, 1] - [4.7758e-3, 2.8667e-3, 6.5628e-3]).max() < 5e-8 and np.abs(p[:, 0, 1] - [2.24846e-2, 1.35966e-2, 3.24481e-2]).max() < 5e-8 and p[2, 0, 1] > 0.01 and p[:, 0, 2].tolist() == [23, 21, 22]
    assert (p[:, 1, 3] < 1e-6).all() and (p[:, 1, 4] < 1e-9).all()      # yaw and speed: the midpoint rule is exact for them (what is left is the solve's own residual)
    for i, c in enumerate(R.golden_quad()):
        for restart in R.MODES:
            R.check_record(R.emu_quad(c, 8, restart)[0], q[i, restart], R.TOL_HOST, "quad fixture %d %d" % (i, restart))
    for i, c in enumerate(R.golden_parking()):
        for restart in R.MODES:      # (the fixture's distances are the oracle's DualMultWS: 1e-9, tests/clearance_common.py)
            rec = R.emu_parking(c, 8, restart)[0]
            R.check_record(np.r_[rec[:16], p[i, restart, 16:]], p[i, restart], R.TOL_HOST, "parking fixture %d %d" % (i, restart))
            assert R.close(rec[R.REAL], p[i, restart][R.REAL], K.TOL_PARK) and np.array_equal(rec[[18, 19, 21, 22]], p[i, restart][[18, 19, 21, 22]]) and abs(rec[20] - p[i, restart, 20]) <= 1
    # the car keeps 0.05 to the obstacles at the nodes of the NLP and loses part of it on the way it really drives
    assert (p[:, 0, 16] < p[:, 1, 17] - 0.01).all() and (p[:, 1, 17] >= 0.05).all() and np.abs(p[:, 0, 16] - [0.0302152, 0.0438948, 0.0350757]).max() < 5e-7


# ---------------------------------------------------------------- 6. refusals, the public surface and the build rule
def test_argument_errors():
    lib = R.emu(); c = R.golden_parking()[0]; out = np.zeros(40); w = np.zeros(40000)
    z = np.zeros(8192); prob = np.zeros(4096)
    for S_, restart, need, msg in ((0, 0, 0.05, b"need 1 <= substeps <= 32"), (33, 1, 0.05, b"need 1 <= substeps <= 32"), (8, 2, 0.05, b"restart must be 0 (chain) or 1 (restart at every node)"),
                                   (8, -1, 0.05, b"restart must be 0"), (8, 0, np.nan, b"need a finite `need`"), (8, 1, np.inf, b"need a finite `need`")):
        assert lib.emu_rollout_parking(c["N"], K.dp(prob), K.dp(z), None, 2, S_, restart, need, 0, K.dp(w), K.dp(w), K.dp(out)) == -1 and msg in lib.emu_rollout_last_error()
        assert lib.emu_rollout_quad(5, K.dp(prob), K.dp(z), K.dp(z), K.dp(z), 1, S_, restart, need, 0, K.dp(w), K.dp(w), K.dp(out)) == -1 and msg in lib.emu_rollout_last_error()
    for N in (0, 129):
        assert lib.emu_rollout_parking(N, K.dp(prob), K.dp(z), None, 2, 8, 0, 0.05, 0, K.dp(w), K.dp(w), K.dp(out)) == -1 and b"1 <= N <= OBCA_NMAX" in lib.emu_rollout_last_error()
        assert lib.emu_rollout_quad(N, K.dp(prob), K.dp(z), K.dp(z), K.dp(z), 1, 8, 0, 0.0, 0, K.dp(w), K.dp(w), K.dp(out)) == -1 and b"1 <= N <= OBCA_QUAD_NMAX" in lib.emu_rollout_last_error()
    assert (out == 0).all()
    # the library's own refusals: one text per cause and entry point
    hip = open(os.path.join(ROOT, "obca_amd", "csrc", "obca_hip.hip")).read()
    for e in ("obca_batch_rollout", "obca_quad_batch_rollout"):
        assert '"%s: NULL argument"' % e in hip and '"%s: nothing has been solved since the last upload or shift"' % e in hip
        assert '"%s_ms: no rollout has run on this batch"' % e in hip and 'rollout_states(bt, %s, X, "%s_states")' % ("4" if e == "obca_batch_rollout" else "QX", e) in hip
    assert '": no rollout has run on this batch since it was last filled"' in hip and '"obca_batch_rollout: needs a horizon N>=1"' in hip
    assert '"obca_parking_rollout_batch: need B>=1, 1<=N<=OBCA_NMAX"' in hip and '"obca_quadcopter_rollout_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"' in hip
    assert hip.count("roll::rollout_check_args(substeps, restart, need)") == 4


def test_header_exports_python_and_julia_agree():
    import inspect
    import obca_amd
    from obca_amd import api, cabi, planner as PL
    import test_hybrid_cpu as TH
    import test_julia_shim_cpu as J
    protos = cabi.prototypes("obca_rollout.h")
    assert sorted(protos) == sorted(api.ROLLOUT_EXPORTS) and len(protos) == 8 and "obca_rollout.h" in cabi.__doc__
    others = (set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS) | set(api.REFINE_EXPORTS) | set(api.QUAD_SUBDIVIDE_EXPORTS) | set(api.PLAN_DEVICE_EXPORTS)
              | set(api.SCENE_EXPORTS) | set(api.PLAN_RESIDENT_EXPORTS) | set(api.PLAN_RESIDENT_CHECK_EXPORTS) | set(api.QUAD_PLAN_RESIDENT_EXPORTS) | set(PL.PLAN3D_EXPORTS))
    assert not set(api.ROLLOUT_EXPORTS) & others and not set(protos) & set(cabi.prototypes("obca_hip.h"))
    assert [len(protos[n][1]) for n in api.ROLLOUT_EXPORTS] == [5, 2, 2, 18, 5, 2, 2, 14]
    # no name of the header falls under a filter by which an older test picks ITS entry points out of the library's symbols
    assert not any(w in s for s in api.ROLLOUT_EXPORTS for w in ("refine", "hybrid", "scene", "plan", "subdivide", "clearance", "path_ws", "start_download"))
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {s for s in exported if "rollout" in s} == set(api.ROLLOUT_EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "obca_rollout.h")).read()
    assert re.search(r"#define OBCA_ROLL_OUT 40\b", hdr) and re.search(r"#define OBCA_ROLL_CLR 16\b", hdr) and re.search(r"#define OBCA_ROLL_MAXSUB 32\b", hdr)
    assert V.ROLL_OUT == 40 == 16 + V.CLR_OUT
    lib = api._load(); f = C.c_float(0)
    assert lib.obca_batch_rollout(None, 8, 0, 0.05, np.zeros(40)) == -1 and lib.obca_quad_batch_rollout(None, 8, 0, 0.0, np.zeros(40)) == -1      # no batch: refused, no device touched
    assert lib.obca_batch_rollout_ms(None, C.byref(f)) == -1 and lib.obca_quad_batch_rollout_states(None, np.zeros(1)) == -1 and lib.obca_batch_rollout_states(None, np.zeros(1)) == -1
    with pytest.raises((TypeError, C.ArgumentError)):      # out as int32
        lib.obca_batch_rollout(None, 8, 0, 0.05, np.zeros(40, np.int32))
    for f_ in ("parking_rollout_batch", "quadcopter_rollout_batch"):
        assert hasattr(obca_amd, f_) and f_ in obca_amd.__all__
    for cls, need in ((obca_amd.Batch, V.DMIN), (obca_amd.QuadBatch, 0.0)):
        sig = inspect.signature(cls.rollout).parameters
        assert list(sig) == ["self", "substeps", "restart", "need"] and (sig["substeps"].default, sig["restart"].default, sig["need"].default) == (8, False, need)
        assert all(callable(getattr(cls, m)) for m in ("rollout_states", "rollout_ms")) and "rollout_states" in vars(api._DeviceBatch)
    # every ccall of the shim against the header, parameter by parameter; a library constant of its own
    kinds = TH._kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCARollout.jl")).read()
    assert re.search(r"^const ROL = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), ROL\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
        assert m.group(2) == "Cint"
    assert {n for n, _ in calls} == set(kinds) == set(api.ROLLOUT_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])
    assert src.count("ccall(") == len(calls) + 1 and "ccall((:obca_last_error, LIB)" in src


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu"); name = "rollout_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_rollout_emu.so")
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
    for h in ("obca_rollout.h", "obca_clearance.h", "obca_quad_model.h", "obca_model.h"):
        assert os.path.realpath(os.path.join(csrc, h)) in seen, h
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_rollout_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/rollout_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # the kernel text is nothing the solve kernels use, and it comes before the planner's text switches contraction off
    for f in os.listdir(csrc):
        if f.endswith(".h") and f != "obca_rollout.h":
            assert not re.search(r'#\s*include\s*"obca_rollout.h"', open(os.path.join(csrc, f)).read()), f
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    assert hip.count('#include "obca_rollout.h"') == 1 and '#include "obca_rollout.h"' in hip.split('#include "obca_hybrid.h"')[0]
    txt = re.sub(r"//.*", "", open(os.path.join(csrc, "obca_rollout.h")).read())
    assert "sincos_bounded" not in txt and "rcp_nr" not in txt and "atomic" not in txt and "dyn_g_value" not in txt
    model = open(os.path.join(csrc, "obca_quad_model.h")).read()
    body = model.split("OBCA_FN void dyn_g_continuous(")[1].split("\n}\n")[0]
    assert "sincos_bounded" not in body and "rcp_nr" not in body and "gyro" not in body
