"""One step of the closed receding-horizon loop, without a GPU: the kernel text of obca_amd/csrc/obca_advance.h compiled for the host (tests/emu/advance_emu.cpp) against the
numpy statement (validate.advance_parking / advance_quad / advance_record) on the solved trajectories of tests/golden/rollout_cases.npz and on synthetic ones at the loop
edges; the restart part against the EXISTING numpy shifts (tests/shift_common.py, tests/quad_shift_common.py) fed the host build's own plant state, bit for bit in both lane
orders; bad instances among healthy neighbours; the log; the public surface, the build rule and the Julia shim.  tests/advance_common.py has the tolerances."""
import inspect
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import packing as P
import rollout_common as R
import advance_common as A
from obca_amd import validate as V

KICK4 = np.array([0.02, -0.02, 0.01, -0.03]); KICK12 = 0.02 * np.cos(np.arange(12.0))
WORST = {"v": 0.0}


def _park_step(inst, shift, S, kick, logged=-1, tol=A.TOL_HOST):
    """one parking instance: record and plant state against numpy within tol; the restart against the numpy shift, bit for bit, both lane orders; the record's bits do
    not depend on the lane order"""
    ref, X, st = A.ref_parking(inst, shift, S, kick, logged=logged)
    runs = [A.emu_parking([inst], shift, S, kick, rev=rev) for rev in (0, 1)]
    for e in runs:
        what = ("parking", inst["N"], shift, S, kick is not None)
        A.check_record(e["out"][0], ref, tol, what)
        assert R.close(e["st"][0], st, tol), what
        WORST["v"] = max(WORST["v"], R.worst(e["out"][0][A.REAL], ref[A.REAL]), R.worst(e["st"][0], st))
        prob, z0 = A.restart_parking(inst, shift, e["st"][0])
        assert A.same(e["prob"][0], prob), what + (np.flatnonzero(A.bits(e["prob"][0]) != A.bits(prob))[:8].tolist(),)
        assert A.same(e["z0"][0], z0), what + (np.flatnonzero(A.bits(e["z0"][0]) != A.bits(z0))[:8].tolist(),)
        assert np.isnan(e["tmp"][0, 3 * (inst["N"] + 1):]).all(), what      # the scratch is used for the reference alone
    assert all(A.same(runs[0][k], runs[1][k]) for k in ("out", "st", "prob", "z0"))
    return runs[0], X, st


def _quad_step(inst, shift, S, kick, xF_new=None, tol=A.TOL_HOST):
    ref, X, st = A.ref_quad(inst, shift, S, kick, xF_new)
    runs = [A.emu_quad([inst], shift, S, kick, xF_new, rev=rev) for rev in (0, 1)]
    for e in runs:
        what = ("quad", inst["N"], shift, S, kick is not None, xF_new is not None)
        A.check_record(e["out"][0], ref, tol, what)
        assert R.close(e["st"][0], st, tol), what
        WORST["v"] = max(WORST["v"], R.worst(e["out"][0][A.REAL], ref[A.REAL]), R.worst(e["st"][0], st))
        assert A.same(e["prob"][0], A.restart_quad(inst, shift, e["st"][0], xF_new)), what
    assert all(A.same(runs[0][k], runs[1][k]) for k in ("out", "st", "prob"))
    return runs[0], X, st


# ---------------------------------------------------------------- 1. host build against numpy, restart against the numpy shifts
@pytest.mark.parametrize("i", range(3))
def test_parking_host_build_matches_numpy_and_the_numpy_shift(i):
    """The solved parking instances of the golden file, shift 0, 1, N-1, N (and 4), S = 1, 8 and 32, with and without a kick: record and plant state within 3.1e-10
    max(1, |value|) of the numpy statement.  Measured maximum on x86-64 (g++ -O1, glibc): 0 -- both sides run the same operations in the same order, the bits agree.  The
    restart is the numpy shift's, fed the host build's plant state: bit-equal, both lane orders."""
    inst = A.park_instance(R.golden_parking()[i], seed=i); N = inst["N"]
    for shift, S, kick in ((0, 8, None), (0, 8, KICK4), (1, 1, KICK4), (1, 32, None), (4, 8, KICK4), (4, 32, KICK4), (N - 1, 8, None), (N, 1, KICK4), (N, 8, None)):
        e, X, st = _park_step(inst, shift, S, kick)
        assert e["out"][0, 0] == 0 and e["out"][0, 12] == shift and e["out"][0, 11] == S and e["out"][0, 15] == -1
        if shift == 0:      # the plant stands: X0 + kick, to the bit
            assert A.same(e["st"][0], inst["x0"] + (0 if kick is None else kick)) and e["out"][0, 2] == -1 and e["out"][0, 1] == 0 and e["out"][0, 13] == 0
    print("worst host build against numpy:", WORST["v"])
    assert WORST["v"] <= A.TOL_HOST


@pytest.mark.parametrize("i", range(4))
def test_quad_host_build_matches_numpy_and_the_numpy_shift(i):
    """make_quad_batch(4, 20), solved (the golden file): the same for the quadcopter, with a moving goal and with an instance whose last solve failed (it keeps its uploaded
    start, X0 moves on).  Measured maximum: 0."""
    c = R.golden_quad()[i]; N = c["N"]
    for flag in (1.0, 0.0):
        inst = A.quad_instance(c, seed=i, flag=flag)
        for shift, S, kick, xf in ((0, 8, KICK12, None), (1, 1, None, None), (1, 32, KICK12, inst["xF"] + 1.0), (N - 1, 8, KICK12, None), (N, 8, None, inst["xF"] - 1.0)):
            e, X, st = _quad_step(inst, shift, S, kick, xf)
            assert e["out"][0, 0] == 0 and e["out"][0, 12] == shift
            if flag == 0.0:      # nothing but X0 (and XF) of the record has moved
                keep = inst["prob"].copy(); keep[P.QPH_X0:P.QPH_X0 + 12] = e["st"][0]
                if xf is not None:
                    keep[P.QPH_XF:P.QPH_XF + 12] = xf
                assert A.same(e["prob"][0], keep)
    assert WORST["v"] <= A.TOL_HOST


def test_the_plant_starts_at_the_records_x0_not_at_the_solutions_node_0():
    c = R.golden_parking()[0]
    a = A.park_instance(c, seed=1, x0=c["x"][:, 0]); b = A.park_instance(c, seed=1, x0=c["x"][:, 0] + [0.5, 0, 0, 0])
    ea = A.emu_parking([a], 3); eb = A.emu_parking([b], 3)
    assert abs((eb["st"][0, 0] - ea["st"][0, 0]) - 0.5) < 1e-12 and eb["out"][0, 1] > 0.4 > ea["out"][0, 1]
    # at the solution's own node 0 and without a kick the step is the chain rollout's first intervals: the rollout's host build gives the same node state, bit for bit
    _, X, _ = R.emu_parking(dict(c, ts=np.full(c["N"] + 1, a["t"])), 8, 0)
    assert A.same(ea["st"][0], X[:, 3])


# ---------------------------------------------------------------- 2. the loop edges
@pytest.mark.parametrize("N,shift", [(64, 1), (65, 64), (128, 127), (128, 128), (2, 2)])
def test_parking_loop_edges(N, shift):
    for j, c in enumerate(R.synthetic_parking(N)):
        _park_step(A.park_instance(c, seed=N + j), shift, 2 if shift > 60 else 8, KICK4)


@pytest.mark.parametrize("N,shift", [(2, 0), (2, 1), (2, 2), (64, 1), (65, 64), (128, 127)])
def test_quad_loop_edges(N, shift):
    for j, c in enumerate(R.synthetic_quad(N)):
        _quad_step(A.quad_instance(c, seed=N + j), shift, 2 if shift > 60 else 8, KICK12)


@pytest.mark.parametrize("n", [0, 1, 16])
def test_parking_obstacle_counts(n):
    """no obstacle (nothing to measure: +inf, -1), one, and the sixteen the record holds; in records with the strides of the widest instance"""
    c = A.with_obstacles(R.golden_parking()[1], n); N = c["N"]
    inst = A.park_instance(c, seed=n, strides=(P.OB_HDR + 3 * (N + 1) + 5, P.layout(N, 16, 64)["len"] + 3))
    e, _, _ = _park_step(inst, 3, 8, KICK4)
    o = e["out"][0]
    if n == 0:
        assert o[16] == o[17] == np.inf and o[18] == o[19] == -1 and o[20] == 0 and o[21] == 25 and np.isinf(o[24:]).all()
    else:
        assert np.isfinite(o[24:24 + n]).all() and np.isinf(o[24 + n:]).all() and 0 <= o[19] < min(n, 3)      # (a repeated obstacle ties: the smaller index)


# ---------------------------------------------------------------- 3. bad instances among healthy neighbours
def _assert_bad(out, st, nS, shift, S, logged=-1):
    assert out[0] == 1 and np.isnan(out[[1, 3, 4, 5, 6, 7, 8, 9, 13, 14, 16, 17]]).all() and np.isnan(out[24:]).all() and np.isnan(st).all()
    assert out[2] == out[18] == out[19] == -1 and out[20] == out[21] == nS and out[22] == 1 and out[10] == 0 and out[11] == S and out[12] == shift and out[15] == logged


def test_parking_bad_instances_leave_their_neighbours_and_themselves_alone():
    """A NaN input and a NaN kick among healthy instances of a ragged batch: the neighbours' bits equal a run without the bad ones; a bad instance's problem record, start
    iterate and log rows are untouched to the last bit, its record is filled as the rollout fills a bad one."""
    N, shift, S, cap = 30, 2, 8, 5
    strides = (P.OB_HDR + 3 * (N + 1) + 5, P.layout(N, 16, 64)["len"] + 3)
    cs = [A.with_obstacles(R.golden_parking()[j % 3], n) for j, n in enumerate((3, 1, 16, 2))]
    good = [A.park_instance(c, seed=j, strides=strides) for j, c in enumerate(cs)]
    u = cs[1]["u"].copy(); u[0, 1] = np.nan                                                   # input 0 of interval 1: driven, shift = 2
    nan_u = A.park_instance(dict(cs[1], u=u), seed=1, strides=strides)
    kick = np.tile(KICK4, (4, 1)); kick_bad = kick.copy(); kick_bad[3, 2] = np.nan
    log0 = A.pattern(4 * cap * 4, 9).reshape(4, cap, 4)
    log = log0.copy(); e = A.emu_parking([good[0], nan_u, good[2], good[3]], shift, S, kick_bad, log=log, cap=cap, logged=1, vmax=8)
    logh = log0.copy(); h = A.emu_parking(good, shift, S, kick, log=logh, cap=cap, logged=1, vmax=8)
    for j in (0, 2):
        assert all(A.same(e[k][j], h[k][j]) for k in ("out", "st", "prob", "z0")) and A.same(log[j], logh[j]) and e["out"][j, 0] == 0 and e["out"][j, 15] == 3
        assert A.same(log[j, 1:3], np.vstack([A.ref_parking(good[j], shift, S, None)[1][:, 1], e["st"][j]])) and A.same(log[j, [0, 3, 4]], log0[j, [0, 3, 4]])
    for j, inst in ((1, nan_u), (3, good[3])):
        _assert_bad(e["out"][j], e["st"][j], shift * S + 1, shift, S, 3)
        assert A.same(e["prob"][j], inst["prob"]) and A.same(e["z0"][j], inst["z0"]) and A.same(log[j], log0[j])
        ref, _, st = A.ref_parking(inst, shift, S, kick_bad[j], logged=3)
        A.check_record(e["out"][j], ref, 0.0, j); assert np.isnan(st).all()
    # a NaN behind the driven part of the solution is not read by the plant: the instance advances (its restart carries the NaN, as after a shift)
    far = dict(good[0], z=good[0]["z"].copy()); far["z"][P.layout(N, 3, 5)["u"] + 2 * 10] = np.nan
    assert A.emu_parking([far], shift, S, vmax=8)["out"][0, 0] == 0


def test_quad_bad_instances_leave_their_neighbours_and_themselves_alone():
    """a NaN input, a NaN kick and a pitch driven through pi/2 among healthy quadcopter instances"""
    N, shift, S, cap = 20, 4, 8, 6
    good = [A.quad_instance(c, seed=j) for j, c in enumerate(R.golden_quad())] + [A.quad_instance(R.golden_quad()[0], seed=9)]
    x = R.golden_quad()[1]["x"].copy(); x[5, 2] = np.nan                                        # a state of node 2 <= shift
    nan_x = A.quad_instance(dict(R.golden_quad()[1], x=x), seed=1)
    x0 = good[3]["x0"].copy(); x0[3] = np.pi / 2 - 0.05; x0[9] = 2.0
    pole = A.quad_instance(R.golden_quad()[3], seed=3, x0=x0)
    kick = np.tile(KICK12, (5, 1)); kick_bad = kick.copy(); kick_bad[4, 7] = np.inf
    log0 = A.pattern(5 * cap * 12, 9).reshape(5, cap, 12)
    batch = [good[0], nan_x, good[2], pole, good[4]]
    log = log0.copy(); e = A.emu_quad(batch, shift, S, kick_bad, log=log, cap=cap, logged=2)
    logh = log0.copy(); h = A.emu_quad(good, shift, S, kick, log=logh, cap=cap, logged=2)
    for j in (0, 2):
        assert all(A.same(e[k][j], h[k][j]) for k in ("out", "st", "prob")) and A.same(log[j], logh[j]) and e["out"][j, 0] == 0 and e["out"][j, 15] == 6
        X = A.ref_quad(good[j], shift, S, None)[1]
        assert A.same(log[j, 2:6], np.vstack([X[:, 1:4].T, e["st"][j][None]])) and A.same(log[j, :2], log0[j, :2])
    for j in (1, 3, 4):
        _assert_bad(e["out"][j], e["st"][j], shift * S + 1, shift, S, 6)
        assert A.same(e["prob"][j], batch[j]["prob"]) and A.same(log[j], log0[j])
        ref, _, st = A.ref_quad(batch[j], shift, S, kick_bad[j], logged=6)
        A.check_record(e["out"][j], ref, 0.0, j); assert np.isnan(st).all()
    # the pole instance without the turn is healthy, and numpy's rollout calls the turned one bad because of the pole, not of a number
    Xp, _, _, ok = V.advance_quad(pole["x"], pole["u"], pole["t"], pole["Ts"], shift, S, pole["x0"])
    assert not ok and h["out"][3, 0] == 0


# ---------------------------------------------------------------- 4. the log
def test_three_advances_append_their_plant_trajectories_and_overflow_is_refused():
    """three steps of shift 2 (each restarted instance re-packed as the next step's solution: a solve that changes nothing) append 6 nodes that equal the three plant
    trajectories, the last node of each after the kick; a fourth step into a log of 7 is refused with nothing written"""
    c = R.golden_parking()[0]; N = c["N"]; cap = 7
    log = A.pattern(cap * 4, 5).reshape(1, cap, 4); inst = A.park_instance(c, seed=4); want = []
    for step in range(3):
        e = A.emu_parking([inst], 2, 8, KICK4 * (step + 1), log=log, cap=cap, logged=2 * step)
        _, X, st = A.ref_parking(inst, 2, 8, KICK4 * (step + 1))
        assert e["out"][0, 15] == 2 * step + 2 and A.same(e["st"][0], st)
        want += [X[:, 1], st]
        # the next "solution" is the restart itself: x, u, multipliers of z0, the record as the step left it (X0 = the plant state)
        xp, up, _, lp, npp, _ = P.unpack_solution(e["z0"][0], N, inst["nOb"], inst["M"], A=inst["A"])
        N1 = N + 1; ref = e["prob"][0, P.OB_HDR:P.OB_HDR + 3 * N1].reshape(3, N1)
        inst = A.park_instance(dict(c, x=xp, u=up, ts=np.ones(N1)), seed=4, x0=e["prob"][0, P.PH["X0"]:P.PH["X0"] + 4], xF=inst["xF"], lp=lp, npp=npp, ref=ref)
        assert A.same(inst["x0"], st)
    assert A.same(log[0, :6], np.array(want)) and A.same(log[0, 6], A.pattern(cap * 4, 5).reshape(cap, 4)[6])
    before = log.copy()
    e = A.emu_parking([inst], 2, 8, None, log=log, cap=cap, logged=6, expect=-1)
    assert A.same(log, before) and (e["out"] == -7.0).all() and (e["st"] == -7.0).all() and A.same(e["prob"][0], inst["prob"]) and A.same(e["z0"][0], inst["z0"])
    assert b"log" in A.emu().emu_advance_last_error()


def test_argument_errors():
    inst = A.park_instance(R.golden_parking()[0]); q = A.quad_instance(R.golden_quad()[0])
    for kw in (dict(shift=-1), dict(shift=31), dict(substeps=0), dict(substeps=33), dict(need=np.nan), dict(need=np.inf)):
        a = dict(shift=2, substeps=8, need=0.05); a.update(kw)
        e = A.emu_parking([inst], a["shift"], a["substeps"], None, a["need"], expect=-1)
        assert (e["out"] == -7.0).all() and A.same(e["prob"][0], inst["prob"]) and A.same(e["z0"][0], inst["z0"])
        a["shift"] = min(a["shift"], 21)
        assert (A.emu_quad([q], a["shift"], a["substeps"], None, None, a["need"], expect=-1)["out"] == -7.0).all()


# ---------------------------------------------------------------- 5. the public surface, the build rule, the Julia shim
def test_header_exports_python_and_julia_agree():
    import obca_amd
    from obca_amd import api, cabi, planner as PL
    import test_hybrid_cpu as TH
    import test_julia_shim_cpu as J
    protos = cabi.prototypes("obca_advance.h")
    assert sorted(protos) == sorted(api.ADVANCE_EXPORTS) and len(protos) == 10 and "obca_advance.h" in cabi.__doc__
    others = (set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS) | set(api.REFINE_EXPORTS) | set(api.QUAD_SUBDIVIDE_EXPORTS) | set(api.PLAN_DEVICE_EXPORTS)
              | set(api.SCENE_EXPORTS) | set(api.PLAN_RESIDENT_EXPORTS) | set(api.PLAN_RESIDENT_CHECK_EXPORTS) | set(api.QUAD_PLAN_RESIDENT_EXPORTS) | set(api.ROLLOUT_EXPORTS)
              | set(api.TRACK_EXPORTS) | set(api.ENSEMBLE_EXPORTS) | set(api.CERTIFY_EXPORTS) | set(PL.PLAN3D_EXPORTS))
    assert not set(api.ADVANCE_EXPORTS) & others
    assert not any(set(protos) & set(cabi.prototypes(h)) for h in ("obca_hip.h", "obca_rollout.h", "obca_track.h", "obca_ensemble.h"))
    assert [len(protos[n][1]) for n in api.ADVANCE_EXPORTS] == [6, 2, 2, 2, 3, 7, 2, 2, 2, 3]
    # no name of the header falls under a filter by which an older test picks ITS entry points out of the library's symbols
    assert not any(w in s for s in api.ADVANCE_EXPORTS for w in ("track", "rollout", "plan", "refine", "hybrid", "scene", "subdivide", "clearance", "path_ws", "start_download",
                                                                 "ensemble", "certify", "shift"))
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {s for s in exported if "advance" in s} == set(api.ADVANCE_EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "obca_advance.h")).read()
    txt = open(os.path.join(ROOT, "obca_amd", "csrc", "obca_advance.h")).read()
    assert re.search(r"#define OBCA_ADV_OUT 40\b", hdr) and re.search(r"#define AV_OUT 40\b", txt) and V.ADV_OUT == V.ROLL_OUT == 40
    for cls, need, extra in ((obca_amd.Batch, V.DMIN, []), (obca_amd.QuadBatch, 0.0, ["xF_new"])):
        sig = inspect.signature(cls.advance).parameters
        assert list(sig) == ["self", "shift", "substeps", "kick"] + extra + ["need"]
        assert [sig[n].default for n in list(sig)[2:]] == [8, None] + [None] * len(extra) + [need]
        assert all(callable(getattr(cls, m)) and m in vars(api._DeviceBatch) for m in ("advance_state", "advance_log", "advance_log_states", "advance_ms"))
    # every ccall of the shim against the header, parameter by parameter; a library constant of its own
    kinds = TH._kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCAAdvance.jl")).read()
    assert re.search(r"^const ADV = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), ADV\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
        assert m.group(2) == "Cint"
    assert {n for n, _ in calls} == set(kinds) == set(api.ADVANCE_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])
    assert src.count("ccall(") == len(calls) + 1 and "ccall((:obca_last_error, LIB)" in src


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu"); name = "advance_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_advance_emu.so")
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
    for h in ("obca_advance.h", "obca_rollout.h", "obca_shift.h", "obca_quad_shift.h", "obca_clearance.h", "obca_quad_model.h", "obca_model.h"):
        assert os.path.realpath(os.path.join(csrc, h)) in seen, h
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_advance_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/advance_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # nothing in csrc includes the kernel text but the one line of the library
    for f in os.listdir(csrc):
        if f.endswith((".h", ".hip", ".cpp")) and f != "obca_hip.hip":
            assert not re.search(r'#\s*include\s*"obca_advance.h"', open(os.path.join(csrc, f)).read()), f
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    assert hip.count('#include "obca_advance.h"') == 1 and hip.count('#include "../../include/obca_advance.h"') == 1
    assert max(hip.index('#include "obca_%s.h"' % h) for h in ("rollout", "shift", "quad_shift")) < hip.index('#include "obca_advance.h"')
    # the plant, the measurement and the restart are the existing device functions, and the text says when the rewrite may start
    raw = open(os.path.join(csrc, "obca_advance.h")).read(); txt = re.sub(r"//.*", "", raw)
    assert "#include" not in txt and '#error "include the rollout' in raw and '#error "include the two shift texts' in raw      # (older tests let no header name those files)
    assert txt.count("integrate<") == 2 and txt.count("write_head<") == 2 and "shf::shift_instance(" in txt and "quad::quad_shift_instance(" in txt and "dualws_one<VM>" in txt
    assert not re.search(r"\bwhile\b|\bbreak\b|\bgoto\b|atomic", txt)
    for fn in ("shf::shift_instance(", "quad::quad_shift_instance("):      # a synchronisation stands right in front of each rewrite
        assert re.search(r"SYNC\(\);\s*" + re.escape(fn), txt), fn
    assert "ORDER" in open(os.path.join(csrc, "obca_advance.h")).read()
