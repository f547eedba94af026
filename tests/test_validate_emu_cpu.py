"""Device-side feasibility checks (obca_amd/csrc/obca_validate.h) compiled for the host (tests/emu/validate_emu.cpp) against the numpy checkers of
obca_amd/validate.py: the full golden solutions of configs 2 and 3, one oracle quadcopter solution per formulation, and perturbed copies of them.
Comparison rules and the derivation of the bound: tests/validate_compare.py."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from conftest import ROOT, golden
import packing as P
import validate_compare as K
from obca_amd import buildflags, scenarios as S, validate as V

D = C.POINTER(C.c_double)


def dp(a):
    return None if a is None else a.ctypes.data_as(D)


@pytest.fixture(scope="module")
def vemu():
    lib = C.CDLL(buildflags.build("validate_emu"))
    a, b, c, d = (C.c_int(0) for _ in range(4))
    lib.emu_validate_sizes(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    assert (a.value, b.value, c.value, d.value) == (len(V.VIOL_NAMES), 16, len(V.QUAD_VIOL_NAMES), 10)
    return lib


def emu_parking(lib, pr, x, u, ts, l, n, sl, tol=5e-5, host_style=False):
    """one instance through the kernel text.  host_style=False: everything in the iterate (a resident batch: one t, the iterate's slack);
    True: timeScale per stage and the slack beside it (the host-pointer entry)"""
    N, vOb, A = pr["N"], pr["vOb"], pr["A"]; nOb, M = len(vOb), int(np.sum(vOb)); Lz = P.layout(N, nOb, M)
    zero = np.zeros(N + 1)
    prob = P.pack_problem(pr["x0"], pr["xF"], N, pr["Ts"], pr["L"], pr["ego"], pr["XYb"], vOb, A, pr["b"], zero, zero, zero, pr.get("fixTime", 0), dist=int(pr.get("dist", False)))
    z = P.pack_start(N, nOb, M, x.T, u.T, l.T, n.T, A=A)
    ts = np.ascontiguousarray(np.broadcast_to(np.ravel(np.asarray(ts, float)), (N + 1,)))
    slp = np.ascontiguousarray(sl.T).ravel()
    if not host_style:
        z[Lz["t"]] = ts[0]; z[Lz["sl"]:Lz["sl"] + nOb * (N + 1)] = slp
    rl = np.ascontiguousarray(P.row_lengths(A)); out = np.zeros(16)
    lib.emu_validate_parking(C.c_int(N), dp(prob), dp(z), dp(rl), dp(ts) if host_style else None, dp(slp) if host_style else None, C.c_double(tol), dp(out))
    return int(out[14]), int(out[15]), out[:14].copy()


def check_parking(lib, pr, x, u, ts, l, n, sl, band, what, host_style=False, tol=5e-5):
    ok, rok, vec = K.numpy_parking(pr["x0"], pr["xF"], pr["N"], pr["Ts"], pr["L"], pr["ego"], pr["XYb"], pr["vOb"], pr["A"], pr["b"], x, u, ts, l, n, sl,
                                   fixTime=pr.get("fixTime", 0), dist=pr.get("dist", False), tol=tol)
    dok, drok, dvec = emu_parking(lib, pr, x, u, ts, l, n, sl, tol, host_style)
    bnd = K.bound(l, n)
    K.check_classes(dvec, vec, bnd, V.VIOL_NAMES, what)
    finite = all(np.isfinite(a).all() for a in (x, u, np.asarray(ts, float), l, n, sl))
    eok, erok = K.parking_flags_expected(vec, finite, tol, bnd)
    band.check(dok, eok, what + " ok"); band.check(drok, erok, what + " ref_ok")
    return dok, drok, dvec, vec


def golden_instances(name):
    g = golden(name); B, N = int(g["B"]), int(g["N"])
    if name == "oracle_cfg2.npz":
        bt = S.make_batch(S.BACKWARDS, B, N)
        prs = [dict(N=N, x0=bt["x0"][i], xF=bt["xF"][i], Ts=bt["Ts"][i], L=bt["L"], ego=bt["ego"], XYb=bt["XYbounds"], vOb=bt["vOb"], A=bt["A"], b=bt["b"]) for i in range(B)]
    else:
        A, b, v = S.scenario_hrep(S.PARALLEL)
        prs = [dict(N=N, x0=g["x0"][i], xF=g["xF"][i], Ts=g["Ts"][i], L=S.L_WHEELBASE, ego=S.EGO, XYb=S.XYBOUNDS, vOb=v, A=A, b=b) for i in range(B)]
    return g, prs


@pytest.mark.parametrize("name", ["oracle_cfg2.npz", "oracle_cfg3.npz"])
def test_parking_classes_and_flags_match_numpy_on_golden_solutions(vemu, name):
    g, prs = golden_instances(name); band = K.Band(); N = prs[0]["N"]
    for i, pr in enumerate(prs):
        args = (g["xp"][i], g["up"][i], np.full(N + 1, g["t"][i]), g["lp"][i], g["np"][i], g["sl"][i])
        dok, drok, dvec, vec = check_parking(vemu, pr, *args, band, "%s[%d]" % (name, i))
        assert dok == 1 and vec[:12].max() < 5e-5                 # the golden solutions are feasible at 5e-5
        _, _, hvec, _ = check_parking(vemu, pr, *args, K.Band(), "%s[%d] host style" % (name, i), host_style=True)
        assert np.array_equal(hvec, dvec)                          # the same point through the host-pointer arguments: the same bits


@pytest.mark.parametrize("name", ["oracle_cfg2.npz", "oracle_cfg3.npz"])
def test_parking_perturbed_solutions(vemu, name):
    g, prs = golden_instances(name); N = prs[0]["N"]
    for i, pr in enumerate(prs):
        base = dict(x=g["xp"][i], u=g["up"][i], ts=np.full(N + 1, g["t"][i]), l=g["lp"][i], n=g["np"][i], sl=g["sl"][i])

        def run(what, host_style=False, **kw):
            a = {k: np.array(v, float) for k, v in base.items()}; a.update(kw)
            return check_parking(vemu, pr, a["x"], a["u"], a["ts"], a["l"], a["n"], a["sl"], K.Band(), "%s[%d] %s" % (name, i, what), host_style)
        x = base["x"].copy(); x[0, N // 2] += 0.01                 # 1 cm off the dynamics
        dok, drok, dvec, _ = run("dyn", x=x)
        assert dok == 0 and dvec[V.VIOL_NAMES.index("dyn")] > 1e-3
        l = base["l"].copy(); l[0, 5] = -0.1                       # a negative dual
        dok, drok, dvec, _ = run("dual", l=l)
        assert dok == 0 and drok == 0 and abs(dvec[V.VIOL_NAMES.index("dual_pos")] - 0.1) < 1e-12
        u = base["u"].copy(); u[0, 3] = 0.7                        # steering beyond 0.6
        dok, drok, dvec, _ = run("u", u=u)
        assert dok == 0 and drok == 0 and dvec[0] > 0.09
        x = base["x"].copy(); x[0, 7] = np.nan                     # a NaN in x
        dok, drok, dvec, _ = run("nan", x=x)
        assert dok == 0 and drok == 0 and np.isnan(dvec[V.VIOL_NAMES.index("x_bounds")]) and np.isnan(dvec[V.VIOL_NAMES.index("dyn")])
        # a timeScale that varies over the stages (host-pointer entry only): ts_chain and dyn honour it
        ts = base["ts"] * (1 + 0.01 * np.sin(np.arange(N + 1)))
        dok, drok, dvec, vec = run("ts", host_style=True, ts=ts)
        assert dok == 0 and vec[V.VIOL_NAMES.index("ts_chain")] > 1e-3
        # without the slack (sl = zeros): sep reports what the slack absorbed
        run("no slack", host_style=True, sl=np.zeros_like(base["sl"]))
        # the dist conventions and fixTime on the same point
        for extra in (dict(dist=True), dict(fixTime=1)):
            pr2 = dict(pr, **extra)
            check_parking(vemu, pr2, *(base[k] for k in ("x", "u", "ts", "l", "n", "sl")), K.Band(), "%s[%d] %s" % (name, i, extra))
        # half-space rows that are not of unit length: lambda comes back in the caller's scaling
        pr3 = dict(pr, A=3.0 * np.asarray(pr["A"], float), b=3.0 * np.asarray(pr["b"], float))
        l = base["l"] / 3.0; l[1, 4] = -0.2
        _, _, dvec, _ = check_parking(vemu, pr3, base["x"], base["u"], base["ts"], l, base["n"], base["sl"], K.Band(), "%s[%d] scaled rows" % (name, i))
        assert abs(dvec[V.VIOL_NAMES.index("dual_pos")] - 0.2) < 1e-12


def emu_quad(lib, N, x0, xF, Ts, R, ob, x, u, ts, lam, tol=1e-3):
    prob = P.pack_quad_problem(x0, xF, N, Ts, R, ob, np.zeros((N + 1, 12)), 1.0)
    xs = np.ascontiguousarray(x.T); us = np.ascontiguousarray(u.T); ls = np.ascontiguousarray(lam.T)
    ts = np.ascontiguousarray(np.broadcast_to(np.ravel(np.asarray(ts, float)), (N + 1,))); out = np.zeros(10)
    lib.emu_validate_quad(C.c_int(N), dp(prob), dp(xs), dp(us), dp(ts), C.c_int(1), dp(ls), C.c_double(tol), dp(out))
    out1 = np.zeros(10)
    if np.ptp(ts) == 0:                                              # one t, as a resident batch holds it: the same bits
        lib.emu_validate_quad(C.c_int(N), dp(prob), dp(xs), dp(us), dp(ts[:1].copy()), C.c_int(0), dp(ls), C.c_double(tol), dp(out1))
        assert np.array_equal(out, out1, equal_nan=True)
    return int(out[9]), out[:9].copy()


@pytest.mark.parametrize("dist", [0, 1])
def test_quadcopter_classes_and_flag_match_numpy(vemu, dist):
    import oracle_quad as Q
    N = 30; Ts = S.quad_sample_time(N); xWS = S.quad_warm_start(S.QUAD_X0, S.QUAD_XF, N)
    r = Q.quadcopter_signed_dist(Q.X0, Q.XF, N, Ts, Q.EGO_R, S.QUAD_OB, xWS, 1.0, dist=dist)
    assert r["exitflag"] == 1
    x0 = np.ravel(Q.X0).astype(float); xF = np.ravel(Q.XF).astype(float)
    base = dict(x=r["xp"], u=r["up"], ts=np.broadcast_to(np.ravel(r["timeScale"]), (N + 1,)).copy(), lam=r["lp"])

    def run(what, **kw):
        a = {k: np.array(v, float) for k, v in base.items()}; a.update(kw)
        ok, vec = K.numpy_quad(a["x"], a["u"], a["ts"], x0, xF, Ts, a["lam"], S.QUAD_OB, Q.EGO_R)
        dok, dvec = emu_quad(vemu, N, x0, xF, Ts, Q.EGO_R, S.QUAD_OB, a["x"], a["u"], a["ts"], a["lam"])
        bnd = K.bound(a["lam"])
        K.check_classes(dvec, vec, bnd, V.QUAD_VIOL_NAMES, what)
        finite = all(np.isfinite(v).all() for v in a.values())
        K.Band().check(dok, K.quad_flag_expected(vec, finite, 1e-3, bnd), what)
        return dok, dvec
    assert run("solution")[0] == 1
    x = base["x"].copy(); x[0, N // 2] += 0.01
    dok, dvec = run("dyn", x=x); assert dok == 0 and dvec[4] > 1e-3
    lam = base["lam"].copy(); lam[7, 5] = -0.1
    dok, dvec = run("dual", lam=lam); assert dok == 0 and abs(dvec[6] - 0.1) < 1e-12
    u = base["u"].copy(); u[0, 3] = 8.0
    dok, dvec = run("u", u=u); assert dok == 0 and dvec[2] > 0.19
    x = base["x"].copy(); x[0, 7] = np.nan
    dok, dvec = run("nan", x=x); assert dok == 0 and np.isnan(dvec[3]) and np.isnan(dvec[4])
    ts = base["ts"] * (1 + 0.01 * np.sin(np.arange(N + 1)))
    dok, dvec = run("ts", ts=ts); assert dok == 0 and dvec[5] > 1e-3


def test_ref_worst_is_what_the_reference_checker_thresholds():
    g, prs = golden_instances("oracle_cfg2.npz"); N = prs[0]["N"]
    for i, pr in enumerate(prs):
        for dx in (0.0, 1e-5, 1e-3):
            x = g["xp"][i].copy(); x[3, N // 2] += dx
            args = (pr["x0"], pr["xF"], N, pr["Ts"], pr["L"], pr["ego"], pr["XYb"], 3, pr["vOb"], pr["A"], pr["b"], x, g["up"][i], g["lp"][i], g["np"][i], np.full(N + 1, g["t"][i]), 0, 1)
            assert V.parking_constraints_ref(*args) == int(V.parking_constraints_ref_worst(*args) <= 5e-5)


def test_shim_and_header_carry_the_new_entry_points():
    jl = open(os.path.join(ROOT, "julia", "OBCAHip.jl")).read()
    for f in ("function ParkingConstraints(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd",
              "function constrSatisfaction(x, u, timeScale, x0, xF, Ts, lambda, ob1, ob2, ob3, ob4, ob5, R", "ParkingConstraints_batch(", "constrSatisfaction_batch("):
        assert f in jl, f
    assert "OBCAHip.constrSatisfaction(" in open(os.path.join(ROOT, "julia", "main_quadcopter.jl")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "obca_hip.h")).read(), flags=re.S)
    for s in ("obca_batch_validate", "obca_batch_validate_ms", "obca_quad_batch_validate", "obca_quad_batch_validate_ms", "obca_parking_constraints_batch",
              "obca_quadcopter_constr_satisfaction_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    from obca_amd.api import EXPORTS
    assert "obca_batch_validate" in EXPORTS and hasattr(__import__("obca_amd"), "parking_constraints_batch") and hasattr(__import__("obca_amd"), "quadcopter_constr_satisfaction_batch")
