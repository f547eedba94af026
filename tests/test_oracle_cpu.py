"""CPU tests of the oracle: known answers, golden fixtures, derivative / linear-algebra cross-checks (no GPU)."""
import ctypes as C
import types
import numpy as np
import pytest
import packing as P
from conftest import golden
from kkt_certificate import DIRECTION_CASES, direction_obstacles, parking_point
from obca_amd import scenarios as S


def test_obst_hrep_known_answers():
    # computed from obstHrep.jl:57-86 and main.jl:102-104,154-157
    A, b, v = S.scenario_hrep(S.BACKWARDS)
    assert A.tolist() == [[0, 1], [1, 0], [-1, 0], [0, 1], [0, -1]] and b.tolist() == [5, -1.3, -1.3, 5, -11] and v.tolist() == [2, 2, 1]
    A, b, v = S.scenario_hrep(S.PARALLEL)
    assert A.tolist() == [[0, 1], [1, 0], [-1, 0], [0, 1], [0, 1], [0, -1]] and b.tolist() == [5, -3, -3, 5, 2.5, -11]
    assert v.tolist() == [2, 2, 1, 1]


def test_obst_hrep_general_edge():
    A, b = S.obst_hrep(1, [3], [[[0, 0], [1, 1], [2, 0]]])     # rising then falling edge, clock-wise
    assert np.allclose(A, [[-1, 1], [1, 1]]) and np.allclose(b, [0, 2])   # y<=x and y<=2-x: the triangle below the apex


def test_dualws_known_answers(oracle, backwards):
    # reference scenario, values verified with SLSQP in the survey session: distance = dual optimum
    d = lambda X, Y, psi: oracle.dualmult_ws(0, backwards["vOb"], backwards["A"], backwards["b"], [X], [Y], [psi], backwards["ego"])[2][0]
    dd = d(-6, 9.5, 0.0)
    assert abs(dd[0] - 3.5) < 1e-6 and abs(dd[2] - 0.5) < 1e-6
    assert abs(d(0, 3, np.pi / 2)[0] - 0.3) < 1e-6
    assert abs(d(2, 8, 0.7)[2]) < 1e-6      # penetrating pose: plain distance is clipped at 0 (lambda = mu = 0 is feasible)


def test_dualws_halfplane_closed_form(oracle):
    g = golden("dualws_known.npz")
    for i in range(len(g["d"])):
        X, Y, psi = g["poses"][i]
        # obstacle {p: a'p <= beta} in the reference's H-rep is written A p <= b
        l, n, d = oracle.dualmult_ws(0, [1], g["a"][i][None, :], [g["beta"][i]], [X], [Y], [psi], S.EGO)
        # the car is OUTSIDE the half-plane obstacle when a'c - support > beta  -> distance = that gap
        assert abs(d[0, 0] - g["d"][i]) < 2e-7, (i, d, g["d"][i])
        assert l.min() >= 0 and n.min() >= 0
        p = g["a"][i] * l[0, 0]
        assert p @ p <= 1 + 1e-9
        cs, sn = np.cos(psi), np.sin(psi)
        assert abs(n[0, 0] - n[0, 2] + cs * p[0] + sn * p[1]) < 1e-9 and abs(n[0, 1] - n[0, 3] - sn * p[0] + cs * p[1]) < 1e-9


def test_oracle_matches_dense_ipm_fixture(oracle, backwards):
    """independent algebra: autograd derivatives + dense LDL^T IPM (fixture) vs closed-form structured oracle"""
    g = golden("dense_N8.npz")
    N = int(g["N"])
    r = oracle.parking_signed_dist(g["x0"], g["xF"], N, float(g["Ts"]), backwards["L"], backwards["ego"], backwards["XYb"],
                                   backwards["vOb"], backwards["A"], backwards["b"], g["xWS"][:, 0], g["xWS"][:, 1], g["xWS"][:, 2],
                                   0, g["xWS"], g["uWS"], g["lWS"], g["nWS"])
    assert str(g["status"]) == "Optimal" and r["exitflag"] == 1
    assert abs(r["obj"] - float(g["obj"])) <= 1e-4 * max(1, abs(float(g["obj"])))
    assert np.abs(r["xp"] - g["xp"]).max() < 1e-3 and np.abs(r["up"] - g["up"]).max() < 1e-3
    assert abs(r["t"] - float(g["t"])) < 1e-4


def test_oracle_optimum_matches_third_party_sqp_fixture(oracle, backwards):
    """the same N=8 NLP solved by scipy's SLSQP (a sequential-quadratic-programming code unrelated to the oracle's interior point):
    same optimum.  The objective is flat along the trajectory (weights 1e-3), hence the looser state tolerance."""
    g = golden("slsqp_N8.npz"); N = int(g["N"])
    assert int(g["status"]) == 0 and float(g["cviol"]) < 1e-10
    r = oracle.parking_signed_dist(g["x0"], g["xF"], N, float(g["Ts"]), backwards["L"], backwards["ego"], backwards["XYb"], backwards["vOb"],
                                   backwards["A"], backwards["b"], g["xWS"][:, 0], g["xWS"][:, 1], g["xWS"][:, 2], 0, g["xWS"], g["uWS"],
                                   g["lWS"], g["nWS"])
    assert r["exitflag"] == 1
    assert abs(r["obj"] - float(g["obj"])) < 1e-4 * abs(float(g["obj"])) and r["obj"] >= float(g["obj"]) - 1e-9   # barrier: from above
    assert np.abs(r["xp"] - g["xp"]).max() < 1e-2 and np.abs(r["up"] - g["up"]).max() < 5e-3 and abs(r["t"] - float(g["t"])) < 1e-5


@pytest.mark.parametrize("name,scn", [("oracle_cfg2.npz", "backwards")])
def test_oracle_reproduces_golden(oracle, name, scn):
    g = golden(name)
    sc = S.BACKWARDS if scn == "backwards" else S.PARALLEL
    B, N = int(g["B"]), int(g["N"])
    bt = S.make_batch(sc, B, N, goal_jitter=(scn == "parallel"))
    for i in range(0, B, 2):
        xWS = bt["xWS"][i].copy(); xWS[0] = bt["x0"][i]
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"],
                                       bt["A"], bt["b"], xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, bt["uWS"][i])
        assert r["exitflag"] == g["exitflag"][i] and r["iters"] == g["iters"][i]
        assert np.abs(r["xp"] - g["xp"][i]).max() < 1e-9 and np.abs(r["up"] - g["up"][i]).max() < 1e-9


def test_reference_checker_accepts_oracle_solutions(oracle):
    from obca_amd import validate as K
    g = golden("oracle_cfg2.npz")
    B, N = int(g["B"]), int(g["N"])
    bt = S.make_batch(S.BACKWARDS, B, N)
    for i in range(B):
        ts = np.full(N + 1, g["t"][i])
        args = (bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], 3, bt["vOb"], bt["A"], bt["b"],
                g["xp"][i], g["up"][i], g["lp"][i], g["np"][i], ts, 0)
        assert K.parking_constraints_ref(*args, 1) == 1                       # ParkingConstraints.jl @ 5e-5
        assert K.feasible(K.parking_constraints_full(*args, g["sl"][i]))       # every row, with the slack
        # free slack settles at -0.005 where the obstacle row is inactive
        assert g["sl"][i].min() > -0.005 - 1e-6


def test_oracle_config3_parallel_parking_golden_and_reference_checker(oracle):
    """BASELINE config 3: the parallel scenario (4 obstacles, main.jl:151-162) from Hybrid A* warm starts stored in the fixture"""
    from obca_amd import validate as K
    g = golden("oracle_cfg3.npz"); B, N = int(g["B"]), int(g["N"])
    A, b, v = S.scenario_hrep(S.PARALLEL)
    assert len(v) == 4 and int(v.sum()) == 6                                   # nOb = 4, M = 6
    for i in range(B):
        xWS = g["xWS"][i]
        r = oracle.parking_signed_dist(g["x0"][i], g["xF"][i], N, g["Ts"][i], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b,
                                       xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, g["uWS"][i])
        assert r["exitflag"] == 1 == g["exitflag"][i] and r["iters"] == g["iters"][i]
        assert np.abs(r["xp"] - g["xp"][i]).max() < 1e-9 and np.abs(r["up"] - g["up"][i]).max() < 1e-9
        ts = np.full(N + 1, r["t"])
        args = (g["x0"][i], g["xF"][i], N, g["Ts"][i], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, 4, v, A, b, r["xp"], r["up"], r["lp"], r["np"], ts, 0)
        assert K.feasible(K.parking_constraints_full(*args, r["sl"]))          # every row of the NLP, with the slack
        assert r["sl"].max() < 0.02                                            # penetration below 2 cm: the bay is 1.3 m longer than the car


# ---------------------------------------------------------------- directions of every obstacle-block class against the dense autograd KKT system
# (formulation, obstacle set of kkt_certificate.direction_obstacles); the shipped scenario keeps the ids it always had
_DIRECTION_PARAMS = [pytest.param(d, c, id=("dist" if d else "signed_dist") + ("" if c == "shipped" else "-" + c)) for c in DIRECTION_CASES for d in (0, 1)]
_DX, _DY, _DLSQ = 1e-9, 1e-8, 1e-9      # relative bounds on the primal part, the multiplier part, the least-squares multipliers
D_ = C.POINTER(C.c_double)
_dp = lambda a: a.ctypes.data_as(D_)


def _direction_problem(case, dist, N, seed):
    """a random interior primal-dual point, far from a solution, of the backwards scenario's start with the obstacle set `case` (rng draws in the order the shipped case always had)"""
    rng = np.random.default_rng(seed)
    v, A, b = direction_obstacles(case); nOb = len(v); M = int(v.sum()); sc = S.BACKWARDS
    x0 = np.array([-6, 9.5, 0.1, 0.]); Ts, xWS, uWS = S.warm_start_backwards(x0, sc["xF"], N); Ts = 0.6
    L = P.layout(N, nOb, M)
    z = np.zeros(L["len"])
    X = xWS.copy(); X[1:] += 0.05 * rng.standard_normal((N, 4)); X[0] = x0
    z[L["x"]:L["x"] + 4 * (N + 1)] = X.reshape(-1)
    z[L["u"]:L["u"] + 2 * N] = np.clip(uWS + 0.05 * rng.standard_normal((N, 2)), -0.3, 0.3).reshape(-1)
    z[L["t"]] = 1.05
    for k, lo, hi in (("lam", 0.1, 1), ("mu", 0.1, 1), ("so", 0.1, 1), ("ss", -0.3, 0.3)):
        n = L[P.LAYOUT_FIELDS[P.LAYOUT_FIELDS.index(k) + 1]] - L[k]
        z[L[k]:L[k] + n] = rng.uniform(lo, hi, n)
    z[L["sl"]:L["so"]] = rng.uniform(0.1, 1, L["so"] - L["sl"]) if dist else 0.01 * rng.standard_normal(L["so"] - L["sl"])
    z[L["pi"]:L["zxL"]] = rng.standard_normal(L["zxL"] - L["pi"])
    z[L["zxL"]:] = rng.uniform(0.1, 2, L["len"] - L["zxL"])
    geo = (N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, 0, x0, sc["xF"], v, A, b, xWS[:, 0], xWS[:, 1], xWS[:, 2])      # the argument list of the oracle's hooks
    return types.SimpleNamespace(case=case, dist=dist, N=N, rng=rng, v=v, A=A, b=b, nOb=nOb, M=M, x0=x0, xF=sc["xF"], Ts=Ts, xWS=xWS, L=L, z=z, geo=geo,
                                 emu=not case.endswith("as_emitted"))      # (the host build packs unit rows: its lambda is the iterate's only for those)


def _dense_parts(q, A=None, hessian=True):
    """the flat restatement at q.z with autograd derivatives (obstacle rows A instead of q.A for the mutation checks): nlp, the maps of iterates / directions to its
    variable and row order, (v, y, zL, zU) with the time scale's multipliers per copy, and f, g, c, J, H"""
    from nlp_ref import ParkingNLP
    xWS = q.xWS
    nlp = ParkingNLP(q.x0, q.xF, q.N, q.Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, q.v, q.A if A is None else A, q.b, xWS[:, 0], xWS[:, 1], xWS[:, 2], dist=q.dist)
    point = lambda w: parking_point(w, q.N, q.v, nlp, q.dist, multiplicity=False)
    vv, y, zL, zU = point(q.z)
    import torch
    vt, yt = torch.tensor(vv), torch.tensor(y); F = torch.autograd.functional      # (vectorised: the 16-obstacle set has 900 variables)
    H = F.hessian(lambda w: nlp.f(w) + (yt * nlp.c(w)).sum(), vt, vectorize=True).numpy() if hessian else None
    d = (nlp.f(vt).item(), F.jacobian(nlp.f, vt).numpy(), nlp.c(vt).numpy(), F.jacobian(nlp.c, vt, vectorize=True).numpy(), H)
    return nlp, (lambda w: point(w)[0]), (lambda w: point(w)[1]), vv, y, zL, zU, d


def _newton_system(q, nlp, vv, y, zL, zU, g, c, J, H, mu, dw, dc):
    """the regularised primal-dual system of Waechter & Biegler (13) at q.z, dense: matrix, right-hand-side gradient part"""
    N, nOb = q.N, q.nOb
    IL = np.isfinite(nlp.lb); IU = np.isfinite(nlp.ub)
    dL = np.where(IL, vv - nlp.lb, 1.0); dU = np.where(IU, nlp.ub - vv, 1.0)
    Sig = nlp.mult * (np.where(IL, zL / dL, 0) + np.where(IU, zU / dU, 0))
    gphi = g - mu * nlp.mult * np.where(IL, 1 / dL, 0) + mu * nlp.mult * np.where(IU, 1 / dU, 0)
    dcv = np.concatenate([np.zeros(4 * N + 4), dc * np.ones(N + 4 * nOb * (N + 1))])   # delta_c only on steering/obstacle rows
    return np.block([[H + np.diag(Sig + dw), J.T], [J, -np.diag(dcv)]]), gphi + J.T @ y


def _emu_newton(emu, q, mu, dw, dc, csoc=None):
    prob = P.pack_problem(q.x0, q.xF, q.N, q.Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, q.v, q.A, q.b, q.xWS[:, 0], q.xWS[:, 1], q.xWS[:, 2], 0, dist=q.dist)
    d = np.zeros_like(q.z); head = (C.c_int(q.N), _dp(prob), _dp(q.z), C.c_int(q.L["len"]), C.c_double(mu), C.c_double(dw), C.c_double(dc), C.c_double(1e3), C.c_double(0.99))
    if csoc is None:
        aux = np.zeros(10)
        return emu.emu_newton(*head, _dp(d), _dp(aux)), d
    return emu.emu_newton_soc(*head, _dp(csoc), _dp(d)), d


@pytest.mark.parametrize("dist,case", _DIRECTION_PARAMS)
def test_newton_direction_vs_dense_autograd(oracle, emu, dist, case):
    """closed-form derivatives + condensation + Riccati + border == dense solve of the autograd KKT system
    (both formulations: ParkingSignedDist and the next-1 sibling ParkingDist), for the oracle AND the kernels' phases (host build), on an obstacle set of every
    instantiation of the obstacle block: 2-row, 3-4-row (two lane rounds of block items) and 5-8-row obstacles"""
    pytest.importorskip("torch")
    q = _direction_problem(case, dist, 4, 1); z, L, rng = q.z, q.L, q.rng
    mu, dw, dc = 0.1, 3.0, 1e-6
    ok, d, errs = oracle.newton(*q.geo, z, mu, dw, dc, dist=dist)
    assert ok == 1
    nlp, to_ref, ym, vv, y, zL, zU, (f, g, c, J, H) = _dense_parts(q)
    n, m = nlp.n, nlp.m
    K, rhs = _newton_system(q, nlp, vv, y, zL, zU, g, c, J, H, mu, dw, dc)
    sol = np.linalg.solve(K, -np.concatenate([rhs, c]))
    ev = np.linalg.eigvalsh(K)
    assert (ev > 0).sum() == n and (ev < 0).sum() == m          # oracle says inertia ok -> dense inertia must be (n,m,0)
    sx, sy = max(1, np.abs(sol[:n]).max()), max(1, np.abs(sol[n:]).max())
    worst = {"oracle": (np.abs(to_ref(d) - sol[:n]).max() / sx, np.abs(ym(d) - sol[n:]).max() / sy)}
    assert worst["oracle"][0] < _DX and worst["oracle"][1] < _DY
    rd = g + J.T @ y - nlp.mult * zL + nlp.mult * zU
    assert abs(errs[0] - np.abs(rd).max()) < 1e-9 * np.abs(rd).max() and abs(errs[1] - np.abs(c).max()) < 1e-12
    # second-order correction: the same matrix, GIVEN constraint values on the right-hand side (c_soc = alpha c(z) + c(trial) in the solver) -- oracle and kernel phases
    csoc = 0.3 * c + 0.05 * rng.standard_normal(m)
    cfull = np.zeros(L["zxL"] - L["pi"]); cfull[:] = csoc          # (pi | nu | yg | yo are contiguous in the layout, in the order of the dense rows)
    sol2 = np.linalg.solve(K, -np.concatenate([rhs, csoc]))
    sx2, sy2 = max(1, np.abs(sol2[:n]).max()), max(1, np.abs(sol2[n:]).max())
    ok2, d2 = oracle.newton_soc(*q.geo, z, mu, dw, dc, cfull, dist=dist)
    worst["oracle soc"] = (np.abs(to_ref(d2) - sol2[:n]).max() / sx2, np.abs(ym(d2) - sol2[n:]).max() / sy2)
    assert ok2 == 1 and worst["oracle soc"][0] < _DX and worst["oracle soc"][1] < _DY
    assert np.abs(sol2[:n] - sol[:n]).max() > 1e-3                 # it is a different step
    if q.emu:
        ok3, d3 = _emu_newton(emu, q, mu, dw, dc, cfull)
        worst["host build soc"] = (np.abs(to_ref(d3) - sol2[:n]).max() / sx2, np.abs(ym(d3) - sol2[n:]).max() / sy2)
        assert ok3 == 1 and worst["host build soc"][0] < _DX and worst["host build soc"][1] < _DY
        ok4, d4 = _emu_newton(emu, q, mu, dw, dc)
        worst["host build"] = (np.abs(to_ref(d4) - sol[:n]).max() / sx, np.abs(ym(d4) - sol[n:]).max() / sy)
        assert ok4 == 1 and worst["host build"][0] < _DX and worst["host build"][1] < _DY
    print("\nNewton direction, %s, dist %d: n %d, m %d, %d block items, inertia (%d, %d, 0); relative deviation from the dense autograd solve (primal, multipliers): %s"
          % (case, dist, n, m, (q.N + 1) * q.nOb, n, m, ", ".join("%s %.1e %.1e" % (k, a, b_) for k, (a, b_) in worst.items())))


@pytest.mark.parametrize("dist,case", _DIRECTION_PARAMS)
def test_least_squares_multipliers_vs_dense_autograd(oracle, emu, dist, case):
    """recalc_y / lsq_init: the least-squares multiplier estimate through the structured solve (unit Hessian on every variable of the reference's model, z-form gradients, zero constraint right-hand
    side) == the dense solve of [I J'; J 0](w, y) = (-(grad f - zL + zU), 0) with autograd derivatives -- for the oracle AND for the kernels' phases (host emulation), at a random
    interior point far from a solution, on an obstacle set of every instantiation of the obstacle block"""
    pytest.importorskip("torch")
    q = _direction_problem(case, dist, 5, 5); z, L = q.z, q.L
    nlp, to_ref, ym, vv, y, zL, zU, (f, g, c, J, H) = _dense_parts(q, hessian=False)      # (the least-squares system has the identity in the Hessian's place)
    n, m = nlp.n, nlp.m
    K = np.block([[np.diag(nlp.mult.astype(float)), J.T], [J, np.zeros((m, m))]])      # identity on every variable of the reference's model: its N + 1 timeScale variables are one t here
    sol = np.linalg.solve(K, -np.concatenate([g - nlp.mult * zL + nlp.mult * zU, np.zeros(m)]))       # y_new = sol[n:] (absolute); the structured solves return y_new - y
    ev = np.linalg.eigvalsh(K)
    ok, d = oracle.lsq_multipliers(*q.geo, z, dist=dist)
    assert ok == 1 and (ev > 0).sum() == n and (ev < 0).sum() == m
    scale = max(1.0, np.abs(sol[n:]).max())
    worst = {"oracle": np.abs(y + ym(d) - sol[n:]).max() / scale}
    assert worst["oracle"] < _DLSQ
    assert np.abs(sol[n:] - y).max() > 0.1                       # far from a solution: the estimate is not the multiplier at hand
    if q.emu:
        prob = P.pack_problem(q.x0, q.xF, q.N, q.Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, q.v, q.A, q.b, q.xWS[:, 0], q.xWS[:, 1], q.xWS[:, 2], 0, dist=dist)
        d2 = np.zeros_like(z)
        assert emu.emu_lsq(C.c_int(q.N), _dp(prob), _dp(z), C.c_int(L["len"]), _dp(d2)) == 1
        worst["host build"] = np.abs(y + ym(d2) - sol[n:]).max() / scale
        assert worst["host build"] < _DLSQ and np.abs(d2[:L["pi"]]).max() == 0 and np.abs(d2[L["zxL"]:]).max() == 0
    print("\nleast-squares multipliers, %s, dist %d: n %d, m %d, inertia (%d, %d, 0); relative deviation from the dense autograd solve: %s"
          % (case, dist, n, m, n, m, ", ".join("%s %.1e" % kv for kv in worst.items())))


@pytest.mark.parametrize("dist", [0, 1], ids=["signed_dist", "dist"])
def test_direction_tests_notice_one_row_entry_off_by_1e_6(oracle, emu, dist):
    """what shows that the two tests above can fail: the dense system with ONE entry of A of a 7-row obstacle changed by 1e-6 -- the structured directions (oracle and host
    build, on the true rows) then miss that dense solution by more than the bounds asserted above"""
    pytest.importorskip("torch")
    mu, dw, dc = 0.1, 3.0, 1e-6
    for N, seed, lsq in ((4, 1, False), (5, 5, True)):
        q = _direction_problem("rows_5_to_8", dist, N, seed)
        r0 = int(np.sum(q.v[:5])); assert q.v[5] == 7
        A = q.A.copy(); A[r0 + 3, 1] += 1e-6
        nlp, to_ref, ym, vv, y, zL, zU, (f, g, c, J, H) = _dense_parts(q, A, hessian=not lsq)
        n, m = nlp.n, nlp.m
        if lsq:
            K = np.block([[np.diag(nlp.mult.astype(float)), J.T], [J, np.zeros((m, m))]])
            sol = np.linalg.solve(K, -np.concatenate([g - nlp.mult * zL + nlp.mult * zU, np.zeros(m)]))
            ok, d = oracle.lsq_multipliers(*q.geo, q.z, dist=dist)
            prob = P.pack_problem(q.x0, q.xF, q.N, q.Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, q.v, q.A, q.b, q.xWS[:, 0], q.xWS[:, 1], q.xWS[:, 2], 0, dist=dist)
            d2 = np.zeros_like(q.z); ok2 = emu.emu_lsq(C.c_int(q.N), _dp(prob), _dp(q.z), C.c_int(q.L["len"]), _dp(d2))
            dev = [np.abs(y + ym(w) - sol[n:]).max() / max(1.0, np.abs(sol[n:]).max()) for w in (d, d2)]
            print("\nleast-squares multipliers against the dense solve with one row entry off by 1e-6, dist %d: oracle %.1e, host build %.1e (bound %.0e)" % (dist, dev[0], dev[1], _DLSQ))
            assert ok == 1 and ok2 == 1 and min(dev) > _DLSQ
        else:
            K, rhs = _newton_system(q, nlp, vv, y, zL, zU, g, c, J, H, mu, dw, dc)
            sol = np.linalg.solve(K, -np.concatenate([rhs, c]))
            ok, d, _ = oracle.newton(*q.geo, q.z, mu, dw, dc, dist=dist); ok2, d2 = _emu_newton(emu, q, mu, dw, dc)
            dev = [(np.abs(to_ref(w) - sol[:n]).max() / max(1, np.abs(sol[:n]).max()), np.abs(ym(w) - sol[n:]).max() / max(1, np.abs(sol[n:]).max())) for w in (d, d2)]
            print("\nNewton direction against the dense solve with one row entry off by 1e-6, dist %d (primal, multipliers): oracle %.1e %.1e, host build %.1e %.1e (bounds %.0e, %.0e)"
                  % (dist, dev[0][0], dev[0][1], dev[1][0], dev[1][1], _DX, _DY))
            assert ok == 1 and ok2 == 1 and all(a > _DX or b_ > _DY for a, b_ in dev)


def test_oracle_fixtime_and_retry_paths(oracle, backwards):
    N = 30
    x0 = np.array([-3.0, 8.5, 0.05, 0.0]); sc = S.BACKWARDS
    Ts, xWS, uWS = S.warm_start_backwards(x0, sc["xF"], N); xWS[0] = x0
    r = oracle.parking_signed_dist(x0, sc["xF"], N, Ts, backwards["L"], backwards["ego"], backwards["XYb"], backwards["vOb"],
                                   backwards["A"], backwards["b"], xWS[:, 0], xWS[:, 1], xWS[:, 2], 1, xWS, uWS)
    assert r["exitflag"] == 1 and np.all(r["timeScale"] == 1.0)
    o = oracle.default_opts(); o.max_iter = 3          # both attempts hit the iteration limit -> exitflag 0 (:256-290)
    r = oracle.parking_signed_dist(x0, sc["xF"], N, Ts, backwards["L"], backwards["ego"], backwards["XYb"], backwards["vOb"],
                                   backwards["A"], backwards["b"], xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, uWS, opts=o)
    assert r["exitflag"] == 0 and r["status"] == 1 and r["iters"] == 6


def test_second_order_correction_and_recalc_y_options(oracle):
    """IPOPT's second-order correction (max_soc = 4, A-5.5 of Waechter & Biegler) and recalc_y = "yes" (ParkingSignedDist.jl:41) exist as oracle options, off by
    default (tools/soc_probe.py is the A/B behind that default: config 5, 512 instances: 506 -> 507 solved, +1.5 % iterations; config 3: -0.7 % iterations;
    recalc_y changes 6 of 768 instances by one iteration).  Here: the options take a different path on some instance of the config-3 distribution and arrive at the
    same optimum."""
    bt = S.make_batch(S.PARALLEL, 16, 80, seed=20260925, goal_jitter=True)
    A, b, v = S.scenario_hrep(S.PARALLEL)
    base, soc = oracle.default_opts(), oracle.default_opts()
    assert base.max_soc == 0 and base.recalc_y == 0
    soc.max_soc = 4; soc.recalc_y = 1
    changed = elsewhere = 0
    for i in range(16):
        xWS = bt["xWS"][i]; a = (bt["x0"][i], bt["xF"][i], 80, bt["Ts"][i], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b, xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, bt["uWS"][i])
        r0 = oracle.parking_signed_dist(*a, opts=base); r1 = oracle.parking_signed_dist(*a, opts=soc)
        assert r0["exitflag"] == 1 and r1["exitflag"] == 1
        changed += r0["iters"] != r1["iters"]
        # (the NLP is non-convex: another iteration path may end in another local solution -- 239 of 1 024 config-3 instances between the option sets, profiles/r05_options_census.txt;
        #  such an instance is counted here, the others must arrive at the same optimum)
        if abs(r0["obj"] - r1["obj"]) <= 1e-5 * abs(r0["obj"]):
            assert np.abs(r0["xp"] - r1["xp"]).max() < 2e-3 and abs(r0["t"] - r1["t"]) < 1e-4
        else:
            elsewhere += 1
    assert changed >= 1 and elsewhere <= 4, (changed, elsewhere)


def test_half_space_rows_of_any_length_describe_the_same_problem(oracle, backwards):
    """a_r.p <= b_r and (s_r a_r).p <= s_r b_r are the same half-plane: the solve runs on unit-length rows (what IPOPT's gradient-based scaling does for the
    reference when obstHrep.jl leaves a steep edge with |a| ~ 1e3) and hands lambda back in the caller's scaling -- states, inputs, iteration count do not depend on
    the row lengths, lambda_r scales with 1 / s_r (A'lambda and b'lambda do not change).  DualMultWS likewise."""
    bt = S.make_batch(S.BACKWARDS, 2, 40, seed=5)
    A, b, v = S.scenario_hrep(S.BACKWARDS)
    s = np.array([250.0, 0.02, 1e3, 7.0, 0.3])
    for i in range(2):
        xWS = bt["xWS"][i]; a = (bt["x0"][i], bt["xF"][i], 40, bt["Ts"][i], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v)
        w = (xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, bt["uWS"][i])
        r0 = oracle.parking_signed_dist(*a, A, b, *w); r1 = oracle.parking_signed_dist(*a, A * s[:, None], b * s, *w)
        assert r0["exitflag"] == r1["exitflag"] == 1 and r0["iters"] == r1["iters"]
        assert np.abs(r0["xp"] - r1["xp"]).max() < 1e-9 and np.abs(r0["up"] - r1["up"]).max() < 1e-9 and abs(r0["obj"] - r1["obj"]) < 1e-9 * abs(r0["obj"])
        assert np.abs(r0["lp"] - r1["lp"] * s[:, None]).max() < 1e-8 * max(1.0, np.abs(r0["lp"]).max())
        l0, n0, d0 = oracle.dualmult_ws(40, v, A, b, xWS[:, 0], xWS[:, 1], xWS[:, 2], S.EGO)
        l1, n1, d1 = oracle.dualmult_ws(40, v, A * s[:, None], b * s, xWS[:, 0], xWS[:, 1], xWS[:, 2], S.EGO)
        assert np.abs(d0 - d1).max() < 1e-10 and np.abs(l0 - l1 * s[None, :]).max() < 1e-9 and np.abs(n0 - n1).max() < 1e-9


@pytest.mark.parametrize("name", ["backwards", "parallel"])
def test_oracle_solves_the_reference_main_jl_call(oracle, name):
    """BASELINE config 1 on the CPU side: warm start of main.jl:216-252 from the REFERENCE-mode search (hybrid_a_star.jl restated, its own point-cloud obstacles),
    horizon from the path length, ParkingDist then ParkingSignedDist; both reach exit flag 1 and the collision-free solution passes the reference's acceptance test"""
    from obca_amd import validate as K
    from obca_amd import planner as PL
    sc = S.BACKWARDS if name == "backwards" else S.PARALLEL
    N, Ts, xWS, uWS, path = PL.reference_warm_start(sc, sc["x0"], sc["xF"])
    assert N == (64 if name == "backwards" else 60)
    A, b, v = S.scenario_hrep(sc); x0, xF = sc["x0"], sc["xF"]
    rx, ry, ryaw = xWS[:, 0].copy(), xWS[:, 1].copy(), xWS[:, 2].copy()
    r20 = oracle.parking_dist(x0, xF, N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b, rx, ry, ryaw, 0, xWS, uWS)
    r10 = oracle.parking_signed_dist(x0, xF, N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b, rx, ry, ryaw, 0, xWS, uWS)
    assert r20["exitflag"] == 1 and r10["exitflag"] == 1
    ts = np.full(N + 1, r20["t"])
    assert K.parking_constraints_ref(x0, xF, N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, len(v), v, A, b, r20["xp"], r20["up"], r20["lp"], r20["np"], ts, 0, 0) == 1


def test_corridor_batch_binding_obstacles_are_well_formed_and_solvable(oracle):
    """scenarios.make_corridor_batch: wedges on the road's two sides (sloped rows through obstHrep), none overlapping a pose of the warm start; the oracle solves the
    instances with the reference's IPOPT configuration and the solutions pass the full checker"""
    from obca_amd import scenarios as S, validate as V
    N, B = 80, 6
    bt = S.make_corridor_batch(B, N, seed=11)
    assert all(len(v) >= 3 and (np.asarray(v) >= 1).all() for v in bt["vOb"]) and max(len(v) for v in bt["vOb"]) > 3
    for i in range(B):
        A, b = bt["A"][i], bt["b"][i]
        assert A.shape == (int(np.sum(bt["vOb"][i])), 2) and np.isfinite(A).all() and np.isfinite(b).all()
        if len(A) > 5:
            assert (np.abs(A[5:]).max(axis=1) > 0).all() and np.any(np.abs(A[5:, 0]) != 0)      # sloped rows [-s 1] / [s -1] (obstHrep.jl:73-86)
        xWS = bt["xWS"][i].copy(); xWS[0] = bt["x0"][i]
        oo = oracle.default_opts(); oo.max_soc = 4; oo.recalc_y = 1; oo.lsq_init = 1; oo.restoration = 1
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"][i], A, b, xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS,
                                       bt["uWS"][i], opts=oo)
        assert r["exitflag"] == 1
        ok, why = V.validate_parking(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], np.ravel(bt["vOb"][i]), A, b, r["xp"], r["up"], r["timeScale"],
                                     r["lp"], r["np"], r["sl"], tol=1e-4)[:2]
        assert ok, why


def test_block_restoration_solves_warm_starts_that_penetrate_the_obstacles():
    """opts.restoration (stand-in for IPOPT's restoration phase, which the reference leans on: ParkingSignedDist.jl:228-231).  DualMultWS returns lambda = mu = 0 at a pose that
    penetrates an obstacle; the signed-distance NLP started there is rank-deficient (|A'lam|^2 = 0 against == 1) and this interior point does not leave it.  Corridor
    instances whose wedges intrude 0.05 / 0.15 m into the warm start's swept body, reference configuration, 64 each: without the restoration 57 / 45 solve, with it (degenerate
    blocks get the feasible dual of their obstacle's best edge) 64 / 64 in fewer iterations; with the mid-solve trigger alone (restoration = 2, a test knob) >= 60.  And it
    changes NOTHING where no block is degenerate: the bench batch of config 2 solves to the same bits with and without."""
    import oracle_pool
    from obca_amd import scenarios as S
    N, B = 80, 64
    for intr, need_on, most_off in ((0.05, 60, 60), (0.15, 50, 50)):
        bt = S.make_corridor_batch(B, N, seed=11, clearance=(-intr, 0.2))
        xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
        off = oracle_pool.mixed_oracle_all(bt, xWS, switches=(4, 1, 1, 0)); on = oracle_pool.mixed_oracle_all(bt, xWS, switches=(4, 1, 1, 1)); mid = oracle_pool.mixed_oracle_all(bt, xWS, switches=(4, 1, 1, 2))
        n_off, n_on, n_mid = (sum(1 for r in x if r[1] == 1) for x in (off, on, mid))
        it_off, it_on = np.mean([r[2] for r in off]), np.mean([r[2] for r in on])
        print("corridor, tips intruding %.2f m: solved %d without / %d with the block restoration (%d with its mid-solve trigger alone) of %d; mean iterations %.0f -> %.0f" % (intr, n_off, n_on, n_mid, B, it_off, it_on))
        assert n_on >= need_on + 2 and n_on > n_off and n_off < most_off and n_mid >= n_on - 6 and it_on < it_off, (intr, n_off, n_on, n_mid)
    bt = S.make_batch(S.BACKWARDS, 64, N)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    a = oracle_pool.parking_oracle_all(bt, xWS, switches=(4, 1, 1, 0)); b = oracle_pool.parking_oracle_all(bt, xWS, switches=(4, 1, 1, 1))
    assert all(x[1] == y[1] == 1 and x[2] == y[2] and x[3] == y[3] and np.array_equal(x[4], y[4]) for x, y in zip(a, b))
