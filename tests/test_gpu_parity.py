"""GPU parity tests (run on the MI355X box with -m gpu).  Every call goes through the C ABI of libobca_hip.so; the oracle is
only the checker.  Tolerances: the HIP path and the oracle implement the same iteration in fp64, so agreement is far inside
the stated parity tolerance (objective 1e-4 rel., states/inputs 1e-3 abs.); the tests assert 1e-6."""
import numpy as np
import pytest
from conftest import golden
from obca_amd import scenarios as S

pytestmark = pytest.mark.gpu
TOL_X, TOL_F = 1e-6, 1e-8


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.Context(0).close()      # fails loudly if the HIP library / device is missing
    return obca_amd


def _census(name, text):
    """the counts the tolerant tests print also go to gpurun_out/ (merged back from the GPU box; the ones to be judged are copied to profiles/)"""
    import os
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_census_%s.txt" % name), "w") as f:
            f.write(text + "\n")
    except OSError:
        pass


def _solve_batch(OA, bt, fixTime=0, lWS=None, nWS=None, opts=None, dist=False):
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    return OA.parking_signed_dist_batch(bt["x0"], bt["xF"], bt["N"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"],
                                        bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], fixTime, xWS, bt["uWS"], lWS, nWS, opts, dist=dist), xWS


def test_dualws_matches_oracle_and_geometry(OA, oracle):
    """the device against the oracle on a scenario batch, and against closed-form answers on 64 single HALF-PLANES (the one shape on which the sub-problem is nearly
    trivial; polygons, at every gap, against exact geometry: tests/test_gpu_dualws_geometry.py)"""
    N, B = 80, 64
    bt = S.make_batch(S.BACKWARDS, B, N)
    xWS = bt["xWS"]
    ls, ns, ds = OA.dualmult_ws_batch(N, bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], bt["ego"])
    for i in range(0, B, 7):
        lo, no, do = oracle.dualmult_ws(N, bt["vOb"], bt["A"], bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], bt["ego"])
        assert np.abs(ds[i] - do).max() < 1e-9 and np.abs(ls[i] - lo).max() < 1e-8 and np.abs(ns[i] - no).max() < 1e-8
    # known answers: single half-plane obstacle = closed-form rectangle/half-plane gap
    g = golden("dualws_known.npz"); n = len(g["d"])
    ls, ns, ds = OA.dualmult_ws_batch(0, [[1]] * n, [a[None, :] for a in g["a"]], [[bb] for bb in g["beta"]],
                                      g["poses"][:, 0:1], g["poses"][:, 1:2], g["poses"][:, 2:3], S.EGO)
    assert np.abs(np.array([d[0, 0] for d in ds]) - g["d"]).max() < 2e-7


def test_parking_matches_oracle_config2(OA, oracle):
    N, B = 80, 16
    bt = S.make_batch(S.BACKWARDS, B, N)
    out, xWS = _solve_batch(OA, bt)
    for i in range(B):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"],
                                       bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i])
        assert out["exitflag"][i] == r["exitflag"] == 1
        assert out["iters"][i] == r["iters"]
        assert abs(out["obj"][i] - r["obj"]) <= TOL_F * max(1, abs(r["obj"]))
        assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and np.abs(out["up"][i] - r["up"]).max() < TOL_X
        assert np.abs(out["timeScale"][i] - r["timeScale"]).max() < 1e-9
        assert np.abs(out["lp"][i] - r["lp"]).max() < 1e-5 and np.abs(out["np"][i] - r["np"]).max() < 1e-5


def test_every_instance_of_the_benchmark_batch_matches_oracle(OA):
    """ALL 1 024 instances of BASELINE config 2 (the batch bench.py times, including the 103-pass straggler, instance 768): exit flag, iteration
    count, regularisation count, objective and trajectory against the oracle (run on all host cores in spawned workers)"""
    import oracle_pool
    N, B = 80, 1024
    bt = S.make_batch(S.BACKWARDS, B, N)
    out, xWS = _solve_batch(OA, bt)
    ref = oracle_pool.parking_oracle_all(bt, xWS)
    assert len(ref) == B and (out["exitflag"] == 1).all()
    worst_x = worst_u = worst_f = 0.0
    for (i, ef, it, obj, xp, up, t) in ref:
        assert out["exitflag"][i] == ef and out["iters"][i] == it, (i, out["iters"][i], it)
        worst_f = max(worst_f, abs(out["obj"][i] - obj) / max(1, abs(obj)))
        worst_x = max(worst_x, np.abs(out["xp"][i] - xp).max()); worst_u = max(worst_u, np.abs(out["up"][i] - up).max())
        assert abs(out["timeScale"][i, 0] - t) < 1e-9
    assert worst_x < TOL_X and worst_u < TOL_X and worst_f < TOL_F, (worst_x, worst_u, worst_f)
    assert out["iters"][768] + out["info"][768, 6] >= 100          # the straggler that ends the synchronous step is among the compared


@pytest.mark.parametrize("N", [33, 101, 128], ids=["odd_horizon", "beyond_the_composed_pairs", "longest_horizon"])
def test_parking_matches_oracle_other_horizons(OA, oracle, N):
    """horizons that exercise the tails of the sweeps: odd N (one leftover stage after the two-stage steps of the forward sweep), N > 96 (more
    stage pairs than the composed-map buffer holds) and OBCA_NMAX itself (every LDS array at its limit)"""
    B = 3
    bt = S.make_batch(S.BACKWARDS, B, N)
    out, xWS = _solve_batch(OA, bt)
    for i in range(B):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"],
                                       bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i])
        assert out["exitflag"][i] == r["exitflag"] == 1 and out["iters"][i] == r["iters"]
        assert abs(out["obj"][i] - r["obj"]) <= TOL_F * max(1, abs(r["obj"]))
        assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and np.abs(out["up"][i] - r["up"]).max() < TOL_X


def test_parking_matches_golden_fixture(OA):
    g = golden("oracle_cfg2.npz")
    B, N = int(g["B"]), int(g["N"])
    bt = S.make_batch(S.BACKWARDS, B, N)
    out, _ = _solve_batch(OA, bt)
    assert np.array_equal(out["exitflag"], g["exitflag"]) and np.array_equal(out["iters"], g["iters"])
    assert np.abs(out["xp"] - g["xp"]).max() < TOL_X and np.abs(out["up"] - g["up"]).max() < TOL_X
    assert np.abs(out["obj"] - g["obj"]).max() < 1e-7


def test_second_order_correction_matches_the_oracle_option(OA, oracle):
    """obca_opts.max_soc = 4 (IPOPT's default second-order correction; off by default here): 64 config-3 instances through the C ABI against the oracle with the same
    option -- exit flags, iteration counts (the corrections change them on about a third of the instances), trajectories."""
    N, B = 80, 64
    bt = S.make_batch(S.PARALLEL, B, N, seed=20260925, goal_jitter=True)
    o = OA.default_opts(); o.max_soc = 4
    out, xWS = _solve_batch(OA, bt, opts=o)
    base, xW0 = _solve_batch(OA, bt)
    oo = oracle.default_opts(); oo.max_soc = 4
    changed = 0
    for i in range(B):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"],
                                       bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i], opts=oo)
        assert out["exitflag"][i] == r["exitflag"] == 1 and out["iters"][i] == r["iters"], (i, out["iters"][i], r["iters"])
        assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and abs(out["obj"][i] - r["obj"]) < TOL_F * abs(r["obj"])
        changed += out["iters"][i] != base["iters"][i]
    assert changed >= 8                                             # the option does something
    with pytest.raises(OA.ObcaError):
        o.max_soc = 99; _solve_batch(OA, bt, opts=o)


def test_recalc_y_matches_the_oracle_option(OA, oracle):
    """obca_opts.recalc_y = 1 (the reference's recalc_y = "yes", ParkingSignedDist.jl:41; off by default here): 48 config-3 instances through the C ABI against the oracle
    with the same option -- exit flags, iteration counts, trajectories; and both switches together (max_soc = 4, recalc_y = 1)."""
    N, B = 80, 48
    bt = S.make_batch(S.PARALLEL, B, N, seed=20260926, goal_jitter=True)
    base, xWS = _solve_batch(OA, bt)
    for soc in (0, 4):
        o = OA.default_opts(); o.recalc_y = 1; o.max_soc = soc
        oo = oracle.default_opts(); oo.recalc_y = 1; oo.max_soc = soc
        out, _ = _solve_batch(OA, bt, opts=o)
        for i in range(B):
            r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"],
                                           bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i], opts=oo)
            assert out["exitflag"][i] == r["exitflag"] == 1 and out["iters"][i] == r["iters"], (soc, i, out["iters"][i], r["iters"])
            assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and abs(out["obj"][i] - r["obj"]) < TOL_F * abs(r["obj"])
        if soc == 0:
            assert (out["xp"] != base["xp"]).any()                  # the option does something (an instance that re-estimates before its last iteration continues from other multipliers)


def test_least_squares_initial_multipliers_match_the_oracle_option(OA, oracle):
    """obca_opts.lsq_init = 1 (IPOPT's default initial multipliers; y0 = 0 by default here): 32 config-3 instances through the C ABI against the oracle with the same option, and
    all three IPOPT switches together (lsq_init, max_soc = 4, recalc_y) -- the reference's IPOPT configuration as far as the kernels carry it."""
    N, B = 80, 32
    bt = S.make_batch(S.PARALLEL, B, N, seed=20260927, goal_jitter=True)
    base, xWS = _solve_batch(OA, bt)
    for soc, rc in ((0, 0), (4, 1)):
        o = OA.default_opts(); o.lsq_init = 1; o.max_soc = soc; o.recalc_y = rc
        oo = oracle.default_opts(); oo.lsq_init = 1; oo.max_soc = soc; oo.recalc_y = rc
        out, _ = _solve_batch(OA, bt, opts=o)
        for i in range(B):
            r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"],
                                           bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i], opts=oo)
            assert out["exitflag"][i] == r["exitflag"] and out["iters"][i] == r["iters"], (soc, rc, i, out["iters"][i], r["iters"])
            if r["exitflag"] == 1:
                assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and abs(out["obj"][i] - r["obj"]) < TOL_F * abs(r["obj"])
        assert (out["iters"] != base["iters"]).sum() >= B // 2          # the initial estimate changes the path of most instances


@pytest.mark.parametrize("dist", [0, 1], ids=["signed_dist", "dist"])
@pytest.mark.parametrize("s_max", [1e-2, 1e-4], ids=["s_max_0.01", "s_max_0.0001"])
def test_termination_scaling_factors_active_on_the_gpu_follow_the_oracle(OA, oracle, s_max, dist):
    """GPU twin of tests/test_emu_cpu.py::test_termination_scaling_factors_in_the_kernels_follow_the_oracle.  IPOPT's s_d, s_c (mean multiplier magnitude over s_max, at
    least 1) scale the optimality error of the termination test (the test ParkingSignedDist.jl:41-43's `tol` belongs to).  With the default s_max = 100 both are 1 on every
    instance of the bench batches, which is why parity never noticed that the parking kernels' multiplier sums were not stored from round 4 to the end of round 5 (DESIGN.md
    section 11).  A small s_max makes them bite: through the C ABI, both option sets, both formulations -- the kernels stop at the oracle's iteration, at the oracle's point."""
    N, B = 40, 24
    bt = S.make_batch(S.BACKWARDS, B, N, seed=7)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    for ref_opts in (0, 1):
        o = OA.ipopt_opts() if ref_opts else OA.default_opts(); o.s_max = s_max
        oo = oracle.default_opts(); oo.s_max = s_max
        if ref_opts:
            oo.max_soc = 4; oo.recalc_y = 1; oo.lsq_init = 1; oo.restoration = 1
        o1 = oracle.default_opts()
        if ref_opts:
            o1.max_soc = 4; o1.recalc_y = 1; o1.lsq_init = 1; o1.restoration = 1
        out = OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0,
                                           xWS, bt["uWS"], opts=o, dist=bool(dist))
        fewer = 0
        for i in range(B):
            a = (bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i])
            r = oracle.parking_signed_dist(*a, opts=oo, dist=dist); r1 = oracle.parking_signed_dist(*a, opts=o1, dist=dist)
            assert out["exitflag"][i] == r["exitflag"] == 1 and out["iters"][i] == r["iters"], (ref_opts, i, out["exitflag"][i], r["exitflag"], out["iters"][i], r["iters"], r1["iters"])
            assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and abs(out["obj"][i] - r["obj"]) < TOL_F * max(1.0, abs(r["obj"]))
            fewer += r["iters"] < r1["iters"]
        assert fewer >= B // 4, (ref_opts, fewer)      # the factors WERE active: with them the oracle itself stops earlier than with s_max = 100


def test_parking_matches_oracle_config3_parallel(OA, oracle):
    """BASELINE config 3: parallel parking, 4 obstacles / 6 half-space rows, Hybrid A* warm starts (golden fixture + a fresh batch)"""
    from obca_amd import validate as K
    g = golden("oracle_cfg3.npz"); B, N = int(g["B"]), int(g["N"])
    A, b, v = S.scenario_hrep(S.PARALLEL)
    fresh = S.make_batch(S.PARALLEL, 32, N, seed=7)                 # (the planner's worker processes are spawned: safe next to a live HIP runtime)
    bt = dict(x0=g["x0"], xF=g["xF"], Ts=g["Ts"], xWS=g["xWS"], uWS=g["uWS"], A=A, b=b, vOb=v, N=N, L=S.L_WHEELBASE, ego=S.EGO, XYbounds=S.XYBOUNDS)
    out, _ = _solve_batch(OA, bt)
    assert (out["exitflag"] == 1).all() and (out["iters"] == g["iters"]).all()
    assert np.abs(out["xp"] - g["xp"]).max() < TOL_X and np.abs(out["up"] - g["up"]).max() < TOL_X
    assert np.abs(out["obj"] - g["obj"]).max() < TOL_F * np.abs(g["obj"]).max()
    bt = fresh
    out, xWS = _solve_batch(OA, bt)
    assert (out["exitflag"] == 1).all()
    for i in range(0, 32, 5):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"],
                                       bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i])
        assert out["exitflag"][i] == r["exitflag"] and out["iters"][i] == r["iters"]
        assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X
    for i in np.where(out["exitflag"] == 1)[0]:
        ts = out["timeScale"][i]
        args = (bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], 4, bt["vOb"], bt["A"], bt["b"],
                out["xp"][i], out["up"][i], out["lp"][i], out["np"][i], ts, 0)
        assert K.feasible(K.parking_constraints_full(*args, out["sl"][i]), tol=1e-4)


def test_parking_dist_variant_matches_oracle(OA, oracle):
    """ParkingDist: no penetration slack, |A'lam|^2 <= 1 with its own slack, 0.5 a^2, its own exit-flag logic"""
    from obca_amd import validate as K
    N, B = 80, 48
    bt = S.make_batch(S.BACKWARDS, B, N)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    out = OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"],
                                       xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"], dist=True)
    assert (out["exitflag"] == 1).all()
    for i in range(0, B, 6):
        r = oracle.parking_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"],
                                xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i])
        assert r["exitflag"] == 1 and out["iters"][i] == r["iters"]
        assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and np.abs(out["up"][i] - r["up"]).max() < TOL_X
        assert abs(out["obj"][i] - r["obj"]) < TOL_F * abs(r["obj"])
    for i in range(B):      # collision-free: every separation row holds without any slack; the reference's own acceptance test (sd = 0) passes
        ts = out["timeScale"][i]
        args = (bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], 3, bt["vOb"], bt["A"], bt["b"],
                out["xp"][i], out["up"][i], out["lp"][i], out["np"][i], ts, 0)
        assert K.parking_constraints_ref(*args, 0) == 1
        viol = K.parking_constraints_full(*args, np.zeros_like(out["sl"][i]))
        assert viol["penetration"] <= 1e-6
    # single-instance wrapper and the exit-flag quirk after two failed attempts (ParkingDist.jl:277-282)
    xp, up, ts, ef, t, lp, npp = OA.ParkingDist(bt["x0"][0], bt["xF"][0], N, bt["Ts"][0], bt["L"], bt["ego"], bt["XYbounds"], 3, bt["vOb"],
                                               bt["A"], bt["b"], xWS[0, :, 0], xWS[0, :, 1], xWS[0, :, 2], 0, xWS[0], bt["uWS"][0], opts=OA.default_opts())
    assert ef == 1 and np.abs(xp - out["xp"][0]).max() < 1e-12
    # ... and with its own default, the reference's IPOPT configuration (ParkingDist.jl:41: recalc_y = "yes"; IPOPT's second-order correction and least-squares start): against the
    # oracle with the same three options
    xp, up, ts, ef, t, lp, npp = OA.ParkingDist(bt["x0"][0], bt["xF"][0], N, bt["Ts"][0], bt["L"], bt["ego"], bt["XYbounds"], 3, bt["vOb"],
                                               bt["A"], bt["b"], xWS[0, :, 0], xWS[0, :, 1], xWS[0, :, 2], 0, xWS[0], bt["uWS"][0])
    oo = oracle.default_opts(); oo.max_soc = 4; oo.recalc_y = 1; oo.lsq_init = 1; oo.restoration = 1
    r = oracle.parking_dist(bt["x0"][0], bt["xF"][0], N, bt["Ts"][0], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"],
                            xWS[0, :, 0], xWS[0, :, 1], xWS[0, :, 2], 0, xWS[0], bt["uWS"][0], opts=oo)
    assert ef == r["exitflag"] == 1 and np.abs(xp - r["xp"]).max() < TOL_X
    o = OA.default_opts(); o.max_iter = 3
    bad = OA.parking_signed_dist_batch(bt["x0"][:4], bt["xF"][:4], N, bt["Ts"][:4], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"],
                                       bt["b"], xWS[:4, :, 0], xWS[:4, :, 1], xWS[:4, :, 2], 0, xWS[:4], bt["uWS"][:4], opts=o, dist=True)
    assert (bad["status"] == 1).all() and (bad["iters"] == 6).all() and (bad["exitflag"] == 1).all()


def test_full_size_properties_config2(OA):
    """B=1024 (BASELINE config 2): size-independent properties -- every converged instance passes the reference's own
    acceptance test (ParkingConstraints.jl @5e-5) and the full checker; boundary conditions hold exactly; solving twice is
    deterministic."""
    from obca_amd import validate as K
    N, B = 80, 1024
    bt = S.make_batch(S.BACKWARDS, B, N)
    out, _ = _solve_batch(OA, bt)
    ok = out["exitflag"] == 1
    assert ok.all()
    assert np.abs(out["xp"][:, :, 0] - bt["x0"]).max() == 0.0
    assert np.abs(out["xp"][ok][:, :, N] - bt["xF"][ok]).max() < 5e-5
    for i in np.flatnonzero(ok)[::8]:
        args = (bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], 3, bt["vOb"], bt["A"], bt["b"],
                out["xp"][i], out["up"][i], out["lp"][i], out["np"][i], out["timeScale"][i], 0)
        viol = K.parking_constraints_full(*args, out["sl"][i])
        assert K.feasible(viol, tol=1e-4), (i, viol)      # every row incl. the slack, at IPOPT's constr_viol_tol
        if viol["penetration"] <= 0:                      # ParkingConstraints.jl ignores the slack (Q5): it can only pass when
            assert K.parking_constraints_ref(*args, 1) == 1, i   # no pose (incl. the fixed start pose) needs positive slack
    for rep in range(12):       # race detector: the lanes of an instance exchange state through LDS (wave-level ordering only, LDS atomics for the obstacle sums); repeated solves are bit-identical
        out2, _ = _solve_batch(OA, bt)
        assert np.array_equal(out["iters"], out2["iters"]) and np.abs(out["xp"] - out2["xp"]).max() == 0.0, rep


def test_two_launch_schedule_is_bit_identical_to_a_single_launch(OA, monkeypatch):
    """B=1536 exceeds the resident capacity (4 one-wavefront instances per CU = 1024), so obca_batch_solve uses the two-launch schedule (slice, rank, finish
    hardest-first).  Parking a solve and resuming it must not change a single bit of any output; an odd slice length also cuts solves inside
    their inertia-retry sequence and right before convergence."""
    N, B = 80, 1536
    bt = S.make_batch(S.BACKWARDS, B, N)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    ctx = OA.Context(0); b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    monkeypatch.setenv("OBCA_SLICE_PASSES", "0")
    b.solve(); ref = b.download(); assert b.last_schedule() == (1, 0)
    for q in (6, 1, 27):
        monkeypatch.setenv("OBCA_SLICE_PASSES", str(q))
        b.solve(); out = b.download(); assert b.last_schedule() == (2, q)
        for k in ("xp", "up", "timeScale", "lp", "np", "sl", "info", "exitflag"):
            assert np.array_equal(ref[k], out[k]), (q, k)
    b.close(); ctx.close()


def test_batches_in_flight_on_several_contexts_do_not_interfere(OA):
    """the deployment pattern of INTEGRATION.md / bench.py: several contexts (one HIP stream each), each with its own batch, solves submitted
    round-robin without synchronising in between.  Every batch must come out exactly as when it is solved alone."""
    N, B = 80, 640                      # > 512: the two-launch schedule is active, its ordering kernel and slice records are per batch
    bts = [S.make_batch(S.BACKWARDS, B, N, seed=100 + i) for i in range(3)]
    ctxs = [OA.Context(0) for _ in bts]; bs = []
    for ctx, bt in zip(ctxs, bts):
        xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
        b = OA.Batch(ctx, B, N)
        b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
        bs.append(b)
    alone = []
    for b in bs:
        b.solve(); alone.append(b.download())
    for rep in range(3):
        for b in bs:
            b.solve(sync=False)
    for b in bs:
        b.sync()
    for i, b in enumerate(bs):
        out = b.download()
        for k in ("xp", "up", "timeScale", "lp", "np", "sl", "info", "exitflag"):
            assert np.array_equal(alone[i][k], out[k]), (i, k)
        assert (out["exitflag"] == 1).mean() > 0.97
    for b in bs:
        b.close()
    for c in ctxs:
        c.close()


def test_single_instance_wrapper_and_shapes(OA, oracle, backwards):
    N = 40; sc = S.BACKWARDS; x0 = sc["x0"]
    Ts, xWS, uWS = S.warm_start_backwards(x0, sc["xF"], N); xWS[0] = x0
    xp, up, ts, ef, tm, lp, npp = OA.ParkingSignedDist(x0, sc["xF"], N, Ts, backwards["L"], backwards["ego"], backwards["XYb"], 3,
                                                       backwards["vOb"], backwards["A"], backwards["b"], xWS[:, 0], xWS[:, 1], xWS[:, 2],
                                                       0, xWS, uWS)
    assert xp.shape == (4, N + 1) and up.shape == (2, N) and ts.shape == (N + 1,) and lp.shape == (5, N + 1) and npp.shape == (12, N + 1)
    oo = oracle.default_opts(); oo.max_soc = 4; oo.recalc_y = 1; oo.lsq_init = 1; oo.restoration = 1      # the drop-in's default IS the reference's IPOPT configuration (obca_reference_opts)
    r = oracle.parking_signed_dist(x0, sc["xF"], N, Ts, backwards["L"], backwards["ego"], backwards["XYb"], backwards["vOb"],
                                   backwards["A"], backwards["b"], xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, uWS, opts=oo)
    assert ef == r["exitflag"] == 1 and np.abs(xp - r["xp"]).max() < TOL_X and tm > 0
    xq = OA.ParkingSignedDist(x0, sc["xF"], N, Ts, backwards["L"], backwards["ego"], backwards["XYb"], 3, backwards["vOb"], backwards["A"], backwards["b"], xWS[:, 0], xWS[:, 1],
                              xWS[:, 2], 0, xWS, uWS, opts=OA.default_opts())[0]      # the throughput defaults: the oracle's defaults
    r0 = oracle.parking_signed_dist(x0, sc["xF"], N, Ts, backwards["L"], backwards["ego"], backwards["XYb"], backwards["vOb"],
                                    backwards["A"], backwards["b"], xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, uWS)
    assert np.abs(xq - r0["xp"]).max() < TOL_X
    l1, n1 = OA.DualMultWS(N, 3, backwards["vOb"], backwards["A"], backwards["b"], xWS[:, 0], xWS[:, 1], xWS[:, 2], backwards["ego"])
    assert l1.shape == (N + 1, 5) and n1.shape == (N + 1, 12)          # DualMultWS.jl:81-84 returns the transposed shapes


def test_fixtime_and_supplied_duals(OA, oracle):
    N, B = 30, 6
    bt = S.make_batch(S.BACKWARDS, B, N, seed=5)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    duals = [oracle.dualmult_ws(N, bt["vOb"], bt["A"], bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], bt["ego"]) for i in range(B)]
    out, _ = _solve_batch(OA, bt, fixTime=1, lWS=[d[0] for d in duals], nWS=[d[1] for d in duals])
    assert np.all(out["timeScale"] == 1.0)
    for i in range(B):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"],
                                       bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 1, xWS[i], bt["uWS"][i], duals[i][0], duals[i][1])
        assert out["exitflag"][i] == r["exitflag"] and out["iters"][i] == r["iters"]
        if r["exitflag"]:
            assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X


def test_mixed_obstacle_counts_ragged_batch(OA, oracle):
    """per-instance obstacle sets of different size in ONE batch (irregular H-rep packing)"""
    N = 40; full = S.scenario_hrep(S.BACKWARDS)
    A, b, v = full
    sets = [([2, 2, 1], A, b), ([2, 2], A[:4], b[:4]), ([1], A[4:5], b[4:5]), ([2, 1], np.vstack([A[:2], A[4:5]]), np.concatenate([b[:2], b[4:5]]))]
    B = 8
    bt = S.make_batch(S.BACKWARDS, B, N, seed=11)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    vl = [sets[i % 4][0] for i in range(B)]; Al = [sets[i % 4][1] for i in range(B)]; bl = [sets[i % 4][2] for i in range(B)]
    out = OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], vl, Al, bl,
                                       xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    for i in range(B):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], vl[i], Al[i], bl[i],
                                       xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i])
        assert out["lp"][i].shape == (sum(vl[i]), N + 1) and out["np"][i].shape == (4 * len(vl[i]), N + 1)
        assert out["exitflag"][i] == r["exitflag"] and out["iters"][i] == r["iters"]
        if r["exitflag"]:
            assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X


def test_ordered_obstacle_sums_across_round_boundaries_follow_the_oracle(OA, oracle):
    """The GPU build of obs_sum_ordered (a running sum that walks down the lanes of a stage with wave_shr:1 moves, continued across the rounds of 64 items) has no twin in the host
    emulation, whose PAR loop cannot shift between lanes (advisor, round 5).  So it is pinned here, end to end: instances with 3, 5, 7, 10, 13 and 16 obstacles at horizons where
    (N + 1) nOb is not a multiple of 64 -- stages straddle round boundaries at every possible position, the last round is partial -- against the oracle, iteration for iteration:
    a wrong or mis-ordered obstacle sum changes the Newton direction of its stage and with it every iterate."""
    seen = set()
    for N, seed in ((20, 3), (37, 4), (50, 5), (64, 6)):
        bt = S.make_mixed_batch(40, N, seed=seed, min_obstacles=1, max_extra=13, rows=(3, 4), max_rows=64)
        pick = {}
        for i, v in enumerate(bt["vOb"]):
            n = len(v)
            if n in (3, 5, 7, 10, 13, 16) and n not in pick and ((N + 1) * n) % 64 != 0: pick[n] = i
        idx = sorted(pick.values()); assert len(idx) >= 3, (N, pick)
        sub = {k: ([v[i] for i in idx] if isinstance(v, list) else (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == 40 else v)) for k, v in bt.items()}
        out, xWS = _solve_batch(OA, dict(sub, N=N))
        for q, i in enumerate(idx):
            r = oracle.parking_signed_dist(sub["x0"][q], sub["xF"][q], N, sub["Ts"][q], sub["L"], sub["ego"], sub["XYbounds"], sub["vOb"][q], sub["A"][q], sub["b"][q],
                                           xWS[q, :, 0], xWS[q, :, 1], xWS[q, :, 2], 0, xWS[q], sub["uWS"][q])
            assert out["exitflag"][q] == r["exitflag"] == 1 and out["iters"][q] == r["iters"], (N, len(sub["vOb"][q]), out["iters"][q], r["iters"])
            assert np.abs(out["xp"][q] - r["xp"]).max() < TOL_X and abs(out["obj"][q] - r["obj"]) < TOL_F * max(1.0, abs(r["obj"]))
            seen.add(len(sub["vOb"][q]))
    assert len(seen) >= 5, seen


@pytest.mark.timeout(900)
def test_random_problems_on_the_gpu_follow_the_oracle(OA, oracle):
    """GPU twin of tests/test_emu_cpu.py::test_random_problems_the_kernels_follow_the_oracle: 60 seeded random draws of (horizon 10-100, backwards / parallel / 1-16 obstacles of
    up to 8 rows, formulation, fixed or variable time, option set incl. the block restoration), 6 instances each, through the C ABI against the oracle: exit flags equal, iteration
    counts equal on all but a handful (knife edges; their solves must end at the oracle's objective), trajectories to 1e-6 where the counts agree."""
    off = []; flat = []; worst = 0.0; solved = 0; total = 0
    for seed in range(3000, 3060):
        rng = np.random.default_rng(seed)
        N = int(rng.choice([10, 20, 33, 48, 64, 80, 100])); kind = int(rng.integers(0, 3)); dist = bool(rng.integers(0, 2)) if kind != 2 else False; fix = int(rng.integers(0, 4) == 0)
        ref = bool(rng.integers(0, 2)); B = 6
        if kind == 2:
            bt = S.make_mixed_batch(B, N, seed=int(rng.integers(1, 10000)), min_obstacles=1, max_extra=int(rng.choice([7, 13])), rows=(3, 8) if rng.integers(0, 2) else (3, 4), max_rows=64)
        else:
            bt = S.make_batch(S.BACKWARDS if kind == 0 else S.PARALLEL, B, N, seed=int(rng.integers(1, 10000)))
        xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]; Ts = np.broadcast_to(bt["Ts"], (B,))
        o = OA.ipopt_opts() if ref else OA.default_opts()
        out = OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, Ts, bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], fix, xWS, bt["uWS"],
                                           opts=o, dist=dist)
        oo = oracle.default_opts()
        if ref:
            oo.max_soc = 4; oo.recalc_y = 1; oo.lsq_init = 1; oo.restoration = 1
        for i in range(B):
            v, A, b = (bt["vOb"][i], bt["A"][i], bt["b"][i]) if kind == 2 else (bt["vOb"], bt["A"], bt["b"])
            r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, float(Ts[i]), bt["L"], bt["ego"], bt["XYbounds"], v, A, b, xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], fix, xWS[i], bt["uWS"][i],
                                           opts=oo, dist=int(dist))
            total += 1
            assert int(out["exitflag"][i]) == r["exitflag"], (seed, i, N, kind, dist, fix, ref, int(out["exitflag"][i]), r["exitflag"])
            if int(out["iters"][i]) != r["iters"]:
                off.append((seed, i, int(out["iters"][i]), r["iters"]))
                if r["exitflag"] == 1: assert abs(out["obj"][i] - r["obj"]) < 1e-4 * max(1.0, abs(r["obj"])), off[-1]
            elif r["exitflag"] == 1 and r["status"] == 0 and int(out["info"][i, 0]) == 0:      # (an exit flag 1 that the reference's own acceptance test grants after a failed attempt is not a converged point)
                dx = float(np.abs(out["xp"][i] - r["xp"]).max()); df = abs(out["obj"][i] - r["obj"]) / max(1.0, abs(r["obj"])); solved += 1
                if dx >= TOL_X:      # a long solve around a flat optimum: the same iterations, the points apart within the path's stated tolerance -- counted, bounded
                    flat.append((seed, i, N, r["iters"], dx, df)); assert dx < 1e-3 and df < 2e-4, flat[-1]
                else: worst = max(worst, dx)
    msg = ("random problems on the GPU against the oracle: %d instances in 60 draws, exit flags equal on all, %d converged with equal iteration counts (worst |dx| %.2e; flat-optimum instances "
           "within the stated tolerance: %s), iteration counts differ on %s" % (total, solved, worst, flat, off))
    print(msg); _census("random_problems", msg)
    assert len(off) <= 4 and len(flat) <= 3 and solved >= 0.9 * total and worst < TOL_X, msg


def test_config5_mixed_obstacle_counts_up_to_the_limits(OA, oracle):
    """BASELINE config 5 (reduced batch): 3..10 obstacles with 1..4 half-space rows each per instance, M up to 33, in ONE launch"""
    N, B = 80, 96
    bt = S.make_mixed_batch(B, N)
    assert max(len(v) for v in bt["vOb"]) == 10 and max(int(v.max()) for v in bt["vOb"]) == 4 and min(len(v) for v in bt["vOb"]) == 3
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    out = OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"],
                                       xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    assert (out["exitflag"] == 1).all()                   # (every instance converges since the half-space rows enter with unit length)
    for i in range(0, B, 9):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"][i], bt["A"][i],
                                       bt["b"][i], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i])
        assert r["exitflag"] == 1 == out["exitflag"][i]
        assert out["iters"][i] == r["iters"] and np.abs(out["xp"][i] - r["xp"]).max() < TOL_X
        assert out["lp"][i].shape == (int(bt["vOb"][i].sum()), N + 1) and np.abs(out["lp"][i] - r["lp"]).max() < 1e-5


def test_receding_horizon_restart_on_the_device(OA, oracle):
    """next-4: the previous solution advanced by `shift` stages becomes the warm start of the next solve without leaving the GPU;
    the oracle started from the same (host-built) shifted warm start takes the same iterations to the same trajectory"""
    N, B, sh = 80, 16, 8
    bt = S.make_batch(S.BACKWARDS, B, N)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = OA.Batch(OA.Context(0), B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    b.solve(); o1 = b.download()
    assert (o1["exitflag"] == 1).all()
    wo = OA.warm_restart_opts()                                  # small initial barrier / bound push: the standard interior-point warm start
    b.shift_warm_start(sh); b.solve(wo); o2 = b.download()
    assert (o2["exitflag"] == 1).all() and o2["iters"].mean() < 0.75 * o1["iters"].mean()      # a warm restart is cheaper than the cold solve
    oo = oracle.default_opts(); oo.mu_init = wo.mu_init; oo.bound_push = wo.bound_push; oo.bound_frac = wo.bound_frac
    idx = np.minimum(np.arange(N + 1) + sh, N); iu = np.minimum(np.arange(N) + sh, N - 1)
    for i in range(0, B, 5):
        xw = o1["xp"][i].T[idx]; uw = o1["up"][i].T[iu].copy(); uw[np.arange(N) + sh > N - 1, 1] = 0.0
        r = oracle.parking_signed_dist(xw[0], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"],
                                       xWS[i, idx, 0], xWS[i, idx, 1], xWS[i, idx, 2], 0, xw, uw, o1["lp"][i].T[idx], o1["np"][i].T[idx], opts=oo)
        assert r["exitflag"] == 1 and r["iters"] == o2["iters"][i]
        assert np.abs(r["xp"] - o2["xp"][i]).max() < TOL_X and np.abs(o2["xp"][i][:, 0] - o1["xp"][i][:, sh]).max() == 0.0
    # a measured state instead of the predicted one
    x0n = o2["xp"][:, :, 4].copy(); x0n[:, 0] += 0.02
    b.shift_warm_start(4, x0n); b.solve(wo); o3 = b.download()
    assert (o3["exitflag"] == 1).all() and np.abs(o3["xp"][:, :, 0] - x0n).max() == 0.0
    b.close()


def test_bad_inputs_fail_loudly_not_crash(OA):
    N = 10; bt = S.make_batch(S.BACKWARDS, 2, N)
    xWS = bt["xWS"].copy()
    with pytest.raises(OA.ObcaError):      # 9 rows in one obstacle > OBCA_VMAX
        OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], [9], np.zeros((9, 2)), np.zeros(9),
                                     xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    with pytest.raises(OA.ObcaError):      # 10 x 7 = 70 rows in one instance > OBCA_MMAX
        OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], [7] * 10, np.ones((70, 2)), np.zeros(70),
                                     xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    with pytest.raises(OA.ObcaError):      # 17 obstacles > OBCA_NOBMAX
        OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], [1] * 17, np.ones((17, 2)), np.zeros(17),
                                     xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    with pytest.raises(OA.ObcaError):      # objective scaling is a switch of the quadcopter kernel: refused on the parking path, not ignored
        o = OA.default_opts(); o.obj_scaling = 1
        OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS,
                                     bt["uWS"], opts=o)
    bad = bt["x0"].copy(); bad[0, 0] = np.nan  # NaN input: exitflag 0 for that instance, the other one still solves
    out = OA.parking_signed_dist_batch(bad, bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"],
                                       xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    assert out["exitflag"][0] == 0 and out["exitflag"][1] in (0, 1)


def test_iteration_limit_and_retry_exitflag(OA, oracle):
    N, B = 30, 4
    bt = S.make_batch(S.BACKWARDS, B, N, seed=3)
    o = OA.default_opts(); o.max_iter = 3
    out, _ = _solve_batch(OA, bt, opts=o)
    assert np.all(out["exitflag"] == 0) and np.all(out["iters"] == 6) and np.all(out["status"] == 1)   # two attempts (:256-290)


def test_wide_obstacles_up_to_eight_rows(OA, oracle):
    """polygons with 5..8 edges (OBCA_VMAX = 8; obstHrep.jl:31-102 emits one row per edge): the widest instantiation of the block code and of
    the DualMultWS kernel through the C ABI against the oracle, in one batch with narrow instances (per-instance dispatch of the block size)"""
    N, B = 40, 24
    bt = S.make_mixed_batch(B, N, seed=11, rows=(5, 8), max_extra=4)
    assert max(int(np.max(v)) for v in bt["vOb"]) >= 7 and min(int(np.max(v)) for v in bt["vOb"]) == 2
    out, xWS = _solve_batch(OA, dict(bt, N=N))
    ls, ns, ds = OA.dualmult_ws_batch(N, bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], bt["ego"])
    assert (out["exitflag"] == 1).all()
    n = 0
    for i in range(B):
        if np.max(bt["vOb"][i]) <= 4 and i % 4:
            continue
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"][i], bt["A"][i],
                                       bt["b"][i], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i])
        lo, no, do = oracle.dualmult_ws(N, bt["vOb"][i], bt["A"][i], bt["b"][i], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], bt["ego"])
        assert np.abs(ds[i] - do).max() < 1e-9 and np.abs(ls[i] - lo).max() < 1e-7
        assert out["exitflag"][i] == r["exitflag"] and out["iters"][i] == r["iters"]
        if r["exitflag"] == 1:
            assert abs(out["obj"][i] - r["obj"]) <= TOL_F * max(1, abs(r["obj"])) and np.abs(out["xp"][i] - r["xp"]).max() < TOL_X
        n += 1
    assert n >= 8


def test_ipopt_switches_on_wide_obstacles_match_the_oracle_options(OA, oracle):
    """max_soc = 4, recalc_y and lsq_init together on a ragged batch with 2- to 8-row obstacles: every row-class instantiation of the correction and least-squares phases
    through the C ABI against the oracle with the same options"""
    N, B = 40, 24
    bt = S.make_mixed_batch(B, N, seed=11, rows=(5, 8), max_extra=4)
    o = OA.default_opts(); o.max_soc = 4; o.recalc_y = 1; o.lsq_init = 1; o.restoration = 1
    oo = oracle.default_opts(); oo.max_soc = 4; oo.recalc_y = 1; oo.lsq_init = 1; oo.restoration = 1
    out, xWS = _solve_batch(OA, dict(bt, N=N), opts=o)
    base, _ = _solve_batch(OA, dict(bt, N=N))
    for i in range(B):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"][i], bt["A"][i],
                                       bt["b"][i], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i], opts=oo)
        assert out["exitflag"][i] == r["exitflag"] and out["iters"][i] == r["iters"], (i, out["iters"][i], r["iters"])
        if r["exitflag"] == 1:
            assert abs(out["obj"][i] - r["obj"]) <= TOL_F * max(1, abs(r["obj"])) and np.abs(out["xp"][i] - r["xp"]).max() < TOL_X
    assert (out["iters"] != base["iters"]).sum() >= B // 2


def test_hip_reproduces_the_independently_certified_solutions(OA):
    """tests/golden/kkt_pin.npz: solutions whose optimality is certified with independent (autograd) derivatives at the benchmark size (test_pin_cpu.py):
    the HIP path must return the same arrays -- config 2 and config 3 at N = 80, quadcopter at N = 60 -- without the oracle at run time"""
    recs = list(golden("kkt_pin.npz")["records"])
    for tag, sc in (("cfg2", S.BACKWARDS), ("cfg3", S.PARALLEL)):
        rs = [r for r in recs if r["tag"] == tag]; A, b, v = S.scenario_hrep(sc); N = rs[0]["xp"].shape[1] - 1
        bt = dict(x0=np.stack([r["x0"] for r in rs]), xF=np.stack([r["xF"] for r in rs]), Ts=np.array([float(r["Ts"]) for r in rs]), xWS=np.stack([r["xWS"] for r in rs]),
                  uWS=np.stack([r["uWS"] for r in rs]), A=A, b=b, vOb=v, N=N, L=S.L_WHEELBASE, ego=S.EGO, XYbounds=S.XYBOUNDS)
        out, _ = _solve_batch(OA, bt)
        for i, r in enumerate(rs):
            assert out["exitflag"][i] == 1 and out["iters"][i] == r["iters"], (tag, i)
            assert abs(out["obj"][i] - r["oracle_obj"]) <= TOL_F * max(1, abs(r["oracle_obj"]))
            assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and np.abs(out["up"][i] - r["up"]).max() < TOL_X and abs(out["timeScale"][i, 0] - r["t"]) < 1e-9
    rs = [r for r in recs if r["tag"] == "quad"]; N = rs[0]["xp"].shape[1] - 1
    out = OA.quadcopter_signed_dist_batch(np.stack([r["x0"] for r in rs]), np.stack([r["xF"] for r in rs]), N, float(rs[0]["Ts"]), float(rs[0]["R"]), rs[0]["ob"],
                                          np.stack([r["xWS"] for r in rs]), np.ones(len(rs)))
    for i, r in enumerate(rs):
        assert out["exitflag"][i] == 1 and abs(out["obj"][i] - r["oracle_obj"]) <= 1e-8 * abs(r["oracle_obj"])
        assert np.abs(out["up"][i] - r["up"]).max() < 1e-5 and abs(out["timeScale"][i, 0] - r["t"]) < 1e-8 and np.abs(out["xp"][i] - r["xp"]).max() < 1e-3


def test_hip_reproduces_the_certified_solutions_of_the_kernel_text(OA):
    """tests/golden/kkt_classes.npz: the final iterates of the host build of the kernel text at N = 20, certified with independent (autograd) derivatives by
    tests/test_kkt_classes_cpu.py -- ParkingSignedDist and ParkingDist, obstacles of up to 7 rows, both option sets, solves in which the block restoration fired.  The HIP path
    must return the same arrays without the oracle at run time: records grouped by formulation and option set into ragged batches, exit flag, iteration count and the point
    (TOL_X / TOL_F).  For the restoration records the iteration count is printed, not asserted, and the solve with restoration = 0 must be another run, longer or shorter as
    the fixture says."""
    import kkt_classes_common as K
    recs = [r for r in golden("kkt_classes.npz")["records"] if not K.is_quad(r)]
    groups = {}
    for r in recs:
        groups.setdefault((r["dist"], r["ref"], r["restoration"]), []).append(r)
    assert len(recs) == 15 and max(len(g) for g in groups.values()) <= 8
    lines = []
    for (dist, ref, rest), rs in sorted(groups.items()):
        bt = dict(x0=np.stack([r["x0"] for r in rs]), xF=np.stack([r["xF"] for r in rs]), Ts=np.array([float(r["Ts"]) for r in rs]), xWS=np.stack([r["xWS"] for r in rs]),
                  uWS=np.stack([r["uWS"] for r in rs]), A=[r["A"] for r in rs], b=[r["b"] for r in rs], vOb=[r["vOb"] for r in rs], N=K.N, L=S.L_WHEELBASE, ego=S.EGO, XYbounds=S.XYBOUNDS)
        o = OA.ipopt_opts() if ref else OA.default_opts(); o.restoration = rest
        out, _ = _solve_batch(OA, bt, opts=o, dist=bool(dist))
        if rest:
            o0 = OA.ipopt_opts(); o0.restoration = 0
            out0, _ = _solve_batch(OA, bt, opts=o0, dist=bool(dist))
        for i, r in enumerate(rs):
            tag = K.name(r); fired = r["tag"] == "corridor"
            dx = max(np.abs(out["xp"][i] - r["xp"]).max(), np.abs(out["up"][i] - r["up"]).max()); df = abs(out["obj"][i] - r["solver_obj"]) / max(1, abs(r["solver_obj"]))
            lines.append("%s: exit flag %d, %d iterations (fixture %d), largest deviation of states / inputs %.1e, objective %.1e relative%s"
                         % (tag, out["exitflag"][i], out["iters"][i], r["iters"], dx, df, ", %d iterations with restoration = 0 (fixture %d)" % (out0["iters"][i], r["rest0_iters"]) if fired else ""))
            print(lines[-1])
            assert out["exitflag"][i] == r["exitflag"] == 1, tag
            if fired:
                assert out0["iters"][i] != out["iters"][i] and (out0["iters"][i] > out["iters"][i]) == (r["rest0_iters"] > r["iters"]), tag
            else:
                assert out["iters"][i] == r["iters"], tag
            assert df <= TOL_F and dx < TOL_X and abs(out["timeScale"][i, 0] - r["t"]) < 1e-9, tag
    _census("kkt_classes_parking", "\n".join(lines))


@pytest.mark.timeout(900)
def test_every_instance_of_the_config5_bench_batch_matches_oracle(OA):
    """BASELINE config 5 at size -- rank 0's batch of `bench.py --config 5`: 4 096 instances with 1-10 obstacles of 1-4 rows each (per-instance H-rep packing, the three
    block-size instantiations mixed in one call) against the oracle on all host cores: every exit flag, every iteration count, every trajectory (1e-6).  No instance is
    exempt (round 2 skipped those beyond 100 iterations; with unit-length rows there is nothing left to skip)."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_pool
    N, B = 80, 4096
    bt = S.make_mixed_batch(B, N, seed=20260925, min_obstacles=1)
    out, xWS = _solve_batch(OA, dict(bt, N=N))
    ref = oracle_pool.mixed_oracle_all(bt, xWS)
    assert len(ref) == B and (out["exitflag"] == 1).all()
    worst_x = worst_f = 0.0
    for (i, ef, it, obj, xp) in ref:
        assert out["exitflag"][i] == ef == 1 and out["iters"][i] == it, (i, out["exitflag"][i], ef, out["iters"][i], it)
        worst_f = max(worst_f, abs(out["obj"][i] - obj) / max(1, abs(obj))); worst_x = max(worst_x, np.abs(out["xp"][i] - xp).max())
    assert worst_x < TOL_X and worst_f < TOL_F, (worst_x, worst_f)
    assert sorted(set(len(v) for v in bt["vOb"])) == list(range(1, 11))


def test_config5_with_binding_obstacles_matches_oracle(OA):
    """config-5 variant whose extra obstacles narrow the road beside the car (scenarios.make_corridor_batch: wedges with sloped rows standing on the walls, tips 0-0.2 m
    beside the warm start's body -- the optimum leans on them where make_mixed_batch's decoys are never near): 256 instances under the reference's IPOPT configuration
    against the oracle with the same options.  These are HARD solves (40-350 iterations, many inertia rungs, large multipliers: IPOPT's termination scaling factors exceed 1
    on them) and two roundings of the same algorithm part ways on a few per cent of them, mostly to the same point after another number of iterations.  Measured on the
    GPU in round 6 (profiles/r06_parity_census_corridor.txt; the library with the multiplier sums stored): 250 / 250 of 256 solved, exit flags equal on
    all 256, iteration counts differ on 12 (4.7 %; 26 before the fix), 10 of those end at the oracle's objective to 1e-4 and 2 in another local solution; where the counts
    agree the trajectories agree to 1.1e-7.  The bounds below are those numbers plus a margin; the test REPORTS the counts."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_pool
    N, B = 80, 256
    bt = S.make_corridor_batch(B, N, seed=11)
    assert max(len(v) for v in bt["vOb"]) >= 6 and min(len(v) for v in bt["vOb"]) >= 3
    out, xWS = _solve_batch(OA, dict(bt, N=N), opts=OA.ipopt_opts())
    ref = oracle_pool.mixed_oracle_all(bt, xWS, switches=oracle_pool.IPOPT)
    nit = nef = 0; worst = 0.0; nsame = 0; same_point = 0; other = []
    for (i, ef, it, obj, xp) in ref:
        nef += int(out["exitflag"][i] != ef)
        if out["iters"][i] != it:
            nit += 1
            if ef == 1 and out["exitflag"][i] == 1:      # both sides solved it after another number of iterations: the same point (objective 1e-4), or another local solution -- listed
                df = abs(out["obj"][i] - obj) / max(1.0, abs(obj))
                if df < 1e-4: same_point += 1
                else: other.append((i, int(out["iters"][i]), it, float(df)))
            continue
        if ef == 1 and out["exitflag"][i] == 1:
            nsame += 1; worst = max(worst, np.abs(out["xp"][i] - xp).max())
    ngpu = int((out["exitflag"] == 1).sum()); nora = sum(1 for r in ref if r[1] == 1)
    msg = ("corridor batch (binding obstacles), reference IPOPT configuration: solved %d (GPU) / %d (oracle) of %d; exit flags differ on %d; iteration counts differ on %d (%d of them "
           "reach the oracle's objective to 1e-4, %d solved on both sides end elsewhere: %s); where they agree (%d solved): worst |dx| %.2e" % (ngpu, nora, B, nef, nit, same_point, len(other), other, nsame, worst))
    print(msg); _census("corridor", msg)
    assert ngpu >= 0.95 * B and nora >= 0.95 * B and nef <= 3 and nit <= 0.08 * B and len(other) <= 5 and worst < 1e-6, (ngpu, nora, nef, nit, other, worst)


@pytest.mark.parametrize("intr,need,most_off", [(0.05, 60, 62), (0.15, 60, 52), (0.3, 56, 40)], ids=["0.05m", "0.15m", "0.30m"])
def test_block_restoration_on_warm_starts_that_penetrate_the_obstacles(OA, intr, need, most_off):
    """obca_opts.restoration through the C ABI (obca_reference_opts sets it): 64 corridor instances whose wedges intrude up to 0.05 / 0.15 / 0.3 m INTO the warm start's swept
    body -- DualMultWS (on the device) returns lambda = mu = 0 on the penetrating poses, the signed-distance NLP started there is rank-deficient, and without IPOPT's restoration
    phase 57 / 45 / 29 of the 64 solve (oracle).  With the block restoration (oracle: 64 / 64 / 63): the GPU solves >= 60 / 60 / 56, agrees with the oracle's
    exit flag on every instance but 2, with its iteration count on >= 75 % (>= 65 % at 0.3 m: 60-300 iteration solves; where the counts agree the trajectories agree to 1e-6, elsewhere nearly all
    reach the same objective), and switching the option off through the ABI reproduces the failures.  REPORTS the counts (profiles/r06_parity_census_restoration_*.txt)."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_pool
    N, B = 80, 64
    bt = S.make_corridor_batch(B, N, seed=11, clearance=(-intr, 0.2))
    o = OA.ipopt_opts(); assert o.restoration == 1
    out, xWS = _solve_batch(OA, dict(bt, N=N), opts=o)
    o0 = OA.ipopt_opts(); o0.restoration = 0
    out0, _ = _solve_batch(OA, dict(bt, N=N), opts=o0)
    ref = oracle_pool.mixed_oracle_all(bt, xWS, switches=oracle_pool.IPOPT)
    nef = nit = 0; worst = 0.0; elsewhere = []
    for (i, ef, it, obj, xp) in ref:
        nef += int(out["exitflag"][i] != ef)
        if ef == 1 and out["exitflag"][i] == 1:
            if out["iters"][i] == it: worst = max(worst, np.abs(out["xp"][i] - xp).max())
            else:
                nit += 1
                if abs(out["obj"][i] - obj) > 1e-4 * max(1.0, abs(obj)): elsewhere.append((i, int(out["iters"][i]), it))
    ngpu, n0, nora = int((out["exitflag"] == 1).sum()), int((out0["exitflag"] == 1).sum()), sum(1 for r in ref if r[1] == 1)
    msg = ("corridor batch with wedges intruding %.2f m into the warm start, reference configuration: solved %d (GPU, block restoration) / %d (oracle, the same) / %d (GPU, restoration = 0) of %d; "
           "exit flags differ from the oracle's on %d; iteration counts differ on %d (%d of them end elsewhere: %s); where they agree worst |dx| %.2e; mean iterations %.0f (restoration) against %.0f (without)"
           % (intr, ngpu, nora, n0, B, nef, nit, len(elsewhere), elsewhere, worst, out["iters"].mean(), out0["iters"].mean()))
    print(msg); _census("restoration_%.2fm" % intr, msg)
    # (iteration counts: measured 4 / 9 / 18 of 64 differ at 0.05 / 0.15 / 0.3 m -- the deeper the intrusion the longer and the more chaotic the solves, 58 / 75 / 112 iterations)
    assert ngpu >= need and nora >= need and n0 <= most_off and nef <= 2 and nit <= (0.35 if intr > 0.2 else 0.25) * B and len(elsewhere) <= 4 and worst < 1e-6, msg
    if intr == 0.15:
        # parked and resumed (the two-launch schedule forced on this small batch): the restoration count and the pending threshold reset travel in the slice record -- same bits;
        # with the mid-solve trigger alone (restoration = 2) as well, where restorations happen INSIDE the solves
        import os
        for mode in (1, 2):
            om = OA.ipopt_opts(); om.restoration = mode
            one, _ = _solve_batch(OA, dict(bt, N=N), opts=om)
            os.environ["OBCA_SLICE_ALWAYS"] = "1"; os.environ["OBCA_SLICE_PASSES"] = "5"
            try:
                two, _ = _solve_batch(OA, dict(bt, N=N), opts=om)
            finally:
                os.environ.pop("OBCA_SLICE_ALWAYS", None); os.environ.pop("OBCA_SLICE_PASSES", None)
            assert np.array_equal(one["info"], two["info"]) and np.array_equal(np.asarray(one["xp"]), np.asarray(two["xp"])), mode
            if mode == 2: assert (one["exitflag"] == 1).sum() >= 58
        bad = OA.ipopt_opts(); bad.restoration = 7
        with pytest.raises(OA.ObcaError):
            _solve_batch(OA, dict(bt, N=N), opts=bad)


@pytest.mark.timeout(1200)
def test_every_instance_of_the_config3_bench_batch_matches_oracle(OA):
    """BASELINE config 3 at size -- rank 0's batch of `bench.py --config 3`: 2 048 parallel-parking instances (4 obstacles / 6 rows, randomised start and goal, Hybrid A*
    warm starts planned here on the host cores) against the oracle: every exit flag and every trajectory (1e-6); iteration counts equal except where round-off decides an
    acceptance test on a knife edge (measured: 1 of 2 048, 51 against 52 iterations to the same point) -- at most 4 are tolerated."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_pool
    N, B = 80, 2048
    bt = S.make_batch(S.PARALLEL, B, N, seed=20260925, goal_jitter=True)
    out, xWS = _solve_batch(OA, bt)
    ref = oracle_pool.parking_oracle_all(bt, xWS)
    assert len(ref) == B and (out["exitflag"] == 1).all()
    off = []; worst_x = worst_f = 0.0
    for (i, ef, it, obj, xp, up, t) in ref:
        assert out["exitflag"][i] == ef == 1, (i, out["exitflag"][i], ef)
        df = abs(out["obj"][i] - obj) / max(1, abs(obj)); dx = np.abs(out["xp"][i] - xp).max()
        if out["iters"][i] != it:      # a knife-edge acceptance test went the other way: reported, bounded in number, and the solve must still end at the oracle's objective (1e-4)
            off.append((i, int(out["iters"][i]), it, float(dx), float(df))); assert df < 1e-4 and dx < 1e-3, off[-1]
            continue
        worst_f = max(worst_f, df); worst_x = max(worst_x, dx)
    print("config 3 bench batch against the oracle: iteration counts differ on", off, "; where they agree: worst |dx| %.2e, worst rel. objective %.2e" % (worst_x, worst_f))
    assert len(off) <= 4 and worst_x < TOL_X and worst_f < TOL_F, (off, worst_x, worst_f)


def test_half_space_rows_of_any_length_describe_the_same_problem(OA, oracle):
    """the rows of the H-representation may have any length (obstHrep.jl leaves sloped edges unnormalised): through the C ABI, rows scaled by 0.02 .. 1e3 give the
    same states, inputs and iteration counts, lambda in the caller's scaling (lambda_r / s_r), the same DualMultWS distances -- and a warm start with the returned
    duals (caller's scaling in, caller's scaling out) is accepted as is"""
    N, B = 40, 8
    bt = S.make_batch(S.BACKWARDS, B, N, seed=5)
    s = np.array([250.0, 0.02, 1e3, 7.0, 0.3])
    b1 = dict(bt); b1["A"] = bt["A"] * s[:, None]; b1["b"] = bt["b"] * s
    o0, xWS = _solve_batch(OA, bt); o1, _ = _solve_batch(OA, b1)
    assert (o0["exitflag"] == 1).all() and (o1["exitflag"] == 1).all() and (o0["iters"] == o1["iters"]).all()
    assert np.abs(o0["xp"] - o1["xp"]).max() < 1e-9 and np.abs(o0["up"] - o1["up"]).max() < 1e-9
    for i in range(B):
        assert np.abs(o0["lp"][i] - o1["lp"][i] * s[:, None]).max() < 1e-8 * max(1.0, np.abs(o0["lp"][i]).max())
    r = oracle.parking_signed_dist(bt["x0"][3], bt["xF"][3], N, bt["Ts"][3], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], b1["A"], b1["b"],
                                   xWS[3, :, 0], xWS[3, :, 1], xWS[3, :, 2], 0, xWS[3], bt["uWS"][3])
    assert r["iters"] == o1["iters"][3] and np.abs(r["xp"] - o1["xp"][3]).max() < TOL_X and np.abs(r["lp"] - o1["lp"][3]).max() < 1e-6 * max(1.0, np.abs(r["lp"]).max())
    l0, n0, d0 = OA.dualmult_ws_batch(N, bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], bt["ego"])
    l1, n1, d1 = OA.dualmult_ws_batch(N, bt["vOb"], b1["A"], b1["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], bt["ego"])
    assert np.abs(np.array(d0) - np.array(d1)).max() < 1e-10 and np.abs(np.array(l0) - np.array(l1) * s[None, None, :]).max() < 1e-9
    # duals handed back in: the solve starts from them in the caller's scaling
    o2, _ = _solve_batch(OA, b1, lWS=np.array(l1), nWS=np.array(n1))
    assert (o2["iters"] == o1["iters"]).all() and np.abs(o2["xp"] - o1["xp"]).max() < 1e-9


@pytest.mark.parametrize("name", ["backwards", "parallel"])
def test_reference_main_jl_call_runs_as_is(OA, oracle, name):
    """BASELINE config 1 (main.jl as it stands, single instance): the reference's own Hybrid A* on its point-cloud obstacles (REFERENCE mode of the planner:
    hybrid_a_star.jl restated), the speed profile / veloSmooth / steering / every-third-sample warm start of main.jl:216-252, the horizon the path length gives
    (N = 64 / 60), then ParkingDist (main.jl:258) and ParkingSignedDist (:269) from that warm start -- both against the oracle"""
    from obca_amd import planner as PL
    from obca_amd import validate as K
    sc = S.BACKWARDS if name == "backwards" else S.PARALLEL
    N, Ts, xWS, uWS, path = PL.reference_warm_start(sc, sc["x0"], sc["xF"])
    A, b, v = S.scenario_hrep(sc); x0, xF = sc["x0"], sc["xF"]; nOb = len(v)
    rx, ry, ryaw = xWS[:, 0].copy(), xWS[:, 1].copy(), xWS[:, 2].copy()
    oo = oracle.default_opts(); oo.max_soc = 4; oo.recalc_y = 1; oo.lsq_init = 1; oo.restoration = 1      # the drop-ins run the reference's IPOPT configuration by default (obca_reference_opts)
    for fn, ofn in ((OA.ParkingDist, oracle.parking_dist), (OA.ParkingSignedDist, oracle.parking_signed_dist)):
        xp, up, ts, ef, t, lp, npp = fn(x0, xF, N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, nOb, v, A, b, rx, ry, ryaw, 0, xWS, uWS)
        r = ofn(x0, xF, N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b, rx, ry, ryaw, 0, xWS, uWS, opts=oo)
        assert ef == r["exitflag"] == 1
        assert xp.shape == (4, N + 1) and up.shape == (2, N)
        assert np.abs(xp - r["xp"]).max() < TOL_X and np.abs(up - r["up"]).max() < TOL_X and abs(float(np.ravel(ts)[0]) - r["t"]) < 1e-9


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("cfg", [2, 3, 5])
def test_the_reference_ipopt_configuration_at_bench_size_matches_the_oracle_with_the_same_options(OA, cfg):
    """The reference runs IPOPT with recalc_y = "yes" (ParkingSignedDist.jl:41) and IPOPT's defaults max_soc = 4 and least-squares initial multipliers: obca_reference_opts /
    obca_amd.ipopt_opts().  With those three switches on in the kernels AND in the oracle: the FULL bench batches of BASELINE configs 2 / 3 / 5 (1 024 / 2 048 / 4 096 instances,
    rank 0's batch of `bench.py --config c`) -- every exit flag equal, every trajectory to 1e-5 (objective 1e-7) where the iteration counts agree, and the iteration counts themselves equal except
    where round-off decides an acceptance test on a knife edge (measured in round 4: 0 / 2 / 1 instances; at most 4 of a batch tolerated).  The test REPORTS the counts."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_pool
    N = 80
    bt = S.make_batch(S.BACKWARDS, 1024, N, seed=20260925) if cfg == 2 else (S.make_batch(S.PARALLEL, 2048, N, seed=20260925, goal_jitter=True) if cfg == 3 else S.make_mixed_batch(4096, N, seed=20260925, min_obstacles=1))
    B = len(bt["x0"])
    out, xWS = _solve_batch(OA, dict(bt, N=N), opts=OA.ipopt_opts())
    ref = oracle_pool.mixed_oracle_all(bt, xWS, switches=oracle_pool.IPOPT) if cfg == 5 else oracle_pool.parking_oracle_all(bt, xWS, switches=oracle_pool.IPOPT)
    assert len(ref) == B
    off = 0; offs = []; flat = []; worst_x = worst_f = 0.0
    for r in ref:
        i, ef, it, obj, xp = r[0], r[1], r[2], r[3], r[4]
        assert out["exitflag"][i] == ef == 1, (i, out["exitflag"][i], ef)
        df = abs(out["obj"][i] - obj) / max(1, abs(obj)); dx = np.abs(out["xp"][i] - xp).max()
        if out["iters"][i] != it:      # a knife-edge acceptance test went the other way: counted, bounded in number -- and the solve must still end at the oracle's point (objective 1e-4, states 1e-3: SURVEY 8c)
            off += 1; offs.append((i, int(out["iters"][i]), it, float(dx), float(df))); assert df < 1e-4 and dx < 1e-3, offs[-1]
            continue
        if dx >= 1e-5:      # a flat direction around the solution: the same iterations, the same objective, the states further apart than usual -- counted with the knife edges
            flat.append((i, float(dx), float(df))); assert dx < 1e-3 and df < 1e-6, flat[-1]
            continue
        worst_f = max(worst_f, df); worst_x = max(worst_x, dx)
    msg = ("config %d, reference IPOPT configuration on both sides: %d instances, iteration counts differ on %d %s, flat-direction instances %s, elsewhere worst |dx| %.2e, worst rel. objective %.2e"
           % (cfg, B, off, offs, flat, worst_x, worst_f))
    print(msg); _census("reference_options_config%d" % cfg, msg)
    # (flat directions around a solution: two fp64 implementations that take the same number of iterations stop up to a few 1e-6 apart in the states at 2e-8 in the objective;
    #  round 5, Hybrid A* warm starts with more direction switches: one instance of 2 048 at 1.7e-4 in the states and 1.4e-8 in the objective)
    assert off + len(flat) <= 4 and worst_x < 1e-5 and worst_f < 1e-7, (off, flat, worst_x, worst_f)


def test_parking_dist_with_the_reference_ipopt_configuration_matches_the_oracle(OA, oracle):
    """ParkingDist (ParkingDist.jl:41 sets recalc_y = "yes" too) with max_soc = 4, recalc_y, lsq_init on both sides: the LSQ / SOC instantiations of the block code in the
    ParkingDist formulation (norm-row slack s1 and its multiplier) -- 48 instances of the backwards scenario, iteration for iteration"""
    N, B = 80, 48
    bt = S.make_batch(S.BACKWARDS, B, N, seed=11)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    out = OA.parking_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0,
                                       xWS, bt["uWS"], opts=OA.ipopt_opts(), dist=True)
    oo = oracle.default_opts(); oo.max_soc = 4; oo.recalc_y = 1; oo.lsq_init = 1; oo.restoration = 1
    nsolved = 0; off = []
    for i in range(B):
        r = oracle.parking_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"],
                                xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i], opts=oo)
        assert out["exitflag"][i] == r["exitflag"], (i, out["exitflag"][i], r["exitflag"])
        if out["iters"][i] != r["iters"]:
            off.append((i, int(out["iters"][i]), r["iters"])); continue
        if r["exitflag"] == 1:
            nsolved += 1
            assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and np.abs(out["up"][i] - r["up"]).max() < TOL_X
    # Instance 17 of this batch is a hard one (81 iterations, multipliers ~1e7 and a dual infeasibility of 1e5 on the way): two builds of the SAME kernel source that differ in the
    # rounding of a handful of sums walk apart there -- last-digit differences at iteration 2 grow to 1e-8 by iteration 23 and to another local solution after it (host emulation,
    # round 4).  Such an instance cannot be pinned iteration for iteration between two implementations; at most two are tolerated and they are reported.
    print("ParkingDist, reference IPOPT configuration on both sides: %d instances, iteration counts differ on %s" % (B, off))
    assert len(off) <= 2 and nsolved >= B - 4 - len(off)


def test_instances_at_the_obstacle_and_row_limits(OA, oracle):
    """OBCA_NOBMAX = 16 obstacles / OBCA_MMAX = 64 rows per instance through the C ABI (round 4 lifted the limits from 10 / 40): a ragged batch whose instances carry 3-16
    obstacles of 3-4 rows (up to 60 rows) against the oracle -- exit flags, iteration counts, trajectories"""
    N, B = 40, 24
    bt = S.make_mixed_batch(B, N, seed=5, max_extra=13, rows=(3, 4), max_rows=64)
    assert max(len(v) for v in bt["vOb"]) == 16 and max(int(np.sum(v)) for v in bt["vOb"]) > 40
    out, xWS = _solve_batch(OA, dict(bt, N=N))
    for i in range(B):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"][i], bt["A"][i], bt["b"][i],
                                       xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0, xWS[i], bt["uWS"][i])
        assert out["exitflag"][i] == r["exitflag"] and out["iters"][i] == r["iters"], (i, out["exitflag"][i], r["exitflag"], out["iters"][i], r["iters"])
        if r["exitflag"] == 1:
            assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X
    assert (out["exitflag"] == 1).sum() >= B - 2


def test_hip_path_lands_on_the_unreformulated_dense_solution_at_N80(OA):
    """tests/golden/dense_N80.npz: the reference's NLP as JuMP hands it to IPOPT (N + 1 time-scale variables, x[:, 1] == x0 kept, bounds as rows with slacks, unnormalised rows with
    gradient-based scaling), solved at N = 80 by a dense Algorithm A that shares nothing with the kernels' structure (oracle/ipm_ref80.py).  The HIP path -- with the reference's
    IPOPT configuration and with the throughput defaults -- must land on that solution (1e-6; the parallel-parking instances at the path's stated 1e-3, all but one); iteration counts are reported, not asserted (tests/test_pin_cpu.py holds the C
    oracle to the same fixture)."""
    g = golden("dense_N80.npz")
    n = len(g["tag"]); N = int(g["N"]); assert n >= 8
    b5 = S.make_mixed_batch(64, 80, seed=20260925, min_obstacles=1) if "cfg5" in set(map(str, g["tag"])) else None
    for tag, sc in (("cfg2", S.BACKWARDS), ("cfg3", S.PARALLEL), ("cfg5", None)):
        idx = [i for i in range(n) if str(g["tag"][i]) == tag]
        if not idx:
            continue
        xWS = g["xWS"][idx]
        if sc is None:      # per-instance obstacle sets with sloped, unnormalised edges
            js = [int(g["idx"][i]) for i in idx]; v = [np.ravel(b5["vOb"][j]).astype(int) for j in js]; A = [np.asarray(b5["A"][j], float) for j in js]; b = [np.asarray(b5["b"][j], float) for j in js]
        else:
            A, b, v = S.scenario_hrep(sc)
        ref_o = OA.ipopt_opts(); ref_o.restoration = 0      # (the dense solve carries IPOPT's three switches and no block restoration)
        for name, o in (("reference IPOPT configuration", ref_o), ("throughput defaults", OA.default_opts())):
            out = OA.parking_signed_dist_batch(g["x0"][idx], g["xF"][idx], N, g["Ts"][idx], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b, xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0,
                                               xWS, g["uWS"][idx], opts=o)
            tx, tt = (1e-3, 1e-4) if tag == "cfg3" else (1e-6, 1e-8)      # config 3 is flat around its solutions: two solves that stop at tol = 1e-5 sit 1e-6 .. 1e-4 apart (tests/test_pin_cpu.py): the path's stated tolerance
            same = [bool(out["exitflag"][k] == 1 and np.abs(out["xp"][k] - g["xp"][i]).max() < tx and np.abs(out["up"][k] - g["up"][i]).max() < tx
                         and abs(out["timeScale"][k, 0] - g["ts"][i][0]) < tt) for k, i in enumerate(idx)]
            print("%s, %s: HIP iterations %s, dense iterations %s, same point %s" % (tag, name, out["iters"].tolist(), [int(g["iters"][i]) for i in idx], same))
            if tag in ("cfg2", "cfg5"):
                assert all(same), (tag, name, same)
            elif name.startswith("reference"):
                assert sum(same) >= len(same) - 1, (tag, name, same)


# ---------------------------------------------------------------- horizons at the edges of the kernels' loops, first iterates, full machine at N = 128
def _oracle_opts(oracle, ref, max_iter=None):
    oo = oracle.default_opts()
    if ref:
        oo.max_soc = 4; oo.recalc_y = 1; oo.lsq_init = 1; oo.restoration = 1      # obca_reference_opts
    if max_iter is not None:
        oo.max_iter = max_iter
    return oo


def _sub(bt, idx):
    """instances idx of a batch (uniform or ragged obstacle sets)"""
    B = len(bt["x0"])
    return {k: ([v[i] for i in idx] if isinstance(v, list) else (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == B and k not in ("vOb", "A", "b", "ego", "XYbounds") else v))
            for k, v in bt.items()}


def _ragged_at_round_boundaries(N, n, seed):
    """n instances of a ragged batch (up to 16 obstacles of up to 8 rows) with n different obstacle counts, the largest first: the (N + 1) nOb block items of the instances
    end at different places of their last round of 64"""
    bt = S.make_mixed_batch(40, N, seed=seed, min_obstacles=1, max_extra=13, rows=(3, 8), max_rows=64)
    nob = [len(v) for v in bt["vOb"]]; pick = []
    for i in sorted(range(40), key=lambda i: (-nob[i], i)):
        if nob[i] not in [nob[j] for j in pick]:
            pick.append(i)
    pick = pick[:n]
    assert len(pick) == n and nob[pick[0]] >= 8, (N, sorted(set(nob)))
    return _sub(dict(bt, N=N), pick)


def _sweep_batches(N):
    if N <= 7:
        return [S.make_hop_batch(N)]
    if N in (63, 64, 65):
        return [S.make_batch(S.BACKWARDS, 3, N, seed=N), _ragged_at_round_boundaries(N, 3, seed=N)]
    return [S.make_batch(S.BACKWARDS, 4, N, seed=N)]


def _oracle_parking(oracle, bt, i, xWS, oo, dist):
    ragged = isinstance(bt["vOb"], list)
    v, A, b = (bt["vOb"][i], bt["A"][i], bt["b"][i]) if ragged else (bt["vOb"], bt["A"], bt["b"])
    return oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], bt["N"], bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], v, A, b, xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0,
                                      xWS[i], bt["uWS"][i], opts=oo, dist=dist)


@pytest.mark.parametrize("N", [2, 3, 4, 5, 7, 63, 64, 65, 126, 127])
def test_parking_horizon_sweep_matches_oracle(OA, oracle, N):
    """Horizons at the edges of the kernels' loops (the forward sweep's single pair at N = 2 / 3 and its pair lanes up to 63 at N = 126 / 127; the stage loops going from one
    round of 64 lanes to two at N = 64; (N + 1) nOb block items on both sides of a multiple of 64 on ragged 1-16-obstacle batches at N = 63 .. 65), both formulations, both
    option sets, against the oracle: exit flag, status, iteration and regularisation counts equal, the point to 1e-6 and the objective to 1e-8 -- converged or not.  A converged
    fraction is asserted per horizon.
    N = 2 leaves the NLP too few degrees of freedom: every attempt ends in status 2 (the inertia ladder runs out on a singular system) after 0 .. 28 iterations.  Which rung of
    the ladder first passes, and so after how many iterations the attempt gives up, is decided by round-off there: the host emulation of this very kernel source and the oracle
    already stop after different iteration counts (0-18 against 1-28), at different points.  So at N = 2 the kernels must end the way the oracle ends -- the same exit flag and
    status 2 on every solve, none converged -- with finite outputs; iteration and regularisation counts and the point are not compared."""
    nconv = ntot = 0
    for dist in (0, 1):
        for ref in (0, 1):
            for bt in _sweep_batches(N):
                out, xWS = _solve_batch(OA, bt, opts=OA.ipopt_opts() if ref else OA.default_opts(), dist=bool(dist))
                for i in range(len(bt["x0"])):
                    r = _oracle_parking(oracle, bt, i, xWS, _oracle_opts(oracle, ref), dist)
                    tag = (N, dist, ref, i, int(out["exitflag"][i]), r["exitflag"], int(out["status"][i]), r["status"], int(out["iters"][i]), r["iters"], int(out["info"][i, 6]), r["nreg"])
                    assert out["exitflag"][i] == r["exitflag"] and out["status"][i] == r["status"], tag
                    ntot += 1; nconv += int(r["status"] == 0 and r["exitflag"] == 1)
                    if N == 2:
                        assert out["status"][i] == 2, tag
                        assert all(np.isfinite(np.asarray(out[q][i])).all() for q in ("xp", "up", "lp", "np", "timeScale")) and np.isfinite(out["info"][i, :7]).all(), tag
                        continue
                    assert out["iters"][i] == r["iters"] and out["info"][i, 6] == r["nreg"], tag
                    assert abs(out["obj"][i] - r["obj"]) <= TOL_F * max(1, abs(r["obj"])), tag
                    assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and np.abs(out["up"][i] - r["up"]).max() < TOL_X, tag
                    assert abs(out["timeScale"][i, 0] - r["t"]) < 1e-9, tag
    _census("horizon_sweep_N%d" % N, "parking, N = %d: %d of %d solves converged (status 0), all with the oracle's exit flag and status%s" % (
        N, nconv, ntot, "" if N == 2 else ", iteration and regularisation counts"))
    if N == 2:
        assert nconv == 0
    else:
        assert nconv >= (0.6 if N == 3 else 0.8) * ntot, (N, nconv, ntot)


def _first_iterate_cases(N):
    if N == 3:
        return [S.make_hop_batch(3, S.HOP_STARTS[:2])]
    cases = [S.make_batch(S.BACKWARDS, 2, N, seed=N)]
    if N in (64, 65):
        bt = S.make_mixed_batch(40, N, seed=N, min_obstacles=1, max_extra=13, rows=(3, 4), max_rows=64)
        i16 = [i for i, v in enumerate(bt["vOb"]) if len(v) == 16][:1]
        assert i16, N
        cases.append(_sub(dict(bt, N=N), i16))
    if N == 20:      # obstacles of 5-8 rows: the widest instantiation of the obstacle block (the instance of tests/golden/kkt_classes.npz)
        bt = S.make_mixed_batch(24, N, seed=11, rows=(5, 8), max_extra=4)
        assert np.ravel(bt["vOb"][3]).tolist() == [2, 2, 1, 5, 6, 7, 7]
        cases.append(_sub(dict(bt, N=N), [3]))
    return cases


_WORST_FIRST = {}


@pytest.mark.parametrize("N", [3, 20, 64, 65, 127, 128])
def test_parking_first_iterates_match_the_oracle_tightly(OA, oracle, N):
    """max_iter = k (k = 0 .. 5): both attempts stop after k iterations and the retry resumes from the last iterate, so the point handed back is the start (k = 0) or the
    iterate after 2k Newton steps -- where a slightly wrong direction shows before the interior point corrects it.  Every returned quantity against the oracle run with the
    same options, relative to max(1, |oracle|): 1e-9 (the host emulation of the same source agrees to a few 1e-12); the regularisation count exactly.  The cases reach every
    instantiation of the obstacle block: 2-row obstacles at every N, sixteen 3-4-row obstacles at N = 64 / 65, rows 2, 2, 1, 5, 6, 7, 7 at N = 20."""
    worst = {}
    for dist in (0, 1):
        for ref in (0, 1):
            for bt in _first_iterate_cases(N):
                for k in range(6):
                    o = OA.ipopt_opts() if ref else OA.default_opts(); o.max_iter = k
                    out, xWS = _solve_batch(OA, bt, opts=o, dist=bool(dist))
                    for i in range(len(bt["x0"])):
                        r = _oracle_parking(oracle, bt, i, xWS, _oracle_opts(oracle, ref, k), dist)
                        tag = (N, dist, ref, k, i)
                        assert out["status"][i] == r["status"] == 1 and out["iters"][i] == r["iters"] == 2 * k and out["info"][i, 6] == r["nreg"], tag + (int(out["info"][i, 6]), r["nreg"])
                        dev = {q: np.abs(np.asarray(out[q][i]) - r[q]).max() / max(1.0, np.abs(r[q]).max()) for q in ("xp", "up", "lp", "np") + (() if dist else ("sl",))}      # (the ParkingDist entry point returns no slack)
                        dev["timeScale"] = np.abs(out["timeScale"][i] - r["timeScale"]).max() / max(1.0, np.abs(r["timeScale"]).max())
                        for j, q in ((2, "obj"), (3, "pinf"), (4, "dinf"), (5, "mu")):
                            dev[q] = abs(out["info"][i, j] - r[q]) / max(1.0, abs(r[q]))
                        q = max(dev, key=dev.get)
                        if dev[q] > worst.get(k, (0.0,))[0]:
                            worst[k] = (float(dev[q]), q, dist, ref, i)
                        assert dev[q] < 1e-9, tag + (q, dev[q])
    _WORST_FIRST[N] = worst
    _census("first_iterates_parking_N%d" % N, "parking, N = %d: worst relative deviation from the oracle per k (value, quantity, dist, ref, instance): %s" % (N, worst))


def test_hip_path_on_the_third_party_short_horizon_fixtures(OA):
    """tests/golden/dense_N8.npz (dense interior point), slsqp_N8.npz (scipy SLSQP) and pin_cfg2_N24.npz (SLSQP from eight config-2 starts): solutions of solvers that share
    nothing with the oracle, so far held against the oracle only (test_oracle_cpu.py, test_pin_cpu.py).  The HIP path, with the fixtures' own duals where they carry them,
    must meet the same bars: objective, time scale, inputs and states -- from above where the fixture is an active-set optimum and the kernels stop at a barrier solution."""
    A, b, v = S.scenario_hrep(S.BACKWARDS)

    def run(x0, xF, N, Ts, xWS, uWS, lWS=None, nWS=None):
        B = len(x0)
        return OA.parking_signed_dist_batch(x0, xF, N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b, xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, uWS, lWS, nWS,
                                            opts=OA.default_opts()) if B else None
    g = golden("dense_N8.npz"); N = int(g["N"])
    o = run(g["x0"][None], g["xF"][None], N, float(g["Ts"]), g["xWS"][None], g["uWS"][None], [g["lWS"]], [g["nWS"]])
    assert str(g["status"]) == "Optimal" and o["exitflag"][0] == 1
    assert abs(o["obj"][0] - float(g["obj"])) <= 1e-4 * max(1, abs(float(g["obj"])))
    assert np.abs(o["xp"][0] - g["xp"]).max() < 1e-3 and np.abs(o["up"][0] - g["up"]).max() < 1e-3 and abs(o["timeScale"][0, 0] - float(g["t"])) < 1e-4
    g = golden("slsqp_N8.npz"); N = int(g["N"])
    o = run(g["x0"][None], g["xF"][None], N, float(g["Ts"]), g["xWS"][None], g["uWS"][None], [g["lWS"]], [g["nWS"]])
    assert o["exitflag"][0] == 1
    assert abs(o["obj"][0] - float(g["obj"])) < 1e-4 * abs(float(g["obj"])) and o["obj"][0] >= float(g["obj"]) - 1e-9      # barrier: from above
    assert np.abs(o["xp"][0] - g["xp"]).max() < 1e-2 and np.abs(o["up"][0] - g["up"]).max() < 5e-3 and abs(o["timeScale"][0, 0] - float(g["t"])) < 1e-5
    recs = list(golden("pin_cfg2_N24.npz")["records"]); assert len(recs) == 8
    N = recs[0]["xp"].shape[1] - 1
    o = run(np.stack([r["x0"] for r in recs]), np.stack([r["xF"] for r in recs]), N, np.array([float(r["Ts"]) for r in recs]), np.stack([r["xWS"] for r in recs]),
            np.stack([r["uWS"] for r in recs]))
    for i, r in enumerate(recs):
        assert o["exitflag"][i] == 1 and o["iters"][i] == r["oracle_iters"], (i, o["iters"][i], r["oracle_iters"])
        assert 0 <= o["obj"][i] - r["obj"] <= 2e-5 * abs(r["obj"]), i
        assert abs(o["timeScale"][i, 0] - r["t"]) < 1e-5 and np.abs(o["up"][i] - r["up"]).max() < 1.1e-2 and np.abs(o["xp"][i] - r["xp"]).max() < 2.5e-2, i


def _chunked(OA, bt, xWS, step=64):
    outs = [OA.parking_signed_dist_batch(bt["x0"][lo:lo + step], bt["xF"][lo:lo + step], bt["N"], bt["Ts"][lo:lo + step], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"],
                                         xWS[lo:lo + step, :, 0], xWS[lo:lo + step, :, 1], xWS[lo:lo + step, :, 2], 0, xWS[lo:lo + step], bt["uWS"][lo:lo + step])
            for lo in range(0, len(bt["x0"]), step)]
    return {k: np.concatenate([np.asarray(o[k]) for o in outs]) for k in ("xp", "up", "timeScale", "lp", "np", "sl", "info", "exitflag")}


def _parking_longest_horizon_checks(OA, oracle, bt, out, xWS):
    from obca_amd import validate as K
    N, B = bt["N"], len(bt["x0"])
    ch = _chunked(OA, bt, xWS)
    for k in ("xp", "up", "timeScale", "lp", "np", "sl", "info", "exitflag"):
        assert np.array_equal(np.asarray(out[k]), ch[k]), k      # results independent of how the batch is cut
    ok = out["exitflag"] == 1
    assert ok.mean() > 0.97, ok.mean()
    for i in np.linspace(0, B - 1, 32).astype(int):
        r = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[i, :, 0], xWS[i, :, 1], xWS[i, :, 2], 0,
                                       xWS[i], bt["uWS"][i])
        assert out["exitflag"][i] == r["exitflag"] and out["status"][i] == r["status"] and out["iters"][i] == r["iters"] and out["info"][i, 6] == r["nreg"], (i, out["iters"][i], r["iters"])
        assert abs(out["obj"][i] - r["obj"]) <= TOL_F * max(1, abs(r["obj"])) and np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and np.abs(out["up"][i] - r["up"]).max() < TOL_X, i
    for i in np.flatnonzero(ok):
        args = (bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], 3, bt["vOb"], bt["A"], bt["b"], out["xp"][i], out["up"][i], out["lp"][i], out["np"][i],
                out["timeScale"][i], 0)
        viol = K.parking_constraints_full(*args, out["sl"][i])
        assert K.feasible(viol, tol=1e-4), (i, viol)
        if viol["penetration"] <= 0:
            assert K.parking_constraints_ref(*args, 1) == 1, i


def test_full_size_parking_at_the_longest_horizon(OA, oracle):
    """B = 1 024 instances at N = OBCA_NMAX = 128, every LDS array at its limit on a full machine: bit-identical to the same instances solved in host-pointer chunks of 64, a
    sample of 32 against the oracle, the reference's acceptance check on every converged instance"""
    N, B = 128, 1024
    bt = S.make_batch(S.BACKWARDS, B, N, seed=128)
    out, xWS = _solve_batch(OA, bt)
    _parking_longest_horizon_checks(OA, oracle, bt, out, xWS)


def test_two_launch_schedule_at_the_longest_horizon(OA, oracle):
    """B = 1 100 at N = 128 exceeds the resident capacity: the two-launch schedule (obca_batch_last_schedule) -- with the same checks as the single launch"""
    N, B = 128, 1100
    bt = S.make_batch(S.BACKWARDS, B, N, seed=1100)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    ctx = OA.Context(0); bb = OA.Batch(ctx, B, N)
    try:
        bb.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
        bb.solve(); out = bb.download()
        assert bb.last_schedule()[0] == 2, bb.last_schedule()
    finally:
        bb.close(); ctx.close()
    _parking_longest_horizon_checks(OA, oracle, bt, out, xWS)
