"""GPU parity of the quadcopter path (QuadcopterSignedDist) through the C ABI against the quadcopter oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Q():
    import oracle_quad
    oracle_quad.lib()
    return oracle_quad


def _clearance(xp, ob):
    """Euclidean distance of every stage position to every box: (N+1, 5)"""
    p = xp[:3].T[:, None, :]; hi = ob[None, :, :3]; lo = -ob[None, :, 3:]
    return np.linalg.norm(p - np.clip(p, lo, hi), axis=2)


def test_quad_shipped_scenario_matches_oracle(Q):
    import obca_amd
    from obca_amd import scenarios as S
    N = 60; Ts = S.quad_sample_time(N)
    xWS = S.quad_warm_start(S.QUAD_X0, S.QUAD_XF, N)
    assert np.array_equal(xWS, Q.warm_start(Q.X0, Q.XF, N, S.QUAD_VIA)) and np.array_equal(S.QUAD_OB, Q.OB_CLAMPED)
    ob = S.QUAD_OB
    xp, up, ts, ef, t, lp, status = obca_amd.QuadcopterSignedDist(S.QUAD_X0, S.QUAD_XF, N, Ts, S.QUAD_R, *ob, xWS, np.zeros((N, 4)), 1.0)
    oo = Q.default_opts(); oo.max_soc = 4; oo.lsq_init = 1; oo.obj_scaling = 1            # the drop-in runs the reference's IPOPT configuration (obca_quadcopter_reference_opts): so does the checker
    r = Q.quadcopter_signed_dist(Q.X0, Q.XF, N, Ts, Q.EGO_R, ob, xWS, 1.0, opts=oo)
    assert ef == 1 and r["exitflag"] == 1 and status == "Optimal"
    assert xp.shape == (12, N + 1) and up.shape == (4, N) and lp.shape == (30, N + 1) and ts.shape == (N + 1,)
    assert np.abs(xp - r["xp"]).max() < 1e-6 and np.abs(up - r["up"]).max() < 1e-6 and np.abs(ts - r["timeScale"]).max() < 1e-9
    assert np.abs(lp - r["lp"]).max() < 1e-4
    assert _clearance(xp, ob).min() >= S.QUAD_R - 2e-3


def test_quad_batch_parity_and_feasibility(Q):
    import obca_amd
    from obca_amd import scenarios as S
    B, N = 48, 30
    bt = S.make_quad_batch(B, N)
    out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    ok = out["exitflag"] == 1
    assert ok.all(), (ok.mean(), out["iters"])
    for rep in range(4):        # repeated solves are bit-identical (no race between the lanes of an instance: LDS exchanges with wave-level ordering only)
        o2 = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
        assert np.array_equal(o2["iters"], out["iters"]) and np.abs(o2["xp"] - out["xp"]).max() == 0.0, rep
    # Two fp64 implementations of the same iteration: iteration counts, regularisation counts, objective, time scale and inputs agree tightly.
    # Positions and multipliers agree only to ~1e-4 / 1e-2: the cost has no term on the path (QuadcopterSignedDist.jl:110-128), so the minimiser is
    # not unique along flat directions and round-off decides where on the optimal face the iteration stops (measured between the oracle and the
    # host emulation of this very kernel source at identical iteration counts: 4e-5 in x, 1.6e-2 in lambda, 5e-11 in the objective).
    flips = []
    for i in range(12):
        r = Q.quadcopter_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], 1.0)
        assert r["exitflag"] == out["exitflag"][i]
        if r["exitflag"] == 1:
            assert abs(out["obj"][i] - r["obj"]) < 1e-8 * abs(r["obj"])
            assert abs(out["timeScale"][i, 0] - r["t"]) < 1e-8 and np.abs(out["up"][i] - r["up"]).max() < 1e-4      # (flat directions reach the inputs at the 1e-5 level)
            assert np.abs(out["xp"][i] - r["xp"]).max() < 1e-3
            if out["iters"][i] != r["iters"] or out["info"][i, 6] != r["nreg"]:
                flips.append((i, int(out["iters"][i]), r["iters"]))
    assert len(flips) <= 1, flips          # an inertia test decided by round-off (Quu pivot ~ 0) may take a different branch: at most one in twelve
    # size-independent properties on every converged instance: bounds, terminal state, dynamics residual, clearance >= R
    from nlp_ref_quad import XLB, XUB
    import oracle_quad
    for i in np.where(ok)[0]:
        xp, up, t = out["xp"][i], out["up"][i], out["timeScale"][i, 0]
        assert np.abs(xp[:, 0] - bt["x0"][i]).max() == 0 and np.abs(xp[:, N] - bt["xF"][i]).max() < 1e-4
        assert (xp >= XLB[:, None] - 1e-6).all() and (xp <= XUB[:, None] + 1e-6).all() and up.min() >= 1.2 - 1e-6 and up.max() <= 7.8 + 1e-6
        assert _clearance(xp, bt["ob"]).min() >= bt["R"] - 2e-3
        assert out["slack"][i].sum() <= 1e-3


def test_quadcopter_dist_variant_matches_oracle(Q):
    """QuadcopterDist (the collision-free sibling): no slack variable, x[10] in [-1.5, 3], exit flag 0/1"""
    import obca_amd
    from obca_amd import scenarios as S
    N = 60; Ts = S.quad_sample_time(N)
    xWS = S.quad_warm_start(S.QUAD_X0, S.QUAD_XF, N)
    xp, up, ts, ef, t, lp, status = obca_amd.QuadcopterDist(S.QUAD_X0, S.QUAD_XF, N, Ts, S.QUAD_R, *S.QUAD_OB, xWS, None, 1.0)
    oo = Q.default_opts(); oo.max_soc = 4; oo.lsq_init = 1; oo.obj_scaling = 1            # the drop-in's default option set
    r = Q.quadcopter_dist(Q.X0, Q.XF, N, Ts, Q.EGO_R, S.QUAD_OB, xWS, 1.0, opts=oo)
    assert ef == 1 and r["exitflag"] == 1 and status == "Optimal"
    assert np.abs(xp - r["xp"]).max() < 1e-5 and np.abs(up - r["up"]).max() < 1e-5 and np.abs(ts - r["timeScale"]).max() < 1e-8
    assert _clearance(xp, S.QUAD_OB).min() >= S.QUAD_R - 1e-4
    bt = S.make_quad_batch(24, 30)
    out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], 30, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"], dist=True)
    assert (out["exitflag"] == 1).all() and np.abs(out["slack"]).max() == 0
    for i in np.where(out["exitflag"] == 1)[0]:
        assert _clearance(out["xp"][i], bt["ob"]).min() >= bt["R"] - 1e-4


def test_reference_main_call_runs_as_is(Q):
    """mainQuadcopter.jl's own call sequence: the 3-D A* path on the 1.0 grid from x = 10 to x = 90 (a_star_3D.jl restated: planner.reference_quad_warm_start), Ts_as
    rounded to two decimals (:131), the warm start stacks the path positions with zeros (:134-136), the boxes are the ones clamped by the plot call
    (SURVEY Q3), and BOTH functions are called with the reference's start lambda = 0.05 (QuadcopterDist :145, QuadcopterSignedDist :152)"""
    import obca_amd
    from obca_amd import scenarios as S, planner as PL, validate as V
    N_as, Ts_as, xWS, uWS_as, path = PL.reference_quad_warm_start()      # a_star_3D.jl restated, on the reference's own point walls (round 4; a stand-in search until then)
    assert N_as == 99 and Ts_as == 0.2                                    # :129-131: N_as = length(rx) - 1 (the path repeats its goal cell once), Ts_as = round(0.25 * 80 / N_as, 2)
    assert np.array_equal(path[0], S.QUAD_X0[:3]) and np.array_equal(path[-1], S.QUAD_XF[:3])
    for fn, orc in ((obca_amd.QuadcopterDist, Q.quadcopter_dist), (obca_amd.QuadcopterSignedDist, Q.quadcopter_signed_dist)):
        xp, up, ts, ef, t, lp, status = fn(S.QUAD_X0, S.QUAD_XF, N_as, Ts_as, S.QUAD_R, *S.QUAD_OB, xWS, 0.5 * np.ones((N_as, 4)), 1, dual_ws=False)
        oo = Q.default_opts(); oo.max_soc = 4; oo.lsq_init = 1; oo.obj_scaling = 1        # the drop-ins' default option set (IPOPT's second-order correction and least-squares y0 on)
        r = orc(Q.X0, Q.XF, N_as, Ts_as, Q.EGO_R, S.QUAD_OB, xWS, 1.0, opts=oo, dual_ws=0)
        assert ef == 1 and r["exitflag"] == 1 and status == "Optimal", (fn.__name__, ef, status)
        assert xp.shape == (12, N_as + 1) and up.shape == (4, N_as) and lp.shape == (30, N_as + 1)
        assert abs(ts[0] - r["t"]) < 1e-8 and np.abs(up - r["up"]).max() < 1e-5 and np.abs(xp - r["xp"]).max() < 1e-3
        ok, w = V.validate_quadcopter(xp, up, ts, S.QUAD_X0, S.QUAD_XF, Ts_as, lp, S.QUAD_OB, S.QUAD_R)
        assert ok, (fn.__name__, w)


def test_quad_random_endpoints_with_astar_warm_starts(Q):
    """start / goal anywhere on either side of the two walls, warm starts from the 3-D grid A* planner"""
    import obca_amd
    from obca_amd import scenarios as S, validate as V
    B, N = 32, 60
    bt = S.make_quad_batch(B, N, random_endpoints=True)
    out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    assert (out["exitflag"] == 1).all()
    for i in range(0, B, 6):
        r = Q.quadcopter_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], 1.0)
        assert r["exitflag"] == out["exitflag"][i]
        if r["exitflag"] == 1:
            same = out["iters"][i] == r["iters"] and out["info"][i, 6] == r["nreg"]
            if same:
                assert abs(out["obj"][i] - r["obj"]) < 1e-6 * abs(r["obj"]) and np.abs(out["xp"][i] - r["xp"]).max() < 1e-3
            else:      # an inertia test decided by round-off took the other branch: another path through the iteration, the same optimum to the termination tolerance
                assert abs(out["obj"][i] - r["obj"]) < 1e-4 * abs(r["obj"]), (i, out["obj"][i], r["obj"])
    for i in np.where(out["exitflag"] == 1)[0]:
        ok, w = V.validate_quadcopter(out["xp"][i], out["up"][i], out["timeScale"][i], bt["x0"][i], bt["xF"][i], bt["Ts"], out["lp"][i], bt["ob"], bt["R"])
        assert ok, (i, w)


def test_quad_matches_golden_fixture_config4():
    """tests/golden/oracle_quad_cfg4.npz (the quadcopter oracle on config 4 at N=60, generated by tests/golden/make_golden.py --quad): the HIP
    path reproduces the stored trajectories without the oracle at run time"""
    import obca_amd
    from conftest import golden
    g = golden("oracle_quad_cfg4.npz"); B, N = int(g["B"]), int(g["N"])
    out = obca_amd.quadcopter_signed_dist_batch(g["x0"], g["xF"], N, float(g["Ts"]), float(g["R"]), g["ob"], g["xWS"], np.ones(B))
    assert (out["exitflag"] == 1).all() and (g["exitflag"] == 1).all()
    assert np.abs(out["obj"] - g["obj"]).max() < 1e-6 * np.abs(g["obj"]).max()
    assert np.abs(out["xp"] - g["xp"]).max() < 1e-3 and np.abs(out["up"] - g["up"]).max() < 1e-3
    assert np.abs(out["timeScale"][:, 0] - g["t"]).max() < 1e-6
    assert np.abs(out["up"] - g["up"]).max() < 1e-5
    assert (out["iters"] == g["iters"]).sum() >= B - 1        # round-off may flip one inertia test


def test_quad_hip_reproduces_the_certified_solutions_of_the_kernel_text():
    """tests/golden/kkt_classes.npz: the final iterates of the host build of the quadcopter kernel text at N = 20 -- QuadcopterSignedDist and QuadcopterDist, throughput options
    and the reference options (obj_scaling: multipliers of sigma f) -- certified with independent (autograd) derivatives by tests/test_kkt_classes_cpu.py.  The HIP path must
    return the same arrays without the oracle at run time: one batch per formulation and option set, exit flag, iteration count, and the point within the tolerances of
    test_hip_reproduces_the_independently_certified_solutions"""
    import obca_amd
    import kkt_classes_common as K
    from conftest import golden
    recs = [r for r in golden("kkt_classes.npz")["records"] if K.is_quad(r)]
    assert len(recs) == 8
    lines = []
    for dist in (0, 1):
        for ref in (0, 1):
            rs = [r for r in recs if (r["dist"], r["ref"]) == (dist, ref)]
            assert len(rs) == 2 and len({(float(r["Ts"]), float(r["R"])) for r in rs}) == 1 and np.array_equal(rs[0]["ob"], rs[1]["ob"])
            o = obca_amd.quadcopter_ipopt_opts() if ref else obca_amd.quadcopter_default_opts()
            out = obca_amd.quadcopter_signed_dist_batch(np.stack([r["x0"] for r in rs]), np.stack([r["xF"] for r in rs]), K.N, float(rs[0]["Ts"]), float(rs[0]["R"]), rs[0]["ob"],
                                                        np.stack([r["xWS"] for r in rs]), np.ones(len(rs)), opts=o, dist=bool(dist))
            for i, r in enumerate(rs):
                tag = K.name(r); dx = np.abs(out["xp"][i] - r["xp"]).max(); du = np.abs(out["up"][i] - r["up"]).max(); df = abs(out["obj"][i] - r["solver_obj"]) / abs(r["solver_obj"])
                lines.append("%s: exit flag %d, %d iterations (fixture %d), largest deviation of the states %.1e, inputs %.1e, time scale %.1e, objective %.1e relative"
                             % (tag, out["exitflag"][i], out["iters"][i], r["iters"], dx, du, abs(out["timeScale"][i, 0] - r["t"]), df))
                print(lines[-1])
                assert out["exitflag"][i] == r["exitflag"] == 1 and out["iters"][i] == r["iters"], tag
                assert df <= 1e-8 and du < 1e-5 and abs(out["timeScale"][i, 0] - r["t"]) < 1e-8 and dx < 1e-3, tag
    _census("kkt_classes_quad", "\n".join(lines))


@pytest.mark.timeout(900)
def test_all_1024_quadcopter_bench_instances_match_oracle(Q):
    """every instance of the config-4 bench batch (N = 60, random end points, A* warm starts) against the oracle run on all host cores: exit flags equal everywhere;
    objective, time scale and inputs agree tightly on every instance whose iteration took the same branches (same iteration and regularisation counts: two fp64
    implementations of one algorithm); the few instances where an inertia test decided by round-off takes the other branch must still reach the same optimum"""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import obca_amd, oracle_pool
    from obca_amd import scenarios as S
    B, N = 1024, 60
    bt = S.make_quad_batch(B, N, random_endpoints=True)
    out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    ref = oracle_pool.quad_oracle_all(bt)
    assert len(ref) == B
    flips = 0; worst_f = worst_u = worst_t = 0.0
    for (i, ef, it, nreg, obj, up, t) in ref:
        assert out["exitflag"][i] == ef, (i, out["exitflag"][i], ef)
        if ef != 1:
            continue
        same = out["iters"][i] == it and out["info"][i, 6] == nreg
        flips += int(not same)
        df = abs(out["obj"][i] - obj) / abs(obj)
        if same:
            worst_f = max(worst_f, df); worst_u = max(worst_u, np.abs(out["up"][i] - up).max()); worst_t = max(worst_t, abs(out["timeScale"][i, 0] - t))
        else:
            assert df < 1e-4, (i, df)            # another path through the iteration, the same optimum to the termination tolerance (observed <= 1.2e-5)
    assert (out["exitflag"] == 1).mean() > 0.99
    assert flips <= 0.03 * B, flips
    assert worst_f < 1e-8 and worst_t < 1e-7 and worst_u < 1e-3, (worst_f, worst_t, worst_u)


@pytest.mark.timeout(900)
def test_quadcopter_ipopt_configuration_matches_oracle_options(Q):
    """obca_quadcopter_reference_opts (IPOPT's defaults the reference's call runs with: max_soc = 4, least-squares initial multipliers, gradient-based objective scaling; recalc_y = "no") in the
    quadcopter kernel against the oracle run with the same options, on 256 instances of the config-4 distribution: the same bar as the default option set (exit
    flags equal; same counts -> tight agreement; a branch flipped by round-off -> the same optimum); the options change the path of most instances, each of them
    alone too, and the kernel still refuses the switch it does not carry"""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import obca_amd, oracle_pool
    from obca_amd import scenarios as S
    B, N = 256, 60
    bt = S.make_quad_batch(B, N, random_endpoints=True)
    o = obca_amd.quadcopter_ipopt_opts()
    assert o.max_soc == 4 and o.recalc_y == 0 and o.lsq_init == 1 and o.obj_scaling == 1 and o.max_iter == 3000
    base = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"], opts=o)
    ref = oracle_pool.quad_oracle_all(bt, max_soc=4, lsq_init=1, obj_scaling=1)
    flips = 0
    for (i, ef, it, nreg, obj, up, t) in ref:
        assert out["exitflag"][i] == ef, (i, out["exitflag"][i], ef)
        if ef != 1:
            continue
        same = out["iters"][i] == it and out["info"][i, 6] == nreg
        flips += int(not same)
        df = abs(out["obj"][i] - obj) / abs(obj)
        if same:
            assert df < 1e-8 and np.abs(out["up"][i] - up).max() < 1e-4 and abs(out["timeScale"][i, 0] - t) < 1e-8, (i, df)
        else:
            assert df < 1e-4, (i, df)
    assert flips <= 0.03 * B, flips
    assert (out["exitflag"] == 1).mean() > 0.99
    assert (out["iters"] != base["iters"]).mean() > 0.5      # the options are exercised
    print("quadcopter IPOPT configuration vs oracle options: %d / %d instances on another branch; iterations %d -> %d" % (flips, B, base["iters"].sum(), out["iters"].sum()))
    n = 64      # each switch alone, against the oracle with that switch alone
    for (msoc, lsq, osc) in ((4, 0, 0), (0, 1, 0), (0, 0, 1)):
        o1 = obca_amd.quadcopter_default_opts(); o1.max_soc = msoc; o1.lsq_init = lsq; o1.obj_scaling = osc
        sub = {k: (v[:n] if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == B else v) for k, v in bt.items()}
        o1out = obca_amd.quadcopter_signed_dist_batch(sub["x0"], sub["xF"], N, bt["Ts"], bt["R"], bt["ob"], sub["xWS"], bt["timeWS"], opts=o1)
        r1 = oracle_pool.quad_oracle_all(sub, max_soc=msoc, lsq_init=lsq, obj_scaling=osc)
        same = sum(int(o1out["exitflag"][i] == ef and o1out["iters"][i] == it and o1out["info"][i, 6] == nreg) for (i, ef, it, nreg, obj, up, t) in r1)
        assert all(o1out["exitflag"][i] == ef for (i, ef, *_r) in r1) and same >= n - 3, (msoc, lsq, osc, same)
        assert (o1out["iters"] != base["iters"][:n]).mean() > 0.3, (msoc, lsq, osc)
    bad = obca_amd.quadcopter_ipopt_opts(); bad.recalc_y = 1
    with pytest.raises(obca_amd.ObcaError):
        obca_amd.quadcopter_signed_dist_batch(bt["x0"][:2], bt["xF"][:2], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][:2], bt["timeWS"], opts=bad)


@pytest.mark.parametrize("s_max", [1e-2, 1e-4], ids=["s_max_0.01", "s_max_0.0001"])
def test_quad_termination_scaling_factors_active_on_the_gpu_follow_the_oracle(Q, s_max):
    """GPU twin of tests/test_emu_quad_cpu.py::test_quad_termination_scaling_factors_follow_the_oracle: IPOPT's s_d, s_c made active by a small s_max (with the default 100 they
    are 1 on these instances), through the C ABI, default and reference option sets: kernel and oracle stop at the same iteration at the same objective (the quadcopter kernel
    always stored its multiplier sums; this is the check that would have found the parking kernels' lost stores).  One instance of twelve may take
    another branch at an inertia test decided by round-off, as in test_quad_batch_parity_and_feasibility; it must still reach the oracle's objective."""
    import obca_amd
    from obca_amd import scenarios as S
    B, N = 12, 20
    bt = S.make_quad_batch(B, N)
    for ref_opts in (0, 1):
        o = obca_amd.quadcopter_ipopt_opts() if ref_opts else obca_amd.quadcopter_default_opts(); o.s_max = s_max
        oo = Q.default_opts(); oo.s_max = s_max; o1 = Q.default_opts()
        if ref_opts:
            for x in (oo, o1):
                x.max_soc = 4; x.lsq_init = 1; x.obj_scaling = 1
        out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"], opts=o)
        flips = []; active = 0
        for i in range(B):
            r = Q.quadcopter_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], 1.0, opts=oo)
            r1 = Q.quadcopter_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], 1.0, opts=o1)
            assert out["exitflag"][i] == r["exitflag"] == 1, (ref_opts, i, out["exitflag"][i], r["exitflag"])
            active += r["iters"] != r1["iters"]
            if out["iters"][i] != r["iters"] or out["info"][i, 6] != r["nreg"]:
                flips.append((i, int(out["iters"][i]), r["iters"])); assert abs(out["obj"][i] - r["obj"]) < 1e-4 * abs(r["obj"]), flips[-1]
                continue
            # (a solve that the active factors end EARLY stops where two roundings of the iteration are still 1e-8 apart in the objective -- measured 1.3e-8 -- against 1e-11 at
            #  the default s_max; the stated tolerance of the path is 1e-4)
            assert abs(out["obj"][i] - r["obj"]) < 1e-6 * abs(r["obj"]) and abs(out["timeScale"][i, 0] - r["t"]) < 1e-6 and np.abs(out["up"][i] - r["up"]).max() < 1e-3, (ref_opts, i)
        assert len(flips) <= 1, (ref_opts, flips)
        assert active >= B - 2, (ref_opts, active)      # the factors were active (they also enter the barrier update: the count may go either way)


def test_unreformulated_quadcopter_model_accepts_the_hip_solutions_at_N60(Q):
    """the reference's quadcopter NLP as JuMP states it (oracle/ipm_ref60_quad.py; tests/test_pin_cpu.py: unreformulated_quad_certificate) at the HIP path's solutions of two
    config-4 instances, with the reference's IPOPT configuration and with the throughput defaults: same objective, rows satisfied, no bound violated, first-order stationarity
    with correctly signed multipliers -- the reformulations the kernel makes (one t, x_0 eliminated, bounds as bounds) are pinned at the benchmark size"""
    pytest.importorskip("torch")
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import obca_amd
    from obca_amd import scenarios as S
    from test_pin_cpu import unreformulated_quad_certificate
    N = 60; bt = S.make_quad_batch(8, N, seed=20260925, random_endpoints=True)
    for name, o in (("reference IPOPT configuration", obca_amd.quadcopter_ipopt_opts()), ("throughput defaults", None)):
        out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"], opts=o)
        tol_s = 1e-3 if o is None else 0.2      # (with IPOPT's objective scaling 1 / 21 the scaled problem is solved to tol, barrier parameter and stationarity are 21 x looser in
                                                 #  unscaled terms -- IPOPT's own unscaled acceptance is dual_inf_tol = 1 --: measured 0.08)
        for i in range(2):
            assert out["exitflag"][i] == 1
            c = unreformulated_quad_certificate(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], out["xp"][i], out["up"][i], out["timeScale"][i, 0], out["lp"][i], out["slack"][i])
            print("%s, instance %d: f %.10f (HIP %.10f), |c| %.1e, bound violation %.1e, stationarity %.1e, wrong-sign multiplier %.1e" % (name, i, c["f"], out["obj"][i], c["c"], c["viol"], c["stationarity"], c["wrong_sign"]))
            assert abs(c["f"] - out["obj"][i]) < 1e-10 * abs(out["obj"][i]) and c["c"] < 1e-4 and c["viol"] == 0 and c["stationarity"] < tol_s and c["wrong_sign"] < 1e-6


# ---------------------------------------------------------------- horizons at the edges of the kernel's loops, first iterates, full machine at N = 128
def _quad_opts(Q, ref, max_iter=None):
    import obca_amd
    o = obca_amd.quadcopter_ipopt_opts() if ref else obca_amd.quadcopter_default_opts(); oo = Q.default_opts()
    if ref:
        oo.max_soc = 4; oo.lsq_init = 1; oo.obj_scaling = 1
    if max_iter is not None:
        o.max_iter = oo.max_iter = max_iter
    return o, oo


def _census(name, text):
    from test_gpu_parity import _census as c
    c(name, text)


# Horizons at which the quadcopter NLP is so ill-conditioned that two fp64 implementations of the same iteration part ways: measured between the host emulation of this very
# kernel source and the oracle on the sweep's own instances, inertia tests decided by round-off (Quu pivots ~ 0) take the other branch on 16 / 24 solves at N = 4, 20 / 24 at
# N = 5 (one of them with the other exit flag: 1 against 2, the slack test of QuadcopterSignedDist.jl:285-288 on a knife edge), 5 / 24 at N = 16 and 3 / 16 at N = 127.  There
# the bar of test_quad_batch_parity_and_feasibility (at most one flip) cannot hold between ANY two correct implementations; the sweep checks what does (see the test).  On the
# GPU (the same instances): 38 / 48, 23 / 24, 5 / 24 and 3 / 16 flips; at N = 5 the 100-1 000-iteration solves of two of the six instances end in a collision-free local solution
# (exit flag 1) where the oracle ends in one that needs slack (exit flag 2), or the other way round.
_QUAD_ILL_CONDITIONED = (4, 5, 16, 127)


def _quad_outputs_finite(out, i):
    return all(np.isfinite(np.asarray(out[q][i])).all() for q in ("xp", "up", "lp", "slack", "timeScale")) and np.isfinite(out["info"][i, :7]).all()


@pytest.mark.parametrize("N", [2, 3, 4, 5, 16, 63, 64, 65, 127, 128])
def test_quad_horizon_sweep_matches_oracle(Q, N):
    """Horizons at the edges of the quadcopter kernel's loops: the backward sweep's gathers QMD = 2 stages ahead whose prologue and epilogue overlap at N = 2 .. 4, the stage
    loops going from one round of QNT = 64 lanes to two at N = 64, the LDS trajectory full at N = QNMAX = 128.  Both option sets, the dual warm start and the reference's own
    start (dual_ws = 0: the block restoration), QuadcopterDist at N = 4 and 128, against the oracle; finite outputs everywhere, the reference's acceptance check on every
    converged instance.
    N = 2 / 3: the oracle stops before the first iteration -- so must the kernel, with the same exit flag, status and counts.
    N = 3, 63 .. 65, 128: exit flag and status equal everywhere; the same branches (iteration and regularisation counts) -> objective 1e-8, time scale 1e-8, inputs 1e-4,
    states 1e-3; at most one branch flipped by round-off per horizon, and it reaches the oracle's objective to 1e-4.
    N = 4, 5, 16, 127 (_QUAD_ILL_CONDITIONED: branch flips are the rule there, also between the emulation and the oracle): status equal everywhere; flips and differing exit
    flags counted and reported, and the kernel ends collision-free (exit flag 1) at least as often as the oracle, less one; where both sides end collision-free after different
    paths the objectives agree to 1e-4 on all but one solve per horizon (another local solution: reported); on the same branch the objective agrees to 1e-6."""
    import obca_amd
    from obca_amd import scenarios as S, validate as V
    B = 6 if N <= 16 else 4
    ill = N in _QUAD_ILL_CONDITIONED
    bt = S.make_quad_batch(B, N, seed=N)
    flips = []; elsewhere = []; ef_off = []; nconv = ntot = n1_gpu = n1_ora = 0
    for dist in ((0, 1) if N in (4, 128) else (0,)):
        for ref in (0, 1):
            for dws in (1, 0):
                o, oo = _quad_opts(Q, ref)
                out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"], dual_ws=bool(dws), opts=o, dist=bool(dist))
                for i in range(B):
                    r = Q.quadcopter_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], 1.0, opts=oo, dual_ws=dws, dist=dist)
                    tag = (N, dist, ref, dws, i, int(out["exitflag"][i]), r["exitflag"], int(out["status"][i]), r["status"], int(out["iters"][i]), r["iters"], int(out["info"][i, 6]), r["nreg"])
                    assert _quad_outputs_finite(out, i), tag
                    assert out["status"][i] == r["status"], tag
                    if out["exitflag"][i] != r["exitflag"]:
                        assert ill, tag
                        ef_off.append(tag)
                    same = out["iters"][i] == r["iters"] and out["info"][i, 6] == r["nreg"]
                    ntot += 1; nconv += int(r["status"] == 0); n1_gpu += int(out["exitflag"][i] == 1); n1_ora += int(r["exitflag"] == 1)
                    df = abs(out["obj"][i] - r["obj"]) / max(1.0, abs(r["obj"]))
                    if same:
                        if ill:
                            assert df < 1e-6, tag
                        else:
                            assert df < 1e-8 and abs(out["timeScale"][i, 0] - r["t"]) < 1e-8 and np.abs(out["up"][i] - r["up"]).max() < 1e-4 and np.abs(out["xp"][i] - r["xp"]).max() < 1e-3, tag
                    else:
                        assert r["status"] == 0, tag          # a solve the oracle stops unfinished stops at the same iteration on the GPU
                        flips.append(tag[:5])
                        if df >= 1e-4 and not (ill and out["exitflag"][i] != r["exitflag"]):      # (differing exit flags: another local solution by definition, counted above)
                            assert ill, tag + (df,)
                            elsewhere.append(tag[:5] + (float(df),))
                    if out["exitflag"][i] == 1:
                        ok, w = V.validate_quadcopter(out["xp"][i], out["up"][i], out["timeScale"][i], bt["x0"][i], bt["xF"][i], bt["Ts"], out["lp"][i], bt["ob"], bt["R"])
                        assert ok, tag + (w,)
    msg = ("quadcopter, N = %d: %d of %d solves converged (status 0), %d collision-free (exit flag 1; the oracle: %d); branches flipped by round-off on %d: %s; exit flags differ on "
           "%s; flipped collision-free solves ending elsewhere (objective > 1e-4 apart): %s" % (N, nconv, ntot, n1_gpu, n1_ora, len(flips), flips, ef_off, elsewhere))
    print(msg); _census("quad_horizon_sweep_N%d" % N, msg)
    if ill:
        assert n1_gpu >= n1_ora - 1 and len(elsewhere) <= 1, msg
    else:
        assert len(flips) <= 1, msg
    if N <= 3:
        assert nconv == 0
    else:
        assert nconv >= 0.9 * ntot, (nconv, ntot)


@pytest.mark.parametrize("N", [4, 64, 65, 128])
def test_quad_first_iterates_match_the_oracle_tightly(Q, N):
    """max_iter = k (k = 0 .. 3; the quadcopter path makes one attempt): the point after k Newton steps, both option sets, both starts, against the oracle with the same options
    -- every returned quantity (states, inputs, time scale, multipliers, slacks, objective, infeasibilities, barrier parameter) relative to max(1, |oracle|) to 1e-8 (the reduced
    Hessian has near-zero input pivots), the regularisation count exactly.  At N = 4 (the gather pipeline's prologue and epilogue overlap) only k <= 1: from the second step on,
    round-off on that ill-conditioned system is amplified past the bar between any two implementations -- the host emulation of this source and the oracle are 1e-8 .. 7e-8
    apart in the multipliers at k = 2 .. 3 there."""
    import obca_amd
    from obca_amd import scenarios as S
    B = 2; bt = S.make_quad_batch(B, N, seed=N); worst = {}
    for ref in (0, 1):
        for dws in (1, 0):
            for k in range(2 if N == 4 else 4):
                o, oo = _quad_opts(Q, ref, k)
                out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"], dual_ws=bool(dws), opts=o)
                for i in range(B):
                    r = Q.quadcopter_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], 1.0, opts=oo, dual_ws=dws)
                    tag = (N, ref, dws, k, i)
                    assert out["status"][i] == r["status"] == 1 and out["iters"][i] == r["iters"] == k and out["info"][i, 6] == r["nreg"], tag + (int(out["info"][i, 6]), r["nreg"])
                    dev = {q: np.abs(out[q][i] - r[q]).max() / max(1.0, np.abs(r[q]).max()) for q in ("xp", "up", "timeScale", "lp", "slack")}
                    for j, q in ((2, "obj"), (3, "pinf"), (4, "dinf"), (5, "mu")):
                        dev[q] = abs(out["info"][i, j] - r[q]) / max(1.0, abs(r[q]))
                    q = max(dev, key=dev.get)
                    if dev[q] > worst.get(k, (0.0,))[0]:
                        worst[k] = (float(dev[q]), q, ref, dws, i)
                    assert dev[q] < 1e-8, tag + (q, dev[q])
    _census("first_iterates_quad_N%d" % N, "quadcopter, N = %d: worst relative deviation from the oracle per k (value, quantity, ref, dual_ws, instance): %s" % (N, worst))


def test_quad_hip_path_on_the_third_party_short_horizon_fixture(Q):
    """tests/golden/slsqp_quad_N8.npz (a short hop solved by scipy SLSQP, held against the oracle in test_oracle_quad_cpu.py) through the C ABI, at the same bars: objective from
    above to 1e-4, time scale 1e-5, inputs 5e-3 (the cost has no term on the path: positions are not unique)"""
    import obca_amd
    from conftest import golden
    g = golden("slsqp_quad_N8.npz"); N = int(g["N"])
    out = obca_amd.quadcopter_signed_dist_batch(g["x0"][None], g["xF"][None], N, float(g["Ts"]), Q.EGO_R, Q.OB_CLAMPED, g["xWS"][None], 1.0)
    assert out["exitflag"][0] == 1
    assert abs(out["obj"][0] - float(g["obj"])) < 1e-4 * abs(float(g["obj"])) and out["obj"][0] >= float(g["obj"]) - 1e-9
    assert abs(out["timeScale"][0, 0] - float(g["t"])) < 1e-5 and np.abs(out["up"][0] - g["up"]).max() < 5e-3


def test_full_size_quadcopter_at_the_longest_horizon(Q):
    """B = 1 024 instances at N = OBCA_QUAD_NMAX = 128 (the LDS trajectory full) on a full machine: bit-identical to the same instances solved in host-pointer chunks of 64, a sample
    of 32 against the oracle (the bars of test_quad_horizon_sweep_matches_oracle), the reference's acceptance check on every converged instance"""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import obca_amd, oracle_pool
    from obca_amd import scenarios as S, validate as V
    N, B = 128, 1024
    bt = S.make_quad_batch(B, N, seed=128)
    out = obca_amd.quadcopter_signed_dist_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    outs = [obca_amd.quadcopter_signed_dist_batch(bt["x0"][lo:lo + 64], bt["xF"][lo:lo + 64], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][lo:lo + 64], bt["timeWS"]) for lo in range(0, B, 64)]
    for k in ("xp", "up", "timeScale", "lp", "slack", "info", "exitflag"):
        assert np.array_equal(out[k], np.concatenate([o[k] for o in outs])), k
    ok = out["exitflag"] == 1
    assert ok.mean() > 0.97, ok.mean()
    idx = np.linspace(0, B - 1, 32).astype(int)
    sub = {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == B else v) for k, v in bt.items()}
    flips = []
    for (j, ef, it, nreg, obj, up, t) in oracle_pool.quad_oracle_all(sub):
        i = idx[j]
        assert out["exitflag"][i] == ef, (i, out["exitflag"][i], ef)
        df = abs(out["obj"][i] - obj) / max(1.0, abs(obj))
        if out["iters"][i] == it and out["info"][i, 6] == nreg:
            assert df < 1e-8 and abs(out["timeScale"][i, 0] - t) < 1e-8 and np.abs(out["up"][i] - up).max() < 1e-4, (i, df)
        else:
            flips.append(int(i)); assert df < 1e-4, (i, df)
    assert len(flips) <= 1, flips
    for i in np.flatnonzero(ok):
        good, w = V.validate_quadcopter(out["xp"][i], out["up"][i], out["timeScale"][i], bt["x0"][i], bt["xF"][i], bt["Ts"], out["lp"][i], bt["ob"], bt["R"])
        assert good, (i, w)
