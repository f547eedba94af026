"""Host-side Hybrid A* warm-start planner (obca_amd/planner.py, csrc/obca_planner.cpp): the step before the hot path."""
import numpy as np
import pytest
from obca_amd import scenarios as S, planner as PL


@pytest.mark.parametrize("sc", [S.BACKWARDS, S.PARALLEL], ids=["backwards", "parallel"])
def test_plan_is_collision_free_and_reaches_the_goal(sc):
    A, b, v = S.scenario_hrep(sc)
    o, _ = PL.SCENARIO_OPTS[sc["name"]]
    path, dr, nexp = PL.hybrid_astar(sc["x0"][:3], sc["xF"][:3], v, A, b, **o)
    assert np.allclose(path[0], sc["x0"][:3]) and nexp > 0
    assert np.hypot(*(path[-1, :2] - sc["xF"][:2])) <= 0.3 + 1e-9
    assert abs((path[-1, 2] - sc["xF"][2] + np.pi) % (2 * np.pi) - np.pi) <= np.deg2rad(8) + 1e-9
    assert not any(PL.collides(p, v, A, b) for p in path)                      # exact rectangle / convex-set test, no inflation
    assert set(np.unique(dr)) <= {-1, 1}
    # kinematics: consecutive poses lie on arcs no tighter than the minimum turning radius (0.2 m sub-steps)
    ds = np.hypot(np.diff(path[:, 0]), np.diff(path[:, 1])); dpsi = np.abs(np.diff(np.unwrap(path[:, 2])))
    assert ds.max() < 0.21 and (dpsi <= 0.2 * np.tan(0.6) / S.L_WHEELBASE + 1e-9).all()      # 0.2 m of arc per sub-step
    # the parallel bay is too short for a single reverse S-curve: the plan changes direction at least twice
    if sc["name"] == "parallel":
        assert (np.diff(dr) != 0).sum() >= 2


def test_collision_test_known_answers():
    A, b, v = S.scenario_hrep(S.PARALLEL)
    assert not PL.collides(S.PARALLEL["xF"], v, A, b) and not PL.collides(S.PARALLEL["x0"], v, A, b)
    assert PL.collides([-1.35, 2.9, 0.0], v, A, b)              # rear-right corner below the bay floor y = 2.5 + width
    assert PL.collides([0.0, 4.0, 0.0], v, A, b)                # nose through the right wall x = 3
    assert PL.collides([0.0, 20.0, 0.0], v, A, b)               # outside XYbounds
    with pytest.raises(ValueError):
        PL.hybrid_astar([0.0, 4.0, 0.0], S.PARALLEL["xF"][:3], v, A, b)


@pytest.mark.parametrize("k, bad", [(0, np.nan), (1, np.nan), (2, np.nan), (2, np.inf), (2, -np.inf), (0, np.inf), (1, -np.inf)])
def test_a_pose_that_is_not_a_number_collides(k, bad):
    """The host planner refuses no pose at its door (the device planner does): in a field with an obstacle a NaN or an infinity in the pose counts as a collision, for the
    exported test and as a start or a goal of the search (return code -2), never as a free pose to search from."""
    A, b, v = S.scenario_hrep(S.PARALLEL)
    pose = np.array(S.PARALLEL["x0"][:3], float)
    assert PL.collides(pose, v, A, b) is False      # (the pose the case is made from is free)
    pose[k] = bad
    assert PL.collides(pose, v, A, b) is True
    for start, goal in ((pose, S.PARALLEL["xF"][:3]), (S.PARALLEL["x0"][:3], pose)):
        with pytest.raises(ValueError, match="collides"):
            PL.hybrid_astar(start, goal, v, A, b)


def _overlap_area2(pose, rows_A, rows_b, ego, margin):
    """twice the area of (car rectangle inflated by margin) cut by the half-planes rows_A p <= rows_b: the definition of the planner's collision test, in numpy"""
    x, y, yaw = pose; c, s = np.cos(yaw), np.sin(yaw); f, l, r, rt = (e + margin for e in ego)
    poly = [(x + f * c - l * s, y + f * s + l * c), (x - r * c - l * s, y - r * s + l * c), (x - r * c + rt * s, y - r * s - rt * c), (x + f * c + rt * s, y + f * s - rt * c)]
    for (ax, ay), bb in zip(rows_A, rows_b):
        out = []
        for i, p in enumerate(poly):
            q = poly[(i + 1) % len(poly)]; dp = ax * p[0] + ay * p[1] - bb; dq = ax * q[0] + ay * q[1] - bb
            if dp <= 0:
                out.append(p)
            if dp * dq < 0:
                t = dp / (dp - dq); out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out
        if not poly:
            return 0.0
    return abs(sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(poly, poly[1:] + poly[:1]))) if len(poly) >= 3 else 0.0


@pytest.mark.parametrize("sc", [S.BACKWARDS, S.PARALLEL], ids=lambda s: s["name"])
def test_collision_test_equals_its_definition_on_random_poses(sc):
    """the separating-axis shortcuts of the planner's collision test (a row every corner violates, a car side every obstacle vertex lies beyond, a corner deep inside)
    must agree with the overlap area that defines it -- bounded and unbounded obstacles, poses concentrated where the car nearly touches"""
    A, b, v = S.scenario_hrep(sc); A = np.asarray(A, float).reshape(-1, 2); b = np.ravel(b); off = np.concatenate([[0], np.cumsum(v)])
    rng = np.random.default_rng(11); xy = S.XYBOUNDS; n_hit = 0
    for k in range(1500):
        pose = np.array([rng.uniform(xy[0], xy[1]), rng.uniform(xy[2], xy[3]), rng.uniform(-np.pi, np.pi)]); margin = [0.0, 0.02, 0.1][k % 3]
        area = max(_overlap_area2(pose, A[off[j]:off[j + 1]], b[off[j]:off[j + 1]], S.EGO, margin) for j in range(len(v)))
        if abs(area - 1e-9) < 1e-10:
            continue
        assert PL.collides(pose, v, A, b, margin=margin) == (area > 1e-9), (pose, margin, area)
        n_hit += area > 1e-9
    assert n_hit > 200 and n_hit < 1300


def test_path_to_warm_start_shapes_and_consistency():
    sc = S.PARALLEL; N = 80
    Ts, xWS, uWS = PL.warm_start(sc, sc["x0"], sc["xF"], N)
    assert xWS.shape == (N + 1, 4) and uWS.shape == (N, 2) and Ts > 0
    assert np.allclose(xWS[0, :3], sc["x0"][:3]) and np.allclose(xWS[-1, :3], sc["xF"][:3], atol=1e-12)
    assert xWS[0, 3] == 0 and xWS[-1, 3] == 0 and np.abs(xWS[:, 3]).max() <= 0.25 + 1e-12
    assert np.abs(uWS[:, 0]).max() <= 0.6 and np.abs(uWS[:, 1]).max() <= 0.4
    step = np.hypot(np.diff(xWS[:, 0]), np.diff(xWS[:, 1]))
    assert step.max() < 1.5 * step.mean()                                       # uniform in arc length
    # batch helper: same result per instance, in order
    r = PL.warm_start_many(sc, np.stack([sc["x0"]] * 4), np.stack([sc["xF"]] * 4), N, workers=2)
    assert all(np.array_equal(q[1], xWS) for q in r)


def test_planner_library_exports_every_symbol_of_its_header():
    import ctypes as C, os, re
    from conftest import ROOT
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "obca_plan.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(obca_plan_[a-z_0-9]+)\s*\(", txt)))
    lib = C.CDLL(PL.build_library())
    assert syms == ["obca_plan_astar3d", "obca_plan_collides", "obca_plan_hybrid_astar", "obca_plan_hybrid_astar2", "obca_plan_hybrid_astar_batch", "obca_plan_hybrid_astar_batch2",
                    "obca_plan_reeds_shepp", "obca_plan_reference_astar3d", "obca_plan_reference_hybrid_astar"] and all(hasattr(lib, s) for s in syms)


def test_option_arrays_carry_their_length_and_the_old_entry_point_reads_fourteen():
    """Round 5 made obca_plan_hybrid_astar read opts[14], opts[15] from an array documented as 14 doubles (an out-of-bounds read for every older caller).  Now: the *2 entry points
    take the length; the old symbol reads 14 options and searches with weight 1 / no Reeds-Shepp heuristic -- checked with a 14-double array that ENDS at the end of its buffer's
    readable values (two poison doubles behind it must not matter); a heuristic weight of 0, a negative one, NaN and a bad length are refused."""
    import ctypes as C
    lib = C.CDLL(PL.build_library()); D = C.POINTER(C.c_double); I = C.POINTER(C.c_int)
    sc = S.BACKWARDS; A, b, v = S.scenario_hrep(sc); v = np.ascontiguousarray(v, np.int32); A = np.ascontiguousarray(A, float); b = np.ascontiguousarray(b, float)
    s = np.array(sc["x0"][:3], float); g = np.array(sc["xF"][:3], float); e = np.ascontiguousarray(S.EGO, float); xy = np.ascontiguousarray(S.XYBOUNDS, float)
    od = dict(PL.DEFAULT_OPTS); od.update(PL.SCENARIO_OPTS[sc["name"]][0])
    o16 = np.array([od[k] for k in PL.DEFAULT_OPTS], float)[:16]; assert len(PL.DEFAULT_OPTS) == 18
    cap = 4096

    def run(fn, opts, nopts=None):
        path = np.zeros((cap, 3)); dr = np.zeros(cap, np.int32); ne = C.c_int(0)
        a = [s.ctypes.data_as(D), g.ctypes.data_as(D), C.c_int(len(v)), v.ctypes.data_as(I), A.ctypes.data_as(D), b.ctypes.data_as(D), e.ctypes.data_as(D), C.c_double(S.L_WHEELBASE), xy.ctypes.data_as(D),
             opts.ctypes.data_as(D) if opts is not None else None]
        if nopts is not None: a.append(C.c_int(nopts))
        n = getattr(lib, fn)(*a, path.ctypes.data_as(D), dr.ctypes.data_as(I), C.c_int(cap), C.byref(ne))
        return n, path[:max(n, 0)].copy(), ne.value
    w1 = o16.copy(); w1[14] = 1.0; w1[15] = 0.0
    n_ref, p_ref, e_ref = run("obca_plan_hybrid_astar2", w1, 16)
    assert n_ref >= 2
    for tail in (1e300, -1.0, np.nan):      # what lies behind a 14-double array must not be read
        buf = np.concatenate([w1[:14], [tail, tail]])
        n, p, ne = run("obca_plan_hybrid_astar", buf)
        assert n == n_ref and ne == e_ref and np.array_equal(p, p_ref), tail
        n, p, ne = run("obca_plan_hybrid_astar2", buf, 14)
        assert n == n_ref and ne == e_ref and np.array_equal(p, p_ref), tail
    n15, _, e15 = run("obca_plan_hybrid_astar2", np.concatenate([w1[:14], [1.5]]), 15)
    assert n15 >= 2 and e15 != e_ref                     # fifteen options: the weight is taken (another search order)
    for bad in (0.0, -2.0, np.nan, np.inf):
        w = w1.copy(); w[14] = bad
        assert run("obca_plan_hybrid_astar2", w, 16)[0] == -1, bad
    assert run("obca_plan_hybrid_astar2", np.concatenate([w1, [0.0, 7.5, 1.0]]), 19)[0] == -1 and run("obca_plan_hybrid_astar2", w1, -1)[0] == -1
    assert run("obca_plan_hybrid_astar2", np.concatenate([w1, [-1.0, 7.5]]), 18)[0] == -1      # a negative lattice cell
    assert run("obca_plan_hybrid_astar2", None, 0)[0] >= 2


def test_astar3d_waypoints_clear_the_boxes_and_warm_start_the_quadcopter_nlp():
    """3-D grid A* (the a_star_3D.jl step): way-points stay outside the inflated boxes; the oracle converges from the resampled path"""
    import oracle_quad as Q
    wp = PL.astar3d(S.QUAD_X0, S.QUAD_XF, clear=0.4)
    assert np.allclose(wp[0], S.QUAD_X0[:3]) and np.allclose(wp[-1], S.QUAD_XF[:3]) and len(wp) > 10
    hi = S.QUAD_OB[:, :3]; lo = -S.QUAD_OB[:, 3:]
    d = np.linalg.norm(wp[:, None, :] - np.clip(wp[:, None, :], lo[None], hi[None]), axis=2)
    assert d.min() >= 0.4 - 1e-9 and np.linalg.norm(np.diff(wp, axis=0), axis=1).max() <= 0.25 * np.sqrt(3) + 0.26
    assert PL.astar3d([2.2, 5.0, 2.0], S.QUAD_XF) is None            # start inside the first wall
    bt = S.make_quad_batch(4, 40, random_endpoints=True)
    for i in range(4):
        r = Q.quadcopter_signed_dist(bt["x0"][i], bt["xF"][i], 40, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], 1.0)
        assert r["exitflag"] == 1 and r["slack"].sum() < 1e-3


def test_velo_smooth_ramps_the_planner_speed_profile():
    """veloSmooth.jl restated (planner.velo_smooth): jumps of the piecewise-constant +-v_nom profile become ramps of slope amax; the middle of
    a long constant segment is untouched; signs are kept; the profile starts from rest and ends at rest"""
    from obca_amd.planner import velo_smooth
    vn, amax, Ts = 0.5, 0.3, 0.12
    acc = int(round(vn / amax / Ts))
    v = np.r_[np.full(40, vn), np.full(35, -vn), np.full(30, vn), 0.0]
    vs, a = velo_smooth(v, amax, Ts)
    assert vs.shape == v.shape and a.shape == (len(v) - 1,)
    assert np.abs(a).max() <= amax * 1.02 and np.allclose(a, np.diff(vs) / Ts)
    assert vs[0] == 0.0 and vs[-1] == 0.0
    assert np.all(vs[:40] >= 0) and np.all(vs[40:75] <= 0) and np.all(vs[75:] >= 0)          # never against the planner's direction
    assert np.all(np.abs(vs) <= vn + 1e-12)
    assert np.allclose(vs[acc:40 - acc], vn) and np.allclose(vs[40 + acc:75 - acc], -vn)      # plateaus between the ramps
    assert np.allclose(vs[:acc + 1], np.linspace(0, vn, acc + 1))                              # start ramp
    k = int(np.argmin(np.abs(vs[30:50]))) + 30
    assert abs(k - 40) <= 1                                                                    # the reversal ramp is centred on the switch
    # a profile that only drives backwards (the reverse-parking scenario)
    vs2, a2 = velo_smooth(np.r_[np.full(50, -vn), 0.0], amax, Ts)
    assert vs2[0] == 0.0 and vs2[-1] == 0.0 and np.all(vs2 <= 0) and np.abs(a2).max() <= amax * 1.02


def test_reeds_shepp_paths_reach_the_goal_and_respect_the_symmetries():
    """obca_plan_reeds_shepp (the planner's analytic expansion, reeds_shepp.jl in the reference): every path ends exactly on the goal pose, never
    turns tighter than R, is no shorter than the straight line, and its length is invariant under the time-flip and reflection symmetries of
    the problem (a missing family would break one of them); known closed-form cases"""
    rng = np.random.default_rng(11); words = set()
    for t in range(1500):
        R = rng.uniform(0.5, 5.0)
        s = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-np.pi, np.pi)])
        g = np.array([s[0] + rng.uniform(-12, 12), s[1] + rng.uniform(-12, 12), rng.uniform(-np.pi, np.pi)])
        if t % 4 == 0: g[:2] = s[:2] + rng.uniform(-1, 1, 2) * R                 # near goals: the CCC / CCCC words
        path, dr, word, seg, tot = PL.reeds_shepp(s, g, R, step=0.05)
        words.add(word)
        assert np.hypot(*(path[-1, :2] - g[:2])) < 1e-9 and abs((path[-1, 2] - g[2] + np.pi) % (2 * np.pi) - np.pi) < 1e-9
        assert np.allclose(path[0], [s[0], s[1], (s[2] + np.pi) % (2 * np.pi) - np.pi]) and abs(np.abs(seg).sum() - tot) < 1e-9
        assert tot >= np.hypot(*(g[:2] - s[:2])) - 1e-9
        d = np.hypot(np.diff(path[:, 0]), np.diff(path[:, 1])); dyaw = np.abs((np.diff(path[:, 2]) + np.pi) % (2 * np.pi) - np.pi)
        assert np.all(dyaw <= d / R * (1 + 1e-3) + 1e-9) and abs(d.sum() - tot) < 5e-3 * max(1.0, tot)      # curvature <= 1/R, samples follow the path
    assert len(words) >= 16                                                       # all families of words occur
    for t in range(300):                                                          # symmetries, normalised problem
        x, y = rng.uniform(-4, 4, 2) if t % 2 else rng.uniform(-1.5, 1.5, 2); phi = rng.uniform(-np.pi, np.pi)
        L0 = PL.reeds_shepp([0, 0, 0], [x, y, phi], 1.0)[4]
        for q in ([x, -y, -phi], [-x, y, -phi], [-x, -y, phi]):
            assert abs(PL.reeds_shepp([0, 0, 0], q, 1.0)[4] - L0) < 1e-9
    assert abs(PL.reeds_shepp([0, 0, 0], [3, 0, 0], 1.0)[4] - 3.0) < 1e-12 and abs(PL.reeds_shepp([0, 0, 0], [-3, 0, 0], 1.0)[4] - 3.0) < 1e-12
    assert abs(PL.reeds_shepp([0, 0, 0], [1, 1, np.pi / 2], 1.0)[4] - np.pi / 2) < 1e-12       # a quarter turn to the left
    assert PL.reeds_shepp([0, 0, 0], [0, 0.5, 0], 1.0)[4] < 2.5                                 # a sideways shift needs cusps, not a full circle


def test_hybrid_astar_finishes_on_the_exact_goal_with_the_analytic_expansion(backwards):
    """with the Reeds-Shepp expansion the planner's path ends ON the goal pose (without it: within the goal tolerance), is collision-free
    pose by pose, and needs fewer expansions"""
    A, b, v = backwards["A"], backwards["b"], backwards["vOb"]
    x0 = np.array([-6.0, 9.5, 0.0]); xF = S.BACKWARDS["xF"][:3]
    p1, d1, n1 = PL.hybrid_astar(x0, xF, v, A, b)
    p0, d0, n0 = PL.hybrid_astar(x0, xF, v, A, b, analytic=0)
    assert np.hypot(*(p1[-1, :2] - xF[:2])) < 1e-9 and abs((p1[-1, 2] - xF[2] + np.pi) % (2 * np.pi) - np.pi) < 1e-9
    assert np.hypot(*(p0[-1, :2] - xF[:2])) <= 0.3 + 1e-9 and n1 <= n0
    for q in p1:
        assert not PL.collides(q, v, A, b, margin=0.1 - 1e-9)
    assert np.all(np.hypot(np.diff(p1[:, 0]), np.diff(p1[:, 1])) <= 0.2 + 1e-6)


def _check_path(path, start, goal, step, pose_tol=0.01, step_tol=0.001):
    """the reference's acceptance criteria for a Reeds-Shepp path (reeds_shepp.jl:846-869, check_path): starts on the start pose, ends on the end pose
    (x, y, yaw to 0.01), course sampled every STEP_SIZE (0.001; the reference's loop `for i in length(d)` only looks at the last interior step -- here all of them)"""
    ang = lambda a, b: abs((a - b + np.pi) % (2 * np.pi) - np.pi)
    assert abs(path[0, 0] - start[0]) <= pose_tol and abs(path[0, 1] - start[1]) <= pose_tol and ang(path[0, 2], start[2]) <= pose_tol
    assert abs(path[-1, 0] - goal[0]) <= pose_tol and abs(path[-1, 1] - goal[1]) <= pose_tol and ang(path[-1, 2], goal[2]) <= pose_tol
    d = np.hypot(np.diff(path[:-1, 0]), np.diff(path[:-1, 1]))
    # the reference walks STEP_SIZE along the word and adds the segment ends (its own test only looks at ONE step, `for i in length(d)`); this planner spaces the
    # samples of every segment evenly, at most STEP_SIZE of arc apart (a chord is shorter than its arc): never farther apart than the reference's, rarely much closer
    assert d.max() <= step + step_tol
    assert (d >= 0.5 * step).mean() > 0.9


def test_reeds_shepp_reference_test_cases():
    """The six fixed cases of the reference's own Reeds-Shepp test (reeds_shepp.jl:871-932; tests/golden/reeds_shepp_cases.json) -- the only numerical fixtures the
    reference holds.  (1) obca_plan_reeds_shepp passes the reference's acceptance criteria; (2) the restatement of the reference's path families
    (oracle/reeds_shepp_ref.py) is pinned by the same criteria: every candidate word ends on the goal pose; (3) the planner returns the word and the length the
    reference's calc_shortest_path selects, to 1e-9."""
    import json, os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import reeds_shepp_ref as R
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reeds_shepp_cases.json")))
    ang = lambda a, b: abs((a - b + np.pi) % (2 * np.pi) - np.pi)
    assert len(g["cases"]) == 6
    for c in g["cases"]:
        path, dr, w, seg, tot = PL.reeds_shepp(c["start"], c["goal"], 1.0 / c["maxc"], step=g["step_size"])
        _check_path(path, c["start"], c["goal"], g["step_size"], g["pose_tol"], g["step_tol"])
        cands = R.calc_paths(c["start"], c["goal"], c["maxc"])
        assert len(cands) >= 1                                             # check_path: `@test length(paths) >= 1`
        for L, ls, word in cands:
            ex, ey, eth = R.end_pose(c["start"], [l * c["maxc"] for l in ls], word, c["maxc"])
            assert abs(ex - c["goal"][0]) <= 1e-9 and abs(ey - c["goal"][1]) <= 1e-9 and ang(eth, c["goal"][2]) <= 1e-9
        best = R.shortest(c["start"], c["goal"], c["maxc"])
        assert w == best[2] and abs(tot - best[0]) <= 1e-9 * max(1.0, tot)
        assert np.abs(np.asarray(seg) - np.asarray(best[1])).max() <= 1e-8 * max(1.0, tot)
        assert w == c["regression_word"] and abs(tot - c["regression_length"]) <= 1e-9 * max(1.0, tot)


def test_reeds_shepp_random_cases_against_the_reference_families():
    """the reference's random test (reeds_shepp.jl:934-945: poses in [-50, 50]^2 x [-180, 180] deg, max curvature U[0, 0.1]): the planner's path meets the reference's
    criteria and is never longer than the shortest word of the reference's families (it knows all 48 Reeds-Shepp words; the reference's family set is not complete)"""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import reeds_shepp_ref as R
    rng = np.random.default_rng(20260925); equal = 0
    for i in range(100):
        s = [rng.uniform(-50, 50), rng.uniform(-50, 50), np.deg2rad(rng.uniform(-180, 180))]; e = [rng.uniform(-50, 50), rng.uniform(-50, 50), np.deg2rad(rng.uniform(-180, 180))]
        maxc = max(rng.uniform(0, 0.1), 0.005)                           # (a radius beyond 200 m only makes the sampled path long)
        path, dr, w, seg, tot = PL.reeds_shepp(s, e, 1.0 / maxc, step=0.5)
        _check_path(path, s, e, 0.5, step_tol=0.005)
        best = R.shortest(s, e, maxc)
        assert tot <= best[0] + 1e-9 * max(1.0, tot), (i, tot, best)
        equal += abs(tot - best[0]) <= 1e-9 * max(1.0, tot)
    assert equal >= 80


def test_batched_search_on_library_threads_equals_the_single_calls():
    """obca_plan_hybrid_astar_batch (threads inside the library, one shared work counter) returns exactly what one obca_plan_hybrid_astar call per pair returns,
    colliding start poses included; warm_start_many is built on it"""
    rng = np.random.default_rng(11)
    x0, xF = S.sample_poses(S.BACKWARDS, 24, rng, False)
    x0[3, :2] = [0.0, -5.0]                                      # inside an obstacle: no path
    A, b, v = S.scenario_hrep(S.BACKWARDS)
    many = PL.hybrid_astar_many(x0[:, :3], xF[:, :3], v, A, b, threads=4)
    for i in range(len(x0)):
        try:
            one = PL.hybrid_astar(x0[i, :3], xF[i, :3], v, A, b)
        except ValueError:
            one = None
        assert (one is None) == (many[i] is None)
        if one is not None:
            assert np.array_equal(one[0], many[i][0]) and np.array_equal(one[1], many[i][1]) and one[2] == many[i][2]
    assert many[3] is None
    ws = PL.warm_start_many(S.BACKWARDS, x0, xF, 80, workers=3)
    ref = [PL.warm_start(S.BACKWARDS, x0[i], xF[i], 80) for i in range(len(x0))]
    for a_, b_ in zip(ws, ref):
        assert (a_ is None) == (b_ is None)
        if a_ is not None:
            assert a_[0] == b_[0] and np.array_equal(a_[1], b_[1]) and np.array_equal(a_[2], b_[2])


def _ref_rect_hit(x, y, yaw, px, py):
    """the reference's point-in-car test (collision_check.jl:57-98) written independently of the product: signed angles subtended by the four edges of the car
    rectangle (3.7 m ahead of / 1.0 m behind the rear axle, 2.0 m wide) at the obstacle point; a sum of pi or more means the point lies inside"""
    c, s = np.cos(-yaw), np.sin(-yaw); lx = c * (px - x) - s * (py - y); ly = s * (px - x) + c * (py - y)
    vx = np.array([3.7, 3.7, -1.0, -1.0, 3.7]) - lx; vy = np.array([-1.0, 1.0, 1.0, -1.0, -1.0]) - ly
    tot = 0.0
    for i in range(4):
        d = np.hypot(vx[i], vy[i]) * np.hypot(vx[i + 1], vy[i + 1]); cosang = min((vx[i] * vx[i + 1] + vy[i] * vy[i + 1]) / d, 1.0)
        cross = vx[i] * vy[i + 1] - vy[i] * vx[i + 1]
        tot += np.arccos(cosang) if cross >= 0 else -np.arccos(cosang)
    return tot >= np.pi


@pytest.mark.parametrize("name", ["backwards", "parallel"])
def test_reference_mode_search_reproduces_the_reference_call(name):
    """REFERENCE mode (obca_planner_ref.cpp: hybrid_a_star.jl restated) on main.jl's own call: the scenario's point cloud (main.jl:111-133 / 172-198), start
    x0 = (-6, 9.5, 0), the reference's grid constants.  The path starts on the start pose, ends on the goal pose, advances 0.1 m per pose (the Euler steps of
    calc_next_node / the sampling of the analytic expansion), never turns tighter than the steering lock allows and every pose passes the reference's own
    collision test, evaluated here by an independent restatement."""
    sc = S.BACKWARDS if name == "backwards" else S.PARALLEL
    ox, oy = S.reference_obstacle_points(sc)
    assert len(ox) == (257 if name == "backwards" else 230)                      # 108 + 8 + 8 + 108 + 25 / 91 + 8 + 7 + 8 + 91 + 25 points
    r = PL.reference_hybrid_astar(sc["x0"][:3], sc["xF"][:3], ox, oy)
    assert r is not None
    path, nexp = r
    assert np.abs(path[0] - sc["x0"][:3]).max() < 1e-12 and np.abs(path[-1, :2] - sc["xF"][:2]).max() < 1e-9
    assert abs(np.angle(np.exp(1j * (path[-1, 2] - sc["xF"][2])))) < 1e-9
    d = np.hypot(np.diff(path[:, 0]), np.diff(path[:, 1]))
    assert d.max() <= 0.1 + 1e-9 and d.min() > 0.05                              # (the last sample of a Reeds-Shepp segment may be shorter)
    dyaw = np.abs(np.angle(np.exp(1j * np.diff(path[:, 2]))))
    assert dyaw.max() <= 0.1 * np.tan(0.6) / 2.7 + 1e-9                           # |d yaw| <= step * tan(max steer) / wheelbase
    for x, y, yaw in path:
        cx, cy = x + 1.35 * np.cos(yaw), y + 1.35 * np.sin(yaw)
        near = np.hypot(ox - cx, oy - cy) <= 2.35
        assert not any(_ref_rect_hit(x, y, yaw, px, py) for px, py in zip(ox[near], oy[near]))
    assert 1 <= nexp < 20000


def test_reference_mode_node_costs_follow_the_reference_constants():
    """a switch-back costs 10, reverse arcs are free, a steer change costs 10 per radian (hybrid_a_star.jl:60-63): with the switch-back cost raised the search must not
    return a path with MORE direction changes; with every cost but the arc length removed the path is not longer than with the reference's costs"""
    sc = S.PARALLEL; ox, oy = S.reference_obstacle_points(sc)
    def switches(path):
        s = np.sign(np.diff(path[:, 0]) * np.cos(path[:-1, 2]) + np.diff(path[:, 1]) * np.sin(path[:-1, 2])); s = s[s != 0]
        return int((np.diff(s) != 0).sum())
    base = PL.reference_hybrid_astar(sc["x0"][:3], sc["xF"][:3], ox, oy)[0]
    dear = PL.reference_hybrid_astar(sc["x0"][:3], sc["xF"][:3], ox, oy, switch_cost=100.0)[0]
    assert switches(dear) <= switches(base)
    plain = PL.reference_hybrid_astar(sc["x0"][:3], sc["xF"][:3], ox, oy, switch_cost=0.0, steer_change_cost=0.0, reverse_cost=1.0)[0]
    length = lambda p: np.hypot(np.diff(p[:, 0]), np.diff(p[:, 1])).sum()
    assert length(plain) <= length(base) + 0.5


def test_reference_warm_start_pipeline_matches_main_jl():
    """main.jl:216-252 on the reference search: speed from the path differences at Ts / sampleN per step (0.5 m/s backwards, 0.333 m/s parallel), veloSmooth at
    0.3 m/s^2, steering from the yaw differences, every third sample; the horizon is what the path length gives (N = samples - 1)"""
    for sc, vnom in ((S.BACKWARDS, 0.5), (S.PARALLEL, 1.0 / 3.0)):
        N, Ts, xWS, uWS, path = PL.reference_warm_start(sc, sc["x0"], sc["xF"])
        assert Ts == sc["Ts"] and xWS.shape == (N + 1, 4) and uWS.shape == (N, 2) and N == (len(path) - 1) // 3
        assert np.array_equal(xWS[:, :3], path[::3]) and np.abs(xWS[:, 3]).max() <= vnom + 1e-9
        assert np.abs(uWS[:, 0]).max() <= 0.6 + 1e-9 and np.abs(uWS[:, 1]).max() <= 0.32      # steering lock; the ramps of the smoother take round(v / 0.3 / dt) samples, so their slope is 0.3 up to that rounding (0.3125)
        assert abs(xWS[0, 3]) < 1e-12 or abs(xWS[0, 3]) <= vnom                                        # (the smoother ramps up from rest)


def test_reference_astar3d_restated_on_the_reference_call():
    """QuadcopterNavigation/a_star_3D.jl restated (REFERENCE mode, obca_plan_reference_astar3d) on mainQuadcopter.jl:59-121's own call -- the two point walls, room 105 x 105 x 55,
    start (10, 10, 30), goal (90, 30, 20), grid 1.0.  The reference ships no output for it, so the pin is (a) the definition, checked independently: every way-point is a cell whose
    NEAREST obstacle point (the two appended room corners included, :196-198) is farther than VEHICLE_RADIUS = 2.5, strictly inside the room (:118-123), consecutive way-points
    are 26-neighbours, the path starts on the start cell and ends on the goal cell TWICE (get_final_path pushes the goal and then walks the closed set from the goal, :243-250);
    (b) weighted A* with H_WEIGHT = 1.1 and a consistent heuristic is at most 1.1 x the optimum: against scipy's Dijkstra on the same 26-connected grid; (c) the numbers the
    caller derives (:129-131): N_as = 99, Ts_as = 0.2 -- a regression fixture of THIS restatement."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    ox, oy, oz = PL.reference_quad_obstacle_points()
    assert len(ox) == 67494                                             # 6 x 106 x 50 + 6 x (41 x 56 + 56 x 56 + 11 x 26 + 11 x 21)
    s3, g3 = np.array([10.0, 10.0, 30.0]), np.array([90.0, 30.0, 20.0])
    wp, nexp, cost = PL.reference_astar3d(s3, g3, ox, oy, oz)
    assert np.array_equal(wp[0], s3) and np.array_equal(wp[-1], g3) and np.array_equal(wp[-2], g3) and len(wp) == 100
    st = np.abs(np.diff(wp[:-1], axis=0))
    assert st.max() == 1.0 and (st.sum(1) >= 1).all()
    assert abs(np.sqrt((np.diff(wp[:-1], axis=0) ** 2).sum(1)).sum() - cost) < 1e-9
    pts = np.stack([np.append(ox, [0.0, 105.0]), np.append(oy, [0.0, 105.0]), np.append(oz, [0.0, 55.0])], axis=1)
    for p in wp:
        assert np.sqrt(((pts - p) ** 2).sum(1)).min() > 2.5 and (p > 0).all() and (p < [105, 105, 55]).all()
    # (b) the optimum on the same map: blocked = nearest obstacle point within 2.5, cells x, y, z in 1 .. width - 1
    X, Y, Z = 105, 105, 55
    blocked = np.zeros((X, Y, Z), bool)
    r = 3
    off = np.array([(a, b, c) for a in range(-r, r + 1) for b in range(-r, r + 1) for c in range(-r, r + 1) if a * a + b * b + c * c <= 6.25])
    ip = pts.astype(int)                                                # (all obstacle points lie on integer coordinates here)
    for o in off:
        q = ip + o; ok = ((q >= 0) & (q < [X, Y, Z])).all(1); blocked[q[ok, 0], q[ok, 1], q[ok, 2]] = True
    blocked[0] = blocked[:, 0] = blocked[:, :, 0] = True               # (node - min) <= 0 is outside the search (:118-123)
    idx = np.arange(X * Y * Z).reshape(X, Y, Z); rows, cols, w = [], [], []
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for c in (-1, 0, 1):
                if (a, b, c) <= (0, 0, 0):
                    continue
                sl = lambda d, n: (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
                (xa, xb), (ya, yb), (za, zb) = sl(a, X), sl(b, Y), sl(c, Z)
                free = ~blocked[xa, ya, za] & ~blocked[xb, yb, zb]
                rows.append(idx[xa, ya, za][free]); cols.append(idx[xb, yb, zb][free]); w.append(np.full(int(free.sum()), np.sqrt(a * a + b * b + c * c)))
    G = sp.csr_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(X * Y * Z, X * Y * Z))
    d = dijkstra(G, directed=False, indices=idx[10, 10, 30])[idx[90, 30, 20]]
    assert d <= cost + 1e-9 <= 1.1 * d + 1e-9, (d, cost)
    # (c) what mainQuadcopter.jl derives from the path
    N_as, Ts_as, xWS, uWS, wpm = PL.reference_quad_warm_start()
    assert N_as == 99 and Ts_as == 0.2 and xWS.shape == (100, 12) and np.abs(xWS[:, :3] - wp / 10).max() == 0 and (xWS[:, 3:] == 0).all() and (uWS == 0.5).all()


def test_lattice_heuristic_plans_are_valid_and_cheaper_to_find():
    """options 16, 17 (round 6): the non-holonomic-with-obstacles cost-to-go on a coarse (x, y, yaw, direction) lattice as a third heuristic -- one backward Dijkstra per batch.
    24 parallel-parking searches with randomised starts and goals: every plan collision-free and at its goal as with the default heuristics, in fewer expansions; one shared table
    serves goals a metre apart (the batch call) and gives exactly what a table of the search's own gives when the goal is the table's."""
    sc = S.PARALLEL; A, b, v = S.scenario_hrep(sc)
    rng = np.random.default_rng(7); B = 24
    x0 = np.stack([rng.uniform(-10, 10, B), rng.uniform(6.5, 9.5, B), rng.uniform(-0.2, 0.2, B)], 1)
    xF = np.stack([rng.uniform(-1.85, -0.85, B), np.full(B, 4.0), np.zeros(B)], 1)
    o = dict(PL.SCENARIO_OPTS["parallel"][0])
    base = PL.hybrid_astar_many(x0, xF, v, A, b, threads=4, **o)
    nh = PL.hybrid_astar_many(x0, xF, v, A, b, threads=4, **dict(o, nh_res=0.25, nh_yaw_res_deg=7.5, rs_heuristic=0, h_weight=1.5))
    nb = ne = 0
    for i in range(B):
        assert (base[i] is None) == (nh[i] is None), i
        if nh[i] is None:
            continue
        path, dr, nexp = nh[i]
        assert np.allclose(path[0], x0[i]) and np.hypot(*(path[-1, :2] - xF[i, :2])) <= 0.3 + 1e-9 and abs((path[-1, 2] - xF[i, 2] + np.pi) % (2 * np.pi) - np.pi) <= np.deg2rad(8) + 1e-9
        assert not any(PL.collides(p, v, A, b) for p in path[::3])
        nb += base[i][2]; ne += nexp
    assert ne < 0.7 * nb, (ne, nb)
    # the single call builds its own table: for the batch's median goal the two are the same search
    gm = np.array([np.partition(xF[:, 0], B // 2)[B // 2], 4.0, 0.0]); k = int(np.argmin(np.abs(xF[:, 0] - gm[0])))
    if nh[k] is not None and abs(xF[k, 0] - gm[0]) < 1e-12:
        one = PL.hybrid_astar(x0[k], xF[k], v, A, b, **dict(o, nh_res=0.25, nh_yaw_res_deg=7.5, rs_heuristic=0, h_weight=1.5))
        assert one[2] == nh[k][2] and np.array_equal(one[0], nh[k][0])
