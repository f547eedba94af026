"""Receding-horizon restart of the resident quadcopter batch (QuadBatch.shift_warm_start / obca_quad_batch_shift_warm_start) on the GPU, through the C ABI, against the CPU
checker started from the host build of the same shift text (tests/quad_shift_common.py) applied to the GPU's OWN previous solution: the quadcopter optimum has flat directions
(test_gpu_quad_parity.py), so a checker started from its own previous solution would start somewhere else."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Q():
    import oracle_quad
    oracle_quad.lib()
    return oracle_quad


def _opts(Q, reference, warm, max_iter=None):
    """(library options, checker options): the throughput defaults or the reference's switches, cold or with the warm-restart values"""
    import obca_amd
    if warm:
        o = obca_amd.quad_warm_restart_opts(reference=reference)
        assert o.mu_init == o.bound_push == o.bound_frac == 1e-4 and (o.max_soc, o.lsq_init, o.obj_scaling) == ((4, 1, 1) if reference else (0, 0, 0)) and o.max_iter == 3000
    else:
        o = obca_amd.quadcopter_ipopt_opts() if reference else obca_amd.quadcopter_default_opts()
    oo = Q.default_opts()
    if reference:
        oo.max_soc = 4; oo.lsq_init = 1; oo.obj_scaling = 1
    if warm:
        oo.mu_init = oo.bound_push = oo.bound_frac = 1e-4
    if max_iter is not None:
        o.max_iter = oo.max_iter = max_iter
    return o, oo


def _batch(bt, B, N, dist=False):
    import obca_amd
    from obca_amd.api import _ctx
    qb = obca_amd.QuadBatch(_ctx(0), B, N)
    qb.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"], dist=dist)
    return qb


def _shifted(bt, N, shift, o1, i, **kw):
    import quad_shift_common as QS
    return QS.shifted_problem(N, shift, bt["x0"][i], bt["xF"][i], bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], bt["timeWS"], 1, o1, i, **kw)


def _same_bits(a, b, idx=slice(None)):
    return all(np.array_equal(a[k][idx], b[k][idx], equal_nan=True) for k in ("xp", "up", "timeScale", "lp", "slack", "info", "exitflag"))


@pytest.mark.parametrize("reference,dist", [(0, 0), (1, 0), (0, 1)], ids=["throughput", "reference", "dist"])
def test_restart_parity_through_the_c_abi(Q, reference, dist):
    """solve, shift 3 on the device, solve with the warm-restart options: against the checker started from the host-built shift of the GPU's own first solution, at the bars of
    test_quad_batch_parity_and_feasibility (exit flags equal, objective 1e-8 relative, t 1e-8, inputs 1e-4, states 1e-3, counts differing on at most 1 of 6)"""
    from obca_amd import scenarios as S
    B, N, shift = 6, 30, 3
    bt = S.make_quad_batch(B, N)
    qb = _batch(bt, B, N, dist=bool(dist))
    qb.solve(opts=_opts(Q, reference, False)[0]); o1 = qb.download()
    assert np.isin(o1["exitflag"], (1, 2)).all(), o1["exitflag"]
    qb.shift_warm_start(shift)
    o, oo = _opts(Q, reference, True)
    qb.solve(opts=o); o2 = qb.download(); qb.close()
    assert np.array_equal(o2["xp"][:, :, 0], o1["xp"][:, :, shift])
    flips = []
    for i in range(B):
        s = _shifted(bt, N, shift, o1, i)
        assert s["dual_ws"] == 1 and s["timeWS"] == o1["timeScale"][i, 0]
        r = Q.quadcopter_signed_dist(s["x0"], s["xF"], N, bt["Ts"], bt["R"], bt["ob"], s["xWS"], s["timeWS"], opts=oo, dual_ws=s["dual_ws"], dist=dist)
        print("instance %d: cold %d iterations, restart %d (checker %d), exit flag %d (%d)" % (i, o1["iters"][i], o2["iters"][i], r["iters"], o2["exitflag"][i], r["exitflag"]))
        assert r["exitflag"] == o2["exitflag"][i], (i, r["exitflag"], o2["exitflag"][i])
        if r["exitflag"] == 1:
            assert abs(o2["obj"][i] - r["obj"]) < 1e-8 * abs(r["obj"]), (i, o2["obj"][i], r["obj"])
            assert abs(o2["timeScale"][i, 0] - r["t"]) < 1e-8 and np.abs(o2["up"][i] - r["up"]).max() < 1e-4, i
            assert np.abs(o2["xp"][i] - r["xp"]).max() < 1e-3, i
            if o2["iters"][i] != r["iters"] or o2["info"][i, 6] != r["nreg"]:
                flips.append((i, int(o2["iters"][i]), r["iters"]))
    assert len(flips) <= 1, flips


@pytest.mark.parametrize("N,shift", [(64, 1), (65, 64), (128, 127), (30, 0), (30, 30)])
def test_starting_point_after_the_shift_at_loop_edges(Q, N, shift):
    """max_iter = 0 after the shift returns the starting point of the restart (status 1, no iteration): every returned quantity against the checker's max_iter = 0 call from the
    host-built shift, relative to max(1, |checker|) to 1e-8 -- the bar of test_quad_first_iterates_match_the_oracle_tightly; both option sets"""
    from obca_amd import scenarios as S
    B = 2; bt = S.make_quad_batch(B, N, seed=N)
    for reference in (0, 1):
        qb = _batch(bt, B, N)
        qb.solve(opts=_opts(Q, reference, False)[0]); o1 = qb.download()
        assert np.isin(o1["exitflag"], (1, 2)).all(), (reference, o1["exitflag"])
        qb.shift_warm_start(shift)
        o, oo = _opts(Q, reference, True, max_iter=0)
        qb.solve(opts=o); o2 = qb.download(); qb.close()
        for i in range(B):
            s = _shifted(bt, N, shift, o1, i)
            r = Q.quadcopter_signed_dist(s["x0"], s["xF"], N, bt["Ts"], bt["R"], bt["ob"], s["xWS"], s["timeWS"], opts=oo, dual_ws=s["dual_ws"])
            tag = (N, shift, reference, i)
            assert r["status"] == 1 and r["iters"] == 0, tag + (r["status"], r["iters"])      # the checker's max_iter = 0 is its starting point
            assert o2["status"][i] == 1 and o2["iters"][i] == 0 and o2["info"][i, 6] == r["nreg"], tag + (int(o2["status"][i]), int(o2["iters"][i]))
            dev = {q: np.abs(o2[q][i] - r[q]).max() / max(1.0, np.abs(r[q]).max()) for q in ("xp", "up", "timeScale", "lp", "slack")}
            for j, q in ((2, "obj"), (3, "pinf"), (4, "dinf"), (5, "mu")):
                dev[q] = abs(o2["info"][i, j] - r[q]) / max(1.0, abs(r[q]))
            q = max(dev, key=dev.get)
            print("N %d shift %d reference %d instance %d: worst deviation %.2e (%s)" % (N, shift, reference, i, dev[q], q))
            assert dev[q] < 1e-8, tag + (q, dev[q])


def test_measured_state_and_moving_goal():
    from obca_amd import scenarios as S
    import obca_amd
    B, N, shift = 4, 30, 3
    bt = S.make_quad_batch(B, N)
    warm = obca_amd.quad_warm_restart_opts()
    # the measured state: the predicted one, 2 cm off in every position coordinate
    qb = _batch(bt, B, N); qb.solve(); o1 = qb.download()
    assert (o1["exitflag"] == 1).all()
    x0n = o1["xp"][:, :, shift].copy(); x0n[:, :3] += 0.02
    qb.shift_warm_start(shift, x0_new=x0n); qb.solve(opts=warm); o2 = qb.download(); v = qb.validate()
    assert (o2["exitflag"] == 1).all(), o2["exitflag"]
    assert np.array_equal(o2["xp"][:, :, 0], x0n) and v["ok"].all(), v["viol"]
    assert np.abs(o2["xp"][:, :, N] - bt["xF"]).max() < 1e-4
    qb.close()
    # a goal that moved by 0.1 m
    qb = _batch(bt, B, N); qb.solve()
    xFn = bt["xF"].copy(); xFn[:, 0] += 0.1
    qb.shift_warm_start(shift, xF_new=xFn); qb.solve(opts=warm); o3 = qb.download(); v = qb.validate()
    print("moving goal: exit flags %s, iterations %s (cold %s)" % (o3["exitflag"], o3["iters"], o1["iters"]))
    assert np.abs(o3["xp"][:, :, N] - xFn).max() < 1e-4 and v["ok"].all(), v["viol"]
    assert np.array_equal(o3["xp"][:, :, 0], o1["xp"][:, :, shift])
    qb.close()


def test_failed_instance_keeps_its_uploaded_warm_start_and_leaves_its_neighbours_alone():
    """Options belong to a solve, not to an instance: the first solve is capped one iteration below what the slowest instance of the batch needs, so exactly that instance ends
    with exit flag 0 while its neighbours finish.  With max_iter = 3 on the first solve EVERY instance fails: the last part checks that the shift then leaves the whole batch
    as it was uploaded."""
    from obca_amd import scenarios as S
    import obca_amd
    B, N, shift = 4, 30, 3
    bt = S.make_quad_batch(B, N)
    warm = obca_amd.quad_warm_restart_opts()
    # the run without a failure
    qb = _batch(bt, B, N); qb.solve(); o1 = qb.download()
    assert (o1["exitflag"] == 1).all()
    qb.shift_warm_start(shift); qb.solve(opts=warm); ref = qb.download(); qb.close()
    it = o1["iters"]; j = int(np.argmax(it)); others = np.array([i for i in range(B) if i != j])
    assert it[others].max() < it[j], it
    # the same with instance j cut short
    cap = obca_amd.quadcopter_default_opts(); cap.max_iter = int(it[j]) - 1
    qb = _batch(bt, B, N); qb.solve(opts=cap); oc = qb.download()
    assert oc["exitflag"][j] == 0 and (oc["exitflag"][others] == 1).all() and _same_bits(oc, o1, others)
    qb.shift_warm_start(shift); qb.solve(opts=warm); o2 = qb.download(); v = qb.validate(); qb.close()
    assert _same_bits(o2, ref, others)
    assert o2["exitflag"][j] == 1 and v["ok"].all()
    # ... which solved its UPLOADED problem from its uploaded warm start: the bits of a fresh batch solved with the same options
    qb = _batch(bt, B, N); qb.solve(opts=warm); fresh = qb.download(); qb.close()
    assert _same_bits(o2, fresh, [j])
    # every instance failed after three iterations: the shift leaves the whole problem as uploaded
    cap.max_iter = 3
    qb = _batch(bt, B, N); qb.solve(opts=cap); o3 = qb.download()
    assert (o3["exitflag"] == 0).all() and (o3["iters"] == 3).all()
    qb.shift_warm_start(shift); qb.solve(opts=warm); o4 = qb.download(); qb.close()
    assert _same_bits(o4, fresh)


def test_refusals_leave_the_batch_usable():
    from obca_amd import scenarios as S
    import obca_amd
    B, N = 2, 30
    bt = S.make_quad_batch(B, N)
    qb = _batch(bt, B, N)
    with pytest.raises(obca_amd.ObcaError, match="nothing has been solved"):
        qb.shift_warm_start(1)                                   # before a solve
    qb.solve(); o1 = qb.download()
    with pytest.raises(obca_amd.ObcaError, match="out of range"):
        qb.shift_warm_start(N + 1)
    with pytest.raises(obca_amd.ObcaError, match="out of range"):
        qb.shift_warm_start(-1)
    bad = o1["xp"][:, :, 1].copy(); bad[1, 4] = np.nan
    with pytest.raises(obca_amd.ObcaError, match="non-finite entry in x0_new"):
        qb.shift_warm_start(1, x0_new=bad)
    bad[1, 4] = np.inf
    with pytest.raises(obca_amd.ObcaError, match="non-finite entry in xF_new"):
        qb.shift_warm_start(1, xF_new=bad)
    assert qb.validate()["ok"].all()                             # none of the refused calls touched the batch
    qb.shift_warm_start(1)
    with pytest.raises(obca_amd.ObcaError, match="nothing has been solved"):
        qb.validate()                                            # between shift and solve
    with pytest.raises(obca_amd.ObcaError, match="nothing has been solved"):
        qb.shift_warm_start(1)                                   # a second shift without a solve
    qb.solve(opts=obca_amd.quad_warm_restart_opts()); o2 = qb.download()
    assert (o2["exitflag"] == 1).all() and qb.validate()["ok"].all() and np.array_equal(o2["xp"][:, :, 0], o1["xp"][:, :, 1])
    qb.close()
    fresh = obca_amd.QuadBatch(obca_amd.api._ctx(0), B, N)
    with pytest.raises(obca_amd.ObcaError, match="nothing uploaded"):
        fresh.shift_warm_start(1)
    fresh.close()


def test_upload_solve_shift_solve_is_deterministic():
    from obca_amd import scenarios as S
    import obca_amd
    B, N = 6, 30
    bt = S.make_quad_batch(B, N)
    qb = _batch(bt, B, N); outs = []
    for rep in range(2):
        if rep:
            qb.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
        qb.solve(); a = qb.download()
        qb.shift_warm_start(2); qb.solve(opts=obca_amd.quad_warm_restart_opts()); outs.append((a, qb.download()))
    qb.close()
    assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1])
