"""Receding-horizon restart of the parking batch on the device (obca_batch_shift_warm_start, kernel text obca_amd/csrc/obca_shift.h) through the C ABI.  The oracle is the
checker: it is started from tests/shift_common.py's statement of the shift applied to the device's OWN previous download, so a wrong word of the device's shift shows as a
different starting point -- at max_iter = 0 to 1e-9, the bar of test_gpu_parity.py::test_parking_first_iterates_match_the_oracle_tightly (the objective carries the advanced
reference, pinf the dynamics of the advanced states: a shift off by one stage is orders of magnitude above it) -- or as another iteration path of the full restart."""
import numpy as np
import pytest
from obca_amd import scenarios as S
import shift_common as SC
from test_gpu_parity import TOL_X, TOL_F, _census, _oracle_opts, _sub

pytestmark = pytest.mark.gpu
WARM = 1e-4                                    # mu_init = bound_push = bound_frac of a warm restart (obca_amd.warm_restart_opts)
SCALES = np.array([3.0, 0.25, 100.0, 7.0, 0.5])


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.Context(0).close()      # fails loudly if the HIP library / device is missing
    return obca_amd


@pytest.fixture(scope="module")
def ctx(OA):
    c = OA.Context(0)
    yield c
    c.close()


def _opts(OA, oracle, ref, warm=True, max_iter=None):
    """(device options, oracle options): the default or the reference option set, with the warm-restart values"""
    o = OA.ipopt_opts() if ref else OA.default_opts(); oo = _oracle_opts(oracle, ref, max_iter)
    if warm:
        o.mu_init = o.bound_push = o.bound_frac = WARM; oo.mu_init = oo.bound_push = oo.bound_frac = WARM
    if max_iter is not None:
        o.max_iter = max_iter
    return o, oo


def _uploaded(OA, ctx, bt, dist, b=None):
    """the batch uploaded as the solve calls of test_gpu_parity.py upload it (stage 0 of the warm start = x0, reference = the warm start's poses); returns (batch, xWS)"""
    B, N = len(bt["x0"]), bt["N"]
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = b or OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"], dist=bool(dist))
    return b, xWS


def _reference(xWS):
    """per instance (rx, ry, ryaw) as uploaded"""
    return [(xWS[i, :, 0].copy(), xWS[i, :, 1].copy(), xWS[i, :, 2].copy()) for i in range(len(xWS))]


def _oracle_from(oracle, bt, i, st, oo, dist):
    """the oracle started from a shifted problem `st` (shift_common.numpy_shift) of instance i"""
    ragged = isinstance(bt["vOb"], list)
    v, A, b = (bt["vOb"][i], bt["A"][i], bt["b"][i]) if ragged else (bt["vOb"], bt["A"], bt["b"])
    return oracle.parking_signed_dist(st["x0"], bt["xF"][i], bt["N"], bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], v, A, b, st["rx"], st["ry"], st["ryaw"], 0,
                                      st["xWS"], st["uWS"], st["lWS"], st["nWS"], opts=oo, dist=dist)


def _finite(out, i):
    return all(np.isfinite(np.asarray(out[q][i])).all() for q in ("xp", "up", "lp", "np"))


def _tight(out, i, r, dist, tag):
    """every returned quantity of a max_iter = 0 call against the oracle's, relative to max(1, |oracle|), at 1e-9; returns (worst deviation, its quantity)"""
    assert out["status"][i] == r["status"] == 1 and out["iters"][i] == r["iters"] == 0, tag + (int(out["status"][i]), r["status"], int(out["iters"][i]), r["iters"])
    dev = {q: np.abs(np.asarray(out[q][i]) - r[q]).max() / max(1.0, np.abs(r[q]).max()) for q in ("xp", "up", "lp", "np") + (() if dist else ("sl",))}
    dev["timeScale"] = np.abs(out["timeScale"][i] - r["timeScale"]).max() / max(1.0, np.abs(r["timeScale"]).max())
    for j, q in ((2, "obj"), (3, "pinf"), (4, "dinf"), (5, "mu")):
        dev[q] = abs(out["info"][i, j] - r[q]) / max(1.0, abs(r[q]))
    q = max(dev, key=dev.get)
    print("max_iter=0 after the shift", tag, "worst relative deviation %.3e (%s)" % (dev[q], q))
    assert dev[q] < 1e-9, tag + (q, dev[q])
    return float(dev[q]), q


def _parity(out, i, r, tag):
    """a full restart against the oracle's: exit flag, status, iteration and regularisation counts equal, the point at TOL_X, the objective at TOL_F"""
    tag = tag + (int(out["exitflag"][i]), r["exitflag"], int(out["status"][i]), r["status"], int(out["iters"][i]), r["iters"], int(out["info"][i, 6]), r["nreg"])
    assert out["exitflag"][i] == r["exitflag"] and out["status"][i] == r["status"] and out["iters"][i] == r["iters"] and out["info"][i, 6] == r["nreg"], tag
    assert np.abs(out["xp"][i] - r["xp"]).max() < TOL_X and np.abs(out["up"][i] - r["up"]).max() < TOL_X, tag
    assert abs(out["obj"][i] - r["obj"]) <= TOL_F * max(1, abs(r["obj"])) and abs(out["timeScale"][i, 0] - r["t"]) < 1e-9, tag


def _same_bits(a, b):
    def eq(x, y):
        return np.array_equal(np.ascontiguousarray(x, float).view(np.uint64), np.ascontiguousarray(y, float).view(np.uint64))
    return all(eq(a[k], b[k]) for k in ("xp", "up", "timeScale", "info")) and np.array_equal(a["exitflag"], b["exitflag"]) and \
        all(eq(x, y) for k in ("lp", "np", "sl") for x, y in zip(a[k], b[k]))


# ---------------------------------------------------------------- the starting point after the shift
@pytest.mark.parametrize("N,shift", [(64, 1), (65, 64), (128, 127), (30, 0), (30, 30)])
def test_starting_point_after_the_shift_at_the_loop_edges(OA, ctx, oracle, N, shift):
    """solve, shift, solve with max_iter = 0: what comes back is the start the shift wrote, evaluated (objective, pinf, dinf of the first assembly).  Horizons on both sides
    of the 64- and 128-lane loops, shifts at both ends of the clamps (0: nothing moves; N: every stage is the terminal one; N - 1, 1), both formulations, both option sets."""
    bt = S.make_batch(S.BACKWARDS, 2, N, seed=N); B = 2
    worst = (0.0, "")
    for dist in (0, 1):
        b = None
        for ref in (0, 1):
            b, xWS = _uploaded(OA, ctx, bt, dist, b); ref0 = _reference(xWS)      # (a shift advances the reference in the record: every option set starts from the upload)
            o, _ = _opts(OA, oracle, ref, warm=False); o0, oo0 = _opts(OA, oracle, ref, max_iter=0)
            b.solve(o); o1 = b.download()
            b.shift_warm_start(shift); b.solve(o0); o2 = b.download()
            for i in range(B):
                tag = (N, shift, dist, ref, i)
                assert _finite(o1, i), tag
                r = _oracle_from(oracle, bt, i, SC.shifted_problem(N, shift, o1, i, *ref0[i]), oo0, dist)
                worst = max(worst, _tight(o2, i, r, dist, tag))
                assert np.array_equal(o2["xp"][i][:, 0], o1["xp"][i][:, shift]), tag
        b.close()
    _census("restart_start_N%d_shift%d" % (N, shift), "parking restart, N = %d, shift %d: worst relative deviation of a max_iter = 0 call after the shift from the oracle: %.3e (%s)" % ((N, shift) + worst))


# ---------------------------------------------------------------- full restarts where the index maps differ
def _wide_rows():
    bt = S.make_mixed_batch(24, 20, seed=11, rows=(5, 8), max_extra=4)
    assert np.ravel(bt["vOb"][3]).tolist() == [2, 2, 1, 5, 6, 7, 7]
    return _sub(dict(bt, N=20), [0, 3, 1]), 3, [1]


def _sixteen(with_one):
    bt = S.make_mixed_batch(40, 64, seed=64, min_obstacles=1, max_extra=13, rows=(3, 4), max_rows=64)
    nob = [len(v) for v in bt["vOb"]]
    i16 = nob.index(16); i1 = nob.index(1); mid = [i for i, n in enumerate(nob) if 4 <= n <= 9][0]
    return (_sub(dict(bt, N=64), [i1, i16]), 5, [0, 1]) if with_one else (_sub(dict(bt, N=64), [mid, i16]), 5, [1])


@pytest.mark.parametrize("case,dist", [("rows_up_to_7_N20", 0), ("rows_up_to_7_N20", 1), ("sixteen_obstacles_N64", 0), ("one_beside_sixteen_N64", 0)])
def test_restart_parity_in_ragged_batches(OA, ctx, oracle, case, dist):
    """lambda moves with the instance's own M, mu with its own 4 nOb, inside the record stride of the batch's widest instance: obstacles of up to 7 rows, sixteen obstacles,
    and a 1-obstacle instance beside a 16-obstacle one, each through a ragged upload -- the full restart against the oracle"""
    bt, shift, check = _wide_rows() if case.startswith("rows") else _sixteen(case.startswith("one"))
    N = bt["N"]
    b, xWS = _uploaded(OA, ctx, bt, dist); ref0 = _reference(xWS)
    o, oo = _opts(OA, oracle, 0)
    b.solve(); o1 = b.download()
    b.shift_warm_start(shift); b.solve(o); o2 = b.download(); b.close()
    for i in check:
        tag = (case, dist, i)
        assert _finite(o1, i), tag
        assert o2["lp"][i].shape == (int(np.sum(bt["vOb"][i])), N + 1) and o2["np"][i].shape == (4 * len(bt["vOb"][i]), N + 1), tag
        r = _oracle_from(oracle, bt, i, SC.shifted_problem(N, shift, o1, i, *ref0[i]), oo, dist)
        _parity(o2, i, r, tag)
        assert r["exitflag"] == 1, tag
        assert np.array_equal(o2["xp"][i][:, 0], o1["xp"][i][:, shift]), tag


def test_rows_of_any_length_restart_in_the_callers_scaling(OA, ctx, oracle):
    """the iterate holds lambda for unit-length rows and the shift leaves it there: with rows scaled by (3, 0.25, 100, 7, 0.5) the download hands lambda back in the caller's
    scaling before and after the shift, the start after the shift is the oracle's (given the same scaled rows) to 1e-9, and the full restart follows the oracle"""
    N, shift = 30, 3
    bt = S.make_batch(S.BACKWARDS, 2, N, seed=N)
    b1 = dict(bt); b1["A"] = bt["A"] * SCALES[:, None]; b1["b"] = bt["b"] * SCALES
    b, xWS = _uploaded(OA, ctx, bt, 0); b.solve(); plain = b.download(); b.close()
    b, xWS = _uploaded(OA, ctx, b1, 0); ref0 = _reference(xWS)
    o0, oo0 = _opts(OA, oracle, 0, max_iter=0); o, oo = _opts(OA, oracle, 0)
    b.solve(); o1 = b.download()
    assert (o1["exitflag"] == 1).all() and (o1["iters"] == plain["iters"]).all()
    for i in range(2):      # before: lambda of the scaled rows = lambda of the unit rows / row length
        assert np.abs(plain["lp"][i] - o1["lp"][i] * SCALES[:, None]).max() < 1e-8 * max(1.0, np.abs(plain["lp"][i]).max())
    b.shift_warm_start(shift); b.solve(o0); o2 = b.download()
    for i in range(2):
        _tight(o2, i, _oracle_from(oracle, b1, i, SC.shifted_problem(N, shift, o1, i, *ref0[i]), oo0, 0), 0, ("scaled rows", i))
    b, xWS = _uploaded(OA, ctx, b1, 0, b)
    b.solve(); o1 = b.download(); b.shift_warm_start(shift); b.solve(o); o3 = b.download(); b.close()
    for i in range(2):
        r = _oracle_from(oracle, b1, i, SC.shifted_problem(N, shift, o1, i, *ref0[i]), oo, 0)
        _parity(o3, i, r, ("scaled rows, restart", i))
        assert r["exitflag"] == 1 and np.abs(r["lp"] - o3["lp"][i]).max() < 1e-6 * max(1.0, np.abs(r["lp"]).max())      # after: the caller's scaling again


def test_an_unconverged_finite_iterate_is_a_legitimate_restart(OA, ctx, oracle):
    """the exit flag of the last solve is not consulted: a first solve cut off after one iteration per attempt (every exit flag 0, the iterate finite) is shifted like any
    other, and the restart follows the oracle started from the shifted download"""
    N, shift, B = 30, 3, 4
    bt = S.make_batch(S.BACKWARDS, B, N, seed=N)
    b, xWS = _uploaded(OA, ctx, bt, 0); ref0 = _reference(xWS)
    cut = OA.default_opts(); cut.max_iter = 1
    o, oo = _opts(OA, oracle, 0)
    b.solve(cut); o1 = b.download()
    assert (o1["exitflag"] == 0).all() and (o1["status"] == 1).all() and all(_finite(o1, i) for i in range(B))
    b.shift_warm_start(shift); b.solve(o); o2 = b.download(); b.close()
    for i in range(B):
        _parity(o2, i, _oracle_from(oracle, bt, i, SC.shifted_problem(N, shift, o1, i, *ref0[i]), oo, 0), ("unconverged", i))


def test_two_launch_schedule_before_and_after_a_shift_is_bit_identical(OA, ctx, monkeypatch):
    """solve, shift, solve with both solves parked after q passes and finished by a second launch: the bits of a single launch (the shift reads the iterate a resumed solve
    left, and the restart is itself parked and resumed)"""
    N, B = 30, 8
    bt = S.make_batch(S.BACKWARDS, B, N, seed=N)
    wo = OA.warm_restart_opts()
    monkeypatch.setenv("OBCA_SLICE_ALWAYS", "1")
    runs = {}
    for q in (0, 6, 1):
        monkeypatch.setenv("OBCA_SLICE_PASSES", str(q))
        b, _ = _uploaded(OA, ctx, bt, 0)
        b.solve(); s1 = b.last_schedule(); a = b.download()
        b.shift_warm_start(3); b.solve(wo); s2 = b.last_schedule(); runs[q] = (a, b.download()); b.close()
        assert s1 == s2 == ((2, q) if q else (1, 0)), (q, s1, s2)
    assert (runs[0][1]["exitflag"] == 1).all()
    for q in (6, 1):
        assert _same_bits(runs[0][0], runs[q][0]) and _same_bits(runs[0][1], runs[q][1]), q


# ---------------------------------------------------------------- a loop with measured states
@pytest.mark.parametrize("dist", [0, 1], ids=["signed_dist", "dist"])
def test_five_steps_with_measured_states_follow_the_oracle(OA, ctx, oracle, dist):
    """N = 30, shift 2, x0_new = the predicted state +- (0.02, -0.02, 0.01, 0): every step against the oracle started from the shifted problem of the device's previous
    download with the same x0_new; stage 0 of the result is x0_new exactly; after five shifts the record's reference is the uploaded one advanced by 10 (the objective of a
    sixth call at max_iter = 0 carries it)"""
    N, shift, B, steps = 30, 2, 4, 5
    bt = S.make_batch(S.BACKWARDS, B, N, seed=N)
    b, xWS = _uploaded(OA, ctx, bt, dist); ref = _reference(xWS)
    o, oo = _opts(OA, oracle, 0); o0, oo0 = _opts(OA, oracle, 0, max_iter=0)
    ks = np.minimum(np.arange(N + 1) + shift, N)
    b.solve(); prev = b.download()
    for step in range(steps):
        x0n = prev["xp"][:, :, shift] + (1 if step % 2 == 0 else -1) * np.array([0.02, -0.02, 0.01, 0.0])
        b.shift_warm_start(shift, x0n); b.solve(o); cur = b.download()
        for i in range(B):
            r = _oracle_from(oracle, bt, i, SC.shifted_problem(N, shift, prev, i, *ref[i], x0n[i]), oo, dist)
            _parity(cur, i, r, ("loop", dist, step, i))
            assert r["exitflag"] == 1 and np.array_equal(cur["xp"][i][:, 0], x0n[i]), (dist, step, i)
        ref = [tuple(a[ks] for a in ref[i]) for i in range(B)]; prev = cur
    b.shift_warm_start(0); b.solve(o0); last = b.download(); b.close()
    k10 = np.minimum(np.arange(N + 1) + steps * shift, N); k8 = np.minimum(np.arange(N + 1) + (steps - 1) * shift, N)
    for i in range(B):
        up10 = tuple(xWS[i, k10, c] for c in range(3))
        assert all(np.array_equal(a, c) for a, c in zip(ref[i], up10))
        r = _oracle_from(oracle, bt, i, SC.shifted_problem(N, 0, prev, i, *up10), oo0, dist)
        _tight(last, i, r, dist, ("loop, sixth call", dist, i))
        wrong = _oracle_from(oracle, bt, i, SC.shifted_problem(N, 0, prev, i, *(xWS[i, k8, c] for c in range(3))), oo0, dist)
        assert abs(wrong["obj"] - r["obj"]) > 1e-6 * max(1.0, abs(r["obj"])), (dist, i)      # (a reference one shift behind is visible in that objective)


def test_solve_shift_solve_keeps_its_bits(OA, ctx):
    """the same sequence twice, and once more after a foreign pattern was left in the CUs' LDS"""
    from obca_amd import diag
    N, B = 30, 4
    bt = S.make_batch(S.BACKWARDS, B, N, seed=N)
    wo = OA.warm_restart_opts(); x0n = None; outs = []
    b, _ = _uploaded(OA, ctx, bt, 0)
    for rep in range(3):
        if rep:
            _uploaded(OA, ctx, bt, 0, b)
        if rep == 2:
            diag.leave_pattern(ctx, 4, 1e30)
        b.solve(); a = b.download()
        x0n = a["xp"][:, :, 2] + np.array([0.01, 0.0, -0.01, 0.0])
        b.shift_warm_start(2, x0n); b.solve(wo); outs.append((a, b.download()))
    b.close()
    assert (outs[0][1]["exitflag"] == 1).all()
    for rep in (1, 2):
        assert _same_bits(outs[0][0], outs[rep][0]) and _same_bits(outs[0][1], outs[rep][1]), rep


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_batch_usable(OA, ctx):
    N, B = 30, 2
    bt = S.make_batch(S.BACKWARDS, B, N, seed=N)
    wo = OA.warm_restart_opts()
    fresh = OA.Batch(ctx, B, N)
    with pytest.raises(OA.ObcaError, match="nothing uploaded"):
        fresh.shift_warm_start(1)
    fresh.close()
    b, _ = _uploaded(OA, ctx, bt, 0)
    b.solve(); o1 = b.download(); b.shift_warm_start(1); b.solve(wo); clean = b.download()      # the sequence no refusal disturbs
    _uploaded(OA, ctx, bt, 0, b)
    with pytest.raises(OA.ObcaError, match="nothing has been solved since the last upload or shift"):
        b.shift_warm_start(1)                                    # before a solve
    b.solve(); v0 = b.validate()
    with pytest.raises(OA.ObcaError, match="out of range"):
        b.shift_warm_start(N + 1)
    with pytest.raises(OA.ObcaError, match="out of range"):
        b.shift_warm_start(-1)
    for bad in (np.nan, np.inf, -np.inf):
        x0n = o1["xp"][:, :, 1].copy(); x0n[1, 2] = bad
        with pytest.raises(OA.ObcaError, match="non-finite entry in x0_new"):
            b.shift_warm_start(1, x0n)
    v1 = b.validate()
    assert np.array_equal(v0["ok"], v1["ok"]) and np.array_equal(v0["viol"], v1["viol"], equal_nan=True) and _same_bits(b.download(), o1)      # none of the refused calls touched the batch
    b.shift_warm_start(1)
    with pytest.raises(OA.ObcaError, match="nothing has been solved since the last upload or shift"):
        b.shift_warm_start(1)                                    # a second shift without a solve: the reference would advance twice, the iterate once
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.validate()
    b.solve(wo); o2 = b.download(); b.close()
    assert (o2["exitflag"] == 1).all() and _same_bits(o2, clean) and np.array_equal(o2["xp"][:, :, 0], o1["xp"][:, :, 1])
