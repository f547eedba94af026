"""Device-side feasibility checks on the GPU (run with -m gpu): Batch.validate / QuadBatch.validate on resident solutions and the host-pointer entries
parking_constraints_batch / quadcopter_constr_satisfaction_batch, against the numpy checkers of obca_amd/validate.py on the downloaded solutions.
Comparison rules and the derivation of the bound (1e-9 * max(1, max|lambda|, max|mu|); flags outside tol +- that bound, at most one instance of a batch inside it):
tests/validate_compare.py."""
import time
import numpy as np
import pytest
import validate_compare as K
from obca_amd import scenarios as S, validate as V

pytestmark = pytest.mark.gpu
PEN, SEP, REFW = V.VIOL_NAMES.index("penetration"), V.VIOL_NAMES.index("sep"), V.VIOL_NAMES.index("ref_worst")


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


def _obst(bt, i):
    return (bt["vOb"][i], bt["A"][i], bt["b"][i]) if isinstance(bt["vOb"], list) else (bt["vOb"], bt["A"], bt["b"])


def _solve_resident(OA, ctx, bt, N, fixTime=0, dist=False):
    B = len(bt["x0"])
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], fixTime, xWS, bt["uWS"], dist=dist)
    b.solve(opts=OA.ipopt_opts())
    return b


def _host_entry(OA, bt, N, out, fixTime=0, dist=False, device=0, **kw):
    a = dict(x=out["xp"], u=out["up"], timeScale=out["timeScale"], l=out["lp"], n=out["np"], sl=None if dist else out["sl"]); a.update(kw)
    return OA.parking_constraints_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], a["x"], a["u"], a["timeScale"],
                                        a["l"], a["n"], a["sl"], fixTime=fixTime, dist=dist, device=device)


def _check_parking(OA, ctx, bt, N, what, fixTime=0, dist=False):
    """solve, validate on the device, download, compare instance by instance with numpy; then the downloaded solution through the host-pointer entry"""
    B = len(bt["x0"])
    b = _solve_resident(OA, ctx, bt, N, fixTime, dist)
    res = b.validate(); out = b.download(); b.close()
    assert res["viol"].shape == (B, 14) and res["names"] == V.VIOL_NAMES and res["ok"].dtype == bool
    host = _host_entry(OA, bt, N, out, fixTime, dist)
    band, hband = K.Band(), K.Band()
    n_np = n_dev = 0; refs = []
    for i in range(B):
        vOb, A, bb = _obst(bt, i)
        ok, rok, vec = K.numpy_parking(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], vOb, A, bb, out["xp"][i], out["up"][i], out["timeScale"][i],
                                       out["lp"][i], out["np"][i], out["sl"][i], fixTime=fixTime, dist=dist)
        bnd = K.bound(out["lp"][i], out["np"][i]); w = "%s[%d]" % (what, i)
        K.check_classes(res["viol"][i], vec, bnd, V.VIOL_NAMES, w)
        finite = all(np.isfinite(out[k][i]).all() for k in ("xp", "up", "timeScale", "lp", "np", "sl"))
        eok, erok = K.parking_flags_expected(vec, finite, 5e-5, bnd)
        band.check(res["ok"][i], eok, w + " ok"); band.check(res["ref_ok"][i], erok, w + " ref_ok")
        if eok is not None:
            n_np += int(ok and finite); n_dev += int(res["ok"][i])
        # the downloaded solution through the host-pointer entry: lambda went through the caller's row scaling and back
        assert np.all((np.abs(host["viol"][i] - res["viol"][i]) <= bnd) | (~np.isfinite(host["viol"][i]) & ~np.isfinite(res["viol"][i]))), (w, host["viol"][i], res["viol"][i])
        hband.check(host["ok"][i], eok, w + " host ok"); hband.check(host["ref_ok"][i], erok, w + " host ref_ok")
        refs.append((vec, bnd, erok))
    assert n_dev == n_np, (what, n_dev, n_np)
    return out, res, refs


def test_config2_bench_batch_validate_matches_numpy_and_costs_less_than_the_solve(OA, ctx):
    """The config-2 bench batch (1 024 instances, N = 80), reference options: every class and both flags against numpy; ok.sum() equals numpy's count; the host-pointer
    entry on the downloaded solution agrees with the resident call; a multi-device context with device 0 listed twice returns the same bits; and the whole validate() call,
    result download included, takes less than the interior-point kernel of the same solve (expected: far less -- 18 MB read once against 15.6 GB per solve launch)."""
    N, B = 80, 1024
    bt = S.make_batch(S.BACKWARDS, B, N)
    out, res, _ = _check_parking(OA, ctx, bt, N, "config 2")
    print("config 2: %d of %d solved, %d pass the full check at 5e-5, %d the reference's" % ((out["exitflag"] == 1).sum(), B, res["ok"].sum(), res["ref_ok"].sum()))
    # cost: minimum over 5 repeats of the validate() wall time against the IPM kernel time of the same batch's solve in the same process
    b = _solve_resident(OA, ctx, bt, N)
    b.sync(); ipm_ms = b.kernel_ms()[0]
    b.validate()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter(); r = b.validate(); walls.append((time.perf_counter() - t0) * 1e3)
    kern_ms = b.validate_ms(); b.close()
    print("config 2, B = %d: validate() wall min %.3f ms of %s, validate kernel %.3f ms, ipm kernel %.3f ms" % (B, min(walls), ["%.3f" % w for w in walls], kern_ms, ipm_ms))
    assert np.array_equal(r["viol"], res["viol"]) and np.array_equal(r["ok"], res["ok"])
    assert min(walls) < ipm_ms, (walls, ipm_ms)
    # several chunks over the lanes of one device / of a context that lists device 0 twice: the same bits
    one = _host_entry(OA, bt, N, out)
    mc = OA.Context(devices=[0, 0])
    two = _host_entry(OA, bt, N, out, device=mc); mc.close()
    for k in ("ok", "ref_ok", "viol"):
        assert np.array_equal(one[k], two[k]), k


@pytest.mark.parametrize("case", ["dist", "fixTime", "ragged", "N33", "N128"])
def test_small_batches_validate_matches_numpy(OA, ctx, case):
    N = {"N33": 33, "N128": 128}.get(case, 80)
    if case == "ragged":      # config-5 style: 1..10 obstacles, polygons of 3..8 rows beside the scenario's 1- and 2-row obstacles: all three row classes of the block code
        bt = S.make_mixed_batch(48, N, min_obstacles=1, rows=(3, 8), max_rows=64)
        nob = [len(v) for v in bt["vOb"]]; rows = np.concatenate(bt["vOb"])
        assert min(nob) <= 2 and max(nob) >= 8 and rows.min() <= 2 and ((rows > 2) & (rows <= 4)).any() and (rows >= 5).any()
    else:
        bt = S.make_batch(S.BACKWARDS, 32, N)
    out, res, _ = _check_parking(OA, ctx, bt, N, case, fixTime=int(case == "fixTime"), dist=(case == "dist"))
    print("%s: %d of %d solved, %d pass the full check at 5e-5, %d the reference's" % (case, (out["exitflag"] >= 1).sum(), len(out["exitflag"]), res["ok"].sum(), res["ref_ok"].sum()))


def test_corridor_solutions_with_positive_slack(OA, ctx, oracle):
    """Wedges that intrude into the warm start's body: some solutions keep a positive slack.  There the penetration class is positive, `ok` follows the separation rows WITH the
    slack, and the reference's test -- which evaluates the last obstacle's row without it -- fails where that obstacle is the penetrated one."""
    N, B = 80, 64
    bt = S.make_corridor_batch(B, N, seed=11, clearance=(-0.15, 0.2))
    out, res, refs = _check_parking(OA, ctx, bt, N, "corridor")
    solved = out["exitflag"] >= 1
    slack = np.array([out["sl"][i].max() for i in range(B)]); last = np.array([out["sl"][i][-1].max() for i in range(B)])
    pos = solved & (slack > 1e-3)
    print("corridor: %d solved, %d with slack > 1e-3 (%d on the last obstacle), ok %d, ref_ok %d" % (solved.sum(), pos.sum(), (pos & (last > 1e-3)).sum(), res["ok"].sum(), res["ref_ok"].sum()))
    assert pos.any()
    assert (res["viol"][pos, PEN] > 0).all()
    assert (res["viol"][pos, PEN] >= slack[pos] - 1e-4).all()                 # the slack absorbs what the row lacks
    assert (res["viol"][pos, SEP] <= 5e-5).all()                              # ... so the row holds WITH it
    assert not res["ref_ok"][pos & (last > 1e-3)].any()                       # the reference ignores the slack (ParkingConstraints.jl:127-128)
    for i in range(B):
        vec, bnd, erok = refs[i]
        if erok is None or not solved[i]:
            continue
        vOb, A, bb = _obst(bt, i)
        args = (bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], len(vOb), vOb, A, bb, out["xp"][i], out["up"][i], out["lp"][i], out["np"][i], out["timeScale"][i], 0, 1)
        assert int(res["ref_ok"][i]) == V.parking_constraints_ref(*args), i
        # the C restatement in the oracle uses the solver's bounded-range sin / cos: compared where the deciding value is clear of the threshold by 1e-9
        if abs(vec[REFW] - 5e-5) > 1e-9:
            assert int(res["ref_ok"][i]) == oracle.ref_constraints(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], vOb, A, bb, out["xp"][i], out["up"][i],
                                                                   float(out["timeScale"][i][0]), out["lp"][i], out["np"][i], 0, 1), i


@pytest.mark.parametrize("dist", [0, 1])
def test_quadcopter_config4_validate_matches_numpy(OA, ctx, dist):
    N, B = 60, 64
    q = S.make_quad_batch(B, N, random_endpoints=True)
    b = OA.QuadBatch(ctx, B, N)
    b.upload(q["x0"], q["xF"], q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"], dual_ws=True, dist=bool(dist))
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.validate()
    b.solve(opts=OA.quadcopter_ipopt_opts())
    res = b.validate(); out = b.download(); ms = b.validate_ms(); b.close()
    assert res["viol"].shape == (B, 9) and res["names"] == V.QUAD_VIOL_NAMES and ms > 0
    host = OA.quadcopter_constr_satisfaction_batch(out["xp"], out["up"], out["timeScale"], q["x0"], q["xF"], q["Ts"], out["lp"], q["ob"], q["R"])
    band = K.Band(); n_np = n_dev = 0
    for i in range(B):
        ok, vec = K.numpy_quad(out["xp"][i], out["up"][i], out["timeScale"][i], q["x0"][i], q["xF"][i], q["Ts"], out["lp"][i], q["ob"], q["R"])
        bnd = K.bound(out["lp"][i]); w = "quad dist=%d [%d]" % (dist, i)
        K.check_classes(res["viol"][i], vec, bnd, V.QUAD_VIOL_NAMES, w)
        finite = all(np.isfinite(out[k][i]).all() for k in ("xp", "up", "timeScale", "lp"))
        e = K.quad_flag_expected(vec, finite, 1e-3, bnd)
        band.check(res["ok"][i], e, w)
        if e is not None:
            n_np += int(ok and finite); n_dev += int(res["ok"][i])
        assert np.array_equal(host["viol"][i], res["viol"][i]) and host["ok"][i] == res["ok"][i], w      # the same numbers in, the same kernel text: the same bits
    assert n_dev == n_np
    print("quadcopter dist=%d: %d of %d solved, %d pass constrSatisfaction at 1e-3; validate kernel %.3f ms" % (dist, (out["exitflag"] >= 1).sum(), B, n_dev, ms))
    # an input beyond its bound, a NaN
    up = out["up"].copy(); up[3, 0, 5] = 8.0
    xp = out["xp"].copy(); xp[5, 0, 7] = np.nan
    bad = OA.quadcopter_constr_satisfaction_batch(xp, up, out["timeScale"], q["x0"], q["xF"], q["Ts"], out["lp"], q["ob"], q["R"])
    assert not bad["ok"][3] and bad["viol"][3, 2] > 0.19 and not bad["ok"][5] and np.isnan(bad["viol"][5, 3])
    keep = np.ones(B, bool); keep[[3, 5]] = False
    assert np.array_equal(bad["viol"][keep], res["viol"][keep]) and np.array_equal(bad["ok"][keep], res["ok"][keep])


def test_error_cases(OA, ctx):
    N, B = 40, 16
    bt = S.make_batch(S.BACKWARDS, B, N, seed=3)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b.validate()
    with pytest.raises(OA.ObcaError):
        b.validate_ms()
    b.solve(opts=OA.ipopt_opts())
    res = b.validate(); out = b.download()
    assert res["ok"].shape == (B,) and b.validate_ms() > 0
    b.shift_warm_start(1)
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):      # the problem has moved on: the old solution is not the answer to it
        b.validate()
    b.solve(opts=OA.warm_restart_opts())
    assert b.validate()["ok"].shape == (B,)
    b.close()
    # infeasible and NaN-carrying trajectories through the host-pointer entry
    good = _host_entry(OA, bt, N, out)
    assert np.array_equal(good["ok"], res["ok"])
    xp = out["xp"].copy(); xp[2, 0, N // 2] += 0.01; xp[4, 1, 9] = np.nan
    up = out["up"].copy(); up[6, 0, 3] = 0.7
    lp = np.array(out["lp"]); lp[8, 0, 5] = -0.1
    sl = np.array(out["sl"]); sl[10, 1, 3] = np.inf; sl[12, 1, 3] = np.nan
    bad = _host_entry(OA, bt, N, out, x=xp, u=up, l=lp, sl=sl)
    for i in (2, 4, 6, 8, 10, 12):
        assert not bad["ok"][i], i
    for i in (4, 6, 8, 10, 12):      # (the reference's test does not look at the slack: a non-finite entry there clears its flag all the same)
        assert not bad["ref_ok"][i], i
    assert bad["viol"][2, V.VIOL_NAMES.index("dyn")] > 1e-3 and np.isnan(bad["viol"][4, V.VIOL_NAMES.index("x_bounds")]) and abs(bad["viol"][8, V.VIOL_NAMES.index("dual_pos")] - 0.1) < 1e-12
    assert np.isnan(bad["viol"][12, SEP]) and bad["viol"][10, SEP] == 0.0      # DMIN - (row + inf) = -inf is no violation; the flags fall all the same
    keep = np.ones(B, bool); keep[[2, 4, 6, 8, 10, 12]] = False
    assert np.array_equal(bad["viol"][keep], good["viol"][keep]) and np.array_equal(bad["ok"][keep], good["ok"][keep])
    # a timeScale that varies over the stages: ts_chain and dyn see it
    ts = out["timeScale"] * (1 + 0.01 * np.sin(np.arange(N + 1)))[None, :]
    var = _host_entry(OA, bt, N, out, timeScale=ts)
    for i in range(0, B, 5):
        _, _, vec = K.numpy_parking(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], out["xp"][i], out["up"][i], ts[i],
                                    out["lp"][i], out["np"][i], out["sl"][i])
        K.check_classes(var["viol"][i], vec, K.bound(out["lp"][i], out["np"][i]), V.VIOL_NAMES, "varying timeScale [%d]" % i)
    assert not var["ok"].any()
    with pytest.raises(OA.ObcaError):
        OA.parking_constraints_batch(bt["x0"], bt["xF"], N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], out["xp"][:, :, :N], out["up"], 1.0, out["lp"], out["np"])
    # the single-instance drop-ins
    assert OA.ParkingConstraints(bt["x0"][0], bt["xF"][0], N, bt["Ts"][0], bt["L"], bt["ego"], bt["XYbounds"], 3, bt["vOb"], bt["A"], bt["b"], out["xp"][0], out["up"][0], out["lp"][0],
                                 out["np"][0], out["timeScale"][0], 0, 1) == int(res["ref_ok"][0])
