"""Refinement of solved parking batches onto a finer horizon on the device (include/obca_refine.h): the host-pointer call against the host build of the same kernel text
(tests/emu/refine_emu.cpp), the resident call against the host-pointer call and -- through the solve that follows it -- against the oracle started from the same refined
start, the loop clearance -> refine -> solve -> clearance, the refusals.  Trajectories, comparison rules and the tolerance: tests/refine_common.py.  The largest
differences seen are printed (tools/refine_rate.py writes them to the profile)."""
import json
import os
import numpy as np
import pytest
from conftest import golden
import clearance_common as K
import refine_common as R
from obca_amd import scenarios as S, validate as V

pytestmark = pytest.mark.gpu
TOL_TRAJ = 1e-6      # TOL_X of tests/test_gpu_parity.py: the device and the oracle walk through the same iterates in fp64
WORST = {}
SEL = [11, 0, 5, 5, 3]


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.build_library()
    return obca_amd


def host_call(OA, batch, r, ts=True):
    return OA.parking_refine_batch(batch[0]["N"], [c["Ts"] for c in batch], batch[0]["L"], np.stack([c["x"] for c in batch]), np.stack([c["u"] for c in batch]),
                                   np.stack([c["ts"] for c in batch]) if ts else None, r)


# ---------------------------------------------------------------- 1. host-pointer call against the host build
@pytest.mark.parametrize("N,r", R.SHAPES)
def test_host_pointer_call_matches_the_host_build(OA, N, r):
    for bi, batch in enumerate(K.parking_cases(N, 12)):
        out = host_call(OA, batch, r)
        assert out["x"].shape == (12, 4, N * r + 1) and out["u"].shape == (12, 2, N * r)
        for i, c in enumerate(batch):
            what = "N=%d r=%d batch %d instance %d" % (N, r, bi, i)
            rc, Tsf, xf, uf = R.emu_host(c, r)
            d = float(np.abs(out["x"][i] - xf).max()); WORST["device_vs_host_build"] = max(WORST.get("device_vs_host_build", 0.0), d)
            assert rc == 0 and out["Ts"][i] == Tsf and np.array_equal(out["u"][i], uf), what
            assert R.close_x(out["x"][i], xf), (what, d)
            assert np.array_equal(out["x"][i][:, ::r], c["x"]), what
            ref = V.refine_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], r)
            WORST["device_vs_numpy"] = max(WORST.get("device_vs_numpy", 0.0), float(np.abs(out["x"][i] - ref["x"]).max()))
            assert R.close_x(out["x"][i], ref["x"]), what
    print("largest difference so far, device - host build: %.3g, device - numpy: %.3g" % (WORST["device_vs_host_build"], WORST["device_vs_numpy"]))


def test_host_pointer_call_marks_a_non_finite_instance_and_no_other(OA):
    N, r = 7, 3; batch = K.parking_cases(N, 12)[1]
    whole = host_call(OA, batch, r)
    bad = [dict(c) for c in batch]
    bad[2] = dict(bad[2], x=bad[2]["x"].copy()); bad[2]["x"][1, 3] = np.nan
    bad[5] = dict(bad[5], u=bad[5]["u"].copy()); bad[5]["u"][0, 2] = np.inf
    bad[9] = dict(bad[9], ts=bad[9]["ts"].copy()); bad[9]["ts"][4] = np.nan
    rb = host_call(OA, bad, r)
    for i in range(12):
        if i in (2, 5, 9):
            assert np.isnan(rb["Ts"][i]) and np.isnan(rb["x"][i]).all() and np.isnan(rb["u"][i]).all(), i
        else:
            assert all(np.array_equal(rb[k][i], whole[k][i]) for k in ("Ts", "x", "u")), i
    one = host_call(OA, K.parking_cases(N, 12)[0], r, ts=False)      # (this batch's timeScale is 1)
    assert all(np.array_equal(one[k], host_call(OA, K.parking_cases(N, 12)[0], r)[k]) for k in ("Ts", "x", "u"))
    for rbad in (0, 33, 19):      # 19 x 7 > 128
        with pytest.raises(OA.ObcaError, match="factor"):
            host_call(OA, batch, rbad)


# ---------------------------------------------------------------- 2. / 3. resident against the host-pointer call and the oracle, from the same start
def upload(OA, ctx, bt):
    B, N = len(bt["Ts"]), bt["N"]
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    return b, xWS


def obstacles(bt, i):
    per = isinstance(bt["vOb"], list)
    return tuple(bt[k][i] if per else bt[k] for k in ("vOb", "A", "b"))


@pytest.mark.parametrize("which", ["backwards", "mixed"])
def test_resident_pipeline_matches_the_host_pointer_call_and_the_oracle(OA, oracle, which):
    r = 2
    bt = S.make_batch(S.BACKWARDS, 16, 30) if which == "backwards" else S.make_mixed_batch(12, 20, min_obstacles=1, rows=(3, 8), max_rows=64)
    B, N = len(bt["Ts"]), bt["N"]; Nf = r * N; ctx = OA.Context(0)
    b, xWS = upload(OA, ctx, bt)
    b.solve(); o1 = b.download()
    dst = OA.Batch(ctx, 8, Nf); sel = np.array(SEL)
    # the start the resident call must have written: the host-pointer call on the downloaded solution (the same instance function), the reference by numpy
    pr = OA.parking_refine_batch(N, bt["Ts"][sel], bt["L"], o1["xp"][sel], o1["up"][sel], o1["timeScale"][sel], r)
    assert np.array_equal(pr["Ts"], bt["Ts"][sel] / r) and np.array_equal(pr["x"][:, :, ::r], o1["xp"][sel]) and np.array_equal(pr["u"], np.repeat(o1["up"][sel], r, axis=2))
    k_of = np.minimum(np.arange(Nf + 1) // r, N)
    refs = [V.refine_parking(o1["xp"][i], o1["up"][i], 1.0, bt["Ts"][i], bt["L"], r, ref=xWS[i, :, :3].T)["ref"] for i in sel]
    per = isinstance(bt["vOb"], list)
    sub = [[bt[k][i] for i in sel] if per else bt[k] for k in ("vOb", "A", "b")]
    for duals in (False, True):
        d, st = b.refine(r, select=sel, duals=duals, into=dst)
        assert d is dst and d.B == len(sel) and d.refine_ms() > 0
        assert st.tolist() == [0 if o1["exitflag"][i] == 1 else 1 for i in sel], (st, o1["exitflag"][sel])
        opts = OA.warm_restart_opts() if duals else None
        d.solve(opts); o2 = d.download()
        assert np.array_equal(o2["xp"][2], o2["xp"][3], equal_nan=True) and np.array_equal(o2["info"][2], o2["info"][3], equal_nan=True)      # the duplicate of the selection: the same bits
        assert [a.shape for a in o2["lp"]] == [(int(np.sum(obstacles(bt, i)[0])), Nf + 1) for i in sel]      # packed outputs in selection order
        # the host-pointer solve of the same fine problems from the same start: the same kernels on the same bits (carried multipliers go through the caller's row
        # scaling and back, which is exact for rows of unit length only: the mixed batch is compared with DualMultWS duals)
        if not duals or which == "backwards":
            lw = [o1["lp"][i][:, k_of].T for i in sel] if duals else None; nw = [o1["np"][i][:, k_of].T for i in sel] if duals else None
            xw = np.transpose(pr["x"], (0, 2, 1)); rf = np.stack(refs)
            h = OA.parking_signed_dist_batch(bt["x0"][sel], bt["xF"][sel], Nf, pr["Ts"], bt["L"], bt["ego"], bt["XYbounds"], *sub, rf[:, 0], rf[:, 1], rf[:, 2], 0, xw,
                                             np.transpose(pr["u"], (0, 2, 1)), lw, nw, opts)
            ok = np.flatnonzero(st == 0)
            for k in ("xp", "up", "timeScale", "exitflag", "info"):
                assert np.array_equal(np.asarray(o2[k])[ok], np.asarray(h[k])[ok], equal_nan=True), (which, duals, k)
            for j in ok:
                assert np.array_equal(o2["lp"][j], h["lp"][j]) and np.array_equal(o2["np"][j], h["np"][j]), (which, duals, j)
        # the oracle from that start
        oo = oracle.default_opts()
        if duals:
            oo.mu_init = opts.mu_init; oo.bound_push = opts.bound_push; oo.bound_frac = opts.bound_frac
        for j, i in enumerate(sel):
            if st[j] != 0 or (j == 3):
                continue
            vOb, A, bb = obstacles(bt, i)
            lw, nw = (o1["lp"][i][:, k_of].T, o1["np"][i][:, k_of].T) if duals else (None, None)
            q = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], Nf, pr["Ts"][j], bt["L"], bt["ego"], bt["XYbounds"], vOb, A, bb, refs[j][0], refs[j][1], refs[j][2], 0,
                                           pr["x"][j].T, pr["u"][j].T, lw, nw, opts=oo)
            what = "%s duals %s slot %d (instance %d): device exit flag %d, %d iterations; oracle %d, %d" % (which, duals, j, i, o2["exitflag"][j], o2["iters"][j], q["exitflag"], q["iters"])
            print(what)
            assert o2["exitflag"][j] == q["exitflag"] and o2["iters"][j] == q["iters"], what
            dx = float(max(np.abs(o2["xp"][j] - q["xp"]).max(), np.abs(o2["up"][j] - q["up"]).max())); WORST["pipeline_vs_oracle"] = max(WORST.get("pipeline_vs_oracle", 0.0), dx)
            assert dx < TOL_TRAJ, (what, dx)
            assert np.abs(o2["lp"][j] - q["lp"]).max() < 1e-6 * max(1.0, np.abs(q["lp"]).max()) and np.abs(o2["np"][j] - q["np"]).max() < 1e-6 * max(1.0, np.abs(q["np"]).max()), what
    print("largest trajectory difference, resident pipeline - oracle from the same start: %.3g" % WORST.get("pipeline_vs_oracle", float("nan")))
    # the source is untouched, the destination takes a plain upload again
    o1b = b.download()
    assert all(np.array_equal(o1[k], o1b[k], equal_nan=True) for k in ("xp", "up", "timeScale", "exitflag", "info"))
    b.close(); dst.close(); ctx.close()


# ---------------------------------------------------------------- 4. closing the loop
def record(r, i):
    """row i of a clearance dict, back in the layout of the C record"""
    out = np.zeros(V.CLR_OUT); out[8:] = np.inf
    out[0], out[1], out[2], out[3], out[4], out[5], out[6] = r["min"][i], r["min_nodes"][i], r["sample"][i], r["obstacle"][i], r["below"][i], r["samples"][i], 0.0 if r["finite"][i] else 1.0
    po = r["per_obstacle"][i]; out[8:8 + len(po)] = po
    return out


def test_clearance_refine_solve_clearance_closes_the_gap(OA, oracle):
    B, N = 16, 30; bt = S.make_batch(S.BACKWARDS, B, N); ctx = OA.Context(0)
    b, _ = upload(OA, ctx, bt)
    b.solve(); o1 = b.download()
    c1 = b.clearance(substeps=8)
    select = c1["below"] > 0
    assert select.any() and select[2] and (o1["exitflag"] == 1).all()
    d, st = b.refine(2, select)
    idx = np.flatnonzero(select)
    assert d.B == len(idx) and d.N == 2 * N and (st == 0).all()
    d.solve(); o2 = d.download()
    c2 = d.clearance(substeps=4, need=0.05)
    good = o2["exitflag"] == 1
    print("selected %s: below before %s, after %s; min before %s, after %s; min_nodes after %s; exit flags %s, iterations %s" % (
        idx.tolist(), c1["below"][idx].tolist(), c2["below"].tolist(), np.round(c1["min"][idx], 5).tolist(), np.round(c2["min"], 5).tolist(), np.round(c2["min_nodes"], 5).tolist(),
        o2["exitflag"].tolist(), o2["iters"].tolist()))
    assert good.any() and good[idx.tolist().index(2)]
    assert (c2["below"][good] == 0).all() and (c2["min_nodes"][good] >= 0.05 - 1e-6).all() and (c2["samples"] == 4 * 2 * N + 1).all()
    # the fixture's fine solutions of the same instances (the oracle, DualMultWS duals, default options), under clearance_common's parking rules
    g = golden("refine_cases.npz")
    for j, i in enumerate(idx):
        if i >= len(g["ws_x"]) or not good[j]:
            continue
        c = dict(N=2 * N, Ts=float(g["fTs"][i]), L=bt["L"], ego=bt["ego"], vOb=np.asarray(bt["vOb"], np.int32), A=np.asarray(bt["A"], float), b=np.asarray(bt["b"], float),
                 x=g["ws_x"][i], u=g["ws_u"][i], ts=np.full(2 * N + 1, g["ws_t"][i]))
        table = K.ref_parking_table(c, 4); rec = record(c2, j)
        print("instance %d: device min %.9g, min_nodes %.9g, below %d; fixture min %.9g, min_nodes %.9g, below %d" % (i, rec[0], rec[1], rec[4], g["ws_rec"][i][0], g["ws_rec"][i][1], g["ws_rec"][i][4]))
        print("instance %d: device %d iterations, fixture %d; largest trajectory difference %.3g" % (i, o2["iters"][j], g["ws_iters"][i], np.abs(o2["xp"][j] - g["ws_x"][i]).max()))
        K.check_parking_record(rec, table, 4, 0.05, "instance %d against the fixture's fine solution" % i)
    b.close(); d.close(); ctx.close()


# ---------------------------------------------------------------- 5. refusals, 6. refine_ms
def test_refusals_leave_both_batches_usable(OA):
    B, N = 4, 30; bt = S.make_batch(S.BACKWARDS, B, N); ctx = OA.Context(0)
    b, _ = upload(OA, ctx, bt); dst = OA.Batch(ctx, 3, 2 * N)
    with pytest.raises(OA.ObcaError, match="refine"):      # before any call
        dst.refine_ms()
    with pytest.raises(OA.ObcaError, match="solved"):      # unsolved source
        b.refine(2, into=dst, select=[0])
    b.solve(); o1 = b.download()
    for kw, msg in ((dict(factor=3, select=[0], into=dst), "horizon"), (dict(factor=0, select=[0], into=dst), "factor"), (dict(factor=33, select=[0], into=dst), "factor"),
                    (dict(factor=0, select=[0]), "factor"), (dict(factor=33, select=[0]), "factor"), (dict(factor=5, select=[0]), "NMAX"),      # 5 x 30 > 128
                    (dict(factor=2, select=[0, 1, 2, 3], into=dst), "more instances"), (dict(factor=2, select=[0, 4], into=dst), "index"), (dict(factor=2, select=[-1], into=dst), "index"),
                    (dict(factor=1, select=[0], into=b), "two batches"), (dict(factor=2, select=[0], duals=2, into=dst), "duals"), (dict(factor=2, select=np.zeros(B, bool), into=dst), "empty")):
        with pytest.raises(OA.ObcaError, match=msg):
            b.refine(**kw)
    with pytest.raises(OA.ObcaError, match="refine"):      # no refusal has run a kernel
        dst.refine_ms()
    o1b = b.download()
    assert all(np.array_equal(o1[k], o1b[k]) for k in ("xp", "up", "info"))
    d, st = b.refine(2, select=[3, 1], into=dst)
    assert d is dst and (st == 0).all() and dst.refine_ms() > 0
    for call in (dst.validate, dst.clearance):      # uploaded, not solved
        with pytest.raises(OA.ObcaError, match="nothing has been solved"):
            call()
    dst.solve(); o2 = dst.download()
    assert (o2["exitflag"] == 1).all() and dst.validate()["ok"].shape == (2,) and dst.clearance()["finite"].all()
    # a mask selects like its indices; a new batch is made where none is given; the destination takes a plain upload again
    d2, st2 = b.refine(2, select=np.array([False, True, False, True]))
    assert d2.B == 2 and d2.N == 2 * N and (st2 == 0).all()
    d2.solve(); o3 = d2.download()
    assert np.array_equal(o3["xp"][0], o2["xp"][1]) and np.array_equal(o3["xp"][1], o2["xp"][0]) and np.array_equal(o3["info"][::-1], o2["info"])
    bt3 = S.make_batch(S.BACKWARDS, 3, 2 * N); xw = bt3["xWS"].copy(); xw[:, 0, :] = bt3["x0"]
    dst.upload(bt3["x0"], bt3["xF"], bt3["Ts"], bt3["L"], bt3["ego"], bt3["XYbounds"], bt3["vOb"], bt3["A"], bt3["b"], xw[:, :, 0], xw[:, :, 1], xw[:, :, 2], 0, xw, bt3["uWS"])
    dst.solve()
    assert dst.B == 3 and dst.download()["xp"].shape == (3, 4, 2 * N + 1)
    b.close(); dst.close(); d2.close(); ctx.close()


def test_largest_differences_are_on_record():
    """the figures tools/refine_rate.py copies into profiles/refine_device_vs_host.json (OBCA_REFINE_DIFFS names the file they are left in)"""
    print("device against host build, numpy and the oracle:", WORST)
    path = os.environ.get("OBCA_REFINE_DIFFS")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f)
