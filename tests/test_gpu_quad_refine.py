"""Refinement of solved quadcopter batches onto a finer horizon on the device (include/obca_quad_subdivide.h): the host-pointer call against the host build of the same kernel
text (tests/emu/quad_subdivide_emu.cpp); the promise that the refined nodes are the points clearance(substeps = r) looked at; the resident call -- through the solve that
follows it -- against the host-pointer solve and the CPU oracle started from the host build's refinement of the device's own coarse solution (the quadcopter optimum has flat
directions, tests/test_gpu_quad_restart.py: a checker started from its own coarse solution would start somewhere else); the margin; selections and statuses; the refusals.
Trajectories, comparison rules and the tolerance: tests/quad_refine_common.py.  The largest differences seen are printed by the last test."""
import numpy as np
import pytest
import packing as P
import quad_refine_common as R
from obca_amd import scenarios as S, validate as V

pytestmark = pytest.mark.gpu
KEYS = ("xp", "up", "timeScale", "lp", "slack", "info", "exitflag")


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.build_library()
    return obca_amd


@pytest.fixture(scope="module")
def Q():
    import oracle_quad
    oracle_quad.lib()
    return oracle_quad


def _batch(OA, ctx, bt, B=None, N=None):
    qb = OA.QuadBatch(ctx, B or len(bt["x0"]), N or bt["N"])
    qb.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    return qb


def _same_bits(a, b, ia=slice(None), ib=slice(None)):
    return all(np.array_equal(a[k][ia], b[k][ib], equal_nan=True) for k in KEYS)


def _records(bt, o, sel, r, margin):
    """the destination records the host build writes from the download `o` of the source for the selection: [(status, record)]"""
    return [R.refined_record(bt, i, o["xp"][i], o["timeScale"][i, 0], o["info"][i], r, margin) for i in sel]


def _host_pointer_solve(OA, bt, recs, Nf, opts=None):
    """the fine problems of the records through the host-pointer solve: the same kernels on the same bits as a resident batch that holds these records"""
    p = [R.refined_problem(pd, Nf) for _, pd in recs]
    assert len({q["R"] for q in p}) == 1 and len({q["dual_ws"] for q in p}) == 1
    return OA.quadcopter_signed_dist_batch(np.stack([q["x0"] for q in p]), np.stack([q["xF"] for q in p]), Nf, np.array([q["Ts"] for q in p]), p[0]["R"], bt["ob"],
                                           np.stack([q["xWS"] for q in p]), np.array([q["timeWS"] for q in p]), dual_ws=bool(p[0]["dual_ws"]), opts=opts)


# ---------------------------------------------------------------- 1. host-pointer call against the host build
def _arrays(N, B=6):
    cs = R.cases(N, B)
    return cs, np.stack([c["x"] for c in cs]), np.stack([c["ts"] for c in cs])


@pytest.mark.parametrize("N,r", R.SHAPES)
def test_host_pointer_call_matches_the_host_build(OA, N, r):
    cs, x, ts = _arrays(N)
    for t in (ts, None):
        out = OA.quadcopter_refine_batch(x, t, cs[0]["Ts"], r)
        Tsf, xf = R.emu_host_batch(x, t, cs[0]["Ts"], r)
        assert out["x"].shape == (6, 12, N * r + 1) and np.array_equal(out["Ts"], Tsf) and (Tsf == cs[0]["Ts"] / r).all()
        d = R.note("device against host build", out["x"], xf)
        assert d <= R.TOL and np.array_equal(out["x"], xf), (N, r, d)
        assert np.array_equal(out["x"][:, :, ::r], x)
        R.note("device against numpy", out["x"][3], V.refine_quad(x[3], 1.0 if t is None else t[3], cs[0]["Ts"], r)["x"])
    assert R.WORST["device against numpy"] <= R.TOL


def test_host_pointer_call_marks_a_non_finite_instance_and_no_other(OA):
    N, r = 7, 4; cs, x, ts = _arrays(N); Ts = np.full(6, cs[0]["Ts"])
    whole = OA.quadcopter_refine_batch(x, ts, Ts, r)
    xb = x.copy(); tb = ts.copy(); Tb = Ts.copy()
    xb[1, 7, 3] = np.nan; tb[3, N] = np.inf; Tb[5] = np.nan
    bad = OA.quadcopter_refine_batch(xb, tb, Tb, r)
    for i in range(6):
        if i in (1, 3, 5):
            assert np.isnan(bad["Ts"][i]) and np.isnan(bad["x"][i]).all(), i
        else:
            assert bad["Ts"][i] == whole["Ts"][i] and np.array_equal(bad["x"][i], whole["x"][i]), i
    for rbad, msg in ((0, "factor"), (33, "factor"), (19, "NMAX")):      # 19 x 7 > 128
        with pytest.raises(OA.ObcaError, match=msg):
            OA.quadcopter_refine_batch(x, ts, Ts, rbad)


# ---------------------------------------------------------------- 2. the promise on the device
@pytest.mark.parametrize("N,r", [(7, 4), (60, 2)])
def test_refined_nodes_are_the_points_clearance_sampled(OA, N, r):
    cs, x, ts = _arrays(N); Ts, ob, Rr = cs[0]["Ts"], cs[0]["ob"], cs[0]["R"]
    xf = OA.quadcopter_refine_batch(x, ts, Ts, r)["x"]
    for need in (0.0, 0.4):
        a = OA.quadcopter_clearance_batch(x, ts, Ts, ob, Rr, substeps=r, need=need)
        b = OA.quadcopter_clearance_batch(xf, None, Ts / r, ob, Rr, substeps=1, need=need)
        for k in ("min", "sample", "obstacle", "below", "per_obstacle", "samples"):
            assert np.array_equal(a[k], b[k]), (N, r, need, k, a[k], b[k])
        assert a["finite"].all() and b["finite"].all() and (need == 0.0 or a["below"].sum() > 0)


# ---------------------------------------------------------------- 3. the resident pipeline
@pytest.fixture(scope="module")
def coarse(OA):
    """make_quad_batch(16, 20) solved on the device, once: (batch dict, context, source batch, its download, its clearance at 8 samples per interval)"""
    bt = S.make_quad_batch(16, 20); ctx = OA.Context(0)
    src = _batch(OA, ctx, bt); src.solve(); o1 = src.download(); c1 = src.clearance(8)
    assert (o1["exitflag"] == 1).all(), o1["exitflag"]
    yield bt, ctx, src, o1, c1
    src.close(); ctx.close()


def _against_the_oracle(Q, bt, recs, Nf, o2, label):
    """the rules of tests/test_gpu_quad_restart.py::test_restart_parity_through_the_c_abi: exit flags equal, objective 1e-8 relative, t 1e-8, inputs 1e-4, states 1e-3,
    iteration or regularisation counts differing on at most one instance.  Returns the oracle's exit flags."""
    flips = []; efs = []
    for j, (st, pd) in enumerate(recs):
        p = R.refined_problem(pd, Nf)
        q = Q.quadcopter_signed_dist(p["x0"], p["xF"], Nf, p["Ts"], p["R"], bt["ob"], p["xWS"], p["timeWS"], dual_ws=p["dual_ws"])
        efs.append(q["exitflag"])
        assert q["exitflag"] == o2["exitflag"][j], (label, j, q["exitflag"], o2["exitflag"][j])
        if q["exitflag"] == 1:
            assert abs(o2["obj"][j] - q["obj"]) < 1e-8 * abs(q["obj"]), (label, j, o2["obj"][j], q["obj"])
            assert abs(o2["timeScale"][j, 0] - q["t"]) < 1e-8 and np.abs(o2["up"][j] - q["up"]).max() < 1e-4, (label, j)
            assert R.note(label + ": states against the oracle from the same start", o2["xp"][j], q["xp"]) < 1e-3, (label, j)
            if o2["iters"][j] != q["iters"] or o2["info"][j, 6] != q["nreg"]:
                flips.append((j, int(o2["iters"][j]), q["iters"]))
    print("%s: device iterations %s, exit flags %s; counts that differ from the oracle's: %s" % (label, o2["iters"].tolist(), o2["exitflag"].tolist(), flips))
    assert len(flips) <= 1, flips
    return np.array(efs)


def test_resident_pipeline_solve_clearance_refine_solve_validate_clearance(OA, Q, coarse):
    bt, ctx, src, o1, c1 = coarse; N, r = 20, 2; Nf = N * r
    dst = OA.QuadBatch(ctx, 16, Nf)
    d, st = src.refine(r, into=dst)
    assert d is dst and d.B == 16 and (st == 0).all() and d.refine_ms() > 0
    recs = _records(bt, o1, range(16), r, 0.0)
    assert all(s == 0 for s, _ in recs)
    # the start the destination holds: a solve capped at no iteration returns the starting point (the warm start with x0 at stage 0, pushed off its bounds) -- against the
    # oracle's from the host build's record of the same instance, relative to max(1, |oracle|) to 1e-8: the bar of test_starting_point_after_the_shift_at_loop_edges
    zero = OA.quadcopter_default_opts(); zero.max_iter = 0; oo = Q.default_opts(); oo.max_iter = 0
    d.solve(opts=zero); s0 = d.download()
    assert (s0["iters"] == 0).all()
    for j, (_, pd) in enumerate(recs):
        p = R.refined_problem(pd, Nf)
        q = Q.quadcopter_signed_dist(p["x0"], p["xF"], Nf, p["Ts"], p["R"], bt["ob"], p["xWS"], p["timeWS"], opts=oo, dual_ws=p["dual_ws"])
        assert q["iters"] == 0 and np.array_equal(s0["xp"][j][:, 0], p["x0"])
        assert p["timeWS"] == o1["timeScale"][j, 0] and abs(s0["timeScale"][j, 0] - q["t"]) < 1e-8      # (t starts pushed off its lower bound)
        for k in ("xp", "up", "lp", "slack"):
            assert R.note("resident start against the oracle's from the host build's record (relative)", s0[k][j] / max(1.0, np.abs(q[k]).max()), q[k] / max(1.0, np.abs(q[k]).max())) < 1e-8, (j, k)
    d.solve(); o2 = d.download(); v = d.validate(); c2 = d.clearance(4)
    # the same kernels on the same bits: the host-pointer solve of the host build's records
    h = _host_pointer_solve(OA, bt, recs, Nf)
    assert _same_bits(o2, h)
    _against_the_oracle(Q, bt, recs, Nf, o2, "refine x 2")
    ok = o2["exitflag"] == 1
    assert ok.any() and v["ok"][ok].all(), (o2["exitflag"], v["viol"])
    print("below %d -> %d, worst min %.6g -> %.6g (the oracle: 247 -> 66, -0.240 -> -0.076)" % (c1["below"].sum(), c2["below"].sum(), c1["min"].min(), c2["min"].min()))
    assert (c1["samples"] == 8 * N + 1).all() and (c2["samples"] == 4 * Nf + 1).all()
    assert c2["below"].sum() < c1["below"].sum() and c2["min"].min() > c1["min"].min()
    assert all(np.array_equal(o1[k], src.download()[k], equal_nan=True) for k in ("xp", "info"))      # the source is untouched
    dst.close()


# ---------------------------------------------------------------- 4. margin
def test_margin_closes_the_cut_against_the_true_radius(OA, Q, coarse):
    bt, ctx, src, o1, c1 = coarse; N, r, margin = 20, 4, 0.02; Nf = N * r
    d, st = src.refine(r, margin=margin)
    assert d.N == Nf and d.B == 16 and (st == 0).all()
    d.solve(); o2 = d.download(); c2 = d.clearance(2, need=-margin); v = d.validate()
    recs = _records(bt, o1, range(16), r, margin)
    assert all(pd[P.QPH_R] == bt["R"] + margin for _, pd in recs)
    efs = np.array([Q.quadcopter_signed_dist(p["x0"], p["xF"], Nf, p["Ts"], p["R"], bt["ob"], p["xWS"], p["timeWS"], dual_ws=p["dual_ws"])["exitflag"]
                    for p in (R.refined_problem(pd, Nf) for _, pd in recs)])
    both = (o2["exitflag"] == 1) & (efs == 1)
    print("exit flags device %s, oracle %s; below at need = -margin %s; smallest clearance against the true R %.6g (the oracle from its own coarse solutions: 0.0051)"
          % (o2["exitflag"].tolist(), efs.tolist(), c2["below"].tolist(), c2["min"][both].min() + margin))
    assert both.sum() >= 15, (o2["exitflag"], efs)      # at most one instance may be left out
    assert (c2["below"][both] == 0).all() and (c2["samples"] == 2 * Nf + 1).all() and v["ok"][both].all()
    assert (c2["min"][both] + margin > 0).all()
    d.close()


# ---------------------------------------------------------------- 5. selection and status
def test_selection_with_a_duplicate_and_a_permutation_on_a_two_lane_context(OA):
    bt = S.make_quad_batch(6, 20); ctx = OA.Context(devices=[0, 0]); N, r = 20, 2
    src = _batch(OA, ctx, bt); src.solve(); o1 = src.download()
    assert (o1["exitflag"] == 1).all()
    full, stf = src.refine(r); full.solve(); of = full.download()
    sel = [4, 0, 5, 5, 2]
    d, st = src.refine(r, select=sel, margin=0.0)
    assert d.B == 5 and (st == 0).all() and (stf == 0).all()
    d.solve(); o2 = d.download()
    assert o2["xp"].shape == (5, 12, r * N + 1) and _same_bits(o2, of, ib=sel)      # in the order of the selection, the duplicate twice
    mask = np.array([True, False, True, False, False, True])
    dm, stm = src.refine(r, select=mask, into=d)
    assert dm is d and d.B == 3
    d.solve(); om = d.download()
    assert _same_bits(om, of, ib=[0, 2, 5])
    for b in (src, full, d):
        b.close()
    ctx.close()


def test_failed_instance_gets_status_1_and_leaves_the_others_alone(OA, coarse):
    bt, ctx, src0, o1, c1 = coarse; N, r = 20, 2; Nf = N * r
    it = o1["iters"]; j = int(np.argmax(it)); others = np.array([i for i in range(16) if i != j])
    assert it[others].max() < it[j], it
    ref, _ = src0.refine(r); ref.solve(); oref = ref.download(); ref.close()
    cap = OA.quadcopter_default_opts(); cap.max_iter = int(it[j]) - 1
    src = _batch(OA, ctx, bt); src.solve(opts=cap); oc = src.download()
    assert oc["exitflag"][j] == 0 and (oc["exitflag"][others] == 1).all()
    d, st = src.refine(r)
    assert st[j] == 1 and (st[others] == 0).all(), st
    d.solve(); o2 = d.download()
    assert _same_bits(o2, oref, others, others)
    # instance j: the uploaded warm start interpolated linearly, timeWS and dual_ws as uploaded -- the host-pointer solve of that problem, bit for bit
    up = V.refine_quad(bt["xWS"][j].T, 1.0, bt["Ts"], r, euler=False)["x"].T
    st_h, pd = R.refined_record(bt, j, oc["xp"][j], oc["timeScale"][j, 0], oc["info"][j], r, 0.0)
    assert st_h == 1 and np.array_equal(pd[P.QPH_SIZE:], up.reshape(-1)) and pd[P.QPH_TWS] == bt["timeWS"]
    h = _host_pointer_solve(OA, bt, [(st_h, pd)], Nf)
    assert _same_bits(o2, h, [j], [0])
    # every instance failed after three iterations, as in the restart test: every status is 1
    cap.max_iter = 3
    src.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"]); src.solve(opts=cap)
    assert (src.download()["exitflag"] == 0).all()
    d3, st3 = src.refine(r, into=d)
    assert (st3 == 1).all()
    for b in (src, d):
        b.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_both_batches_usable(OA):
    bt = S.make_quad_batch(4, 20); ctx = OA.Context(0); other = OA.Context(0); N = 20
    src = _batch(OA, ctx, bt); dst = OA.QuadBatch(ctx, 3, 2 * N); far = OA.QuadBatch(other, 3, 2 * N)
    lib = OA.api._load(); st = np.zeros(4, np.int32)
    with pytest.raises(OA.ObcaError, match="subdivide"):      # before any call
        dst.refine_ms()
    with pytest.raises(OA.ObcaError, match="solved"):         # unsolved source
        src.refine(2, select=[0], into=dst)
    src.solve(); o1 = src.download()
    src.shift_warm_start(1)
    with pytest.raises(OA.ObcaError, match="solved"):         # ... and not solved since its shift
        src.refine(2, select=[0], into=dst)
    src.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"]); src.solve()
    for kw, msg in ((dict(factor=3, select=[0], into=dst), "horizon"), (dict(factor=0, select=[0], into=dst), "factor"), (dict(factor=33, select=[0], into=dst), "factor"),
                    (dict(factor=0, select=[0]), "factor"), (dict(factor=33, select=[0]), "factor"), (dict(factor=7, select=[0], into=dst), "NMAX"),      # 7 x 20 > 128
                    (dict(factor=2, select=[0, 1, 2, 3], into=dst), "more instances"), (dict(factor=2, select=[0, 4], into=dst), "index"), (dict(factor=2, select=[-1], into=dst), "index"),
                    (dict(factor=1, select=[0], into=src), "two batches"), (dict(factor=2, select=[0], into=far), "two batches"),
                    (dict(factor=2, select=[0], margin=-0.01, into=dst), "margin"), (dict(factor=2, select=[0], margin=np.nan, into=dst), "margin"),
                    (dict(factor=2, select=[0], margin=np.inf, into=dst), "margin"), (dict(factor=2, select=np.zeros(4, bool), into=dst), "empty")):
        with pytest.raises(OA.ObcaError, match=msg):
            src.refine(**kw)
    # what the Python layer catches first, asked of the library itself: NULL arguments, n < 1, an index outside the source
    sel = np.array([0, 9], np.int32)
    for args in ((dst._h, src._h, 2, 0.0, None, 1, None), (None, src._h, 2, 0.0, None, 1, st), (dst._h, None, 2, 0.0, None, 1, st), (dst._h, src._h, 2, 0.0, None, 0, st),
                 (dst._h, src._h, 2, 0.0, None, -1, st), (dst._h, src._h, 2, 0.0, sel, 2, st)):
        assert lib.obca_quad_batch_subdivide_into(*args) == -1, args[2:6]
    with pytest.raises(OA.ObcaError, match="subdivide"):      # no refusal has run a kernel
        dst.refine_ms()
    assert _same_bits(o1, src.download())
    d, s = src.refine(2, select=[3, 1], into=dst)
    assert d is dst and (s == 0).all() and dst.refine_ms() > 0
    for call in (dst.validate, dst.clearance):      # uploaded, not solved
        with pytest.raises(OA.ObcaError, match="nothing has been solved"):
            call()
    dst.solve(); o2 = dst.download()
    assert (o2["exitflag"] == 1).all() and dst.validate()["ok"].all() and o2["xp"].shape == (2, 12, 2 * N + 1)
    src.solve(); assert _same_bits(o1, src.download())      # both batches solve again
    bt3 = S.make_quad_batch(3, 2 * N)      # the destination takes a plain upload again
    dst.upload(bt3["x0"], bt3["xF"], bt3["Ts"], bt3["R"], bt3["ob"], bt3["xWS"], bt3["timeWS"]); dst.solve()
    assert dst.B == 3 and dst.download()["xp"].shape == (3, 12, 2 * N + 1)
    for b in (src, dst, far):
        b.close()
    ctx.close(); other.close()


# ---------------------------------------------------------------- 7. record
def test_zz_largest_differences_are_on_record():
    print("largest differences: " + ", ".join("%s %.3g" % kv for kv in sorted(R.WORST.items())))
