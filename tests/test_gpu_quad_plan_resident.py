"""The resident route of the quadcopter's grid planner on the GPU (run with -m gpu): QuadBatch.plan_warm_start / plan_paths / plan_ms / warm_start
(include/obca_quad_plan_resident.h) against the host build of the same kernel text (tests/emu/quad_plan_resident_emu.cpp), against the host-pointer route on the device
(planner.quad_warm_start_many), down to solved batches, with a selection, and against itself.  "The 20" instances and the helpers: tests/quad_plan_resident_common.py.
B = 20, N = 20 unless said; bounded kernels only."""
import numpy as np
import pytest
import packing as PK
import plan3d_common as K
import quad_plan_resident_common as Q
import quad_shift_common as QS
import obca_amd as OA
from obca_amd import scenarios as S, planner as PL

pytestmark = pytest.mark.gpu
N = 20


@pytest.fixture(scope="module")
def ctx():
    c = OA.Context(0)
    yield c
    c.close()


def uploaded(ctx, tile=1, xws=None, tws=None):
    """a QuadBatch holding the 20 (tiled) with the way-point start and timeWS 0.9, or with the given start"""
    x0, xF, ob = Q.the20(); w, t = Q.uploaded_start(N)
    w = w if xws is None else xws; t = t if tws is None else tws
    qb = OA.QuadBatch(ctx, Q.NI * tile, N)
    qb.upload(np.tile(x0, (tile, 1)), np.tile(xF, (tile, 1)), S.quad_sample_time(N), S.QUAD_R, np.tile(ob, (tile, 1, 1)), np.tile(w, (tile, 1, 1)), np.tile(t, tile))
    return qb


@pytest.fixture(scope="module")
def host_pointer_route():
    """planner.quad_warm_start_many on the device with the instances' own boxes: (xWS (20, N+1, 12), ok)"""
    x0, xF, ob = Q.the20()
    return PL.quad_warm_start_many(x0, xF, N, boxes=ob, device=0)


def test_device_equals_the_host_build_bit_for_bit(ctx):
    e = Q.planned(N)
    qb = uploaded(ctx)
    cnt, sw = qb.plan_warm_start()
    assert np.array_equal(cnt, e["counts"]), (cnt, e["counts"])
    assert Q.bits(qb.plan_paths(), e["paths"])
    w, t = qb.warm_start(); ew, et = Q.ws_of(e["prob"], N)
    assert Q.bits(w, ew) and Q.bits(t, np.ascontiguousarray(et))
    # the sweep count depends on the order in which the waves run: only bounded -- at least one where there is a path, except (c), whose end points share a node: the
    # relaxation is skipped there on the device as in the host build (0 sweeps, count 3)
    searched = (cnt >= 3) & (np.arange(Q.NI) != Q.C_)
    assert searched.sum() == 17 and (sw[searched] >= 1).all() and sw.max() < np.prod(K.DIMS) and sw[Q.B_] == 0 and sw[Q.C_] == 0 == e["sweeps"][Q.C_]
    print("kernel %.3f ms for %d plans; sweeps device %s, sequential host build %s" % (qb.plan_ms(), Q.NI, sw.tolist(), e["sweeps"].tolist()))
    qb.close()


def test_resident_route_equals_the_host_pointer_route_on_the_device(ctx, host_pointer_route):
    xws, ok = host_pointer_route
    qb = uploaded(ctx)
    cnt, _ = qb.plan_warm_start()
    w, t = qb.warm_start(); w0, t0 = Q.uploaded_start(N)
    assert np.array_equal(cnt >= 2, ok) and ok.sum() == 18 and not ok[Q.A_] and not ok[Q.B_]
    assert Q.bits(w[ok], xws[ok])
    assert Q.bits(w[~ok], w0[~ok]) and Q.bits(t, t0)      # (a) and (b) return the uploaded start; no timeWS was passed
    qb.close()


def test_down_to_solved_batches(ctx, host_pointer_route):
    xws, ok = host_pointer_route
    a = uploaded(ctx)
    a.plan_warm_start(timeWS=1.0)
    with pytest.raises(OA.ObcaError):
        a.validate()      # planned, not solved
    a.solve()
    w0, t0 = Q.uploaded_start(N)
    b = uploaded(ctx, xws=np.where(ok[:, None, None], xws, w0), tws=np.where(ok, 1.0, t0))
    b.solve()
    oa, ob_ = a.download(), b.download()
    assert sorted(oa) == sorted(ob_)
    for k in oa:
        assert Q.bits(oa[k], ob_[k]), k
    assert a.validate()["ok"].shape == (Q.NI,)
    print("exit flags", oa["exitflag"].tolist(), "iterations", oa["iters"].tolist())
    a.close(); b.close()


def test_replanning_a_selection_of_a_solved_batch(ctx, host_pointer_route):
    xws, ok = host_pointer_route
    qb = uploaded(ctx)
    qb.plan_warm_start(timeWS=1.0)
    qb.solve()
    failed = np.flatnonzero(qb.download()["exitflag"] == 0)
    sel = failed if len(failed) else np.array([16, 0, 18])
    before_w, before_t = qb.warm_start()
    cnt, sw = qb.plan_warm_start(select=sel.astype(np.int32))
    w, t = qb.warm_start()
    others = np.setdiff1d(np.arange(Q.NI), sel)
    assert Q.bits(w[others], before_w[others]) and Q.bits(t, before_t) and (cnt[others] == OA.api.QUAD_PLAN_SKIPPED).all() and (sw[others] == 0).all()
    assert np.array_equal(cnt[sel] >= 2, ok[sel])
    planned = sel[ok[sel]]; kept = sel[~ok[sel]]
    assert Q.bits(w[planned], xws[planned]) and Q.bits(w[kept], before_w[kept])
    assert (qb.plan_paths()[others] == 0).all()
    with pytest.raises(OA.ObcaError):
        qb.clearance()      # unsolved again
    print("selected", sel.tolist(), "counts", cnt[sel].tolist())
    qb.close()


def test_warm_start_read_back_on_its_own(ctx):
    x0, xF, ob = Q.the20(); w0, t0 = Q.uploaded_start(N)
    qb = uploaded(ctx)
    w, t = qb.warm_start()
    assert Q.bits(w, w0) and Q.bits(t, t0)
    qb.solve()
    out = qb.download()
    qb.shift_warm_start(4)
    w, t = qb.warm_start()
    Ts = S.quad_sample_time(N)
    for i in range(Q.NI):
        prob = PK.pack_quad_problem(x0[i], xF[i], N, Ts, S.QUAD_R, ob[i], w0[i], t0[i], 1)
        new = QS.emu_shift(N, 4, prob, QS.iterate_of(N, out["xp"][i], out["timeScale"][i, 0]), out["info"][i])
        assert Q.bits(w[i].reshape(-1), new[PK.QPH_SIZE:]) and t[i] == new[PK.QPH_TWS], i
    assert (out["exitflag"] != 0).any() and not Q.bits(w, w0)      # (some instance solved: the shift moved something)
    qb.close()


def test_same_inputs_same_bits(ctx):
    from obca_amd import diag
    qb = uploaded(ctx)
    c1, _ = qb.plan_warm_start(timeWS=1.0); p1 = qb.plan_paths(); w1 = qb.warm_start()
    qb.close()
    qb = uploaded(ctx)
    c2, _ = qb.plan_warm_start(timeWS=1.0); p2 = qb.plan_paths(); w2 = qb.warm_start()
    qb.close()
    assert np.array_equal(c1, c2) and Q.bits(p1, p2) and Q.bits(w1[0], w2[0]) and Q.bits(w1[1], w2[1])
    qb = uploaded(ctx)
    cover = diag.leave_pattern(0, mask=4)
    c3, _ = qb.plan_warm_start(timeWS=1.0); p3 = qb.plan_paths(); w3 = qb.warm_start()
    qb.close()
    assert np.array_equal(c1, c3) and Q.bits(p1, p3) and Q.bits(w1[0], w3[0]) and Q.bits(w1[1], w3[1]), cover
    # more workgroups than CUs: instance i of 260 is instance i mod 20
    big = uploaded(ctx, tile=13)
    cb, _ = big.plan_warm_start(timeWS=1.0); pb = big.plan_paths(); wb = big.warm_start()
    ms = big.plan_ms()
    big.close()
    assert np.array_equal(cb, np.tile(c1, 13)) and Q.bits(pb, np.tile(p1, (13, 1, 1))) and Q.bits(wb[0], np.tile(w1[0], (13, 1, 1))) and Q.bits(wb[1], np.tile(w1[1], 13))
    print("260 plans: kernel %.3f ms" % ms)


def test_the_library_refuses_before_it_writes(ctx):
    fresh = OA.QuadBatch(ctx, Q.NI, N)
    for call in (fresh.plan_warm_start, fresh.warm_start, fresh.plan_ms, fresh.plan_paths):
        with pytest.raises(OA.ObcaError):      # nothing uploaded / nothing planned
            call()
    fresh.close()
    qb = uploaded(ctx); w0, t0 = Q.uploaded_start(N)
    for kw, text in ((dict(cap=1), "cap"), (dict(cap=PL.PLAN3D_WS_CAP + 1), "WS_CAP"), (dict(res=0.2), "MAXCELLS"), (dict(res=0.0), "res"), (dict(room=(10.0, 0.0, 5.0)), "room"),
                     (dict(clear=float("nan")), "clear"), (dict(select=[0, Q.NI]), "outside"), (dict(select=[3, 3]), "twice"), (dict(select=np.zeros(Q.NI, bool)), "empty"),
                     (dict(timeWS=0.0), "timeWS"), (dict(timeWS=float("inf")), "timeWS")):
        with pytest.raises(OA.ObcaError, match=text):
            qb.plan_warm_start(**kw)
    with pytest.raises(OA.ObcaError):
        qb.plan_paths()      # still no plan on this batch: no path buffer was made
    w, t = qb.warm_start()
    assert Q.bits(w, w0) and Q.bits(t, t0)
    qb.solve()
    assert qb.download()["exitflag"].shape == (Q.NI,)      # the refusals left the batch usable, and solved batches stay solved through a refusal:
    with pytest.raises(OA.ObcaError):
        qb.plan_warm_start(cap=1)
    assert qb.validate()["ok"].shape == (Q.NI,)
    qb.close()
