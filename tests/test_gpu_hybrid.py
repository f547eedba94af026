"""The parking planner on the device (obca_hybrid_astar_batch, include/obca_plan_device.h) against the host build of the same kernel text (tests/emu/hybrid_emu.cpp): bit for bit
where no libm result enters the search (analytic expansion off), within the issue's cap where the Reeds-Shepp curves do; the parallel scenario (the 27 391-cell map in LDS);
planner.warm_start_many(search="device").  Inputs and the validity rules: tests/hybrid_common.py."""
import numpy as np
import pytest
import hybrid_common as H
from obca_amd import api, planner as PL, scenarios as S

pytestmark = pytest.mark.gpu


def device_plan(which, B, slots, analytic=None, bw=None, nodes=H.NODES, chunks=0, sel=None):
    sc, x0, xF, kw = H.poses(which, B)
    if analytic is not None:
        kw = dict(kw, analytic=analytic)
    if sel is not None:
        x0, xF = x0[sel], xF[sel]
    v, A, b = H.field(sc)
    api.hybrid_configure(slots=slots, max_nodes=nodes, max_chunks=chunks)
    paths, dirs, cnt, nexp, rounds = api.hybrid_astar_batch(x0, xF, v, A, b, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, H.opts_array(kw), bw, H.CAP)
    assert api.hybrid_ms() > 0
    return dict(paths=paths, dirs=dirs, counts=cnt, expansions=nexp, rounds=rounds)


def compare_with_libm(which, B, dev, ref, max_differ):
    """counts, dirs, expansions, rounds equal and poses within 1e-9 -- except on at most max_differ instances (a Reeds-Shepp sample or family tie within rounding of a boundary),
    whose own paths must still be valid"""
    sc, x0, xF, kw = H.poses(which, B); margin = H.opts_array(kw)[5]
    differ = [i for i in range(B) if dev["counts"][i] != ref["counts"][i]]
    print("%s: instances that differ in counts: %s (device %s, host build %s)" % (which, differ, dev["counts"][differ], ref["counts"][differ]))
    assert len(differ) <= max_differ, (differ, dev["counts"][differ], ref["counts"][differ])
    for i in range(B):
        n = dev["counts"][i]
        if i in differ:
            if n > 0:
                H.check_path(sc, x0[i], xF[i], dev["paths"][i, :n], dev["dirs"][i, :n], margin, what=(which, i))
            continue
        assert dev["expansions"][i] == ref["expansions"][i] and dev["rounds"][i] == ref["rounds"][i], (which, i, dev["expansions"][i], ref["expansions"][i], dev["rounds"][i], ref["rounds"][i])
        assert np.array_equal(dev["dirs"][i], ref["dirs"][i]), (which, i)
        err = np.abs(dev["paths"][i] - ref["paths"][i]); err[:, 2] = np.abs(np.angle(np.exp(1j * (dev["paths"][i, :, 2] - ref["paths"][i, :, 2]))))
        assert err.max() <= 1e-9, (which, i, err.max())


def test_analytic_expansion_off_device_equals_host_build_bit_for_bit():
    B = 33
    dev = device_plan("backwards", B, slots=4, analytic=0.0)
    ref = H.emu_plan("backwards", B, analytic=0.0)
    assert (ref["counts"] > 0).sum() >= B - 2
    for k in H.FIELDS:
        assert np.array_equal(dev[k], ref[k]), (k, np.flatnonzero((dev[k] != ref[k]).reshape(B, -1).any(axis=1)))
    # a pool of 6000 nodes: too small for the search with the most expansions (9005 popped nodes), enough for the three with the fewest (at most 2326 popped, fewer than 3 kept
    # successors each): -3 for that search alone, on the device as in the host build
    sc, x0, xF, kw = H.poses("backwards", B)
    sel = np.argsort(ref["expansions"])[[-1, 0, 1, 2]]
    small = device_plan("backwards", B, slots=2, analytic=0.0, nodes=6000, sel=sel)
    want = H.run_emu(sc, x0[sel], xF[sel], dict(kw, analytic=0.0), nodes=6000, slots=2)
    assert small["counts"][0] == -3 and (small["counts"][1:] > 0).all()
    for k in H.FIELDS:
        assert np.array_equal(small[k], want[k]), k


def test_analytic_expansion_on_device_matches_host_build():
    B = 33
    dev = device_plan("backwards", B, slots=4)
    ref = H.emu_plan("backwards", B)
    assert (ref["counts"] > 0).sum() >= B - 1
    compare_with_libm("backwards", B, dev, ref, max_differ=1)


def test_parallel_scenario_paths_are_valid_and_match_the_host_build():
    B = 4; sc, x0, xF, kw = H.poses("parallel", B); margin = H.opts_array(kw)[5]
    dev = device_plan("parallel", B, slots=2)
    for i in range(B):
        n = dev["counts"][i]
        assert n > 0, (i, n)
        H.check_path(sc, x0[i], xF[i], dev["paths"][i, :n], dev["dirs"][i, :n], margin, what=("parallel", i))
        assert (dev["paths"][i, n:] == 0).all() and (dev["dirs"][i, n:] == 0).all()
    compare_with_libm("parallel", B, dev, H.emu_plan("parallel", B), max_differ=1)


def test_far_list_on_the_device():
    """a bucket width of 0.002: 2 m of f per window, the window moves; no libm in the search (analytic expansion off)"""
    sc, x0, xF, kw = H.poses("backwards", 33); sel = np.arange(6)
    dev = device_plan("backwards", 33, slots=3, analytic=0.0, bw=0.002, sel=sel)
    ref = H.run_emu(sc, x0[sel], xF[sel], dict(kw, analytic=0.0), bw=0.002)
    for k in H.FIELDS:
        assert np.array_equal(dev[k], ref[k]), k


def test_warm_start_many_with_the_search_on_the_device():
    B, N = 16, 30; sc, x0, xF, kw = H.poses("backwards", 33); x0, xF = x0[:B], xF[:B]
    api.hybrid_configure(slots=4, max_nodes=H.NODES)
    got = PL.warm_start_many(sc, x0, xF, N, device=0, search="device")
    v, A, b = H.field(sc)
    paths, dirs, cnt, _, _ = api.hybrid_astar_batch(x0, xF, v, A, b, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, H.opts_array(kw), None, H.CAP)
    Ts, xWS, uWS, ok = PL.path_to_warm_start_many(paths, dirs, cnt, N, xF, v_nom=0.5, device=0)
    assert len(got) == B and ok.sum() >= B - 1
    for i in range(B):
        if not ok[i]:
            assert got[i] is None
        else:
            assert got[i][0] == Ts[i] and np.array_equal(got[i][1], xWS[i]) and np.array_equal(got[i][2], uWS[i]), i
    # the list form: the same paths as the dense call
    many = PL.hybrid_astar_many(x0, xF, v, A, b, device=0, **kw)
    for i in range(B):
        assert (many[i] is None) == (cnt[i] <= 0)
        if many[i] is not None:
            assert np.array_equal(many[i][0], paths[i, :cnt[i]]) and np.array_equal(many[i][1], dirs[i, :cnt[i]])
    # a batch made with the searches on the device solves as one made with the host planner does
    bt = S.make_batch(S.BACKWARDS, 8, N, planner=True, device=0, search="device")
    assert bt["xWS"].shape == (8, N + 1, 4) and np.isfinite(bt["xWS"]).all() and (bt["Ts"] > 0).all()
