"""The resident route of the parking planner on the device (obca_batch_plan_warm_start, include/obca_plan_resident.h): an uploaded batch planned from its own records.
The block the device's packing kernel wrote against the host build's packing, bit for bit, and the host build of the route (tests/emu/plan_resident_emu.cpp) run over the
device's own block -- bit for bit with the analytic expansion off, where nothing but the block's sines and cosines comes from a libm --, against the host-pointer route on the device (scene_astar_batch + set_path_warm_start) with it on, and down to
solved batches.  Inputs: the 16 scenes of tests/plan_resident_common.py, N = 30."""
import numpy as np
import pytest
import hybrid_common as H
import plan_resident_common as R
import scenes_common as SC
import obca_amd
from obca_amd import api, planner as PL, scenarios as S

pytestmark = pytest.mark.gpu
OUT = ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info")
_runs = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_batches():
    yield
    for r in _runs.values():
        r["batch"].close()
    _runs.clear()


def _bits(a, b):
    if isinstance(a, (list, tuple)):      # (the multipliers of a download: one array per instance)
        return len(a) == len(b) and all(_bits(x, y) for x, y in zip(a, b))
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _upload(x0, xF, fields, Ts=None, xWS=None, uWS=None):
    """a batch as the resident route expects it: poses, fields, a tracking reference and a start of zeros unless given"""
    B = len(fields); z = np.zeros((B, R.N + 1))
    b = obca_amd.Batch(api._ctx(0), B, R.N)
    ref = (z, z, z) if xWS is None else (xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2])
    b.upload(x0, xF, np.full(B, R.TS) if Ts is None else Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, *SC.lists(fields), *ref, 0, xWS, uWS)
    return b


def _plan(x0, xF, fields, kw, **more):
    api.hybrid_configure(slots=16, max_nodes=H.NODES)
    b = _upload(x0, xF, fields)
    cnt, st, nexp, rounds = b.plan_warm_start(**kw, **more)
    paths, dirs, inst = b.plan_paths()
    block, dims = b.plan_block()
    return dict(batch=b, counts=cnt, status=st, expansions=nexp, rounds=rounds, paths=paths, dirs=dirs, inst=inst, block=block, dims=dims)


def _run16(analytic):
    """the 16 scenes through the resident route, once per setting of the analytic expansion; the batch stays open for the tests that solve it"""
    if analytic not in _runs:
        x0, xF, kw, fields = R.scenes16()
        _runs[analytic] = _plan(x0, xF, fields, kw if analytic is None else dict(kw, analytic=analytic))
    return _runs[analytic]


def test_analytic_expansion_off_device_equals_the_host_build_on_the_devices_block():
    """the block the device's packing kernel wrote (obca_batch_packed_block): every word an instance uses against the host build's packing, bit for bit -- rows, norms, counts,
    offsets, the clipped vertices: the device check of the clipping divisions, the count exchange through LDS and the vertex prefix --, the sines and cosines within their
    bound; then the host build's search over THAT block against the device's search"""
    x0, xF, kw, fields = R.scenes16()
    dev = _run16(0.0); inst = dev["inst"]
    prob, z0, nObMax, MMax = R.records(x0, xF, fields)
    assert dev["dims"]["B"] == R.NS and dev["dims"]["nObMax"] == nObMax and dev["dims"]["MMax"] == MMax
    mine = R.views(dev["block"], R.NS, nObMax, MMax); host = R.views(R.pack_block(prob, nObMax, MMax), R.NS, nObMax, MMax)
    assert _bits(mine["rec"], host["rec"]) and _bits(mine["inst"].reshape(R.NS, 10), inst)
    for i in range(R.NS):
        a, b = R.field_of(mine, i), R.field_of(host, i)
        for k in ("v", "off", "voff", "A", "b", "rn", "nrm", "vert"):
            assert _bits(a[k], b[k]), (i, k, a[k], b[k])
    assert _bits(inst[:, :3], x0[:, :3]) and _bits(inst[:, 5:8], xF[:, :3])
    err = max(np.abs(inst[:, 3] - np.sin(x0[:, 2])).max(), np.abs(inst[:, 4] - np.cos(x0[:, 2])).max(), np.abs(inst[:, 8] - np.sin(xF[:, 2])).max(), np.abs(inst[:, 9] - np.cos(xF[:, 2])).max())
    print("largest difference of the device's sines and cosines from numpy's: %.3g" % err)
    assert err <= 1e-15      # 2 ulp of the device functions + 1 ulp of the host's, of values <= 1, times three
    ref = R.plan(prob, z0, nObMax, MMax, dict(kw, analytic=0.0), block=dev["block"])
    assert ref["rc"] == 0 and (ref["counts"] >= 2).all(), ref["err"]
    for k in H.FIELDS + ("status",):
        assert np.array_equal(dev[k], ref[k]), (k, np.flatnonzero((dev[k] != ref[k]).reshape(R.NS, -1).any(axis=1)))


def test_analytic_expansion_on_matches_the_host_pointer_route():
    """tests/test_gpu_hybrid.py's rule: counts, dirs, expansions and rounds equal and poses within 1e-9, at most ONE of the 16 may differ (the two routes start from sines and
    cosines of two libms; test_plan_resident_cpu.py moves each by an ulp on the host build and no count of these 16 changes)"""
    x0, xF, kw, fields = R.scenes16(); margin = H.opts_array(kw)[5]
    dev = _run16(None)
    api.hybrid_configure(slots=16, max_nodes=H.NODES)
    ref = dict(zip(H.FIELDS, api.scene_astar_batch(x0, xF, *SC.lists([R.unit(f) for f in fields]), S.EGO, S.L_WHEELBASE, S.XYBOUNDS, H.opts_array(kw), None, H.CAP)))
    differ = [i for i in range(R.NS) if dev["counts"][i] != ref["counts"][i]]
    print("scenes that differ in counts: %s (resident %s, host-pointer route %s)" % (differ, dev["counts"][differ], ref["counts"][differ]))
    assert len(differ) <= 1, (differ, dev["counts"][differ], ref["counts"][differ])
    for i in range(R.NS):
        n = dev["counts"][i]
        if i in differ:
            assert n >= 2
            SC.check_path_in(fields[i], x0[i], xF[i], dev["paths"][i, :n], dev["dirs"][i, :n], margin, what="scene %d" % i)
            continue
        assert dev["expansions"][i] == ref["expansions"][i] and dev["rounds"][i] == ref["rounds"][i], (i, dev["expansions"][i], ref["expansions"][i])
        assert np.array_equal(dev["dirs"][i], ref["dirs"][i]), i
        err = np.abs(dev["paths"][i] - ref["paths"][i]); err[:, 2] = np.abs(np.angle(np.exp(1j * (dev["paths"][i, :, 2] - ref["paths"][i, :, 2]))))
        assert err.max() <= 1e-9, (i, err.max())


def test_the_start_written_equals_set_path_warm_start_of_the_downloaded_paths():
    """a second batch from the same inputs, its start written by the existing call from the paths the resident call planned: both solved with the throughput options, every
    output bit for bit"""
    x0, xF, kw, fields = R.scenes16()
    dev = _run16(0.0)
    other = _upload(x0, xF, fields)
    st = other.set_path_warm_start(dev["paths"], dev["dirs"], dev["counts"])
    assert np.array_equal(st, dev["status"]) and (st == 0).all()
    dev["batch"].solve(); other.solve()
    a = dev["batch"].download(); b = other.download(); other.close()
    for k in OUT:
        assert _bits(a[k], b[k]), k
    assert (a["exitflag"] == 1).sum() >= R.NS // 2      # (the starts are usable ones)


def test_upload_plan_solve_validate_and_an_instance_that_keeps_its_start():
    x0, xF, kw, fields = R.scenes16()
    fl = list(fields); fl[5] = SC.with_box(fields[5], *SC.box_over(x0[5]))
    run = _plan(x0, xF, fl, kw)
    b = run["batch"]
    keep = np.arange(R.NS) != 5
    assert run["counts"][5] == -2 and run["status"][5] < 0 and (run["status"][keep] == 0).all()
    b.solve(); v = b.validate(); out = b.download(); b.close()
    # the host route from the same inputs: scene_warm_start_many, upload, solve (the instance without a plan uploads the zeros it kept here)
    vl, Al, bl = SC.lists(fl)
    ws = PL.scene_warm_start_many(x0, xF, R.N, vl, Al, bl, device=0, **kw)
    assert ws[5] is None and all(w is not None for i, w in enumerate(ws) if i != 5)
    Ts = np.array([R.TS if w is None else w[0] for w in ws]); xWS = np.stack([np.zeros((R.N + 1, 4)) if w is None else w[1] for w in ws])
    uWS = np.stack([np.zeros((R.N, 2)) if w is None else w[2] for w in ws])
    hb = _upload(x0, xF, fl, Ts, xWS, uWS)
    hb.solve(); hout = hb.download(); hb.close()
    print("resident exit flags %s, host route %s, validate ok %s" % (out["exitflag"].tolist(), hout["exitflag"].tolist(), v["ok"].astype(int).tolist()))
    assert out["exitflag"].tolist() == hout["exitflag"].tolist() and (out["exitflag"][keep] == 1).sum() >= R.NS // 2
    assert v["ok"][out["exitflag"] == 1].all()
    # the neighbours of the blocked instance: what they are in the batch without the box
    base = _run16(None)
    assert all(np.array_equal(run[k][keep], base[k][keep]) for k in H.FIELDS + ("status",))
    base["batch"].solve(); bout = base["batch"].download()
    assert np.array_equal(out["exitflag"][keep], bout["exitflag"][keep]) and _bits(out["xp"][keep], bout["xp"][keep]) and _bits(out["up"][keep], bout["up"][keep])


def test_timers_slots_and_refusals():
    x0, xF, kw, fields = R.scenes16(); n = 4
    api.hybrid_configure(slots=4, max_nodes=H.NODES)
    b = _upload(x0[:n], xF[:n], fields[:n])
    with pytest.raises(api.ObcaError):      # no call yet
        b.plan_ms()
    with pytest.raises(api.ObcaError, match="no plan of this batch"):
        b.plan_paths()
    with pytest.raises(api.ObcaError, match="no plan of this batch"):
        b.plan_block()
    first = b.plan_warm_start(**kw)
    ms = b.plan_ms()
    assert len(ms) == 3 and all(m > 0 for m in ms), ms
    bytes0 = b.scratch_bytes(); allocs0 = b.plan_block()[1]
    again = b.plan_warm_start(bucket_width=0.35, **kw)      # another bucket width: other rounds, the same slots
    allocs1 = b.plan_block()[1]
    assert b.scratch_bytes() == bytes0 and all(m > 0 for m in b.plan_ms())
    # the slots and the staging block live in the context: neither was allocated again by the second call
    assert allocs0["slot_allocs"] >= 1 and allocs0["io_allocs"] >= 1 and (allocs1["slot_allocs"], allocs1["io_allocs"]) == (allocs0["slot_allocs"], allocs0["io_allocs"])
    short = b.plan_warm_start(cap=600, **kw)      # plan_paths sizes its arrays by what the library says the last call's cap was
    assert b.plan_paths()[0].shape == (n, 600, 3) and np.array_equal(short[0], first[0])
    again = b.plan_warm_start(bucket_width=0.35, **kw)
    assert (again[0] >= 2).all() and (first[0] >= 2).all() and not np.array_equal(again[3], first[3])
    paths, dirs, inst = b.plan_paths()
    assert paths.shape == (n, 1024, 3) and inst.shape == (n, 10) and all(not paths[i, c:].any() and not dirs[i, c:].any() and paths[i, :c].any() for i, c in enumerate(again[0]))
    # another planner call of the context takes the staging block: the paths of the batch's call are gone, and the call says so
    api.scene_astar_batch(x0[:1], xF[:1], *SC.lists(fields[:1]), S.EGO, S.L_WHEELBASE, S.XYBOUNDS, H.opts_array(kw), None, H.CAP)
    with pytest.raises(api.ObcaError, match="later planner call"):
        b.plan_paths()
    with pytest.raises(api.ObcaError, match="later planner call"):
        b.plan_block()
    # refusals, each -1 with a message before anything is launched: the record and the start stay what they are
    for bad, text in ((dict(cap=1), "cap"), (dict(cap=1025), "cap"), (dict(v_nom=0.0), "v_nom"), (dict(nh_res=1.0), "lattice"), (dict(xy_res=0.0), "out of range"), (dict(bucket_width=1e-9), "bucket_width")):
        with pytest.raises(api.ObcaError, match=text):
            b.plan_warm_start(**{**kw, **bad})
    st = np.zeros(n, np.int32)
    assert api._load().obca_batch_plan_warm_start(b._h, None, 0, 0.0, 1024, 1, 0.5, 0.0, None, st, None, None) == -1
    assert api._load().obca_batch_plan_warm_start(b._h, None, 0, 0.0, 1024, 1, 0.5, 0.0, st, None, None, None) == -1
    empty = obca_amd.Batch(api._ctx(0), n, R.N)
    with pytest.raises(api.ObcaError, match="nothing uploaded"):
        empty.plan_warm_start(**kw)
    empty.close()
    # the destination of refine starts from a solution: it has no ego / XYbounds of an upload and is refused
    b.solve()
    fine, _ = b.refine(2)
    with pytest.raises(api.ObcaError, match="nothing uploaded"):
        fine.plan_warm_start(**kw)
    fine.close(); b.close()
