"""The device planner in PER-INSTANCE obstacle fields (include/obca_plan_scenes.h) on a machine without a GPU: the host build of the kernel text's per-instance route
(tests/emu/scenes_emu.cpp) against the existing shared-field host build (tests/emu/hybrid_emu.cpp), the host planner's collision test and the oracle.

The inputs (scenes_common.scenes): the first 32 of hybrid_common's 33 backwards poses; per instance the backwards field plus 1-3 boxes on the road from
scenarios.scene_field, default_rng(5), one stream over the instances in order.  Measured here with the host build: 4-6 obstacles and 9-17 rows per instance; all 32 have a
path with and without the analytic expansion; at most 7 520 expansions with it, 11 061 without; 13 of the 32 plans made in the shared three-obstacle field collide with
their own instance's field (11 without the analytic expansion), none of the own-field plans does."""
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import hybrid_common as H
import scenes_common as SC
from obca_amd import planner as PL, scenarios as S


def _rows_equal(a, b, rows_a, rows_b):
    return all(np.array_equal(a[k][rows_a], b[k][rows_b]) for k in H.FIELDS)


# ---------------------------------------------------------------- 1. one field, copied
@pytest.mark.parametrize("analytic", [None, 0.0])
def test_copies_of_one_field_equal_the_shared_field_call(analytic):
    """33 copies of the backwards field through the per-instance route = emu_hybrid_astar_batch, all five arrays bit for bit: loop orders 0 / 1 / 2, 1 and 4 slots"""
    sc, x0, xF, kw = H.poses("backwards", 33)
    ref = H.emu_plan("backwards", 33, analytic=analytic)
    assert ref["rc"] == 0 and (ref["counts"] > 0).sum() >= 30
    kw = kw if analytic is None else dict(kw, analytic=analytic)
    f = SC.shared_field()
    for order, slots in ((0, 1), (1, 4), (2, 4), (0, 4)):
        r = SC.run_scenes(x0, xF, [f] * 33, kw, slots=slots, order=order)
        assert r["rc"] == 0 and H.same(r, ref), (order, slots)


# ---------------------------------------------------------------- 2. own fields
def test_one_call_over_32_fields_equals_32_calls_of_the_shared_field_entry():
    """the 32 scenes in ONE per-instance call with 3 slots = 32 single-instance calls of the existing emu_hybrid_astar_batch, each given that instance's field: nothing
    of a slot's cell table, claim words or map is carried from one field into the next.  Also in descending loop order."""
    x0, xF, kw, fields = SC.scenes()
    own = SC.own_plan(); desc = SC.own_plan(order=1)
    assert own["rc"] == 0 and H.same(own, desc)
    assert sorted({len(f[0]) for f in fields}) == [4, 5, 6] and min(int(f[0].sum()) for f in fields) == 9 and max(int(f[0].sum()) for f in fields) == 17
    for i in range(SC.NSCENES):
        one = H.run_emu(None, x0[i:i + 1], xF[i:i + 1], kw, field_=fields[i])
        assert one["rc"] == 0 and _rows_equal(one, own, 0, i), i
    assert (own["counts"] >= 2).all() and own["expansions"].max() == 7520


# ---------------------------------------------------------------- 3. blocked map
def test_blocked_cells_from_the_device_text_equal_the_hosts_map():
    """hy::cell_blocked (what a search without a host map calls per cell) against blocked_out of the existing entry point (the host's disc_collides), byte for byte, and
    the holonomic map relaxed from it, for 8 of the scenes"""
    x0, xF, kw, fields = SC.scenes()
    for i in (0, 3, 5, 9, 13, 14, 22, 31):
        mine = SC.run_scenes(x0, xF, fields, kw, which=i)
        host = H.run_emu(None, x0[i:i + 1], xF[i:i + 1], kw, field_=fields[i], want_map=True)
        assert mine["dims"] == host["dims"] and np.array_equal(mine["blocked"], host["blocked"]), i
        assert host["blocked"].sum() > 2000 and np.array_equal(mine["map"], host["map"]), i
    free_ = H.run_emu(S.BACKWARDS, x0[:1], xF[:1], kw, want_map=True)
    assert not np.array_equal(free_["blocked"], host["blocked"])      # (the boxes do block cells)


# ---------------------------------------------------------------- 4. validity
@pytest.mark.parametrize("analytic", [None, 0.0])
def test_own_field_paths_are_valid_and_shared_field_plans_are_not(analytic):
    x0, xF, kw, fields = SC.scenes()
    own = SC.own_plan(analytic=analytic); sh = SC.shared_plan(analytic=analytic)
    margin = PL.DEFAULT_OPTS["margin"]
    hit = []
    for i in range(SC.NSCENES):
        n = own["counts"][i]
        assert n >= 2, i
        SC.check_path_in(fields[i], x0[i], xF[i], own["paths"][i, :n], own["dirs"][i, :n], margin, exact_goal=analytic is None, what="scene %d" % i)
        assert sh["counts"][i] >= 2
        hit.append(SC.collides_on(fields[i], sh["paths"][i, :sh["counts"][i]], margin))
    print("shared-field plans that collide with their own instance's field: %d of 32" % sum(hit))
    assert sum(hit) >= 8 and sum(hit) == (13 if analytic is None else 11)
    assert own["expansions"].max() == (7520 if analytic is None else 11061)


def test_the_host_planner_finds_a_path_in_every_scene():
    x0, xF, kw, fields = SC.scenes()
    for i in range(SC.NSCENES):
        assert PL.hybrid_astar(x0[i, :3], xF[i, :3], *fields[i], **kw) is not None, i


# ---------------------------------------------------------------- 5. codes and refusals
def test_a_box_over_one_start_pose_stops_that_instance_alone():
    x0, xF, kw, fields = SC.scenes(); base = SC.own_plan()
    fl = list(fields); fl[5] = SC.with_box(fields[5], *SC.box_over(x0[5]))
    r = SC.run_scenes(x0, xF, fl, kw)
    others = [i for i in range(SC.NSCENES) if i != 5]
    assert r["rc"] == 0 and r["counts"][5] == -2 and r["expansions"][5] == 0 and not r["paths"][5].any() and not r["dirs"][5].any()
    assert _rows_equal(r, base, others, others)


def test_a_closed_slot_mouth_gives_no_path():
    """A box across the slot's mouth, |x| <= 1.3, up to y = 6.5.  From y = 5.2 the goal pose stays free (the car's front stands at y = 5.0, the margin is 0.1 m) and the
    0.2 m left open lets nothing through: the open set runs empty, count 0.  From y = 5 (the blocks' top edge, the box as the issue words it) the goal pose itself overlaps
    the box by the margin, and by the ABI's rule for a pose that collides with its own field the count is -2 (measured: -2, 0 expansions)."""
    x0, xF, kw, fields = SC.scenes()
    for y0, want in ((5.2, 0), (5.0, -2)):
        pts = [[-1.3, 6.5], [1.3, 6.5], [1.3, y0], [-1.3, y0]]
        A2, b2 = S.obst_hrep(1, [5], [pts + [pts[0]]])
        r = SC.run_scenes(x0[3:5], xF[3:5], [SC.with_box(fields[3], A2, b2), fields[4]], kw, slots=1)
        assert r["rc"] == 0 and r["counts"][0] == want and not r["paths"][0].any(), (y0, r["counts"])
        assert (r["expansions"][0] > 1000 and r["rounds"][0] > 100) if want == 0 else r["expansions"][0] == 0
        assert _rows_equal(r, SC.own_plan(slots=3), 1, 4)      # the next search of the same slot is what it is alone


@pytest.mark.parametrize("analytic", [None, 0.0])
def test_a_small_node_pool_ends_the_large_searches_alone(analytic):
    x0, xF, kw, fields = SC.scenes(); full = SC.own_plan(analytic=analytic)
    r = SC.run_scenes(x0, xF, fields, kw if analytic is None else dict(kw, analytic=analytic), nodes=6000)
    order = np.argsort(full["expansions"], kind="stable")
    assert r["rc"] == 0 and r["counts"][order[-1]] == -3 and order[-1] == 13
    done = np.flatnonzero(r["counts"] != -3)
    assert set(order[:3].tolist()) <= set(done.tolist()) and (r["counts"][done] >= 2).all() and _rows_equal(r, full, done, done)
    assert not r["paths"][r["counts"] == -3].any()


def test_refusals_name_the_instance_and_touch_nothing():
    x0, xF, kw, fields = SC.scenes()
    box = SC.box_over(x0[5])
    many = fields[7]
    while len(many[0]) < 17:
        many = SC.with_box(many, *box)
    v, A, b = fields[7]
    long_ = (np.concatenate([v, [13]]).astype(np.int32), np.concatenate([A, np.tile([[1.0, 0.0]], (13, 1))]), np.concatenate([b, np.ones(13)]))
    An = A.copy(); An[2, 1] = np.nan
    zero = (np.concatenate([v, [0]]).astype(np.int32), A, b)
    for bad, word in ((many, "MAXOB"), (long_, "MAXROWS"), ((v, An, b), "not finite"), (zero, "MAXROWS")):
        fl = list(fields); fl[7] = bad
        if word == "not finite":
            fl[9] = many      # (a later instance that is wrong as well: the first one is named)
        r = SC.run_scenes(x0, xF, fl, kw)
        assert r["rc"] == -1 and "instance 7" in r["err"] and word in r["err"], r["err"]
        assert (r["paths"] == 7.0).all() and (r["dirs"] == 7).all() and (r["counts"] == 99).all() and (r["expansions"] == 55).all() and (r["rounds"] == 55).all()
    # NULL arrays; what the shared-field call refuses (an option out of range) is refused here with its words
    nOb, vv, AA, bb = SC.pack(fields)
    for packed in ((None, vv, AA, bb), (nOb, None, AA, bb), (nOb, vv, None, bb), (nOb, vv, AA, None)):
        r = SC.run_scenes(x0, xF, fields, kw, packed=packed)
        assert r["rc"] == -1 and (r["counts"] == 99).all(), r["err"]
    r = SC.run_scenes(x0, xF, fields, dict(kw, xy_res=0.001))
    assert r["rc"] == -1 and "option" in r["err"] and (r["counts"] == 99).all()
    # exactly the limits are legal
    sixteen = fields[7]
    while len(sixteen[0]) < 16:
        sixteen = SC.with_box(sixteen, *SC.box_over([-14.0, 3.0]))      # (inside the left block: they change nothing on the road)
    r = SC.run_scenes(x0[7:8], xF[7:8], [sixteen], kw)
    assert r["rc"] == 0 and _rows_equal(r, SC.own_plan(), 0, 7)


def test_an_instance_without_obstacles_is_a_free_field():
    x0, xF, kw, fields = SC.scenes()
    none = (np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0))
    r = SC.run_scenes(x0[:3], xF[:3], [none, fields[1], none], kw, which=0)
    assert r["rc"] == 0 and (r["counts"] >= 2).all() and not r["blocked"].any()
    assert _rows_equal(r, SC.own_plan(), 1, 1)
    for i in (0, 2):
        n = r["counts"][i]
        SC.check_path_in(none, x0[i], xF[i], r["paths"][i, :n], r["dirs"][i, :n], PL.DEFAULT_OPTS["margin"], what="free %d" % i)
    alone = SC.run_scenes(x0[:1], xF[:1], [none], kw, packed=(np.zeros(1, np.int32), None, None, None))      # (no obstacle in the batch: the arrays may be NULL)
    assert alone["rc"] == 0 and _rows_equal(alone, r, 0, 0)


# ---------------------------------------------------------------- 6. the oracle judges
def test_nlp_iterations_from_own_field_plans_total_less_where_the_shared_field_plan_collides(oracle):
    """Instances 0 .. 15 at N = 30, throughput options, each NLP with its own instance's field.  On the instances whose shared-field plan drives through a box of their own
    field -- 7 here: iterations 79, 84, 108, 101, 89, 141, 25 = 627 from those starts, 33, 61, 46, 23, 24, 144, 48 = 379 from the own-field plans -- the own-field total
    must be the smaller one.  No per-instance ordering is asserted (two instances go the other way); where the shared-field plan stays clear the two routes are the same
    path.  The test prints the figures."""
    N = 30; x0, xF, kw, fields = SC.scenes()
    own = SC.own_plan(); sh = SC.shared_plan(); margin = PL.DEFAULT_OPTS["margin"]
    hit = [i for i in range(16) if SC.collides_on(fields[i], sh["paths"][i, :sh["counts"][i]], margin)]
    clear = [i for i in range(16) if i not in hit]
    assert len(hit) >= 4 and all(np.array_equal(own[k][i], sh[k][i]) for i in clear for k in ("paths", "dirs", "counts"))      # (expansions may differ: the boxes change the map)
    iters = {"own": [], "shared": []}; flags = {"own": [], "shared": []}
    for i in hit:
        v, A, b = fields[i]
        for name, e in (("own", own), ("shared", sh)):
            n = e["counts"][i]
            Ts, xWS, uWS = PL.path_to_warm_start(e["paths"][i, :n], e["dirs"][i, :n], N, xF[i], v_nom=0.5)
            xWS = xWS.copy(); xWS[0] = x0[i]
            r = oracle.parking_signed_dist(x0[i], xF[i], N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b, xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, uWS, opts=oracle.default_opts())
            iters[name].append(int(r["iters"])); flags[name].append(int(r["exitflag"]))
    print("instances whose shared-field plan collides with their own field: %s" % hit)
    print("oracle iterations from own-field plans %s = %d (exit flags %s), from shared-field plans %s = %d (exit flags %s)"
          % (iters["own"], sum(iters["own"]), flags["own"], iters["shared"], sum(iters["shared"]), flags["shared"]))
    assert sum(iters["own"]) < sum(iters["shared"]), (iters, hit)


# ---------------------------------------------------------------- 7. surface
def _kinds(hdr):
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S); kinds = {}
    for m in re.finditer(r"\bint\s*(obca_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        kinds[m.group(1)] = ["ptr" if "*" in p or "[" in p else ("double" if re.match(r"\s*(const\s+)?double\b", p) else "int") for p in m.group(2).split(",")]
    return kinds


def test_header_exports_python_and_julia_agree():
    import ctypes as C
    import inspect
    import obca_amd
    from obca_amd import api, cabi
    protos = cabi.prototypes("obca_plan_scenes.h")
    assert sorted(protos) == sorted(api.SCENE_EXPORTS) and len(protos) == 2
    others = set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS) | set(api.REFINE_EXPORTS) | set(api.QUAD_SUBDIVIDE_EXPORTS) | set(api.PLAN_DEVICE_EXPORTS) | set(PL.PLAN3D_EXPORTS)
    assert not set(api.SCENE_EXPORTS) & others
    assert len(protos["obca_scene_astar_batch"][1]) == 20 and len(protos["obca_scene_astar_ms"][1]) == 2
    assert "obca_plan_scenes.h" in cabi.__doc__ and len(cabi.prototypes("obca_plan_device.h")) == 3
    # the per-instance call takes nOb as an array where the shared-field call takes a count; everything else is the same list
    dev = cabi.prototypes("obca_plan_device.h")["obca_hybrid_astar_batch"][1]
    mine = protos["obca_scene_astar_batch"][1]
    assert [type(a).__name__ for k, a in enumerate(mine) if k != 4] == [type(a).__name__ for k, a in enumerate(dev) if k != 4] and isinstance(mine[4], cabi.ArrayParam) and mine[4].const
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {s for s in exported if "scene" in s} == set(api.SCENE_EXPORTS)
    assert not any(w in s for s in api.SCENE_EXPORTS for w in ("hybrid", "refine", "subdivide", "clearance"))
    lib = api._load()
    assert [type(a).__name__ for a in lib.obca_scene_astar_batch.argtypes] == [type(a).__name__ for a in mine] and lib.obca_scene_astar_ms.argtypes[1] is C.POINTER(C.c_float)
    z = np.zeros(3)
    with pytest.raises((TypeError, C.ArgumentError)):      # nOb as float64
        lib.obca_scene_astar_batch(None, 1, z, z, np.zeros(1), np.zeros(1, np.int32), z, z, z, 1.0, z, None, 0, 0.0, z, np.zeros(3, np.int32), 2, np.zeros(1, np.int32), None, None)
    # no context: refused before anything else
    i1 = np.zeros(1, np.int32)
    assert lib.obca_scene_astar_batch(None, 1, z, z, i1, i1, z, z, z, 1.0, z, None, 0, 0.0, np.zeros(6), np.zeros(2, np.int32), 2, i1, None, None) == -1
    for f in ("scene_astar_batch", "scene_ms"):
        assert hasattr(obca_amd, f) and f in obca_amd.__all__
    sig = inspect.signature(api.scene_astar_batch).parameters
    assert list(sig) == ["starts", "goals", "vOb", "A", "b", "ego", "L", "XYbounds", "opts", "bucket_width", "cap", "device"] and sig["cap"].default == 1024 and sig["device"].default == 0
    sig = inspect.signature(PL.scene_astar_many).parameters
    assert sig["device"].default == 0 and sig["bucket_width"].default is None and sig["cap"].default == 1024
    sig = inspect.signature(PL.scene_warm_start_many).parameters
    assert list(sig)[:6] == ["x0", "xF", "N", "vOb", "A", "b"] and sig["device"].default == 0 and sig["smooth"].default is False and sig["v_nom"].default == 0.5
    sig = inspect.signature(S.make_scene_batch).parameters
    assert list(sig) == ["B", "N", "seed", "boxes", "device"] and sig["boxes"].default == (1, 3) and sig["device"].default is None and sig["N"].default == 80
    # every ccall of the shim against the header, parameter by parameter
    import test_julia_shim_cpu as J
    hdr = open(os.path.join(ROOT, "include", "obca_plan_scenes.h")).read()
    kinds = _kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCAPlanScenes.jl")).read()
    assert re.search(r"^const SCN = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), SCN\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
    assert {n for n, _ in calls} == set(kinds) == set(api.SCENE_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])


def test_python_routes_long_paths_and_limits_per_instance(monkeypatch):
    """planner.scene_astar_many / scene_warm_start_many with the device call replaced by the host build (no GPU here): per-instance lists reach the call as they are, an
    instance that outgrew its slot (-3) is None alone, and a path of more than cap nodes (-1) is searched again through the DEVICE call with ITS field and room for 20000."""
    from obca_amd import api
    x0, xF, kw, fields = SC.scenes(); own = SC.own_plan(); calls = []
    vl, Al, bl = SC.lists(fields[:4])

    def fake(starts, goals, vOb, A_, b_, ego, L, XYb, opts=None, bucket_width=None, cap=1024, device=0):
        nObs, vflat, Aflat, bflat = api._norm_obstacles(len(starts), vOb, A_, b_)
        calls.append((len(starts), cap, nObs.tolist()))
        idx = [int(np.flatnonzero((x0[:4, :3] == s_).all(axis=1))[0]) for s_ in starts]
        assert nObs.tolist() == [len(fields[i][0]) for i in idx] and np.array_equal(bflat, np.concatenate([fields[i][2] for i in idx])) and np.array_equal(opts, H.opts_array(kw))
        paths = np.zeros((len(idx), cap, 3)); dirs = np.zeros((len(idx), cap), np.int32); cnt = own["counts"][idx].copy()
        for j, i in enumerate(idx):
            paths[j, :cnt[j]] = own["paths"][i, :cnt[j]]; dirs[j, :cnt[j]] = own["dirs"][i, :cnt[j]]
            if i == 1:
                cnt[j] = -3; paths[j] = 0; dirs[j] = 0
            if i == 2 and cap == 1024:
                cnt[j] = -1; paths[j] = 0; dirs[j] = 0
        return paths, dirs, cnt, own["expansions"][idx].copy(), own["rounds"][idx].copy()
    monkeypatch.setattr(api, "scene_astar_batch", fake)
    res = PL.scene_astar_many(x0[:4], xF[:4], vl, Al, bl, device=0, **kw)
    assert calls == [(4, 1024, [len(f[0]) for f in fields[:4]]), (1, 20000, [len(fields[2][0])])] and res[1] is None
    for i in (0, 2, 3):
        assert np.array_equal(res[i][0], own["paths"][i, :own["counts"][i]]) and np.array_equal(res[i][1], own["dirs"][i, :own["counts"][i]]) and res[i][2] == own["expansions"][i]

    def fake_ws(paths, dirs, counts, N, xF_=None, v_nom=0.5, L=S.L_WHEELBASE, smooth=False, device=0):
        B = len(counts); Ts = np.zeros(B); xWS = np.zeros((B, N + 1, 4)); uWS = np.zeros((B, N, 2)); ok = np.zeros(B, bool)
        for i in range(B):
            if counts[i] >= 2:
                Ts[i], xWS[i], uWS[i] = PL.path_to_warm_start(paths[i, :counts[i]], dirs[i, :counts[i]], N, xF_[i], v_nom=v_nom); ok[i] = True
        return Ts, xWS, uWS, ok
    monkeypatch.setattr(PL, "path_to_warm_start_many", fake_ws)
    del calls[:]
    ws = PL.scene_warm_start_many(x0[:4], xF[:4], 30, vl, Al, bl, device=0, **kw)
    assert [c[:2] for c in calls] == [(4, 1024), (1, 20000)] and ws[1] is None
    for i in (0, 2, 3):
        Ts, xWS, uWS = PL.path_to_warm_start(own["paths"][i, :own["counts"][i]], own["dirs"][i, :own["counts"][i]], 30, xF[i], v_nom=0.5)
        assert ws[i][0] == Ts and np.array_equal(ws[i][1], xWS) and np.array_equal(ws[i][2], uWS), i
    # one field for all is broadcast by the call's own normalisation
    del calls[:]
    monkeypatch.setattr(api, "scene_astar_batch", lambda *a, **k: (calls.append(api._norm_obstacles(2, a[2], a[3], a[4])[0].tolist()), fake(a[0], a[1], vl[:2], Al[:2], bl[:2], *a[5:], **k))[1])
    v3, A3, b3 = SC.shared_field()
    PL.scene_astar_many(x0[:2], xF[:2], v3, A3, b3, device=0, **kw)
    assert calls[0] == [3, 3]


def test_make_scene_batch_on_the_host_route():
    bt = S.make_scene_batch(4, 30)
    assert bt["xWS"].shape == (4, 31, 4) and bt["uWS"].shape == (4, 30, 2) and np.isfinite(bt["xWS"]).all() and np.isfinite(bt["uWS"]).all() and (bt["Ts"] > 0).all()
    assert all(isinstance(bt[k], list) and len(bt[k]) == 4 for k in ("vOb", "A", "b"))
    for i in range(4):
        v, A, b = bt["vOb"][i], bt["A"][i], bt["b"][i]
        assert 4 <= len(v) <= 6 and list(v[:3]) == [2, 2, 1] and (np.asarray(v[3:]) == 4).all() and A.shape == (int(np.sum(v)), 2) and b.shape == (int(np.sum(v)),)
        assert np.abs(bt["xWS"][i, -1, :3] - bt["xF"][i, :3]).max() < 1e-9
        assert not any(PL.collides(p, v, A, b) for p in bt["xWS"][i, ::3, :3])      # (the resampled plan stays clear of the instance's own boxes)
    again = S.make_scene_batch(4, 30)
    assert all(np.array_equal(bt[k], again[k]) for k in ("x0", "Ts", "xWS", "uWS"))
    assert sorted(set(S.make_mixed_batch(2, 30)) ^ set(bt)) == []      # make_mixed_batch's dict


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu")
    GXX = ["g++", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-misleading-indentation"]
    name = "scenes_emu"
    assert name in BF.EMU_PIECES and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES)) and name not in BF.DEFAULT
    assert not set(BF.EMU_PIECES) & (set(BF.PIECES) | set(BF.TEST_PIECES) | set(BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_scenes_emu.so")
    deps = {os.path.realpath(d) for d in BF.dependencies(p.sources)}
    todo = [os.path.realpath(s) for s in p.sources]; seen = set()
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        assert f in deps, f
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', open(f).read(), flags=re.M):
            assert os.path.exists(os.path.join(os.path.dirname(f), inc)), (f, inc)
            todo.append(os.path.realpath(os.path.join(os.path.dirname(f), inc)))
    csrc = os.path.join(ROOT, "obca_amd", "csrc")
    for h in (os.path.join(csrc, "obca_hybrid.h"), os.path.join(csrc, "obca_plan_geom.h"), os.path.join(ROOT, "include", "obca_plan_scenes.h"), os.path.join(ROOT, "include", "obca_plan_device.h")):
        assert os.path.realpath(h) in seen, h
    assert os.path.realpath(os.path.join(csrc, "obca_solver.h")) not in seen
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_scenes_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == GXX + ["-O1"] and argv[i + 2:] == [EMU + "/scenes_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # one kernel in the source, two code paths: a template on a boolean, instantiated by the two host calls
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    after = hip.split('#include "obca_hybrid.h"')[1]
    assert after.count("__global__") == 1 and re.search(r"template <bool SCENES>\s*__global__ __launch_bounds__\(HY_NT\) void obca_hybrid_kernel\(", after)
    assert "obca_hybrid_kernel<false>" in after and "obca_hybrid_kernel<true>" in after
