"""The round-synchronous Hybrid A* of the device (obca_amd/csrc/obca_hybrid.h) compiled for the host (tests/emu/hybrid_emu.cpp): order independence, validity of the paths, return
codes, the holonomic map against a heapq Dijkstra, slot reuse, the NLP's view of the plans (oracle), the public surface and the host build as a piece of the build rule.  No GPU.
Inputs and the validity rules: tests/hybrid_common.py."""
import ctypes as C
import heapq
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import hybrid_common as H
from obca_amd import planner as PL, scenarios as S


# ---------------------------------------------------------------- 1. order independence
@pytest.mark.parametrize("which,B", [("backwards", 32), ("parallel", 4)])
def test_results_do_not_depend_on_the_order_of_a_rounds_items(which, B):
    ref = H.emu_plan(which, B, order=0)
    assert ref["rc"] == 0 and (ref["counts"] > 0).sum() >= B - 1 and (ref["rounds"][ref["counts"] > 0] > 0).all()
    for order in (1, 2):      # descending, shuffled
        got = H.emu_plan(which, B, order=order)
        for k in H.FIELDS:
            assert np.array_equal(ref[k], got[k]), (which, order, k, np.flatnonzero((ref[k] != got[k]).reshape(B, -1).any(axis=1)))


def test_order_independence_holds_with_the_far_list_in_use():
    """a bucket width of 0.002 puts f beyond the window of 1024 bucket heads (2 m of f): entries wait in the far list and the window moves"""
    sc, x0, xF, kw = H.poses("backwards", 32)
    runs = [H.run_emu(sc, x0[:6], xF[:6], kw, bw=0.002, order=o) for o in (0, 1, 2)]
    assert (runs[0]["counts"] > 0).all()
    assert H.same(runs[0], runs[1]) and H.same(runs[0], runs[2])
    wide = H.run_emu(sc, x0[:6], xF[:6], kw, bw=0.002 * 4096)      # the same searches inside one window
    assert (wide["counts"] > 0).all() and (runs[0]["rounds"] > wide["rounds"]).all()


# ---------------------------------------------------------------- 2. validity
@pytest.mark.parametrize("which,B", [("backwards", 64), ("parallel", 8)])
def test_paths_are_valid_and_as_many_as_the_host_search_finds(which, B):
    sc, x0, xF, kw = H.poses(which, B)
    e = H.emu_plan(which, B); host = H.host_plan(which, B)
    assert e["rc"] == 0
    margin = H.opts_array(kw)[5]
    for i in np.flatnonzero(e["counts"] > 0):
        n = e["counts"][i]
        H.check_path(sc, x0[i], xF[i], e["paths"][i, :n], e["dirs"][i, :n], margin, what=(which, int(i)))
        assert (e["paths"][i, n:] == 0).all() and (e["dirs"][i, n:] == 0).all()
    lost = np.flatnonzero((e["counts"] <= 0) & (host[4] > 0))
    assert len(lost) <= (1 if B == 64 else 0), (which, lost, e["counts"][lost])
    assert np.array_equal(e["counts"] == -2, host[4] == -2)      # a colliding start is one for both
    # the host search alone meets the cap on these inputs
    assert (host[4] <= 0).sum() <= 1


# ---------------------------------------------------------------- 3. return codes
def test_return_codes():
    sc, x0, xF, kw = H.poses("backwards", 32)
    v, A, b = H.field(sc)
    good = H.emu_plan("backwards", 32)
    s3, g3 = x0[:3].copy(), xF[:3].copy()
    # a colliding start: -2 for that instance, its neighbours as they were
    s = s3.copy(); s[1, :3] = [0.0, 20.0, 0.0]
    r = H.run_emu(sc, s, g3, kw)
    assert r["counts"][1] == -2 and r["expansions"][1] == 0 and (r["paths"][1] == 0).all()
    for i in (0, 2):
        assert r["counts"][i] == good["counts"][i] and np.array_equal(r["paths"][i], good["paths"][i])
    # a goal walled in by four obstacles: no path, and the search ends because the open set is empty
    gx, gy = 5.0, 6.0
    walls = [(gx - 4, gx + 4, gy + 3, gy + 3.5), (gx - 4, gx + 4, gy - 3.5, gy - 3), (gx - 4.5, gx - 4, gy - 3.5, gy + 3.5), (gx + 4, gx + 4.5, gy - 3.5, gy + 3.5)]
    Aw = np.tile(np.array([[1.0, 0], [-1, 0], [0, 1], [0, -1]]), (4, 1)); bw_ = np.concatenate([[x1, -x0_, y1, -y0_] for x0_, x1, y0_, y1 in walls])
    fld = (np.full(4, 4, np.int32), Aw, bw_)
    r = H.run_emu(sc, np.array([[-8.0, 6.0, 0.0]]), np.array([[gx, gy, 0.0]]), dict(max_expansions=400000), field_=fld)
    assert r["rc"] == 0 and r["counts"][0] == 0 and 0 < r["expansions"][0] < 400000
    # cap smaller than the path: -1
    n0 = int(good["counts"][0])
    r = H.run_emu(sc, s3, g3, kw, cap=n0 - 1)
    assert r["counts"][0] == -1 and (r["paths"][0] == 0).all()
    r = H.run_emu(sc, s3[:1], g3[:1], kw, cap=n0)
    assert r["counts"][0] == n0 and np.array_equal(r["paths"][0], good["paths"][0, :n0])
    # node pool and chunk pool forced tiny: -3 for the instance that needs more, the others as they were
    need = np.argsort(good["expansions"][:8])      # the instance of the first eight with the fewest expansions fits a pool the one with the most does not
    pick = np.array([need[0], need[-1], need[0]])
    # (600 nodes: the easy search pops 123 entries of at most 10 successors each and commits fewer than 600, the hard one pops 2086; 200 chunks: the easy one runs 62 rounds,
    #  the hard one 172 rounds and more than 200 x 15 entries)
    for nodes, chunks in ((600, 0), (H.NODES, 200)):
        r = H.run_emu(sc, x0[pick], xF[pick], kw, nodes=nodes, chunks=chunks, slots=1)
        assert r["counts"][1] == -3 and (r["paths"][1] == 0).all(), (nodes, chunks, r["counts"])
        for j in (0, 2):
            assert r["counts"][j] == good["counts"][pick[j]] and np.array_equal(r["paths"][j], good["paths"][pick[j]]), (nodes, chunks, j, r["counts"])
    # max expansions 50: no path
    hard = int(np.argmax(good["expansions"]))
    r = H.run_emu(sc, x0[hard:hard + 1], xF[hard:hard + 1], dict(kw, max_expansions=50))
    assert r["counts"][0] == 0 and r["expansions"][0] <= 50
    # ... decided by the LIVE entries of a round: a bound one above what the search needs lets it finish with the same path, one below what it needs ends it with 0
    need_ = int(good["expansions"][hard])
    r = H.run_emu(sc, x0[hard:hard + 1], xF[hard:hard + 1], dict(kw, max_expansions=need_))
    assert r["counts"][0] == good["counts"][hard] and r["expansions"][0] == need_ and np.array_equal(r["paths"][0], good["paths"][hard])
    r = H.run_emu(sc, x0[hard:hard + 1], xF[hard:hard + 1], dict(kw, max_expansions=need_ - 1))
    assert r["counts"][0] == 0 and r["expansions"][0] < need_
    # the lattice heuristic, non-finite input, other refusals: -1 for the call, nothing written
    for bad_kw, msg in ((dict(nh_res=0.5), b"lattice"), (dict(h_weight=0.0), b"weight"), (dict(steer_samples=16), b"range"), (dict(xy_res=0.05), b"OBCA_HYBRID_MAXMAP"),
                        (dict(reverse_cost=-0.1), b"negative"), (dict(switch_cost=-1.0), b"negative"), (dict(steer_cost=-0.3), b"negative"), (dict(steer_change_cost=-1e-9), b"negative")):
        r = H.run_emu(sc, s3, g3, dict(kw, **bad_kw))
        assert r["rc"] == -1 and msg in H.emu().emu_hybrid_last_error() and (r["counts"] == 99).all() and (r["paths"] == 7.0).all(), bad_kw
    for where in ("start", "goal", "opts", "A", "bw"):
        s = s3.copy(); g = g3.copy(); k2 = dict(kw); f = [v, A.copy(), b.copy()]; bw = 0.0
        if where == "start": s[2, 1] = np.nan
        if where == "goal": g[0, 2] = np.inf
        if where == "opts": k2["step"] = np.nan
        if where == "A": f[1][0, 0] = np.nan
        if where == "bw": bw = np.nan
        r = H.run_emu(sc, s, g, k2, bw=bw, field_=tuple(f))
        assert r["rc"] == -1 and b"finite" in H.emu().emu_hybrid_last_error() and (r["counts"] == 99).all(), where


# ---------------------------------------------------------------- 4. the holonomic map
@pytest.mark.parametrize("which", ["backwards", "parallel"])
def test_holonomic_map_is_the_dijkstra_field_bit_for_bit(which):
    """The relaxation ends in the largest fixed point below the start field; Dijkstra with the same fp32 additions computes the same numbers, because fp32 addition of a
    non-negative weight is monotone: both are the minimum over all cell paths of the left-to-right fp32 sum of their edge weights."""
    sc, x0, xF, kw = H.poses(which, 8)
    maps = [H.run_emu(sc, x0[:1], xF[:1], dict(kw, max_expansions=0), want_map=True, order=o) for o in (0, 1, 2)]
    r = maps[0]; nx, ny = r["dims"]; blocked = r["blocked"].astype(bool); res = H.opts_array(kw)[0]
    if which == "parallel":
        assert (nx, ny) == (301, 91)
    assert blocked.any() and not blocked.all()
    w = {1: np.float32(res * np.hypot(1.0, 0.0)), 2: np.float32(res * np.hypot(1.0, 1.0))}
    gx = min(nx - 1, max(0, int(np.floor((xF[0, 0] - S.XYBOUNDS[0]) / res + 0.5)))); gy = min(ny - 1, max(0, int(np.floor((xF[0, 1] - S.XYBOUNDS[2]) / res + 0.5))))
    d = np.full((ny, nx), np.inf, np.float32); d[gy, gx] = 0; pq = [(np.float32(0), gy, gx)]
    while pq:
        c, y, x = heapq.heappop(pq)
        if c > d[y, x]:
            continue
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                qx, qy = x + dx, y + dy
                if (dx or dy) and 0 <= qx < nx and 0 <= qy < ny and not blocked[qy, qx]:
                    cn = np.float32(c + w[dx * dx + dy * dy])
                    if cn < d[qy, qx]:
                        d[qy, qx] = cn; heapq.heappush(pq, (cn, qy, qx))
    got = r["map"].copy()
    free = ~blocked; free[gy, gx] = True
    assert (got[~free] == -1).all()
    assert np.array_equal(got[free], d[free])      # bit equality, the unreached cells (+inf) included
    assert np.isfinite(got[free]).sum() > 0.3 * nx * ny
    for other in maps[1:]:
        assert np.array_equal(other["map"], r["map"])
    # the blocked cells are the host planner's: a disc of 0.9 x the half width
    v, A, b = H.field(sc); rad = 0.9 * min(S.EGO[1], S.EGO[3], 0.5 * (S.EGO[0] + S.EGO[2]))
    rows = np.cumsum(np.concatenate([[0], v]))
    for iy, ix in [(0, 0), (ny // 2, nx // 2), (ny - 1, nx - 1), (ny // 3, nx // 4)]:
        p = np.array([S.XYBOUNDS[0] + ix * res, S.XYBOUNDS[2] + iy * res])
        inside = any(((A[rows[j]:rows[j + 1]] @ p - b[rows[j]:rows[j + 1]]) / np.hypot(*A[rows[j]:rows[j + 1]].T)).max() <= 0 for j in range(len(v)))
        far = all(((A[rows[j]:rows[j + 1]] @ p - b[rows[j]:rows[j + 1]]) / np.hypot(*A[rows[j]:rows[j + 1]].T)).max() >= rad for j in range(len(v)))
        assert (not inside or blocked[iy, ix]) and (not far or not blocked[iy, ix])


# ---------------------------------------------------------------- 5. slot reuse
def test_slots_leave_nothing_behind():
    sc, x0, xF, kw = H.poses("backwards", 32)
    slots = 3; B = 2 * slots + 1
    batch = H.run_emu(sc, x0[:B], xF[:B], kw, slots=slots)
    assert batch["rc"] == 0 and (batch["counts"] > 0).sum() >= B - 1
    for i in range(B):
        one = H.run_emu(sc, x0[i:i + 1], xF[i:i + 1], kw, slots=1)
        for k in H.FIELDS:
            assert np.array_equal(one[k][0], batch[k][i]), (i, k)
    # a search that ended on a limit resets its cells too: the same slot plans the next instance as a fresh one does
    r = H.run_emu(sc, x0[[3, 0, 3, 1]], xF[[3, 0, 3, 1]], kw, slots=1, nodes=700)
    full = H.emu_plan("backwards", 32)
    assert r["counts"][0] == r["counts"][2] == -3
    for j, i in ((1, 0), (3, 1)):
        if full["counts"][i] > 0 and r["counts"][j] != -3:
            assert np.array_equal(r["paths"][j], full["paths"][i])


# ---------------------------------------------------------------- 6. quality: the oracle judges
def test_nlp_iterations_from_device_plans_stay_within_ten_percent_of_the_host_plans(oracle):
    """8 backwards instances at N = 30, throughput options: the same number solved, and the device plans' mean iteration count at most 1.10 x the host plans' (VERDICT's
    criterion for this feature).  At the default bucket width 0.2: 23.50 against 23.25 iterations, 8 of 8 solved from either; the test prints the figures."""
    N = 30; sc, x0, xF, kw = H.poses("backwards", 64)
    v, A, b = H.field(sc); e = H.emu_plan("backwards", 64); host = H.host_plan("backwards", 64)
    pick = [i for i in range(64) if e["counts"][i] > 0 and host[4][i] > 0][:8]
    iters = {"device": [], "host": []}; solved = {"device": 0, "host": 0}
    for i in pick:
        for name, (P_, D_) in (("device", (e["paths"][i, :e["counts"][i]], e["dirs"][i, :e["counts"][i]])), ("host", (host[2][i, :host[4][i]], host[3][i, :host[4][i]]))):
            Ts, xWS, uWS = PL.path_to_warm_start(P_, D_, N, xF[i], v_nom=0.5)
            xWS = xWS.copy(); xWS[0] = x0[i]
            r = oracle.parking_signed_dist(x0[i], xF[i], N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b, xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, uWS, opts=oracle.default_opts())
            solved[name] += int(r["exitflag"] == 1); iters[name].append(int(r["iters"]))
    md, mh = np.mean(iters["device"]), np.mean(iters["host"])
    print("oracle iterations from device plans %s (mean %.2f), from host plans %s (mean %.2f); solved %d / %d" % (iters["device"], md, iters["host"], mh, solved["device"], solved["host"]))
    assert solved["device"] == solved["host"]
    assert md <= 1.10 * mh, (md, mh)


def test_python_routes_limits_and_long_paths_per_instance(monkeypatch):
    """planner.hybrid_astar_many / warm_start_many with the device call replaced by a stand-in (no GPU here): an instance that outgrew its slot (-3) is None and its
    neighbours keep their results; a path of more than cap nodes (-1) is searched again through the DEVICE call with room for 20000 nodes, never by the host planner."""
    from obca_amd import api
    sc, x0, xF, kw = H.poses("backwards", 32); v, A, b = H.field(sc)
    e = H.emu_plan("backwards", 32); calls = []

    def fake(starts, goals, vOb, A_, b_, ego, L, XYb, opts=None, bucket_width=None, cap=1024, device=0):
        calls.append((len(starts), cap))
        idx = [int(np.flatnonzero((x0[:4, :3] == s_).all(axis=1))[0]) for s_ in starts]
        paths = np.zeros((len(idx), cap, 3)); dirs = np.zeros((len(idx), cap), np.int32); cnt = e["counts"][idx].copy()
        for j, i in enumerate(idx):
            paths[j, :cnt[j]] = e["paths"][i, :cnt[j]]; dirs[j, :cnt[j]] = e["dirs"][i, :cnt[j]]
            if i == 1:
                cnt[j] = -3; paths[j] = 0; dirs[j] = 0
            if i == 2 and cap < 20000:
                cnt[j] = -1; paths[j] = 0; dirs[j] = 0
        return paths, dirs, cnt, e["expansions"][idx].copy(), e["rounds"][idx].copy()
    monkeypatch.setattr(api, "hybrid_astar_batch", fake)
    monkeypatch.setattr(PL, "hybrid_astar", lambda *a, **k: pytest.fail("the host planner was called"))
    monkeypatch.setattr(PL, "_hybrid_astar_dense", lambda *a, **k: pytest.fail("the host planner was called"))
    many = PL.hybrid_astar_many(x0[:4], xF[:4], v, A, b, device=0, **kw)
    assert calls == [(4, 1024), (1, 20000)] and many[1] is None
    for i in (0, 2, 3):
        assert np.array_equal(many[i][0], e["paths"][i, :e["counts"][i]]) and np.array_equal(many[i][1], e["dirs"][i, :e["counts"][i]]) and many[i][2] == e["expansions"][i]
    # warm_start_many: the resampling of the batch on the device is replaced by numpy per instance here; instance 2 goes the long-path way
    def fake_ws(paths, dirs, counts, N, xF_=None, v_nom=0.5, L=S.L_WHEELBASE, smooth=False, device=0):
        B = len(counts); Ts = np.zeros(B); xWS = np.zeros((B, N + 1, 4)); uWS = np.zeros((B, N, 2)); ok = np.zeros(B, bool)
        for i in range(B):
            if counts[i] >= 2:
                Ts[i], xWS[i], uWS[i] = PL.path_to_warm_start(paths[i, :counts[i]], dirs[i, :counts[i]], N, xF_[i], v_nom=v_nom); ok[i] = True
        return Ts, xWS, uWS, ok
    monkeypatch.setattr(PL, "path_to_warm_start_many", fake_ws)
    del calls[:]
    ws = PL.warm_start_many(sc, x0[:4], xF[:4], 30, device=0, search="device")
    assert calls == [(4, 1024), (1, 20000)] and ws[1] is None
    for i in (0, 2, 3):
        Ts, xWS, uWS = PL.path_to_warm_start(e["paths"][i, :e["counts"][i]], e["dirs"][i, :e["counts"][i]], 30, xF[i], v_nom=0.5)
        assert ws[i][0] == Ts and np.array_equal(ws[i][1], xWS) and np.array_equal(ws[i][2], uWS), i


# ---------------------------------------------------------------- 7. ABI, marshalling, Julia shim, build piece
def _kinds(hdr):
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S); kinds = {}
    for m in re.finditer(r"\bint\s*(obca_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        kinds[m.group(1)] = ["ptr" if "*" in p or "[" in p else ("double" if re.match(r"\s*(const\s+)?double\b", p) else "int") for p in m.group(2).split(",")]
    return kinds


def test_header_exports_python_and_julia_agree():
    from obca_amd import api, cabi
    import obca_amd
    protos = cabi.prototypes("obca_plan_device.h")
    assert sorted(protos) == sorted(api.PLAN_DEVICE_EXPORTS) and len(protos) == 3
    assert not set(api.PLAN_DEVICE_EXPORTS) & (set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS) | set(api.REFINE_EXPORTS) | set(api.QUAD_SUBDIVIDE_EXPORTS))
    assert len(protos["obca_hybrid_astar_batch"][1]) == 20 and len(protos["obca_hybrid_configure"][1]) == 4 and len(protos["obca_hybrid_ms"][1]) == 2
    assert "obca_plan_device.h" in cabi.__doc__
    hdr = open(os.path.join(ROOT, "include", "obca_plan_device.h")).read()
    defs = {k: v for k, v in re.findall(r"#define (OBCA_HYBRID_\w+) (\S+|\(1 << 20\))", hdr)}
    assert (int(defs["OBCA_HYBRID_MAXMAP"]), int(defs["OBCA_HYBRID_MAXCELLS"]), int(defs["OBCA_HYBRID_MAXSLOTS"]), float(defs["OBCA_HYBRID_DEFAULT_WIDTH"])) == \
        (api.HYBRID_MAXMAP, api.HYBRID_MAXCELLS, api.HYBRID_MAXSLOTS, api.HYBRID_DEFAULT_WIDTH) and H.OBCA_HYBRID_MAXMAP == api.HYBRID_MAXMAP
    # the map and the bucket heads fit the 160 KiB of LDS one workgroup may use; the parallel scenario's grid fits the map
    mm, win, chunk, lds, node = (C.c_int() for _ in range(5))
    H.emu().emu_hybrid_sizes(*(C.byref(x) for x in (mm, win, chunk, lds, node)))
    assert mm.value == api.HYBRID_MAXMAP >= 301 * 91 and lds.value <= 160 * 1024 and win.value == int(defs["OBCA_HYBRID_WINDOW"]) and chunk.value == int(defs["OBCA_HYBRID_CHUNK"]) and node.value == 64
    # what the library exports (no device: the symbol table)
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {s for s in exported if "hybrid" in s} == set(api.PLAN_DEVICE_EXPORTS)
    lib = api._load()
    assert [type(a).__name__ for a in lib.obca_hybrid_astar_batch.argtypes] == [type(a).__name__ for a in protos["obca_hybrid_astar_batch"][1]]
    # marshalling: an array of another dtype is a TypeError before anything reaches the library
    z = np.zeros(3)
    with pytest.raises((TypeError, C.ArgumentError)):
        lib.obca_hybrid_astar_batch(None, 1, z, z, 0, np.zeros(1), z, z, z, 1.0, z, None, 0, 0.0, z, z, 2, z, None, None)
    for f in ("hybrid_astar_batch", "hybrid_configure", "hybrid_ms", "HYBRID_STATUS"):
        assert hasattr(obca_amd, f) and f in obca_amd.__all__
    assert sorted(obca_amd.HYBRID_STATUS) == [-3, -2, -1, 0]
    import inspect
    assert inspect.signature(PL.hybrid_astar_many).parameters["device"].default is None and inspect.signature(PL.hybrid_astar_many).parameters["bucket_width"].default is None
    assert inspect.signature(PL.warm_start_many).parameters["search"].default == "host"
    assert inspect.signature(S.make_batch).parameters["search"].default == "host" and inspect.signature(S.plan_batch).parameters["search"].default == "host"
    with pytest.raises(ValueError):
        PL.warm_start_many(S.BACKWARDS, np.zeros((1, 4)), np.zeros((1, 4)), 10, search="device")
    with pytest.raises(ValueError):
        PL.warm_start_many(S.BACKWARDS, np.zeros((1, 4)), np.zeros((1, 4)), 10, search="gpu")
    # every ccall of the shim against the header, parameter by parameter
    import test_julia_shim_cpu as J
    kinds = _kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCAPlanDevice.jl")).read()
    assert re.search(r"^const HYB = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), HYB\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
    assert {n for n, _ in calls} == set(kinds) == set(api.PLAN_DEVICE_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu")
    GXX = ["g++", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-misleading-indentation"]
    name = "hybrid_emu"
    assert name in BF.EMU_PIECES and not set(BF.EMU_PIECES) & (set(BF.PIECES) | set(BF.TEST_PIECES) | set(BF.CHECK_PIECES)) and name not in BF.DEFAULT
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_hybrid_emu.so")
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
    assert os.path.realpath(os.path.join(csrc, "obca_hybrid.h")) in seen and os.path.realpath(os.path.join(ROOT, "include", "obca_plan_device.h")) in seen
    assert os.path.realpath(os.path.join(csrc, "obca_plan_geom.h")) in seen      # the geometry and the Reeds-Shepp curves, one text with the host search
    assert os.path.realpath(os.path.join(csrc, "obca_solver.h")) not in seen      # the planner shares no text with the solve kernels
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_hybrid_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == GXX + ["-O1"] and argv[i + 2:] == [EMU + "/hybrid_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # the kernel text is included by the product library's source and by no other header
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    assert hip.count('#include "obca_hybrid.h"') == 1
    # ... as the LAST thing: the header switches fp contraction off to the end of the translation unit, so every other kernel is defined before it and only the planner's after
    before, after = hip.split('#include "obca_hybrid.h"')
    assert after.count("__global__") == 1 and "obca_hybrid_kernel" in after and "hy::" not in before and before.count("__global__") >= 10
    assert "fp contract(off)" not in before and "fp contract(off)" in open(os.path.join(csrc, "obca_hybrid.h")).read()
    for f in os.listdir(csrc):
        if f.endswith(".h") and f != "obca_hybrid.h":
            assert "obca_hybrid.h" not in open(os.path.join(csrc, f)).read(), f
    # the text both planners share is included by the host search and by the kernel text (there behind the pragma), by nothing else
    users = {f for f in os.listdir(csrc) if f.endswith((".h", ".hip", ".cpp")) and re.search(r'#[ \t]*include[ \t]*"obca_plan_geom\.h"', open(os.path.join(csrc, f)).read())}
    assert users == {"obca_planner.cpp", "obca_hybrid.h"}, users
    kernel_text = open(os.path.join(csrc, "obca_hybrid.h")).read()
    assert kernel_text.index("fp contract(off)") < kernel_text.index('#include "obca_plan_geom.h"')
