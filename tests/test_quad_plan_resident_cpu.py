"""The RESIDENT route of the quadcopter's grid planner (include/obca_quad_plan_resident.h) on a machine without a GPU: the host build of its kernel text
(tests/emu/quad_plan_resident_emu.cpp) over problem records against the host-pointer route's host build (plan3d_common.emu_warm_start / emu_paths) on "the 20" of
tests/quad_plan_resident_common.py -- 17 instances with a path, one walled off (count 0), one with a blocked start (-2), one whose end points share a node (3)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import packing as PK
import plan3d_common as K
import quad_plan_resident_common as Q
from obca_amd import planner as PL, scenarios as S

HDR = PK.QPH_SIZE
SHIPPED_COUNTS_CAP8 = {0: -1, Q.A_: 0, Q.B_: -2, Q.C_: 3}


# ---------------------------------------------------------------- 1. the warm start against the host-pointer route
@pytest.mark.parametrize("N", [1, 20, 128])
def test_records_hold_the_host_pointer_routes_warm_start(N):
    before = Q.records(N); r = Q.planned(N); xws, cnt, paths = Q.host_route(N)
    assert r["rc"] == 0, r["err"]
    assert np.array_equal(r["counts"], cnt) and cnt[Q.A_] == 0 and cnt[Q.B_] == -2 and cnt[Q.C_] == 3 and (cnt[:17] >= 36).all() and (cnt[:17] <= 61).all()
    assert Q.bits(r["paths"], paths)      # way-points, and the zeros behind them
    has = cnt >= 2
    w, t = Q.ws_of(r["prob"], N)
    assert has.sum() == 18 and Q.bits(w[has], xws[has])
    assert (w[has][:, :, 3:] == 0).all() and not Q.bits(w[has], Q.ws_of(before, N)[0][has])      # (the uploaded start was another one)
    for i in (Q.A_, Q.B_):
        assert Q.bits(r["prob"][i], before[i]), i
    assert Q.bits(r["prob"][:, :HDR], before[:, :HDR]) and (t == Q.TWS).all()      # no header word of any instance
    assert (r["sweeps"][:17] >= 33).all() and (r["sweeps"][:17] <= 50).all() and r["sweeps"][Q.B_] == 0 and r["sweeps"][Q.C_] == 0


# ---------------------------------------------------------------- 2. a cap that the shipped path does not fit
def test_cap_8():
    N = 20; before = Q.records(N); r = Q.planned(N, cap=8)
    assert r["rc"] == 0, r["err"]
    for i, c in SHIPPED_COUNTS_CAP8.items():
        assert r["counts"][i] == c, (i, r["counts"][i])
    assert (r["counts"][:17] == -1).all() and r["paths"].shape == (Q.NI, 8, 3)
    assert Q.bits(r["prob"][:19], before[:19])      # the shipped instance, and everyone else without a path that fits
    x0, xF, ob = Q.the20()
    rc, p8, c8, _ = K.emu_paths(x0[:, :3], xF[:, :3], boxes=ob, cap=8)
    assert rc == 0 and np.array_equal(c8, r["counts"]) and Q.bits(p8, r["paths"])
    w, _ = Q.ws_of(r["prob"], N)
    assert Q.bits(w[Q.C_], Q.host_route(N)[0][Q.C_])


# ---------------------------------------------------------------- 3. the time scale
def test_time_scale_only_where_a_path_is():
    N = 20; r = Q.planned(N, timeWS=1.0); base = Q.planned(N)
    has = base["counts"] >= 2
    assert r["rc"] == 0 and np.array_equal(r["counts"], base["counts"])
    assert (r["prob"][has, PK.QPH_TWS] == 1.0).all() and (r["prob"][~has, PK.QPH_TWS] == Q.TWS).all() and (base["prob"][:, PK.QPH_TWS] == Q.TWS).all()
    a = r["prob"].copy(); a[:, PK.QPH_TWS] = Q.TWS
    assert Q.bits(a, base["prob"])      # nothing else differs


# ---------------------------------------------------------------- 4. a selection
def test_selection():
    N = 20; before = Q.records(N); base = Q.planned(N); sel = [16, 0, 18]
    r = Q.plan(before, N, sel=sel, timeWS=1.0)
    assert r["rc"] == 0, r["err"]
    full = Q.planned(N, timeWS=1.0)
    others = [i for i in range(Q.NI) if i not in sel]
    assert Q.bits(r["prob"][sel], full["prob"][sel]) and Q.bits(r["paths"][sel], base["paths"][sel]) and np.array_equal(r["counts"][sel], base["counts"][sel])
    assert np.array_equal(r["sweeps"][sel], base["sweeps"][sel])
    assert Q.bits(r["prob"][others], before[others]) and (r["counts"][others] == Q.SKIPPED).all() and (r["sweeps"][others] == 0).all() and (r["paths"][others] == 0).all()


# ---------------------------------------------------------------- 5. node order, selection order, what the LDS held
def test_node_order_and_selection_order():
    N = 20; before = Q.records(N); base = Q.planned(N)
    rev = Q.plan(before, N, reverse=1, lds_fill=-1.0)
    assert rev["rc"] == 0 and Q.bits(rev["prob"], base["prob"]) and Q.bits(rev["paths"], base["paths"]) and np.array_equal(rev["counts"], base["counts"])
    assert not np.array_equal(rev["sweeps"], base["sweeps"])      # (the two orders really differ)
    perm = np.random.default_rng(5).permutation(Q.NI)
    other = Q.plan(before, N, sel=perm)
    assert other["rc"] == 0 and all(Q.bits(other[k], base[k]) for k in ("prob", "paths", "counts", "sweeps"))


# ---------------------------------------------------------------- 6. refusals, and a record that is not finite
def test_refusals_touch_nothing():
    N = 20; before = Q.records(N)[:4]
    nan = float("nan")
    cases = [(dict(cap=1), "cap"), (dict(cap=PL.PLAN3D_WS_CAP + 1), "WS_CAP"), (dict(res=0.0), "res"), (dict(res=nan), "res"), (dict(clear=float("inf")), "clear"),
             (dict(room=[10.0, -1.0, 5.0]), "room"), (dict(room=None), "room"), (dict(res=0.2), "MAXCELLS"), (dict(counts=False), "counts"),
             (dict(sel=[0, 4]), "outside"), (dict(sel=[-1]), "outside"), (dict(sel=[1, 2, 1]), "twice"), (dict(sel=[0, 1], n=0), "1 <= n"), (dict(sel=[0, 1, 2, 3], n=5), "1 <= n"),
             (dict(timeWS=0.0), "timeWS"), (dict(timeWS=-1.0), "timeWS"), (dict(timeWS=nan), "timeWS"), (dict(timeWS=float("inf")), "timeWS")]
    for kw, text in cases:
        r = Q.plan(before, N, **kw)
        assert r["rc"] == -1 and text in r["err"], (kw, r["err"])
        assert Q.bits(r["prob"], before) and (r["paths"] == 7.0).all() and (r["counts"] == 99).all() and (r["sweeps"] == 99).all(), kw


def test_a_record_that_is_not_finite_stops_its_instance_alone():
    """NaN passes every comparison of `blocked` as "not blocked": the kernel text tests the 36 numbers itself.  -2, no sweeps, the record as it was; the neighbours as without it"""
    N = 20; base = Q.planned(N)
    for word in (PK.QPH_X0 + 1, PK.QPH_XF + 2, PK.QPH_OB + 7):
        for bad in (float("nan"), float("inf"), -float("inf")):
            p = Q.records(N)[[0, Q.C_, 1]]; p[1] = Q.records(N)[0]; p[1, word] = bad; p[2] = Q.records(N)[Q.C_]
            r = Q.plan(p, N, sel=[1, 2], timeWS=1.0)
            assert r["rc"] == 0 and r["counts"].tolist() == [Q.SKIPPED, -2, 3] and r["sweeps"].tolist() == [0, 0, 0], (word, bad, r["counts"])
            assert Q.bits(r["prob"][:2], p[:2]) and (r["paths"][:2] == 0).all() and Q.bits(r["paths"][2], base["paths"][Q.C_])


# ---------------------------------------------------------------- 7. header, exports, Python, Julia, the build
def test_header_exports_python_and_julia_agree():
    import obca_amd
    from obca_amd import api, cabi
    import test_hybrid_cpu as TH
    import test_julia_shim_cpu as J
    protos = cabi.prototypes("obca_quad_plan_resident.h")
    assert sorted(protos) == sorted(api.QUAD_PLAN_RESIDENT_EXPORTS) and len(protos) == 4
    others = (set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS) | set(api.REFINE_EXPORTS) | set(api.QUAD_SUBDIVIDE_EXPORTS) | set(api.PLAN_DEVICE_EXPORTS)
              | set(api.SCENE_EXPORTS) | set(api.PLAN_RESIDENT_EXPORTS) | set(api.PLAN_RESIDENT_CHECK_EXPORTS) | set(PL.PLAN3D_EXPORTS))
    assert not set(api.QUAD_PLAN_RESIDENT_EXPORTS) & others
    assert [len(protos[n][1]) for n in api.QUAD_PLAN_RESIDENT_EXPORTS] == [10, 2, 3, 3] and "obca_quad_plan_resident.h" in cabi.__doc__
    # no name of the header falls under a filter by which an older test picks ITS entry points out of the library's symbols
    assert not any(w in s for s in api.QUAD_PLAN_RESIDENT_EXPORTS for w in ("batch_plan", "hybrid", "scene", "refine", "subdivide", "clearance", "plan3d"))
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert set(api.QUAD_PLAN_RESIDENT_EXPORTS) <= exported and {s for s in exported if "grid_plan" in s or "start_download" in s} == set(api.QUAD_PLAN_RESIDENT_EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "obca_quad_plan_resident.h")).read()
    assert int(re.search(r"#define OBCA_QUAD_PLAN_SKIPPED \((-?\d+)\)", hdr).group(1)) == api.QUAD_PLAN_SKIPPED == Q.SKIPPED == -4 and sorted(api.QUAD_PLAN_STATUS) == [-4, -3, -2, -1, 0]
    lay = np.zeros(11, np.int32); Q.emu().emu_qpr_layout(lay.ctypes.data_as(Q.I))
    assert lay.tolist() == [PK.QPH_TS, PK.QPH_R, PK.QPH_X0, PK.QPH_XF, PK.QPH_OB, PK.QPH_TWS, PK.QPH_DWS, PK.QPH_DIST, PK.QPH_SIZE, -4, 1024]
    lib = api._load()
    assert [type(a).__name__ for a in lib.obca_quad_batch_grid_plan_warm_start.argtypes] == [type(a).__name__ for a in protos["obca_quad_batch_grid_plan_warm_start"][1]]
    assert lib.obca_quad_batch_grid_plan_ms.argtypes[1] is C.POINTER(C.c_float)
    i1 = np.zeros(1, np.int32); f = C.c_float(0); room = np.array(PL.QUAD_ROOM, float)
    with pytest.raises((TypeError, C.ArgumentError)):      # counts as float64
        lib.obca_quad_batch_grid_plan_warm_start(None, 0.4, room, 0.25, 1024, None, 0, None, np.zeros(1), None)
    # no batch: refused before anything else, no device touched
    assert lib.obca_quad_batch_grid_plan_warm_start(None, 0.4, room, 0.25, 1024, None, 0, None, i1, None) == -1
    assert lib.obca_quad_batch_grid_plan_ms(None, C.byref(f)) == -1 and lib.obca_quad_batch_grid_plan_download(None, None, 0) == -1
    assert lib.obca_quad_batch_start_download(None, np.zeros(1), np.zeros(1)) == -1
    for m in ("plan_warm_start", "plan_ms", "plan_paths", "warm_start"):
        assert callable(getattr(obca_amd.QuadBatch, m))
    assert "QuadBatch" in obca_amd.__all__ and "QUAD_PLAN_STATUS" in obca_amd.__all__
    sig = inspect.signature(api.QuadBatch.plan_warm_start).parameters
    assert list(sig) == ["self", "clear", "room", "res", "cap", "select", "timeWS"]
    many = inspect.signature(PL.quad_warm_start_many).parameters      # the two routes are comparable bit for bit: the same defaults
    assert all(sig[k].default == many[k].default for k in ("clear", "room", "res")) and sig["room"].default == PL.QUAD_ROOM and sig["cap"].default == PL.PLAN3D_WS_CAP
    assert sig["select"].default is None and sig["timeWS"].default is None
    # the two scenario functions keep their signatures
    assert list(inspect.signature(S.make_quad_batch).parameters) == ["B", "N", "seed", "jitter", "random_endpoints", "device"]
    assert list(inspect.signature(S.plan_quad_batch).parameters) == ["x0", "xF", "N", "rng", "first_is_fixed", "device"]
    # every ccall of the shim against the header, parameter by parameter
    kinds = TH._kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCAQuadPlanResident.jl")).read()
    assert re.search(r"^const QPR = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), QPR\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
        assert m.group(2) == "Cint"
    assert {n for n, _ in calls} == set(kinds) == set(api.QUAD_PLAN_RESIDENT_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])
    assert src.count("ccall(") == len(calls) + 1 and "ccall((:obca_last_error, LIB)" in src      # (+ the error text)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()      # the call sequence upload -> plan -> solve
    assert doc.index("obca_quad_batch_upload(bt,") < doc.index("obca_quad_batch_grid_plan_warm_start(bt,") < doc.index("obca_quad_batch_solve(bt, NULL); obca_quad_batch_download")


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu")
    name = "quad_plan_resident_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_quad_plan_resident_emu.so")
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
    for h in (os.path.join(csrc, "obca_quad_plan_resident.h"), os.path.join(csrc, "obca_plan3d.h"), os.path.join(csrc, "obca_quad_solver.h"),
              os.path.join(ROOT, "include", "obca_quad_plan_resident.h"), os.path.join(ROOT, "include", "obca_plan3d.h")):
        assert os.path.realpath(h) in seen, h
    assert os.path.realpath(os.path.join(csrc, "obca_hybrid.h")) not in seen      # the quadcopter's planner shares no text with the parking planner
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_quad_plan_resident_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/quad_plan_resident_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # the kernel text comes where fp contraction is already off in the product's source: behind the parking planner's text, which is behind every solver kernel
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    after = hip.split('#include "obca_hybrid.h"')[1]
    assert after.count('#include "obca_quad_plan_resident.h"') == 1 and hip.count('#include "obca_quad_plan_resident.h"') == 1
    for k in ("obca_parking_ipm_kernel", "obca_quad_ipm_kernel"):
        assert k in hip.split('#include "obca_hybrid.h"')[0]
    txt = open(os.path.join(csrc, "obca_quad_plan_resident.h")).read()
    assert "__global__ __launch_bounds__(PL3_NT) void obca_quad_plan_resident_kernel(" in txt and txt.count("pl3::plan_instance(") == 1
    code = re.sub(r"//.*", "", txt)
    assert "fma" not in code and "atomic" not in code and "relax_node" not in code and "best_step" not in code      # one search: the reused one
    # the one kernel of the host-pointer library still reads its record in one piece
    assert "pl3::plan_instance(in + i * PL3_IN_STRIDE(nBox), G," in open(os.path.join(csrc, "obca_plan3d.hip")).read()


def test_device_source_compiles_for_gfx950_without_a_warning():
    from obca_amd.buildflags import HIPCC
    base = [f for f in HIPCC if f not in ("-shared", "-fPIC")] + ["-fsyntax-only", "-Wno-unused-command-line-argument"]
    for src in ("obca_hip.hip", "obca_plan3d.hip"):
        r = subprocess.run(base + [os.path.join(ROOT, "obca_amd", "csrc", src)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stdout.strip() and not r.stderr.strip(), (src, r.stdout[-2000:], r.stderr[-2000:])
