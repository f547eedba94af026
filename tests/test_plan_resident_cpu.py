"""The RESIDENT route of the parking planner (include/obca_plan_resident.h) on a machine without a GPU: the host build of its kernel text and of the two kernels behind
it (tests/emu/plan_resident_emu.cpp) against the host-pointer route's host code -- hy::make_fields / make_params for the packing, scenes_common.run_scenes for the search,
emu_path_ws_record for the warm start.

The inputs (plan_resident_common.scenes16): the first 16 of scenes_common.scenes() -- the backwards field plus 1-3 boxes, 4-6 obstacles with 2, 2, 1, 4, ... rows, all
axis-parallel: hypot is exactly 1 and a / 1 = a, so the record's unit rows ARE the caller's rows and the two routes must agree bit for bit.  N = 30, hybrid_common.NODES
nodes per slot."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import hybrid_common as H
import packing as PK
import plan_resident_common as R
import scenes_common as SC
from obca_amd import planner as PL, scenarios as S

FIELD_KEYS = ("v", "off", "voff", "A", "b", "rn", "nrm", "vert")


def _bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_fields(x0, xF, fields, what):
    """the packed block of the records against hy::make_fields of the same unit rows, instance by instance (the strides differ), in the three loop orders"""
    B = len(fields)
    prob, _, nObMax, MMax = R.records(x0, xF, fields)
    host = R.host_fields(x0, xF, [R.unit(f) for f in fields])
    blocks = [R.pack_block(prob, nObMax, MMax, order) for order in (0, 1, 2)]
    assert blocks[0].tobytes() == blocks[1].tobytes() == blocks[2].tobytes(), what
    mine = R.views(blocks[0], B, nObMax, MMax)
    _, nv = R.layout(B, nObMax, MMax)
    assert nv >= 4 + PK.OB_VMAX
    for i in range(B):
        assert mine["rec"][4 * i:4 * i + 4].tolist() == [i * nObMax, i * MMax, i * nObMax * nv, len(fields[i][0])], (what, i)
        a, b = R.field_of(mine, i), R.field_of(host, i)
        for k in FIELD_KEYS:
            assert _bits(a[k], b[k]), (what, i, k, a[k], b[k])
        assert (a["rn"] == 1.0).all() and (a["nrm"] == 1.0).all() and a["v"].tolist() == list(fields[i][0])
    assert _bits(mine["inst"], host["inst"]), what
    return mine


# ---------------------------------------------------------------- 1. packing against the host
def test_packed_fields_equal_make_fields_bit_for_bit():
    x0, xF, kw, fields = R.scenes16()
    assert sorted({len(f[0]) for f in fields}) == [4, 5, 6] and all(list(f[0][:3]) == [2, 2, 1] and (np.asarray(f[0][3:]) == 4).all() for f in fields)
    mine = _same_fields(x0, xF, fields, "16 scenes")
    # the 1-row obstacle is an unbounded half-plane cut from the far square: a quadrilateral with vertices about 1e3 m out
    f0 = R.field_of(mine, 0)
    one = f0["vert"][2 * f0["voff"][2]:2 * f0["voff"][3]].reshape(-1, 2)
    assert f0["v"][2] == 1 and len(one) == 4 and np.abs(one).max() > 1e3
    inst = mine["inst"].reshape(-1, 10)
    assert _bits(inst[:, :3], x0[:, :3]) and _bits(inst[:, 5:8], xF[:, :3]) and _bits(inst[:, 3], np.sin(x0[:, 2])) and _bits(inst[:, 9], np.cos(xF[:, 2]))


def test_sixteen_obstacles_and_64_rows_beside_one_obstacle():
    """the limits of a record: 16 boxes of 4 rows fill every obstacle slot and every row of the header; its neighbour has one obstacle of one row, so the strides of the
    block (16 obstacles, 64 rows) are far from what the neighbour uses"""
    x0, xF, _, _ = R.scenes16()
    lOb = []
    for k in range(16):
        cx, cy, h = -13.0 + 1.7 * k, 6.0 + 0.25 * (k % 5), 0.3 + 0.03 * k
        pts = [[cx - h, cy + h], [cx + h, cy + h], [cx + h, cy - h], [cx - h, cy - h]]
        lOb.append(pts + [pts[0]])
    A, b = S.obst_hrep(16, [5] * 16, lOb)
    big = (np.full(16, 4, np.int32), A, b)
    small = (np.array([1], np.int32), np.array([[0.0, -1.0]]), np.array([-11.0]))      # the road's upper edge: y >= 11
    assert int(big[0].sum()) == PK.OB_MMAX and len(big[0]) == PK.OB_NOBMAX
    mine = _same_fields(x0[:3], xF[:3], [small, big, small], "16 x 4 rows beside 1 x 1")
    assert R.field_of(mine, 1)["voff"].tolist() == list(range(0, 65, 4)) and R.field_of(mine, 0)["voff"].tolist() == [0, 4]


# ---------------------------------------------------------------- 2. rows that are not unit on input
def _turned_box(cx, cy, half=0.4, angle=0.3):
    c, s = np.cos(angle), np.sin(angle)
    pts = [[cx + c * dx - s * dy, cy + s * dx + c * dy] for dx, dy in ((-half, half), (half, half), (half, -half), (-half, -half))]      # clockwise
    return S.obst_hrep(1, [5], [pts + [pts[0]]])


def test_turned_boxes_are_planned_on_the_records_unit_rows():
    """A box turned by 0.3 rad has rows [-s 1] of length sqrt(1 + s^2): the record holds a / |a|, whose own length is 1 +- rounding, and the packing takes those rows with
    rn = nrm = 1.  No bit comparison with the host-pointer route here: given the same rows that route computes hypot(a) -- 1 to within an ulp, not 1 -- and divides by it, so
    its blocked cells and depths may differ from the device's in the last bit, and which of the two is `right` is not defined.  What must hold: every planned path is valid
    in the instance's field by the host planner's own collision test."""
    x0, xF, kw, fields = R.scenes16()
    n = 6; fl = []
    for i in range(n):
        for cx, cy in ((9.5, 9.2), (-9.5, 9.2), (6.5, 9.4), (-6.5, 9.4)):
            A1, b1 = _turned_box(cx, cy)
            if not PL.collides(x0[i, :3], np.array([4]), A1, b1, margin=0.5):      # (the start pose stays clear, as scenarios.scene_field keeps it)
                break
        else:
            raise AssertionError("no place for the turned box in scene %d" % i)
        fl.append(SC.with_box(fields[i], A1, b1))
        lens = PK.row_lengths(A1)
        assert (np.abs(lens - 1.0) > 1e-3).any()      # not unit on input
    prob, z0, nObMax, MMax = R.records(x0[:n], xF[:n], fl)
    mine = R.views(R.pack_block(prob, nObMax, MMax), n, nObMax, MMax)
    for i in range(n):
        f = R.field_of(mine, i)
        assert (f["nrm"] == 1.0).all() and (f["rn"] == 1.0).all() and np.abs(np.hypot(f["A"][0::2], f["A"][1::2]) - 1.0).max() <= 2.3e-16
        assert _bits(f["A"], R.unit(fl[i])[1].ravel()) and _bits(f["b"], R.unit(fl[i])[2])
    r = R.plan(prob, z0, nObMax, MMax, kw)
    assert r["rc"] == 0, r["err"]
    margin = PL.DEFAULT_OPTS["margin"]
    for i in range(n):
        c = r["counts"][i]
        assert c >= 2 and r["status"][i] == 0, (i, c)
        SC.check_path_in(fl[i], x0[i], xF[i], r["paths"][i, :c], r["dirs"][i, :c], margin, what="turned box, scene %d" % i)


# ---------------------------------------------------------------- 3. the whole route
@pytest.mark.parametrize("analytic", [None, 0.0])
def test_route_equals_the_host_pointer_route_and_the_path_warm_start(analytic):
    x0, xF, kw, fields = R.scenes16()
    mine = R.plan16(analytic); ref = R.host16(analytic)
    assert mine["rc"] == 0 and ref["rc"] == 0, (mine["err"], ref["err"])
    assert H.same(mine, ref) and (mine["counts"] >= 2).all()
    for order in (1, 2):
        other = R.plan16(analytic, order)
        assert H.same(other, mine) and _bits(other["prob"], mine["prob"]) and _bits(other["z0"], mine["z0"]) and np.array_equal(other["status"], mine["status"])
    prob, z0, _, _ = R.records(x0, xF, fields)
    assert (mine["status"] == 0).all()
    for i in range(R.NS):
        st, p, z = R.path_ws_record(prob[i], z0[i], mine["paths"][i], mine["dirs"][i], mine["counts"][i])
        assert st == 0 and _bits(p, mine["prob"][i]) and _bits(z, mine["z0"][i]), i
        assert not _bits(z0[i], mine["z0"][i]) and mine["prob"][i][PK.PH["TS"]] != R.TS


def test_an_ulp_on_every_sine_and_cosine_changes_no_count():
    """The condition of the GPU test's cap (at most one of the 16 may differ from the host-pointer route with the analytic expansion on): the device's sines and cosines of
    the poses differ from the host's by an ulp or two, so the host build is run with every one of them moved by +-1 ulp, in the four sign patterns -- no count of these 16
    scenes changes, the scenes stand as the issue lists them."""
    x0, xF, kw, fields = R.scenes16(); base = R.plan16()
    prob, z0, nObMax, MMax = R.records(x0, xF, fields)
    for ds, dc in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        inst = base["inst"].copy()
        for col, d in ((3, ds), (4, dc), (8, ds), (9, dc)):
            inst[:, col] = np.nextafter(inst[:, col], d * np.inf)
        r = R.plan(prob, z0, nObMax, MMax, kw, inst=inst)
        assert r["rc"] == 0 and np.array_equal(r["counts"], base["counts"]), (ds, dc, r["counts"], base["counts"])


def test_a_blocked_start_and_a_closed_mouth_stop_their_instances_alone():
    """Scene A (instance 5): a box over its start pose -- counts -2, a negative status, the uploaded record and start unchanged to the last bit.  Scene B (instance 3): a box
    across the slot's mouth from y = 5.2 (test_scenes_cpu.py: the goal stays free, nothing gets through) -- counts 0, status -1.  Everyone else: as without the two."""
    x0, xF, kw, fields = R.scenes16(); base = R.plan16()
    fl = list(fields)
    fl[5] = SC.with_box(fields[5], *SC.box_over(x0[5]))
    pts = [[-1.3, 6.5], [1.3, 6.5], [1.3, 5.2], [-1.3, 5.2]]
    fl[3] = SC.with_box(fields[3], *S.obst_hrep(1, [5], [pts + [pts[0]]]))
    prob, z0, nObMax, MMax = R.records(x0, xF, fl)
    r = R.plan(prob, z0, nObMax, MMax, kw)
    assert r["rc"] == 0, r["err"]
    assert r["counts"][5] == -2 and r["status"][5] < 0 and r["expansions"][5] == 0 and _bits(r["prob"][5], prob[5]) and _bits(r["z0"][5], z0[5])
    assert r["counts"][3] == 0 and r["status"][3] == -1 and r["expansions"][3] > 1000 and _bits(r["prob"][3], prob[3]) and _bits(r["z0"][3], z0[3])
    others = [i for i in range(R.NS) if i not in (3, 5)]
    assert all(np.array_equal(r[k][others], base[k][others]) for k in H.FIELDS + ("status",))
    # (the neighbours' rows moved in the block -- MMax grew by the boxes' rows --, their records did not)
    z_base, z_r = base["z0"][others], r["z0"][others]
    lx = PK.layout(R.N, 0, 0)["lam"]
    assert _bits(z_r[:, :lx], z_base[:, :lx]) and _bits(r["prob"][others][:, PK.OB_HDR:], base["prob"][others][:, PK.OB_HDR:])


# ---------------------------------------------------------------- 4. header, exports, Python, Julia
def test_header_exports_python_and_julia_agree():
    import inspect
    import obca_amd
    from obca_amd import api, cabi
    import test_hybrid_cpu as TH
    protos = cabi.prototypes("obca_plan_resident.h")
    assert sorted(protos) == sorted(api.PLAN_RESIDENT_EXPORTS) and len(protos) == 3
    others = (set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS) | set(api.REFINE_EXPORTS) | set(api.QUAD_SUBDIVIDE_EXPORTS) | set(api.PLAN_DEVICE_EXPORTS)
              | set(api.SCENE_EXPORTS) | set(PL.PLAN3D_EXPORTS))
    assert not set(api.PLAN_RESIDENT_EXPORTS) & others
    assert [len(protos[n][1]) for n in ("obca_batch_plan_warm_start", "obca_batch_plan_ms", "obca_batch_plan_download")] == [12, 4, 5]
    assert "obca_plan_resident.h" in cabi.__doc__
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {s for s in exported if "batch_plan" in s} == set(api.PLAN_RESIDENT_EXPORTS) and set(api.PLAN_RESIDENT_EXPORTS) <= exported
    assert not any(w in s for s in api.PLAN_RESIDENT_EXPORTS for w in ("hybrid", "scene", "refine", "subdivide", "clearance"))
    lib = api._load()
    assert [type(a).__name__ for a in lib.obca_batch_plan_warm_start.argtypes] == [type(a).__name__ for a in protos["obca_batch_plan_warm_start"][1]]
    assert lib.obca_batch_plan_ms.argtypes[1] is C.POINTER(C.c_float)
    i1 = np.zeros(1, np.int32); f = C.c_float(0)
    with pytest.raises((TypeError, C.ArgumentError)):      # counts as float64
        lib.obca_batch_plan_warm_start(None, None, 0, 0.0, 1024, 1, 0.5, 0.0, np.zeros(1), i1, None, None)
    # no batch: refused before anything else, no device touched
    assert lib.obca_batch_plan_warm_start(None, None, 0, 0.0, 1024, 1, 0.5, 0.0, i1, i1, None, None) == -1
    assert lib.obca_batch_plan_ms(None, C.byref(f), C.byref(f), C.byref(f)) == -1
    assert lib.obca_batch_plan_download(None, None, None, 1024, np.zeros(10)) == -1
    # the diagnostic that hands out the packed block: a header and a list of its own, a name none of the filters of the older tests catches
    chk = cabi.prototypes("obca_plan_resident_check.h")
    assert sorted(chk) == sorted(api.PLAN_RESIDENT_CHECK_EXPORTS) == ["obca_batch_packed_block"] and len(chk["obca_batch_packed_block"][1]) == 4 and "obca_plan_resident_check.h" in cabi.__doc__
    assert set(chk) <= exported and not set(chk) & (others | set(api.PLAN_RESIDENT_EXPORTS))
    assert not any(w in "obca_batch_packed_block" for w in ("batch_plan", "hybrid", "scene", "refine", "subdivide", "clearance", "debug"))
    assert lib.obca_batch_packed_block(None, None, 0, np.zeros(6, np.int32)) == -1
    for m in ("plan_warm_start", "plan_ms", "plan_paths", "plan_block"):
        assert callable(getattr(obca_amd.Batch, m))
    assert "Batch" in obca_amd.__all__
    sig = inspect.signature(api.Batch.plan_warm_start).parameters
    assert list(sig) == ["self", "bucket_width", "cap", "v_nom", "smooth", "use_xF", "planner_options"] and sig["planner_options"].kind is inspect.Parameter.VAR_KEYWORD
    assert sig["bucket_width"].default is None and sig["cap"].default == 1024 and sig["v_nom"].default == 0.5 and sig["smooth"].default is False and sig["use_xF"].default is True
    assert sig["cap"].default <= api.PATH_WS_MAXNODES
    # every ccall of the shim against the header, parameter by parameter
    import test_julia_shim_cpu as J
    kinds = TH._kinds(open(os.path.join(ROOT, "include", "obca_plan_resident.h")).read())
    src = open(os.path.join(ROOT, "julia", "OBCAPlanResident.jl")).read()
    assert re.search(r"^const PLR = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), PLR\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
    assert {n for n, _ in calls} == set(kinds) == set(api.PLAN_RESIDENT_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])
    # the new entry points hang on no constant the older shim test reads against obca_hip.h / obca_plan.h
    assert not re.search(r"ccall\(\(:obca_batch_plan\w*, (LIB|PLAN)\)", src)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()      # the call sequence upload -> plan -> solve
    assert doc.index("obca_batch_upload(bt,") < doc.index("obca_batch_plan_warm_start(bt,") < doc.index("obca_batch_solve(bt, NULL); obca_batch_download")


def test_a_given_block_stands_in_for_the_packing_and_is_checked():
    """the host build's second entry: the search over a packed block GIVEN by the caller (on a GPU machine: the device's own) -- the block of emu_plr_pack gives the route's
    own results; a block whose offsets leave it is refused"""
    x0, xF, kw, fields = R.scenes16(); base = R.plan16()
    prob, z0, nObMax, MMax = R.records(x0, xF, fields)
    block = R.pack_block(prob, nObMax, MMax, order=2)
    r = R.plan(prob, z0, nObMax, MMax, kw, block=block)
    assert r["rc"] == 0 and H.same(r, base) and np.array_equal(r["status"], base["status"]) and _bits(r["z0"], base["z0"]) and _bits(r["inst"], base["inst"])
    bad = block.copy(); R.views(bad, R.NS, nObMax, MMax)["voff"][3] = 10 ** 6
    r = R.plan(prob, z0, nObMax, MMax, kw, block=bad)
    assert r["rc"] == -1 and "leave the block" in r["err"] and (r["counts"] == 99).all()


def test_the_host_build_refuses_what_the_library_refuses():
    """the argument checks the two builds share (cap, the option checks of make_params, the warm start's numbers): -1 with a message, nothing written"""
    x0, xF, kw, fields = R.scenes16()
    prob, z0, nObMax, MMax = R.records(x0[:2], xF[:2], fields[:2])
    for bad, text in ((dict(cap=1), "cap"), (dict(cap=1025), "cap"), (dict(v_nom=0.0), "v_nom"), (dict(a_max=-1.0), "a_max"), (dict(kw=dict(kw, nh_res=1.0)), "lattice"),
                      (dict(kw=dict(kw, xy_res=0.0)), "out of range"), (dict(kw=dict(kw, reverse_cost=-1.0)), "negative"), (dict(bw=1e-9), "bucket_width")):
        r = R.plan(prob, z0, nObMax, MMax, **{"kw": kw, **bad})
        assert r["rc"] == -1 and text in r["err"], (bad, r["err"])
        assert (r["counts"] == 99).all() and _bits(r["prob"], prob) and _bits(r["z0"], z0)


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu")
    name = "plan_resident_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_plan_resident_emu.so")
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
    for h in ("obca_plan_resident.h", "obca_hybrid.h", "obca_plan_geom.h", "obca_path_ws.h"):
        assert os.path.realpath(os.path.join(csrc, h)) in seen, h
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_plan_resident_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/plan_resident_emu.cpp"]
    # the kernel text comes behind the planner's in the product's source (its contraction rule, its names)
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    after = hip.split('#include "obca_hybrid.h"')[1]
    assert after.count('#include "obca_plan_resident.h"') == 1 and hip.count('#include "obca_plan_resident.h"') == 1


# ---------------------------------------------------------------- 5. the device source
def test_device_source_compiles_for_gfx950_without_a_warning():
    from obca_amd.buildflags import HIPCC
    base = [f for f in HIPCC if f not in ("-shared", "-fPIC")] + ["-fsyntax-only", "-Wno-unused-command-line-argument"]
    r = subprocess.run(base + [os.path.join(ROOT, "obca_amd", "csrc", "obca_hip.hip")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stdout.strip() and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-2000:])
    txt = open(os.path.join(ROOT, "obca_amd", "csrc", "obca_plan_resident.h")).read()
    assert "__global__ __launch_bounds__(PLR_NT) void obca_plan_pack_kernel(" in txt and txt.count("sin(") == 1 and txt.count("cos(") == 1
    assert "hypot" not in re.sub(r"//.*", "", txt)
