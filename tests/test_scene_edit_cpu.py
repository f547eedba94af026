"""The obstacles of a resident batch moved and inflated in place, without a GPU: the kernel text of obca_amd/csrc/obca_scene_edit.h compiled for the host
(tests/emu/scene_edit_emu.cpp) against the numpy statement (validate.move_obstacles_parking / move_obstacles_quad) on a ragged batch at both limits of the header, in both lane
orders; identity, translation and round trip; the moved H-rep against polygons whose VERTICES were moved with plain numpy, through the exact distance of
tests/polygon_distance.py; inflation; the quadcopter's boxes; the public surface, the build rule and the Julia shim.  None of these needs a solve.
tests/scene_edit_common.py has the batch and the tolerances."""
import inspect
import os
import re
import subprocess
import ctypes as C
import numpy as np
import pytest
from conftest import ROOT, golden
import packing as P
import polygon_distance as PD
import scene_edit_common as E
from obca_amd import validate as V

TOL_D = 2e-8      # tests/test_dualws_geometry_cpu.py: the duality gap DualMultWS leaves, at every distance
ULP = np.finfo(float).eps


# ---------------------------------------------------------------- 1. the ragged batch at both limits
def test_ragged_batch_matches_numpy_and_a_bad_instance_keeps_every_bit():
    """Five instances at N = 6 -- 1 x 3 rows; 16 x 4 rows (the obstacle limit and the 64-row limit together); 8 + 3 rows; the shipped scene as 3 x 4 rows, twice, the second
    with one NaN in its motion -- moved by a seeded general motion with pivots and inflation.  Host build against the numpy statement within 3.1e-10 max(1, |value|); measured
    on x86-64 (g++ -O1, glibc; numpy's own sine and cosine): 0, the bits agree.  The lane order changes no bit.  The NaN instance: status 1, every bit kept.  Row norms within
    4 ulp of 1.  No word outside the rows in use of PH_A / PH_B changes: counts, offsets, every other header word, the reference rows, the pattern behind the records."""
    bt = E.ragged_batch(); prob = E.pack_ragged(bt, s_prob=P.OB_HDR + 3 * (bt["N"] + 1) + 5)
    nObs = prob[:, P.PH["NOB"]].astype(int); Ms = prob[:, P.PH["M"]].astype(int)
    assert nObs.tolist() == [1, 16, 2, 3, 3] and Ms.tolist() == [3, 64, 11, 12, 12] and prob[1, P.PH["VOB"]:P.PH["VOB"] + 16].tolist() == [4.0] * 16 and prob[2, P.PH["VOB"]] == 8
    motion, pivot, inflate = E.ragged_motion()
    ref, rst = E.numpy_move_parking(prob, motion, pivot, inflate)
    runs = [E.emu_move_parking(prob, motion, pivot, inflate, rev=rev) for rev in (0, 1)]
    assert E.same(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    out, st = runs[0]
    assert st.tolist() == rst.tolist() == [0, 0, 0, 0, 1]
    assert E.same(out[4], prob[4]) and E.same(ref[4], prob[4])
    w = E.worst(out, ref); print("host build against numpy, ragged batch: %.3g" % w)
    assert w <= E.TOL_HOST
    mask = E.obstacle_mask(prob)
    assert E.same(out[~mask], prob[~mask])
    assert not E.same(out[:4][mask[:4]], prob[:4][mask[:4]])
    A, b, v = E.rows_of(out)
    assert np.abs(np.hypot(A[:, 0], A[:, 1]) - 1.0).max() <= 4 * ULP
    # a start iterate beside the records is not an argument of the kernel at all: the instance function takes the record, the motions and the status word
    sig = re.search(r"OBCA_FN void move_parking_instance\(([^)]*)\)", open(os.path.join(ROOT, "obca_amd", "csrc", "obca_scene_edit.h")).read()).group(1)
    assert [s.strip().split()[-1].lstrip("*") for s in sig.split(",")] == ["prob", "in", "rev", "status"]


def test_every_bad_input_marks_its_instance_alone():
    bt = E.ragged_batch(); prob = E.pack_ragged(bt); good = E.ragged_motion(nan=False)
    whole, st0 = E.emu_move_parking(prob, *good)
    assert st0.tolist() == [0] * 5
    for which, row, col, val in ((0, 0, 2, np.inf), (0, 16, 0, np.nan), (1, 17, 1, -np.inf), (2, 19, None, np.nan), (0, 20, 1, 1e308), (2, 3, None, np.inf)):
        args = [a.copy() for a in good]
        if col is None:
            args[which][row] = val
        else:
            args[which][row, col] = val
        hit = int(np.searchsorted(np.cumsum([1, 16, 2, 3, 3]), row, side="right"))
        if val == 1e308:      # a finite motion with a result that is not: b' overflows
            args[0][row, 0] = 1e308; args[1][row] = (1e308, 1e308)
        for rev in (0, 1):
            out, st = E.emu_move_parking(prob, *args, rev=rev)
            r2, s2 = E.numpy_move_parking(prob, *args)
            assert st.tolist() == s2.tolist() == [int(i == hit) for i in range(5)], (which, row, col, st, s2)
            assert E.same(out[hit], prob[hit]) and all(E.same(out[i], whole[i]) for i in range(5) if i != hit)


def test_an_instance_without_obstacles_has_nothing_to_move():
    """(host build only: a resident parking batch cannot hold such an instance) no row, no obstacle: status 0 and every bit kept, in both lane orders, beside a neighbour
    that moves"""
    bt = E.ragged_batch(); prob = E.pack_ragged(bt)[[0, 3]]
    prob[0, P.PH["NOB"]] = prob[0, P.PH["M"]] = 0; prob[0, P.PH["VOB"]] = 0; prob[0, P.PH["ROFF"] + 1] = 0
    motion = np.tile([0.3, -0.2, 0.4], (3, 1)); whole, _ = E.emu_move_parking(E.pack_ragged(bt)[[3]], motion, None, np.full(3, 0.1))
    for rev in (0, 1):
        out, st = E.emu_move_parking(prob, motion, None, np.full(3, 0.1), rev=rev)
        assert st.tolist() == [0, 0] and E.same(out[0], prob[0]) and E.same(out[1], whole[0]) and not E.same(out[1], prob[1])


# ---------------------------------------------------------------- 2. identity and translation
def test_identity_changes_no_bit_and_a_translation_no_bit_of_A():
    bt = E.ragged_batch(); prob = E.pack_ragged(bt); nt = 25
    prob[3, P.PH["B"] + 1] = -0.0      # (x + 0.0 would turn this word into +0.0)
    for args in ((None, None, None), (np.zeros((nt, 3)), None, None), (np.zeros((nt, 3)), np.ones((nt, 2)), np.zeros(nt)), (None, np.full((nt, 2), 3.5), None), (None, None, np.zeros(nt))):
        for rev in (0, 1):
            out, st = E.emu_move_parking(prob, *args, rev=rev)
            assert E.same(out, prob) and not st.any()
        assert E.same(E.numpy_move_parking(prob, *args)[0], prob)
    motion, pivot, inflate = E.ragged_motion(nan=False); motion[:, 2] = 0.0
    out, st = E.emu_move_parking(prob, motion, pivot, None)
    a = slice(P.PH["A"], P.PH["A"] + 2 * P.OB_MMAX); bw = slice(P.PH["B"], P.PH["B"] + P.OB_MMAX)
    assert not st.any() and E.same(out[:, a], prob[:, a]) and not E.same(out[:, bw], prob[:, bw])
    assert E.worst(out, E.numpy_move_parking(prob, motion, pivot, None)[0]) == 0.0
    # the translation is b += a.d, whatever the pivot
    A, b, v = E.rows_of(prob); A2, b2, _ = E.rows_of(out); d = np.repeat(motion[:, :2], v, axis=0)
    assert np.abs(b2 - (b + (A * d).sum(axis=1))).max() <= 1e-13


# ---------------------------------------------------------------- 3. round trip
def test_a_motion_and_its_inverse_return_the_scene():
    """metre-scale scenes, pivots within 3 m: |A - A''| and |b - b''| <= 1e-12 (measured: 1.1e-16 and 3.6e-15)"""
    bt = E.ragged_batch(); prob = E.pack_ragged(bt); motion, pivot, inflate = E.ragged_motion(nan=False)
    out, st = E.emu_move_parking(prob, motion, pivot, inflate)
    inv, minf = E.inverse_motion(motion, inflate)
    back, st2 = E.emu_move_parking(out, inv, pivot, minf)
    assert not st.any() and not st2.any()
    A, b, _ = E.rows_of(prob); A2, b2, _ = E.rows_of(back)
    print("round trip: A %.3g, b %.3g" % (np.abs(A - A2).max(), np.abs(b - b2).max()))
    assert np.abs(A - A2).max() <= 1e-12 and np.abs(b - b2).max() <= 1e-12


# ---------------------------------------------------------------- 4. against geometry that shares no code with the kernel
def _one_obstacle_record(A, b):
    return P.pack_problem(np.zeros(4), np.zeros(4), 2, 0.5, 2.7, [3.7, 1, 1, 1], [-100, 100, -100, 100], [len(b)], A, b, np.zeros(3), np.zeros(3), np.zeros(3), 0)[None, :]


def _host_distance(emu, pose, ego, A, b):
    """dualws_one<8> of the kernel text on unit rows (tests/test_dualws_geometry_cpu.py: run_host_build)"""
    g, off = PD.car_geometry(ego); X, Y, psi = pose; cs, sn = np.cos(psi), np.sin(psi); lam = np.zeros(8); mu = np.zeros(4); d = C.c_double(0)
    a1 = np.ascontiguousarray(A[:, 0]); a2 = np.ascontiguousarray(A[:, 1]); bj = np.ascontiguousarray(b)
    emu.emu_dualws(C.c_int(len(b)), E.dp(a1), E.dp(a2), E.dp(bj), E.dp(g), C.c_double(X + off * cs), C.c_double(Y + off * sn), C.c_double(cs), C.c_double(sn), E.dp(lam), E.dp(mu), C.byref(d))
    return d.value


def test_moved_rows_against_moved_vertices(emu):
    """Polygons of tests/golden/dualws_polygons.npz (bounded ones: 3 to 8 rows, every family that has them): their VERTICES are moved by p' = R(dth)(p - c) + c + d with
    plain numpy, their H-rep by the host build.  dualws_one's distance of the car to the moved H-rep agrees with the exact distance to the polygon of the moved vertices
    (tests/polygon_distance.py on an H-rep made from those vertices) within that file's 2e-8: sign, rotation sense and pivot are pinned by geometry."""
    g = golden("dualws_polygons.npz"); rng = np.random.default_rng(5); n = 0; worst = 0.0
    pick = [i for i in range(len(g["v"])) if g["v"][i] >= 3 and g["family"][i] in ("regular", "box", "small", "stretched", "overlap")][::9]
    for i in pick:
        v = int(g["v"][i]); A0, b0 = g["A"][i, :v], g["b"][i, :v]; nr = np.hypot(A0[:, 0], A0[:, 1]); pose = g["pose"][i]; ego = g["ego"]
        V0 = PD.hrep_vertices(A0, b0)
        if len(V0) != v or np.abs(V0).max() > 50:
            continue
        d = rng.uniform(-2, 2, 2); th = rng.uniform(-3, 3); c = rng.uniform(-4, 4, 2)
        A1, b1 = E.polygon_hrep(E.move_vertices(V0, d, th, c))
        want = PD.polygon_distance(*pose, ego, A1, b1)
        out, st = E.emu_move_parking(_one_obstacle_record(A0, b0), np.r_[d, th][None], c[None], None)
        A2, b2, _ = E.rows_of(out)
        got = _host_distance(emu, pose, ego, A2, b2)
        assert st[0] == 0 and abs(got - want) <= TOL_D and got >= -TOL_D, (g["name"][i], got, want)
        worst = max(worst, abs(got - want)); n += 1
    print("%d polygons, largest |d(moved H-rep) - d(moved vertices)| %.3g" % (n, worst))
    assert n >= 20


# ---------------------------------------------------------------- 5. inflation
def test_inflation_moves_edges_out_by_m_and_over_covers_at_corners():
    ego = [3.7, 1, 1, 1]; A, b = E.polygon_hrep(E.box(2.0, 6.0, -1.0, 1.0)); rec = _one_obstacle_record(A, b)
    for m in (0.1, 0.013, -0.2):
        out, st = E.emu_move_parking(rec, None, None, np.array([m])); A2, b2, _ = E.rows_of(out)
        assert st[0] == 0 and E.same(A2, A) and np.abs(b2 - (b + m)).max() <= 1e-15
        # the car far on the -x side, heading along x: its nose faces the edge x = 2
        face = (-6.0, 0.2, 0.0); d0 = PD.polygon_distance(*face, ego, A, b); d1 = PD.polygon_distance(*face, ego, A2, b2)
        assert d0 > 1.0 and abs((d0 - d1) - m) <= TOL_D, (m, d0, d1)
        # diagonally off the corner (2, -1): the offset polygon's corner lies sqrt(2) m out, the disc sum's only m
        for corner in ((-3.0, -4.0, 0.3), (-1.5, -5.0, 1.2)):
            c0 = PD.polygon_distance(*corner, ego, A, b); c1 = PD.polygon_distance(*corner, ego, A2, b2)
            assert c0 > 0.5 and ((c0 - c1) >= m * (1 - 1e-12) if m > 0 else (c0 - c1) <= m * (1 - 1e-12)), (m, corner, c0, c1)


# ---------------------------------------------------------------- 6. the quadcopter
def test_quadcopter_boxes_move_bit_for_bit_with_numpy():
    B = 4; prob = E.quad_records(B); rng = np.random.default_rng(2)
    motion = rng.uniform(-0.5, 0.5, (B, 5, 3)); inflate = rng.uniform(-0.05, 0.2, (B, 5))
    motion[2, 3, 1] = np.nan
    ref, rst = E.numpy_move_quad(prob, motion, inflate)
    runs = [E.emu_move_quad(prob, motion, inflate, rev=rev) for rev in (0, 1)]
    assert E.same(runs[0][0], runs[1][0]) and E.same(runs[0][0], ref)
    out, st = runs[0]
    assert st.tolist() == rst.tolist() == [0, 0, 1, 0] and E.same(out[2], prob[2])
    ob = slice(P.QPH_OB, P.QPH_OB + 30); keep = np.ones(prob.shape[1], bool); keep[ob] = False
    assert E.same(out[:, keep], prob[:, keep]) and out[0, P.QPH_R] == prob[0, P.QPH_R]
    for args in ((None, None), (np.zeros(3), 0.0)):
        assert E.same(E.emu_move_quad(prob, *args)[0], prob) and E.same(E.numpy_move_quad(prob, *args)[0], prob)
    for bad_inflate in (np.inf, np.nan):
        mg = inflate.copy(); mg[1, 0] = bad_inflate
        assert E.emu_move_quad(prob, None, mg)[1].tolist() == E.numpy_move_quad(prob, None, mg)[1].tolist() == [0, 1, 0, 0]
    # a pure motion: the distance of a point to the moved box is the distance of the point minus d to the old box
    d = np.array([0.4, -0.3, 0.25]); moved, _ = E.emu_move_quad(prob, d, None)
    for pt in rng.uniform(0, 8, (20, 3)):
        for i in (0, 1, 3):
            assert np.abs(E.box_distance(pt, moved[i, ob]) - E.box_distance(pt - d, prob[i, ob])).max() <= 1e-14
    # an inflation grows every box by m on all six sides
    grown, _ = E.emu_move_quad(prob, None, 0.1)
    assert np.array_equal(grown[:, ob], prob[:, ob] + 0.1)


# ---------------------------------------------------------------- 7. the front end's broadcasting
def test_front_end_broadcasts_per_obstacle_and_per_instance():
    from obca_amd import api
    nObs = np.array([1, 16, 2, 3, 3]); nt = 25
    assert api._per_obstacle(None, nObs, 3) is None
    assert np.array_equal(api._per_obstacle([1, 2, 3], nObs, 3), np.tile([1.0, 2, 3], (nt, 1))) and np.array_equal(api._per_obstacle(0.5, nObs, 0), np.full(nt, 0.5))
    per = np.arange(10.0).reshape(5, 2)
    assert np.array_equal(api._per_obstacle(per, nObs, 2), np.repeat(per, nObs, axis=0)) and np.array_equal(api._per_obstacle(np.arange(5.0), nObs, 0), np.repeat(np.arange(5.0), nObs))
    packed = np.arange(75.0).reshape(25, 3)
    assert np.array_equal(api._per_obstacle(packed, nObs, 3), packed) and api._per_obstacle(packed, nObs, 3).flags.c_contiguous
    with pytest.raises(ValueError):
        api._per_obstacle(np.zeros((4, 3)), nObs, 3)
    assert api._per_box([1, 2, 3], 4, 3).shape == (4, 5, 3) and api._per_box(np.arange(4.0), 4, 0)[:, 0].tolist() == [0, 1, 2, 3] and api._per_box(np.arange(5.0), 4, 0)[0].tolist() == [0, 1, 2, 3, 4]
    assert api._per_box(np.arange(12.0).reshape(4, 3), 4, 3)[2, 4].tolist() == [6, 7, 8] and api._per_box(None, 4, 0) is None


# ---------------------------------------------------------------- 8. the public surface, the build rule, the Julia shim
def test_header_exports_python_and_julia_agree():
    import obca_amd
    from obca_amd import api, cabi, planner as PL
    import test_hybrid_cpu as TH
    import test_julia_shim_cpu as J
    protos = cabi.prototypes("obca_scene_edit.h")
    assert sorted(protos) == sorted(api.SCENE_EDIT_EXPORTS) and len(protos) == 6 and "obca_scene_edit.h" in cabi.__doc__
    others = set()
    for name in dir(api):
        if name.endswith("EXPORTS") and name != "SCENE_EDIT_EXPORTS":
            others |= set(getattr(api, name))
    assert len(others) > 100 and not set(api.SCENE_EDIT_EXPORTS) & (others | set(PL.PLAN3D_EXPORTS))
    assert [len(protos[n][1]) for n in api.SCENE_EDIT_EXPORTS] == [5, 2, 3, 4, 2, 2]
    # no name of the header falls under a filter by which an older test picks ITS entry points out of the library's symbols
    assert not any(w in s for s in api.SCENE_EDIT_EXPORTS for w in ("track", "rollout", "plan", "refine", "hybrid", "scene", "subdivide", "clearance", "path_ws", "start_download",
                                                                    "ensemble", "certify", "shift", "advance"))
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {s for s in exported if "obstacles" in s} == set(api.SCENE_EDIT_EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "obca_scene_edit.h")).read()
    for cls, params in ((obca_amd.Batch, ["motion", "pivot", "inflate"]), (obca_amd.QuadBatch, ["motion", "inflate"])):
        sig = inspect.signature(cls.move_obstacles).parameters
        assert list(sig) == ["self"] + params and all(sig[n].default is None for n in params)
        assert callable(cls.obstacles) and "move_obstacles_ms" in vars(api._DeviceBatch)
    assert "not scaled back" in obca_amd.Batch.obstacles.__doc__ and "describes the scene it was computed in" in obca_amd.Batch.move_obstacles.__doc__
    assert inspect.signature(V.move_obstacles_parking).parameters.keys() >= {"A", "b", "vOb", "motion", "pivot", "inflate"}
    assert list(inspect.signature(V.move_obstacles_quad).parameters) == ["ob", "motion", "inflate"]
    # every ccall of the shim against the header, parameter by parameter; a library constant of its own
    kinds = TH._kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCASceneEdit.jl")).read()
    assert re.search(r"^const SED = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), SED\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
        assert m.group(2) == "Cint"
    assert {n for n, _ in calls} == set(kinds) == set(api.SCENE_EDIT_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])
    assert src.count("ccall(") == len(calls) + 1 and "ccall((:obca_last_error, LIB)" in src


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu"); name = "scene_edit_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_scene_edit_emu.so")
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
    for h in ("obca_scene_edit.h", "obca_validate.h", "obca_solver.h", "obca_quad_solver.h", "obca_model.h"):
        assert os.path.realpath(os.path.join(csrc, h)) in seen, h
    assert os.path.realpath(os.path.join(ROOT, "include", "obca_scene_edit.h")) in deps
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_scene_edit_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/scene_edit_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # nothing in csrc includes the kernel text but the one line of the library
    for f in os.listdir(csrc):
        if f.endswith((".h", ".hip", ".cpp")) and f != "obca_hip.hip":
            assert not re.search(r'#\s*include\s*"obca_scene_edit.h"', open(os.path.join(csrc, f)).read()), f
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    assert hip.count('#include "obca_scene_edit.h"') == 1 and hip.count('#include "../../include/obca_scene_edit.h"') == 1
    assert hip.index('#include "obca_validate.h"') < hip.index('#include "obca_scene_edit.h"')
    # all or nothing: one reduction per instance function stands between the last computed word and the first store; no atomics, no loops that wait, no LDS of its own
    raw = open(os.path.join(csrc, "obca_scene_edit.h")).read(); txt = re.sub(r"//.*", "", raw)
    assert "#include" not in txt and '#error "include the validate kernel text' in raw and "ORDER" in raw
    assert not re.search(r"\bwhile\b|\bbreak\b|\bgoto\b|atomic|__shared__|CL_LDS", txt)
    for fn in ("move_parking_instance", "move_quad_instance"):
        body = txt[txt.index("void " + fn):]; body = body[:body.index("\n}\n")]
        assert body.count("wred_max(") == 1 and "prob[" not in body[:body.index("wred_max(")] and "status[0]" not in body[:body.index("wred_max(")], fn
    assert txt.count("sin(") == 1 and txt.count("cos(") == 1
    # the kernels of the library write nothing but the records and the status: no solve buffer is among their arguments
    for k in re.findall(r"void (obca_move_\w+_kernel)\(([^)]*)\)", hip):
        assert not re.search(r"DevBufs|\bz0?\b|\binfo\b", k[1]), k
