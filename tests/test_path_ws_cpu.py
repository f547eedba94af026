"""Parking warm starts from planner paths: the kernel text of obca_amd/csrc/obca_path_ws.h compiled for the host (tests/emu/path_ws_emu.cpp, emu_path_ws_*) against the numpy
statement planner.path_to_warm_start / velo_smooth -- planner paths of both scenarios, synthetic edge shapes, every status and every refusal, guard words around every output
(tests/path_ws_common.py has the helpers and the derivation of the tolerances); and the ABI of include/obca_path_ws.h: prototypes, exports, the Python list, the Julia ccalls."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import packing as PK
import path_ws_common as K
from obca_amd import api, cabi, planner as PL, scenarios as S

HORIZONS = (7, 80, 128)
EDGE_HORIZONS = (1, 2, 63, 64, 65, 128)


@pytest.fixture(scope="module")
def planned():
    """both scenarios, 96 start poses each, planned once"""
    return {sc["name"]: K.planner_paths(sc) + (PL.SCENARIO_OPTS[sc["name"]][1],) for sc in (S.BACKWARDS, S.PARALLEL)}


@pytest.fixture(scope="module")
def syn():
    return K.synthetic()


def test_planner_paths_against_numpy(planned):
    """sign(v) equal on EVERY instance and stage; Ts, poses, v, a within 1e-11, delta within 1e-9"""
    n = 0; worst = [0.0, 0.0]
    for name, (paths, dirs, cnt, xF, v_nom) in planned.items():
        have = np.flatnonzero(cnt >= 2)
        assert len(have) >= 48 and cnt.max() <= K.MAXNODES, (name, cnt)
        for N in HORIZONS:
            for xf in (None, xF):
                for a_max in (0.0, 0.3):
                    rc, Ts, x, u, st = K.emu_batch(paths, dirs, cnt, N, xf, v_nom=v_nom, a_max=a_max)
                    assert rc == 0 and (st[have] == 0).all() and (st[cnt < 2] == -1).all()
                    e, ed = K.compare((Ts, x, u), K.numpy_batch(paths, dirs, cnt, N, xf, v_nom=v_nom, a_max=a_max), have, (name, N, xf is not None, a_max))
                    worst = [max(worst[0], e), max(worst[1], ed)]
        n += len(have)
    print("paths compared: %d, largest difference %.3g (Ts, pose, v, a), %.3g (delta)" % (n, worst[0], worst[1]))


def test_synthetic_edges_against_numpy(syn):
    paths, dirs, cnt, xF = syn
    have = np.flatnonzero(cnt >= 2); none = np.flatnonzero(cnt < 2)
    assert set(K.NODE_COUNTS) <= set(cnt.tolist()) and len(none) == 1 and 0 < none[0] < len(cnt) - 1          # an instance without a path in the middle of the batch
    jumps = [np.diff(paths[i, :cnt[i], 2]) for i in have]
    assert any((j > np.pi).any() for j in jumps) and any((j < -np.pi).any() for j in jumps)                    # the yaw runs across +-pi in both senses
    assert any((np.hypot(*np.diff(paths[i, :cnt[i], :2], axis=0).T) == 0).any() for i in have) and any((dirs[i, :cnt[i]] == 0).any() for i in have)
    nsw = [int((np.diff(dirs[i, 1:cnt[i]]) != 0).sum()) for i in have]
    assert {0, 1}.issubset(nsw) and max(nsw) >= 3
    accs = set()
    for N in EDGE_HORIZONS + (3,):
        for xf in (None, xF):
            for a_max in (0.0, 0.3):
                rc, Ts, x, u, st = K.emu_batch(paths, dirs, cnt, N, xf, a_max=a_max)
                assert rc == 0 and (st[have] == 0).all() and st[none[0]] == -1
                assert Ts[none[0]] == 0 and not x[none[0]].any() and not u[none[0]].any()                      # the host call zeros what it does not write
                K.compare((Ts, x, u), K.numpy_batch(paths, dirs, cnt, N, xf, a_max=a_max), have, ("synthetic", N, xf is not None, a_max))
                if a_max:
                    acc = np.round(0.5 / a_max / Ts[have])
                    accs |= {(int(a) == 0, bool(a > N + 41), bool(0 < 2 * a and N > 8 and a > N / 8)) for a in acc}
    # acc = 0, ramps longer than the whole padded profile, ramps long enough to overlap their neighbours' on a path with three switches: all met
    assert any(z for z, _, _ in accs) and any(l for _, l, _ in accs) and any(o for _, _, o in accs)


def test_rows_beyond_the_count_are_never_read(syn):
    paths, dirs, cnt, xF = syn
    p2 = paths.copy(); d2 = dirs.copy()
    for i, c in enumerate(cnt):
        p2[i, max(c, 0):] = 1e300; d2[i, max(c, 0):] = -5
    a = K.emu_batch(paths, dirs, cnt, 64, xF, a_max=0.3); b = K.emu_batch(p2, d2, cnt, 64, xF, a_max=0.3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_every_status_code():
    rng = np.random.default_rng(5); cap = 40; N = 20
    P, D = K.make_path(rng, 30, switch_at=(9,))
    B = 9; paths = np.full((B, cap, 3), np.nan); dirs = np.full((B, cap), 9, np.int32); cnt = np.full(B, 30, np.int32)
    paths[:, :30] = P; dirs[:, :30] = D
    cnt[1] = 0; cnt[2] = 1; cnt[3] = -1                                 # no path
    cnt[4] = cap + 1                                                    # more nodes than rows
    paths[5, 29, 1] = np.inf                                            # a non-finite pose among the used rows
    paths[6, :30, :2] = paths[6, 0, :2]                                 # zero length
    cnt[7] = 29; paths[7, 29] = np.nan                                  # the NaN is behind the count: not read
    rc, Ts, x, u, st = K.emu_batch(paths, dirs, cnt, N)
    assert rc == 0 and st.tolist() == [0, -1, -1, -1, -2, -3, -4, 0, 0], st
    for i in (1, 2, 3, 4, 5, 6):
        assert Ts[i] == 0 and not x[i].any() and not u[i].any(), i
    ref = K.numpy_batch(paths, dirs, np.where(st == 0, cnt, 0), N)
    K.compare((Ts, x, u), ref, [0, 7, 8], "neighbours of refused instances")
    assert np.array_equal(x[0], x[8]) and np.array_equal(u[0], u[8]) and Ts[0] == Ts[8]      # the neighbours are unaffected
    # a non-finite goal is a non-finite pose; a count above the limit of the kernel is -2 even where the rows exist
    xF = np.zeros((B, 4)); xF[:, :3] = P[-1]; xF[0, 2] = np.nan; xF[6, :2] = paths[6, 0, :2]      # (the goal is the last node: instance 6 stays without length)
    assert K.emu_batch(paths, dirs, cnt, N, xF)[4].tolist() == [-3, -1, -1, -1, -2, -3, -4, 0, 0]
    big = np.zeros((1, K.MAXNODES + 8, 3)); big[0, :, 0] = np.arange(K.MAXNODES + 8) * 0.01
    assert K.emu_batch(big, np.ones((1, K.MAXNODES + 8), np.int32), [K.MAXNODES + 1], N)[4].tolist() == [-2]
    assert K.emu_batch(big, np.ones((1, K.MAXNODES + 8), np.int32), [K.MAXNODES], N)[4].tolist() == [0]


def test_every_refusal_of_the_call(syn):
    """the one validation function of the kernel text (path_ws_check_args), which the library's two calls use as well"""
    paths, dirs, cnt, xF = syn
    mx, nmax = C.c_int(0), C.c_int(0)
    K.emu().emu_path_ws_limits(C.byref(mx), C.byref(nmax))
    assert (mx.value, nmax.value) == (K.MAXNODES, 128) == (api.PATH_WS_MAXNODES, 128)
    ok = dict(N=8, v_nom=0.5, L=2.7, a_max=0.3)
    assert K.emu_batch(paths, dirs, cnt, **ok)[0] == 0
    inf, nan = np.inf, np.nan
    bad = [dict(B=0), dict(B=-3), dict(N=0), dict(N=nmax.value + 1), dict(cap=1), dict(cap=0)]
    bad += [{k: v} for k in ("v_nom", "L") for v in (0.0, -0.5, inf, nan)] + [dict(a_max=v) for v in (-0.1, inf, nan)]
    bad += [dict(null=(k,)) for k in ("paths", "dirs", "counts", "Ts", "xWS", "uWS", "status")]
    for kw in bad:
        a = dict(ok); a.update(kw)
        rc, Ts, x, u, st = K.emu_batch(paths, dirs, cnt, **a)
        assert rc == -1 and K.emu().emu_path_ws_last_error(), kw
        assert (Ts == K.SENTINEL).all() and (x == K.SENTINEL).all() and (st == -77777).all(), kw      # a refused call writes nothing
    assert K.emu_batch(paths, dirs, cnt, 8, a_max=0.0)[0] == 0 and K.emu_batch(paths, dirs, cnt, nmax.value)[0] == 0


def test_resident_record(syn):
    """path_ws_record, the instance body of obca_batch_set_path_warm_start: Ts, the reference rows, x, u, t of the start iterate as the host call returns them, zeros from the
    multipliers to the end of the row, every other word of the record as uploaded; a negative status touches nothing."""
    paths, dirs, cnt, xF = syn
    A, b, vrows = S.scenario_hrep(S.BACKWARDS); nOb, M = len(vrows), int(np.sum(vrows))
    rng = np.random.default_rng(1); D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    for N, a_max, use_xF in ((40, 0.0, 1), (65, 0.3, 1), (7, 0.3, 0)):
        lay = PK.layout(N, nOb, M); zlen = lay["len"] + 11
        _, Ts, x, u, st = K.emu_batch(paths, dirs, cnt, N, xF if use_xF else None, v_nom=0.4, a_max=a_max)
        for i in (0, 20, 43, 60, len(cnt) - 1):
            p0 = PK.pack_problem(rng.normal(size=4), xF[i], N, 0.77, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, vrows, A, b, *rng.normal(size=(3, N + 1)), 0)
            z0 = rng.normal(size=zlen); g = np.full(8, K.SENTINEL)
            pb = np.concatenate([g, p0, g]); zb = np.concatenate([g, z0, g]); p = pb[8:-8]; z = zb[8:-8]
            rc = K.emu().emu_path_ws_record(N, int(cnt[i]), paths.shape[1], paths[i].ctypes.data_as(D), np.ascontiguousarray(dirs[i]).ctypes.data_as(I), use_xF, 0.4, a_max,
                                            p.ctypes.data_as(D), z.ctypes.data_as(D), zlen)
            assert rc == st[i] and (pb[:8] == K.SENTINEL).all() and (pb[-8:] == K.SENTINEL).all() and (zb[:8] == K.SENTINEL).all() and (zb[-8:] == K.SENTINEL).all()
            if rc:
                assert np.array_equal(p, p0) and np.array_equal(z, z0)
                continue
            want = p0.copy(); want[PK.PH["TS"]] = Ts[i]; want[PK.OB_HDR:] = x[i, :, :3].T.ravel()
            assert np.array_equal(p, want)
            assert np.array_equal(z[lay["x"]:lay["u"]], x[i].ravel()) and np.array_equal(z[lay["u"]:lay["t"]], u[i].ravel()) and z[lay["t"]] == 1.0 and not z[lay["lam"]:].any()
    assert any(st < 0)


def test_device_none_keeps_the_numpy_loop():
    """the default of the new keyword is the code path of before"""
    sc = S.BACKWARDS; x0, xF = S.sample_poses(sc, 4, np.random.default_rng(3)); N = 30
    a = PL.warm_start_many(sc, x0, xF, N); b = PL.warm_start_many(sc, x0, xF, N, device=None)
    A, bb, vrows = S.scenario_hrep(sc)
    res = PL.hybrid_astar_many(x0[:, :3], xF[:, :3], vrows, A, bb, threads=PL.effective_cpus())
    for i in range(4):
        w = PL.path_to_warm_start(res[i][0], res[i][1], N, xF[i], v_nom=0.5)
        assert all(np.array_equal(p, q) and np.array_equal(p, r) for p, q, r in zip(a[i], b[i], w))
    m = S.make_batch(S.PARALLEL, 2, 20, seed=4); m2 = S.make_batch(S.PARALLEL, 2, 20, seed=4, device=None)
    assert all(np.array_equal(m[k], m2[k]) for k in ("x0", "Ts", "xWS", "uWS"))


def test_no_cpu_fallback_of_the_device_calls(syn):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    paths, dirs, cnt, xF = syn
    with pytest.raises(api.ObcaError):
        PL.path_to_warm_start_many(paths, dirs, cnt, 20, xF)
    with pytest.raises(api.ObcaError):
        S.make_batch(S.PARALLEL, 2, 20, seed=4, device=0)
    with pytest.raises(api.ObcaError, match="paths must be"):
        api._path_arrays(paths[:, :, :2], dirs, cnt, len(cnt))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "obca_path_ws.h")).read(), flags=re.S)


def test_header_prototypes_exports_and_the_python_list():
    protos = cabi.prototypes("obca_path_ws.h")
    declared = sorted(set(re.findall(r"\b(obca_[a-z_0-9]+)\s*\(", _header())))
    assert sorted(protos) == declared == sorted(api.PATH_WS_EXPORTS) and len(declared) == 3
    assert not set(api.PATH_WS_EXPORTS) & set(api.EXPORTS)
    args = protos["obca_parking_path_warm_start_batch"][1]
    assert len(args) == 15 and args[0] is C.c_void_p and args[1:3] == [C.c_int, C.c_int] and args[8:11] == [C.c_double] * 3
    assert [isinstance(a, cabi.ArrayParam) and a.const for a in args[3:6]] == [True] * 3 and [a.dtype for a in args[3:6]] == [np.float64, np.int32, np.int32]
    assert [isinstance(a, cabi.ArrayParam) and not a.const for a in args[11:]] == [True] * 4 and args[14].dtype == np.int32
    assert len(protos["obca_batch_set_path_warm_start"][1]) == 9 and protos["obca_batch_path_ws_ms"][1] == [C.c_void_p, C.POINTER(C.c_float)]
    import obca_amd
    lib = obca_amd.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"}
    assert set(declared) <= exported
    assert int(re.search(r"#define OBCA_PATH_WS_MAXNODES (\d+)", _header()).group(1)) == api.PATH_WS_MAXNODES == K.MAXNODES
    # the library binds both headers: the new entry points carry their argument types
    assert api._load().obca_batch_path_ws_ms.argtypes == protos["obca_batch_path_ws_ms"][1]


def test_the_device_source_compiles_without_a_warning():
    from obca_amd.buildflags import HIPCC
    base = [f for f in HIPCC if f not in ("-shared", "-fPIC")] + ["-fsyntax-only", "-Wno-unused-command-line-argument"]
    r = subprocess.run(base + [os.path.join(ROOT, "obca_amd", "csrc", "obca_hip.hip")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stdout.strip() and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-2000:])
    src = open(os.path.join(ROOT, "obca_amd", "csrc", "obca_path_ws.h")).read()
    assert len(re.findall(r"\b(?:atan2?|sin|cos|tan|exp|log|pow|hypot|fmod|floor|ceil|round|rint|fma)\(", re.sub(r"//.*", "", src))) == 1      # atan is the one libm call of the text


JL = {"Cint": "int", "Cdouble": "double", "Cfloat": "float"}


def test_julia_wrapper_matches_the_header():
    """every ccall of julia/OBCAPathWS.jl against its prototype in include/obca_path_ws.h, parameter by parameter (the method of tests/test_plan3d_cpu.py)"""
    protos = {}
    for m in re.finditer(r"\b(?:int|const char \*)\s*(obca_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", _header(), flags=re.S):
        kinds = []
        for p in [q.strip() for q in m.group(2).split(",")]:
            kinds.append("ptr" if "*" in p or "[" in p else "double" if re.match(r"(const\s+)?double\b", p) else "int" if re.match(r"(const\s+)?int\b", p) else "?" + p)
        protos[m.group(1)] = kinds
    assert sorted(protos) == sorted(api.PATH_WS_EXPORTS)
    src = open(os.path.join(ROOT, "julia", "OBCAPathWS.jl")).read()
    seen = set()
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), PATHWS\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        kinds = ["ptr" if t.startswith(("Ptr{", "Ref{")) or t == "Cstring" else JL.get(t, "?" + t) for t in types]
        assert m.group(1) in protos and kinds == protos[m.group(1)], (m.group(1), kinds, protos.get(m.group(1)))
        assert m.group(2) == "Cint", m.group(1)
        seen.add(m.group(1))
    assert seen == set(protos)
    assert src.count("ccall(") == len(re.findall(r"ccall\(\(:obca_[a-z_]+, PATHWS\)", src))
    assert "OBCAHip.LIB" in src      # the same library file as the solves


# ---------------------------------------------------------------- the host build as a piece of the build rule (what tests/test_build_cpu.py checks for the pieces of PIECES)
def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch, capsys):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu")
    GXX = ["g++", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-misleading-indentation"]
    assert sorted(BF.TEST_PIECES) == ["path_ws_emu"] and not set(BF.TEST_PIECES) & set(BF.PIECES) and "path_ws_emu" not in BF.DEFAULT
    p = BF.TEST_PIECES["path_ws_emu"]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_path_ws_emu.so")
    # the include closure lies inside what the rule compares the output's age with
    deps = {os.path.realpath(d) for d in BF.dependencies(p.sources)}
    todo = [os.path.realpath(s) for s in p.sources]; seen = set()
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        assert f in deps, f
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', open(f).read(), flags=re.M):
            found = [c for c in (os.path.join(os.path.dirname(f), inc),) if os.path.exists(c)]
            assert found, (f, inc)
            todo.append(os.path.realpath(found[0]))
    assert os.path.realpath(os.path.join(ROOT, "obca_amd", "csrc", "obca_path_ws.h")) in seen and os.path.realpath(os.path.join(ROOT, "obca_amd", "csrc", "obca_solver.h")) in seen
    # the argv is pinned; build(NAME, out=, flags=) and the command line reach the piece
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_path_ws_emu.so")
    assert BF.build("path_ws_emu", force=True, out=aside) == aside and os.path.exists(aside)
    assert BF.build("path_ws_emu", force=True, out=aside, flags=["-O0", "-g"]) == aside
    for argv, flags in zip(calls, (["-O1"], ["-O0", "-g"])):
        i = argv.index("-o")
        assert argv[:i] == GXX + flags and argv[i + 2:] == [EMU + "/path_ws_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path) and argv[i + 1].endswith(".so")
    built = []
    monkeypatch.setattr(BF, "build", lambda n: built.append(n) or "/x/" + n)
    BF.main(["build", "path_ws_emu"])
    assert built == ["path_ws_emu"] and capsys.readouterr().out.split() == ["/x/path_ws_emu"]


def test_device_branch_binds_the_keywords_like_the_numpy_branch(monkeypatch):
    """warm_start_many(..., device=...) with the device call replaced by the host build of its kernel text: cap, ego, L and XYbounds reach the search as hybrid_astar_many's
    named parameters, not as search options, and the warm starts are the numpy branch's within the tolerances"""
    seen = {}

    def stand_in(paths, dirs, counts, N, xF=None, v_nom=0.5, L=S.L_WHEELBASE, smooth=False, device=0):
        seen.update(cap=paths.shape[1], device=device)
        rc, Ts, x, u, st = K.emu_batch(paths, dirs, counts, N, xF, v_nom=v_nom, L=L, a_max=0.3 if smooth else 0.0)
        assert rc == 0
        return Ts, x, u, st == 0
    monkeypatch.setattr(PL, "path_to_warm_start_many", stand_in)
    sc = S.BACKWARDS; x0, xF = S.sample_poses(sc, 5, np.random.default_rng(11)); N = 30
    kw = dict(cap=512, ego=S.EGO.copy(), L=S.L_WHEELBASE, XYbounds=S.XYBOUNDS.copy(), switch_cost=2.5)
    for smooth in (False, True):
        a = PL.warm_start_many(sc, x0, xF, N, smooth=smooth, device=3, **kw); b = PL.warm_start_many(sc, x0, xF, N, smooth=smooth, **kw)
        assert seen == dict(cap=512, device=3) and len(a) == len(b) == 5
        for p, q in zip(a, b):
            assert (p is None) == (q is None)
            if p is not None:
                assert abs(p[0] - q[0]) <= K.TOL and np.abs(p[1] - q[1]).max() <= K.TOL and np.abs(p[2][:, 1] - q[2][:, 1]).max() <= K.TOL and np.abs(p[2][:, 0] - q[2][:, 0]).max() <= K.TOL_DELTA
    assert any(p is not None for p in a)
