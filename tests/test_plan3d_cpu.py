"""The device-side 3-D grid planner (obca_amd/csrc/obca_plan3d.h) compiled for the host (tests/emu/plan3d_emu.cpp) against the host A* (obca_plan_astar3d through
planner.astar3d): statuses, path costs, path validity, the resampled warm start, order independence of the relaxation, the oracle's solves from its paths; and the
library's export list, warnings and Julia wrapper.  Helpers and the derivation of the cost tolerance: tests/plan3d_common.py."""
import ctypes as C
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from conftest import ROOT
import plan3d_common as K
from obca_amd import scenarios as S, planner as PL

NPAIRS = 256


@pytest.fixture(scope="module")
def planned():
    """256 random pairs + the shipped one, planned by the emulation and by the host A*"""
    x0, xF = K.endpoints(NPAIRS)
    rc, paths, cnt, sw = K.emu_paths(x0[:, :3], xF[:, :3])
    assert rc == 0
    return dict(x0=x0, xF=xF, paths=paths, cnt=cnt, sweeps=sw, host=K.host_paths(x0, xF))


def test_cost_agreement_with_the_host_astar(planned):
    p = planned; worst = 0.0; n = 0
    assert p["cnt"][0] >= 3 and p["host"][0] is not None      # the shipped scenario has a path
    for i in range(NPAIRS + 1):
        h = p["host"][i]
        assert (h is None) == (p["cnt"][i] in (0, -2)), (i, p["cnt"][i], None if h is None else len(h))
        assert p["cnt"][i] in (0, -2) or p["cnt"][i] >= 3, (i, p["cnt"][i])
        if h is None:
            continue
        e = p["paths"][i, :p["cnt"][i]]
        (ce, _), (ch, _) = K.chain_cost(e), K.chain_cost(h); tol = K.cost_tolerance(e, h)
        assert tol < 2e-4 and abs(ce - ch) <= tol, (i, ce, ch, tol)
        worst = max(worst, abs(ce - ch)); n += 1
    print("paths compared: %d, largest cost difference %.3g m, sweeps mean %.1f max %d" % (n, worst, p["sweeps"].mean(), p["sweeps"].max()))
    assert n >= 200


def test_paths_are_valid(planned):
    p = planned
    for i in range(NPAIRS + 1):
        if p["cnt"][i] >= 2:
            K.assert_valid_path(p["paths"][i, :p["cnt"][i]], p["x0"][i], p["xF"][i], what=i)


def test_status_codes():
    g = S.QUAD_XF[:3]
    rc, _, cnt, _ = K.emu_paths([[2.2, 5.0, 2.0]], [g])                  # start inside the first wall
    assert rc == 0 and cnt[0] == -2
    assert PL.astar3d([2.2, 5.0, 2.0], g) is None                        # (the host's -2 reads None there)
    # a goal sealed by boxes: a closed shell around (5, 5, 2.5), the goal point itself free
    shell = []
    lo, hi = np.array([4.0, 4.0, 1.5]), np.array([6.0, 6.0, 3.5]); t = 0.1
    for ax in range(3):
        for side in (0, 1):
            a, b = lo.copy(), hi.copy()
            if side: a[ax] = hi[ax] - t
            else: b[ax] = lo[ax] + t
            shell.append(np.concatenate([b, -a]))
    shell = np.array(shell)
    assert len(shell) == 6
    goal = [5.0, 5.0, 2.5]
    rc, _, cnt, _ = K.emu_paths([[1.0, 1.0, 1.0]], [goal], boxes=shell, clear=0.3)
    assert rc == 0 and cnt[0] == 0
    assert PL.astar3d([1.0, 1.0, 1.0], goal, shell, 0.3) is None
    rc, _, cnt, _ = K.emu_paths([[1.0, 1.0, 1.0]], [[9.0, 9.0, 4.0]], boxes=shell, clear=0.3)      # ... and the same boxes let a path by
    assert rc == 0 and cnt[0] >= 3
    # cap too small: -1 for that instance; one more way-point fits
    rc, _, cnt, _ = K.emu_paths([S.QUAD_X0[:3]], [g])
    n = int(cnt[0]); assert n >= 3
    rc, _, c2, _ = K.emu_paths([S.QUAD_X0[:3]], [g], cap=n - 1)
    assert rc == 0 and c2[0] == -1
    rc, _, c2, _ = K.emu_paths([S.QUAD_X0[:3]], [g], cap=n)
    assert rc == 0 and c2[0] == n
    # beyond the limits: -1 from the call, with a message
    rc = K.emu_paths([S.QUAD_X0[:3]], [g], res=0.2)[0]                   # 51 x 51 x 26 nodes
    assert rc == -1 and b"MAXCELLS" in K.emu().emu_plan3d_last_error()
    rc = K.emu_paths([S.QUAD_X0[:3]], [g], boxes=np.tile(S.QUAD_OB[:1], (9, 1)))[0]
    assert rc == -1 and b"nBox" in K.emu().emu_plan3d_last_error()
    rc = K.emu_warm_start(S.QUAD_X0, S.QUAD_XF, PL.PLAN3D_NMAX + 1)[0]
    assert rc == -1 and b"NMAX" in K.emu().emu_plan3d_last_error()
    assert K.emu_warm_start(S.QUAD_X0, S.QUAD_XF, PL.PLAN3D_NMAX)[0] == 0
    rc = K.emu_paths([S.QUAD_X0[:3]], [g], cap=1)[0]
    assert rc == -1
    a = C.c_int(0); b = C.c_int(0); c = C.c_int(0); d = C.c_int(0)
    K.emu().emu_plan3d_limits(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    assert (a.value, b.value, c.value, d.value) == (PL.PLAN3D_MAXCELLS, PL.PLAN3D_MAXBOX, PL.PLAN3D_NMAX, PL.PLAN3D_WS_CAP)
    hdr = open(os.path.join(ROOT, "include", "obca_hip.h")).read()
    assert int(re.search(r"#define OBCA_QUAD_NMAX (\d+)", hdr).group(1)) == c.value
    assert np.prod(K.DIMS) <= a.value and (a.value + 4) * 4 <= 160 * 1024      # the shipped room fits the budget, the budget fits the LDS


def test_per_instance_obstacles():
    """instances of one batch carry different boxes: each gets what a batch of it alone gets"""
    x0, xF = K.endpoints(5, seed=7)
    sets = [S.QUAD_OB, S.QUAD_OB[:1], S.QUAD_OB[1:], np.array([[5.5, 10, 5, -4.5, 0, -1.0]] * 5, float), S.QUAD_OB[[0, 0, 0, 0, 0]], S.QUAD_OB[::-1]]
    boxes = np.stack([np.asarray(s_, float).reshape(-1, 6)[np.arange(5) % len(s_)] for s_ in sets])
    rc, paths, cnt, _ = K.emu_paths(x0[:, :3], xF[:, :3], boxes=boxes)
    assert rc == 0 and (cnt >= 3).sum() >= 4
    for i in range(len(x0)):
        rc, p1, c1, _ = K.emu_paths(x0[i:i + 1, :3], xF[i:i + 1, :3], boxes=boxes[i])
        assert rc == 0 and c1[0] == cnt[i] and np.array_equal(p1[0], paths[i]), i
        h = PL.astar3d(x0[i, :3], xF[i, :3], boxes[i])
        assert (h is None) == (cnt[i] < 2), i
        if h is not None:
            assert abs(K.chain_cost(h)[0] - K.chain_cost(paths[i, :cnt[i]])[0]) <= K.cost_tolerance(h, paths[i, :cnt[i]]), i
    assert len({int(c) for c in cnt}) > 1 or not np.array_equal(paths[0], paths[1])      # the boxes matter


@pytest.mark.parametrize("N", [20, 60, 128])
def test_resampling(N):
    x0, xF = K.endpoints(24, seed=3)
    rc, xWS, cnt, paths = K.emu_warm_start(x0, xF, N, with_paths=True)
    assert rc == 0 and (cnt >= 3).sum() >= 20
    rc2, p2, c2, _ = K.emu_paths(x0[:, :3], xF[:, :3])
    assert rc2 == 0 and np.array_equal(c2, cnt)
    for i in range(len(x0)):
        assert (xWS[i, :, 3:] == 0).all(), i
        if cnt[i] < 2:
            assert (xWS[i] == 0).all(), i
            continue
        assert np.array_equal(p2[i, :cnt[i]], paths[i, :cnt[i]]), i
        chain = paths[i, 1:cnt[i] - 1]
        want = S.quad_warm_start(x0[i], xF[i], N, via=[tuple(p) for p in chain])
        assert np.abs(xWS[i] - want).max() <= 1e-12, (i, np.abs(xWS[i] - want).max())
        assert np.array_equal(xWS[i, 0, :3], x0[i, :3]), i


def test_order_independence_on_the_host():
    """the relaxation is in place: visiting the nodes of every sweep in the opposite order must end in the same field, bit for bit"""
    x0, xF = K.endpoints(16, seed=5)
    rc, p0, c0, s0, f0 = K.emu_paths(x0[:, :3], xF[:, :3], field=True)
    rc1, p1, c1, s1, f1 = K.emu_paths(x0[:, :3], xF[:, :3], field=True, reverse=1)
    assert rc == 0 and rc1 == 0 and np.array_equal(c0, c1) and np.array_equal(p0, p1)
    assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
    assert not np.array_equal(s0, s1)      # the orders really differ: they need different numbers of sweeps
    ok = c0 >= 3
    assert ok.sum() >= 12 and np.isfinite(f0[ok]).any() and (f0[ok] == -1.0).any()
    print("sweeps ascending", s0.tolist(), "descending", s1.tolist())


def test_oracle_solves_from_the_emulated_paths():
    """the 12 pairs of np.random.default_rng(11), N = 40: every NLP the oracle solves from the host A* path it also solves from the relaxation's path"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_quad as Q
    rng = np.random.default_rng(11); N = 40
    pairs = [S._draw_quad_endpoints(rng) for _ in range(12)]
    x0 = np.zeros((12, 12)); xF = np.zeros((12, 12))
    for i, (a, b) in enumerate(pairs):
        x0[i, :3] = a; xF[i, :3] = b
    rc, xWS, cnt = K.emu_warm_start(x0, xF, N)
    assert rc == 0
    its = []
    for i in range(12):
        wh = PL.quad_warm_start(x0[i], xF[i], N)
        assert (wh is None) == (cnt[i] < 2), i
        if wh is None:
            continue
        rh = Q.quadcopter_signed_dist(x0[i], xF[i], N, S.quad_sample_time(N), S.QUAD_R, S.QUAD_OB, wh, 1.0)
        re_ = Q.quadcopter_signed_dist(x0[i], xF[i], N, S.quad_sample_time(N), S.QUAD_R, S.QUAD_OB, xWS[i], 1.0)
        its.append((rh["iters"], re_["iters"]))
        assert rh["exitflag"] != 1 or re_["exitflag"] == 1, (i, rh["exitflag"], re_["exitflag"])
    print("oracle iterations (host path, relaxation path):", its)
    assert len(its) == 12


def test_exports_and_warnings():
    lib = PL.build_plan3d_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "obca_plan3d.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(obca_[a-z_0-9]+)\s*\(", hdr)))
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and not l.split()[2].startswith("_"))
    assert declared == exported == sorted(PL.PLAN3D_EXPORTS) and len(declared) == 6, (declared, exported)
    from obca_amd.buildflags import HIPCC
    base = [f for f in HIPCC if f not in ("-shared", "-fPIC")] + ["-fsyntax-only", "-Wno-unused-command-line-argument"]
    r = subprocess.run(base + [os.path.join(ROOT, "obca_amd", "csrc", "obca_plan3d.hip")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stdout.strip() and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-2000:])
    # the older libraries keep their symbols: nothing of the new one leaked into them
    for other in ("libobca_plan.so", "libobca_hip.so"):
        p = os.path.join(ROOT, "obca_amd", "csrc", other)
        if os.path.exists(p):
            assert "plan3d" not in subprocess.run(["nm", "-D", "--defined-only", p], capture_output=True, text=True).stdout, other


def test_no_cpu_fallback_of_the_device_call():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(PL.Plan3DError):
        PL.astar3d_many([S.QUAD_X0[:3]], [S.QUAD_XF[:3]])
    with pytest.raises(PL.Plan3DError):
        S.make_quad_batch(2, 20, random_endpoints=True, device=0)


def test_device_none_keeps_the_host_loop():
    """the default of the new keyword is the code path of before: same end points, same warm starts"""
    a = S.make_quad_batch(3, 20, random_endpoints=True); b = S.make_quad_batch(3, 20, random_endpoints=True, device=None)
    assert all(np.array_equal(a[k], b[k]) for k in ("x0", "xF", "xWS"))
    w = np.stack([PL.quad_warm_start(a["x0"][i], a["xF"][i], 20) for i in range(3)])
    assert np.array_equal(w, a["xWS"])
    x0 = a["x0"].copy(); xF = a["xF"].copy()
    assert np.array_equal(S.plan_quad_batch(x0, xF, 20, np.random.default_rng(1)), a["xWS"])


JL = {"Cint": "int", "Cdouble": "double", "Cfloat": "float"}


def test_julia_wrapper_matches_the_header():
    """every ccall of julia/OBCAPlan3D.jl against its prototype in include/obca_plan3d.h, parameter by parameter (the method of tests/test_julia_shim_cpu.py)"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "obca_plan3d.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(?:int|const char \*)\s*(obca_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        kinds = []
        for p in [q.strip() for q in m.group(2).split(",")]:
            kinds.append("ptr" if "*" in p or "[" in p else "double" if re.match(r"(const\s+)?double\b", p) else "int" if re.match(r"(const\s+)?int\b", p) else "?" + p)
        protos[m.group(1)] = kinds
    assert sorted(protos) == sorted(PL.PLAN3D_EXPORTS)
    src = open(os.path.join(ROOT, "julia", "OBCAPlan3D.jl")).read()
    seen = set()
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), PLAN3D\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        kinds = ["ptr" if t.startswith(("Ptr{", "Ref{")) or t == "Cstring" else JL.get(t, "?" + t) for t in types]
        assert m.group(1) in protos and kinds == protos[m.group(1)], (m.group(1), kinds, protos.get(m.group(1)))
        assert m.group(2) == ("Cstring" if m.group(1) == "obca_plan3d_last_error" else "Cint"), m.group(1)
        seen.add(m.group(1))
    assert seen == set(protos)
    assert src.count("ccall(") == len(re.findall(r"ccall\(\(:obca_plan3d_[a-z_]+, PLAN3D\)", src))
