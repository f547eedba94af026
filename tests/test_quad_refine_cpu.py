"""Refinement of solved quadcopter instances onto a finer horizon (obca_amd/csrc/obca_quad_subdivide.h) compiled for the host (tests/emu/quad_subdivide_emu.cpp) against its
numpy statement validate.refine_quad; the promise that the refined NLP constrains the points clearance(substeps = r) looked at; the statuses; the margin; the oracle's fine
solves of tests/golden/quad_refine_cases.npz; the public surface, the host build as a piece of the build rule and a stand-alone sanitizer run.  No GPU.  Trajectories,
comparison rules and the tolerance: tests/quad_refine_common.py."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT, golden
import packing as P
import clearance_common as K
import quad_shift_common as QS
import quad_refine_common as R
from obca_amd import validate as V


# ---------------------------------------------------------------- 1. the host build against validate.refine_quad
@pytest.mark.parametrize("N,r", R.SHAPES)
def test_host_pointer_form_matches_numpy(N, r):
    for i, c in enumerate(R.cases(N)):
        what = "N=%d r=%d instance %d" % (N, r, i)
        rc, Tsf, xf = R.emu_host(c, r)
        ref = V.refine_quad(c["x"], c["ts"], c["Ts"], r)
        assert rc == 0 and Tsf == c["Ts"] / r == ref["Ts"], what
        assert xf.shape == ref["x"].shape == (12, N * r + 1) and R.note("host build against numpy", xf, ref["x"]) <= R.TOL, what
        assert np.array_equal(xf[:, ::r], c["x"]), what      # s = 0 and the last node: the source's nodes, bit for bit
        rc2, Ts2, x2 = R.emu_host(c, r, rev=1)              # dealing the words to the lanes backwards: the same bits
        assert rc2 == 0 and Ts2 == Tsf and np.array_equal(x2, xf), what
        # no timeScale array means 1
        assert np.array_equal(R.emu_host(c, r, ts=None)[2], R.emu_host(c, r, ts=np.ones(N + 1))[2]), what
        assert R.note("host build against numpy", R.emu_host(c, r, ts=None)[2], V.refine_quad(c["x"], 1.0, c["Ts"], r)["x"]) <= R.TOL, what
        if r == 1:
            assert np.array_equal(xf, c["x"]) and Tsf == c["Ts"], what


@pytest.mark.parametrize("N,r", R.SHAPES)
def test_resident_form_writes_every_word_of_the_record(N, r):
    for i, c in enumerate(R.cases(N)[:4]):
        what = "N=%d r=%d instance %d" % (N, r, i)
        src = R.source(c, seed=i)
        st, pd = R.emu_record(src, r)
        assert st == 0, what
        R.check_record(src, r, 0.0, 0, pd, what)
        st2, pd2 = R.emu_record(src, r, rev=1)
        assert st2 == 0 and np.array_equal(pd2, pd), what
        # the trajectory is the host-pointer form's, bit for bit, with the solution's one t on every stage
        assert np.array_equal(pd[P.QPH_SIZE:], R.emu_host(c, r, ts=np.full(N + 1, src["t"]))[2].T.reshape(-1)), what
        assert pd[P.QPH_TWS] == src["t"] and pd[P.QPH_DWS] == 1.0 and src["prob"][P.QPH_DWS] == 0.0 and src["prob"][P.QPH_TWS] == 1.25, what
        if r == 1:      # factor 1, margin 0: the solved nodes and the header, bit for bit (timeWS and dual_ws are the status's)
            keep = np.setdiff1d(np.arange(P.QPH_SIZE), [P.QPH_TWS, P.QPH_DWS])
            assert np.array_equal(pd[keep], src["prob"][keep]) and np.array_equal(pd[P.QPH_SIZE:], np.ascontiguousarray(c["x"].T).reshape(-1)), what


# ---------------------------------------------------------------- 2. the promise
def _same_record(a, b, what):
    for idx, name in ((0, "min"), (2, "sample"), (3, "obstacle"), (4, "below"), (slice(8, 24), "per_obstacle")):
        assert np.array_equal(a[idx], b[idx]), (what, name, a[idx], b[idx])
    assert a[5] == b[5] and a[6] == b[6] == 0, what


@pytest.mark.parametrize("N,r", R.SHAPES)
def test_refined_nodes_are_the_points_clearance_sampled(N, r):
    """clearance(substeps = r) of a trajectory and clearance(substeps = 1) of its refinement at timeScale 1 and Ts / r: the same record bit for bit in min, sample, obstacle,
    below and per_obstacle -- through numpy, and through the host builds of both kernel texts"""
    for i, c in enumerate(R.cases(N)):
        for need in (0.0, 0.4):
            what = "N=%d r=%d instance %d need %g" % (N, r, i, need)
            xf = V.refine_quad(c["x"], c["ts"], c["Ts"], r)["x"]
            _same_record(V.quad_clearance(c["x"], c["ts"], c["Ts"], c["ob"], c["R"], r, need), V.quad_clearance(xf, 1, c["Ts"] / r, c["ob"], c["R"], 1, need), what + " (numpy)")
            rc, Tsf, xe = R.emu_host(c, r)
            fine = dict(c, N=N * r, Ts=Tsf, x=xe, ts=np.ones(N * r + 1))
            _same_record(K.emu_quad(c, r, need), K.emu_quad(fine, 1, need), what + " (host builds)")


def test_the_promise_on_the_solved_instances_of_the_fixture():
    g = golden("quad_refine_cases.npz"); n = 0
    from obca_amd import scenarios as S
    for N, B, r, _ in {(int(c[0]), int(c[1]), int(c[2]), 0) for c in g["cases"]}:
        bt = S.make_quad_batch(B, N)
        for i in range(B):
            x, t = g["N%d_x" % N][i], float(g["N%d_t" % N][i])
            xf = V.refine_quad(x, t, bt["Ts"], r)["x"]
            _same_record(V.quad_clearance(x, t, bt["Ts"], bt["ob"], bt["R"], r), V.quad_clearance(xf, 1, bt["Ts"] / r, bt["ob"], bt["R"], 1), (N, r, i))
            n += 1
    assert n == 16 + 16 + 8


# ---------------------------------------------------------------- 3. status
def test_status_marks_its_slot_and_reads_nothing_of_a_failed_iterate():
    N, r = 7, 4
    c = R.cases(N)[1]; src = R.source(c, seed=3); L = P.quad_layout(N)
    good = R.emu_record(src, r)

    def variant(flag=1.0, z=None, zat=None, up=None):
        s = dict(src); s["z"] = src["z"].copy() if z is None else z; s["prob"] = src["prob"].copy(); s["info"] = src["info"].copy(); s["info"][7] = flag
        if zat is not None:
            s["z"][zat[0]] = zat[1]
        if up is not None:
            s["prob"][P.QPH_SIZE + up[0]] = up[1]
        return s
    # exit flag 0: the interpolated uploaded start, timeWS and dual_ws as uploaded; the iterate may be all NaN -- nothing of it is read
    for z in (None, np.full(L["len"], np.nan), QS.iterate_of(N, np.full((12, N + 1), np.nan), np.nan)):
        st, pd = R.emu_record(variant(flag=0.0, z=z), r)
        assert st == 1
        e = R.check_record(src, r, 0.0, 1, pd, "exit flag 0")
        assert pd[P.QPH_TWS] == 1.25 and pd[P.QPH_DWS] == 0.0 and np.array_equal(e[P.QPH_SIZE:].reshape(-1, 12)[::r].reshape(-1), src["prob"][P.QPH_SIZE:])
    # exit flag 2 counts as solved
    st, pd = R.emu_record(variant(flag=2.0), r)
    assert st == 0 and np.array_equal(pd, good[1])
    # a non-finite number in x or t of the iterate
    for at in (L["x"], L["x"] + 12 * N + 11, L["x"] + 40, L["t"]):
        for v in (np.nan, np.inf, -np.inf):
            st, pd = R.emu_record(variant(zat=(at, v)), r)
            assert st == 1, (at, v)
            R.check_record(src, r, 0.0, 1, pd, "iterate[%d] = %r" % (at, v))
    # ... and nowhere else: u, lambda and the rest of the iterate are NaN already (iterate_of)
    assert np.isnan(src["z"][L["u"]]) and np.isnan(src["z"][L["lam"]]) and good[0] == 0
    # the uploaded start is not finite either: zeros, timeWS = 1, dual_ws = 1
    for up in (0, 12 * N + 11, 17):
        for kw in (dict(flag=0.0), dict(zat=(L["t"], np.nan))):
            st, pd = R.emu_record(variant(up=(up, np.nan), **kw), r, margin=0.01)
            assert st == -1
            s = variant(up=(up, np.nan)); R.check_record(dict(src, prob=s["prob"]), r, 0.01, -1, pd, "zero start")
            assert (pd[P.QPH_SIZE:] == 0).all() and pd[P.QPH_TWS] == 1.0 and pd[P.QPH_DWS] == 1.0
    # a solved instance does not look at its uploaded start
    st, pd = R.emu_record(variant(up=(5, np.nan)), r)
    assert st == 0 and np.array_equal(pd, good[1])
    # the host-pointer form: a non-finite input marks the instance, its outputs are NaN
    for field, idx in (("x", (2, 3)), ("x", (11, N)), ("ts", (N,)), ("ts", (0,))):
        a = np.array(c[field], float); a[idx] = np.nan
        rc, Tsf, xf = R.emu_host(dict(c, **{field: a}), r)
        assert rc == 1 and np.isnan(Tsf) and np.isnan(xf).all(), field
    rc, Tsf, xf = R.emu_host(dict(c, Ts=np.inf), r)
    assert rc == 1 and np.isnan(xf).all() and R.emu_host(c, r)[0] == 0


# ---------------------------------------------------------------- 4. margin
def test_margin_is_one_addition_to_the_radius_and_nothing_else():
    for (N, r), margin in zip(R.SHAPES, (0.005, 0.02, 1e-300, 0.1, 3.0, 0.25)):
        src = R.source(R.cases(N)[2], seed=N)
        st0, p0 = R.emu_record(src, r)
        st1, p1 = R.emu_record(src, r, margin)
        moved = src["prob"][P.QPH_R] + margin != src["prob"][P.QPH_R]      # (1e-300 is below half an ulp of R: one addition leaves the bits)
        assert st0 == st1 == 0 and np.flatnonzero(p0 != p1).tolist() == ([P.QPH_R] if moved else []) and moved == (margin > 1e-100)
        assert p1[P.QPH_R] == src["prob"][P.QPH_R] + margin and p0[P.QPH_R] == src["prob"][P.QPH_R]
    lib = R.emu()
    for args, msg in (((0, 5, 2, 0.0), b"n >= 1"), ((1, 5, 0, 0.0), b"factor"), ((1, 5, 33, 0.0), b"factor"), ((1, 0, 2, 0.0), b"OBCA_QUAD_NMAX"), ((1, 65, 2, 0.0), b"OBCA_QUAD_NMAX"),
                      ((1, 129, 1, 0.0), b"OBCA_QUAD_NMAX"), ((1, 5, 2, -1e-9), b"margin"), ((1, 5, 2, np.nan), b"margin"), ((1, 5, 2, np.inf), b"margin")):
        assert lib.emu_quad_subdivide_check_args(*args) == -1 and msg in lib.emu_quad_subdivide_last_error(), args
    for args in ((1, 64, 2, 0.0), (1, 128, 1, 0.5), (7, 4, 32, 0.0), (1, 1, 1, 0.0)):
        assert lib.emu_quad_subdivide_check_args(*args) == 0, args


# ---------------------------------------------------------------- 5. what the finer grid buys: the oracle's fine solves
PINNED = {      # case -> (samples under the true R, instances with such a sample, worst clearance against the true R), as tests/golden/make_quad_refine_cases.py prints them
    (20, 2, 0.0): (66, 16, -0.0758645), (20, 4, 0.0): (15, 11, -0.016121), (20, 4, 0.02): (0, 0, 0.00513089), (60, 2, 0.0): (17, 5, -0.00351492), (60, 2, 0.005): (0, 0, 0.000871226)}


@pytest.fixture(scope="module")
def Q():
    import oracle_quad
    oracle_quad.lib()
    return oracle_quad


def test_fixture_coarse_solutions_lose_the_separation_between_their_nodes():
    g = golden("quad_refine_cases.npz")
    assert int(g["substeps_coarse"]) == R.S_COARSE == 8 and [tuple(c) for c in g["cases"].tolist()] == [tuple(map(float, c)) for c in R.FIXTURE_CASES]
    for N, B, below, worst in ((20, 16, 247, -0.239954), (60, 8, 62, -0.0296448)):
        rec = g["N%d_rec" % N]
        assert (g["N%d_exitflag" % N] == 1).all() and rec.shape == (B, V.CLR_OUT) and (rec[:, 5] == N * 8 + 1).all()
        assert rec[:, 4].sum() == below and (rec[:, 4] > 0).all() and abs(rec[:, 0].min() - worst) < 1e-6 and (rec[:, 1] > -1e-6).all()      # held at the nodes, lost between them


@pytest.mark.parametrize("N,B,r,margin", R.FIXTURE_CASES)
def test_fixture_refined_solves_reproduce_the_stored_records(Q, N, B, r, margin):
    """the stored coarse solutions refined by the host build and solved by the oracle at its default options: exit flags, iteration counts and clearance records as
    tests/golden/make_quad_refine_cases.py stored them.  The two margin cases: every instance ends with exit flag 1, no sample under the true R, the minimum above 0."""
    from obca_amd import scenarios as S
    g = golden("quad_refine_cases.npz"); key = R.case_key(N, r, margin); bt = S.make_quad_batch(B, N)
    fine = [R.oracle_fine(Q, bt, i, g["N%d_x" % N][i], float(g["N%d_t" % N][i]), r, margin) for i in range(B)]
    ef = np.array([q["exitflag"] for q, _ in fine]); it = np.array([q["iters"] for q, _ in fine]); rec = np.array([c for _, c in fine])
    coarse = g["N%d_rec" % N]
    print("%s: exit flags %s, iterations %s (coarse %s); below %d -> %d, worst clearance against the true R %.6g -> %.6g"
          % (key, ef.tolist(), it.tolist(), g["N%d_iters" % N].tolist(), coarse[:, 4].sum(), rec[:, 4].sum(), coarse[:, 0].min(), rec[:, 0].min() + margin))
    assert np.array_equal(ef, g[key + "_exitflag"]) and np.array_equal(it, g[key + "_iters"]), (ef, it)
    assert np.array_equal(rec[:, [2, 3, 4, 5, 6]], g[key + "_rec"][:, [2, 3, 4, 5, 6]]) and np.abs(rec[:, :13] - g[key + "_rec"][:, :13]).max() < 1e-9
    assert (rec[:, 5] == N * 8 + 1).all()      # the same sample density as the coarse records
    below, flagged, worst = PINNED[(N, r, margin)]
    assert (rec[:, 4].sum(), (rec[:, 4] > 0).sum()) == (below, flagged) and abs(rec[:, 0].min() + margin - worst) < 1e-6
    assert rec[:, 4].sum() < coarse[:, 4].sum() and rec[:, 0].min() + margin > coarse[:, 0].min()
    if margin:
        assert (ef == 1).all() and (rec[:, 4] == 0).all() and rec[:, 0].min() + margin > 0


# ---------------------------------------------------------------- 6. the public surface and the build rule
def _kinds(hdr):
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S); kinds = {}
    for m in re.finditer(r"\bint\s*(obca_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        kinds[m.group(1)] = ["ptr" if "*" in p or "[" in p else ("double" if re.match(r"\s*(const\s+)?double\b", p) else "int") for p in m.group(2).split(",")]
    return kinds


def test_header_exports_python_and_julia_agree():
    from obca_amd import api, cabi
    import obca_amd
    protos = cabi.prototypes("obca_quad_subdivide.h")
    assert sorted(protos) == sorted(api.QUAD_SUBDIVIDE_EXPORTS) and len(protos) == 3 and not any("refine" in n for n in protos)
    assert not set(api.QUAD_SUBDIVIDE_EXPORTS) & (set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS) | set(api.REFINE_EXPORTS))
    assert len(cabi.prototypes("obca_hip.h")) == 44 and len(cabi.prototypes("obca_refine.h")) == 3
    hdr = open(os.path.join(ROOT, "include", "obca_quad_subdivide.h")).read()
    assert re.search(r"#define OBCA_QUAD_SUBDIVIDE_MAXFACTOR 32\b", hdr) and api.QUAD_SUBDIVIDE_MAXFACTOR == 32
    # what the library exports (no device: the symbol table)
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {e for e in exported if "subdivide" in e} == set(api.QUAD_SUBDIVIDE_EXPORTS)
    lib = api._load()
    for n, (_, argtypes) in protos.items():
        assert [type(a).__name__ for a in getattr(lib, n).argtypes] == [type(a).__name__ for a in argtypes], n
    assert len(lib.obca_quad_batch_subdivide_into.argtypes) == 7 and len(lib.obca_quadcopter_subdivide_batch.argtypes) == 9
    for f in ("quadcopter_refine_batch", "QUAD_REFINE_STATUS"):
        assert hasattr(obca_amd, f) and f in obca_amd.__all__
    assert all(hasattr(obca_amd.QuadBatch, m) for m in ("refine", "refine_ms")) and callable(V.refine_quad) and sorted(obca_amd.QUAD_REFINE_STATUS) == [-1, 0, 1]
    assert "clearance(need=-margin)" in obca_amd.QuadBatch.refine.__doc__
    # every ccall of the shim on these entry points against the header, parameter by parameter
    import test_julia_shim_cpu as J
    kinds = _kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCAHip.jl")).read()
    assert re.search(r"^const QSD = LIB$", src, flags=re.M) and "function refine(dst::QuadBatch" in src and "function QuadcopterRefine_batch(" in src
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), QSD\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
    assert {n for n, _ in calls} == set(kinds) == set(api.QUAD_SUBDIVIDE_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu")
    GXX = ["g++", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-misleading-indentation"]
    name = "quad_subdivide_emu"
    assert name in BF.EMU_PIECES and not set(BF.EMU_PIECES) & (set(BF.PIECES) | set(BF.TEST_PIECES) | set(BF.CHECK_PIECES)) and name not in BF.DEFAULT
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_quad_subdivide_emu.so")
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
    assert os.path.realpath(os.path.join(csrc, "obca_quad_subdivide.h")) in seen and os.path.realpath(os.path.join(csrc, "obca_quad_solver.h")) in seen
    assert not {os.path.realpath(os.path.join(csrc, h)) for h in ("obca_validate.h", "obca_clearance.h", "obca_refine.h", "obca_quad_shift.h")} & seen      # it states its own helper lines
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_quad_subdivide_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == GXX + ["-O1"] and argv[i + 2:] == [EMU + "/quad_subdivide_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # the kernel text is nothing the solve kernels use: no other header includes it
    for f in os.listdir(csrc):
        if f.endswith(".h") and f != "obca_quad_subdivide.h":
            assert "obca_quad_subdivide.h" not in open(os.path.join(csrc, f)).read(), f


def test_host_build_compiles_under_the_warning_flags(tmp_path):
    from obca_amd import buildflags as BF
    out = BF.build("quad_subdivide_emu", force=True, out=str(tmp_path / "libobca_quad_subdivide_emu.so"))
    assert os.path.getsize(out) > 0 and hasattr(C.CDLL(out), "emu_quad_subdivide_record")


# ---------------------------------------------------------------- 7. a stand-alone program under the host compiler's sanitizers
def test_stand_alone_program_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/emu/quad_subdivide_check_main.cpp: the kernel text for the host on the shapes above, every buffer from malloc with exactly the size the HIP host code gives it,
    instances addressed as the kernels address them.  A program of its own: nothing is loaded into this process."""
    from obca_amd import buildflags as BF
    exe = str(tmp_path / "quad_subdivide_check")
    flags = [f for f in BF.GXX if f not in ("-fPIC", "-shared")] + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(flags + ["-o", exe, os.path.join(ROOT, "tests", "emu", "quad_subdivide_check_main.cpp")], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "48 calls, 0 mismatches" in r.stdout and not r.stderr.strip(), (r.returncode, r.stdout[-500:], r.stderr[-3000:])


# ---------------------------------------------------------------- 8. record
def test_zz_record_of_the_largest_differences():
    test_host_pointer_form_matches_numpy(7, 4)      # (so that the record is not empty when this test runs alone)
    print("largest differences: " + ", ".join("%s %.3g" % kv for kv in sorted(R.WORST.items())))
    assert R.WORST and all(v <= R.TOL for v in R.WORST.values())
