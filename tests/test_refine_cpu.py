"""Refinement of solved parking instances onto a finer horizon (obca_amd/csrc/obca_refine.h) compiled for the host (tests/emu/refine_emu.cpp) against its numpy statement
validate.refine_parking; the fallbacks; the shared argument refusals; the oracle's fine solves of tests/golden/refine_cases.npz; solve -> refine -> solve through the host builds against the oracle; the public surface and the host build as a
piece of the build rule.  No GPU.  Trajectories, comparison rules and the derivation of the tolerance: tests/refine_common.py."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT, golden
import packing as P
import refine_common as R
from obca_amd import validate as V


# ---------------------------------------------------------------- 1. the host build against validate.refine_parking
@pytest.mark.parametrize("N,r", R.SHAPES)
def test_host_pointer_form_matches_numpy_and_the_clearance_samples(N, r):
    for bi, batch in enumerate(R.cases(N)):
        for i, c in enumerate(batch):
            what = "N=%d r=%d batch %d instance %d" % (N, r, bi, i)
            rc, Tsf, xf, uf = R.emu_host(c, r)
            ref = V.refine_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], r)
            assert rc == 0 and Tsf == c["Ts"] / r == ref["Ts"], what
            assert np.array_equal(uf, ref["u"]) and np.array_equal(uf, np.repeat(c["u"], r, axis=1)), what
            assert R.close_x(xf, ref["x"]), (what, np.abs(xf - ref["x"]).max())
            assert np.array_equal(xf[:, ::r], c["x"]) and np.array_equal(xf[:, -1], c["x"][:, -1]), what      # s = 0 and the last node: the source's nodes, bit for bit
            # the refined NLP constrains the poses clearance(substeps = r) sampled
            assert R.close_x(xf[:3].T, V.parking_samples(c["x"], c["u"], c["ts"], c["Ts"], c["L"], r)), what
            # dealing the nodes to the lanes backwards: the same bits
            rc2, Ts2, x2, u2 = R.emu_host(c, r, rev=1)
            assert rc2 == 0 and Ts2 == Tsf and np.array_equal(x2, xf) and np.array_equal(u2, uf), what
            if np.ptp(c["ts"]) == 0:      # no timeScale array: 1
                assert np.array_equal(R.emu_host(c, r, ts=None)[2], xf), what
            if r == 1:
                assert np.array_equal(xf, c["x"]) and np.array_equal(uf, c["u"]) and Tsf == c["Ts"], what


@pytest.mark.parametrize("N,r", R.SHAPES)
def test_resident_form_writes_every_word_of_the_record_and_the_row(N, r):
    seen = set()
    for bi, batch in enumerate(R.cases(N)):
        for i, c in enumerate(batch[:4]):
            src = R.source(c, seed=10 * bi + i, fixTime=(bi + i) % 2 if bi == 1 else 0, dist=int(bi == 2))
            seen.add((src["nOb"], src["M"]))
            for duals in (0, 1):
                what = "N=%d r=%d batch %d instance %d duals %d" % (N, r, bi, i, duals)
                st, pd, zd = R.emu_record(src, r, duals)
                assert st == 0, what
                R.check_record(src, r, duals, 0, pd, zd, what)
                st2, pd2, zd2 = R.emu_record(src, r, duals, rev=1)
                assert st2 == 0 and np.array_equal(pd2, pd) and np.array_equal(zd2, zd), what
                # the primal part is the host-pointer form's, bit for bit: both run the same instance function
                ld = P.layout(N * r, src["nOb"], src["M"]); t = 1.0 if src["fix"] else src["parts"]["sol"][2]
                _, _, xf, uf = R.emu_host(c, r, ts=np.full(N + 1, t))
                assert np.array_equal(zd[ld["x"]:ld["x"] + xf.size], xf.T.reshape(-1)) and np.array_equal(zd[ld["u"]:ld["u"] + uf.size], uf.T.reshape(-1)), what
                if r == 1:      # a bit-equal copy of header, reference, x, u, (lam, mu)
                    ls = src["lay"]; n = ls["sl"] if duals else ls["lam"]
                    assert np.array_equal(pd, src["prob"]) and np.array_equal(np.delete(zd[:n], ls["t"]), np.delete(src["z"][:n], ls["t"])) and zd[ls["t"]] == 1.0, what
    assert len(seen) >= 3


# ---------------------------------------------------------------- 2. fallbacks
def test_fallbacks_mark_their_slot_and_leave_the_neighbours():
    N, r = 5, 3; batch = R.cases(N)[2]
    srcs = [R.source(c, seed=i) for i, c in enumerate(batch[:3])]
    good = [[R.emu_record(s, r, d) for d in (0, 1)] for s in srcs]
    lay = srcs[1]["lay"]

    def variant(z=None, z0=None, flag=1.0):
        s = dict(srcs[1]); s["z"] = srcs[1]["z"].copy(); s["z0"] = srcs[1]["z0"].copy(); s["info"] = srcs[1]["info"].copy(); s["info"][7] = flag
        for key, at in (("z", z), ("z0", z0)):
            if at is not None:
                s[key][at[0]] = at[1]
        return s
    # exit flag 0: the refinement of the start iterate, with duals its multipliers
    for duals in (0, 1):
        st, pd, zd = R.emu_record(variant(flag=0.0), r, duals)
        assert st == 1
        R.check_record(srcs[1], r, duals, 1, pd, zd, "exit flag 0, duals %d" % duals)
    # a non-finite number in x, u, t of the iterate; in lam / mu only where they are carried
    for name, at in (("x", lay["x"] + 7), ("u", lay["u"] + 2 * N - 1), ("t", lay["t"]), ("x", lay["x"])):
        for v in (np.nan, np.inf, -np.inf):
            for duals in (0, 1):
                st, pd, zd = R.emu_record(variant(z=(at, v)), r, duals)
                assert st == 1, (name, v, duals)
                R.check_record(srcs[1], r, duals, 1, pd, zd, "%s = %r, duals %d" % (name, v, duals))
    for at in (lay["lam"] + 3, lay["mu"] + 4 * srcs[1]["nOb"] * (N + 1) - 1):
        assert R.emu_record(variant(z=(at, np.nan)), r, 1)[0] == 1
        st, pd, zd = R.emu_record(variant(z=(at, np.nan)), r, 0)
        assert st == 0 and np.array_equal(zd, good[1][0][2]) and np.array_equal(pd, good[1][0][1])
    # the start iterate is not finite either: the zero slot -- what an upload without a warm start leaves
    for z0at in (lay["x"] + 1, lay["u"], lay["t"]):
        for duals in (0, 1):
            st, pd, zd = R.emu_record(variant(flag=0.0, z0=(z0at, np.nan)), r, duals)
            assert st == -1
            R.check_record(srcs[1], r, duals, -1, pd, zd, "zero slot")
            ld = P.layout(N * r, srcs[1]["nOb"], srcs[1]["M"])
            assert (np.delete(zd, ld["t"]) == 0).all() and zd[ld["t"]] == 1.0
    assert R.emu_record(variant(flag=0.0, z0=(lay["lam"], np.nan)), r, 1)[0] == -1 and R.emu_record(variant(flag=0.0, z0=(lay["lam"], np.nan)), r, 0)[0] == 1
    # instances share nothing: the neighbours come back bit for bit
    for s, g in zip(srcs, good):
        for d in (0, 1):
            st, pd, zd = R.emu_record(s, r, d)
            assert st == g[d][0] == 0 and np.array_equal(pd, g[d][1]) and np.array_equal(zd, g[d][2])
    # the host-pointer form: a non-finite input marks the instance, its outputs are NaN
    c = batch[1]
    for field, idx in (("x", (2, 3)), ("u", (1, N - 1)), ("ts", (N,)), ("ts", (0,))):
        a = np.array(c[field], float); a[idx] = np.nan
        rc, Tsf, xf, uf = R.emu_host(dict(c, **{field: a}), r)
        assert rc == 1 and np.isnan(Tsf) and np.isnan(xf).all() and np.isnan(uf).all(), field
    rc, Tsf, xf, uf = R.emu_host(dict(c, Ts=np.inf), r)
    assert rc == 1 and np.isnan(xf).all()
    assert R.emu_host(c, r)[0] == 0


# ---------------------------------------------------------------- 3. the shared refusals
def test_argument_refusals():
    lib = R.emu()
    for args, msg in (((0, 5, 2, 0), b"n >= 1"), ((-3, 5, 2, 0), b"n >= 1"), ((1, 5, 0, 0), b"factor"), ((1, 5, 33, 0), b"factor"), ((1, 5, -1, 0), b"factor"),
                      ((1, 0, 2, 0), b"OBCA_NMAX"), ((1, 65, 2, 0), b"OBCA_NMAX"), ((1, 129, 1, 0), b"OBCA_NMAX"), ((1, 5, 26, 0), b"OBCA_NMAX"), ((1, 5, 2, 2), b"duals"), ((1, 5, 2, -1), b"duals")):
        assert lib.emu_refine_check_args(*args) == -1 and msg in lib.emu_refine_last_error(), args
    for args in ((1, 64, 2, 0), (1, 128, 1, 1), (7, 4, 32, 1), (1, 1, 1, 0)):
        assert lib.emu_refine_check_args(*args) == 0, args
    x = np.zeros(64); out = np.full(64, R.SENTINEL)
    assert lib.emu_refine_host(5, 33, 0.5, 2.7, R.dp(x), R.dp(x), None, 0, R.dp(out), R.dp(out), R.dp(out)) == -1 and (out == R.SENTINEL).all()
    assert lib.emu_refine_host(5, 2, 0.5, 2.7, None, R.dp(x), None, 0, R.dp(out), R.dp(out), R.dp(out)) == -1 and b"NULL" in lib.emu_refine_last_error()


# ---------------------------------------------------------------- 4. what the finer grid buys: the oracle's fine solves
def test_fixture_finer_grid_restores_the_clearance_and_carried_duals_cost_fewer_iterations():
    """tests/golden/make_refine_cases.py: make_batch(BACKWARDS, 8, 30) instances 0 .. 5 solved by the oracle at N = 30, refined x 2 by validate.refine_parking, solved again at
    N = 60 from that start with DualMultWS duals at the default options (`ws`) and with the carried multipliers at mu_init = bound_push = bound_frac = 1e-4 (`carry`).
    Iterations in total, as the script prints them: ws 167, carry 94."""
    g = golden("refine_cases.npz"); N, r = int(g["N"]), int(g["factor"]); n = len(g["x"])
    assert (N, r, n, int(g["substeps_coarse"]), int(g["substeps_fine"])) == (30, 2, 6, 8, 4) and (g["exitflag"] == 1).all()
    from obca_amd import scenarios as S
    bt = S.make_batch(S.BACKWARDS, 8, N)
    for i in range(n):      # the stored refinement is the numpy statement's, and the host build's
        ref = bt["xWS"][i].copy(); ref[0] = bt["x0"][i]
        f = V.refine_parking(g["x"][i], g["u"][i], g["t"][i], bt["Ts"][i], bt["L"], r, ref=ref[:, :3].T, lam=g["lam"][i], mu=g["mu"][i])
        for k, a in (("fx", f["x"]), ("fu", f["u"]), ("fref", f["ref"]), ("flam", f["lam"]), ("fmu", f["mu"])):
            assert np.array_equal(g[k][i], a), (i, k)
        c = dict(N=N, Ts=float(bt["Ts"][i]), L=bt["L"], x=g["x"][i], u=g["u"][i], ts=np.full(N + 1, g["t"][i]))
        rc, Tsf, xf, uf = R.emu_host(c, r)
        assert rc == 0 and Tsf == g["fTs"][i] and np.array_equal(uf, g["fu"][i]) and R.close_x(xf, g["fx"][i])
    coarse = g["rec"]
    assert (coarse[:, 1] >= 0.05 - 1e-6).all() and coarse[2, 4] == 7 and abs(coarse[2, 0] - 0.024412) < 1e-6      # instance 2: the finding of clearance_cases.npz
    lost = coarse[:, 4] > 0
    assert lost[2] and lost.sum() >= 2
    for mode in ("ws", "carry"):
        rec = g[mode + "_rec"]
        assert (g[mode + "_exitflag"] == 1).all(), mode
        assert (rec[:, 1] >= 0.05 - 1e-6).all(), (mode, rec[:, 1])
        assert (rec[lost, 4] == 0).all(), (mode, rec[:, 4])
        assert (rec[:, 5] == N * r * 4 + 1).all() and (coarse[:, 5] == N * 8 + 1).all()      # the same sample density
        assert np.abs(g[mode + "_t"] - g["t"]).max() < 1e-6
    assert abs(g["ws_rec"][2, 0] - 0.0531515) < 1e-6 and abs(g["ws_rec"][2, 1] - 0.0555205) < 1e-6
    ws, carry = int(g["ws_iters"].sum()), int(g["carry_iters"].sum())
    assert (ws, carry) == (167, 94), "iterations of the fine solves, instances 0 .. 5: DualMultWS start %d, carried multipliers %d" % (ws, carry)
    assert carry < ws, "iterations of the fine solves, instances 0 .. 5: DualMultWS start %d, carried multipliers %d" % (ws, carry)


@pytest.mark.parametrize("which,instances", [("backwards", (11, 2)), ("mixed", (0, 3))])
def test_resident_pipeline_through_the_host_builds_matches_the_oracle_from_the_same_start(oracle, which, instances):
    """solve, refine x 2, solve -- the kernel texts of the solver and of the refinement compiled for the host, as a resident batch chains them -- against the oracle started
    from the numpy statement's refinement of the same coarse solution: the same exit flag and iteration count in both modes, the trajectory within 1e-6 (TOL_X of
    tests/test_gpu_parity.py), lambda in the caller's row scaling within 1e-6 max(1, |lambda|).  tests/test_gpu_refine.py asks the device for the same."""
    from obca_amd import scenarios as S
    bt = S.make_batch(S.BACKWARDS, 16, 30) if which == "backwards" else S.make_mixed_batch(12, 20, min_obstacles=1, rows=(3, 8), max_rows=64)
    N, r = bt["N"], 2
    for i in instances:
        for duals in (0, 1):
            coarse, st, fine, f = R.emu_pipeline(bt, i, r, duals)
            assert coarse["exitflag"] == 1 and st == 0
            oo = oracle.default_opts()
            if duals:
                oo.mu_init = oo.bound_push = oo.bound_frac = 1e-4
            q = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], N * r, f["Ts"], bt["L"], bt["ego"], bt["XYbounds"], f["vOb"], f["A"], f["b"], f["ref"][0], f["ref"][1], f["ref"][2], 0,
                                           f["x"].T, f["u"].T, *((f["lam"].T, f["mu"].T) if duals else (None, None)), opts=oo)
            what = "%s instance %d duals %d: host builds exit flag %d, %d iterations; oracle %d, %d" % (which, i, duals, fine["exitflag"], fine["iters"], q["exitflag"], q["iters"])
            assert fine["exitflag"] == q["exitflag"] == 1 and fine["iters"] == q["iters"], what
            assert max(np.abs(fine["x"] - q["xp"]).max(), np.abs(fine["u"] - q["up"]).max()) < 1e-6 and abs(fine["t"] - q["timeScale"][0]) < 1e-9, what
            assert np.abs(fine["lp"] - q["lp"]).max() < 1e-6 * max(1.0, np.abs(q["lp"]).max()) and np.abs(fine["np"] - q["np"]).max() < 1e-6 * max(1.0, np.abs(q["np"]).max()), what
            if duals:
                assert fine["iters"] < coarse["iters"], what      # the carried multipliers with the warm-restart options: cheaper than the coarse solve itself


# ---------------------------------------------------------------- 5. the public surface and the build rule
def _kinds(hdr):
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S); kinds = {}
    for m in re.finditer(r"\bint\s*(obca_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        kinds[m.group(1)] = ["ptr" if "*" in p or "[" in p else ("double" if re.match(r"\s*(const\s+)?double\b", p) else "int") for p in m.group(2).split(",")]
    return kinds


def test_header_exports_python_and_julia_agree():
    from obca_amd import api, cabi
    import obca_amd
    protos = cabi.prototypes("obca_refine.h")
    assert sorted(protos) == sorted(api.REFINE_EXPORTS) and len(protos) == 3
    assert not set(api.REFINE_EXPORTS) & (set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS))
    assert len(cabi.prototypes("obca_hip.h")) == 44
    hdr = open(os.path.join(ROOT, "include", "obca_refine.h")).read()
    assert re.search(r"#define OBCA_REFINE_MAXFACTOR 32\b", hdr) and api.REFINE_MAXFACTOR == 32
    # what the library exports (no device: the symbol table)
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert set(api.REFINE_EXPORTS) <= exported and {e for e in exported if "refine" in e} == set(api.REFINE_EXPORTS)
    lib = api._load()
    assert [type(a).__name__ for a in lib.obca_batch_refine_into.argtypes] == [type(a).__name__ for a in protos["obca_batch_refine_into"][1]] and len(lib.obca_parking_refine_batch.argtypes) == 12
    for f in ("parking_refine_batch", "REFINE_STATUS"):
        assert hasattr(obca_amd, f) and f in obca_amd.__all__
    assert all(hasattr(obca_amd.Batch, m) for m in ("refine", "refine_ms")) and callable(V.refine_parking) and sorted(obca_amd.REFINE_STATUS) == [-1, 0, 1]
    # every ccall of the shim on the refine entry points against the header, parameter by parameter
    import test_julia_shim_cpu as J
    kinds = _kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCAHip.jl")).read()
    assert re.search(r"^const RFN = LIB$", src, flags=re.M) and "function refine(" in src and "function ParkingRefine_batch(" in src
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), RFN\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
    assert {n for n, _ in calls} == set(kinds) == set(api.REFINE_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu")
    GXX = ["g++", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-misleading-indentation"]
    assert "refine_emu" in BF.EMU_PIECES and not set(BF.EMU_PIECES) & (set(BF.PIECES) | set(BF.TEST_PIECES) | set(BF.CHECK_PIECES)) and "refine_emu" not in BF.DEFAULT
    p = BF.EMU_PIECES["refine_emu"]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_refine_emu.so")
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
    assert os.path.realpath(os.path.join(csrc, "obca_refine.h")) in seen and os.path.realpath(os.path.join(csrc, "obca_validate.h")) in seen
    assert os.path.realpath(os.path.join(csrc, "obca_clearance.h")) not in seen      # park_step comes from obca_validate.h
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_refine_emu.so")
    assert BF.build("refine_emu", force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == GXX + ["-O1"] and argv[i + 2:] == [EMU + "/refine_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # the kernel text is nothing the solve kernels use: no other header includes it
    for f in os.listdir(csrc):
        if f.endswith(".h") and f != "obca_refine.h":
            assert "obca_refine.h" not in open(os.path.join(csrc, f)).read(), f
    assert C.sizeof(C.c_double) == 8


# ---------------------------------------------------------------- 6. warnings are errors
def test_host_build_compiles_under_the_warning_flags(tmp_path):
    from obca_amd import buildflags as BF
    assert "-Werror" in BF.GXX and "-Wall" in BF.GXX and "-Wextra" in BF.GXX
    out = BF.build("refine_emu", force=True, out=str(tmp_path / "libobca_refine_emu.so"))
    assert os.path.getsize(out) > 0 and hasattr(C.CDLL(out), "emu_refine_record")
