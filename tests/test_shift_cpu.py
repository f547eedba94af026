"""Receding-horizon restart of the parking batch, without a GPU: the shift text of obca_amd/csrc/obca_shift.h compiled for the host (tests/emu/shift_emu.cpp) against the numpy
statement of the same rules (tests/shift_common.py).  The shift only copies, so every comparison is bit for bit; the iterate it reads is NaN wherever it may not look, the
records it writes hold a pattern wherever it may not write.  One test runs the host-built shift of an oracle solution through the host emulation of the solver."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import packing as P
import shift_common as SC
from conftest import ROOT

SETS = {"rows_2_2_1": [2, 2, 1], "rows_up_to_7": [2, 2, 1, 5, 6, 7, 7], "sixteen_obstacles": [3, 4] * 8, "one_obstacle": [2]}
WIDEST = (16, 64)                      # obstacles and rows of the widest instance a batch may hold: the record strides of a ragged batch are sized for it
HORIZONS = [1, 2, 63, 64, 65, 127, 128]


def _bits(a):
    return np.ascontiguousarray(a, float).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _pattern(n, salt):
    """n distinct finite words no copy can produce"""
    return -(1e6 * (salt + 1) + np.arange(n, dtype=float)) - 0.5


def _strides(N):
    return P.OB_HDR + 3 * (N + 1) + 5, P.layout(N, *WIDEST)["len"] + 3


def _instance(N, v, seed, dist=0):
    """one instance with random caller-level arrays (the shift copies: any numbers do) and rows of any length: dict with the arrays, the packed records in rows of the
    widest instance's strides, pattern / NaN wherever the shift may not write / read"""
    rng = np.random.default_rng(seed); v = np.asarray(v); nOb, M = len(v), int(v.sum()); N1 = N + 1
    s_prob, s_z = _strides(N)
    c = dict(N=N, v=v, nOb=nOb, M=M, xp=rng.normal(size=(4, N1)), up=rng.normal(size=(2, N)), lp=rng.uniform(0.1, 2, (M, N1)), npp=rng.uniform(0.1, 2, (4 * nOb, N1)),
             ref=rng.normal(size=(3, N1)), x0=rng.normal(size=4), A=rng.normal(size=(M, 2)) * rng.uniform(0.2, 50, (M, 1)), b=rng.normal(size=M), dist=dist)
    p = P.pack_problem(c["x0"], rng.normal(size=4), N, 0.6, 2.7, [3.7, 1, 1, 1], [-15, 15, 1, 10], v, c["A"], c["b"], *c["ref"], 0, dist=dist)
    prob = _pattern(s_prob, 1); prob[:len(p)] = p
    for lo, hi in ((P.PH["VOB"] + nOb, P.PH["ROFF"]), (P.PH["ROFF"] + nOb + 1, P.PH["DIST"]), (P.PH["A"] + 2 * M, P.PH["B"]), (P.PH["B"] + M, P.OB_HDR)):
        prob[lo:hi] = _pattern(hi - lo, 2)                    # the unused words of the header too
    c.update(prob=prob, z=SC.iterate_of(N, v, c["A"], c["xp"], c["up"], c["lp"], c["npp"], zlen=s_z), z0=_pattern(s_z, 3), tmp=np.full(s_z, np.nan))
    return c


def _expected(c, shift, x0_new):
    """(prob, z0) the statement asks for: X0, the reference and the primal part of z0 rewritten, every other word as it was"""
    N = c["N"]; N1 = N + 1
    st = SC.numpy_shift(N, shift, c["xp"], c["up"], c["lp"], c["npp"], *c["ref"], x0_new)
    L = P.layout(N, c["nOb"], c["M"])
    z0 = c["z0"].copy(); z0[:L["nprimal"]] = SC.start_of(N, c["v"], c["A"], st)[:L["nprimal"]]
    prob = c["prob"].copy(); prob[P.PH["X0"]:P.PH["X0"] + 4] = st["x0"]
    prob[P.OB_HDR:P.OB_HDR + 3 * N1] = np.concatenate([st["rx"], st["ry"], st["ryaw"]])
    return prob, z0, L


def _shifts(N):
    return sorted({0, 1, N - 1, N})


def test_layout_and_header_length_of_the_kernel_text_are_those_of_the_packing():
    for N, nOb, M in ((1, 1, 2), (30, 3, 5), (20, 7, 30), (128, 16, 64)):
        lay, hdr = SC.emu_layout(N, nOb, M)
        assert lay == P.layout(N, nOb, M) and hdr == P.OB_HDR


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("N", HORIZONS + [30])
def test_host_build_matches_the_statement_bit_for_bit(N, name):
    """every (N, shift) at the edges of the lane loops and of the clamps, both formulations, with and without a measured state, in records with the strides of a wider instance:
    the words the shift owns are the statement's, the result is finite although everything it may not read is NaN, every other word of z0 and of the problem record is
    untouched, and the scratch is used for the reference alone"""
    for shift in ([4] if N == 30 else _shifts(N)):
        for dist in (0, 1):
            c = _instance(N, SETS[name], seed=1000 * N + shift, dist=dist)
            for x0_new in (None, c["x0"] + 1.0):
                prob, z0, tmp = SC.emu_shift(N, shift, c["prob"], c["z"], c["z0"], c["tmp"], x0_new)
                eprob, ez0, L = _expected(c, shift, x0_new)
                tag = (N, shift, name, dist, x0_new is not None)
                assert _same(z0[0], ez0), tag + (np.flatnonzero(_bits(z0[0]) != _bits(ez0))[:8].tolist(),)
                assert _same(prob[0], eprob), tag + (np.flatnonzero(_bits(prob[0]) != _bits(eprob))[:8].tolist(),)
                assert np.isfinite(z0[0, :L["nprimal"]]).all() and np.isfinite(prob[0]).all(), tag
                assert z0[0, L["t"]] == 1.0 and not z0[0, L["sl"]:L["nprimal"]].any(), tag             # t = 1; sl (ParkingDist: the norm-row slack), so, ss = 0
                assert np.isnan(tmp[0, 3 * (N + 1):]).all(), tag
                if x0_new is not None:
                    assert _same(z0[0, L["x"]:L["x"] + 4], x0_new) and _same(prob[0, P.PH["X0"]:P.PH["X0"] + 4], x0_new), tag


@pytest.mark.parametrize("name", sorted(SETS))
def test_shift_by_zero_reproduces_the_solution(name):
    for N in (1, 30, 64, 128):
        c = _instance(N, SETS[name], seed=N, dist=N % 2)
        prob, z0, _ = SC.emu_shift(N, 0, c["prob"], c["z"], c["z0"], c["tmp"])
        L = P.layout(N, c["nOb"], c["M"])
        for a, b in ((L["x"], L["t"]), (L["lam"], L["sl"])):                     # x, u and lambda, mu: word for word
            assert _same(z0[0, a:b], c["z"][a:b]), (N, name, a)
        assert z0[0, L["t"]] == 1.0 and not z0[0, L["sl"]:L["nprimal"]].any()
        keep = c["prob"].copy(); keep[P.PH["X0"]:P.PH["X0"] + 4] = c["xp"][:, 0]                      # X0 = stage 0 of the solution; the reference stays
        assert _same(prob[0], keep), (N, name)


@pytest.mark.parametrize("name", sorted(SETS))
def test_two_shifts_compose(name):
    """shift by a, the result re-packed as the iterate of the next call, then by b: the same words as one shift by a + b"""
    for N, a, b in ((30, 2, 5), (30, 0, 30), (64, 63, 1), (65, 1, 63), (128, 64, 64), (2, 1, 1), (1, 1, 0)):
        c = _instance(N, SETS[name], seed=7 * N + a)
        L = P.layout(N, c["nOb"], c["M"])
        p1, z1, _ = SC.emu_shift(N, a, c["prob"], c["z"], c["z0"], c["tmp"])
        again = np.full_like(c["z"], np.nan)
        for lo, hi in ((L["x"], L["t"]), (L["lam"], L["sl"])):
            again[lo:hi] = z1[0, lo:hi]
        p2, z2, _ = SC.emu_shift(N, b, p1, again, c["z0"], c["tmp"])
        p3, z3, _ = SC.emu_shift(N, a + b, c["prob"], c["z"], c["z0"], c["tmp"])
        assert _same(z2, z3) and _same(p2, p3), (N, a, b, name)


def _ragged(N, seed):
    cs = [_instance(N, SETS[n], seed=seed + j) for j, n in enumerate(("one_obstacle", "rows_up_to_7", "sixteen_obstacles", "rows_2_2_1"))]
    return cs, [np.stack([c[k] for c in cs]) for k in ("prob", "z", "z0", "tmp")]


def test_a_ragged_batch_gives_every_instance_its_own_strides_of_lambda_and_mu():
    """instances of 1, 7, 16 and 3 obstacles side by side in records of one stride: each comes out as it does alone"""
    for N, shift in ((20, 3), (64, 5), (65, 64)):
        cs, (prob, z, z0, tmp) = _ragged(N, seed=N)
        x0n = np.stack([c["x0"] for c in cs]) - 2.0
        p, w, _ = SC.emu_shift(N, shift, prob, z, z0, tmp, x0n)
        for j, c in enumerate(cs):
            eprob, ez0, _ = _expected(c, shift, x0n[j])
            assert _same(w[j], ez0) and _same(p[j], eprob), (N, shift, j)


def test_a_nan_in_one_instance_stays_in_that_instance():
    N, shift = 30, 4
    cs, (prob, z, z0, tmp) = _ragged(N, seed=5)
    L = P.layout(N, cs[1]["nOb"], cs[1]["M"])
    p0, w0, _ = SC.emu_shift(N, shift, prob, z, z0, tmp)
    bad = z.copy(); bad[1, L["x"] + 4 * 9 + 2] = np.nan; bad[1, L["mu"] + 11] = np.inf
    p1, w1, _ = SC.emu_shift(N, shift, prob, bad, z0, tmp)
    for j in (0, 2, 3):
        assert _same(w1[j], w0[j]) and _same(p1[j], p0[j]), j
    assert np.isnan(w1[1, L["x"] + 4 * (9 - shift) + 2]) and not np.isfinite(w1[1, :L["nprimal"]]).all() and np.isfinite(w0[1, :L["nprimal"]]).all()
    assert _same(p1[1], p0[1])                                                   # (stage `shift` itself was finite: X0 and the reference are unchanged)


def test_result_does_not_depend_on_how_the_items_are_dealt_to_the_lanes():
    for N, shift in ((1, 1), (30, 4), (63, 1), (64, 63), (65, 64), (128, 127)):
        cs, (prob, z, z0, tmp) = _ragged(N, seed=N + 1)
        a = SC.emu_shift(N, shift, prob, z, z0, tmp, rev=0); b = SC.emu_shift(N, shift, prob, z, z0, tmp, rev=1)
        assert all(_same(x, y) for x, y in zip(a, b)), (N, shift)


def test_the_statement_in_the_callers_scaling_is_what_the_packed_records_hold():
    """shifted_problem (the statement on a download, lambda in the caller's row scaling) against the records the host build wrote, unpacked: rows whose lengths are powers of
    two make the scaling of lambda exact both ways, so this too is bit for bit -- and a lambda left unscaled would be off by the row length"""
    N, shift = 30, 4
    c = _instance(N, SETS["rows_2_2_1"], seed=3)
    s = np.array([4.0, 0.25, 128.0, 8.0, 0.5])
    c["A"] = np.array([[1.0, 0], [0, -1.0], [-1.0, 0], [0, 1.0], [1.0, 0]]) * s[:, None]
    assert np.array_equal(P.row_lengths(c["A"]), s)
    c["z"] = SC.iterate_of(N, c["v"], c["A"], c["xp"], c["up"], c["lp"], c["npp"], zlen=len(c["z"]))
    L = P.layout(N, c["nOb"], c["M"])
    assert _same(c["z"][L["lam"]:L["mu"]].reshape(N + 1, -1), c["lp"].T * s[None, :])                # the iterate holds lambda of unit rows
    out = dict(xp=[c["xp"]], up=[c["up"]], lp=[c["lp"]], np=[c["npp"]])
    for x0_new in (None, c["x0"]):
        prob, z0, _ = SC.emu_shift(N, shift, c["prob"], c["z"], c["z0"], c["tmp"], x0_new)
        got = SC.unpack_start(N, c["v"], c["A"], z0[0], prob[0]); want = SC.shifted_problem(N, shift, out, 0, *c["ref"], x0_new)
        for k in want:
            assert _same(got[k], want[k]), k
        assert got["t"] == 1.0 and not got["sl"].any()


# ---------------------------------------------------------------- the shifted start through the solver
@pytest.mark.parametrize("dist", [0, 1], ids=["signed_dist", "dist"])
def test_host_built_shift_of_an_oracle_solution_restarts_like_the_oracle(oracle, emu, dist):
    """rows 2, 2, 1, 5, 6, 7, 7 at N = 20, shift 3: the oracle's solution, packed, through the host build of the shift and the host emulation of the solver, against the oracle
    started from the statement's shifted problem with the same warm-restart values -- the oracle's exit flag and iterations, its point at the bar of
    test_emu_cpu.py::test_emu_wide_obstacles_match_oracle"""
    from obca_amd import scenarios as S
    from test_emu_cpu import copy_opts
    N, shift, i = 20, 3, 3
    bt = S.make_mixed_batch(24, N, seed=11, rows=(5, 8), max_extra=4)
    v = np.ravel(bt["vOb"][i]); A, b = bt["A"][i], bt["b"][i]
    assert v.tolist() == [2, 2, 1, 5, 6, 7, 7]
    nOb, M = len(v), int(v.sum()); L = P.layout(N, nOb, M)
    xWS = bt["xWS"][i].copy(); xWS[0] = bt["x0"][i]
    fixed = (N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], v, A, b)
    r1 = oracle.parking_signed_dist(bt["x0"][i], bt["xF"][i], *fixed, xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, bt["uWS"][i], dist=dist)
    assert r1["exitflag"] == 1
    oo = oracle.default_opts(); oo.mu_init = oo.bound_push = oo.bound_frac = 1e-4
    st = SC.shifted_problem(N, shift, {k: [r1[k]] for k in ("xp", "up", "lp", "np")}, 0, xWS[:, 0], xWS[:, 1], xWS[:, 2])
    r2 = oracle.parking_signed_dist(st["x0"], bt["xF"][i], *fixed, st["rx"], st["ry"], st["ryaw"], 0, st["xWS"], st["uWS"], st["lWS"], st["nWS"], opts=oo, dist=dist)
    assert r2["exitflag"] == 1
    prob = P.pack_problem(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], v, A, b, xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, dist=dist)
    z = SC.iterate_of(N, v, A, r1["xp"], r1["up"], r1["lp"], r1["np"])
    p2, z0, _ = SC.emu_shift(N, shift, prob, z, np.zeros(L["len"]), np.full(L["len"], np.nan))      # (behind the primal part a start holds zeros, as an upload leaves them)
    zo = np.zeros(L["len"]); info = np.zeros(8); eo = copy_opts(oo)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    emu.emu_solve(C.c_int(N), dp(np.ascontiguousarray(p2[0])), dp(np.ascontiguousarray(z0[0])), C.c_int(L["len"]), C.byref(eo), dp(zo), dp(info))
    xp, up, t, lp, npp, sl = P.unpack_solution(zo, N, nOb, M, A=A)
    assert int(info[7]) == r2["exitflag"] and int(info[0]) == r2["status"] and int(info[1]) == r2["iters"], (info.tolist(), r2["iters"])
    assert np.abs(xp - r2["xp"]).max() < 1e-7 and np.abs(up - r2["up"]).max() < 1e-7 and abs(t - r2["t"]) < 1e-9
    assert np.abs(lp - r2["lp"]).max() < 1e-5
    assert np.array_equal(xp[:, 0], r1["xp"][:, shift])                          # X0: stage `shift` of the first solution


# ---------------------------------------------------------------- build and call site
def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu"); name = "shift_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_shift_emu.so")
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
    for h in ("obca_shift.h", "obca_solver.h", "obca_model.h"):
        assert os.path.realpath(os.path.join(csrc, h)) in seen, h
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_shift_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/shift_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)


def test_the_kernel_is_the_call_and_the_entry_point_carries_both_guards():
    csrc = os.path.join(ROOT, "obca_amd", "csrc")
    for f in os.listdir(csrc):      # nothing in csrc includes the shift text but the one line of the library
        if f.endswith((".h", ".hip", ".cpp")) and f != "obca_hip.hip":
            assert not re.search(r'#\s*include\s*"obca_shift.h"', open(os.path.join(csrc, f)).read()), f
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    assert hip.count('#include "obca_shift.h"') == 1
    txt = re.sub(r"//.*", "", open(os.path.join(csrc, "obca_shift.h")).read())
    assert re.findall(r'#include\s*"([^"]+)"', txt) == ["obca_solver.h"] and "atomic" not in txt and txt.count("SYNC()") == 1 and "threadIdx" not in txt
    m = re.search(r"void obca_shift_kernel\(([^)]*)\)\s*\{(.*?)\n\}", hip, flags=re.S)
    body = re.sub(r"//.*", "", m.group(2))
    assert "shf::shift_instance(" in body and "for (" not in body and "__syncthreads" not in body
    assert re.search(r"__launch_bounds__\(OB_NT\)\s*void obca_shift_kernel", hip) and "hipLaunchKernelGGL(obca_shift_kernel, dim3(bt->B), dim3(OB_NT)," in hip      # one wavefront: the lanes PAR deals to
    m = re.search(r"int obca_batch_shift_warm_start\(obca_batch \*bt, int shift, const double \*x0_new\) \{(.*?)\n\}", hip, flags=re.S)
    fn = m.group(1); launch = fn.index("hipLaunchKernelGGL")
    for refusal in ("nothing uploaded", "shift out of range 0..N", "nothing has been solved since the last upload or shift", "non-finite entry in x0_new"):
        assert 0 <= fn.find("obca_batch_shift_warm_start: " + refusal) < launch, refusal      # refused before anything is queued
    hdr = open(os.path.join(ROOT, "include", "obca_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int obca_batch_shift_warm_start\(obca_batch \*bt, int shift, const double \*x0_new\);", hdr, flags=re.S)
    assert m and "nothing has been solved since the last upload or shift" in m.group(1) and "non-finite" in m.group(1) and "exit flag" in m.group(1)
