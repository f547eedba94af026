"""Clearance between the nodes (obca_amd/csrc/obca_clearance.h) compiled for the host (tests/emu/clearance_emu.cpp) against its independent statement -- numpy
validate.parking_samples + the oracle's DualMultWS on the sample poses + the clamp; numpy validate.quad_clearance --, the solved trajectories of
tests/golden/clearance_cases.npz that pass at their nodes and touch an obstacle between them, non-finite input, argument errors, order independence, and the
host build as a piece of the build rule.  No GPU.  Trajectories, comparison rules and the derivation of the tolerances: tests/clearance_common.py."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from conftest import ROOT, golden
import clearance_common as K
from obca_amd import validate as V

NEED = V.DMIN


# ---------------------------------------------------------------- 1. against the independent statement
@pytest.mark.parametrize("N,S_", K.SHAPES)
def test_parking_record_matches_samples_plus_oracle_distance(oracle, N, S_):
    seen_nob = set()
    for bi, batch in enumerate(K.parking_cases(N)):
        vm = K.vmax_of(batch)
        for i, c in enumerate(batch):
            what = "N=%d S=%d batch %d instance %d" % (N, S_, bi, i); seen_nob.add(len(c["vOb"]))
            rec = K.emu_parking(c, S_, NEED, vmax=vm); table = K.ref_parking_table(c, S_)
            K.check_parking_record(rec, table, S_, NEED, what)
            if int(c["vOb"].max()) != vm:      # ... and through the row class of its own widest obstacle (a batch of its own): the mixed batch reaches all three
                K.check_parking_record(K.emu_parking(c, S_, NEED), table, S_, NEED, what + " own class")
            # the node samples are the nodes, bit for bit: whatever S, min_nodes is the S = 1 record's minimum
            one = K.emu_parking(c, 1, NEED, vmax=vm)
            assert one[0] == one[1] == rec[1], what
            if np.ptp(c["ts"]) == 0:      # one t, as a resident batch holds it: the same bits
                assert np.array_equal(K.emu_parking(c, S_, NEED, vmax=vm, resident=True), rec), what
    if N >= 5:
        assert len(seen_nob) >= 3 and max(seen_nob) >= 8, seen_nob


def test_mixed_batches_cover_the_three_row_classes():
    for N, _ in K.SHAPES:
        assert [K.vmax_of(b) for b in K.parking_cases(N)] == [2, 2, 8, 4]
    # ... and an instance runs through the class of its BATCH: the widest obstacle of any instance decides
    c = K.parking_cases(7)[0][0]
    a, b, d = (K.emu_parking(c, 4, NEED, vmax=v) for v in (2, 4, 8))
    for r in (b, d):
        assert np.abs(r[[0, 1]] - a[[0, 1]]).max() <= K.TOL_PARK and (r[4:8] == a[4:8]).all()


def test_substep_zero_is_the_node_bit_for_bit():
    for N, S_ in K.SHAPES:
        for c in K.parking_cases(N)[1]:
            p = V.parking_samples(c["x"], c["u"], c["ts"], c["Ts"], c["L"], S_)
            assert p.shape == (N * S_ + 1, 3) and np.array_equal(p[::S_], c["x"][:3].T)
            if S_ > 1:      # the interpolant is the step itself: sub-step S would be the dynamics' own next state
                nxt = V._dyn(c["x"][:, 0], c["u"][:, 0], c["ts"][0], c["Ts"], c["L"])
                half = V._dyn(c["x"][:, 0], c["u"][:, 0], (S_ - 1) / S_ * c["ts"][0], c["Ts"], c["L"])
                assert np.array_equal(p[S_ - 1], half[:3]) and np.abs(half - nxt).max() <= np.abs(nxt - c["x"][:, 0]).max() + 1e-15


# ---------------------------------------------------------------- 2. the finding
def golden_case(name):
    g = golden("clearance_cases.npz")
    c = {k: g[name + "__" + k] for k in ("Ts", "L", "ego", "vOb", "A", "b", "x", "u", "ts", "found")}
    c["N"] = int(g[name + "__N"]); c["Ts"] = float(c["Ts"]); c["L"] = float(c["L"])
    assert int(g[name + "__exitflag"]) == 1 and int(g["substeps"]) == 8
    return c


@pytest.mark.parametrize("name", ["corridor_sd", "corridor_dist"])
def test_solved_corridor_instance_passes_at_its_nodes_and_touches_a_wedge_between_them(name):
    """make_corridor_batch(8, 80, seed=11, clearance=(0.0, 0.2)) instance 1, solved by the oracle (exit flag 1): >= 0.05 at every node, contact at sample 106"""
    c = golden_case(name)
    rec = K.emu_parking(c, 8, NEED)
    assert rec[6] == 0 and rec[5] == 641
    assert rec[1] >= 0.05 - 1e-6 and rec[0] == 0.0
    assert (int(rec[2]) // 8, int(rec[2]) % 8, int(rec[3])) == (13, 2, 3) and rec[4] >= 1
    # what the generator found with the independent statement (tests/golden/make_clearance_cases.py prints it)
    assert tuple(c["found"][[0, 2, 3]]) == (0.0, 106.0, 3.0) and abs(rec[1] - c["found"][1]) <= K.TOL_PARK and abs(rec[4] - c["found"][4]) <= 1
    assert abs(c["found"][1] - {"corridor_sd": 0.0551111, "corridor_dist": 0.0501531}[name]) < 1e-6
    assert K.emu_parking(c, 1, NEED)[0] == rec[1]      # at the nodes alone nothing is seen


def test_solved_backwards_instance_loses_half_its_margin_between_the_nodes():
    """make_batch(BACKWARDS, 8, 30) instance 2, ParkingSignedDist by the oracle: 0.0564 at the nodes, 0.0244 between them"""
    c = golden_case("backwards30")
    rec = K.emu_parking(c, 8, NEED)
    assert rec[6] == 0 and rec[0] < rec[1] - 0.02
    assert abs(rec[0] - 0.024412) < 1e-6 and abs(rec[1] - 0.0563664) < 1e-6 and abs(rec[0] - c["found"][0]) <= K.TOL_PARK
    assert (rec[2], rec[3]) == (c["found"][2], c["found"][3]) == (164.0, 2.0) and rec[4] == c["found"][4] == 7


# ---------------------------------------------------------------- 3. quadcopter
@pytest.mark.parametrize("N,S_", K.QUAD_SHAPES + ((7, 1), (2, 32), (60, 4)))
def test_quadcopter_record_matches_numpy(N, S_):
    for i, c in enumerate(K.quad_cases(N)):
        for need in (0.0, 0.3):
            rec = K.emu_quad(c, S_, need); ref = V.quad_clearance(c["x"], c["ts"], c["Ts"], c["ob"], c["R"], S_, need)
            assert np.abs(rec[[0, 1, *range(8, 13)]] - ref[[0, 1, *range(8, 13)]]).max() <= K.TOL_QUAD, (N, S_, i)
            assert (rec[2:8] == ref[2:8]).all() and np.isinf(rec[13:]).all(), (N, S_, i, rec[2:8], ref[2:8])
            assert rec[0] >= -c["R"] and (S_ > 1 or rec[0] == rec[1])
        one = c["ts"][:1].copy()      # one t, as a resident batch holds it
        assert np.array_equal(K.emu_quad(dict(c, ts=one), S_, tstride=0), K.emu_quad(dict(c, ts=np.full(N + 1, one[0])), S_))


def test_quadcopter_segment_through_a_box_between_two_clear_nodes():
    from obca_amd import scenarios as S
    N, R = 2, 0.25
    ob = np.tile([-50.0, -50, -50, 51, 51, 51], (5, 1)); ob[2] = [5.0, 1.5, 1.5, -4.0, -0.5, -0.5]      # box 2: x in [4, 5], y, z in [0.5, 1.5]; the others far away
    x = np.zeros((12, N + 1)); x[:3, 0] = [3.0, 1.0, 1.0]; x[:3, 1] = [6.0, 1.0, 1.0]; x[:3, 2] = [6.0, 3.0, 1.0]
    Ts = 0.5; x[6:9, 0] = (x[:3, 1] - x[:3, 0]) / Ts; x[6:9, 1] = (x[:3, 2] - x[:3, 1]) / Ts
    c = dict(N=N, Ts=Ts, R=R, ob=ob, x=x, ts=np.ones(N + 1))
    rec = K.emu_quad(c, 4)      # sub-step 2 of interval 0 is (4.5, 1, 1): inside
    assert rec[0] == -R and rec[1] > 0 and rec[1] == 1.0 - R and (rec[2], rec[3]) == (2.0, 2.0) and rec[4] == 1 and rec[5] == 9
    assert np.array_equal(rec, V.quad_clearance(x, c["ts"], Ts, ob, R, 4))
    assert K.emu_quad(c, 1)[0] == rec[1] and S.QUAD_OB.shape == (5, 6)


# ---------------------------------------------------------------- 4. non-finite input, errors, order independence
BAD_RECORD = np.r_[np.nan, np.nan, -1, -1, 0, 0, 1, 0, np.full(16, np.nan)]


def assert_bad(rec, nS):
    exp = BAD_RECORD.copy(); exp[4] = exp[5] = nS
    assert np.array_equal(rec, exp, equal_nan=True), rec


def test_non_finite_input_marks_its_instance_and_no_other():
    N, S_ = 7, 4; batch = K.parking_cases(N)[1]; vm = K.vmax_of(batch)
    good = [K.emu_parking(c, S_, NEED, vmax=vm) for c in batch]
    for field, idx, v in (("x", (0, 3), np.nan), ("x", (3, N), np.inf), ("u", (1, 2), np.inf), ("u", (0, N - 1), -np.inf), ("ts", (4,), np.nan), ("ts", (N,), np.nan)):
        a = np.array(batch[2][field], float); a[idx] = v
        assert_bad(K.emu_parking(dict(batch[2], **{field: a}), S_, NEED, vmax=vm), N * S_ + 1)
        for c, g in zip(batch, good):      # (instances share nothing: the others come back bit for bit)
            assert np.array_equal(K.emu_parking(c, S_, NEED, vmax=vm), g)
    assert_bad(K.emu_parking(dict(batch[0], Ts=np.nan), S_, NEED, vmax=vm), N * S_ + 1)
    q = K.quad_cases(7)[1]
    for field, idx, v in (("x", (1, 3), np.nan), ("x", (7, 0), np.inf), ("ts", (2,), np.nan)):
        a = np.array(q[field], float); a[idx] = v
        assert_bad(K.emu_quad(dict(q, **{field: a}), 4), 29)
        assert np.array_equal(V.quad_clearance(a if field == "x" else q["x"], a if field == "ts" else q["ts"], q["Ts"], q["ob"], q["R"], 4), K.emu_quad(dict(q, **{field: a}), 4), equal_nan=True)


def test_argument_errors():
    lib = K.emu(); c = K.parking_cases(5)[0][0]; out = np.zeros(24)
    z = np.zeros(4096); prob = np.zeros(4096)
    for S_, need, msg in ((0, 0.05, b"substeps"), (33, 0.05, b"substeps"), (-1, 0.05, b"substeps"), (8, np.nan, b"need"), (8, np.inf, b"need"), (8, -np.inf, b"need")):
        assert lib.emu_clearance_parking(c["N"], K.dp(prob), K.dp(z), None, 2, S_, need, 0, K.dp(out)) == -1 and msg in lib.emu_clearance_last_error()
        assert lib.emu_clearance_quad(5, K.dp(prob), K.dp(z), K.dp(z), 1, S_, need, 0, K.dp(out)) == -1 and msg in lib.emu_clearance_last_error()
    assert (out == 0).all()
    for S_ in (1, 32):
        assert K.emu_parking(c, S_)[5] == c["N"] * S_ + 1


@pytest.mark.parametrize("N,S_", [(5, 3), (7, 4), (33, 8)])
def test_record_does_not_depend_on_how_items_are_dealt_to_the_lanes(N, S_):
    for batch in K.parking_cases(N):
        vm = K.vmax_of(batch)
        for c in batch:
            for need in (NEED, 0.2):
                assert np.array_equal(K.emu_parking(c, S_, need, vmax=vm, rev=0), K.emu_parking(c, S_, need, vmax=vm, rev=1))
    for c in K.quad_cases(7):
        assert np.array_equal(K.emu_quad(c, S_, 0.3, rev=0), K.emu_quad(c, S_, 0.3, rev=1))
    # a tie across lanes and rounds: two obstacles that are the same polygon, a trajectory that stands still -- every item of obstacles 0 and 1 has the same clearance
    c = K.parking_cases(5)[0][0]; v0 = int(c["vOb"][0])
    tie = dict(c, vOb=np.r_[c["vOb"][:1], c["vOb"]].astype(np.int32), A=np.r_[c["A"][:v0], c["A"]], b=np.r_[c["b"][:v0], c["b"]],
               x=np.repeat(c["x"][:, :1] * [[1], [1], [1], [0]], 6, axis=1), u=np.zeros((2, 5)))
    for rev in (0, 1):
        rec = K.emu_parking(tie, 3, 10.0, rev=rev)
        first = np.flatnonzero(rec[8:8 + len(tie["vOb"])] == rec[0])[0]
        assert (rec[2], rec[3]) == (0.0, float(first)) and rec[4] == 16 and rec[8] == rec[9], rec


# ---------------------------------------------------------------- the public surface and the build rule
def test_header_exports_python_and_julia_agree():
    from obca_amd import api, cabi
    protos = cabi.prototypes("obca_clearance.h")
    assert sorted(protos) == sorted(api.CLEARANCE_EXPORTS) and len(protos) == 6
    hdr = open(os.path.join(ROOT, "include", "obca_clearance.h")).read()
    assert re.search(r"#define OBCA_CLR_OUT 24\b", hdr) and re.search(r"#define OBCA_CLR_MAXSUB 32\b", hdr) and V.CLR_OUT == 24
    import obca_amd
    for f in ("parking_clearance_batch", "quadcopter_clearance_batch"):
        assert hasattr(obca_amd, f) and f in obca_amd.__all__
    assert all(hasattr(cls, m) for cls in (obca_amd.Batch, obca_amd.QuadBatch) for m in ("clearance", "clearance_ms"))
    # every ccall of the shim on the clearance entry points against the header, parameter by parameter (tests/test_julia_shim_cpu.py does this for include/obca_hip.h)
    import test_julia_shim_cpu as J
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S); kinds = {}
    for m in re.finditer(r"\bint\s*(obca_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        kinds[m.group(1)] = ["ptr" if "*" in p or "[" in p else ("double" if re.match(r"\s*(const\s+)?double\b", p) else "int") for p in m.group(2).split(",")]
    src = open(os.path.join(ROOT, "julia", "OBCAHip.jl")).read()
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), CLR\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
    assert {n for n, _ in calls} == set(kinds), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu")
    GXX = ["g++", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-misleading-indentation"]
    assert sorted(BF.CHECK_PIECES) == ["clearance_emu"] and not set(BF.CHECK_PIECES) & (set(BF.PIECES) | set(BF.TEST_PIECES)) and "clearance_emu" not in BF.DEFAULT
    p = BF.CHECK_PIECES["clearance_emu"]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_clearance_emu.so")
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
    assert os.path.realpath(os.path.join(ROOT, "obca_amd", "csrc", "obca_clearance.h")) in seen and os.path.realpath(os.path.join(ROOT, "obca_amd", "csrc", "obca_model.h")) in seen
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_clearance_emu.so")
    assert BF.build("clearance_emu", force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == GXX + ["-O1"] and argv[i + 2:] == [EMU + "/clearance_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # the kernel text is nothing the solve kernels use: no solver header includes it
    for f in os.listdir(os.path.join(ROOT, "obca_amd", "csrc")):
        if f.endswith(".h") and f != "obca_clearance.h":
            assert "obca_clearance.h" not in open(os.path.join(ROOT, "obca_amd", "csrc", f)).read(), f
    assert C.sizeof(C.c_double) == 8
