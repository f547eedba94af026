"""What tests/test_ensemble_cpu.py and tests/test_gpu_ensemble.py share: the host build of the kernel text of obca_amd/csrc/obca_ensemble.h (tests/emu/ensemble_emu.cpp,
buildflags.build("ensemble_emu")); the numpy records of an ensemble (validate.ensemble_parking / ensemble_quad, ensemble_member_record, ensemble_record); the inputs of both
suites; the comparison rules.  Trajectories are those of tests/rollout_common.py, the fixture tests/golden/rollout_cases.npz, cut to shorter horizons where a case says so.

Tolerances.  Host build against numpy: track_common.TOL_HOST (3.1e-10), the bound tests/test_track_cpu.py asserts for the same two sides -- with a zero bias member m of the
numpy statement IS validate.track_parking / track_quad with dx0[m].  Device against host build: rollout_common.TOL_DEV (1e-9 max(1, |value|)), the bound
tests/test_gpu_track.py uses.  Index and count fields are compared exactly; the offsets below are chosen -- and `separated` asserts it on the numpy side -- so that no
sample lies within 1e-9 of `need` and no two candidates of a minimum or maximum lie within 1e-9 of each other: exact indices are then a fair demand."""
import ctypes as C
import functools
import numpy as np
import packing as P
import rollout_common as R
import track_common as T
from obca_amd import buildflags, validate as V

D = C.POINTER(C.c_double)
dp = R.dp
TOL_HOST, TOL_DEV = T.TOL_HOST, T.TOL_DEV
MEM_REAL = [1, 3, 4, 5, 6, 7, 12, 14]; MEM_EXACT = [0, 2, 8, 9, 10, 11, 13, 15]
OUT_REAL = [8, 12, 15, 17, 18, 19, 20, 23, 24]; OUT_EXACT = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 13, 14, 16, 21, 22, 25, 26, 27, 28, 29, 30, 31]
GAP = 1e-9
SIGMA_PARK = np.array([0.05, 0.05, 0.02, 0.05]); SIGMA_QUAD = np.r_[np.full(3, 0.05), np.full(3, 0.01), np.full(3, 0.05), np.full(3, 0.01)]
# The cases of both suites: (vehicle, instance of the fixture, horizon N -- the fixture's, or cut to its first N intervals --, sub-steps, members, seed of the offsets, need).
# S in {1, 2}, M in {1, 3, 64}, N = 1 and N = 3 among the horizons.  `need` lies between two members' smallest clearances, so members_hit splits the ensemble.  Instances
# and seeds are those for which `separated` holds on the numpy side: quadcopter instances 1 and 3 fly THROUGH an inflated box at the full horizon (clearance exactly -R at
# several samples), and the converged closed loops of parking instances 0 and 2 end within 1e-10 of each other -- on those the indices are no fair demand.
CASES = [("parking", 1, 30, 2, 64, 0, 0.0537352), ("parking", 1, 30, 1, 3, 0, 0.0537298), ("parking", 0, 3, 2, 3, 0, 0.9769746), ("parking", 2, 3, 1, 64, 0, 0.6800184),
         ("parking", 0, 1, 2, 64, 0, 1.0309773), ("parking", 2, 1, 1, 1, 0, 0.7055931), ("parking", 1, 1, 1, 3, 0, 1.7226065),
         ("quad", 0, 20, 2, 64, 0, -0.2119539), ("quad", 0, 20, 1, 3, 0, -0.2047559), ("quad", 2, 20, 1, 3, 0, -0.2419781), ("quad", 1, 3, 2, 3, 0, 0.7972013),
         ("quad", 3, 3, 1, 64, 0, 0.7913713), ("quad", 2, 1, 2, 64, 0, 0.778527), ("quad", 3, 1, 1, 1, 0, 0.9499499), ("quad", 1, 2, 1, 3, 0, 0.8862148)]
NEED_PARK, NEED_QUAD = V.DMIN, 0.0


def case_id(case):
    return "%s%d-N%d-S%d-M%d" % case[:5]


def case_inputs(case):
    """(trajectory, S, M, dx0 (M, nx), need) of a case"""
    kind, i, N, S_, M, seed, need = case
    c = cut((R.golden_parking() if kind == "parking" else R.golden_quad())[i], N)
    return c, S_, M, offsets(M, SIGMA_PARK if kind == "parking" else SIGMA_QUAD, seed), need


@functools.lru_cache(None)
def emu():
    lib = C.CDLL(buildflags.build("ensemble_emu"))
    lib.emu_ensemble_last_error.restype = C.c_char_p
    lib.emu_ensemble_parking.argtypes = [C.c_int, D, D, D, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, D, D, D, D, D, C.c_double, C.c_int, D, D, D]
    lib.emu_ensemble_quad.argtypes = [C.c_int, D, D, D, D, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, D, D, D, D, D, C.c_double, C.c_int, D, D, D]
    lib.emu_ensemble_reduce.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, D, D]
    a, b, c = (C.c_int(0) for _ in range(3))
    lib.emu_ensemble_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (V.ENS_MEM, V.ENS_OUT, V.ENS_MMAX) == (16, 32, 64)
    return lib


# ---------------------------------------------------------------- inputs
def cut(c, N):
    """case c with its horizon cut to the first N intervals"""
    return c if N == c["N"] else dict(c, N=N, x=np.ascontiguousarray(c["x"][:, :N + 1]), u=np.ascontiguousarray(c["u"][:, :N]), ts=np.ascontiguousarray(c["ts"][:N + 1]))


def offsets(M, sigma, seed):
    """(M, n) seeded normal rows, member 0 exactly zero (obca_amd.ensemble_offsets for one instance)"""
    from obca_amd import ensemble_offsets
    return ensemble_offsets(1, M, sigma, seed)[0]


# ---------------------------------------------------------------- the host build
def _opt(a):
    return None if a is None else dp(np.ascontiguousarray(a, float))


def emu_parking(c, S_, M, dx0=None, dub=None, fb=1, cl=1, need=NEED_PARK, rev=0, w=None):
    """one instance through the kernel text: (record (32,), member records (M,16), final states (M,4))"""
    N, vOb = c["N"], c["vOb"]; nOb, Mr = len(vOb), int(vOb.sum()); zero = np.zeros(N + 1)
    prob = P.pack_problem(np.zeros(4), np.zeros(4), N, c["Ts"], c["L"], c["ego"], np.zeros(4), vOb, c["A"], c["b"], zero, zero, zero, 0)
    z = P.pack_start(N, nOb, Mr, c["x"].T, c["u"].T, np.zeros((N + 1, Mr)), np.zeros((N + 1, 4 * nOb)))
    ts = np.ascontiguousarray(c["ts"], float); q, r, qf = T._w(w, T.PARK_W)
    out = np.full(V.ENS_OUT, -7.0); mem = np.full((M, V.ENS_MEM), -7.0); fin = np.full((M, 4), -7.0)
    rc = emu().emu_ensemble_parking(N, dp(prob), dp(z), dp(ts), int(vOb.max()), int(S_), int(M), int(fb), int(cl), dp(q), dp(r), dp(qf), _opt(dx0), _opt(dub), float(need), int(rev),
                                    dp(mem), dp(fin), dp(out))
    assert rc == 0, emu().emu_ensemble_last_error()
    return out, mem, fin


def emu_quad(c, S_, M, dx0=None, dub=None, fb=1, cl=1, need=NEED_QUAD, rev=0, w=None):
    N = c["N"]
    prob = P.pack_quad_problem(np.zeros(12), np.zeros(12), N, c["Ts"], c["R"], c["ob"], np.zeros((N + 1, 12)), 1.0)
    xs = np.ascontiguousarray(c["x"].T); us = np.ascontiguousarray(c["u"].T); ts = np.ascontiguousarray(c["ts"], float); q, r, qf = T._w(w, T.QUAD_W)
    out = np.full(V.ENS_OUT, -7.0); mem = np.full((M, V.ENS_MEM), -7.0); fin = np.full((M, 12), -7.0)
    rc = emu().emu_ensemble_quad(N, dp(prob), dp(xs), dp(us), dp(ts), 1, int(S_), int(M), int(fb), int(cl), dp(q), dp(r), dp(qf), _opt(dx0), _opt(dub), float(need), int(rev),
                                 dp(mem), dp(fin), dp(out))
    assert rc == 0, emu().emu_ensemble_last_error()
    return out, mem, fin


def emu_reduce(mem, S_, fb, cl, inst_bad):
    mem = np.ascontiguousarray(mem, float); out = np.full(V.ENS_OUT, -7.0)
    assert emu().emu_ensemble_reduce(len(mem), int(S_), int(fb), int(cl), int(inst_bad), dp(mem), dp(out)) == 0
    return out


# ---------------------------------------------------------------- the numpy statement
def _ref(c, S_, M, members, ok, table, need, fb, cl):
    """(record, member records, final states, per good member what its indices were picked from: the clearance table, the position deviation per node, the largest
    |U_k - u_k| per interval) from what validate.ensemble_* returned"""
    mem = np.zeros((M, V.ENS_MEM)); fin = np.zeros((M, c["x"].shape[0])); picks = []; npos = 2 if c["x"].shape[0] == 4 else 3
    for m, (X, poses, info) in enumerate(members):
        good = bool(ok and info["finite"])
        tab = table(poses) if good else np.full((len(poses), 1), np.nan)
        mem[m] = V.ensemble_member_record(c["x"], c["u"], X, tab, S_, need, dict(info, finite=good))
        fin[m] = X[:, -1] if mem[m, 0] == 0 else np.nan
        if mem[m, 0] == 0:
            picks.append((tab, np.sqrt(((X[:npos, 1:] - c["x"][:npos, 1:]) ** 2).sum(axis=0)), np.abs(info["U"] - c["u"]).max(axis=0)))
    return V.ensemble_record(mem, S_, fb, cl, ok), mem, fin, picks


def ref_parking(c, S_, M, dx0=None, dub=None, fb=1, cl=1, need=NEED_PARK):
    members, ok = V.ensemble_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], M, S_, dx0, dub, feedback=fb, clamp=cl)
    return _ref(c, S_, M, members, ok, lambda poses: R.host_pose_table(c, poses), need, fb, cl)


def ref_quad(c, S_, M, dx0=None, dub=None, fb=1, cl=1, need=NEED_QUAD):
    members, ok = V.ensemble_quad(c["x"], c["u"], c["ts"], c["Ts"], M, S_, dx0, dub, feedback=fb, clamp=cl)
    return _ref(c, S_, M, members, ok, lambda poses: V.quad_point_clearance(poses, c["ob"], c["R"]), need, fb, cl)


# ---------------------------------------------------------------- comparison
def _lowest_apart(v):
    v = np.sort(np.asarray(v, float).ravel())
    return len(v) < 2 or v[1] - v[0] > GAP


def separated(ref, need):
    """the numpy side of a case, the condition under which exact indices and counts are asked for: no clearance of a sample within GAP of `need`; no two candidates of a
    minimum within GAP of each other -- per member over its (sample, obstacle) table, and over the members; the same for the maxima that carry an index (dev_pos over
    the nodes, du_max over the intervals, dev_pos / end_pos / du_max over the members)"""
    _, mem, _, picks = ref
    for tab, dpos, du in picks:
        if not ((np.abs(tab - need) > GAP).all() and _lowest_apart(tab) and _lowest_apart(-dpos) and _lowest_apart(-du)):
            return False
    g = mem[mem[:, 0] == 0]
    return bool(_lowest_apart(g[:, 7]) and _lowest_apart(-g[:, 1]) and _lowest_apart(-g[:, 3]) and _lowest_apart(-g[:, 12]))


def worst(got, ref):
    return max(R.worst(got[0][OUT_REAL], ref[0][OUT_REAL]), R.worst(got[1][:, MEM_REAL], ref[1][:, MEM_REAL]), R.worst(got[2], ref[2]))


def check(got, ref, tol, what):
    """(record, member records, final states) against the same: real fields within tol max(1, |value|), index and count fields equal"""
    assert R.close(got[1][:, MEM_REAL], ref[1][:, MEM_REAL], tol), (what, "members", got[1], ref[1])
    assert np.array_equal(got[1][:, MEM_EXACT], ref[1][:, MEM_EXACT]), (what, "member indices", got[1][:, MEM_EXACT], ref[1][:, MEM_EXACT])
    assert R.close(got[0][OUT_REAL], ref[0][OUT_REAL], tol), (what, got[0], ref[0])
    assert np.array_equal(got[0][OUT_EXACT], ref[0][OUT_EXACT]), (what, got[0][OUT_EXACT], ref[0][OUT_EXACT])
    assert R.close(got[2], ref[2], tol), (what, "final states")
