"""What tests/test_rollout_cpu.py and tests/test_gpu_rollout.py share: the host build of the kernel text of obca_amd/csrc/obca_rollout.h (tests/emu/rollout_emu.cpp,
buildflags.build("rollout_emu")); the trajectories both suites run -- the solved ones of tests/golden/rollout_cases.npz and synthetic ones at the horizons where the code
takes another path --; the numpy record of a trajectory (validate.rollout_parking / rollout_quad / rollout_record); the comparison rules.

Tolerances.  Host build against numpy: 1e-12 max(1, |value|), the bound tests/test_refine_cpu.py asserts -- both sides run the same operations in the same order on fp64
without contraction, and the statement uses the C library's sin / cos / tan through `math`.  The clearance table of the numpy side: quadcopter validate.quad_point_clearance;
parking the host build's own DualMultWS distance (the clearance emulation, one pose per call) at NUMPY's sample poses with the clamp -- the distance is an iteration that the
project holds to 1e-9 against the oracle (tests/clearance_common.py), so a 1e-12 comparison of records needs the same iteration on both sides; what is compared is
everything the rollout adds: poses, order of the items, the record.  Device against host build: 1e-9 max(1, |value|), the bound tests/test_gpu_clearance.py asserts for the
parking distances: the device contracts products into sums and uses its own sin / cos / tan."""
import ctypes as C
import functools
import os
import numpy as np
import packing as P
import clearance_common as K
from obca_amd import buildflags, scenarios as S, validate as V

D = C.POINTER(C.c_double)
TOL_HOST, TOL_DEV = 1e-12, 1e-9
MODES = (0, 1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_cases.npz")
dp = K.dp


@functools.lru_cache(None)
def emu():
    lib = C.CDLL(buildflags.build("rollout_emu"))
    lib.emu_rollout_last_error.restype = C.c_char_p
    lib.emu_rollout_parking.argtypes = [C.c_int, D, D, D, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, D, D, D]
    lib.emu_rollout_quad.argtypes = [C.c_int, D, D, D, D, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, D, D, D]
    a, b, c = (C.c_int(0) for _ in range(3))
    lib.emu_rollout_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (V.ROLL_OUT, 16, 32)
    return lib


# ---------------------------------------------------------------- trajectories
@functools.lru_cache(None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(None)
def golden_quad():
    """the four solved instances of make_quad_batch(4, 20): x (12,21), u (4,20), one t"""
    g = golden(); bt = S.make_quad_batch(4, 20)
    return [dict(N=20, Ts=float(bt["Ts"]), R=bt["R"], ob=bt["ob"], x=g["quad_x"][i], u=g["quad_u"][i], ts=np.full(21, g["quad_t"][i])) for i in range(4)]


@functools.lru_cache(None)
def golden_parking():
    """instances 0-2 of make_batch(BACKWARDS, 8, 30), solved"""
    g = golden(); bt = S.make_batch(S.BACKWARDS, 8, 30)
    return [dict(N=30, Ts=float(bt["Ts"][i]), L=bt["L"], ego=bt["ego"], vOb=np.asarray(bt["vOb"], np.int32), A=np.asarray(bt["A"], float), b=np.asarray(bt["b"], float),
                 x=g["park_x"][i], u=g["park_u"][i], ts=g["park_ts"][i]) for i in range(3)]


@functools.lru_cache(None)
def synthetic_quad(N, B=2, seed=5):
    """seeded inputs inside their bounds around the hover speed, chained through the DISCRETE model (forward Euler, as the NLP's rows) from a hover state: what a solution
    looks like to the rollout, at any horizon.  Ts = 0.05 keeps the attitude small over 128 intervals."""
    rng = np.random.default_rng(seed + N); bt = S.make_quad_batch(B, max(N, 2)); Ts = 0.05; hover = np.sqrt(V._QC["m"] * V._QC["g"] / (4 * V._QC["kF"]))
    out = []
    for i in range(B):
        u = np.clip(hover + 0.004 * rng.standard_normal((4, N)), 1.2, 7.8); ts = 1 + 0.1 * np.sin(np.arange(N + 1.0) + i)
        x = np.zeros((12, N + 1)); x[:3, 0] = [1.0 + i, 1.0, 2.0]; x[6:9, 0] = [0.3, 0.2, 0.0]
        for k in range(N):
            x[:, k + 1] = x[:, k] + ts[k] * Ts * np.array(V._quad_rhs(x[:, k], u[:, k]))
        out.append(dict(N=N, Ts=Ts, R=bt["R"], ob=bt["ob"], x=x, u=u, ts=ts))
    return out


@functools.lru_cache(None)
def synthetic_parking(N, B=2, seed=7):
    """the same for parking: seeded steering and acceleration inside their bounds, chained through the discrete step (validate._dyn) from the scenario's start pose"""
    rng = np.random.default_rng(seed + N); bt = S.make_batch(S.BACKWARDS, B, N)
    out = []
    for i in range(B):
        u = np.array([0.5 * np.sin(0.3 * np.arange(N) + i) + 0.05 * rng.standard_normal(N), 0.3 * np.cos(0.2 * np.arange(N)) + 0.05 * rng.standard_normal(N)])
        ts = 1 + 0.1 * np.sin(np.arange(N + 1.0) + i); Ts = min(float(bt["Ts"][i]), 1.2) * min(1.0, 30.0 / N)
        x = np.zeros((4, N + 1)); x[:, 0] = bt["x0"][i]
        for k in range(N):
            x[:, k + 1] = V._dyn(x[:, k], u[:, k], ts[k], Ts, bt["L"])
        out.append(dict(N=N, Ts=Ts, L=bt["L"], ego=bt["ego"], vOb=np.asarray(bt["vOb"], np.int32), A=np.asarray(bt["A"], float), b=np.asarray(bt["b"], float), x=x, u=u, ts=ts))
    return out


def quad_cases(N):
    return golden_quad() if N == 20 else synthetic_quad(N)


def parking_cases(N):
    return golden_parking() if N == 30 else synthetic_parking(N)


# ---------------------------------------------------------------- the host build
def emu_parking(c, substeps, restart, need=V.DMIN, rev=0, resident=False, vmax=None):
    """one instance through the kernel text: (record (40,), X (4,N+1), poses (N S + 1, 3))"""
    N, vOb = c["N"], c["vOb"]; nOb, M = len(vOb), int(vOb.sum()); zero = np.zeros(N + 1)
    prob = P.pack_problem(np.zeros(4), np.zeros(4), N, c["Ts"], c["L"], c["ego"], np.zeros(4), vOb, c["A"], c["b"], zero, zero, zero, 0)
    z = P.pack_start(N, nOb, M, c["x"].T, c["u"].T, np.zeros((N + 1, M)), np.zeros((N + 1, 4 * nOb)))
    ts = np.ascontiguousarray(c["ts"], float)
    if resident:
        z[P.layout(N, nOb, M)["t"]] = ts[0]
    out = np.full(V.ROLL_OUT, -7.0); pose = np.full((N * substeps + 1, 3), -7.0); X = np.full((N + 1, 4), -7.0)
    rc = emu().emu_rollout_parking(N, dp(prob), dp(z), None if resident else dp(ts), vmax or int(vOb.max()), int(substeps), int(restart), float(need), int(rev), dp(pose), dp(X), dp(out))
    assert rc == 0, emu().emu_rollout_last_error()
    return out, X.T.copy(), pose


def emu_quad(c, substeps, restart, need=0.0, rev=0, tstride=1):
    N = c["N"]
    prob = P.pack_quad_problem(np.zeros(12), np.zeros(12), N, c["Ts"], c["R"], c["ob"], np.zeros((N + 1, 12)), 1.0)
    xs = np.ascontiguousarray(c["x"].T); us = np.ascontiguousarray(c["u"].T); ts = np.ascontiguousarray(c["ts"], float)
    out = np.full(V.ROLL_OUT, -7.0); pose = np.full((N * substeps + 1, 3), -7.0); X = np.full((N + 1, 12), -7.0)
    rc = emu().emu_rollout_quad(N, dp(prob), dp(xs), dp(us), dp(ts), int(tstride), int(substeps), int(restart), float(need), int(rev), dp(pose), dp(X), dp(out))
    assert rc == 0, emu().emu_rollout_last_error()
    return out, X.T.copy(), pose


# ---------------------------------------------------------------- the numpy statement
def host_pose_table(c, poses):
    """(n, nOb): the host build's DualMultWS distance of every pose to every obstacle, clamped -- the clearance emulation on a one-interval trajectory that stands at the
    pose (one packed record, the pose patched in per call), in the row class of the instance's widest obstacle"""
    vOb = c["vOb"]; nOb, M = len(vOb), int(vOb.sum()); zero = np.zeros(2); lib = K.emu()
    prob = P.pack_problem(np.zeros(4), np.zeros(4), 1, c["Ts"], c["L"], c["ego"], np.zeros(4), vOb, c["A"], c["b"], zero, zero, zero, 0)
    z = P.pack_start(1, nOb, M, np.zeros((2, 4)), np.zeros((1, 2)), np.zeros((2, M)), np.zeros((2, 4 * nOb)))
    ox = P.layout(1, nOb, M)["x"]; out = np.zeros((len(poses), nOb)); rec = np.zeros(V.CLR_OUT); one = np.ones(2)
    for q, p in enumerate(poses):
        z[ox:ox + 3] = p; z[ox + 4:ox + 7] = p
        assert lib.emu_clearance_parking(1, dp(prob), dp(z), dp(one), int(vOb.max()), 1, V.DMIN, 0, dp(rec)) == 0
        out[q] = rec[8:8 + nOb]
    return out


def ref_parking(c, substeps, restart, need=V.DMIN, table=host_pose_table):
    X, poses = V.rollout_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], substeps, restart)
    fin = bool(np.isfinite(X).all() and np.isfinite(c["u"]).all() and np.isfinite(c["x"]).all() and np.isfinite(c["ts"]).all())
    tab = table(c, poses) if fin else np.full((len(poses), len(c["vOb"])), np.nan)
    return V.rollout_record(c["x"], X, tab, substeps, restart, need, fin), X, poses


def ref_quad(c, substeps, restart, need=0.0):
    X, poses = V.rollout_quad(c["x"], c["u"], c["ts"], c["Ts"], substeps, restart)
    fin = bool(np.isfinite(X).all() and np.isfinite(c["u"]).all() and np.isfinite(c["x"]).all() and np.isfinite(c["ts"]).all())
    tab = V.quad_point_clearance(poses, c["ob"], c["R"]) if fin else np.full((len(poses), 5), np.nan)
    return V.rollout_record(c["x"], X, tab, substeps, restart, need, fin), X, poses


# ---------------------------------------------------------------- comparison
REAL = [1, 3, 4, 5, 6, 7, 8, 9, 16, 17] + list(range(24, 40))      # the real-valued fields of a record
EXACT = [0, 2, 10, 11, 12, 13, 14, 15, 18, 19, 20, 21, 22, 23]     # flags, indices, counts


def close(a, b, tol):
    a = np.asarray(a, float); b = np.asarray(b, float)
    with np.errstate(invalid="ignore"):
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        return bool((same | (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))).all())


def worst(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float); m = np.isfinite(a) & np.isfinite(b)
    with np.errstate(invalid="ignore"):
        return float((np.abs(a - b)[m] / np.maximum(1.0, np.abs(b[m]))).max()) if m.any() else 0.0


def check_record(rec, ref, tol, what, exact_idx=True):
    assert close(rec[REAL], ref[REAL], tol), (what, rec, ref)
    if exact_idx:
        assert np.array_equal(rec[EXACT], ref[EXACT]), (what, rec[EXACT], ref[EXACT])
    else:      # flags and sizes always; an index or a count may move where two values lie within the tolerance of each other
        assert np.array_equal(rec[[0, 10, 11, 12, 13, 14, 15, 21, 22, 23]], ref[[0, 10, 11, 12, 13, 14, 15, 21, 22, 23]]), (what, rec, ref)
