"""What tests/test_track_cpu.py and tests/test_gpu_track.py share: the host build of the kernel text of obca_amd/csrc/obca_track.h (tests/emu/track_emu.cpp,
buildflags.build("track_emu")); the numpy record of a tracked trajectory (validate.track_parking / track_quad / track_record); the comparison rules.  Trajectories are those
of tests/rollout_common.py: the solved ones of tests/golden/rollout_cases.npz and its synthetic ones at the horizons where the code takes another path.

Tolerances.  Host build against numpy: both sides run the linearisation and the closed loop as the same operations in the same order on fp64 without contraction; the
Riccati products differ -- the kernel text sums every entry in a fixed order, numpy's matmul in its own -- and the recursion carries that through N steps.  The largest gap
measured on this suite (every shape, mode and lane order of test_host_build_matches_numpy, printed by it) is MEASURED_HOST; asserted is TOL_HOST = 100 x that, which stays
under the 1e-8 the feature's specification allows.  Gains are compared relative to the instance's largest |K|, everything else as rollout_common.close does.  Device
against host build: rollout_common.TOL_DEV (1e-9 max(1, |value|)), the project's rollout bound."""
import ctypes as C
import functools
import numpy as np
import packing as P
import rollout_common as R
from obca_amd import buildflags, validate as V

D = C.POINTER(C.c_double)
dp = R.dp
MEASURED_HOST = 3.1e-12      # quadcopter fixture, N = 20 (parking: 3.5e-15)
TOL_HOST = 100 * MEASURED_HOST
TOL_DEV = R.TOL_DEV
REAL = R.REAL + [43, 45]                 # the real-valued fields of a record
EXACT = R.EXACT + [40, 41, 42, 44, 46, 47]      # flags, indices, counts
DX0_PARK = np.array([0.1, 0.1, 0.05, 0.0])
DX0_QUAD = np.r_[np.full(3, 0.1), np.zeros(3), np.full(3, 0.1), np.zeros(3)]
PARK_W = (V.TRACK_Q_PARKING, V.TRACK_R_PARKING, V.TRACK_QF_PARKING)
QUAD_W = (V.TRACK_Q_QUAD, V.TRACK_R_QUAD, V.TRACK_QF_QUAD)


@functools.lru_cache(None)
def emu():
    lib = C.CDLL(buildflags.build("track_emu"))
    lib.emu_track_last_error.restype = C.c_char_p
    lib.emu_track_parking.argtypes = [C.c_int, D, D, D, C.c_int, C.c_int, C.c_int, C.c_int, D, D, D, D, C.c_double, C.c_int, D, D, D, D, D]
    lib.emu_track_quad.argtypes = [C.c_int, D, D, D, D, C.c_int, C.c_int, C.c_int, C.c_int, D, D, D, D, C.c_double, C.c_int, D, D, D, D, D]
    a, b, c = (C.c_int(0) for _ in range(3))
    lib.emu_track_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (V.TRK_OUT, V.ROLL_OUT, 32)
    return lib


def _w(w, defaults):
    return [np.ascontiguousarray(defaults[i] if w is None or w[i] is None else w[i], float) for i in range(3)]


def _opt(a):
    return None if a is None else dp(np.ascontiguousarray(a, float))


# ---------------------------------------------------------------- the host build
def emu_parking(c, substeps, feedback=1, clamp=1, dx0=None, w=None, need=V.DMIN, rev=0):
    """one instance through the kernel text: (record (48,), X (4,N+1), poses (N S + 1, 3), K (N,2,4), AB (N,4,6))"""
    N, vOb = c["N"], c["vOb"]; nOb, M = len(vOb), int(vOb.sum()); zero = np.zeros(N + 1)
    prob = P.pack_problem(np.zeros(4), np.zeros(4), N, c["Ts"], c["L"], c["ego"], np.zeros(4), vOb, c["A"], c["b"], zero, zero, zero, 0)
    z = P.pack_start(N, nOb, M, c["x"].T, c["u"].T, np.zeros((N + 1, M)), np.zeros((N + 1, 4 * nOb)))
    ts = np.ascontiguousarray(c["ts"], float); q, r, qf = _w(w, PARK_W)
    out = np.full(V.TRK_OUT, -7.0); pose = np.full((N * substeps + 1, 3), -7.0); X = np.full((N + 1, 4), -7.0); K = np.full((N, 2, 4), -7.0); AB = np.full((N, 4, 6), -7.0)
    rc = emu().emu_track_parking(N, dp(prob), dp(z), dp(ts), int(vOb.max()), int(substeps), int(feedback), int(clamp), dp(q), dp(r), dp(qf), _opt(dx0), float(need), int(rev),
                                 dp(AB), dp(pose), dp(X), dp(K), dp(out))
    assert rc == 0, emu().emu_track_last_error()
    return out, X.T.copy(), pose, K, AB


def emu_quad(c, substeps, feedback=1, clamp=1, dx0=None, w=None, need=0.0, rev=0):
    N = c["N"]
    prob = P.pack_quad_problem(np.zeros(12), np.zeros(12), N, c["Ts"], c["R"], c["ob"], np.zeros((N + 1, 12)), 1.0)
    xs = np.ascontiguousarray(c["x"].T); us = np.ascontiguousarray(c["u"].T); ts = np.ascontiguousarray(c["ts"], float); q, r, qf = _w(w, QUAD_W)
    out = np.full(V.TRK_OUT, -7.0); pose = np.full((N * substeps + 1, 3), -7.0); X = np.full((N + 1, 12), -7.0); K = np.full((N, 4, 12), -7.0); AB = np.full((N, 12, 16), -7.0)
    rc = emu().emu_track_quad(N, dp(prob), dp(xs), dp(us), dp(ts), 1, int(substeps), int(feedback), int(clamp), dp(q), dp(r), dp(qf), _opt(dx0), float(need), int(rev),
                              dp(AB), dp(pose), dp(X), dp(K), dp(out))
    assert rc == 0, emu().emu_track_last_error()
    return out, X.T.copy(), pose, K, AB


# ---------------------------------------------------------------- the numpy statement
def _wkw(w):
    return {} if w is None else dict(Q=w[0], R=w[1], Qf=w[2])


def ref_parking(c, substeps, feedback=1, clamp=1, dx0=None, w=None, need=V.DMIN):
    X, poses, info = V.track_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], substeps, dx0, feedback=feedback, clamp=clamp, **_wkw(w))
    fin = bool(info["finite"] and np.isfinite(c["x"]).all() and np.isfinite(c["ts"]).all())
    tab = R.host_pose_table(c, poses) if fin else np.full((len(poses), len(c["vOb"])), np.nan)
    info = dict(info, finite=fin)
    return V.track_record(c["x"], c["u"], X, tab, substeps, need, info), (X if fin else np.full(X.shape, np.nan)), poses, (info["K"] if fin else np.full(info["K"].shape, np.nan)), info["AB"]


def ref_quad(c, substeps, feedback=1, clamp=1, dx0=None, w=None, need=0.0):
    X, poses, info = V.track_quad(c["x"], c["u"], c["ts"], c["Ts"], substeps, dx0, feedback=feedback, clamp=clamp, **_wkw(w))
    fin = bool(info["finite"] and np.isfinite(c["x"]).all() and np.isfinite(c["ts"]).all())
    tab = V.quad_point_clearance(poses, c["ob"], c["R"]) if fin else np.full((len(poses), 5), np.nan)
    info = dict(info, finite=fin)
    return V.track_record(c["x"], c["u"], X, tab, substeps, need, info), (X if fin else np.full(X.shape, np.nan)), poses, (info["K"] if fin else np.full(info["K"].shape, np.nan)), info["AB"]


# ---------------------------------------------------------------- comparison
def gain_gap(K, Kr):
    """the largest difference of two gain arrays of ONE instance relative to the largest |K| of the reference (0 where both are NaN throughout)"""
    K = np.asarray(K, float); Kr = np.asarray(Kr, float)
    if np.isnan(Kr).all() and np.isnan(K).all():
        return 0.0
    return float(np.abs(K - Kr).max() / np.abs(Kr).max())


def gaps(got, ref):
    """(record, X, poses, K, AB) against the same: the largest gap, gains by gain_gap, the rest by rollout_common.worst"""
    return max(R.worst(got[0][REAL], ref[0][REAL]), R.worst(got[1], ref[1]), R.worst(got[2], ref[2]), gain_gap(got[3], ref[3]), R.worst(got[4], ref[4]))


def check(got, ref, tol, what, exact_idx=True):
    rec, ref_rec = got[0], ref[0]
    assert R.close(rec[REAL], ref_rec[REAL], tol), (what, rec, ref_rec)
    if exact_idx:
        assert np.array_equal(rec[EXACT], ref_rec[EXACT]), (what, rec[EXACT], ref_rec[EXACT])
    else:      # flags and sizes always; an index or a count may move where two values lie within the tolerance of each other (the rule of rollout_common.check_record)
        keep = [0, 10, 11, 12, 13, 14, 15, 21, 22, 23, 40, 41, 46, 47]
        assert np.array_equal(rec[keep], ref_rec[keep]), (what, rec, ref_rec)
    assert R.close(got[1], ref[1], tol), (what, "states")
    assert gain_gap(got[3], ref[3]) <= tol, (what, "gains", gain_gap(got[3], ref[3]))
    for a, b in zip(got[2:3] + got[4:], ref[2:3] + ref[4:]):      # poses and [A|B], where both sides have them
        assert R.close(a, b, tol), (what, "poses / AB")
