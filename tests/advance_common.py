"""What tests/test_advance_cpu.py and tests/test_gpu_advance.py share: the host build of the kernel text of obca_amd/csrc/obca_advance.h (tests/emu/advance_emu.cpp,
buildflags.build("advance_emu")); instances packed as the kernel addresses them from the trajectories of tests/rollout_common.py (the solved ones of
tests/golden/rollout_cases.npz, synthetic ones at the loop edges) or from a batch's own download; the numpy record of a step (validate.advance_parking / advance_quad /
advance_record); the restart the existing numpy shifts (tests/shift_common.py, tests/quad_shift_common.py) ask for when they are fed the plant state.

Tolerances.  Host build against numpy: 3.1e-10 max(1, |value|), the bound tests/test_track_cpu.py and tests/test_ensemble_cpu.py assert for host build against numpy.  The
parking clearance table of the numpy side is the host build's own DualMultWS distance at NUMPY's sample poses (rollout_common.host_pose_table), as for the rollout.  The
restart only copies: bit for bit.  Device against host build: 1e-9 max(1, |value|), the bound of tests/test_gpu_rollout.py."""
import ctypes as C
import functools
import numpy as np
import packing as P
import rollout_common as RC
import shift_common as SC
import quad_shift_common as QS
from obca_amd import buildflags, validate as V

D = C.POINTER(C.c_double)
TOL_HOST, TOL_DEV = 3.1e-10, 1e-9
REAL = RC.REAL + [13, 14]                                   # the real-valued fields of a record: the rollout's, the driven time, the distance to the goal
EXACT = [i for i in RC.EXACT if i not in (13, 14)]          # flags, indices, counts: with [12] shift and [15] logged
dp = RC.dp


@functools.lru_cache(None)
def emu():
    lib = C.CDLL(buildflags.build("advance_emu"))
    lib.emu_advance_last_error.restype = C.c_char_p
    LL = C.c_longlong
    lib.emu_advance_parking.argtypes = [C.c_int, C.c_int, C.c_int, D, LL, D, D, D, LL, C.c_int, C.c_int, D, C.c_double, C.c_int, D, D, C.c_int, C.c_int, D]
    lib.emu_advance_quad.argtypes = [C.c_int, C.c_int, C.c_int, D, LL, D, LL, D, C.c_int, D, D, C.c_double, C.c_int, D, D, C.c_int, C.c_int, D]
    a, b, c = (C.c_int(0) for _ in range(3))
    lib.emu_advance_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (V.ADV_OUT, 16, 32)
    return lib


def bits(a):
    return np.ascontiguousarray(a, float).view(np.uint64)


def same(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def pattern(n, salt):
    """n distinct finite words no copy can produce"""
    return -(1e6 * (salt + 1) + np.arange(n, dtype=float)) - 0.5


def check_record(rec, ref, tol, what, exact_idx=True):
    assert RC.close(rec[REAL], ref[REAL], tol), (what, rec, ref)
    idx = EXACT if exact_idx else [0, 10, 11, 12, 15, 21, 22, 23]      # (an index may move where two values lie within the tolerance of each other)
    assert np.array_equal(rec[idx], ref[idx]), (what, rec[idx], ref[idx])


# ---------------------------------------------------------------- parking
def with_obstacles(c, n):
    """the case with its obstacle list cut or repeated to n obstacles (0 .. 16; a repeated obstacle ties with its original: ties go to the smaller index)"""
    v = np.asarray(c["vOb"], np.int32); off = np.r_[0, np.cumsum(v)]; A = np.asarray(c["A"], float).reshape(-1, 2); b = np.asarray(c["b"], float).ravel()
    pick = [j % len(v) for j in range(n)]
    return dict(c, vOb=v[pick], A=np.concatenate([A[off[j]:off[j + 1]] for j in pick]).reshape(-1, 2) if n else np.zeros((0, 2)),
                b=np.concatenate([b[off[j]:off[j + 1]] for j in pick]) if n else np.zeros(0))


def park_instance(c, seed=0, strides=None, x0=None, xF=None, lp=None, npp=None, ref=None):
    """a rollout case (x (4,N+1), u (2,N), ts, Ts, L, ego, vOb, A, b) as an instance of a solved resident batch: its record and iterate as the kernel addresses them, in
    rows of `strides` (s_prob, s_z; default: its own), pattern / NaN wherever the step may not write / read.  X0 of the record is NOT the solution's node 0 unless given:
    the plant starts at X0.  Multipliers and reference are seeded numbers unless given (the restart copies them)."""
    rng = np.random.default_rng(seed); N = c["N"]; N1 = N + 1; v = np.asarray(c["vOb"], np.int64); nOb, M = len(v), int(v.sum())
    A = np.asarray(c["A"], float).reshape(M, 2); b = np.asarray(c["b"], float).ravel(); L = P.layout(N, nOb, M)
    s_prob, s_z = strides or (P.OB_HDR + 3 * N1, L["len"])
    lp = rng.uniform(0.1, 2, (M, N1)) if lp is None else np.asarray(lp, float); npp = rng.uniform(0.1, 2, (4 * nOb, N1)) if npp is None else np.asarray(npp, float)
    ref = rng.normal(size=(3, N1)) if ref is None else np.asarray(ref, float)
    x0 = c["x"][:, 0] + 1e-3 * rng.normal(size=4) if x0 is None else np.asarray(x0, float); xF = c["x"][:, -1] + 0.25 if xF is None else np.asarray(xF, float)
    if nOb:
        p = P.pack_problem(x0, xF, N, c["Ts"], c["L"], c["ego"], [-100, 100, -100, 100], v, A, b, *ref, 0)
    else:      # (the packing refuses an empty list: one row, then taken out of the header again)
        p = P.pack_problem(x0, xF, N, c["Ts"], c["L"], c["ego"], [-100, 100, -100, 100], [1], [[1.0, 0.0]], [0.0], *ref, 0)
        p[P.PH["NOB"]] = p[P.PH["M"]] = 0; p[P.PH["VOB"]] = 0; p[P.PH["ROFF"] + 1] = 0; p[P.PH["A"]:P.PH["A"] + 2] = 0
    prob = pattern(s_prob, 1); prob[:len(p)] = p
    z = SC.iterate_of(N, v, A, c["x"], c["u"], lp, npp, zlen=s_z); t = float(np.ravel(c["ts"])[0]); z[L["t"]] = t
    return dict(c, vOb=v.astype(np.int32), A=A, b=b, nOb=nOb, M=M, t=t, x0=x0, xF=xF, lp=lp, npp=npp, ref=ref, prob=prob, z=z, z0=pattern(s_z, 3), tmp=np.full(s_z, np.nan))


def emu_parking(insts, shift, substeps=8, kick=None, need=V.DMIN, rev=0, log=None, cap=0, logged=0, vmax=None, expect=0):
    """instances of one horizon and one pair of strides through the kernel text; kick (B,4) or None; log (B,cap,4) written in place or None.  Returns dict(out (B,40),
    st (B,4), prob, z0, tmp); no argument but `log` is modified."""
    B = len(insts); N = insts[0]["N"]
    prob, z, z0, tmp = (np.ascontiguousarray(np.stack([c[k] for c in insts])) for k in ("prob", "z", "z0", "tmp"))
    out = np.full((B, V.ADV_OUT), -7.0); st = np.full((B, 4), -7.0); kk = None if kick is None else np.ascontiguousarray(np.reshape(kick, (B, 4)), float)
    vm = vmax or max([int(c["vOb"].max()) for c in insts if c["nOb"]] + [1])
    rc = emu().emu_advance_parking(B, N, int(shift), dp(prob), prob.shape[1], dp(z), dp(z0), dp(tmp), z.shape[1], vm, int(substeps), dp(kk), float(need), int(rev), dp(st),
                                   dp(log), int(cap), int(logged), dp(out))
    assert rc == expect, (rc, emu().emu_advance_last_error())
    return dict(out=out, st=st, prob=prob, z0=z0, tmp=tmp)


def ref_parking(c, shift, substeps=8, kick=None, need=V.DMIN, logged=-1):
    """the numpy statement of the step of instance c: (record (40,), X (4, shift+1) before the kick, state (4,))"""
    X, poses, st, ok = V.advance_parking(c["x"], c["u"], c["t"], c["Ts"], c["L"], shift, substeps, c["x0"], kick)
    tab = (RC.host_pose_table(c, poses) if c["nOb"] else np.zeros((len(poses), 0))) if ok else np.full((len(poses), max(1, c["nOb"])), np.nan)
    return V.advance_record(c["x"], X, tab, st, c["xF"], shift, substeps, need, c["t"] * c["Ts"], logged, ok), X, st


def restart_parking(c, shift, state):
    """(prob, z0) the existing numpy shift asks for when it is given `state` as x0_new: X0, the reference and the primal part of z0 rewritten, every other word as it was"""
    N = c["N"]; N1 = N + 1; L = P.layout(N, c["nOb"], c["M"])
    s = SC.numpy_shift(N, shift, c["x"], c["u"], c["lp"], c["npp"], *c["ref"], state)
    z0 = c["z0"].copy(); z0[:L["nprimal"]] = SC.start_of(N, c["vOb"], c["A"], s)[:L["nprimal"]]
    prob = c["prob"].copy(); prob[P.PH["X0"]:P.PH["X0"] + 4] = s["x0"]
    prob[P.OB_HDR:P.OB_HDR + 3 * N1] = np.concatenate([s["rx"], s["ry"], s["ryaw"]])
    return prob, z0


# ---------------------------------------------------------------- quadcopter
def quad_instance(c, seed=0, x0=None, xF=None, flag=1.0, xWS=None, timeWS=1.25):
    """a rollout case (x (12,N+1), u (4,N), ts, Ts, R, ob) as an instance of a solved resident batch: record, iterate (x, u, t; NaN elsewhere), info (exit flag `flag`)"""
    rng = np.random.default_rng(seed); N = c["N"]; L = P.quad_layout(N); t = float(np.ravel(c["ts"])[0])
    x0 = c["x"][:, 0] + 1e-3 * rng.normal(size=12) if x0 is None else np.asarray(x0, float); xF = c["x"][:, -1] + 0.25 if xF is None else np.asarray(xF, float)
    xWS = rng.normal(size=(N + 1, 12)) if xWS is None else np.asarray(xWS, float)
    prob = P.pack_quad_problem(x0, xF, N, c["Ts"], c["R"], c["ob"], xWS, timeWS, 0)
    z = QS.iterate_of(N, c["x"], t); z[L["u"]:L["u"] + 4 * N] = np.ascontiguousarray(np.asarray(c["u"], float).T).reshape(-1)
    info = np.zeros(8); info[7] = flag
    return dict(c, t=t, x0=x0, xF=xF, prob=prob, z=z, info=info)


def emu_quad(insts, shift, substeps=8, kick=None, xF_new=None, need=0.0, rev=0, log=None, cap=0, logged=0, expect=0):
    B = len(insts); N = insts[0]["N"]
    prob, z, info = (np.ascontiguousarray(np.stack([c[k] for c in insts])) for k in ("prob", "z", "info"))
    out = np.full((B, V.ADV_OUT), -7.0); st = np.full((B, 12), -7.0)
    kk, xf = (None if a is None else np.ascontiguousarray(np.reshape(a, (B, 12)), float) for a in (kick, xF_new))
    rc = emu().emu_advance_quad(B, N, int(shift), dp(prob), prob.shape[1], dp(z), z.shape[1], dp(info), int(substeps), dp(kk), dp(xf), float(need), int(rev), dp(st), dp(log),
                                int(cap), int(logged), dp(out))
    assert rc == expect, (rc, emu().emu_advance_last_error())
    return dict(out=out, st=st, prob=prob)


def ref_quad(c, shift, substeps=8, kick=None, xF_new=None, need=0.0, logged=-1):
    X, poses, st, ok = V.advance_quad(c["x"], c["u"], c["t"], c["Ts"], shift, substeps, c["x0"], kick)
    tab = V.quad_point_clearance(poses, c["ob"], c["R"]) if ok else np.full((len(poses), 5), np.nan)
    return V.advance_record(c["x"], X, tab, st, c["xF"] if xF_new is None else xF_new, shift, substeps, need, c["t"] * c["Ts"], logged, ok), X, st


def restart_quad(c, shift, state, xF_new=None):
    """the problem record the existing numpy shift asks for when it is given `state` as x0_new"""
    return QS.numpy_shift(c["N"], shift, c["prob"], c["z"], c["info"], state, xF_new)
