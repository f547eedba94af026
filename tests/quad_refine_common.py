"""What tests/test_quad_refine_cpu.py, tests/test_gpu_quad_refine.py and tests/golden/make_quad_refine_cases.py share: the host build of the kernel text of
obca_amd/csrc/obca_quad_subdivide.h (tests/emu/quad_subdivide_emu.cpp, buildflags.build("quad_subdivide_emu")); the trajectories both suites run -- the never-solved warm
starts of clearance_common.quad_cases with its wavy timeScale --; a source instance packed as a resident batch holds it (problem record, last iterate, info) with the numpy
statement of what its refinement must be; the refined problem as the CPU oracle takes it; the cases of tests/golden/quad_refine_cases.npz.

Tolerance.  A refined word is one division, at most two products and one sum on numbers of size <= 20 (one rounding is 4e-15 there), numpy and g++ without contraction, the
device with the product kept from fusing into the sum: bits are expected, and every comparison asserts clearance_common.TOL_QUAD = 1e-12 and records the largest difference."""
import ctypes as C
import functools
import numpy as np
import packing as P
import clearance_common as K
import quad_shift_common as QS
from obca_amd import buildflags, validate as V

D = C.POINTER(C.c_double)
TOL = K.TOL_QUAD
SHAPES = ((1, 1), (2, 3), (7, 4), (60, 2), (4, 32), (128, 1))      # (N, r): 24 and 84 words (under and just over 64), ..., the largest factor, the largest horizon
SENTINEL = -7.25
WORST = {}      # the largest differences seen, printed by the last test of each suite
dp = K.dp

# tests/golden/quad_refine_cases.npz: (N, B, factor, margin) -- the coarse batches are make_quad_batch(B, N); clearance at 8 samples per COARSE interval
FIXTURE_CASES = ((20, 16, 2, 0.0), (20, 16, 4, 0.0), (20, 16, 4, 0.02), (60, 8, 2, 0.0), (60, 8, 2, 0.005))
S_COARSE = 8


def case_key(N, r, margin):
    return "N%d_r%d_m%g" % (N, r, margin)


def note(key, a, b):
    """record the largest difference under `key`; returns it"""
    a = np.asarray(a, float); b = np.asarray(b, float)
    d = float(np.abs(a - b).max()) if a.size else 0.0
    WORST[key] = max(WORST.get(key, 0.0), d)
    return d


@functools.lru_cache(None)
def emu():
    lib = C.CDLL(buildflags.build("quad_subdivide_emu"))
    lib.emu_quad_subdivide_last_error.restype = C.c_char_p
    lib.emu_quad_subdivide_check_args.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double]
    lib.emu_quad_subdivide_host.argtypes = [C.c_int, C.c_int, C.c_double, D, D, C.c_int, D, D]
    lib.emu_quad_subdivide_record.argtypes = [C.c_int, C.c_int, C.c_double, D, D, D, C.c_int, D, C.POINTER(C.c_int)]
    a, b, c = (C.c_int(0) for _ in range(3))
    lib.emu_quad_subdivide_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (32, P.QUAD_NMAX, P.QPH_SIZE)
    return lib


def cases(N, B=6):
    """clearance_common.quad_cases(N): the warm starts of make_quad_batch(B, N) with velocities that do not quite lead from node to node, timeScale 1 + 0.1 sin k"""
    return K.quad_cases(N, B)


# ---------------------------------------------------------------- the host-pointer form
def emu_host(c, r, rev=0, ts="own"):
    """one instance through subdivide_host_instance: (rc, Ts', x' (12, rN+1)); the outputs are exactly as long as the call writes them, behind them a sentinel"""
    N = c["N"]; Nf = N * r
    x = np.ascontiguousarray(c["x"].T); t = None if ts is None else np.ascontiguousarray(c["ts"] if isinstance(ts, str) else ts, float)
    Tsf = np.full(1, SENTINEL); xf = np.full((Nf + 1) * 12 + 5, SENTINEL)
    rc = emu().emu_quad_subdivide_host(N, int(r), float(c["Ts"]), dp(x), dp(t), int(rev), dp(Tsf), dp(xf))
    assert rc in (0, 1), emu().emu_quad_subdivide_last_error()
    assert (xf[-5:] == SENTINEL).all()
    return rc, Tsf[0], xf[:-5].reshape(Nf + 1, 12).T.copy()


def emu_host_batch(x, ts, Ts, r):
    """the host build over a batch: x (B,12,N+1), ts (B,N+1) or None, Ts scalar or (B,) -> (Ts' (B,), x' (B,12,rN+1)) -- what the device's host-pointer call must return"""
    B, _, N1 = x.shape; Ts = np.broadcast_to(np.asarray(Ts, float), (B,))
    out = [emu_host(dict(N=N1 - 1, Ts=Ts[i], x=x[i], ts=None if ts is None else ts[i]), r, ts=None if ts is None else "own") for i in range(B)]
    return np.array([o[1] for o in out]), np.stack([o[2] for o in out])


# ---------------------------------------------------------------- the resident form
def source(c, seed=0, flag=1.0, t=None):
    """instance c as a solved resident batch holds it: the problem record with an uploaded warm start of its own (another trajectory, timeWS 1.25, dual_ws 0, a start and a
    goal), the last iterate -- x of the case and one t, everything else NaN: nothing else may be read (quad_shift_common.iterate_of) --, info with exit flag `flag`"""
    rng = np.random.default_rng(2000 + seed); N = c["N"]
    up = c["x"] + 0.05 * rng.standard_normal((12, N + 1)); x0 = rng.standard_normal(12); xF = rng.standard_normal(12)
    prob = P.pack_quad_problem(x0, xF, N, c["Ts"], c["R"], c["ob"], up.T, 1.25, 0)
    t = float(c["ts"][min(1, N)] if t is None else t)
    info = np.array([0.0, 23.0, 1.5, 1e-9, 1e-7, 1e-9, 0.0, flag])
    return dict(c=c, N=N, prob=prob, z=QS.iterate_of(N, c["x"], t), info=info, t=t, up=up)


def emu_record(src, r, margin=0.0, rev=0):
    """the instance through subdivide_record into a sentinel-filled record: (status, pd)"""
    N, Nf = src["N"], src["N"] * r
    pd = np.full(P.quad_problem_len(Nf) + 5, SENTINEL); st = C.c_int(99)
    rc = emu().emu_quad_subdivide_record(N, int(r), float(margin), dp(src["prob"]), dp(src["z"]), dp(src["info"]), int(rev), dp(pd), C.byref(st))
    assert rc == 0, emu().emu_quad_subdivide_last_error()
    assert (pd[-5:] == SENTINEL).all()      # nothing behind the record
    return st.value, pd[:-5]


def expected_record(prob, N, r, margin, status, x=None, t=None):
    """the destination record the numpy statement asks for: prob the source's record, x (12,N+1) / t its solution (status 0)"""
    Nf = N * r; pd = np.zeros(P.quad_problem_len(Nf)); pd[:P.QPH_SIZE] = prob[:P.QPH_SIZE]
    Ts = prob[P.QPH_TS]; pd[P.QPH_TS] = Ts / r
    if margin != 0.0:
        pd[P.QPH_R] = prob[P.QPH_R] + margin
    if status == 0:
        pd[P.QPH_SIZE:] = V.refine_quad(x, t, Ts, r)["x"].T.reshape(-1); pd[P.QPH_TWS] = t; pd[P.QPH_DWS] = 1.0
    elif status == 1:
        up = prob[P.QPH_SIZE:].reshape(N + 1, 12).T
        pd[P.QPH_SIZE:] = V.refine_quad(up, 1.0, Ts, r, euler=False)["x"].T.reshape(-1)
    else:
        pd[P.QPH_TWS] = 1.0; pd[P.QPH_DWS] = 1.0
    return pd


def check_record(src, r, margin, status, pd, what, key="host build against numpy"):
    e = expected_record(src["prob"], src["N"], r, margin, status, src["c"]["x"], src["t"])
    assert pd.shape == e.shape and note(key, pd, e) <= TOL, (what, np.flatnonzero(pd != e)[:8])
    return e


# ---------------------------------------------------------------- the refined problem for the CPU oracle
def refined_problem(prob_f, Nf):
    """a destination record as the oracle's arguments: dict(x0, xF, Ts, R, xWS (Nf+1, 12), timeWS, dual_ws).  Row 0 of xWS is x0: the kernel's starting point holds x0 at
    stage 0 (quad_shift_common.shifted_problem)."""
    w = prob_f[P.QPH_SIZE:].reshape(Nf + 1, 12).copy(); w[0] = prob_f[P.QPH_X0:P.QPH_X0 + 12]
    return dict(x0=prob_f[P.QPH_X0:P.QPH_X0 + 12].copy(), xF=prob_f[P.QPH_XF:P.QPH_XF + 12].copy(), Ts=float(prob_f[P.QPH_TS]), R=float(prob_f[P.QPH_R]), xWS=w,
                timeWS=float(prob_f[P.QPH_TWS]), dual_ws=int(prob_f[P.QPH_DWS]))


def refined_record(bt, i, xp, t, info, r, margin):
    """instance i of the batch dict bt with the solution xp (12,N+1), t, info (8): the destination record the host build writes"""
    N = bt["N"]
    prob = P.pack_quad_problem(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], bt["timeWS"], 1)
    st, pd = emu_record(dict(N=N, prob=prob, z=QS.iterate_of(N, xp, t), info=np.asarray(info, float)), r, margin)
    return st, pd


def oracle_fine(Q, bt, i, xp, t, r, margin, opts=None):
    """the oracle's solve of instance i refined x r with `margin` from the coarse solution (xp, t) with exit flag 1, and its clearance record at S_COARSE / r samples per fine
    interval against the refined NLP's radius with need = -margin (that is: against the true radius with need 0): (result dict, record)"""
    N = bt["N"]; info = np.zeros(8); info[7] = 1.0
    st, pd = refined_record(bt, i, xp, t, info, r, margin)
    assert st == 0
    p = refined_problem(pd, N * r)
    q = Q.quadcopter_signed_dist(p["x0"], p["xF"], N * r, p["Ts"], p["R"], bt["ob"], p["xWS"], p["timeWS"], opts=opts, dual_ws=p["dual_ws"])
    rec = V.quad_clearance(q["xp"], q["t"], p["Ts"], bt["ob"], p["R"], S_COARSE // r, need=-margin)
    return q, rec
