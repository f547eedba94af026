"""What tests/test_path_ws_cpu.py and tests/test_gpu_path_ws.py share: the host build of the kernel text of obca_amd/csrc/obca_path_ws.h (tests/emu/path_ws_emu.cpp,
emu_path_ws_*, buildflags.build("path_ws_emu")), called with guard words around every output array; synthetic planner paths; the numpy statement (planner.path_to_warm_start) of a batch; the comparison.

Tolerances (bounds, not measurements): Ts, poses, v, a within 1e-11 -- values of at most 50 m or rad, at most 1 024 accumulated terms, unit roundoff 1.1e-16 --, the steering
angle within 1e-9 -- that pose error over the smallest ds (about 0.1 m), times L; where either side sits on the +-0.6 clip the other is compared clipped, which both are."""
import ctypes as C
import numpy as np
from obca_amd import buildflags, planner as PL, scenarios as S

GUARD = 16                      # guard words in front of and behind every output array
SENTINEL = -7.25e77             # their value (int arrays: its int32 cast of the bits does not matter, they get -77777)
MAXNODES = 1024
TOL, TOL_DELTA = 1e-11, 1e-9
_lib = None


def emu():
    global _lib
    if _lib is None:
        lib = C.CDLL(buildflags.build("path_ws_emu"))
        D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.emu_path_ws_batch.restype = C.c_int
        lib.emu_path_ws_batch.argtypes = [C.c_int, C.c_int, D, I, I, C.c_int, D, C.c_double, C.c_double, C.c_double, D, D, D, I]
        lib.emu_path_ws_last_error.restype = C.c_char_p
        lib.emu_path_ws_limits.argtypes = [I, I]
        lib.emu_path_ws_record.restype = C.c_int
        lib.emu_path_ws_record.argtypes = [C.c_int, C.c_int, C.c_int, D, I, C.c_int, C.c_double, C.c_double, D, D, C.c_int]
        _lib = lib
    return _lib


def _ptr(a, ct):
    return None if a is None else a.ctypes.data_as(C.POINTER(ct))


def _guarded(n, dtype):
    full = np.full(n + 2 * GUARD, SENTINEL if dtype == float else -77777, dtype)
    return full, full[GUARD:GUARD + n]


def emu_batch(paths, dirs, counts, N, xF=None, v_nom=0.5, L=S.L_WHEELBASE, a_max=0.0, B=None, cap=None, null=()):
    """emu_path_ws_batch on the arrays as they are: (rc, Ts (B,), xWS (B, N+1, 4), uWS (B, N, 2), status (B,)); asserts that the guard words around the four outputs came back
    untouched.  B / cap override what the arrays say (argument checks); null: names of arrays passed as NULL."""
    paths = np.ascontiguousarray(paths, float); dirs = np.ascontiguousarray(dirs, np.int32); counts = np.ascontiguousarray(counts, np.int32)
    nB = len(counts); Bc = nB if B is None else B; capc = paths.shape[1] if cap is None else cap
    xf = None if xF is None else np.ascontiguousarray(np.reshape(xF, (nB, 4)), float)
    Nn = max(int(N), 0)
    full = {}; view = {}
    for k, (n, dt) in dict(Ts=(nB, float), xWS=(nB * 4 * (Nn + 1), float), uWS=(nB * 2 * Nn, float), status=(nB, np.int32)).items():
        full[k], view[k] = _guarded(n, dt)
    arg = dict(paths=_ptr(paths, C.c_double), dirs=_ptr(dirs, C.c_int), counts=_ptr(counts, C.c_int), Ts=_ptr(view["Ts"], C.c_double), xWS=_ptr(view["xWS"], C.c_double),
               uWS=_ptr(view["uWS"], C.c_double), status=_ptr(view["status"], C.c_int))
    for k in null:
        arg[k] = None
    rc = emu().emu_path_ws_batch(Bc, int(N), arg["paths"], arg["dirs"], arg["counts"], capc, _ptr(xf, C.c_double), v_nom, L, a_max, arg["Ts"], arg["xWS"], arg["uWS"], arg["status"])
    for k, f in full.items():
        g = SENTINEL if f.dtype == float else -77777
        assert (f[:GUARD] == g).all() and (f[-GUARD:] == g).all(), "guard words of %s were written" % k
    return rc, view["Ts"].copy(), view["xWS"].reshape(nB, Nn + 1, 4).copy(), view["uWS"].reshape(nB, Nn, 2).copy(), view["status"].copy()


def numpy_batch(paths, dirs, counts, N, xF=None, v_nom=0.5, L=S.L_WHEELBASE, a_max=0.0):
    """planner.path_to_warm_start per instance (a_max: 0 or the 0.3 its smoothing is fixed at); instances with count < 2 stay zero"""
    assert a_max in (0.0, 0.3)
    B = len(counts); Ts = np.zeros(B); xWS = np.zeros((B, N + 1, 4)); uWS = np.zeros((B, N, 2))
    for i in range(B):
        c = int(counts[i])
        if 2 <= c <= paths.shape[1]:
            Ts[i], xWS[i], uWS[i] = PL.path_to_warm_start(paths[i, :c], dirs[i, :c], N, None if xF is None else np.asarray(xF, float).reshape(B, 4)[i], v_nom=v_nom, L=L, smooth=a_max > 0)
    return Ts, xWS, uWS


def compare(got, ref, sel, what):
    """got / ref: (Ts, xWS, uWS); sel: the instances to compare.  Returns the largest differences (pose and v and a and Ts, delta)."""
    (Ts, x, u), (Tr, xr, ur) = got, ref
    sel = np.asarray(sel)
    assert np.array_equal(np.sign(x[sel][:, :, 3]), np.sign(xr[sel][:, :, 3])), (what, "sign(v)", np.argwhere(np.sign(x[sel][:, :, 3]) != np.sign(xr[sel][:, :, 3]))[:5])
    e = max(np.abs(Ts[sel] - Tr[sel]).max(), np.abs(x[sel] - xr[sel]).max(), np.abs(u[sel][:, :, 1] - ur[sel][:, :, 1]).max())
    ed = np.abs(np.clip(u[sel][:, :, 0], -0.6, 0.6) - np.clip(ur[sel][:, :, 0], -0.6, 0.6)).max()
    assert e <= TOL, (what, e)
    assert ed <= TOL_DELTA, (what, ed)
    return e, ed


def make_path(rng, n, switch_at=(), yaw0=0.0, turn=1.0, step=0.2, repeat_at=None, zero_dir=(), d0=1):
    """A car-like path of n nodes: (nodes (n, 3) with the yaw wrapped into (-pi, pi], dirs (n,)).  switch_at: segment numbers (segment i ends in node i, 1 .. n-1) from
    which on the direction is reversed; turn: sign of the curvature; repeat_at: a node that repeats its predecessor (a segment of length 0); zero_dir: nodes whose direction
    entry is 0."""
    P = np.zeros((n, 3)); D = np.zeros(n, np.int32)
    x, y, yaw, d = rng.uniform(-5, 5), rng.uniform(2, 9), yaw0, d0
    P[0] = (x, y, yaw)
    for i in range(1, n):
        if i in switch_at:
            d = -d
        if i != repeat_at:
            ds = step * rng.uniform(0.6, 1.4); kap = turn * rng.uniform(0.05, 0.2)
            x += d * ds * np.cos(yaw); y += d * ds * np.sin(yaw); yaw += d * ds * kap
        P[i] = (x, y, yaw); D[i] = d
    D[0] = D[1]
    for i in zero_dir:
        D[i] = 0
    P[:, 2] = np.pi - np.mod(np.pi - P[:, 2], 2 * np.pi)      # (-pi, pi]
    return P, D


NODE_COUNTS = (2, 3, 63, 64, 65, 129, 1024)


def synthetic(seed=3, counts=NODE_COUNTS, cap=MAXNODES):
    """The edge shapes as one batch: per node count -- no switch; one switch; three switches, the first on the first segment that can carry one and the last on the last
    segment; the yaw running across +pi and across -pi; a repeated node; direction entries of 0; a short step (long ramps for the smoother) -- and, in the middle of the
    batch, an instance without a path.  Returns (paths (B, cap, 3), dirs (B, cap), counts (B,), xF (B, 4)); rows beyond a count hold NaN / 9: nothing may read them."""
    rng = np.random.default_rng(seed); inst = []
    for n in counts:
        step = 0.05 if n >= 1024 else 0.2      # (1 024 nodes stay within the 50 m the tolerance is derived for)
        kinds = [dict(), dict(yaw0=3.0, turn=1.0), dict(yaw0=-3.0, turn=-1.0), dict(d0=-1, yaw0=3.1, turn=-1.0), dict(step=step / 8)]
        if n >= 3:
            kinds += [dict(switch_at=(2,)), dict(switch_at=(n - 1,)), dict(repeat_at=n // 2), dict(repeat_at=n - 1), dict(zero_dir=(1,)), dict(zero_dir=(n - 1,))]
        if n >= 5:
            kinds += [dict(switch_at=(2, n // 2, n - 1)), dict(switch_at=(2, n // 2, n - 1), step=step / 8), dict(repeat_at=1, zero_dir=(n // 2,), switch_at=(n // 2 + 1,))]
        for kw in kinds:
            kw = dict(dict(step=step), **kw)
            inst.append(make_path(rng, n, **kw))
    inst.insert(len(inst) // 2, (np.zeros((0, 3)), np.zeros(0, np.int32)))
    B = len(inst)
    paths = np.full((B, cap, 3), np.nan); dirs = np.full((B, cap), 9, np.int32); cnt = np.zeros(B, np.int32); xF = np.zeros((B, 4))
    for i, (P, D) in enumerate(inst):
        cnt[i] = len(P); paths[i, :len(P)] = P; dirs[i, :len(P)] = D
        if len(P):
            xF[i, :3] = P[-1] + rng.uniform(-0.05, 0.05, 3)
    return paths, dirs, cnt, xF


def planner_paths(sc, B=96, seed=7, with_x0=False):
    """the planner's dense arrays for sample_poses(sc, B, default_rng(seed)), planned with SCENARIO_OPTS: (paths, dirs, counts, xF[, x0])"""
    x0, xF = S.sample_poses(sc, B, np.random.default_rng(seed))
    A, b, vrows = S.scenario_hrep(sc)
    o, _ = PL.SCENARIO_OPTS.get(sc["name"], (dict(), 0.5))
    _, _, paths, dirs, cnt, _ = PL._hybrid_astar_dense(x0[:, :3], xF[:, :3], vrows, A, b, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, PL.effective_cpus(), 1024, dict(o))
    return (paths, dirs, cnt, xF, x0) if with_x0 else (paths, dirs, cnt, xF)


def synthetic67():
    """67 of the synthetic instances: every one with 63, 64, 65 or 1 024 nodes and the one without a path, filled up from the other node counts; batch order kept"""
    paths, dirs, cnt, xF = synthetic()
    first = [i for i in range(len(cnt)) if cnt[i] in (0, 63, 64, 65, 1024)]
    keep = sorted(first + [i for i in range(len(cnt)) if i not in first][:67 - len(first)])
    assert len(keep) == 67
    return paths[keep], dirs[keep], cnt[keep], xF[keep]
