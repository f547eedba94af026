"""What tests/test_hybrid_cpu.py and tests/test_gpu_hybrid.py share: the host build of the device planner (tests/emu/hybrid_emu.cpp), the inputs of the issue's cases
(computed once per process) and the validity rules of a returned path."""
import ctypes as C
import functools
import numpy as np
from obca_amd import buildflags, planner as PL, scenarios as S

CAP = 1024
NODES = 1 << 18      # node pool of the host build in the tests (the default of the device is 1 << 20): enough for every case here, and quick to allocate
_lib = None


def emu():
    global _lib
    if _lib is None:
        _lib = C.CDLL(buildflags.build("hybrid_emu"))
        _lib.emu_hybrid_last_error.restype = C.c_char_p
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        _lib.emu_hybrid_astar_batch.argtypes = [C.c_int, dp, dp, C.c_int, ip, dp, dp, dp, C.c_double, dp, dp, C.c_int, C.c_double, dp, ip, C.c_int, ip, ip, ip,
                                                C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_ubyte), ip]
    return _lib


def _p(a, t=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def field(sc):
    A, b, vrows = S.scenario_hrep(sc)
    return np.ascontiguousarray(vrows, np.int32), np.ascontiguousarray(A, float), np.ascontiguousarray(b, float)


def opts_array(kw):
    o = dict(PL.DEFAULT_OPTS); o.update(kw)
    return np.array([o[k] for k in PL.DEFAULT_OPTS], float)


def run_emu(sc, starts, goals, kw=None, bw=0.0, slots=1, nodes=NODES, chunks=0, order=0, cap=CAP, want_map=False, ego=S.EGO, XYbounds=S.XYBOUNDS, field_=None):
    """the host build on a batch: dict(rc, paths, dirs, counts, expansions, rounds[, map, blocked, dims])"""
    v, A, b = field(sc) if field_ is None else field_
    s = np.ascontiguousarray(np.asarray(starts, float)[:, :3]); g = np.ascontiguousarray(np.asarray(goals, float)[:, :3]); B = len(s)
    o = opts_array(kw or {}); e = np.ascontiguousarray(ego, float); xy = np.ascontiguousarray(XYbounds, float)
    out = dict(paths=np.full((B, cap, 3), 7.0), dirs=np.full((B, cap), 7, np.int32), counts=np.full(B, 99, np.int32), expansions=np.zeros(B, np.int32), rounds=np.zeros(B, np.int32))
    mp = np.zeros(OBCA_HYBRID_MAXMAP, np.float32) if want_map else None; bl = np.zeros(OBCA_HYBRID_MAXMAP, np.uint8) if want_map else None; dims = np.zeros(2, np.int32)
    out["rc"] = emu().emu_hybrid_astar_batch(B, _p(s), _p(g), len(v), _p(v, C.c_int), _p(A), _p(b), _p(e), S.L_WHEELBASE, _p(xy), _p(o), len(o), float(bw), _p(out["paths"]),
                                             _p(out["dirs"], C.c_int), cap, _p(out["counts"], C.c_int), _p(out["expansions"], C.c_int), _p(out["rounds"], C.c_int),
                                             slots, nodes, chunks, order, _p(mp, C.c_float), _p(bl, C.c_ubyte), _p(dims, C.c_int))
    if want_map:
        nx, ny = int(dims[0]), int(dims[1])
        out.update(map=mp[:nx * ny].reshape(ny, nx), blocked=bl[:nx * ny].reshape(ny, nx), dims=(nx, ny))
    return out


OBCA_HYBRID_MAXMAP = 35000
FIELDS = ("paths", "dirs", "counts", "expansions", "rounds")


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in FIELDS)


@functools.lru_cache(None)
def poses(which, B):
    """the issue's inputs: backwards poses of sample_poses(BACKWARDS, B, default_rng(3)); parallel poses with goal jitter from the same seed"""
    sc = S.BACKWARDS if which == "backwards" else S.PARALLEL
    x0, xF = S.sample_poses(sc, B, np.random.default_rng(3), goal_jitter=which == "parallel")
    return sc, x0, xF, dict(PL.SCENARIO_OPTS[which][0])


@functools.lru_cache(None)
def host_plan(which, B):
    sc, x0, xF, kw = poses(which, B)
    v, A, b = field(sc)
    return PL._hybrid_astar_dense(x0, xF, v, A, b, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, 0, CAP, kw)


@functools.lru_cache(None)
def emu_plan(which, B, order=0, slots=1, analytic=None, bw=0.0):
    sc, x0, xF, kw = poses(which, B)
    if analytic is not None:
        kw = dict(kw, analytic=analytic)
    return run_emu(sc, x0, xF, kw, bw=bw, slots=slots, order=order)


def check_path(sc, start, goal, path, dirs, margin, exact_goal=True, what=""):
    """the validity rules of the issue: from the start pose onto the exact goal pose, nodes <= 0.2 m + 1e-9 apart, dirs +-1, every node free of the planner's own collision test"""
    v, A, b = field(sc)
    assert len(path) >= 2 and len(path) == len(dirs), what
    assert np.array_equal(path[0, :2], np.asarray(start, float)[:2]) and abs(np.angle(np.exp(1j * (path[0, 2] - start[2])))) < 1e-12, (what, path[0], start)
    if exact_goal:
        assert np.abs(path[-1, :2] - np.asarray(goal, float)[:2]).max() < 1e-9 and abs(np.angle(np.exp(1j * (path[-1, 2] - goal[2])))) < 1e-9, (what, path[-1], goal)
    assert np.hypot(np.diff(path[:, 0]), np.diff(path[:, 1])).max() <= 0.2 + 1e-9, what
    assert set(np.unique(dirs).tolist()) <= {1, -1}, what
    for k, p in enumerate(path):
        assert not PL.collides(p, v, A, b, margin=margin), (what, k, p)
