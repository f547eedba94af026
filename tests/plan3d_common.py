"""Shared by tests/test_plan3d_cpu.py and tests/test_gpu_plan3d.py: the host build of the device planner (tests/emu/plan3d_emu.cpp), the end points of the tests, path
costs and the tolerance of the cost comparison."""
import ctypes as C
import numpy as np
from obca_amd import buildflags, scenarios as S, planner as PL

D = C.POINTER(C.c_double); I = C.POINTER(C.c_int); F = C.POINTER(C.c_float)
ROOM = np.array(PL.QUAD_ROOM, float); RES = 0.25; CLEAR = 0.4
DIMS = tuple(int(np.floor(r / RES)) + 1 for r in ROOM)      # (41, 41, 21)
_emu = None


def dp(a):
    return None if a is None else a.ctypes.data_as(D)


def ip(a):
    return None if a is None else a.ctypes.data_as(I)


def emu():
    """tests/emu/libobca_plan3d_emu.so, compiled the way the other host emulations are"""
    global _emu
    if _emu is None:
        lib = C.CDLL(buildflags.build("plan3d_emu"))
        lib.emu_plan3d_last_error.restype = C.c_char_p
        lib.emu_plan3d_paths_batch.argtypes = [C.c_int, D, D, C.c_int, D, C.c_double, D, C.c_double, D, C.c_int, I, I, C.c_int, F]
        lib.emu_plan3d_warm_start_batch.argtypes = [C.c_int, C.c_int, D, D, C.c_int, D, C.c_double, D, C.c_double, D, I, D]
        _emu = lib
    return _emu


def boxes_of(boxes, B):
    bx = np.asarray(S.QUAD_OB if boxes is None else boxes, float)
    bx = bx.reshape(-1, 6) if bx.ndim < 3 else bx
    return np.ascontiguousarray(np.broadcast_to(bx, (B,) + bx.shape[-2:]))


def emu_paths(starts, goals, boxes=None, cap=256, reverse=0, field=False, room=ROOM, res=RES, clear=CLEAR, nbox=None):
    """the emulated obca_plan3d_paths_batch: (rc, paths (B, cap, 3), counts, sweeps[, fields (B, ncell) float32])"""
    s = np.ascontiguousarray(np.asarray(starts, float).reshape(-1, 3)); g = np.ascontiguousarray(np.asarray(goals, float).reshape(-1, 3)); B = len(s)
    bx = boxes_of(boxes, B); rm = np.ascontiguousarray(room, float)
    paths = np.zeros((B, max(cap, 0), 3)); cnt = np.zeros(B, np.int32); sw = np.zeros(B, np.int32)
    fl = np.zeros((B, int(np.prod([int(np.floor(r / res)) + 1 for r in rm]))), np.float32) if field else None
    rc = emu().emu_plan3d_paths_batch(B, dp(s), dp(g), bx.shape[1] if nbox is None else nbox, dp(bx), clear, dp(rm), res, dp(paths), cap, ip(cnt), ip(sw), reverse,
                                      None if fl is None else fl.ctypes.data_as(F))
    return (rc, paths, cnt, sw, fl) if field else (rc, paths, cnt, sw)


def emu_warm_start(x0, xF, N, boxes=None, with_paths=False):
    """the emulated obca_plan3d_warm_start_batch: (rc, xWS (B, N+1, 12), counts[, paths (B, WS_CAP, 3)])"""
    a = np.ascontiguousarray(np.asarray(x0, float).reshape(-1, 12)); b = np.ascontiguousarray(np.asarray(xF, float).reshape(-1, 12)); B = len(a)
    bx = boxes_of(boxes, B)
    xWS = np.zeros((B, N + 1, 12)); cnt = np.zeros(B, np.int32); paths = np.zeros((B, PL.PLAN3D_WS_CAP, 3)) if with_paths else None
    rc = emu().emu_plan3d_warm_start_batch(B, N, dp(a), dp(b), bx.shape[1], dp(bx), CLEAR, dp(ROOM), RES, dp(xWS), ip(cnt), dp(paths))
    return (rc, xWS, cnt, paths) if with_paths else (rc, xWS, cnt)


def endpoints(n, seed=20261017, shipped=True):
    """n random end-point pairs of scenarios._draw_quad_endpoints (+ the shipped QUAD_X0 -> QUAD_XF in front): (x0 (B, 12), xF (B, 12))"""
    rng = np.random.default_rng(seed)
    pairs = [S._draw_quad_endpoints(rng) for _ in range(n)]
    B = n + int(shipped)
    x0 = np.zeros((B, 12)); xF = np.zeros((B, 12))
    if shipped:
        x0[0] = S.QUAD_X0; xF[0] = S.QUAD_XF
    for i, (a, b) in enumerate(pairs):
        x0[i + int(shipped), :3] = a; xF[i + int(shipped), :3] = b
    return x0, xF


def host_paths(x0, xF, boxes=None):
    """PL.astar3d per instance: list of (K, 3) or None; -2 (blocked end point) is None too, as astar3d reports it"""
    bx = boxes_of(boxes, len(x0))
    return [PL.astar3d(x0[i, :3], xF[i, :3], bx[i], CLEAR, ROOM, RES) for i in range(len(x0))]


def chain_cost(wp):
    """cost of a way-point list (start point, grid nodes, goal point) on the grid: the fp64 length of its chain of nodes, and the number of steps"""
    ch = np.asarray(wp, float)[1:-1]
    return float(np.sqrt(((ch[1:] - ch[:-1]) ** 2).sum(1)).sum()), len(ch) - 1


def cost_tolerance(wa, wb):
    """Both searches minimise the SAME cost: the sum of the fp32 edge weights (float)(res sqrt(d2)) along the chain.  The host A* is optimal for it because its Euclidean
    heuristic is consistent on this grid; the relaxation's fixed point is optimal by construction.  What each code calls the cost of its path is an fp32 sum of at most K
    terms, each addition rounded by at most half an ulp of a number <= the largest cost g: |computed - exact| <= K g 2^-24 (the rounding of the weights themselves, <= g 2^-24
    in all, is inside the same bound because a chain has fewer additions than steps + 1).  So two optimal chains, costs recomputed in fp64, differ by at most that once per code."""
    (ca, ka), (cb, kb) = chain_cost(wa), chain_cost(wb)
    return 2.0 * max(ka, kb) * max(ca, cb) * 2.0 ** -24


def assert_valid_path(wp, start, goal, boxes=None, what=""):
    """way-points outside the inflated boxes and inside the room, consecutive grid nodes 26-neighbours, first / last way-point the exact end points"""
    wp = np.asarray(wp, float); bx = np.asarray(S.QUAD_OB if boxes is None else boxes, float).reshape(-1, 6)
    assert len(wp) >= 3 and np.array_equal(wp[0], np.asarray(start, float)[:3]) and np.array_equal(wp[-1], np.asarray(goal, float)[:3]), what
    assert (wp >= 0).all() and (wp <= ROOM).all(), what
    for p in wp:
        inside = (p <= bx[:, :3] + CLEAR).all(1) & (p >= -bx[:, 3:] - CLEAR).all(1)
        assert not inside.any(), (what, p)
    idx = np.rint(wp[1:-1] / RES).astype(int)
    assert np.array_equal(idx * RES, wp[1:-1]), what
    if len(idx) > 1:
        d = np.abs(np.diff(idx, axis=0))
        assert d.max() <= 1 and (d.sum(1) > 0).all(), what
