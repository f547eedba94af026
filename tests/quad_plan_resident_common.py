"""Shared by tests/test_quad_plan_resident_cpu.py and tests/test_gpu_quad_plan_resident.py: the host build of the quadcopter planner's resident route
(tests/emu/quad_plan_resident_emu.cpp), "the 20" instances both files plan, their problem records (tests/packing.pack_quad_problem) and the host-pointer route's host build
(plan3d_common.emu_warm_start / emu_paths) they are compared with.  All at the shipped room, res 0.25, clear 0.4.

The 20: the 17 of plan3d_common.endpoints(16) (the shipped pair + 16 random ones; every one has a path), then three with boxes of their own:
  17 (a) the shipped end points, box 1 replaced by a wall across the room [5.5,10,5,-4.5,0,0]            -> count 0
  18 (b) the start (2.2, 5, 3) inside the first inflated box                                              -> count -2
  19 (c) start (1, 1, 3), goal (1.05, 1.02, 3.04) on the same grid node                                   -> count 3
Every instance carries the way-point start of scenarios.quad_warm_start and timeWS = 0.9, so that "left as it was" differs from zeros and from a planned start."""
import ctypes as C
import functools
import numpy as np
import packing as PK
import plan3d_common as K
from obca_amd import buildflags, scenarios as S, planner as PL

D = C.POINTER(C.c_double); I = C.POINTER(C.c_int)
NI = 20; A_, B_, C_ = 17, 18, 19      # the three edge instances
TWS = 0.9
SKIPPED = -4
HDR = PK.QPH_SIZE
_lib = None


def emu():
    global _lib
    if _lib is None:
        lib = C.CDLL(buildflags.build("quad_plan_resident_emu"))
        lib.emu_qpr_last_error.restype = C.c_char_p
        lib.emu_qpr_layout.argtypes = [I]
        lib.emu_qpr_plan.argtypes = [C.c_int, C.c_int, D, C.c_longlong, C.c_double, D, C.c_double, C.c_int, I, C.c_int, D, C.c_int, C.c_float, D, I, I]
        _lib = lib
    return _lib


@functools.lru_cache(None)
def the20():
    """(x0 (20, 12), xF (20, 12), ob (20, 5, 6))"""
    x0, xF = K.endpoints(16)
    x0 = np.concatenate([x0, np.zeros((3, 12))]); xF = np.concatenate([xF, np.zeros((3, 12))])
    ob = np.tile(S.QUAD_OB, (NI, 1, 1))
    x0[A_] = S.QUAD_X0; xF[A_] = S.QUAD_XF; ob[A_, 1] = [5.5, 10, 5, -4.5, 0, 0]
    x0[B_, :3] = [2.2, 5.0, 3.0]; xF[B_] = S.QUAD_XF
    x0[C_, :3] = [1.0, 1.0, 3.0]; xF[C_, :3] = [1.05, 1.02, 3.04]
    for a in (x0, xF, ob):
        a.flags.writeable = False
    return x0, xF, ob


def uploaded_start(N):
    """the start every instance is uploaded with: (xWS (20, N+1, 12), timeWS (20,))"""
    x0, xF, _ = the20()
    return np.stack([S.quad_warm_start(x0[i], xF[i], N) for i in range(NI)]), np.full(NI, TWS)


def records(N, tile=1):
    """the problem records of the 20 (tiled `tile` times) as an upload packs them: (B, QPH_SIZE + 12 (N + 1))"""
    x0, xF, ob = the20(); xws, tws = uploaded_start(N)
    p = np.stack([PK.pack_quad_problem(x0[i], xF[i], N, S.quad_sample_time(N), S.QUAD_R, ob[i], xws[i], tws[i]) for i in range(NI)])
    return np.ascontiguousarray(np.tile(p, (tile, 1)))


def plan(prob, N, clear=K.CLEAR, room=K.ROOM, res=K.RES, cap=PL.PLAN3D_WS_CAP, sel=None, n=None, timeWS=None, reverse=0, lds_fill=1e30, counts=True, paths=None):
    """the host build of the resident call over a COPY of the records: dict(rc, err, prob, paths, counts, sweeps); counts / sweeps start as 99, so a refusal shows"""
    p = np.array(prob, float); B = len(p)
    rm = None if room is None else np.ascontiguousarray(room, float)
    s = None if sel is None else np.ascontiguousarray(sel, np.int32)
    t = None if timeWS is None else np.array([timeWS], float)
    pth = np.full((B, max(int(cap), 1), 3), 7.0) if paths is None else paths
    cnt = np.full(B, 99, np.int32); sw = np.full(B, 99, np.int32)
    rc = emu().emu_qpr_plan(B, N, p.ctypes.data_as(D), p.shape[1], clear, None if rm is None else rm.ctypes.data_as(D), res, cap,
                            None if s is None else s.ctypes.data_as(I), (0 if s is None else len(s)) if n is None else n, None if t is None else t.ctypes.data_as(D),
                            reverse, lds_fill, pth.ctypes.data_as(D), cnt.ctypes.data_as(I) if counts else None, sw.ctypes.data_as(I))
    return dict(rc=rc, err=emu().emu_qpr_last_error().decode(), prob=p, paths=pth, counts=cnt, sweeps=sw)


@functools.lru_cache(None)
def planned(N, cap=PL.PLAN3D_WS_CAP, timeWS=None):
    """the resident route's host build over the 20 (cached: the 20 searches take seconds; callers do not modify it)"""
    return plan(records(N), N, cap=cap, timeWS=timeWS)


@functools.lru_cache(None)
def host_route(N):
    """the host-pointer route's host build on the same inputs: (xWS (20, N+1, 12), counts, paths (20, WS_CAP, 3))"""
    x0, xF, ob = the20()
    rc, xws, cnt, paths = K.emu_warm_start(x0, xF, N, boxes=ob, with_paths=True)
    assert rc == 0
    return xws, cnt, paths


def bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ws_of(prob, N):
    """(xWS (B, N+1, 12), timeWS (B,)) of records"""
    return prob[:, HDR:].reshape(len(prob), N + 1, 12), prob[:, PK.QPH_TWS]
