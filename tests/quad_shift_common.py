"""TEST INFRASTRUCTURE ONLY: the quadcopter receding-horizon shift (obca_amd/csrc/obca_quad_shift.h) built for the host (tests/emu/quad_shift_emu.cpp), a numpy statement of
the same rules, and the packing between a QuadBatch download and the records the shift text reads.  Shared by tests/test_quad_shift_cpu.py and tests/test_gpu_quad_restart.py."""
import ctypes as C
import numpy as np
import packing as P
from obca_amd import buildflags

D = C.POINTER(C.c_double)
_LIB = None


def dp(a):
    return None if a is None else a.ctypes.data_as(D)


def load():
    """the host build of the shift text (built aside and renamed into place: xdist workers may build at once)"""
    global _LIB
    if _LIB is not None:
        return _LIB
    _LIB = C.CDLL(buildflags.build("quad_shift_emu"))
    return _LIB


def sizes(N):
    a, b, c, d = (C.c_int(0) for _ in range(4))
    load().emu_quad_shift_sizes(C.c_int(N), C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    return a.value, b.value, c.value, d.value


def emu_shift(N, shift, prob, z, info, x0_new=None, xF_new=None):
    """one instance through the kernel text; returns the new problem record (prob, z, info are not modified)"""
    out = np.array(prob, float); z = np.ascontiguousarray(z, float); info = np.ascontiguousarray(info, float)
    keep = [None if a is None else np.ascontiguousarray(a, float) for a in (x0_new, xF_new)]
    load().emu_quad_shift(C.c_int(N), C.c_int(shift), dp(out), dp(z), dp(info), dp(keep[0]), dp(keep[1]))
    return out


def numpy_shift(N, shift, prob, z, info, x0_new=None, xF_new=None):
    """the rules of the shift stated with numpy (include/obca_hip.h, obca_quad_batch_shift_warm_start)"""
    L = P.quad_layout(N); out = np.array(prob, float)
    if info[7] in (1.0, 2.0):
        x = z[L["x"]:L["x"] + 12 * (N + 1)].reshape(N + 1, 12)
        ws = x[np.minimum(np.arange(N + 1) + shift, N)].copy()
        if xF_new is not None:
            ws[np.arange(N + 1) + shift > N] = xF_new
        out[P.QPH_SIZE:] = ws.reshape(-1)
        out[P.QPH_TWS] = z[L["t"]]; out[P.QPH_DWS] = 1.0
        if x0_new is None:
            out[P.QPH_X0:P.QPH_X0 + 12] = x[shift]
    if x0_new is not None:
        out[P.QPH_X0:P.QPH_X0 + 12] = x0_new
    if xF_new is not None:
        out[P.QPH_XF:P.QPH_XF + 12] = xF_new
    return out


def iterate_of(N, xp, t):
    """a solver-layout iterate that holds what the shift reads of a solution: the states xp (12, N+1) and t; everything else NaN (nothing else may be read)"""
    L = P.quad_layout(N); z = np.full(L["len"], np.nan)
    z[L["x"]:L["x"] + 12 * (N + 1)] = np.ascontiguousarray(np.asarray(xp, float).T).reshape(-1); z[L["t"]] = t
    return z


def shifted_problem(N, shift, x0, xF, Ts, R, ob, xWS, timeWS, dual_ws, out, i, x0_new=None, xF_new=None):
    """the problem instance i of a batch has AFTER QuadBatch.shift_warm_start, from the host build of the shift text applied to the batch's own download `out`:
    dict(x0, xF, xWS (N+1, 12), timeWS, dual_ws) -- what the CPU checker is started from.  Row 0 of xWS is x0: the kernel's starting point holds x0 at stage 0."""
    prob = P.pack_quad_problem(x0, xF, N, Ts, R, ob, xWS, timeWS, dual_ws)
    new = emu_shift(N, shift, prob, iterate_of(N, out["xp"][i], out["timeScale"][i, 0]), out["info"][i], x0_new, xF_new)
    w = new[P.QPH_SIZE:].reshape(N + 1, 12).copy(); w[0] = new[P.QPH_X0:P.QPH_X0 + 12]
    return dict(x0=new[P.QPH_X0:P.QPH_X0 + 12].copy(), xF=new[P.QPH_XF:P.QPH_XF + 12].copy(), xWS=w, timeWS=float(new[P.QPH_TWS]), dual_ws=int(new[P.QPH_DWS]))
