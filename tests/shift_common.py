"""TEST INFRASTRUCTURE ONLY: the parking receding-horizon shift (obca_amd/csrc/obca_shift.h) built for the host (tests/emu/shift_emu.cpp), a numpy statement of the same rules
written from the header's text, and the packing between a Batch download and the records the shift text reads and writes (tests/packing.py; lambda in the solver's unit-row
scaling).  Shared by tests/test_shift_cpu.py and tests/test_gpu_restart.py."""
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
    if _LIB is None:
        _LIB = C.CDLL(buildflags.build("shift_emu"))
    return _LIB


def emu_layout(N, nOb, M):
    """make_layout of the kernel text as the dict of packing.layout, and OB_HDR"""
    out = np.zeros(26, np.int32); hdr = C.c_int(0)
    load().emu_shift_layout(C.c_int(N), C.c_int(nOb), C.c_int(M), out.ctypes.data_as(C.POINTER(C.c_int)), C.byref(hdr))
    return dict(zip(P.LAYOUT_FIELDS, out.tolist())), hdr.value


def emu_shift(N, shift, prob, z, z0, tmp, x0_new=None, rev=0):
    """B instances through the kernel text, addressed as the kernel addresses them: prob (B, s_prob), z / z0 / tmp (B, s_z).  Returns (prob, z0, tmp) after the call; no
    argument is modified."""
    prob = np.array(prob, float, ndmin=2); z = np.ascontiguousarray(np.array(z, float, ndmin=2)); z0 = np.array(z0, float, ndmin=2); tmp = np.array(tmp, float, ndmin=2)
    B = prob.shape[0]; assert z.shape == z0.shape == tmp.shape and z.shape[0] == B
    x0 = None if x0_new is None else np.ascontiguousarray(np.reshape(x0_new, (B, 4)), float)
    rc = load().emu_shift_batch(C.c_int(B), C.c_int(N), C.c_int(shift), dp(prob), C.c_longlong(prob.shape[1]), dp(z), dp(z0), dp(tmp), C.c_longlong(z.shape[1]), dp(x0), C.c_int(rev))
    assert rc == 0, rc
    return prob, z0, tmp


# ---------------------------------------------------------------- the statement
def numpy_shift(N, shift, xp, up, lp, npp, rx, ry, ryaw, x0_new=None):
    """The rules of obca_batch_shift_warm_start (include/obca_hip.h; obca_amd/csrc/obca_shift.h) on the caller-level arrays of ONE instance: xp (4, N+1), up (2, N), lp (M, N+1),
    npp (4 nOb, N+1) as a download returns them, the reference (N+1 each).  Returns what the next solve starts from, in the oracle's argument shapes:
    dict(x0 (4), rx, ry, ryaw (N+1), xWS (N+1, 4), uWS (N, 2), lWS (N+1, M), nWS (N+1, 4 nOb)); t = 1 and zero slacks are what every start has."""
    xp, up, lp, npp = (np.asarray(a, float) for a in (xp, up, lp, npp))
    ks = np.minimum(np.arange(N + 1) + shift, N)              # states, multipliers, reference: the tail repeats the terminal stage
    ku = np.minimum(np.arange(N) + shift, N - 1)              # inputs: the tail repeats the last interval ...
    xWS = xp[:, ks].T.copy(); uWS = up[:, ku].T.copy()
    uWS[np.arange(N) + shift > N - 1, 1] = 0.0                # ... with acceleration 0
    x0 = xp[:, min(shift, N)].copy() if x0_new is None else np.array(x0_new, float).reshape(4)
    xWS[0] = x0                                               # stage 0 of the warm start holds X0
    return dict(x0=x0, rx=np.asarray(rx, float)[ks].copy(), ry=np.asarray(ry, float)[ks].copy(), ryaw=np.asarray(ryaw, float)[ks].copy(),
                xWS=xWS, uWS=uWS, lWS=lp[:, ks].T.copy(), nWS=npp[:, ks].T.copy())


def shifted_problem(N, shift, out, i, rx, ry, ryaw, x0_new=None):
    """What the CPU oracle must be started from after Batch.shift_warm_start(shift, x0_new) of the batch whose download is `out`, for instance i: the statement applied to the
    device's own download.  rx, ry, ryaw: the reference instance i holds BEFORE the shift (the uploaded one, advanced by every earlier shift).  x0_new: the 4 values of
    instance i, or None."""
    return numpy_shift(N, shift, out["xp"][i], out["up"][i], out["lp"][i], out["np"][i], rx, ry, ryaw, x0_new)


# ---------------------------------------------------------------- packing
def iterate_of(N, vOb, A, xp, up, lp, npp, zlen=None):
    """a solver-layout iterate (row of zlen doubles) that holds what the shift may read of a solution -- x, u, lambda (for unit rows), mu -- and NaN everywhere else: t, sl,
    slacks, every multiplier, the words behind the instance's own layout"""
    v = np.ravel(vOb).astype(int); nOb, M = len(v), int(v.sum()); L = P.layout(N, nOb, M)
    full = P.pack_start(N, nOb, M, np.asarray(xp, float).T, np.asarray(up, float).T, np.asarray(lp, float).T, np.asarray(npp, float).T, zlen=zlen, A=A)
    z = np.full(len(full), np.nan)
    for a, b in ((L["x"], L["t"]), (L["lam"], L["sl"])):
        z[a:b] = full[a:b]
    return z


def start_of(N, vOb, A, st, zlen=None, fill=0.0):
    """the start iterate a statement result `st` (numpy_shift) describes, as the shift must write it: x, u, t = 1, lambda for unit rows, mu, zero sl / so / ss; `fill` behind
    the primal part (what the shift leaves alone)"""
    v = np.ravel(vOb).astype(int); nOb, M = len(v), int(v.sum()); L = P.layout(N, nOb, M)
    z = P.pack_start(N, nOb, M, st["xWS"], st["uWS"], st["lWS"], st["nWS"], zlen=zlen, A=A)
    z[L["nprimal"]:] = fill
    return z


def unpack_start(N, vOb, A, z0, prob):
    """the oracle's arguments from a start iterate and problem record the shift wrote (the inverse of start_of / pack_problem for the words the shift owns)"""
    v = np.ravel(vOb).astype(int); nOb, M = len(v), int(v.sum()); N1 = N + 1
    xp, up, t, lp, npp, sl = P.unpack_solution(z0, N, nOb, M, A=A)
    return dict(x0=prob[P.PH["X0"]:P.PH["X0"] + 4].copy(), rx=prob[P.OB_HDR:P.OB_HDR + N1].copy(), ry=prob[P.OB_HDR + N1:P.OB_HDR + 2 * N1].copy(),
                ryaw=prob[P.OB_HDR + 2 * N1:P.OB_HDR + 3 * N1].copy(), xWS=xp.T.copy(), uWS=up.T.copy(), lWS=lp.T.copy(), nWS=npp.T.copy(), t=t, sl=sl)
