"""
Generates tests/golden/abi_calls.json: what the Python layer (obca_amd.api, .planner's device calls, .diag) hands to the C ABI, call by call and argument by argument.

No device and no library are involved.  A STAND-IN takes the place of the loaded libraries: an object whose obca_* attributes are Python callables that record their
arguments, write a handle through `**` out-parameters, fill every output array with a fixed pattern and return 0.  `drive()` then runs every Python entry point once at the
smallest shapes that reach each marshalling branch (B = 2, N = 3: shared and ragged obstacle sets, duals given and None, both formulations, opts given and None, `buffers=`
reused, fixTime 0 and 1, x0_new / xF_new given and None, scalar and per-instance Ts / timeScale, single- and multi-device contexts, the single-instance drop-ins,
leave_pattern, the device planner with its long-path second call).  All inputs are integers and exact binary fractions, so the bytes are the same on every machine.

Recorded per call: the function's name and per argument
    a scalar                       its value
    NULL                           null
    a handle                       {"handle": value}
    byref(x)                       {"ref": type of x} (+ SHA-256 of the bytes of an option record)
    a ctypes array                 {"carray": element type, "n": length} (+ the values of an int array)
    an array                       {"dtype", "n", "sha256" of its bytes}; the SHA-256 only for `const` parameters of the header: output buffers may be np.empty, their bytes
                                   before the call are nobody's contract
and per Python call what it RETURNED (shape, dtype, bytes, owner or view of every array), which pins the unpacking of the outputs the stand-in wrote.
An array reaches the recorder either as itself or as the pointer numpy's `data_as` made of it (which keeps the array as `_arr`): one recorder reads both styles.
tests/test_marshalling_cpu.py compares the code as it stands with this record.

Run from the repo root (a second):  python tests/golden/make_abi_calls.py
"""
import ctypes as C
import hashlib
import json
import numbers
import os
import re
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "abi_calls.json")
HEADERS = ("obca_hip.h", "obca_plan3d.h", "obca_diag.h")      # the libraries that need a device (libobca_plan.so runs for real on the CPU: tests/test_planner_cpu.py)
B, N = 2, 3


def declared(headers=HEADERS):
    """name -> the parameter texts of every prototype of the headers (this file's own reading: comments stripped, split at commas)"""
    out = {}
    for h in headers:
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        for m in re.finditer(r"\b(?:int|const char \*)\s*(obca_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
            out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")] if m.group(2).strip() not in ("", "void") else []
    return out


def _sha(raw):
    return hashlib.sha256(raw).hexdigest()


def _array(a):
    return a if isinstance(a, np.ndarray) else getattr(a, "_arr", None)


def encode(a, const):
    if a is None:
        return None
    arr = _array(a)
    if arr is not None:
        return dict(dtype=str(arr.dtype), n=int(arr.size), sha256=_sha(arr.tobytes()) if const else None)
    if isinstance(a, C.c_void_p):
        return dict(handle=a.value)
    if isinstance(a, C._SimpleCData):
        return a.value
    if isinstance(a, C.Array):
        d = dict(carray=a._type_.__name__, n=len(a))
        if a._type_ is C.c_int:
            d["values"] = list(a)
        return d
    if type(a).__name__ == "CArgObject":
        o = a._obj
        return dict(ref=type(o).__name__, **(dict(sha256=_sha(bytes(o))) if isinstance(o, C.Structure) else {}))
    if isinstance(a, numbers.Integral):
        return int(a)
    if isinstance(a, numbers.Real):
        return float(a)
    raise TypeError("the recorder does not know %r" % (a,))


class StandIn:
    """the loaded libraries' stand-in; `calls` = the record, `live` = (name, args) as they arrived"""

    def __init__(self):
        self.sig = declared()
        self.calls, self.live = [], []
        self.handle = 0x1000
        self.long_path_once = True
        self.fail = None      # name of the call that answers -1 next

    def __getattr__(self, name):
        if name not in self.__dict__.get("sig", {}):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        params = self.sig[name]
        const = [p.startswith("const ") for p in params] + [False] * len(args)      # (a surplus argument is recorded, and the count then differs from the header's)
        self.calls.append([name] + [encode(a, c) for a, c in zip(args, const)])
        self.live.append((name, args))
        for k, (a, c) in enumerate(zip(args, const)):      # outputs: a pattern that depends on the position of the argument and of the element (below 3: info[0] is a status code)
            if c or a is None:
                continue
            arr = _array(a)
            if arr is not None:
                arr.reshape(-1)[:] = (0.5 * np.arange(arr.size) + k) % 3 if arr.dtype == np.float64 else 1 + np.arange(arr.size) % 2
            elif type(a).__name__ == "CArgObject":
                o = a._obj
                if isinstance(o, C.c_void_p):
                    self.handle += 0x10; o.value = self.handle
                elif isinstance(o, (C.c_int, C.c_longlong)):
                    o.value = 3 + k
                elif isinstance(o, (C.c_float, C.c_double)):
                    o.value = 1.5 + k
            elif isinstance(a, C.Array) and a._type_ is C.c_char:
                a.value = b"stand-in"
        if name in ("obca_last_error", "obca_plan3d_last_error"):
            return b"stand-in says no"
        if name == self.fail:
            self.fail = None
            return -1
        if name in ("obca_device_count", "obca_visible_device_count"):
            return 2
        if name == "obca_plan3d_paths_batch":      # counts: the first call answers "longer than cap" for its first instance, once
            cnt = _array(args[11]); cnt[:] = 3
            if self.long_path_once:
                cnt[0] = -1; self.long_path_once = False
        if name == "obca_plan3d_warm_start_batch":
            _array(args[11])[:] = [2, 0][:len(_array(args[11]))]
        return 0


def digest(v):
    """what a Python call returned, in a form JSON holds"""
    if isinstance(v, np.ndarray):
        return dict(shape=list(v.shape), dtype=str(v.dtype), sha256=_sha(np.ascontiguousarray(v).tobytes()), owndata=bool(v.flags.owndata))
    if isinstance(v, dict):
        return {k: digest(x) for k, x in v.items() if k != "time"}      # (wall-clock)
    if isinstance(v, (list, tuple)):
        return [digest(x) for x in v]
    if isinstance(v, C.Structure):
        return dict(struct=type(v).__name__, sha256=_sha(bytes(v)))
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, numbers.Integral):
        return int(v)
    if isinstance(v, numbers.Real):
        return "float"      # (times)
    if v is None or isinstance(v, str):
        return v
    return type(v).__name__


def seq(shape, start, step=0.125):
    """start, start + step, ...: exact binary fractions"""
    return (start + step * np.arange(int(np.prod(shape)), dtype=float)).reshape(shape)


def drive(lib, opened):
    """every Python entry point once; returns [(label, digest of what it returned)].  `opened` collects what holds a handle of the stand-in."""
    import obca_amd as OA
    from obca_amd import api, diag, planner as PL
    ret = []

    def run(label, f, *a, **kw):
        r = f(*a, **kw)
        if hasattr(r, "close"):
            opened.append(r)
        ret.append([label, digest(r)])
        return r

    def refused(label, fails, f, *a, **kw):      # the error path: the named call answers -1, the wrapper raises with the library's message
        lib.fail = fails
        try:
            f(*a, **kw)
            ret.append([label, None])
        except Exception as e:      # noqa: BLE001 -- type and text are what is recorded
            ret.append([label, [type(e).__name__, str(e)]])
    N1 = N + 1
    ego, XYb, L = [3.5, 1.0, 1.0, 1.0], [-15.0, 15.0, 1.0, 10.0], 2.75
    x0, xF = seq((B, 4), -2.0), seq((B, 4), 1.0)
    rx, ry, ryaw = seq((B, N1), 0.25), seq((B, N1), 3.0), seq((B, N1), -0.5)
    xWS, uWS = seq((B, N1 + 2, 4), 0.5), seq((B, N + 1, 2), -1.0)      # longer than the horizon: cut by the wrapper
    shared = dict(vOb=[3, 4], A=seq((7, 2), -1.0), b=seq((7,), 2.0))
    ragged = dict(vOb=[[3, 4], [4]], A=[seq((7, 2), -1.0), seq((4, 2), 0.5)], b=[seq((7,), 2.0), seq((4,), 5.0)])
    lWS, nWS = [seq((N1, 7), 0.125), seq((N1, 4), 1.125)], [seq((N1, 8), 0.25), seq((N1, 4), 2.25)]
    Tsv = np.array([0.5, 0.75])

    # ---- contexts
    c0 = run("Context(0)", OA.Context, 0); run("device_count", c0.device_count); run("name", c0.name); c0.close()
    c2 = run("Context(devices=[0,1])", OA.Context, devices=[0, 1]); run("devices", lambda: c2.devices); c2.close()
    ca = run("Context(devices='all')", OA.Context, devices="all"); run("devices", lambda: ca.devices); ca.close()
    refused("Context refused", "obca_create", OA.Context, 3); refused("Context multi refused", "obca_create_multi", OA.Context, devices=[2])
    run("visible_device_count", api._load().obca_visible_device_count)      # (bench.py calls it on the raw library)
    for f in ("default_opts", "ipopt_opts", "warm_restart_opts", "quadcopter_default_opts", "quadcopter_ipopt_opts", "quad_warm_restart_opts"):
        run(f, getattr(OA, f))
    run("quad_warm_restart_opts(True)", OA.quad_warm_restart_opts, True)
    opts = api.Opts(); opts.tol = 0.5; opts.max_iter = 7; opts.restoration = 1

    # ---- parking, host pointers
    def park(ob, **kw):
        return OA.parking_signed_dist_batch(x0, xF, N, kw.pop("Ts", 0.5), L, ego, XYb, ob["vOb"], ob["A"], ob["b"], rx, ry, ryaw, kw.pop("fixTime", 0), xWS, uWS, **kw)
    run("parking shared", park, shared)
    keep = {}
    run("parking ragged dist duals opts buffers", park, ragged, Ts=Tsv, fixTime=1, lWS=lWS, nWS=nWS, opts=opts, dist=True, buffers=keep)
    ids = {k: id(v) for k, v in keep.items()}
    run("parking ragged buffers again", park, ragged, Ts=Tsv, lWS=np.concatenate([np.ravel(x) for x in lWS]), nWS=np.concatenate([np.ravel(x) for x in nWS]), buffers=keep, device=[0, 1])
    run("buffers kept", lambda: ids == {k: id(v) for k, v in keep.items()})
    run("parking shared dist all", park, shared, dist=True, device="all")
    cx = OA.Context(1); opened.append(cx)
    run("parking context", park, shared, device=cx, opts=opts)
    one = (x0[0], xF[0], N, 0.5, L, ego, XYb, 2, shared["vOb"], shared["A"], shared["b"], rx[0], ry[0], ryaw[0])
    run("ParkingSignedDist", OA.ParkingSignedDist, *one, 0, xWS[0], uWS[0])
    run("ParkingDist", OA.ParkingDist, *one, 1, xWS[0], uWS[0], opts=opts, device=cx)
    x, u = seq((B, 4, N1), 0.0), seq((B, 2, N), 1.0)
    lr, nr, sr = [seq((7, N1), 0.5), seq((4, N1), 1.5)], [seq((8, N1), 0.25), seq((4, N1), 1.25)], [seq((2, N1), 0.0), seq((1, N1), 1.0)]
    lsh, nsh, ssh = seq((B, 7, N1), 0.5), seq((B, 8, N1), 0.25), seq((B, 2, N1), 0.0)

    def cons(ob, ts, l, n, **kw):
        return OA.parking_constraints_batch(x0, xF, N, kw.pop("Ts", 0.5), L, ego, XYb, ob["vOb"], ob["A"], ob["b"], x, u, ts, l, n, **kw)
    run("constraints shared scalar ts", cons, shared, 1.25, lsh, nsh)
    run("constraints ragged (B,) ts sl dist", cons, ragged, np.array([1.0, 1.5]), lr, nr, sl=sr, fixTime=1, dist=True, tol=0.25, Ts=Tsv, device=cx)
    run("constraints shared (B,N+1) ts sl", cons, shared, seq((B, N1), 1.0), lsh, nsh, sl=ssh, device=[0, 1])
    run("ParkingConstraints", OA.ParkingConstraints, *one[:11], x[0], u[0], lsh[0], nsh[0], 1.25, 0, 1)
    run("ParkingConstraints stages dist", OA.ParkingConstraints, *one[:11], x[0], u[0], lsh[0], nsh[0], seq((N1,), 1.0), 1, 0, device=cx)
    run("dualmult shared", OA.dualmult_ws_batch, N, shared["vOb"], shared["A"], shared["b"], rx, ry, ryaw, ego)
    run("dualmult ragged", OA.dualmult_ws_batch, N, ragged["vOb"], ragged["A"], ragged["b"], rx, ry, ryaw, ego, device=cx)
    run("DualMultWS", OA.DualMultWS, N, 2, shared["vOb"], shared["A"], shared["b"], rx[0], ry[0], ryaw[0], ego)

    # ---- parking, resident batch
    bt = run("Batch", OA.Batch, cx, B, N)
    up = (x0, xF, 0.5, L, ego, XYb, shared["vOb"], shared["A"], shared["b"], rx, ry, ryaw, 0, xWS, uWS)
    run("upload shared", bt.upload, *up)
    run("solve", bt.solve); run("solve opts nosync", bt.solve, opts=opts, sync=False); run("sync", bt.sync)
    refused("sync refused", "obca_batch_sync", bt.sync); refused("parking refused", "obca_parking_dist_batch", park, shared, dist=True, device=cx)
    run("kernel_ms", bt.kernel_ms); run("last_schedule", bt.last_schedule); run("download", bt.download)
    run("validate", bt.validate); run("validate tol", bt.validate, 0.25); run("validate_ms", bt.validate_ms); run("scratch_bytes", bt.scratch_bytes)
    run("shift", bt.shift_warm_start, 1); run("shift x0", bt.shift_warm_start, 2, x0_new=xF)
    run("phase_cycles", bt.phase_cycles)
    run("upload ragged duals dist", bt.upload, x0, xF, Tsv, L, ego, XYb, ragged["vOb"], ragged["A"], ragged["b"], rx, ry, ryaw, 1, xWS, uWS, lWS=lWS, nWS=nWS, dist=True)
    run("download ragged", bt.download)
    bt.close()

    # ---- quadcopter
    R = 0.25
    q0, qF = seq((B, 12), 0.0), seq((B, 12), 4.0)
    ob1, obB = seq((5, 6), 1.0), seq((B, 5, 6), 2.0)
    qWS = seq((B, N1 + 1, 12), 0.5)
    run("quad", OA.quadcopter_signed_dist_batch, q0, qF, N, 0.5, R, ob1, qWS, 1.0)
    run("quad dist opts", OA.quadcopter_signed_dist_batch, q0, qF, N, Tsv, R, obB, qWS, np.array([1.0, 1.25]), dual_ws=False, opts=opts, device=cx, dist=True)
    qone = (q0[0], qF[0], N, 0.5, R, *ob1, qWS[0], None, 1.0)
    run("QuadcopterSignedDist", OA.QuadcopterSignedDist, *qone)
    run("QuadcopterDist", OA.QuadcopterDist, *qone, opts=opts, device=cx, dual_ws=False)
    qx, qu, lam = seq((B, 12, N1), 0.0), seq((B, 4, N), 1.0), seq((B, 30, N1), 0.25)
    run("constr scalar ts", OA.quadcopter_constr_satisfaction_batch, qx, qu, 1.25, q0, qF, 0.5, lam, ob1, R)
    run("constr (B,) ts shared x0", OA.quadcopter_constr_satisfaction_batch, qx, qu, np.array([1.0, 1.5]), q0[0], qF[0], Tsv, lam, obB, R, tol=0.25, device=cx)
    run("constr (B,N+1) ts", OA.quadcopter_constr_satisfaction_batch, qx, qu, seq((B, N1), 1.0), q0, qF, 0.5, lam, ob1, R)
    run("constrSatisfaction", OA.constrSatisfaction, qx[0], qu[0], 1.25, q0[0], qF[0], 0.5, lam[0], *ob1, R)
    qb = run("QuadBatch", OA.QuadBatch, cx, B, N)
    run("qupload", qb.upload, q0, qF, 0.5, R, ob1, qWS, 1.0)
    run("qsolve", qb.solve); run("qsolve opts", qb.solve, opts=opts, sync=False); run("qsync", qb.sync)
    run("qkernel_ms", qb.kernel_ms); run("qdownload", qb.download); run("qvalidate", qb.validate); run("qvalidate tol", qb.validate, 0.5)
    run("qvalidate_ms", qb.validate_ms); run("qscratch", qb.scratch_bytes); run("qphase", qb.phase_cycles)
    run("qshift", qb.shift_warm_start, 1); run("qshift x0", qb.shift_warm_start, 2, x0_new=qF); run("qshift x0 xF", qb.shift_warm_start, 0, q0, qF); run("qshift xF", qb.shift_warm_start, 3, xF_new=q0)
    run("qupload per instance dist", qb.upload, q0, qF, Tsv, R, obB, qWS, np.array([1.0, 1.25]), dual_ws=False, dist=True)
    qb.close()

    # ---- diagnostics and the device planner
    c2 = OA.Context(devices=[0, 1]); opened.append(c2)
    run("leave_pattern ctx", diag.leave_pattern, c2); run("leave_pattern 1", diag.leave_pattern, 1, mask=5, value=0.5); run("leave_pattern list", diag.leave_pattern, [0, 1])
    c2.close()
    s, g = seq((B, 3), 1.0), seq((B, 3), 4.0)
    run("plan3d_paths", PL.plan3d_paths, s, g, cap=4); lib.long_path_once = True
    run("astar3d_many", PL.astar3d_many, q0, qF, boxes=obB[:, :2], clear=0.5, room=(8.0, 8.0, 4.0), res=0.5, device=1)
    refused("plan3d refused", "obca_plan3d_paths_batch", PL.plan3d_paths, s, g); refused("plan3d context refused", "obca_plan3d_create", PL.plan3d_context, 2)
    refused("warm starts refused", "obca_plan3d_warm_start_batch", PL.quad_warm_start_many, q0, qF, N)
    run("quad_warm_start_many", PL.quad_warm_start_many, q0, qF, N)
    run("quad_warm_start_many ms", PL.quad_warm_start_many, q0[0], qF[0], N, boxes=ob1[:1], with_ms=True, device=1)

    cx.close()
    for c in api._default_ctx.values():      # the cached contexts of the `device=` arguments: closed here, not when the collector gets to them
        c.close()
    return ret


def record():
    """(stand-in after the drive, what the Python calls returned); the package's libraries are put back afterwards"""
    from obca_amd import api, diag, planner as PL
    lib = StandIn()
    saved = (api._lib, api._default_ctx, diag._lib, PL._lib3d, PL._ctx3d)
    api._lib, api._default_ctx, diag._lib, PL._lib3d, PL._ctx3d = lib, {}, lib, lib, {}
    opened = []
    try:
        ret = drive(lib, opened)
    finally:
        for o in opened + list(api._default_ctx.values()):      # (after a failure: nothing that holds a stand-in handle may reach the real library's destroy)
            o.close()
        api._lib, api._default_ctx, diag._lib, PL._lib3d, PL._ctx3d = saved
    return lib, ret


def main():
    lib, ret = record()
    with open(OUT, "w") as f:
        json.dump(dict(B=B, N=N, calls=lib.calls, returns=ret), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, len(lib.calls), "calls of", len({c[0] for c in lib.calls}), "entry points,", len(ret), "Python calls")


if __name__ == "__main__":
    main()
