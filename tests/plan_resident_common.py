"""What tests/test_plan_resident_cpu.py and tests/test_gpu_plan_resident.py share: the host build of the planner's resident route (tests/emu/plan_resident_emu.cpp), the
16 scenes of the issue packed into problem records as an upload leaves them (tests/packing.py), and views of the packed block per instance."""
import ctypes as C
import functools
import numpy as np
import hybrid_common as H
import packing as PK
import scenes_common as SC
from obca_amd import buildflags, scenarios as S

NS = 16          # the first 16 of scenes_common.scenes()
N = 30           # horizon of the batches here
TS = 0.6
_lib = None
NAMES = ("inst", "A", "b", "rn", "nrm", "vert", "rec", "v", "off", "voff")


def emu():
    global _lib
    if _lib is None:
        _lib = C.CDLL(buildflags.build("plan_resident_emu"))
        _lib.emu_plr_last_error.restype = C.c_char_p
        dp, ip, ll = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_longlong
        _lib.emu_plr_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(ll), ip]
        _lib.emu_plr_pack.argtypes = [C.c_int, dp, ll, C.c_int, C.c_int, dp, C.c_int, C.c_void_p]
        _lib.emu_plr_host_fields.argtypes = [C.c_int, dp, dp, ip, ip, dp, dp, dp, C.c_double, dp, ip, ip, ip, ip, dp, dp, dp, dp, dp, dp, ip]
        head = [C.c_int, C.c_int, dp, ll, dp, C.c_int, C.c_int, C.c_int, dp, C.c_double, dp, dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double,
                C.c_int, C.c_int, C.c_int, C.c_int]
        _lib.emu_plr_plan.argtypes = head + [dp, ip, ip, ip, ip, ip, dp]
        _lib.emu_plr_plan_given.argtypes = head + [C.c_void_p, dp, ip, ip, ip, ip, ip]
    return _lib


def unit(field):
    """a field on unit rows, as the record holds them (packing.pack_problem: a / |a|, b / |a|)"""
    v, A, b = field
    n = PK.row_lengths(A)
    return np.ascontiguousarray(v, np.int32), np.ascontiguousarray(A / n[:, None]), np.ascontiguousarray(b / n)


def records(x0, xF, fields, seed=11):
    """the batch as an upload leaves it on the device: prob (B, s_prob), z0 (B, zlen) -- a start iterate of random numbers, so that `unchanged` and `rewritten` both show --,
    nObMax, MMax"""
    B = len(fields); rng = np.random.default_rng(seed)
    nObMax = max(len(f[0]) for f in fields); MMax = max(int(np.sum(f[0])) for f in fields)
    zlen = PK.layout(N, nObMax, MMax)["len"]
    zero = np.zeros(N + 1)
    prob = np.stack([PK.pack_problem(x0[i], xF[i], N, TS, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, f[0], f[1], f[2], zero, zero, zero, 0) for i, f in enumerate(fields)])
    z0 = rng.uniform(-1.0, 1.0, (B, zlen))
    return np.ascontiguousarray(prob), np.ascontiguousarray(z0), nObMax, MMax


@functools.lru_cache(None)
def scenes16():
    x0, xF, kw, fields = SC.scenes()
    return x0[:NS], xF[:NS], kw, list(fields[:NS])


def layout(B, nObMax, MMax):
    out = (C.c_longlong * 11)(); nv = C.c_int(0)
    emu().emu_plr_layout(B, nObMax, MMax, out, C.byref(nv))
    return dict(zip(NAMES + ("bytes",), [int(x) for x in out])), nv.value


def views(block, B, nObMax, MMax):
    """the arrays of a packed block (bytes) by name"""
    lay, nv = layout(B, nObMax, MMax)
    cnt = dict(inst=10 * B, A=2 * B * MMax, b=B * MMax, rn=B * MMax, nrm=B * MMax, vert=2 * B * nObMax * nv, rec=4 * B, v=B * nObMax, off=B * (nObMax + 1), voff=B * (nObMax + 1))
    return {k: np.frombuffer(block, np.int32 if k in ("rec", "v", "off", "voff") else np.float64, cnt[k], lay[k]) for k in NAMES}


def pack_block(prob, nObMax, MMax, order=0):
    """plan_pack_instance over the records: the block's bytes"""
    B = len(prob); lay, _ = layout(B, nObMax, MMax)
    block = np.zeros(lay["bytes"], np.uint8); xy = np.ascontiguousarray(S.XYBOUNDS, float)
    rc = emu().emu_plr_pack(B, H._p(prob), prob.shape[1], nObMax, MMax, H._p(xy), order, block.ctypes.data)
    assert rc == 0, emu().emu_plr_last_error()
    return block


def field_of(arr, i):
    """instance i of flat `Fields` arrays, as hy::field_of reads them: dict(v, off, voff, A, b, rn, nrm, vert) cut to the instance's counts"""
    ob, row, vx, nOb = (int(x) for x in arr["rec"][4 * i:4 * i + 4])
    off = arr["off"][ob + i:ob + i + nOb + 1]; voff = arr["voff"][ob + i:ob + i + nOb + 1]
    M, nvx = int(off[-1]), int(voff[-1])
    return dict(v=arr["v"][ob:ob + nOb], off=off, voff=voff, A=arr["A"][2 * row:2 * (row + M)], b=arr["b"][row:row + M], rn=arr["rn"][row:row + M],
                nrm=arr["nrm"][row:row + M], vert=arr["vert"][2 * vx:2 * (vx + nvx)])


def host_fields(x0, xF, fields):
    """hy::make_scenes of the same scenes: flat `Fields` arrays and make_params' instance records"""
    B = len(fields); nOb, v, A, b = SC.pack(fields)
    s = np.ascontiguousarray(np.asarray(x0, float)[:, :3]); g = np.ascontiguousarray(np.asarray(xF, float)[:, :3])
    rows, obs = len(b), len(v)
    out = dict(rec=np.zeros(4 * B, np.int32), v=np.zeros(obs, np.int32), off=np.zeros(obs + B, np.int32), voff=np.zeros(obs + B, np.int32), A=np.zeros(2 * rows), b=np.zeros(rows),
               rn=np.zeros(rows), nrm=np.zeros(rows), vert=np.zeros(2 * 17 * obs), inst=np.zeros(10 * B))
    sizes = np.zeros(3, np.int32); e = np.ascontiguousarray(S.EGO, float); xy = np.ascontiguousarray(S.XYBOUNDS, float)
    P = H._p
    rc = emu().emu_plr_host_fields(B, P(s), P(g), P(nOb, C.c_int), P(v, C.c_int), P(A), P(b), P(e), S.L_WHEELBASE, P(xy), P(out["rec"], C.c_int), P(out["v"], C.c_int),
                                   P(out["off"], C.c_int), P(out["voff"], C.c_int), P(out["A"]), P(out["b"]), P(out["rn"]), P(out["nrm"]), P(out["vert"]), P(out["inst"]), P(sizes, C.c_int))
    assert rc == 0, emu().emu_plr_last_error()
    return out


def plan(prob, z0, nObMax, MMax, kw=None, bw=0.0, cap=H.CAP, use_xF=True, v_nom=0.5, a_max=0.0, slots=3, nodes=H.NODES, chunks=0, order=0, inst=None, block=None):
    """the whole route on the host build; prob and z0 are COPIED: dict(rc, paths, dirs, counts, expansions, rounds, status, prob, z0, inst).  block: a packed block (bytes)
    that stands in for the host build's own packing; inst: instance records laid over the host build's own block"""
    B = len(prob); prob = prob.copy(); z0 = z0.copy()
    o = H.opts_array(kw or {}); e = np.ascontiguousarray(S.EGO, float); xy = np.ascontiguousarray(S.XYBOUNDS, float)
    out = dict(paths=np.full((B, cap, 3), 7.0), dirs=np.full((B, cap), 7, np.int32), counts=np.full(B, 99, np.int32), expansions=np.full(B, 55, np.int32),
               rounds=np.full(B, 55, np.int32), status=np.full(B, 99, np.int32), prob=prob, z0=z0, inst=np.zeros((B, 10)))
    P = H._p
    head = (B, N, P(prob), prob.shape[1], P(z0), z0.shape[1], nObMax, MMax, P(e), S.L_WHEELBASE, P(xy), P(o), len(o), float(bw), cap, int(use_xF), float(v_nom), float(a_max),
            slots, nodes, chunks, order)
    tail = (P(out["paths"]), P(out["dirs"], C.c_int), P(out["counts"], C.c_int), P(out["expansions"], C.c_int), P(out["rounds"], C.c_int), P(out["status"], C.c_int))
    if inst is None and block is None:
        out["rc"] = emu().emu_plr_plan(*head, *tail, P(out["inst"]))
    else:
        if block is None:
            block = pack_block(prob, nObMax, MMax)
            views(block, B, nObMax, MMax)["inst"][:] = np.ascontiguousarray(inst, float).ravel()
        block = np.ascontiguousarray(block, np.uint8); assert len(block) == layout(B, nObMax, MMax)[0]["bytes"]
        out["inst"] = views(block, B, nObMax, MMax)["inst"].reshape(B, 10).copy()
        out["rc"] = emu().emu_plr_plan_given(*head, block.ctypes.data, *tail)
    out["err"] = emu().emu_plr_last_error().decode() if out["rc"] else ""
    return out


@functools.lru_cache(None)
def plan16(analytic=None, order=0):
    """the 16 scenes through the whole route on the host build"""
    x0, xF, kw, fields = scenes16()
    prob, z0, nObMax, MMax = records(x0, xF, fields)
    return plan(prob, z0, nObMax, MMax, kw if analytic is None else dict(kw, analytic=analytic), order=order)


@functools.lru_cache(None)
def host16(analytic=None):
    """the same scenes through the host-pointer route's host build (scenes_common.run_scenes) on the same unit rows"""
    x0, xF, kw, fields = scenes16()
    return SC.run_scenes(x0, xF, [unit(f) for f in fields], kw if analytic is None else dict(kw, analytic=analytic))


def path_ws_record(prob_i, z0_i, path, dirs, count, cap=H.CAP, use_xF=True, v_nom=0.5, a_max=0.0):
    """emu_path_ws_record (tests/emu/path_ws_emu.cpp) on copies of one instance's record and start: (status, prob, z0)"""
    import path_ws_common as W
    p = prob_i.copy(); z = z0_i.copy()
    path = np.ascontiguousarray(path, float); dirs = np.ascontiguousarray(dirs, np.int32)
    st = W.emu().emu_path_ws_record(N, int(count), cap, H._p(path), H._p(dirs, C.c_int), int(use_xF), C.c_double(v_nom), C.c_double(a_max), H._p(p), H._p(z), len(z))
    return st, p, z
