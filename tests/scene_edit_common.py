"""What tests/test_scene_edit_cpu.py and tests/test_gpu_scene_edit.py share: the host build of the kernel text of obca_amd/csrc/obca_scene_edit.h
(tests/emu/scene_edit_emu.cpp, buildflags.build("scene_edit_emu")); the ragged parking batch at both limits of the header and its seeded motions; parking and quadcopter
records packed as the kernel addresses them (tests/packing.py); the numpy statement applied to a packed batch (validate.move_obstacles_parking / move_obstacles_quad).

Tolerances.  Host build against numpy: 3.1e-10 max(1, |value|), the bound tests/test_advance_cpu.py asserts for host build against numpy (the two sides differ in nothing
but the library's sine and cosine).  Device against host build: 1e-9 max(1, |value|), the bound of the sibling GPU tests.  The quadcopter only adds: bit for bit."""
import ctypes as C
import functools
import numpy as np
import packing as P
from obca_amd import buildflags, scenarios as S, validate as V

D = C.POINTER(C.c_double)
TOL_HOST, TOL_DEV = 3.1e-10, 1e-9
N_RAGGED = 6
SE_PIN, SE_QIN = 6, 4


def dp(a):
    return None if a is None else a.ctypes.data_as(D)


@functools.lru_cache(None)
def emu():
    lib = C.CDLL(buildflags.build("scene_edit_emu"))
    lib.emu_scene_edit_last_error.restype = C.c_char_p
    LL = C.c_longlong
    lib.emu_move_parking.argtypes = [C.c_int, D, LL, D, LL, C.c_int, D]
    lib.emu_move_quad.argtypes = [C.c_int, D, LL, D, C.c_int, D]
    a, b, c, d = (C.c_int(0) for _ in range(4))
    lib.emu_scene_edit_sizes(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    assert (a.value, b.value, c.value, d.value) == (SE_PIN, SE_QIN, P.OB_NOBMAX, P.OB_MMAX)
    return lib


def bits(a):
    return np.ascontiguousarray(a, float).view(np.uint64)


def same(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def worst(a, b):
    """largest |a - b| / max(1, |b|)"""
    a = np.asarray(a, float).ravel(); b = np.asarray(b, float).ravel()
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# ---------------------------------------------------------------- polygons
def polygon_hrep(V_):
    """unit outward rows of the convex polygon with counter-clockwise vertices V_ (n, 2): (A (n, 2), b (n,))"""
    V_ = np.asarray(V_, float); E = np.roll(V_, -1, axis=0) - V_
    A = np.c_[E[:, 1], -E[:, 0]]; A = A / np.hypot(A[:, 0], A[:, 1])[:, None]
    return A, (A * V_).sum(axis=1)


def regular_polygon(n, centre, radius, phase=0.0):
    t = phase + 2 * np.pi * np.arange(n) / n
    return np.asarray(centre, float) + radius * np.c_[np.cos(t), np.sin(t)]


def box(x0, x1, y0, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], float)


def move_vertices(V_, d, th, c):
    """p' = R(th)(p - c) + c + d on the vertices of a polygon, plain numpy"""
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return (np.asarray(V_, float) - c) @ R.T + c + d


# the shipped backwards scene with its three obstacles closed into 4-row boxes: the two kerbs beside the slot and the far side of the aisle
SHIPPED_BOXES = [box(-20, -1.3, -5, 5), box(1.3, 20, -5, 5), box(-20, 20, 11, 12)]


def ragged_scenes():
    """the five instances of the ragged batch as lists of polygons (vertex arrays): one triangle; 16 boxes (the obstacle limit and the 64-row limit together); an octagon
    (the row limit of one obstacle) beside a triangle; the shipped scene as 3 boxes; the shipped scene again (its motion carries the NaN)"""
    sixteen = [box(-14 + 1.7 * j, -13.2 + 1.7 * j, 11.5 + 0.1 * j, 12.3 + 0.1 * j) for j in range(16)]
    return [[regular_polygon(3, (4.0, 12.5), 1.1, 0.3)], sixteen, [regular_polygon(8, (-5.0, 13.0), 1.5, 0.1), regular_polygon(3, (6.0, 3.0), 0.9, 1.0)],
            SHIPPED_BOXES, SHIPPED_BOXES]


def ragged_batch(N=N_RAGGED):
    """dict of upload arguments (per-instance lists vOb, A, b as make_mixed_batch returns them) for the five instances; poses and warm start are the hop batch's"""
    sc = ragged_scenes(); B = len(sc)
    hop = S.make_hop_batch(N, S.HOP_STARTS[:B])
    vOb, A, b = [], [], []
    for polys in sc:
        hs = [polygon_hrep(p) for p in polys]
        vOb.append(np.array([len(h[1]) for h in hs], np.int32)); A.append(np.concatenate([h[0] for h in hs])); b.append(np.concatenate([h[1] for h in hs]))
    return dict(hop, vOb=vOb, A=A, b=b, B=B, N=N)


def ragged_motion(seed=11, nan=True):
    """seeded general motions for the ragged batch, packed per obstacle in upload order: (motion (nt,3), pivot (nt,2), inflate (nt,)); instance 4 carries one NaN"""
    nObs = [len(s) for s in ragged_scenes()]; nt = sum(nObs); rng = np.random.default_rng(seed)
    motion = np.c_[rng.uniform(-0.5, 0.5, (nt, 2)), rng.uniform(-0.7, 0.7, nt)]; pivot = rng.uniform(-3, 3, (nt, 2)); inflate = rng.uniform(-0.05, 0.15, nt)
    if nan:
        motion[sum(nObs[:4]) + 1, 1] = np.nan
    return motion, pivot, inflate


def pack_ragged(batch, s_prob=None):
    """the records of the batch as batch_upload_range packs them, (B, s_prob), pattern behind each"""
    N = batch["N"]; B = batch["B"]; n = P.OB_HDR + 3 * (N + 1); s_prob = s_prob or n
    prob = -(1e6 + np.arange(B * s_prob, dtype=float)).reshape(B, s_prob) - 0.5
    for i in range(B):
        ws = batch["xWS"][i]
        prob[i, :n] = P.pack_problem(batch["x0"][i], batch["xF"][i], N, batch["Ts"][i], batch["L"], batch["ego"], batch["XYbounds"], batch["vOb"][i], batch["A"][i], batch["b"][i],
                                     ws[:, 0], ws[:, 1], ws[:, 2], 0)
    return prob


def pack_in(prob, motion, pivot, inflate, nObMax=None):
    """(B, SE_PIN * nObMax) rows as the host layer stages them: [dx, dy, dth, cx, cy, m] per obstacle, zeros behind an instance's last obstacle"""
    nObs = prob[:, P.PH["NOB"]].astype(int); B = len(nObs); nObMax = nObMax or int(nObs.max()); nt = int(nObs.sum())
    mo = np.zeros((nt, 3)) if motion is None else np.asarray(motion, float).reshape(nt, 3)
    pv = np.zeros((nt, 2)) if pivot is None else np.asarray(pivot, float).reshape(nt, 2)
    mg = np.zeros(nt) if inflate is None else np.asarray(inflate, float).reshape(nt)
    a = np.zeros((B, nObMax, SE_PIN)); o = 0
    for i in range(B):
        k = nObs[i]; a[i, :k, :3] = mo[o:o + k]; a[i, :k, 3:5] = pv[o:o + k]; a[i, :k, 5] = mg[o:o + k]; o += k
    return a.reshape(B, -1)


def emu_move_parking(prob, motion=None, pivot=None, inflate=None, rev=0):
    """the packed records through the kernel text: (records after the move, status (B,) int)"""
    p = np.ascontiguousarray(prob, float).copy(); a = np.ascontiguousarray(pack_in(p, motion, pivot, inflate)); st = np.full(len(p), -7.0)
    rc = emu().emu_move_parking(len(p), dp(p), p.shape[1], dp(a), a.shape[1], int(rev), dp(st))
    assert rc == 0, emu().emu_scene_edit_last_error()
    return p, st.astype(int)


def rows_of(prob):
    """(A (Mt, 2), b (Mt,), vOb (nt,)) of packed records, packed as upload takes them"""
    A, b, v = [], [], []
    for p in prob:
        n, m = int(p[P.PH["NOB"]]), int(p[P.PH["M"]])
        A.append(p[P.PH["A"]:P.PH["A"] + 2 * m].reshape(m, 2)); b.append(p[P.PH["B"]:P.PH["B"] + m]); v.append(p[P.PH["VOB"]:P.PH["VOB"] + n].astype(np.int32))
    return np.concatenate(A), np.concatenate(b), np.concatenate(v)


def numpy_move_parking(prob, motion=None, pivot=None, inflate=None):
    """the numpy statement instance by instance on packed records: (records after the move, status)"""
    out = np.array(prob, float); st = np.zeros(len(out), int); o = 0
    for i, p in enumerate(out):
        n, m = int(p[P.PH["NOB"]]), int(p[P.PH["M"]]); sl = slice(o, o + n); o += n
        A2, b2, ok = V.move_obstacles_parking(p[P.PH["A"]:P.PH["A"] + 2 * m].reshape(m, 2), p[P.PH["B"]:P.PH["B"] + m], p[P.PH["VOB"]:P.PH["VOB"] + n],
                                              None if motion is None else np.asarray(motion, float).reshape(-1, 3)[sl],
                                              None if pivot is None else np.asarray(pivot, float).reshape(-1, 2)[sl], None if inflate is None else np.asarray(inflate, float).ravel()[sl])
        p[P.PH["A"]:P.PH["A"] + 2 * m] = A2.reshape(-1); p[P.PH["B"]:P.PH["B"] + m] = b2; st[i] = 0 if ok else 1
    return out, st


def obstacle_mask(prob):
    """True at the words of the records a move may write: the rows in use of PH_A and PH_B"""
    mask = np.zeros(prob.shape, bool)
    for i, p in enumerate(prob):
        m = int(p[P.PH["M"]]); mask[i, P.PH["A"]:P.PH["A"] + 2 * m] = True; mask[i, P.PH["B"]:P.PH["B"] + m] = True
    return mask


def inverse_motion(motion, inflate):
    """the motion that undoes `motion` about the same pivot: -dth, -R(-dth) d, -m"""
    mo = np.asarray(motion, float).reshape(-1, 3); th = -mo[:, 2]
    d = -np.c_[np.cos(th) * mo[:, 0] - np.sin(th) * mo[:, 1], np.sin(th) * mo[:, 0] + np.cos(th) * mo[:, 1]]
    return np.c_[d, th], None if inflate is None else -np.asarray(inflate, float)


# ---------------------------------------------------------------- quadcopter
def quad_records(B, N=4, seed=3):
    """B quadcopter records with the shipped boxes jittered, (B, s_prob)"""
    rng = np.random.default_rng(seed); out = []
    for i in range(B):
        ob = S.QUAD_OB + (0.01 * rng.normal(size=(5, 6)) if i else 0.0)
        out.append(P.pack_quad_problem(rng.normal(size=12), S.QUAD_XF, N, 0.5, S.QUAD_R, ob, rng.normal(size=(N + 1, 12)), 1.25))
    return np.array(out)


def pack_quad_in(B, motion, inflate):
    a = np.zeros((B, 5, SE_QIN))
    if motion is not None:
        a[:, :, :3] = np.broadcast_to(np.asarray(motion, float), (B, 5, 3))
    if inflate is not None:
        a[:, :, 3] = np.broadcast_to(np.asarray(inflate, float), (B, 5))
    return a.reshape(B, -1)


def emu_move_quad(prob, motion=None, inflate=None, rev=0):
    p = np.ascontiguousarray(prob, float).copy(); a = np.ascontiguousarray(pack_quad_in(len(p), motion, inflate)); st = np.full(len(p), -7.0)
    rc = emu().emu_move_quad(len(p), dp(p), p.shape[1], dp(a), int(rev), dp(st))
    assert rc == 0, emu().emu_scene_edit_last_error()
    return p, st.astype(int)


def numpy_move_quad(prob, motion=None, inflate=None):
    out = np.array(prob, float); B = len(out); st = np.zeros(B, int)
    mo = None if motion is None else np.broadcast_to(np.asarray(motion, float), (B, 5, 3)); mg = None if inflate is None else np.broadcast_to(np.asarray(inflate, float), (B, 5))
    for i, p in enumerate(out):
        ob, ok = V.move_obstacles_quad(p[P.QPH_OB:P.QPH_OB + 30].reshape(5, 6), None if mo is None else mo[i], None if mg is None else mg[i])
        p[P.QPH_OB:P.QPH_OB + 30] = ob.reshape(-1); st[i] = 0 if ok else 1
    return out, st


def box_distance(pt, ob):
    """distance of the point pt (3,) to each box of ob (5, 6) = [ub, -lb]; 0 inside"""
    pt = np.asarray(pt, float); ob = np.asarray(ob, float).reshape(5, 6)
    e = np.maximum(np.maximum(-ob[:, 3:] - pt, pt - ob[:, :3]), 0.0)
    return np.sqrt((e * e).sum(axis=1))
