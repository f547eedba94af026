"""What tests/test_certify_cpu.py and tests/test_gpu_certify.py share: the host build of the kernel text of obca_amd/csrc/obca_certify.h (tests/emu/certify_emu.cpp,
buildflags.build("certify_emu")); the trajectories both suites run -- the solved ones of tests/golden/clearance_cases.npz and tests/golden/rollout_cases.npz, synthetic
parking trajectories at N = 1, 2, 3 and the quadcopter segment that slips past a box between two samples --; the numpy statement fed with the host build's own distances;
the dense sampling the certificate is held against; the comparison rules.

Tolerances.  Host build against the statement with the host build's distances: ticks, counts and indices equal; lb and seen within 1e-9 max(1, |value|) -- the statement's
poses come from numpy's sin / cos / tan, the host build's from libm, and the distance is an iteration the project holds to 1e-9 (tests/clearance_common.py); the
quadcopter has no iteration and no transcendental: bits.  lb against a dense sampling: lb <= dense + 1e-7, the issue's bound (CL_TOUCH: a distance below 1e-7 is reported
as 0).  Device against host build: quadcopter bits; parking indices, ticks and counts equal and values within 1e-9, the bound tests/test_gpu_clearance.py asserts for
dualws_one."""
import ctypes as C
import functools
import os
import numpy as np
import packing as P
from obca_amd import buildflags, scenarios as S, validate as V

D = C.POINTER(C.c_double)
TOL_PARK, TOL_DENSE = 1e-9, 1e-7
DENSE = 256      # samples per interval of the dense sampling
G = V.CERT_TICKS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dp(a):
    return None if a is None else a.ctypes.data_as(D)


@functools.lru_cache(None)
def emu():
    lib = C.CDLL(buildflags.build("certify_emu"))
    lib.emu_certify_last_error.restype = C.c_char_p
    lib.emu_certify_check_args.restype = C.c_char_p; lib.emu_certify_check_args.argtypes = [C.c_double, C.c_double, C.c_int]
    lib.emu_certify_lipschitz_parking.restype = C.c_double; lib.emu_certify_lipschitz_parking.argtypes = [D, D, C.c_double, C.c_double, C.c_double, D]
    lib.emu_certify_lipschitz_quad.restype = C.c_double; lib.emu_certify_lipschitz_quad.argtypes = [D]
    lib.emu_certify_parking.argtypes = [C.c_int, D, D, D, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, D, D, D]
    lib.emu_certify_quad.argtypes = [C.c_int, D, D, D, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, D, D, D]
    lib.emu_certify_pose_clearance.restype = C.c_double; lib.emu_certify_pose_clearance.argtypes = [D, C.c_int, D, C.c_int]
    lib.emu_certify_pose_table.argtypes = [D, C.c_int, D, C.c_int, D]
    a, b, c = (C.c_int(0) for _ in range(3))
    lib.emu_certify_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (V.CERT_OUT, V.CERT_TICKS, 3)
    return lib


# ---------------------------------------------------------------- trajectories
@functools.lru_cache(None)
def golden_parking(name):
    """a solved trajectory of tests/golden/clearance_cases.npz: corridor_sd, corridor_dist (N = 80, 5 obstacles, 0.0551 / 0.0502 at the nodes, contact at sub-step 2 of
    interval 13) or backwards30 (N = 30, 3 obstacles, 0.0564 at the nodes, 0.0244 between them)"""
    g = np.load(os.path.join(GOLDEN, "clearance_cases.npz"))
    c = {k: g[name + "__" + k] for k in ("ego", "vOb", "A", "b", "x", "u", "ts")}
    c.update(N=int(g[name + "__N"]), Ts=float(g[name + "__Ts"]), L=float(g[name + "__L"]), name=name)
    return c


SYNTHETIC = ("straight", "turn", "reverse", "rest")


@functools.lru_cache(None)
def synthetic_parking(kind, N):
    """N intervals of the bicycle step from a pose in the aisle of the shipped scenario (the wedges' upper edges at y = 5, the far wall at y = 11; the car is 2 wide):
    straight along the wedges 0.15 above them, a full-lock left turn, reversing with a steered wheel while braking, and a car at rest (Lambda = 0).  timeScale varies."""
    sc = S.BACKWARDS; A, b, vOb = S.scenario_hrep(sc)
    x0, u = {"straight": ((-7.0, 6.15, 0.0, 1.0), (0.0, 0.0)), "turn": ((-4.0, 6.6, 0.1, 0.9), (0.6, 0.3)),
             "reverse": ((3.0, 6.4, 0.05, -0.8), (-0.35, 0.25)), "rest": ((-2.0, 6.3, 0.2, 0.0), (0.4, 0.0))}[kind]
    ts = 1 + 0.1 * np.sin(np.arange(N + 1.0) + 1)
    x = np.zeros((4, N + 1)); x[:, 0] = x0; uu = np.tile(np.array(u, float)[:, None], (1, N))
    for k in range(N):
        x[:, k + 1] = V._dyn(x[:, k], uu[:, k], ts[k], sc["Ts"], S.L_WHEELBASE)
    return dict(N=N, Ts=float(sc["Ts"]), L=S.L_WHEELBASE, ego=S.EGO.copy(), vOb=np.asarray(vOb, np.int32), A=np.asarray(A, float), b=np.asarray(b, float), x=x, u=uu, ts=ts,
                name="%s%d" % (kind, N))


def synthetic_cases():
    return [synthetic_parking(kind, N) for N in (1, 2, 3) for kind in SYNTHETIC]


@functools.lru_cache(None)
def golden_quads():
    """the four solved make_quad_batch(4, 20) states of tests/golden/rollout_cases.npz"""
    g = np.load(os.path.join(GOLDEN, "rollout_cases.npz")); bt = S.make_quad_batch(4, 20)
    assert g["quad_x"].shape == (4, 12, 21)
    return [dict(N=20, Ts=float(bt["Ts"]), R=float(bt["R"]), ob=np.asarray(bt["ob"], float).reshape(5, 6), x=np.ascontiguousarray(g["quad_x"][i]), ts=np.full(21, float(g["quad_t"][i])),
                 name="quad%d" % i) for i in range(4)]


def cut_quad(c, N):
    """the first N intervals of a quadcopter case"""
    return dict(c, N=N, x=np.ascontiguousarray(c["x"][:, :N + 1]), ts=c["ts"][:N + 1].copy(), name="%s_N%d" % (c["name"], N))


def slip_quad():
    """N = 2, R = 0.25, Ts = 0.5, t = 1, p_0 = 0, v_0 = (4, 0, 0): interval 0 runs from x = 0 to x = 2 in steps of 0.25 at 8 sub-steps.  One box is x in [1.10, 1.15],
    y in [0.27, 0.77], z in [-1, 1]; the other four are far away.  The samples at x = 1.0 and 1.25 keep sqrt(0.01 + 0.0729) - 0.25 = 0.0379, the path comes to 0.27 - 0.25
    = 0.02 between them."""
    x = np.zeros((12, 3)); x[6, :] = 4.0; x[0, :] = [0.0, 2.0, 4.0]
    far = [[60.0 + 3 * i, 51.0, 51.0, -(59.0 + 3 * i), -50.0, -50.0] for i in range(4)]
    ob = np.array([[1.15, 0.77, 1.0, -1.10, -0.27, 1.0]] + far)
    return dict(N=2, Ts=0.5, R=0.25, ob=ob, x=x, ts=np.ones(3), name="slip")


def vmax_of(c):
    return int(np.asarray(c["vOb"]).max())


# ---------------------------------------------------------------- the host build
def _park_prob(c):
    N, vOb = c["N"], c["vOb"]; zero = np.zeros(N + 1)
    return P.pack_problem(np.zeros(4), np.zeros(4), N, c["Ts"], c["L"], c["ego"], np.zeros(4), vOb, c["A"], c["b"], zero, zero, zero, 0)


def unpack_items(items, N, nOb):
    """the item table of the kernel text (3 doubles per item) as (N+1, nOb, 5): lb, seen, tick of seen, tick of the first violation (G: none), samples"""
    t = np.asarray(items, float).reshape(N + 1, nOb, 3); pk = t[:, :, 2].astype(np.int64)
    return np.stack([t[:, :, 0], t[:, :, 1], pk & 8191, (pk >> 13) & 8191, pk >> 26], axis=2).astype(float)


def emu_parking(c, need=V.DMIN, slack=0.01, max_steps=G, vmax=None, rev=0, resident=False):
    """one instance through the kernel text: (record (16,), intervals (N+1, 2), items (N+1, nOb, 5)).  resident: timeScale[0] as the point's single t and no timeScale
    array (what a resident batch holds)"""
    N, vOb = c["N"], c["vOb"]; nOb, M = len(vOb), int(np.sum(vOb))
    prob = _park_prob(c)
    z = P.pack_start(N, nOb, M, c["x"].T, c["u"].T, np.zeros((N + 1, M)), np.zeros((N + 1, 4 * nOb)))
    ts = np.ascontiguousarray(c["ts"], float)
    if resident:
        z[P.layout(N, nOb, M)["t"]] = ts[0]
    out = np.full(V.CERT_OUT, -7.0); iv = np.full((N + 1, 2), -7.0); items = np.full((N + 1) * nOb * 3, -7.0)
    rc = emu().emu_certify_parking(N, dp(prob), dp(z), None if resident else dp(ts), vmax or vmax_of(c), float(need), float(slack), int(max_steps), int(rev), dp(iv), dp(out), dp(items))
    assert rc == 0, emu().emu_certify_last_error()
    return out, iv, unpack_items(items, N, nOb)


def _quad_prob(c):
    N = c["N"]
    return P.pack_quad_problem(np.zeros(12), np.zeros(12), N, c["Ts"], c["R"], c["ob"], np.zeros((N + 1, 12)), 1.0)


def emu_quad(c, need=0.0, slack=0.01, max_steps=G, rev=0, tstride=1):
    N = c["N"]; prob = _quad_prob(c)
    xs = np.ascontiguousarray(c["x"].T); ts = np.ascontiguousarray(c["ts"], float)
    out = np.full(V.CERT_OUT, -7.0); iv = np.full((N + 1, 2), -7.0); items = np.full((N + 1) * 5 * 3, -7.0)
    rc = emu().emu_certify_quad(N, dp(prob), dp(xs), dp(ts), int(tstride), float(need), float(slack), int(max_steps), int(rev), dp(iv), dp(out), dp(items))
    assert rc == 0, emu().emu_certify_last_error()
    return out, iv, unpack_items(items, N, 5)


def host_distance(c, vmax=None):
    """dist(pose, j) of validate.certify_parking: the host build's own DualMultWS distance of one pose to obstacle j of case c (with its clamp)"""
    prob = _park_prob(c); vm = vmax or vmax_of(c); lib = emu()

    def dist(pose, j):
        return lib.emu_certify_pose_clearance(dp(prob), vm, dp(np.ascontiguousarray(pose, float)), int(j))
    return dist


def polygon_distance(c):
    """dist(pose, j): the exact distance of the car rectangle to obstacle j (tests/polygon_distance.py)"""
    import polygon_distance as PD
    off = np.r_[0, np.cumsum(c["vOb"])]

    def dist(pose, j):
        return PD.polygon_distance(pose[0], pose[1], pose[2], c["ego"], c["A"][off[j]:off[j + 1]], c["b"][off[j]:off[j + 1]])
    return dist


# ---------------------------------------------------------------- the statement and the dense sampling
def ref_parking(c, need=V.DMIN, slack=0.01, max_steps=G, dist=None):
    """(record, intervals, items, lam) of the numpy statement with the distance `dist` (default: the host build's own)"""
    items, lam = V.certify_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], c["ego"], len(c["vOb"]), dist or host_distance(c), need, slack, max_steps)
    rec, iv = V.certify_record(items, lam)
    return rec, iv, items, lam


def ref_quad(c, need=0.0, slack=0.01, max_steps=G):
    items, lam = V.certify_quad(c["x"], c["ts"], c["Ts"], c["ob"], c["R"], need, slack, max_steps)
    rec, iv = V.certify_record(items, lam)
    return rec, iv, items, lam


@functools.lru_cache(None)
def _dense_parking(name_key):
    c = _BY_NAME[name_key]
    poses = V.parking_samples(c["x"], c["u"], c["ts"], c["Ts"], c["L"], DENSE)
    prob = _park_prob(c); out = np.zeros((len(poses), len(c["vOb"])))
    emu().emu_certify_pose_table(dp(prob), vmax_of(c), dp(np.ascontiguousarray(poses)), len(poses), dp(out))
    return out


_BY_NAME = {}


def dense_parking(c):
    """(N DENSE + 1, nOb) clearances of the same path sampled DENSE times per interval: validate.parking_samples and the host build's distance.  Computed once per case."""
    _BY_NAME[c["name"]] = c
    return _dense_parking(c["name"])


def dense_quad(c):
    """the smallest clearance of the same path sampled DENSE times per interval (validate.quad_clearance)"""
    return V.quad_clearance(c["x"], c["ts"], c["Ts"], c["ob"], c["R"], DENSE)[0]


def pose_at(c, k, m):
    """the parking pose at tick m of interval k, as the statement forms it"""
    return V._dyn(c["x"][:, k], c["u"][:, k], m / G * c["ts"][k], c["Ts"], c["L"])[:3] if m else c["x"][:3, k]


# ---------------------------------------------------------------- rules
def check_invariants(rec, iv, need, slack, dense_min, what):
    """what the header promises of a record: min(need, seen) - slack <= lb <= seen (decided), lb <= dense + 1e-7, certified => dense >= need - slack - 1e-7"""
    assert rec[14] == 0 and rec[15] == 0, what
    lb, seen = rec[0], rec[1]
    if rec[9] == 0:
        assert min(need, seen) - slack <= lb + 1e-15 and lb <= seen, (what, lb, seen)
    else:
        assert lb == -np.inf and rec[13] == 0, what
    assert lb <= dense_min + TOL_DENSE, (what, lb, dense_min)
    if rec[13]:
        assert rec[5] == 0 and rec[9] == 0 and dense_min >= need - slack - TOL_DENSE, (what, dense_min)
    assert rec[13] == (1.0 if rec[5] == 0 and rec[9] == 0 else 0.0), what
    assert np.array_equal(iv[:, 0].min(), lb) and np.array_equal(iv[:, 1].min(), seen), what
    assert (rec[5] == 0) == (rec[6] == -1) and ((rec[6:9] == -1).all() or (rec[6:9] >= 0).all()), what


def check_device_parking(dev, div, host, hiv, what, worst=None):
    """a device record and interval array against the host build's: indices, ticks and counts equal, lb, seen and the interval array within 1e-9 max(1, |host|)"""
    idx = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15]
    assert np.array_equal(dev[idx], host[idx]), (what, dev, host)
    if host[14]:
        assert np.array_equal(dev, host, equal_nan=True) and np.array_equal(div, hiv, equal_nan=True), what
        return
    for a, b in ((dev[[0, 1, 12]], host[[0, 1, 12]]), (div.ravel(), hiv.ravel())):
        inf = np.isinf(b)
        assert np.array_equal(a[inf], b[inf]), (what, a, b)
        diff = np.abs(a[~inf] - b[~inf])
        if worst is not None and diff.size:
            worst["parking_value"] = max(worst.get("parking_value", 0.0), float(diff.max()))
        assert (diff <= TOL_PARK * np.maximum(1.0, np.abs(b[~inf]))).all(), (what, a, b)
