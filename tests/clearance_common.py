"""What tests/test_clearance_cpu.py and tests/test_gpu_clearance.py share: the host build of the kernel text of obca_amd/csrc/obca_clearance.h (tests/emu/clearance_emu.cpp,
buildflags.build("clearance_emu")); the trajectories both suites run -- warm starts, never solved --; the reference record of a parking trajectory (numpy parking_samples +
the oracle's DualMultWS on the sample poses + the clamp); the comparison rules of the two suites.

Tolerances.  Parking values: 1e-9 max(1, |d|), the bound the project holds its DualMultWS against the oracle's with (tests/test_gpu_parity.py, tests/test_emu_cpu.py): both
sides follow the same central path down to a complementarity of 1e-9 and may stop one step apart.  Indices: equal, or the reference's own c at the reported (q, j) lies within
2e-9 of the reference minimum (two values that each side knows to 1e-9).  `below`: between the reference's counts at need -+ 1e-9.  Quadcopter values: 1e-12 -- a dozen
fp64 operations on numbers of size <= 10 (one rounding is 1e-15 there), numpy and g++ without contraction: bits are expected."""
import ctypes as C
import functools
import numpy as np
import packing as P
from obca_amd import buildflags, scenarios as S, validate as V

D = C.POINTER(C.c_double)
TOL_PARK, TOL_TIE, TOL_QUAD = 1e-9, 2e-9, 1e-12
SHAPES = ((1, 1), (5, 3), (7, 4), (33, 8), (128, 32))      # (N, S): items below 64, just above 64, ..., the largest
QUAD_SHAPES = ((2, 1), (7, 4), (60, 32))


def dp(a):
    return None if a is None else a.ctypes.data_as(D)


@functools.lru_cache(None)
def emu():
    lib = C.CDLL(buildflags.build("clearance_emu"))
    lib.emu_clearance_last_error.restype = C.c_char_p
    lib.emu_clearance_parking.argtypes = [C.c_int, D, D, D, C.c_int, C.c_int, C.c_double, C.c_int, D]
    lib.emu_clearance_quad.argtypes = [C.c_int, D, D, D, C.c_int, C.c_int, C.c_double, C.c_int, D]
    a, b, c = (C.c_int(0) for _ in range(3))
    lib.emu_clearance_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (V.CLR_OUT, 32, 16)
    return lib


# ---------------------------------------------------------------- trajectories
def _instances(bt, ts):
    B = len(bt["Ts"]); per = isinstance(bt["vOb"], list)
    return [dict(N=bt["N"], Ts=float(bt["Ts"][i]), L=bt["L"], ego=bt["ego"], vOb=np.asarray(bt["vOb"][i] if per else bt["vOb"], np.int32), A=np.asarray(bt["A"][i] if per else bt["A"], float),
                 b=np.asarray(bt["b"][i] if per else bt["b"], float), x=np.ascontiguousarray(bt["xWS"][i, :bt["N"] + 1].T), u=np.ascontiguousarray(bt["uWS"][i, :bt["N"]].T), ts=ts.copy())
            for i in range(B)]


@functools.lru_cache(None)
def parking_cases(N, B=6):
    """the warm starts of make_batch(BACKWARDS, B, N) with timeScale 1 and with 1 + 0.1 sin k, and of make_mixed_batch(B, N, min_obstacles=1, rows=(3, 8), max_rows=64):
    up to 8 rows per obstacle, 3 .. 10 obstacles at these sizes; and of make_mixed_batch(B, N) (3 or 4 rows per extra obstacle) -- the row class is a BATCH's (its widest
    obstacle, as launch_dualws picks it), and these are the classes 2, 2, 8 and 4.  A list of batches (lists of instances)."""
    one = np.ones(N + 1); wav = 1 + 0.1 * np.sin(np.arange(N + 1.0))
    bw = S.make_batch(S.BACKWARDS, B, N); mx = S.make_mixed_batch(B, N, min_obstacles=1, rows=(3, 8), max_rows=64); m4 = S.make_mixed_batch(B, N)
    return [_instances(bw, one), _instances(bw, wav), _instances(mx, one), _instances(m4, wav)]


@functools.lru_cache(None)
def quad_cases(N, B=6):
    bt = S.make_quad_batch(B, N)
    x = bt["xWS"].copy()
    x[:, :-1, 6:9] = np.diff(x[:, :, :3], axis=1) / bt["Ts"]      # the warm start carries positions only: velocities that lead from node to node ...
    x[:, :, 6:9] *= (1 + 0.2 * np.cos(np.arange(N + 1.0)))[None, :, None]      # ... and then do not quite
    ts = 1 + 0.1 * np.sin(np.arange(N + 1.0))
    return [dict(N=N, Ts=float(bt["Ts"]), R=bt["R"], ob=bt["ob"], x=np.ascontiguousarray(x[i].T), ts=ts.copy()) for i in range(B)]


def vmax_of(batch):
    return int(max(int(c["vOb"].max()) for c in batch))


# ---------------------------------------------------------------- the host build
def emu_parking(c, substeps, need=V.DMIN, vmax=None, rev=0, resident=False):
    """one instance through the kernel text: the record (24,).  resident: timeScale[0] as the point's single t and no timeScale array (what a resident batch holds)"""
    N, vOb = c["N"], c["vOb"]; nOb, M = len(vOb), int(vOb.sum()); zero = np.zeros(N + 1)
    prob = P.pack_problem(np.zeros(4), np.zeros(4), N, c["Ts"], c["L"], c["ego"], np.zeros(4), vOb, c["A"], c["b"], zero, zero, zero, 0)
    z = P.pack_start(N, nOb, M, c["x"].T, c["u"].T, np.zeros((N + 1, M)), np.zeros((N + 1, 4 * nOb)))
    ts = np.ascontiguousarray(c["ts"], float)
    if resident:
        z[P.layout(N, nOb, M)["t"]] = ts[0]
    out = np.full(V.CLR_OUT, -7.0)
    rc = emu().emu_clearance_parking(N, dp(prob), dp(z), None if resident else dp(ts), vmax or int(vOb.max()), int(substeps), float(need), int(rev), dp(out))
    assert rc == 0, emu().emu_clearance_last_error()
    return out


def emu_quad(c, substeps, need=0.0, rev=0, tstride=1):
    N = c["N"]
    prob = P.pack_quad_problem(np.zeros(12), np.zeros(12), N, c["Ts"], c["R"], c["ob"], np.zeros((N + 1, 12)), 1.0)
    xs = np.ascontiguousarray(c["x"].T); ts = np.ascontiguousarray(c["ts"], float); out = np.full(V.CLR_OUT, -7.0)
    rc = emu().emu_clearance_quad(N, dp(prob), dp(xs), dp(ts), int(tstride), int(substeps), float(need), int(rev), dp(out))
    assert rc == 0, emu().emu_clearance_last_error()
    return out


# ---------------------------------------------------------------- the independent statement
def ref_parking_table(c, substeps):
    """c_ref (N S + 1, nOb): numpy sample poses, the oracle's DualMultWS distance of every pose to every obstacle, the clamp"""
    import oracle as O
    poses = V.parking_samples(c["x"], c["u"], c["ts"], c["Ts"], c["L"], substeps)
    _, _, d = O.dualmult_ws(len(poses) - 1, c["vOb"], c["A"], c["b"], poses[:, 0].copy(), poses[:, 1].copy(), poses[:, 2].copy(), c["ego"])
    return np.where(d < V.CLR_TOUCH, 0.0, d)


def check_parking_record(rec, table, substeps, need, what, worst=None):
    """a record of the kernel text (host build or device) against a table of reference clearances, by the rules in this file's head"""
    ref = V.clearance_record(table, substeps, need); nOb = table.shape[1]
    assert rec[6] == 0 and rec[7] == 0 and rec[5] == ref[5] == table.shape[0], what
    for i in (0, 1, *range(8, 8 + nOb)):
        assert abs(rec[i] - ref[i]) <= TOL_PARK * max(1.0, abs(ref[i])), (what, i, rec[i], ref[i])
        if worst is not None:
            worst["parking_value"] = max(worst.get("parking_value", 0.0), abs(rec[i] - ref[i]))
    assert np.isinf(rec[8 + nOb:]).all() and (rec[8 + nOb:] > 0).all(), what
    q, j = int(rec[2]), int(rec[3])
    assert rec[2] == q and rec[3] == j and 0 <= q < table.shape[0] and 0 <= j < nOb, what
    assert (q, j) == (int(ref[2]), int(ref[3])) or abs(table[q, j] - ref[0]) <= TOL_TIE, (what, q, j, ref[2], ref[3], table[q, j], ref[0])
    rowmin = table.min(axis=1)
    assert (rowmin < need - TOL_PARK).sum() <= rec[4] <= (rowmin < need + TOL_PARK).sum(), (what, rec[4])
    if substeps == 1:
        assert rec[0] == rec[1], what
    return ref


def check_against_host_build(dev, host, tol, nOb, what, table=None, substeps=None, need=None, worst=None, key="value"):
    """a device record against the host build's record of the same instance: the same bad flag (then the same record); values within tol max(1, |host|); sample, obstacle and
    `below` equal -- or, where `table` (a callable returning the reference table: parking) is given, the device record passes the rules against the independent statement
    by itself (a near tie, a clearance within 1e-9 of `need`).  worst[key] collects the largest value difference."""
    assert dev[5] == host[5] and dev[6] == host[6] and dev[7] == 0, (what, dev[:8], host[:8])
    if host[6]:
        assert np.array_equal(dev, host, equal_nan=True), what
        return
    idx = [0, 1, *range(8, 8 + nOb)]
    diff = np.abs(dev[idx] - host[idx])
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), float(diff.max()))
    assert (diff <= tol * np.maximum(1.0, np.abs(host[idx]))).all(), (what, dev[idx], host[idx])
    assert np.array_equal(dev[8 + nOb:], host[8 + nOb:]), what
    if not np.array_equal(dev[2:5], host[2:5]):
        assert table is not None, (what, dev[2:5], host[2:5])
        check_parking_record(dev, table(), substeps, need, what + " (device against the independent statement)")
