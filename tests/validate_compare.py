"""TEST INFRASTRUCTURE shared by tests/test_validate_emu_cpu.py and tests/test_gpu_validate.py: the numpy statement of what the device-side checks return
(obca_amd/validate.py) and the comparison rules.

Agreement bound of a class: 1e-9 * max(1, max|lambda|, max|mu|).  The residuals are sums of <= ~20 products of magnitude <= ~50 (positions <= 15, b <= 11, duals <= 3 on
the batches used), so rounding is about 2e-13; the bound leaves three orders of magnitude for differences between the libm of the host and the device's.
Flags: equal for every instance whose numpy worst value lies outside tol +- that bound; at most one instance of a batch may sit inside the band (and is skipped).
Non-finite points: both flags must be 0, and a class is non-finite wherever numpy's is.  The converse is not asked: validate.py takes several maxima with Python's
built-in max(), which keeps its FIRST argument when the other one is NaN, so a numpy class can be finite where the device's propagating maximum is not."""
import numpy as np
from obca_amd import validate as V

REF_TOL = 5e-5


def bound(*duals):
    return 1e-9 * max([1.0] + [float(np.nanmax(np.abs(d))) for d in duals if np.size(d) and np.isfinite(d).any()])


def numpy_parking(x0, xF, N, Ts, L, ego, XYb, vOb, A, b, x, u, ts, l, n, sl, fixTime=0, dist=False, tol=5e-5):
    """(ok, ref_worst-based ref_ok, the 14 values) of one instance in the conventions of validate_parking / parking_constraints_ref"""
    ts = np.broadcast_to(np.ravel(np.asarray(ts, float)), (N + 1,))
    ok, v = V.validate_parking(x0, xF, N, Ts, L, ego, XYb, vOb, A, b, x, u, ts, l, n, sl, fixTime=fixTime, tol=tol, dist=dist)
    rw = V.parking_constraints_ref_worst(x0, xF, N, Ts, L, ego, XYb, len(np.ravel(vOb)), vOb, A, b, x, u, l, n, ts, fixTime, 0 if dist else 1)
    vec = np.array([v[k] for k in V.VIOL_NAMES[:13]] + [rw], float)
    return bool(ok), bool(rw <= REF_TOL), vec


def numpy_quad(x, u, ts, x0, xF, Ts, lam, ob, R, tol=1e-3):
    ok, w = V.validate_quadcopter(x, u, ts, x0, xF, Ts, lam, ob, R, tol)
    return bool(ok), np.array([w[k] for k in V.QUAD_VIOL_NAMES], float)


def check_classes(dev, ref, bnd, names, what=""):
    dev = np.asarray(dev, float); ref = np.asarray(ref, float)
    for k, name in enumerate(names):
        if not np.isfinite(ref[k]):
            assert not np.isfinite(dev[k]), (what, name, dev[k], ref[k])
        elif np.isfinite(dev[k]):
            assert abs(dev[k] - ref[k]) <= bnd, (what, name, dev[k], ref[k], bnd)
        else:
            assert not np.isfinite(ref).all(), (what, name, "non-finite on the device, every numpy class finite")


def flag_expected(worst, tol, bnd):
    """1 / 0, or None inside the band tol +- bnd"""
    if not np.isfinite(worst):
        return 0
    if abs(worst - tol) <= bnd:
        return None
    return int(worst <= tol)


def parking_flags_expected(vec, finite, tol, bnd):
    """(ok, ref_ok) expected from numpy's 14 values; None where the deciding value is inside the band.  `finite`: every entry of the checked point is finite."""
    if not finite:
        return 0, 0
    cls = vec[:12]
    inside = [abs(c - tol) <= bnd for c in cls]
    ok = 0 if any(c > tol + bnd for c in cls) else (None if any(inside) else 1)
    return ok, flag_expected(vec[13], REF_TOL, bnd)


def quad_flag_expected(vec, finite, tol, bnd):
    if not finite:
        return 0
    thr = [tol, tol, 0.0, 0.0, tol, tol, tol, tol, tol]          # bounds fail strictly above 0
    if any(c > t + bnd for c, t in zip(vec, thr)):
        return 0
    return None if any(abs(c - t) <= bnd for c, t in zip(vec, thr)) else 1


class Band:
    """counts the instances of a batch that were skipped because they sit inside the tolerance band: at most one"""

    def __init__(self):
        self.n = 0

    def check(self, got, want, what=""):
        if want is None:
            self.n += 1
            assert self.n <= 1, ("more than one instance of the batch inside the tolerance band", what)
        else:
            assert int(got) == want, (what, got, want)
