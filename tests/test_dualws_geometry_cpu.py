"""DualMultWS on the CPU against exact polygon geometry: the oracle (oracle/obca_oracle.c: dualws_one) and the host build of the kernel text (obca_amd/csrc/obca_model.h:
dualws_one through tests/emu) on EVERY case of tests/golden/dualws_polygons.npz -- expected distances from tests/polygon_distance.py, confirmed with mpmath at 40 digits
by tests/golden/make_dualws_polygons.py.  The other DualMultWS tests compare one statement of the iteration with another; the only geometry they see is 64 half-planes.

Per case:  -2e-8 <= d,  |d - d_exact| <= 2e-8,  and the dual certificate of polygon_distance.certificate holds for the returned multipliers.
2e-8: the path following stops at an average complementarity of 1e-9 over v + 5 <= 13 pairs with residuals below 1e-9, a duality gap of at most 1.3e-8; the same bound at
every gap from 0 to 40 m -- no case is skipped and the tolerance does not grow with the distance.

Before the second attempt of dualws_one existed (the loop ended at 60 passes, converged or not) these tests failed, for the oracle and the host build alike, on 25 cases:
all 3 wedges (9.8 cm, 37 cm and 82 cm short) and 22 of the 432 stretched polygons (all of aspect ratio 0.05, from 1.2e-7 short at a gap of 5 m to 18.3 m short at a gap
of 40 m), every other family passing."""
import ctypes as C
import numpy as np
import pytest
from conftest import golden
import polygon_distance as PD

D = C.POINTER(C.c_double)
dp = lambda a: a.ctypes.data_as(D)
TOL_D = 2e-8
FAMILIES = ("regular", "stretched", "wedge", "box", "overlap", "small", "halfplane", "scenario")


@pytest.fixture(scope="module")
def cases():
    g = golden("dualws_polygons.npz")
    assert sorted(set(g["family"].tolist())) == sorted(FAMILIES) and len(g["d"]) >= 600
    return {k: g[k] for k in g.files}


def run_oracle(oracle, X, Y, psi, ego, A, b):
    l, n, d = oracle.dualmult_ws(0, [len(b)], A, b, [X], [Y], [psi], ego)
    return l[0], n[0], float(d[0, 0])


def run_host_build(emu, X, Y, psi, ego, A, b):
    """dualws_one<8> of the kernel text, on unit rows as the host layer hands them to the kernel; lam back in the caller's scaling"""
    g, off = PD.car_geometry(ego); v = len(b); nr = np.hypot(A[:, 0], A[:, 1])
    a1 = np.ascontiguousarray(A[:, 0] / nr); a2 = np.ascontiguousarray(A[:, 1] / nr); bj = np.ascontiguousarray(b / nr)
    cs, sn = np.cos(psi), np.sin(psi); lam = np.zeros(8); mu = np.zeros(4); d = C.c_double(0)
    emu.emu_dualws(C.c_int(v), dp(a1), dp(a2), dp(bj), dp(g), C.c_double(X + off * cs), C.c_double(Y + off * sn), C.c_double(cs), C.c_double(sn), dp(lam), dp(mu), C.byref(d))
    return lam[:v] / nr, mu, d.value


def check_case(g, i, lam, mu, d):
    """None, or what is wrong with the answer to case i"""
    v = int(g["v"][i]); A, b = g["A"][i, :v], g["b"][i, :v]; X, Y, psi = g["pose"][i]; dx = float(g["d"][i])
    if not (np.isfinite(d) and np.isfinite(lam).all() and np.isfinite(mu).all()):
        return "not finite"
    if d < -TOL_D or abs(d - dx) > TOL_D:
        return "d = %.12g, exact %.12g: off by %.3g" % (d, dx, d - dx)
    c = PD.certificate(X, Y, psi, g["ego"], A, b, lam, mu, d)
    return None if PD.certificate_ok(c) else "certificate %s" % c


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("impl", ["oracle", "host_build"])
def test_dualws_against_polygon_geometry(request, cases, impl, family):
    g = cases
    if impl == "oracle":
        lib = request.getfixturevalue("oracle"); run = run_oracle
    else:
        lib = request.getfixturevalue("emu"); run = run_host_build
    idx = np.flatnonzero(g["family"] == family); bad = []
    for i in idx:
        v = int(g["v"][i])
        why = check_case(g, i, *run(lib, *g["pose"][i], g["ego"], g["A"][i, :v].copy(), g["b"][i, :v].copy()))
        if why:
            bad.append("%s: %s" % (g["name"][i], why))
    assert not bad, "%d of %d %s cases fail:\n  %s" % (len(bad), len(idx), family, "\n  ".join(bad))


def test_fixture_matches_the_reference_module(cases):
    """the expected distances are those of tests/polygon_distance.py on this machine as well (a sample of every family: the whole file takes the generator half a minute),
    no exact gap sits in the window of the clearance threshold, and the named wedge is the one the record speaks of"""
    g = cases
    for f in FAMILIES:
        for i in np.flatnonzero(g["family"] == f)[::17]:
            v = int(g["v"][i])
            assert abs(PD.polygon_distance(*g["pose"][i], g["ego"], g["A"][i, :v], g["b"][i, :v]) - g["d"][i]) <= 1e-13 * max(1.0, g["d"][i]), g["name"][i]
    assert not ((g["d"] > 8e-8) & (g["d"] < 1.2e-7)).any()
    w = int(np.flatnonzero(g["name"] == "wedge_9.8cm")[0])
    assert abs(g["d"][w] - 8.403072014558) < 1e-11 and g["pose"][w].tolist() == [0.0, 0.0, 1.0]
