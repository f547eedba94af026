"""What the Python layer hands to the C ABI, pinned without a device: a stand-in for the loaded libraries records every call (tests/golden/make_abi_calls.py says how, and
drives every Python entry point once at B = 2, N = 3).  tests/golden/abi_calls.json is that record of the code BEFORE the bindings were read from the headers, when every call
site spelled its C types by hand; the code as it stands must hand the same entry points the same values and the same bytes, and return the same arrays."""
import json
import os
import sys
import numpy as np
import pytest
from conftest import GOLDEN
from obca_amd import api, cabi, planner

sys.path.insert(0, GOLDEN)
import make_abi_calls as G      # noqa: E402

# entry points no Python call of the package reaches, with the reason
UNREACHED = {"obca_plan3d_destroy": "the planner contexts live as long as the process (planner._ctx3d); only tools/plan3d_rate.py and the GPU tests destroy one"}


@pytest.fixture(scope="module")
def rec():
    lib, ret = G.record()
    return lib, ret, json.load(open(os.path.join(GOLDEN, "abi_calls.json")))


def test_the_same_calls_reach_the_abi(rec):
    lib, ret, gold = rec
    assert (gold["B"], gold["N"]) == (G.B, G.N)
    now = json.loads(json.dumps(lib.calls))
    assert [c[0] for c in now] == [c[0] for c in gold["calls"]]
    for k, (a, b) in enumerate(zip(now, gold["calls"])):
        assert a == b, (k, a[0], [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y], len(a), len(b))


def test_the_python_calls_return_the_same(rec):
    _, ret, gold = rec
    now = json.loads(json.dumps(ret))
    assert [r[0] for r in now] == [r[0] for r in gold["returns"]]
    for a, b in zip(now, gold["returns"]):
        assert a == b, a[0]
    errors = [r[1] for r in now if "refused" in r[0]]
    assert len(errors) == 7 and all(e and e[0] in ("ObcaError", "Plan3DError") and "stand-in says no" in e[1] for e in errors)      # the library's message, in the package's exception


def test_every_call_has_the_declared_arguments(rec):
    lib = rec[0]
    sig = {n: s for h in G.HEADERS for n, s in cabi.prototypes(h).items()}
    for name, args in lib.live:
        argtypes = sig[name][1]
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for k, (a, t) in enumerate(zip(args, argtypes)):
            t.from_param(a)      # raises if the bound function would refuse it
    reached = {name for name, _ in lib.live}      # (obca_visible_device_count: asked of the raw library, as bench.py does -- no function of the package calls it)
    assert set(api.EXPORTS + planner.PLAN3D_EXPORTS) - reached == set(UNREACHED)


def _rows(args, k_nob, k_vob):
    """(half-space rows, obstacles) of all instances together, from the nOb / vOb arguments of a call"""
    nOb, vOb = args[k_nob], args[k_vob]
    assert nOb.dtype == np.int32 and vOb.dtype == np.int32 and vOb.size == nOb.sum()
    return int(vOb.sum()), int(nOb.sum())


def test_array_lengths_of_the_host_pointer_solves(rec):
    """the sizes include/obca_hip.h states in its comments: the library reads and writes that many elements through the raw pointers"""
    lib = rec[0]
    seen = set()
    for name, a in lib.live:
        if name in ("obca_parking_signed_dist_batch", "obca_parking_dist_batch"):
            B, N = a[1], a[2]; N1 = N + 1
            Mt, nt = _rows(a, 10, 11)
            want = {3: B, 5: 4, 6: 4, 8: 4 * B, 9: 4 * B, 10: B, 12: 2 * Mt, 13: Mt, 14: N1 * B, 15: N1 * B, 16: N1 * B, 17: 4 * N1 * B, 18: 2 * N * B,
                    22: 4 * N1 * B, 23: 2 * N * B, 24: N1 * B, 25: B, 26: Mt * N1, 27: 4 * nt * N1}      # Ts ego XYbounds x0 xF nOb A b rx ry ryaw xWS uWS | xp up timeScale exitflag lp np
            if name == "obca_parking_signed_dist_batch":
                want.update({28: nt * N1, 29: 8 * B})      # slp, info
            else:
                want.update({28: 8 * B})                   # info
            for k in (19, 20):      # lWS, nWS: NULL or packed like lp / np
                assert a[k] is None or a[k].size == want[k + 7], (name, k)
            assert a[25].dtype == np.int32
        elif name in ("obca_quadcopter_signed_dist_batch", "obca_quadcopter_dist_batch"):
            B, N = a[1], a[2]; N1 = N + 1
            assert a[9] is None      # uWS
            want = {3: B, 5: 12 * B, 6: 12 * B, 7: 30 * B, 8: 12 * N1 * B, 10: B, 13: 12 * N1 * B, 14: 4 * N * B, 15: N1 * B, 16: B, 17: 30 * N1 * B}      # Ts x0 xF ob xWS timeWS | xp up timeScale exitflag lp
            want.update({18: 5 * N1 * B, 19: 8 * B} if name == "obca_quadcopter_signed_dist_batch" else {18: 8 * B})      # slack, info
            assert a[16].dtype == np.int32
        else:
            continue
        seen.add(name)
        assert (B, N) in ((G.B, G.N), (1, G.N))
        for k, n in want.items():
            assert isinstance(a[k], np.ndarray) and a[k].size == n and a[k].flags.c_contiguous and a[k].dtype in (np.float64, np.int32), (name, k, n)
    assert len(seen) == 4
