"""What the Python front end above the first ABI hands to the libraries, pinned without a device: the planner routes (host threads, the device planner, per-instance fields,
each with its second search of the long paths), the device search wrappers, the timers, the refines with their selections and the resident planners.  A stand-in for the
loaded libraries, the host planner included, records every call (tests/golden/make_front_end_calls.py says how and what it drives).  tests/golden/front_end_calls.json is
that record of the code BEFORE these routes, timers and refines were stated once; the code as it stands must make the same calls in the same order with the same values and
the same bytes -- not one device call more --, return the same arrays and raise the same exceptions with the same text."""
import json
import os
import sys
import pytest
from conftest import GOLDEN
from obca_amd import cabi

sys.path.insert(0, GOLDEN)
import make_front_end_calls as G      # noqa: E402

# functions of the nine headers no call of the driver reaches, with the reason
UNREACHED = {}


@pytest.fixture(scope="module")
def rec():
    lib, ret = G.record()
    return lib, ret, json.load(open(os.path.join(GOLDEN, "front_end_calls.json")))


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
    by = dict((r[0], r[1]) for r in now)
    refused = [v for k, v in by.items() if k.endswith("refused")]      # the library's message, in the package's exception
    assert len(refused) == 13 and all(e and e[0] == "ObcaError" and "stand-in says no" in e[1] for e in refused)
    # the three refusals of the refines, word for word, and the searches' argument checks
    for q in ("", "quad "):
        assert by[q + "refine empty"] == ["ObcaError", "refine: the selection is empty"]
        assert by[q + "refine index"] == ["ObcaError", "refine: an index outside 0 .. 1"]
        assert by[q + "refine factor"] == ["ObcaError", "refine: need 1 <= factor <= 32"]
    assert by["quad plan_warm_start empty"] == ["ObcaError", "plan_warm_start: the selection is empty"]
    assert by["warm_start_many search"] == ["ValueError", "search must be 'host' or 'device'"] and by["warm_start_many search needs a device"] == ["ValueError", "search='device' needs a device"]
    assert by["astar3d_many unsettled"] == ["Plan3DError", "the relaxation of instances [1] did not settle"]
    assert by["warm_start_many empty"] == [] and by["scene_warm_start_many empty"] == []


def test_every_call_has_the_declared_arguments(rec):
    lib = rec[0]
    sig = {n: s for h in G.HEADERS + G.SUPPORT for n, s in cabi.prototypes(h).items()}
    for name, args in lib.live:
        argtypes = sig[name][1]
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for a, t in zip(args, argtypes):
            t.from_param(a)      # raises if the bound function would refuse it


def test_every_function_of_the_nine_headers_is_reached(rec):
    reached = {name for name, _ in rec[0].live}
    declared = {n for h in G.HEADERS for n in cabi.prototypes(h)}
    assert len(G.HEADERS) == 9 and len(declared) == 28
    assert declared - reached == set(UNREACHED)
