"""Parking warm starts from planner paths on the GPU (run with -m gpu): the host-pointer call obca_parking_path_warm_start_batch against the host build of the same kernel text
(tests/emu/path_ws_emu.cpp) -- bit-equal but for the steering row, where the device library's atan stands against glibc's --, the resident call Batch.set_path_warm_start against
an upload of the arrays the host-pointer call returned, the refusals, and the cost against the interior-point kernel of the same batch.  Helpers: tests/path_ws_common.py."""
import json
import os
import time
import numpy as np
import pytest
from conftest import ROOT
import path_ws_common as K
from obca_amd import api, planner as PL, scenarios as S

pytestmark = pytest.mark.gpu
STEER_BOUND = 1e-14      # both atans keep a few ulp (at most 1.1e-16 each at |delta| <= 0.6 ... 1): the largest difference stays below 1e-15
PROFILE = os.path.join(ROOT, "profiles", "path_ws_device_vs_host.json")
_seen = {"steer_max_abs_diff": 0.0, "steering_angles_compared": 0}


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.Context(0).close()      # fails loudly if the HIP library / device is missing
    return obca_amd


@pytest.fixture(scope="module")
def ctx(OA):
    c = OA.Context(0)
    yield c
    c.close()
    if _seen["steering_angles_compared"]:      # the largest steering difference seen, beside what tools/path_ws_rate.py has written
        try:
            rec = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
            rec["device_vs_host_build"] = dict(_seen, asserted_bound=STEER_BOUND, what="max |delta_device - delta_host| over tests/test_gpu_path_ws.py; every other output bit-equal")
            json.dump(rec, open(PROFILE, "w"), indent=1)
        except OSError:
            pass


@pytest.fixture(scope="module")
def syn():
    return K.synthetic67()


@pytest.fixture(scope="module")
def parked():
    """the start poses of the backwards scenario that have a planner path (of 96 drawn; a start pose may collide), as a problem batch without its warm start"""
    paths, dirs, cnt, xF, x0 = K.planner_paths(S.BACKWARDS, 96, 7, with_x0=True)
    ok = cnt >= 2
    assert ok.sum() >= 80
    paths, dirs, cnt, xF, x0 = (np.ascontiguousarray(a[ok]) for a in (paths, dirs, cnt, xF, x0))
    A, b, vrows = S.scenario_hrep(S.BACKWARDS)
    return dict(paths=paths, dirs=dirs, cnt=cnt, x0=x0, xF=xF, A=A, b=b, vOb=vrows, L=S.L_WHEELBASE, ego=S.EGO.copy(), XYbounds=S.XYBOUNDS.copy())


def _device(ctx, paths, dirs, cnt, N, xF=None, v_nom=0.5, L=S.L_WHEELBASE, a_max=0.0):
    """the C call as it is: (rc, Ts, xWS, uWS, status)"""
    B = len(cnt); paths, dirs, cnt, cap = api._path_arrays(paths, dirs, cnt, B)
    Ts = np.full(B, np.nan); x = np.full((B, N + 1, 4), np.nan); u = np.full((B, N, 2), np.nan); st = np.full(B, 99, np.int32)
    rc = api._load().obca_parking_path_warm_start_batch(ctx._h, B, N, paths, dirs, cnt, cap, None if xF is None else api._in(xF), v_nom, L, a_max, Ts, x, u, st)
    return rc, Ts, x, u, st


def _bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_but_steering(dev, host, what):
    (rc, Ts, x, u, st), (rh, Th, xh, uh, sh) = dev, host
    assert rc == rh == 0 and np.array_equal(st, sh), (what, st, sh)
    assert _bits(Ts, Th) and _bits(x, xh) and _bits(u[:, :, 1], uh[:, :, 1]), (what, np.abs(Ts - Th).max(), np.abs(x - xh).max(), np.abs(u[:, :, 1] - uh[:, :, 1]).max())
    d = float(np.abs(u[:, :, 0] - uh[:, :, 0]).max()) if u.size else 0.0
    print("%s: largest steering difference %.3g" % (what, d))
    _seen["steer_max_abs_diff"] = max(_seen["steer_max_abs_diff"], d); _seen["steering_angles_compared"] += int(u[:, :, 0].size)
    assert d <= STEER_BOUND, (what, d)


@pytest.mark.parametrize("N", [1, 64, 65, 128])
def test_host_pointer_call_against_the_host_build(ctx, syn, N):
    paths, dirs, cnt, xF = syn
    assert len(cnt) == 67 and {63, 64, 65, 1024} <= set(cnt.tolist()) and (cnt < 2).sum() == 1
    for xf in (xF, None):
        for a_max in (0.0, 0.3):
            _same_but_steering(_device(ctx, paths, dirs, cnt, N, xf, a_max=a_max), K.emu_batch(paths, dirs, cnt, N, xf, a_max=a_max), "N = %d, xF %s, a_max %g" % (N, xf is not None, a_max))


def test_planner_paths_and_the_python_entry(ctx, parked):
    """planner paths of another stride (cap 1 024, longest count far below it: the strided staging), through planner.path_to_warm_start_many"""
    p = parked; N = 80
    for smooth in (False, True):
        Ts, x, u, ok = PL.path_to_warm_start_many(p["paths"], p["dirs"], p["cnt"], N, p["xF"], smooth=smooth, device=ctx)
        assert ok.all()
        _same_but_steering((0, Ts, x, u, np.zeros(len(ok), np.int32)), K.emu_batch(p["paths"], p["dirs"], p["cnt"], N, p["xF"], a_max=0.3 if smooth else 0.0), "planner paths, smooth %s" % smooth)
        K.compare((Ts, x, u), K.numpy_batch(p["paths"], p["dirs"], p["cnt"], N, p["xF"], a_max=0.3 if smooth else 0.0), np.arange(len(ok)), "device against numpy")
    sc = S.BACKWARDS
    a = PL.warm_start_many(sc, p["x0"][:6], p["xF"][:6], N, device=ctx); b = PL.warm_start_many(sc, p["x0"][:6], p["xF"][:6], N)
    for (Ta, xa, ua), (Tb, xb, ub) in zip(a, b):
        assert abs(Ta - Tb) <= K.TOL and np.abs(xa - xb).max() <= K.TOL and np.abs(ua - ub).max() <= K.TOL_DELTA


def _upload(OA, ctx, p, sel, N, Ts, ref, xWS, uWS):
    b = OA.Batch(ctx, len(sel), N)
    b.upload(p["x0"][sel], p["xF"][sel], Ts, p["L"], p["ego"], p["XYbounds"], p["vOb"], p["A"], p["b"], ref[:, :, 0], ref[:, :, 1], ref[:, :, 2], 0, xWS, uWS)
    return b


@pytest.mark.parametrize("B", [5, 67])
def test_resident_call_against_upload(OA, ctx, parked, B):
    p = parked; N = 40; sel = np.arange(B)
    paths, dirs, cnt = p["paths"][sel], p["dirs"][sel], p["cnt"][sel]
    rc, Ts, x, u, st = _device(ctx, paths, dirs, cnt, N, p["xF"][sel])
    assert rc == 0 and (st == 0).all()
    # first run: a start of zeros, written on the device
    b1 = _upload(OA, ctx, p, sel, N, np.ones(B), np.zeros((B, N + 1, 3)), None, None)
    st1 = b1.set_path_warm_start(paths, dirs, cnt)
    assert (st1 == 0).all() and b1.path_ws_ms() > 0
    with pytest.raises(OA.ObcaError, match="nothing has been solved"):
        b1.validate()
    b1.solve(opts=OA.ipopt_opts()); v1 = b1.validate(); o1 = b1.download(); b1.close()
    # second run: the arrays the host-pointer call returned, uploaded
    b2 = _upload(OA, ctx, p, sel, N, Ts, x, x, u)
    b2.solve(opts=OA.ipopt_opts()); v2 = b2.validate(); o2 = b2.download()
    for k in ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info"):
        assert _bits(o1[k], o2[k]), k
    assert _bits(v1["viol"], v2["viol"]) and v1["ok"].all() and v2["ok"].all(), (v1["ok"], o1["exitflag"])
    # an instance without a path keeps the uploaded start: the second batch again, its warm start rewritten for all but instance 2
    c2 = cnt.copy(); c2[2] = 0
    st3 = b2.set_path_warm_start(paths, dirs, c2)
    assert st3.tolist() == [0, 0, -1] + [0] * (B - 3)
    b2.solve(opts=OA.ipopt_opts()); o3 = b2.download(); b2.close()
    for k in ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info"):
        assert _bits(o3[k], o2[k]), k


def test_refusals(OA, ctx, syn, parked):
    paths, dirs, cnt, xF = syn; N = 20; B = len(cnt)
    b = OA.Batch(ctx, B, N)
    with pytest.raises(OA.ObcaError, match="nothing uploaded"):      # -1 with a message
        b.set_path_warm_start(paths, dirs, cnt)
    with pytest.raises(OA.ObcaError):
        b.path_ws_ms()
    b.close()
    st = np.zeros(B, np.int32)
    assert api._load().obca_batch_set_path_warm_start(None, paths, dirs, cnt, paths.shape[1], 1, 0.5, 0.0, st) == -1
    for kw in (dict(v_nom=0.0), dict(L=np.inf), dict(a_max=-1.0)):
        assert _device(ctx, paths, dirs, cnt, N, **kw)[0] == -1 and b"obca_parking_path_warm_start_batch" in api._load().obca_last_error(ctx._h)
    assert _device(ctx, paths, dirs, cnt, 0)[0] == -1 and _device(ctx, paths, dirs, cnt, 129)[0] == -1
    # a count above cap: -2 for that instance alone, its neighbours as before; the arrays are cut to 130 rows, so every 1 024-node instance is refused and nothing of it is read
    good = _device(ctx, paths, dirs, cnt, N, xF)
    cut = 130; bad = _device(ctx, np.ascontiguousarray(paths[:, :cut]), np.ascontiguousarray(dirs[:, :cut]), cnt, N, xF)
    long_ = cnt > cut
    assert long_.any() and (bad[4][long_] == -2).all() and np.array_equal(bad[4][~long_], good[4][~long_])
    assert not bad[1][long_].any() and not bad[2][long_].any() and not bad[3][long_].any()
    assert _bits(bad[1][~long_], good[1][~long_]) and _bits(bad[2][~long_], good[2][~long_]) and _bits(bad[3][~long_], good[3][~long_])
    c1 = cnt.copy(); c1[5] = paths.shape[1] + 1
    one = _device(ctx, paths, dirs, c1, N, xF)
    keep = np.arange(B) != 5
    assert one[4][5] == -2 and np.array_equal(one[4][keep], good[4][keep]) and _bits(one[2][keep], good[2][keep]) and _bits(one[3][keep], good[3][keep])
    # the same through the resident call
    p = parked; sel = np.arange(5); Bp = 5
    bb = _upload(OA, ctx, p, sel, N, np.ones(Bp), np.zeros((Bp, N + 1, 3)), None, None)
    cc = p["cnt"][sel].copy(); cc[3] = p["paths"].shape[1] + 1
    assert bb.set_path_warm_start(p["paths"][sel], p["dirs"][sel], cc).tolist() == [0, 0, 0, -2, 0]
    bb.close()


def test_config2_sized_batch_costs_less_than_its_solve(OA, ctx, parked):
    """B = 1 024, N = 80 (the 96 planned paths repeated): the wall time of set_path_warm_start -- packing, transfer, kernel, status download -- against the interior-point
    kernel of that batch's solve, the yardstick of tests/test_gpu_validate.py"""
    p = parked; N, B = 80, 1024; sel = np.arange(B) % len(p["cnt"])
    paths = np.ascontiguousarray(p["paths"][sel]); dirs = np.ascontiguousarray(p["dirs"][sel]); cnt = np.ascontiguousarray(p["cnt"][sel])
    b = _upload(OA, ctx, p, sel, N, np.ones(B), np.zeros((B, N + 1, 3)), None, None)
    assert (b.set_path_warm_start(paths, dirs, cnt) == 0).all()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter(); b.set_path_warm_start(paths, dirs, cnt); walls.append((time.perf_counter() - t0) * 1e3)
    kern = b.path_ws_ms()
    b.solve(); b.sync(); ipm_ms = b.kernel_ms()[0]; out = b.download(); b.close()
    print("B = %d, N = %d: set_path_warm_start wall min %.3f ms of %s, kernel %.3f ms; ipm kernel %.3f ms, %d solved" % (B, N, min(walls), ["%.3f" % w for w in walls], kern, ipm_ms, (out["exitflag"] == 1).sum()))
    assert (out["exitflag"] == 1).sum() >= B // 2      # (the start is a usable one: the solve it is measured against is a real solve)
    assert min(walls) < ipm_ms, (walls, ipm_ms)
