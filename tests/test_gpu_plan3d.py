"""The 3-D grid planner on the GPU (run with -m gpu): libobca_plan3d.so against the sequential host build of the same kernel text (bit for bit: the in-place relaxation is
order independent on the hardware too), against the host A*, against itself (repeats, a foreign pattern in LDS, a batch larger than the machine), the statuses through the
C ABI, the solves from its warm starts, and its cost against the host loop.  Bounded kernels only.  Helpers and the cost tolerance: tests/plan3d_common.py."""
import ctypes as C
import json
import os
import time
import numpy as np
import pytest
import plan3d_common as K
from obca_amd import scenarios as S, planner as PL

pytestmark = pytest.mark.gpu
NPAIRS = 256


@pytest.fixture(scope="module")
def dev():
    PL.plan3d_context(0)      # fails loudly if the library / device is missing
    return 0


@pytest.fixture(scope="module")
def pool():
    """256 random pairs + the shipped one: the emulation's answers and the device's"""
    x0, xF = K.endpoints(NPAIRS)
    rc, paths, cnt, sw = K.emu_paths(x0[:, :3], xF[:, :3])
    assert rc == 0
    return dict(x0=x0, xF=xF, paths=paths, cnt=cnt, sweeps=sw)


def test_device_equals_the_emulation_bit_for_bit(dev, pool):
    p = pool
    dpaths, dcnt, dsw, ms = PL.plan3d_paths(p["x0"][:, :3], p["xF"][:, :3], device=dev)
    assert np.array_equal(dcnt, p["cnt"]), np.flatnonzero(dcnt != p["cnt"])
    for i in range(NPAIRS + 1):
        n = max(int(dcnt[i]), 0)
        assert np.array_equal(dpaths[i, :n].view(np.uint64), p["paths"][i, :n].view(np.uint64)), i
    assert (dsw[dcnt >= 3] >= 1).all() and dsw.max() < np.prod(K.DIMS)
    for N in (20, 60, 128):
        rc, exws, ecnt = K.emu_warm_start(p["x0"], p["xF"], N)
        xws, ok = PL.quad_warm_start_many(p["x0"], p["xF"], N, device=dev)
        assert rc == 0 and np.array_equal(ok, ecnt >= 2) and np.array_equal(xws.view(np.uint64), exws.view(np.uint64)), N
    print("kernel %.3f ms for %d plans; sweeps device mean %.1f max %d, sequential emulation mean %.1f max %d" % (ms, NPAIRS + 1, dsw.mean(), dsw.max(), p["sweeps"].mean(), p["sweeps"].max()))


def test_device_against_the_host_astar(dev, pool):
    p = pool
    dpaths, dcnt, _, _ = PL.plan3d_paths(p["x0"][:, :3], p["xF"][:, :3], device=dev)
    many = PL.astar3d_many(p["x0"][:, :3], p["xF"][:, :3], device=dev)
    host = K.host_paths(p["x0"], p["xF"]); n = 0
    for i in range(NPAIRS + 1):
        assert (host[i] is None) == (dcnt[i] in (0, -2)) == (many[i] is None), (i, dcnt[i])
        if host[i] is None:
            continue
        d = dpaths[i, :dcnt[i]]
        assert np.array_equal(d, many[i]), i
        K.assert_valid_path(d, p["x0"][i], p["xF"][i], what=i)
        tol = K.cost_tolerance(d, host[i])
        assert tol < 2e-4 and abs(K.chain_cost(d)[0] - K.chain_cost(host[i])[0]) <= tol, (i, K.chain_cost(d), K.chain_cost(host[i]), tol)
        n += 1
    assert n >= 200


def test_same_inputs_same_bits(dev, pool):
    from obca_amd import diag
    p = pool
    a = PL.plan3d_paths(p["x0"][:, :3], p["xF"][:, :3], device=dev); wa = PL.quad_warm_start_many(p["x0"], p["xF"], 60, device=dev)
    b = PL.plan3d_paths(p["x0"][:, :3], p["xF"][:, :3], device=dev); wb = PL.quad_warm_start_many(p["x0"], p["xF"], 60, device=dev)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1]) and np.array_equal(wa[0].view(np.uint64), wb[0].view(np.uint64))
    cover = diag.leave_pattern(0, mask=4)
    c = PL.plan3d_paths(p["x0"][:, :3], p["xF"][:, :3], device=dev)
    diag.leave_pattern(0, mask=4)
    wc = PL.quad_warm_start_many(p["x0"], p["xF"], 60, device=dev)
    assert np.array_equal(a[0].view(np.uint64), c[0].view(np.uint64)) and np.array_equal(a[1], c[1]), cover
    assert np.array_equal(wa[0].view(np.uint64), wc[0].view(np.uint64)) and np.array_equal(wa[1], wc[1]), cover


def test_a_batch_larger_than_the_machine(dev):
    """1 024 workgroups of 160 KB of LDS each: more than the CUs hold at once.  Instance i of the batch is instance i planned alone."""
    x0, xF = K.endpoints(1024, seed=99, shipped=False)
    paths, cnt, _, ms = PL.plan3d_paths(x0[:, :3], xF[:, :3], device=dev)
    assert (cnt >= 3).sum() >= 800 and not (cnt == -1).any() and not (cnt == -3).any()
    for i in list(range(0, 1024, 37)) + [1023]:
        p1, c1, _, _ = PL.plan3d_paths(x0[i:i + 1, :3], xF[i:i + 1, :3], device=dev)
        assert c1[0] == cnt[i] and np.array_equal(p1[0].view(np.uint64), paths[i].view(np.uint64)), i
    rc, ep, ec, _ = K.emu_paths(x0[:24, :3], xF[:24, :3])
    assert rc == 0 and np.array_equal(ec, cnt[:24]) and all(np.array_equal(ep[i, :max(ec[i], 0)], paths[i, :max(ec[i], 0)]) for i in range(24))
    print("1024 plans: kernel %.3f ms" % ms)


def test_statuses_and_per_instance_boxes_through_the_c_abi(dev):
    lib = PL._load3d(); h = PL.plan3d_context(dev)
    g = S.QUAD_XF[:3]
    # per-instance boxes: the batch gives what every instance gives alone, and what the emulation gives
    x0, xF = K.endpoints(5, seed=7)
    sets = [S.QUAD_OB, S.QUAD_OB[:1], S.QUAD_OB[1:], np.array([[5.5, 10, 5, -4.5, 0, -1.0]] * 5, float), S.QUAD_OB[[0, 0, 0, 0, 0]], S.QUAD_OB[::-1]]
    boxes = np.stack([np.asarray(s_, float).reshape(-1, 6)[np.arange(5) % len(s_)] for s_ in sets])
    paths, cnt, _, _ = PL.plan3d_paths(x0[:, :3], xF[:, :3], boxes=boxes, device=dev)
    rc, ep, ec, _ = K.emu_paths(x0[:, :3], xF[:, :3], boxes=boxes)
    assert rc == 0 and np.array_equal(cnt, ec) and np.array_equal(paths.view(np.uint64), ep.view(np.uint64))
    for i in range(len(x0)):
        p1, c1, _, _ = PL.plan3d_paths(x0[i:i + 1, :3], xF[i:i + 1, :3], boxes=boxes[i], device=dev)
        assert c1[0] == cnt[i] and np.array_equal(p1[0], paths[i]), i
    # -2: start inside the first wall; 0: a goal sealed by boxes; -1: cap too small -- in ONE batch, beside an instance that has a path
    shell = []
    lo, hi = np.array([4.0, 4.0, 1.5]), np.array([6.0, 6.0, 3.5])
    for ax in range(3):
        for side in (0, 1):
            a, b = lo.copy(), hi.copy()
            if side: a[ax] = hi[ax] - 0.1
            else: b[ax] = lo[ax] + 0.1
            shell.append(np.concatenate([b, -a]))
    shell = np.array(shell); wall = np.tile(S.QUAD_OB[:1], (6, 1))
    starts = np.array([[2.2, 5.0, 2.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]); goals = np.array([g, [5.0, 5.0, 2.5], [9.0, 9.0, 4.0], g])
    bx = np.stack([wall, shell, shell, wall])
    paths, cnt, _, _ = PL.plan3d_paths(starts, goals, boxes=bx, clear=0.3, device=dev)
    assert cnt[0] == -2 and cnt[1] == 0 and cnt[2] >= 3 and cnt[3] >= 3, cnt
    n = int(cnt[3])
    _, c2, _, _ = PL.plan3d_paths(starts, goals, boxes=bx, clear=0.3, device=dev, cap=n - 1)
    assert c2[0] == -2 and c2[1] == 0 and c2[3] == -1 and (c2[2] == cnt[2] or (cnt[2] > n - 1 and c2[2] == -1)), c2
    # beyond the limits: -1 from the call, with a message; the context stays usable
    with pytest.raises(PL.Plan3DError, match="MAXCELLS"):
        PL.plan3d_paths(starts, goals, boxes=bx, res=0.2, device=dev)
    with pytest.raises(PL.Plan3DError, match="nBox"):
        PL.plan3d_paths(starts[2:3], goals[2:3], boxes=np.tile(S.QUAD_OB[:1], (9, 1)), device=dev)
    with pytest.raises(PL.Plan3DError, match="NMAX"):
        PL.quad_warm_start_many(S.QUAD_X0, S.QUAD_XF, PL.PLAN3D_NMAX + 1, device=dev)
    with pytest.raises(PL.Plan3DError, match="cap"):
        PL.plan3d_paths(starts, goals, boxes=bx, device=dev, cap=1)
    cntb = np.zeros(1, np.int32); pth = np.zeros((1, 8, 3))
    assert lib.obca_plan3d_paths_batch(h, 0, K.dp(starts), K.dp(goals), 0, None, 0.4, K.dp(K.ROOM), 0.25, K.dp(pth), 8, K.ip(cntb), None) == -1
    assert lib.obca_plan3d_last_error(h)
    hb = C.c_void_p()
    assert lib.obca_plan3d_create(-1, C.byref(hb)) != 0 and not hb.value and lib.obca_plan3d_last_error(None)
    assert PL.astar3d_many([S.QUAD_X0[:3]], [g], device=dev)[0] is not None


def test_end_to_end_solves_from_the_device_planned_warm_starts(dev):
    """64 random pairs, N = 60: every instance that solves and validates from the host-planned warm start also does from the device-planned one (at most 2 of 64 excepted)"""
    import obca_amd as OA
    N, B = 60, 64
    x0, xF = K.endpoints(400, seed=64, shipped=False)
    xd, ok = PL.quad_warm_start_many(x0, xF, N, device=dev)
    keep = np.flatnonzero(ok)[:B]
    assert len(keep) == B
    x0, xF, xd = x0[keep], xF[keep], xd[keep]
    xh = np.stack([PL.quad_warm_start(x0[i], xF[i], N) for i in range(B)])
    ctx = OA.Context(0); good = {}
    for name, xws in (("host", xh), ("device", xd)):
        qb = OA.QuadBatch(ctx, B, N)
        qb.upload(x0, xF, S.quad_sample_time(N), S.QUAD_R, S.QUAD_OB, xws, 1.0)
        qb.solve(opts=OA.quadcopter_ipopt_opts())
        out = qb.download(); v = qb.validate()
        good[name] = (out["exitflag"] == 1) & v["ok"]; good[name + "_iters"] = out["iters"]; good[name + "_ms"] = qb.kernel_ms()
        qb.close()
    ctx.close()
    lost = np.flatnonzero(good["host"] & ~good["device"])
    print("solved and valid: host-planned %d, device-planned %d of %d; mean iterations %.1f / %.1f; lost %s" % (good["host"].sum(), good["device"].sum(), B, good["host_iters"].mean(), good["device_iters"].mean(), lost.tolist()))
    if os.environ.get("OBCA_PLAN3D_E2E_JSON"):      # (a file for profiles/: the counts, and the end points of the exceptions if there are any)
        json.dump(dict(B=B, N=N, host_ok=int(good["host"].sum()), device_ok=int(good["device"].sum()), lost=lost.tolist(), lost_endpoints=[(x0[i, :3].tolist(), xF[i, :3].tolist()) for i in lost],
                       mean_iters_host=float(good["host_iters"].mean()), mean_iters_device=float(good["device_iters"].mean()), ipm_ms_host=good["host_ms"], ipm_ms_device=good["device_ms"]),
                  open(os.environ["OBCA_PLAN3D_E2E_JSON"], "w"), indent=1)
    assert good["host"].sum() >= B // 2
    assert len(lost) <= 2, "instances that solve and validate from the host-planned warm start but not from the device-planned one: %s" % [(int(i), x0[i, :3].tolist(), xF[i, :3].tolist()) for i in lost]


def test_device_planning_costs_less_than_the_host_loop(dev, pool):
    """both measured here, on the same box: the whole device call (packing, transfers, kernel) against the host loop of plan_quad_batch for the same batch.
    No margin: the host needs seconds, the assertion catches a device path that silently serialises.  It is not a speed claim."""
    p = pool; has = p["cnt"] >= 3; N = 60
    x0, xF = p["x0"][has].copy(), p["xF"][has].copy()
    S.plan_quad_batch(x0.copy(), xF.copy(), N, np.random.default_rng(0), device=dev)      # (context, buffers)
    t = time.perf_counter(); wd = S.plan_quad_batch(x0.copy(), xF.copy(), N, np.random.default_rng(0), device=dev); t_dev = time.perf_counter() - t
    t = time.perf_counter(); wh = S.plan_quad_batch(x0.copy(), xF.copy(), N, np.random.default_rng(0)); t_host = time.perf_counter() - t
    print("planning %d instances: device call %.4f s, host loop %.4f s" % (len(x0), t_dev, t_host))
    assert wd.shape == wh.shape and np.array_equal(wd[:, 0, :3], wh[:, 0, :3])
    assert t_dev < t_host, (t_dev, t_host)
