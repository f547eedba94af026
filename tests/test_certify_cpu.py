"""Clearance certificate (obca_amd/csrc/obca_certify.h): the speed bound behind it on random bicycle steps; the kernel text compiled for the host
(tests/emu/certify_emu.cpp) against the numpy statement (obca_amd/validate.py: certify_parking / certify_quad / certify_record) and against a dense sampling of the same
path, on the solved trajectories of tests/golden/, on synthetic parking trajectories at N = 1, 2, 3 and on the solved quadcopter states; the two cases in which a sampling is
clean and the certificate is not; order independence, non-finite input, the edges of the advancement, refusals; the public surface, the Julia shim and the build rule.
No GPU.  Cases, comparison rules and tolerances: tests/certify_common.py."""
import inspect
import math
import os
import re
import numpy as np
import pytest
from conftest import ROOT
import certify_common as K
from obca_amd import scenarios as S, validate as V

G = V.CERT_TICKS
PARKING = [("golden", "corridor_sd"), ("golden", "corridor_dist"), ("golden", "backwards30")] + [("synthetic", kind, N) for N in (1, 2, 3) for kind in K.SYNTHETIC]
QUADS = [("golden", i, N) for i, N in ((0, 20), (1, 20), (2, 20), (3, 20), (0, 1), (1, 3))] + [("slip",)]


def parking_case(case):
    return K.golden_parking(case[1]) if case[0] == "golden" else K.synthetic_parking(case[1], case[2])


def quad_case(case):
    if case[0] == "slip":
        return K.slip_quad()
    c = K.golden_quads()[case[1]]
    return c if case[2] == 20 else K.cut_quad(c, case[2])


def case_id(case):
    return "-".join(str(v) for v in case)


# ---------------------------------------------------------------- 1. the bound
def test_speed_bound_holds_on_random_bicycle_steps_and_host_build_agrees():
    """12 000 random (x, u, h in [0.05, 2], tau0, tau1) with the shipped car: no corner of the record's rectangle moves farther than Lambda |tau1 - tau0|; the host build's
    Lambda is numpy's to the last bit, or within 4 ulp where libm's tan is not numpy's"""
    import polygon_distance as PD
    rng = np.random.default_rng(20261021); ego, L = S.EGO, S.L_WHEELBASE
    g, off = V._geom(ego); gg = np.ascontiguousarray(g, float)
    worst = 0.0; n_bits = 0; n = 12000
    for _ in range(n):
        x = np.array([rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(-np.pi, np.pi), rng.uniform(-2, 2)])
        u = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-1, 1)]); h = rng.uniform(0.05, 2.0)
        if rng.uniform() < 0.1:
            x[3] = 0.0 if rng.uniform() < 0.5 else x[3]; u[1] = 0.0 if rng.uniform() < 0.5 else u[1]      # (the edges: at rest, no acceleration)
        t0, t1 = rng.uniform(0, h, 2)
        lam = V.certify_lipschitz_parking(x, u, h, L, ego)
        p0 = V._dyn(x, u, t0, 1.0, L); p1 = V._dyn(x, u, t1, 1.0, L)      # (Ts = 1: the step length is tau itself)
        move = np.hypot(*(PD.car_rectangle(p1[0], p1[1], p1[2], ego) - PD.car_rectangle(p0[0], p0[1], p0[2], ego)).T).max()
        assert move <= lam * abs(t1 - t0) * (1 + 1e-12), (x, u, h, t0, t1, move, lam)
        if abs(t1 - t0) > 1e-3 * h and lam > 0:
            worst = max(worst, move / (lam * abs(t1 - t0)))
        host = K.emu().emu_certify_lipschitz_parking(K.dp(x), K.dp(u), h, L, off, K.dp(gg))
        n_bits += host == lam
        assert host == lam or abs(host - lam) <= 4 * np.spacing(lam), (host, lam)
    assert 0.9 < worst <= 1.0 and n_bits >= 0.99 * n, (worst, n_bits)      # nearly tight (the issue measured 0.996), and bits but for a tan here and there


def test_quadcopter_speed_bound_is_the_velocity_norm():
    rng = np.random.default_rng(3)
    for _ in range(200):
        xk = rng.normal(size=12) * 3
        lam = V.certify_lipschitz_quad(xk)
        assert lam == math.sqrt((xk[6] * xk[6] + xk[7] * xk[7]) + xk[8] * xk[8]) == K.emu().emu_certify_lipschitz_quad(K.dp(xk))
        assert abs(lam - np.linalg.norm(xk[6:9])) <= 2 * np.spacing(lam)
    xk = np.zeros(12); xk[6:9] = [3.0, 4.0, 12.0]
    assert V.certify_lipschitz_quad(xk) == 13.0 == K.emu().emu_certify_lipschitz_quad(K.dp(xk))


# ---------------------------------------------------------------- 2. invariants
def _check_items(items, ref, what):
    """the host build's item table against the statement's (given the host build's own distances): ticks and counts equal, values within 1e-9"""
    assert np.array_equal(items[:, :, 2:], ref[:, :, 2:]), (what, np.argwhere(items[:, :, 2:] != ref[:, :, 2:])[:5])
    for i in (0, 1):
        a, b = items[:, :, i], ref[:, :, i]; inf = np.isinf(b)
        assert np.array_equal(a[inf], b[inf]) and (np.abs(a[~inf] - b[~inf]) <= K.TOL_PARK * np.maximum(1.0, np.abs(b[~inf]))).all(), (what, i)


@pytest.mark.parametrize("case", PARKING, ids=case_id)
def test_parking_host_build_keeps_the_guarantees_and_matches_the_statement(case):
    c = parking_case(case); dense = K.dense_parking(c); dist = K.host_distance(c)
    for need, slack in ((V.DMIN, 0.01), (0.02, 0.002), (0.3, 0.05)):
        what = "%s need %g slack %g" % (c["name"], need, slack)
        rec, iv, items = K.emu_parking(c, need, slack)
        K.check_invariants(rec, iv, need, slack, float(dense.min()), what)
        # per interval too: the bound of interval k lies under the dense samples of interval k (node N: its one sample)
        per = np.r_[[dense[k * K.DENSE:(k + 1) * K.DENSE].min() for k in range(c["N"])], dense[-1].min()]
        assert (iv[:, 0] <= per + K.TOL_DENSE).all() and (np.minimum(need, iv[:, 1]) - slack <= iv[:, 0] + 1e-15).all() and (iv[:, 0] <= iv[:, 1]).all(), what
        assert iv[-1, 0] == iv[-1, 1] == dense[-1].min(), what      # (node N is one sample: bound and sample coincide)
        # every violation the items report, re-evaluated at its (interval, tick, obstacle), lies under need; so does the record's first one
        viol = [(k, int(items[k, j, 3]), j) for k in range(c["N"] + 1) for j in range(len(c["vOb"])) if items[k, j, 3] < G]
        for k, m, j in viol:
            d = dist(K.pose_at(c, k, m) if k < c["N"] else c["x"][:3, k], j)
            assert (0.0 if d < V.CLR_TOUCH else d) < need, (what, k, m, j, d)
        assert tuple(rec[6:9]) == (min(viol) if viol else (-1, -1, -1)) and rec[5] == len({k for k, _, _ in viol}), what
        # a sample at tick 0 is the node itself, bit for bit
        for k, j in zip(*np.nonzero(items[:, :, 2] == 0)):
            d = dist(c["x"][:3, k], int(j))
            assert items[k, j, 1] == (0.0 if d < V.CLR_TOUCH else d), what
        assert rec[10] == items[:, :, 4].sum() and rec[11] == items[:, :, 4].max() and (items[-1, :, 4] == 1).all(), what
        # the statement, given the host build's own distances
        want, wiv, witems, lam = K.ref_parking(c, need, slack, dist=dist)
        _check_items(items, witems, what)
        assert np.array_equal(rec[2:12], want[2:12]) and np.array_equal(rec[13:], want[13:]) and abs(rec[12] - want[12]) <= 4 * np.spacing(want[12]), (what, rec, want)
        assert np.abs(rec[:2] - want[:2]).max() <= K.TOL_PARK and np.abs(iv - wiv).max() <= K.TOL_PARK, what
        if np.ptp(c["ts"]) == 0:      # one t, as a resident batch holds it: the same bits
            r2, iv2, it2 = K.emu_parking(c, need, slack, resident=True)
            assert np.array_equal(r2, rec) and np.array_equal(iv2, iv) and np.array_equal(it2, items), what


@pytest.mark.parametrize("case", QUADS, ids=case_id)
def test_quadcopter_host_build_keeps_the_guarantees_and_is_the_statement_bit_for_bit(case):
    c = quad_case(case); dense = K.dense_quad(c)
    for need, slack in ((0.0, 0.01), (0.03, 0.005), (-0.3, 0.05)):
        what = "%s need %g slack %g" % (c["name"], need, slack)
        rec, iv, items = K.emu_quad(c, need, slack)
        K.check_invariants(rec, iv, need, slack, dense, what)
        want, wiv, witems, lam = K.ref_quad(c, need, slack)
        assert np.array_equal(rec, want) and np.array_equal(iv, wiv) and np.array_equal(items, witems), (what, rec, want)
        assert rec[12] == max(V.certify_lipschitz_quad(c["x"][:, k]) for k in range(c["N"])), what
        # every reported violation re-evaluated
        for k, j in zip(*np.nonzero(items[:, :, 3] < G)):
            m = int(items[k, j, 3]); pt = c["x"][:3, k] + m / G * c["ts"][k] * c["Ts"] * c["x"][6:9, k] if m else c["x"][:3, k]
            assert V.quad_point_clearance(pt[None], c["ob"], c["R"])[0, j] < need, (what, k, m, j)


def test_statement_takes_any_distance_exact_polygon_distance():
    """the statement with the exact distance of the rectangle to the polygon (tests/polygon_distance.py) keeps the same guarantees against the same dense sampling"""
    c = K.synthetic_parking("reverse", 3); dense = K.dense_parking(c)
    rec, iv, items, lam = K.ref_parking(c, V.DMIN, 0.01, dist=K.polygon_distance(c))
    K.check_invariants(rec, iv, V.DMIN, 0.01, float(dense.min()), "polygon distance")
    host = K.emu_parking(c)[0]
    assert rec[13] == host[13] == 1 and abs(rec[1] - host[1]) <= 1e-3 and np.array_equal(lam, K.ref_parking(c)[3])


# ---------------------------------------------------------------- 3. sampling misses what the certificate finds
@pytest.mark.parametrize("name", ["corridor_sd", "corridor_dist"])
def test_corridor_instance_is_clean_at_its_nodes_and_violated_in_interval_13(name):
    """make_corridor_batch(8, 80, seed=11, clearance=(0.0, 0.2)) instance 1, solved by the oracle: 0.0551 / 0.0502 at every node, contact at sub-step 2 of interval 13"""
    c = K.golden_parking(name); nodes = K.dense_parking(c)[::K.DENSE]
    assert nodes.shape[0] == c["N"] + 1 and nodes.min() >= 0.05 and int((nodes.min(axis=1) < 0.05).sum()) == 0      # the node-only sampling at need = 0.05: nothing below
    rec, iv, items = K.emu_parking(c, 0.05, 0.01)
    assert rec[14] == 0 and rec[13] == 0 and rec[5] >= 1 and rec[9] == 0
    assert rec[6] == 13 and rec[8] == 3 and iv[13, 1] == 0.0 and rec[1] == 0.0 and (rec[2], rec[4]) == (13, 3)      # the wedge is touched: clearance 0
    assert 0 < rec[7] <= rec[3] and G // 8 < rec[3] < 3 * G // 8      # under 0.05 only after the node; the contact lies about sub-step 2 of 8, between the samples 1 and 3
    assert (iv[:13, 1] >= 0.05).all() and rec[0] <= 0.0


def test_quadcopter_slips_past_a_box_between_two_samples():
    """issue 3(b): the 8-sub-step samples at x = 1.0 and 1.25 keep 0.0379, the path comes to 0.02 between them"""
    c = K.slip_quad()
    assert abs(math.sqrt(0.01 + 0.0729) - 0.25 - 0.0379) < 1e-4
    clr = V.quad_clearance(c["x"], c["ts"], c["Ts"], c["ob"], c["R"], 8, need=0.03)
    assert clr[4] == 0 and abs(clr[0] - 0.0379) < 1e-4 and clr[6] == 0      # below == 0: the sampling is clean
    assert abs(K.dense_quad(c) - 0.02) < 1e-12
    rec, iv, items = K.emu_quad(c, 0.03, 0.005)
    assert rec[14] == 0 and rec[13] == 0 and rec[5] == 1 and tuple(rec[6:9])[::2] == (0, 0) and rec[1] < 0.03 and abs(rec[1] - 0.02) < 1e-12
    assert 1.0 / 2.0 * G < rec[7] < 1.25 / 2.0 * G and rec[2] == 0 and rec[4] == 0      # between the samples at x = 1.0 and 1.25 of the interval's 2.0
    assert iv[0, 1] == rec[1] and (iv[1:, 1] > 0.5).all()      # (the later nodes see the same box from 0.64 and 2.6 away)
    ok = K.emu_quad(c, 0.015, 0.005)[0]      # and a need the path does keep is certified: >= 0.01 everywhere
    assert ok[13] == 1 and ok[0] >= 0.01


# ---------------------------------------------------------------- 4. order and edges
def test_record_does_not_depend_on_how_items_are_dealt_to_the_lanes():
    for c in (K.golden_parking("corridor_sd"), K.golden_parking("backwards30"), K.synthetic_parking("turn", 3)):      # 405 and 93 items: several rounds; 12: one
        a = K.emu_parking(c, V.DMIN, 0.01); b = K.emu_parking(c, V.DMIN, 0.01, rev=1)
        assert all(np.array_equal(p, q) for p, q in zip(a, b)), c["name"]
    for c in (K.golden_quads()[1], K.slip_quad()):
        a = K.emu_quad(c, 0.0, 0.01); b = K.emu_quad(c, 0.0, 0.01, rev=1)
        assert all(np.array_equal(p, q) for p, q in zip(a, b)), c["name"]
    c = K.golden_parking("backwards30")      # ... and the row class of a wider batch gives the same indices
    a, b = K.emu_parking(c, vmax=2)[0], K.emu_parking(c, vmax=8)[0]
    assert np.array_equal(a[2:12], b[2:12]) and np.abs(a[:2] - b[:2]).max() <= K.TOL_PARK


def test_non_finite_input_marks_the_instance():
    c = K.synthetic_parking("turn", 3); nOb = len(c["vOb"])
    want, wiv = V.certify_record(np.zeros((4, nOb, 5)), np.zeros(3), finite=False)
    assert want[14] == 1 and want[13] == 0 and want[5] == 4 and want[9] == 4 * nOb and np.isnan(want[[0, 1, 12]]).all() and (want[[2, 3, 4, 6, 7, 8]] == -1).all()
    for field, idx, v in (("x", (2, 1), np.nan), ("x", (0, 3), np.inf), ("u", (1, 2), np.nan), ("ts", (1,), -np.inf), ("Ts", None, np.nan)):
        bad = dict(c, **{field: v if idx is None else c[field].copy()})
        if idx is not None:
            bad[field][idx] = v
        rec, iv, _ = K.emu_parking(bad)
        assert np.array_equal(rec, want, equal_nan=True) and np.isnan(iv).all(), (field, rec)
    assert K.emu_parking(c)[0][14] == 0      # the trajectory itself is fine
    q = K.cut_quad(K.golden_quads()[0], 3); want, _ = V.certify_record(np.zeros((4, 5, 5)), np.zeros(3), finite=False)
    for field, idx, v in (("x", (7, 1), np.nan), ("x", (11, 3), np.inf), ("ts", (2,), np.nan)):
        bad = dict(q, **{field: q[field].copy()}); bad[field][idx] = v
        rec, iv, _ = K.emu_quad(bad)
        assert np.array_equal(rec, want, equal_nan=True) and np.isnan(iv).all(), (field, rec)
    big = dict(q, x=q["x"].copy()); big["x"][6, 1] = 1e200      # finite input, a clearance that is not: the same mark
    big["x"][0, 1] = 1e200
    rec, iv, _ = K.emu_quad(big)
    assert rec[14] == 1 and np.isnan(iv).all()
    st = V.certify_record(*V.certify_quad(big["x"], big["ts"], big["Ts"], big["ob"], big["R"]))
    assert np.array_equal(rec, st[0], equal_nan=True)


def test_a_vehicle_at_rest_takes_one_sample_per_item():
    for N in (1, 2, 3):
        c = K.synthetic_parking("rest", N); nOb = len(c["vOb"])
        rec, iv, items = K.emu_parking(c, V.DMIN, 1e-6)
        assert rec[12] == 0 and rec[10] == (N + 1) * nOb and rec[11] == 1 and rec[13] == 1 and rec[0] == rec[1] and np.array_equal(iv[:, 0], iv[:, 1])
    q = K.cut_quad(K.golden_quads()[0], 2); q = dict(q, x=q["x"].copy()); q["x"][6:9] = 0.0
    rec, iv, items = K.emu_quad(q, -1.0, 1e-6)
    assert rec[12] == 0 and rec[10] == 15 and rec[11] == 1 and np.array_equal(iv[:, 0], iv[:, 1])


def test_running_out_of_steps_leaves_the_item_undecided():
    c = K.synthetic_parking("straight", 2)      # 0.15 over the wedges at speed 1: several samples per near item
    full = K.emu_parking(c, V.DMIN, 0.01)[0]
    assert full[13] == 1 and full[11] > 1
    rec, iv, items = K.emu_parking(c, V.DMIN, 0.01, max_steps=1)
    assert rec[9] > 0 and rec[0] == -np.inf and rec[13] == 0 and rec[14] == 0 and rec[5] == 0 and rec[11] == 1
    assert rec[9] == (items[:, :, 0] == -np.inf).sum() and (iv[:, 0] == -np.inf).any() and np.isfinite(iv[-1]).all()
    want = K.ref_parking(c, V.DMIN, 0.01, max_steps=1)[0]
    assert np.array_equal(rec[2:], want[2:]) and rec[0] == want[0]
    exact = K.emu_parking(c, V.DMIN, 0.01, max_steps=int(full[11]))[0]      # as many steps as the longest item needs: decided, the same record
    assert np.array_equal(exact, full)
    assert K.emu_parking(c, V.DMIN, 0.01, max_steps=int(full[11]) - 1)[0][9] >= 1


def test_a_floor_of_zero_advances_one_tick():
    """slack so small that floor(G e / (Lambda |h|)) is 0 and `need` above every clearance: the walk goes tick by tick, G samples per moving item, and is decided at
    max_steps = G alone"""
    c = K.cut_quad(K.slip_quad(), 1)
    rec, iv, items = K.emu_quad(c, 1e3, 1e-9)
    assert (items[0, :, 4] == G).all() and (items[1, :, 4] == 1).all() and rec[11] == G and rec[9] == 0 and rec[5] == 2 and rec[13] == 0
    Lh = 4.0 * 0.5
    assert (items[0, :, 0] >= items[0, :, 1] - Lh / G - 1e-15).all() and (items[0, :, 0] <= items[0, :, 1]).all()
    assert abs(rec[1] - 0.02) < 1e-3      # the uniform sampling at spacing |h| / G sees the box it passes: the true minimum is 0.02
    want = K.ref_quad(c, 1e3, 1e-9)
    assert np.array_equal(rec, want[0]) and np.array_equal(items, want[2])
    short = K.emu_quad(c, 1e3, 1e-9, max_steps=G - 1)[0]
    assert short[9] == 5 and short[0] == -np.inf


def test_every_refusal_names_its_argument():
    lib = K.emu()
    txt = lambda *a: lib.emu_certify_check_args(*a).decode()
    assert txt(0.05, 0.01, G) == "" and txt(-3.0, 1e-300, 1) == ""
    for need in (np.nan, np.inf, -np.inf):
        assert "`need`" in txt(need, 0.01, 10)
    for slack in (0.0, -0.01, np.nan, np.inf):
        assert "`slack`" in txt(0.05, slack, 10)
    for ms in (0, -1, G + 1):
        assert "max_steps" in txt(0.05, 0.01, ms) and str(G) in txt(0.05, 0.01, ms)
    c = K.synthetic_parking("rest", 1); N = 1; nOb = len(c["vOb"])
    prob = K._park_prob(c); z = np.zeros(K.P.layout(N, nOb, int(c["vOb"].sum()))["len"]); out = np.zeros(16); iv = np.zeros(4)
    assert lib.emu_certify_parking(N, K.dp(prob), K.dp(z), None, 2, 0.05, 0.0, 10, 0, K.dp(iv), K.dp(out), None) == -1 and b"slack" in lib.emu_certify_last_error()
    assert lib.emu_certify_parking(0, K.dp(prob), K.dp(z), None, 2, 0.05, 0.01, 10, 0, K.dp(iv), K.dp(out), None) == -1 and b"N" in lib.emu_certify_last_error()
    q = K.slip_quad()
    assert lib.emu_certify_quad(2, K.dp(K._quad_prob(q)), K.dp(np.ascontiguousarray(q["x"].T)), K.dp(q["ts"]), 1, np.nan, 0.01, 10, 0, K.dp(np.zeros(6)), K.dp(out), None) == -1
    assert b"need" in lib.emu_certify_last_error()
    # the library's entry points use the same text
    hip = open(os.path.join(ROOT, "obca_amd", "csrc", "obca_hip.hip")).read()
    assert hip.count("cert::certify_check_args(need, slack, max_steps)") == 4


# ---------------------------------------------------------------- 5. shim and build
def test_header_exports_python_and_julia_agree():
    from obca_amd import api, cabi
    import obca_amd
    import test_hybrid_cpu as TH
    import test_julia_shim_cpu as J
    protos = cabi.prototypes("obca_certify.h")
    assert sorted(protos) == sorted(api.CERTIFY_EXPORTS) and len(protos) == 8 and "obca_certify.h" in cabi.__doc__
    others = [getattr(api, n) for n in dir(api) if n.endswith("EXPORTS") and n != "CERTIFY_EXPORTS"]
    assert not set(api.CERTIFY_EXPORTS) & {e for lst in others for e in lst}
    assert len(protos["obca_batch_certify"][1]) == 5 and len(protos["obca_parking_certify_batch"][1]) == 18 and len(protos["obca_quadcopter_certify_batch"][1]) == 13
    src_api = inspect.getsource(api._load)
    assert 'cabi.bind(_lib, "obca_certify.h")' in src_api
    hdr = open(os.path.join(ROOT, "include", "obca_certify.h")).read()
    assert re.search(r"#define OBCA_CERT_OUT 16\b", hdr) and re.search(r"#define OBCA_CERT_TICKS 4096\b", hdr)
    txt = open(os.path.join(ROOT, "obca_amd", "csrc", "obca_certify.h")).read()
    assert re.search(r"#define CT_OUT 16\b", txt) and re.search(r"#define CT_TICKS 4096\b", txt) and (V.CERT_OUT, V.CERT_TICKS) == (16, 4096)
    for f_ in ("parking_certify_batch", "quadcopter_certify_batch"):
        assert hasattr(obca_amd, f_) and f_ in obca_amd.__all__
    for cls, need in ((obca_amd.Batch, V.DMIN), (obca_amd.QuadBatch, 0.0)):
        sig = inspect.signature(cls.certify).parameters
        assert list(sig) == ["self", "need", "slack", "max_steps"] and [sig[n].default for n in list(sig)[1:]] == [need, 0.01, 4096]
        assert all(callable(getattr(cls, m)) for m in ("certify_intervals", "certify_ms")) and "certify_intervals" in vars(api._DeviceBatch)
    for fn, need in ((obca_amd.parking_certify_batch, V.DMIN), (obca_amd.quadcopter_certify_batch, 0.0)):
        sig = inspect.signature(fn).parameters
        assert sig["need"].default == need and sig["slack"].default == 0.01 and sig["max_steps"].default == 4096
    d = api._certify_dict(np.arange(32.0).reshape(2, 16))
    assert set(d) == {"lb", "seen", "interval", "tick", "obstacle", "violated", "first_violation", "undecided", "samples", "samples_max", "lipschitz", "certified", "finite"}
    assert d["first_violation"].shape == (2, 3) and d["certified"].dtype == bool and d["finite"].tolist() == [False, False] and d["tick"].tolist() == [3, 19]
    # every ccall of the shim against the header, parameter by parameter; a library constant of its own
    kinds = TH._kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCACertify.jl")).read()
    assert re.search(r"^const CERT = LIB$", src, flags=re.M) and re.search(r"^const OUT = 16\b", src, flags=re.M) and re.search(r"^const TICKS = 4096\b", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), CERT\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
        assert m.group(2) == "Cint"
    assert {n for n, _ in calls} == set(kinds) == set(api.CERTIFY_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])
    assert src.count("ccall(") == len(calls) + 1 and "ccall((:obca_last_error, LIB)" in src


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu"); name = "certify_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_certify_emu.so")
    deps = {os.path.realpath(d) for d in BF.dependencies(p.sources)}
    todo = [os.path.realpath(s) for s in p.sources]; seen = set()
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        assert f in deps, f
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', open(f).read(), flags=re.M):
            assert os.path.exists(os.path.join(os.path.dirname(f), inc)), (f, inc)
            todo.append(os.path.realpath(os.path.join(os.path.dirname(f), inc)))
    csrc = os.path.join(ROOT, "obca_amd", "csrc")
    for h in ("obca_certify.h", "obca_clearance.h", "obca_validate.h", "obca_quad_model.h", "obca_model.h"):
        assert os.path.realpath(os.path.join(csrc, h)) in seen, h
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_certify_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/certify_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # nothing in csrc includes the kernel text but the one line of the library, behind the clearance text it asks for (tests/test_clearance_cpu.py lets no other header name that one)
    for f in os.listdir(csrc):
        if f.endswith((".h", ".hip", ".cpp")) and f != "obca_hip.hip":
            assert not re.search(r'#\s*include\s*"obca_certify.h"', open(os.path.join(csrc, f)).read()), f
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    assert hip.count('#include "obca_certify.h"') == 1 and hip.count('#include "../../include/obca_certify.h"') == 1
    txt = re.sub(r"//.*", "", open(os.path.join(csrc, "obca_certify.h")).read())
    assert re.findall(r'#include\s*"([^"]+)"', txt) == ["obca_validate.h"] and '#error "include the clearance check' in txt
    assert hip.index('#include "obca_clearance.h"') < hip.index('#include "obca_certify.h"')
    # no atomics; the distances are the clearance call's own
    assert "atomic" not in txt and "dualws_one<VM>" in txt and "val::park_step" in txt and "clr::cl_item" in txt and txt.count("clr::cl_keep") >= 10
