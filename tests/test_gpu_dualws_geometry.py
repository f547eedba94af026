"""DualMultWS and the clearance record on the device against exact polygon geometry (tests/polygon_distance.py, tests/golden/dualws_polygons.npz): what
tests/test_dualws_geometry_cpu.py asks of the oracle and the host build, asked of obca_dualws_kernel<2 / 4 / 8> and of the clearance kernels.  The device forms its
reciprocals with v_rcp_f64 + one correction where the host divides, so its pass count on a problem near the cap of dualws_one need not be the host's: only geometry can
tell whether its answer is right.

Tolerances: |d - d_exact| <= 2e-8 and -2e-8 <= d (the duality gap the stopping rule leaves, see the CPU file), the certificate bounds of polygon_distance.certificate, and
1e-9 between device and host build (the bound of tests/test_gpu_parity.py).  The clearance record clamps below CL_TOUCH = 1e-7: every exact gap the tests use lies outside
(8e-8, 1.2e-7), so the clamp of a value known to 2e-8 is never in doubt."""
import numpy as np
import pytest
from conftest import golden
from obca_amd import scenarios as S, validate as V
import polygon_distance as PD
from test_dualws_geometry_cpu import run_host_build, TOL_D

pytestmark = pytest.mark.gpu
N_POSES = 6
M_MAX = 64      # OBCA_MMAX of include/obca_hip.h: half-space rows per instance
# cases that ran into the cap of the first attempt on the CPU: the second attempt runs on the device in the 4-row and in the 8-row kernel
HARD4 = ("wedge_9.8cm", "stretched_n3_a0.05_gap40_unit", "stretched_n4_a0.05_gap10_edge", "stretched_n4_a0.05_gap40_unit")
HARD8 = ("wedge_82cm", "stretched_n5_a0.05_gap40_edge", "stretched_n6_a0.05_gap40_unit", "stretched_n7_a0.05_gap10_unit", "stretched_n7_a0.05_gap40_edge")


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.Context(0).close()      # fails loudly if the HIP library / device is missing
    return obca_amd


@pytest.fixture(scope="module")
def cases():
    g = golden("dualws_polygons.npz")
    return {k: g[k] for k in g.files}


def pick(g, rng, rows, count, first, every):
    """`count` case indices whose obstacles have at most rows[-1] rows, the named ones first; every: each number of `rows` is present"""
    idx = [int(np.flatnonzero(g["name"] == n)[0]) for n in first]
    assert all(int(g["v"][i]) <= rows[-1] for i in idx)
    for r in rows if every else ():
        if not any(int(g["v"][i]) == r for i in idx):
            idx.append(int(rng.choice(np.flatnonzero(g["v"] == r))))
    while len(idx) < count:      # at most M_MAX rows in an instance: the next one leaves a row for each of those still to come
        room = M_MAX - sum(int(g["v"][i]) for i in idx) - (count - len(idx) - 1)
        pool = np.setdiff1d(np.flatnonzero(g["v"] <= min(rows[-1], room)), idx)
        idx.append(int(rng.choice(pool)))
    assert len(idx) == count and sum(int(g["v"][i]) for i in idx) <= M_MAX
    return idx


def make_batch(g, rows, first, seed):
    """three instances of 1, 3 and 16 obstacles with N_POSES poses each: obstacle j is that of fixture case idx[j], pose k that of case idx[k mod nOb]; so the pairs
    (k, j = k mod nOb) are fixture cases and the others further (pose, obstacle) problems of the same kind.  The 16 hold every width of `rows` (and others up to the widest): padded rows in one instance."""
    rng = np.random.default_rng(seed); inst = []
    for nOb, named in ((1, first[:1]), (3, first[1:2]), (16, first)):
        idx = pick(g, rng, rows, nOb, named, nOb == 16)
        inst.append(dict(idx=idx, v=[int(g["v"][i]) for i in idx], A=np.concatenate([g["A"][i, :g["v"][i]] for i in idx]), b=np.concatenate([g["b"][i, :g["v"][i]] for i in idx]),
                         pose=np.array([g["pose"][idx[k % nOb]] for k in range(N_POSES)])))
    assert set(inst[2]["v"]) >= set(rows)
    return inst


@pytest.mark.parametrize("rows,first", [((1, 2), ()), ((1, 3, 4), HARD4), ((3, 5, 8), HARD8)], ids=["widest_2", "widest_4", "widest_8"])
def test_dualmult_ws_batch_against_polygon_geometry(OA, emu, cases, rows, first):
    g = cases; ego = g["ego"]; inst = make_batch(g, rows, first, 7 + rows[-1]); B = len(inst); N = N_POSES - 1
    assert max(max(c["v"]) for c in inst) == rows[-1] and (B * (N + 1) * 16) % 256 != 0 and B * (N + 1) * 16 > 256
    ls, ns, ds = OA.dualmult_ws_batch(N, [c["v"] for c in inst], [c["A"] for c in inst], [c["b"] for c in inst],
                                      np.stack([c["pose"][:, 0] for c in inst]), np.stack([c["pose"][:, 1] for c in inst]), np.stack([c["pose"][:, 2] for c in inst]), ego)
    bad = []; worst = dict(geometry=0.0, host_build=0.0); n = 0
    for i, c in enumerate(inst):
        nOb = len(c["v"]); r0 = np.r_[0, np.cumsum(c["v"])]
        assert ls[i].shape == (N + 1, r0[-1]) and ns[i].shape == (N + 1, 4 * nOb) and ds[i].shape == (N + 1, nOb)
        for k in range(N + 1):
            X, Y, psi = c["pose"][k]
            for j in range(nOb):
                A, b = c["A"][r0[j]:r0[j + 1]], c["b"][r0[j]:r0[j + 1]]; what = "instance %d pose %d obstacle %d (%s)" % (i, k, j, g["name"][c["idx"][j]]); n += 1
                dx = PD.polygon_distance(X, Y, psi, ego, A, b)
                if j == k % nOb:
                    assert abs(dx - g["d"][c["idx"][j]]) <= 1e-13 * max(1.0, dx), what      # the fixture's own case
                d = ds[i][k, j]; lam = ls[i][k, r0[j]:r0[j + 1]]; mu = ns[i][k, 4 * j:4 * j + 4]
                worst["geometry"] = max(worst["geometry"], abs(d - dx))
                if not (np.isfinite(d) and d >= -TOL_D and abs(d - dx) <= TOL_D):
                    bad.append("%s: d = %.12g, exact %.12g" % (what, d, dx)); continue
                cert = PD.certificate(X, Y, psi, ego, A, b, lam, mu, d)
                if not PD.certificate_ok(cert):
                    bad.append("%s: certificate %s" % (what, cert))
                dh = run_host_build(emu, X, Y, psi, ego, A, b)[2]
                worst["host_build"] = max(worst["host_build"], abs(d - dh))
                if abs(d - dh) >= 1e-9:
                    bad.append("%s: d = %.12g, host build %.12g" % (what, d, dh))
    print("%d sub-problems, widest obstacle %d: largest |d - exact| %.3g, largest |d - host build| %.3g" % (n, rows[-1], worst["geometry"], worst["host_build"]))
    assert not bad, "%d of %d sub-problems fail:\n  %s" % (len(bad), n, "\n  ".join(bad))


# ---------------------------------------------------------------- the clearance record beside the named wedge and a touching box
def wedge(g):
    w = int(np.flatnonzero(g["name"] == "wedge_9.8cm")[0])
    return g["A"][w, :3], g["b"][w, :3], g["pose"][w]


def drive(pose, N, Ts, speed=0.8, u=(0.05, 0.1)):
    """x (4, N + 1), u (2, N): from the pose, N steps of the discretisation's own dynamics"""
    x = np.zeros((4, N + 1)); x[:, 0] = (*pose, speed); uu = np.tile(np.array(u, float)[:, None], (1, N))
    for k in range(N):
        x[:, k + 1] = V._dyn(x[:, k], uu[:, k], 1.0, Ts, S.L_WHEELBASE)
    return x, uu


def box_above(poses, ego, gap):
    """an axis-aligned box whose lower face lies `gap` above the highest corner the car reaches at the poses (corner against face)"""
    top = [PD.car_rectangle(*p, ego) for p in poses]; k = int(np.argmax([r[:, 1].max() for r in top])); c = top[k][np.argmax(top[k][:, 1])]
    y0 = c[1] + gap
    A = np.array([[0.0, -1.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]]); b = np.array([-y0, c[0] + 3.0, y0 + 2.0, -(c[0] - 3.0)])
    return A, b


def exact_table(poses, ego, obstacles):
    """(samples, nOb) exact distances; none in the window around the clamp's threshold"""
    t = np.array([[PD.polygon_distance(*p, ego, A, b) for A, b in obstacles] for p in poses])
    assert not ((t > 8e-8) & (t < 1.2e-7)).any()
    return t


def check_record(r, i, exact, substeps, need, what):
    """row i of a clearance dict against the record of the exact distances (clamped as the kernel clamps)"""
    table = np.where(exact < V.CLR_TOUCH, 0.0, exact); ref = V.clearance_record(table, substeps, need); nOb = table.shape[1]
    rowmin = table.min(axis=1)
    assert (np.abs(rowmin - need) > TOL_D).all(), what      # `below` is not in doubt
    assert r["finite"][i] and r["samples"][i] == table.shape[0] and r["below"][i] == ref[4], (what, r["below"][i], ref[4])
    assert np.abs(r["per_obstacle"][i, :nOb] - table.min(axis=0)).max() <= TOL_D, (what, r["per_obstacle"][i], table.min(axis=0))
    for j in range(nOb):
        if exact[:, j].min() < 8e-8:
            assert r["per_obstacle"][i, j] == 0.0, (what, j, r["per_obstacle"][i, j])      # touches or overlaps: exactly 0
    nodes = np.r_[np.arange(0, table.shape[0] - 1, substeps), table.shape[0] - 1]
    assert abs(r["min"][i] - ref[0]) <= TOL_D and abs(r["min_nodes"][i] - table[nodes].min()) <= TOL_D and r["min"][i] == r["per_obstacle"][i, :nOb].min(), what
    q, j = int(r["sample"][i]), int(r["obstacle"][i])
    if ref[0] == 0.0:      # zeros are exact on both sides: the first in row-major order
        assert (q, j) == (int(ref[2]), int(ref[3])), (what, q, j, ref[2], ref[3])
    else:                  # two values that each side knows to 2e-8
        assert (q, j) == (int(ref[2]), int(ref[3])) or abs(table[q, j] - ref[0]) <= 2 * TOL_D, (what, q, j, ref[2], ref[3])
    return ref


@pytest.mark.parametrize("substeps", [1, 3])
def test_parking_clearance_batch_against_polygon_geometry(OA, cases, substeps):
    g = cases; ego = g["ego"]; Aw, bw, pose = wedge(g); N, Ts = 2, 0.6
    x, u = drive(pose, N, Ts); ts = np.ones(N + 1)
    poses = V.parking_samples(x, u, ts, Ts, S.L_WHEELBASE, substeps); all3 = V.parking_samples(x, u, ts, Ts, S.L_WHEELBASE, 3)
    assert np.array_equal(poses[0], pose)      # the first sample IS the named case
    obs = [[(Aw, bw), box_above(all3, ego, 0.0)], [(Aw, bw), box_above(all3, ego, 5e-8)], [box_above(all3, ego, 1e-6), (Aw, bw)]]
    B = len(obs)
    for need in (V.DMIN, 0.4):
        r = OA.parking_clearance_batch(N, Ts, S.L_WHEELBASE, ego, [[len(b) for _, b in o] for o in obs], [np.concatenate([A for A, _ in o]) for o in obs],
                                       [np.concatenate([b for _, b in o]) for o in obs], np.stack([x] * B), np.stack([u] * B), np.stack([ts] * B), substeps, need)
        for i, o in enumerate(obs):
            exact = exact_table(poses, ego, o); jw = 0 if i < 2 else 1
            assert abs(exact[0, jw] - g["d"][np.flatnonzero(g["name"] == "wedge_9.8cm")[0]]) <= 1e-13 * 9
            ref = check_record(r, i, exact, substeps, need, "substeps %d need %g instance %d" % (substeps, need, i))
            if i < 2:      # exact gaps 0 and 5e-8 report exactly 0, at the last sample (the car climbs towards the box), obstacle 1
                assert r["min"][i] == 0.0 and (r["sample"][i], r["obstacle"][i]) == (N * substeps, 1) and ref[0] == 0.0
            else:          # a gap of 1e-6 is reported, not clamped
                assert abs(exact[:, 0].min() - 1e-6) < 1e-12 and abs(r["min"][i] - 1e-6) <= TOL_D and r["min"][i] > 0 and r["obstacle"][i] == 0


def resident_batch(g):
    """two instances of the shipped backwards scenario, N = 20, with two more obstacles that lie behind its walls (the NLP's feasible set is the scenario's): the named
    wedge, 4 .. 9 m from the car, and a box whose upper face lies in the lower left wall's"""
    Aw, bw, _ = wedge(g); bt = S.make_batch(S.BACKWARDS, 2, 20)
    Ab = np.array([[0.0, -1.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]]); bb = np.array([-3.0, -4.0, 5.0, 6.0])      # [-6, -4] x [3, 5]
    bt["vOb"] = np.r_[bt["vOb"], 3, 4].astype(np.int32); bt["A"] = np.vstack([bt["A"], Aw, Ab]); bt["b"] = np.r_[bt["b"], bw, bb]
    return bt


def test_resident_clearance_against_polygon_geometry(OA, cases):
    """Batch.clearance() of a solved batch: the record of the exact distances at the poses validate.parking_samples gives for the DOWNLOADED solution"""
    g = cases; S_ = 3; bt = resident_batch(g); B, N, ego = len(bt["Ts"]), bt["N"], bt["ego"]
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    ctx = OA.Context(0); rb = OA.Batch(ctx, B, N)
    rb.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], ego, bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    rb.solve(opts=OA.ipopt_opts()); out = rb.download()
    assert (out["exitflag"] == 1).all()
    r0 = np.r_[0, np.cumsum(bt["vOb"])]; obs = [(bt["A"][r0[j]:r0[j + 1]], bt["b"][r0[j]:r0[j + 1]]) for j in range(len(bt["vOb"]))]
    for need in (V.DMIN, 0.6):
        r = rb.clearance(S_, need)
        for i in range(B):
            poses = V.parking_samples(out["xp"][i], out["up"][i], out["timeScale"][i], bt["Ts"][i], bt["L"], S_)
            check_record(r, i, exact_table(poses, ego, obs), S_, need, "resident, need %g instance %d" % (need, i))
    rb.close(); ctx.close()
