"""Closed-loop rollout (obca_amd/csrc/obca_track.h): the derivatives of the numpy statement (obca_amd/validate.py) against automatic differentiation of an interval map
written here in torch; the kernel text compiled for the host (tests/emu/track_emu.cpp) against the statement, against the merged rollout, dealt forwards and backwards, with
the clamp and on bad input; what the feature is for, as conditions on the fixture; refusals, the public surface, the build rule and the Julia shim.  No GPU.
Trajectories: tests/rollout_common.py; comparison rules and tolerances: tests/track_common.py."""
import ctypes as C
import inspect
import os
import re
import subprocess
import numpy as np
import pytest
import torch
from conftest import ROOT
import rollout_common as R
import track_common as T
from obca_amd import validate as V


# ---------------------------------------------------------------- 1. A_k, B_k against automatic differentiation
def _torch_park(X, U, L):
    return torch.stack([X[:, 3] * torch.cos(X[:, 2]), X[:, 3] * torch.sin(X[:, 2]), X[:, 3] * torch.tan(U[:, 0]) / L, U[:, 1]], 1)


def _torch_quad(X, U, L):
    m, g, kF, kM, arm, I1, I2, I3 = 0.5, 9.81, 0.0611, 0.0015, 0.225, 3.9e-3, 4.4e-3, 4.9e-3
    ph, th, ps = X[:, 3], X[:, 4], X[:, 5]; p, q, r = X[:, 9], X[:, 10], X[:, 11]
    T_ = kF * (U * U).sum(1)
    return torch.stack([X[:, 6], X[:, 7], X[:, 8],
                        torch.cos(th) * p + torch.sin(th) * r, torch.tan(ph) * (torch.sin(th) * p - torch.cos(th) * r) + q, (torch.cos(th) * r - torch.sin(th) * p) / torch.cos(ph),
                        T_ / m * (torch.sin(ph) * torch.cos(th) * torch.sin(ps) + torch.sin(th) * torch.cos(ps)),
                        T_ / m * (torch.sin(th) * torch.sin(ps) - torch.sin(ph) * torch.cos(th) * torch.cos(ps)), T_ / m * torch.cos(ph) * torch.cos(th) - g,
                        (arm * kF * (U[:, 1] ** 2 - U[:, 3] ** 2) - (I3 - I2) * q * r) / I1, (arm * kF * (U[:, 2] ** 2 - U[:, 0] ** 2) - (I1 - I3) * p * r) / I2,
                        (kM * (U[:, 0] ** 2 - U[:, 1] ** 2 + U[:, 2] ** 2 - U[:, 3] ** 2) - (I2 - I1) * p * q) / I3], 1)


def _torch_jacobians(f, x, u, h, S, L):
    """(N, nx, nx + nu): the derivative of S RK4 steps of h_k / S with respect to the state and the input (for parking: the steering ANGLE), all intervals at once"""
    X0 = torch.tensor(x[:, :-1].T.copy(), dtype=torch.float64, requires_grad=True); U = torch.tensor(u.T.copy(), dtype=torch.float64, requires_grad=True)
    hh = torch.tensor(h / S, dtype=torch.float64)[:, None]; X = X0
    for _ in range(S):
        k1 = f(X, U, L); k2 = f(X + hh / 2 * k1, U, L); k3 = f(X + hh / 2 * k2, U, L); k4 = f(X + hh * k3, U, L)
        X = X + hh / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    rows = []
    for i in range(X.shape[1]):
        gx, gu = torch.autograd.grad(X[:, i].sum(), (X0, U), retain_graph=True)
        rows.append(torch.cat([gx, gu], 1).numpy())
    return np.stack(rows, 1)


@pytest.mark.parametrize("S_", [1, 8])
def test_interval_map_derivatives_match_automatic_differentiation(S_):
    """bound 1e-10 max(1, |entry|): entries reach 5.5, a few thousand operations at 1e-16 give ~1e-12, two orders of margin"""
    worst = 0.0
    for c in R.golden_quad():
        A, B, _, _ = V.track_gains_quad(c["x"], c["u"], c["ts"], c["Ts"], S_)
        J = _torch_jacobians(_torch_quad, c["x"], c["u"], c["ts"][:-1] * c["Ts"], S_, None); AB = np.concatenate([A, B], 2)
        worst = max(worst, float((np.abs(AB - J) / np.maximum(1.0, np.abs(J))).max()))
        assert (np.abs(AB - J) <= 1e-10 * np.maximum(1.0, np.abs(J))).all()
    for c in R.golden_parking():
        A, B, _, _ = V.track_gains_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], S_)
        J = _torch_jacobians(_torch_park, c["x"], c["u"], c["ts"][:-1] * c["Ts"], S_, c["L"]); AB = np.concatenate([A, B], 2)
        worst = max(worst, float((np.abs(AB - J) / np.maximum(1.0, np.abs(J))).max()))
        assert (np.abs(AB - J) <= 1e-10 * np.maximum(1.0, np.abs(J))).all()
        assert np.abs(B[:, 2, 0]).max() > 0      # the steering column is there: d psi / d delta carries sec^2
    print("largest difference statement - autograd, S = %d: %.2e" % (S_, worst))


# ---------------------------------------------------------------- 2. the host build against the statement
WORST = {}
OPTIONS = [(1, 1, False), (1, 1, True), (0, 1, True), (1, 0, True), (0, 0, False)]      # feedback, clamp, dx0 given


def _host_against_numpy(kind, cases, dx, emu, ref, N, S_):
    for i, c in enumerate(cases):
        for fb, cl, given in OPTIONS:
            dx0 = dx if given else None
            got = emu(c, S_, fb, cl, dx0); want = ref(c, S_, fb, cl, dx0); what = "%s N=%d S=%d fb=%d clamp=%d dx0=%s instance %d" % (kind, N, S_, fb, cl, given, i)
            WORST[kind] = max(WORST.get(kind, 0.0), T.gaps(got, want))
            T.check(got, want, T.TOL_HOST, what)
            assert got[0][0] == 0 and got[0][21] == N * S_ + 1 and (got[0][10], got[0][11], got[0][40], got[0][41]) == (0, S_, fb, cl), what
            back = emu(c, S_, fb, cl, dx0, rev=1)      # the lane order gives the same bits
            assert all(np.array_equal(a, b) for a, b in zip(got, back)), what
    print("largest difference host build - numpy so far:", WORST)


@pytest.mark.parametrize("S_", [1, 8])
@pytest.mark.parametrize("N", [2, 20, 65, 128])
def test_quadcopter_host_build_matches_numpy(N, S_):
    _host_against_numpy("quad", R.quad_cases(N)[:2], T.DX0_QUAD * 0.1 if N != 20 else T.DX0_QUAD, T.emu_quad, T.ref_quad, N, S_)


@pytest.mark.parametrize("S_", [1, 8])
@pytest.mark.parametrize("N", [1, 30, 65, 128])
def test_parking_host_build_matches_numpy(N, S_):
    _host_against_numpy("parking", R.parking_cases(N)[:1 if N * S_ > 1024 else 2], T.DX0_PARK, T.emu_parking, T.ref_parking, N, S_)


# ---------------------------------------------------------------- 3. consistency with the merged rollout
@pytest.mark.parametrize("S_", [1, 8])
def test_without_feedback_clamp_and_offset_it_is_the_chain_rollout_bit_for_bit(S_):
    for c in R.golden_quad() + R.synthetic_quad(65):
        rec, X, P, _, _ = T.emu_quad(c, S_, 0, 0, None); ro, Xo, Po = R.emu_quad(c, S_, 0)
        assert np.array_equal(rec[:40], ro) and np.array_equal(X, Xo) and np.array_equal(P, Po)
        assert rec[40:].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]
    for c in R.golden_parking() + R.synthetic_parking(65):
        rec, X, P, _, _ = T.emu_parking(c, S_, 0, 0, None); ro, Xo, Po = R.emu_parking(c, S_, 0)
        assert np.array_equal(rec[:40], ro) and np.array_equal(X, Xo) and np.array_equal(P, Po)


# ---------------------------------------------------------------- 4. what the feature is for
def test_feedback_beats_the_open_loop_on_the_fixture():
    """Conditions, with the default (untuned) weights at 8 sub-steps.  The statement's own figures, printed by this test -- quadcopter dev_pos / end_pos closed against
    open: 0.489 / 0.325 against 2.008 / 1.611, 0.621 / 0.321 against 1.167 / 0.667, 0.478 / 0.168 against 1.435 / 1.095, 0.552 / 0.380 against 1.123 / 0.467 [m]; from
    0.1 m and 0.1 m/s off the open loop ends 2.1-3.4 m away, the closed loop where it ended before.  Parking end_pos: 0.66 / 0.66 / 1.39 mm closed against
    18.2 / 10.8 / 27.7 mm open (ratio 0.061 at most); from (0.1, 0.1, 0.05, 0) off the same closed against 0.48-0.65 m open (ratio 0.0021 at most)."""
    for dx0 in (None, T.DX0_QUAD):
        for i, c in enumerate(R.golden_quad()):
            cl = T.ref_quad(c, 8, 1, 1, dx0)[0]; op = T.ref_quad(c, 8, 0, 0, dx0)[0]
            print("quadcopter %d dx0 %s: dev_pos %.4f closed, %.4f open; end_pos %.4f closed, %.4f open; du_max %.3f at %d, saturated %d"
                  % (i, dx0 is not None, cl[1], op[1], cl[6], op[6], cl[43], cl[44], cl[42]))
            assert cl[0] == 0 and op[0] == 0 and cl[1] < op[1] and cl[6] < op[6]
            assert np.array_equal(T.emu_quad(c, 8, 1, 1, dx0)[0][[0, 42, 44]], cl[[0, 42, 44]])
    for dx0 in (None, T.DX0_PARK):
        for i, c in enumerate(R.golden_parking()):
            cl = T.ref_parking(c, 8, 1, 1, dx0)[0]; op = T.ref_parking(c, 8, 0, 0, dx0)[0]
            print("parking %d dx0 %s: end_pos %.3e closed, %.3e open (ratio %.4f); dev_pos %.3e / %.3e; clearance %.4f / %.4f; saturated %d"
                  % (i, dx0 is not None, cl[6], op[6], cl[6] / op[6], cl[1], op[1], cl[16], op[16], cl[42]))
            assert cl[0] == 0 and op[0] == 0 and cl[6] < 0.25 * op[6]
    assert "A = I + h f_x" in V.track_gains_quad.__doc__ and not hasattr(V, "track_gains_euler")


# ---------------------------------------------------------------- 5. the clamp
DX0_CLAMP = np.array([0.3, -0.3, 0.2, 0.3])      # the speed error asks for more than 0.4 m/s^2 in the first intervals of every fixture instance


def test_clamp_keeps_the_applied_inputs_inside_the_bounds():
    lo, hi = np.array([-0.6, -0.4])[:, None], np.array([0.6, 0.4])[:, None]
    for c in R.golden_parking():
        _, _, info = V.track_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], 8, DX0_CLAMP)
        _, _, free = V.track_parking(c["x"], c["u"], c["ts"], c["Ts"], c["L"], 8, DX0_CLAMP, clamp=False)
        assert info["clipped"].sum() > 0 and (info["U"] >= lo).all() and (info["U"] <= hi).all() and ((free["U"] < lo) | (free["U"] > hi)).any()
        rec = T.emu_parking(c, 8, 1, 1, DX0_CLAMP)[0]; ref = T.ref_parking(c, 8, 1, 1, DX0_CLAMP)[0]; off = T.emu_parking(c, 8, 1, 0, DX0_CLAMP)[0]
        assert rec[42] == info["clipped"].sum() > 0 and rec[42] == ref[42] and off[42] == 0 and off[43] > rec[43]
        assert abs(rec[45] - np.hypot(0.3, 0.3)) < 1e-15 and rec[0] == 0
    c = R.golden_quad()[0]      # the quadcopter's box: a start that falls at 6 m/s asks for more than 7.8
    dx0 = np.zeros(12); dx0[8] = -6.0
    _, _, info = V.track_quad(c["x"], c["u"], c["ts"], c["Ts"], 8, dx0); _, _, free = V.track_quad(c["x"], c["u"], c["ts"], c["Ts"], 8, dx0, clamp=False)
    assert info["clipped"].sum() > 0 and info["U"].max() <= 7.8 and info["U"].min() >= 1.2 and (free["U"].max() > 7.8 or free["U"].min() < 1.2)
    assert T.emu_quad(c, 8, 1, 1, dx0)[0][42] == info["clipped"].sum()


# ---------------------------------------------------------------- 6. bad input
def assert_bad(got, nS, S_, fb, cl):
    rec, X, _, K, _ = got
    exp = np.r_[1, np.nan, -1, np.full(7, np.nan), 0, S_, 0, 0, 0, 0, np.nan, np.nan, -1, -1, nS, nS, 1, 0, np.full(16, np.nan), fb, cl, -1, np.nan, -1, np.nan, 0, 0]
    assert np.array_equal(rec, exp, equal_nan=True), rec
    assert np.isnan(X).all() and np.isnan(K).all()


def test_bad_input_marks_its_instance_and_no_other():
    q = R.golden_quad(); good = [T.emu_quad(c, 4) for c in q]
    u = np.array(q[1]["u"]); u[1, 3] = np.nan
    assert_bad(T.emu_quad(dict(q[1], u=u), 4), 81, 4, 1, 1)
    ref = T.ref_quad(dict(q[1], u=u), 4)
    assert np.array_equal(ref[0], T.emu_quad(dict(q[1], u=u), 4)[0], equal_nan=True) and np.isnan(ref[1]).all() and np.isnan(ref[3]).all()
    dx0 = T.DX0_QUAD.copy(); dx0[7] = np.nan
    assert_bad(T.emu_quad(q[1], 4, dx0=dx0), 81, 4, 1, 1)
    assert np.array_equal(T.ref_quad(q[1], 4, dx0=dx0)[0], T.emu_quad(q[1], 4, dx0=dx0)[0], equal_nan=True)
    xn = np.array(q[1]["x"]); xn[0, 20] = np.inf      # the last node enters no gain: the chain's own scan finds it
    assert_bad(T.emu_quad(dict(q[1], x=xn), 4), 81, 4, 1, 1)
    # a pitch driven through pi/2 (the rollout test's input), open loop
    N = q[0]["N"]; uo = np.full((4, N), 4.48); uo[1] += 1.0; uo[3] -= 1.0
    over = dict(q[0], u=uo)
    assert_bad(T.emu_quad(over, 8, 0, 0), 8 * N + 1, 8, 0, 0)
    assert np.array_equal(T.ref_quad(over, 8, 0, 0)[0], T.emu_quad(over, 8, 0, 0)[0], equal_nan=True)
    for c, g in zip(q, good):      # (instances share nothing: the others come back bit for bit)
        assert all(np.array_equal(a, b) for a, b in zip(T.emu_quad(c, 4), g))
    p = R.golden_parking(); good = [T.emu_parking(c, 4) for c in p]
    u = np.array(p[2]["u"]); u[0, 29] = np.nan
    assert_bad(T.emu_parking(dict(p[2], u=u), 4), 121, 4, 1, 1)
    assert_bad(T.emu_parking(p[2], 4, dx0=np.array([0.0, np.inf, 0.0, 0.0])), 121, 4, 1, 1)
    assert_bad(T.emu_parking(dict(p[0], Ts=np.nan), 4, 0, 1), 121, 4, 0, 1)
    for c, g in zip(p, good):
        assert all(np.array_equal(a, b) for a, b in zip(T.emu_parking(c, 4), g))


# ---------------------------------------------------------------- 7. refusals
def test_argument_errors():
    lib = T.emu(); out = np.zeros(48); w = np.zeros(40000); z = np.zeros(8192); prob = np.zeros(4096); dp = T.dp
    q4, r2, q12, r4 = np.ones(4), np.ones(2), np.ones(12), np.ones(4)

    def park(S_=8, fb=1, cl=1, q=q4, r=r2, qf=q4, need=0.05, N=30):
        return lib.emu_track_parking(N, dp(prob), dp(z), None, 2, S_, fb, cl, T._opt(q), T._opt(r), T._opt(qf), None, need, 0, dp(w), dp(w), dp(w), dp(w), dp(out))

    def quad(S_=8, fb=1, cl=1, q=q12, r=r4, qf=q12, need=0.0, N=5):
        return lib.emu_track_quad(N, dp(prob), dp(z), dp(z), dp(z), 1, S_, fb, cl, T._opt(q), T._opt(r), T._opt(qf), None, need, 0, dp(w), dp(w), dp(w), dp(w), dp(out))
    bad4 = lambda i, v: np.r_[np.ones(i), v, np.ones(3 - i)]      # noqa: E731
    cases = [(dict(S_=0), b"need 1 <= substeps <= 32"), (dict(S_=33), b"need 1 <= substeps <= 32"), (dict(need=np.nan), b"need a finite `need`"),
             (dict(fb=2), b"feedback must be 0 (open loop) or 1"), (dict(fb=-1), b"feedback must be 0"), (dict(cl=2), b"clamp must be 0 or 1"),
             (dict(q=None), b"the weights q, r and qf must not be NULL"), (dict(r=None), b"must not be NULL"), (dict(qf=None), b"must not be NULL")]
    for kw, msg in cases:
        assert park(**kw) == -1 and msg in lib.emu_track_last_error(), kw
        assert quad(**kw) == -1 and msg in lib.emu_track_last_error(), kw
    for v in (-1.0, np.nan, np.inf):
        assert park(q=bad4(2, v)) == -1 and b"q and qf need finite entries >= 0" in lib.emu_track_last_error()
        assert park(qf=bad4(0, v)) == -1 and b"q and qf need finite entries >= 0" in lib.emu_track_last_error()
        assert quad(q=np.r_[np.ones(11), v]) == -1 and b"q and qf need finite entries >= 0" in lib.emu_track_last_error()
    for v in (0.0, -1.0, np.nan, np.inf):
        assert park(r=np.array([1.0, v])) == -1 and b"r needs finite entries > 0" in lib.emu_track_last_error()
        assert quad(r=np.array([1.0, 1.0, 1.0, v])) == -1 and b"r needs finite entries > 0" in lib.emu_track_last_error()
    for N in (0, 129):
        assert park(N=N) == -1 and b"1 <= N <= OBCA_NMAX" in lib.emu_track_last_error()
        assert quad(N=N) == -1 and b"1 <= N <= OBCA_QUAD_NMAX" in lib.emu_track_last_error()
    assert (out == 0).all()
    # the library's own refusals: one text per cause and entry point
    hip = open(os.path.join(ROOT, "obca_amd", "csrc", "obca_hip.hip")).read()
    for e, dims in (("obca_batch_track", "4, 2"), ("obca_quad_batch_track", "QX, QU")):
        assert '"%s: NULL argument"' % e in hip and '"%s: nothing has been solved since the last upload or shift"' % e in hip
        assert '"%s_ms: no track call has run on this batch"' % e in hip
        assert 'track_fetch(bt, %s, false, X, "%s_states")' % (dims, e) in hip and 'track_fetch(bt, %s, true, K, "%s_gains")' % (dims, e) in hip
    assert '": no track call has run on this batch since it was last filled"' in hip
    assert '"obca_parking_track_batch: need B>=1, 1<=N<=OBCA_NMAX"' in hip and '"obca_quadcopter_track_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"' in hip
    assert hip.count("trk::track_check_args(substeps, feedback, clamp, q, r, qf, ") == 4


# ---------------------------------------------------------------- 8. the public surface, the build rule, 9. the Julia shim
def test_header_exports_python_and_julia_agree():
    import obca_amd
    from obca_amd import api, cabi, planner as PL
    import test_hybrid_cpu as TH
    import test_julia_shim_cpu as J
    protos = cabi.prototypes("obca_track.h")
    assert sorted(protos) == sorted(api.TRACK_EXPORTS) and len(protos) == 10 and "obca_track.h" in cabi.__doc__
    others = (set(api.EXPORTS) | set(api.PATH_WS_EXPORTS) | set(api.CLEARANCE_EXPORTS) | set(api.REFINE_EXPORTS) | set(api.QUAD_SUBDIVIDE_EXPORTS) | set(api.PLAN_DEVICE_EXPORTS)
              | set(api.SCENE_EXPORTS) | set(api.PLAN_RESIDENT_EXPORTS) | set(api.PLAN_RESIDENT_CHECK_EXPORTS) | set(api.QUAD_PLAN_RESIDENT_EXPORTS) | set(api.ROLLOUT_EXPORTS)
              | set(PL.PLAN3D_EXPORTS))
    assert not set(api.TRACK_EXPORTS) & others and not set(protos) & set(cabi.prototypes("obca_hip.h")) and not set(protos) & set(cabi.prototypes("obca_rollout.h"))
    assert [len(protos[n][1]) for n in api.TRACK_EXPORTS] == [10, 2, 2, 2, 24, 10, 2, 2, 2, 20]
    # no name of the header falls under a filter by which an older test picks ITS entry points out of the library's symbols
    assert not any(w in s for s in api.TRACK_EXPORTS for w in ("refine", "hybrid", "scene", "plan", "subdivide", "clearance", "path_ws", "start_download", "rollout"))
    syms = subprocess.run(["nm", "-D", "--defined-only", api.build_library()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (obca_\w+)", syms))
    assert {s for s in exported if "track" in s} == set(api.TRACK_EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "obca_track.h")).read()
    assert re.search(r"#define OBCA_TRK_OUT 48\b", hdr) and V.TRK_OUT == 48 == V.ROLL_OUT + 8
    lib = api._load(); f = C.c_float(0); q, r = np.ones(12), np.ones(4)
    assert lib.obca_batch_track(None, 8, 1, 1, q[:4], r[:2], q[:4], None, 0.05, np.zeros(48)) == -1      # no batch: refused, no device touched
    assert lib.obca_quad_batch_track(None, 8, 1, 1, q, r, q, None, 0.0, np.zeros(48)) == -1
    assert lib.obca_batch_track_ms(None, C.byref(f)) == -1 and lib.obca_quad_batch_track_states(None, np.zeros(1)) == -1 and lib.obca_batch_track_gains(None, np.zeros(1)) == -1
    with pytest.raises((TypeError, C.ArgumentError)):      # out as int32
        lib.obca_batch_track(None, 8, 1, 1, q[:4], r[:2], q[:4], None, 0.05, np.zeros(48, np.int32))
    for f_ in ("parking_track_batch", "quadcopter_track_batch", "TRACK_Q_PARKING", "TRACK_R_PARKING", "TRACK_QF_PARKING", "TRACK_Q_QUAD", "TRACK_R_QUAD", "TRACK_QF_QUAD"):
        assert hasattr(obca_amd, f_) and f_ in obca_amd.__all__
    assert obca_amd.TRACK_Q_PARKING == (10, 10, 10, 1) and obca_amd.TRACK_R_PARKING == (1, 1) and obca_amd.TRACK_QF_PARKING == (100, 100, 100, 10)
    assert obca_amd.TRACK_Q_QUAD == (10, 10, 10, 1, 1, 1, 1, 1, 1, 0.1, 0.1, 0.1) and obca_amd.TRACK_R_QUAD == (0.1,) * 4 and obca_amd.TRACK_QF_QUAD == tuple(10.0 * v for v in obca_amd.TRACK_Q_QUAD)
    for cls, need in ((obca_amd.Batch, V.DMIN), (obca_amd.QuadBatch, 0.0)):
        sig = inspect.signature(cls.track).parameters
        assert list(sig) == ["self", "substeps", "dx0", "Q", "R", "Qf", "feedback", "clamp", "need"]
        assert [sig[n].default for n in list(sig)[1:]] == [8, None, None, None, None, True, True, need]
        assert all(callable(getattr(cls, m)) for m in ("track_states", "track_gains", "track_ms")) and "track_gains" in vars(api._DeviceBatch)
    for fn in (obca_amd.parking_track_batch, obca_amd.quadcopter_track_batch):
        sig = inspect.signature(fn).parameters
        assert sig["states"].default is True and sig["gains"].default is True
    # every ccall of the shim against the header, parameter by parameter; a library constant of its own
    kinds = TH._kinds(hdr)
    src = open(os.path.join(ROOT, "julia", "OBCATrack.jl")).read()
    assert re.search(r"^const TRK = LIB$", src, flags=re.M)
    calls = []
    for m in re.finditer(r"ccall\(\(:(obca_[a-z_0-9]+), TRK\),\s*(\w+),\s*\(", src):
        i = m.end(); depth = 1; j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0); j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        calls.append((m.group(1), ["ptr" if t.startswith(("Ptr{", "Ref{")) else J.JL.get(t, "?" + t) for t in types]))
        assert m.group(2) == "Cint"
    assert {n for n, _ in calls} == set(kinds) == set(api.TRACK_EXPORTS), calls
    for n, k in calls:
        assert k == kinds[n], (n, k, kinds[n])
    assert src.count("ccall(") == len(calls) + 1 and "ccall((:obca_last_error, LIB)" in src


def test_host_build_goes_through_the_one_rule(tmp_path, monkeypatch):
    from obca_amd import buildflags as BF
    EMU = os.path.join(ROOT, "tests", "emu"); name = "track_emu"
    assert name in BF.EMU_PIECES and name not in BF.DEFAULT and not any(name in t for t in (BF.PIECES, BF.TEST_PIECES, BF.CHECK_PIECES))
    p = BF.EMU_PIECES[name]
    assert os.path.realpath(p.out) == os.path.realpath(EMU + "/libobca_track_emu.so")
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
    for h in ("obca_track.h", "obca_rollout.h", "obca_clearance.h", "obca_quad_model.h", "obca_model.h"):
        assert os.path.realpath(os.path.join(csrc, h)) in seen, h
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    aside = str(tmp_path / "libobca_track_emu.so")
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls; i = argv.index("-o")
    assert argv[:i] == BF.GXX + ["-O1"] and argv[i + 2:] == [EMU + "/track_emu.cpp"] and os.path.dirname(argv[i + 1]) == str(tmp_path)
    # the kernel text is nothing the solve kernels use, it follows the rollout's, and no finite difference stands in it
    for f in os.listdir(csrc):
        if f.endswith(".h"):
            assert not re.search(r'#\s*include\s*"obca_track.h"', open(os.path.join(csrc, f)).read()), f
    hip = open(os.path.join(csrc, "obca_hip.hip")).read()
    assert hip.count('#include "obca_track.h"') == 1 and '#include "obca_rollout.h"\n#include "obca_track.h"' in hip
    txt = re.sub(r"//.*", "", open(os.path.join(csrc, "obca_track.h")).read())
    assert "sincos_bounded" not in txt and "rcp_nr" not in txt and "atomic" not in txt and "dyn_g_value" not in txt and "while" not in txt
    model = open(os.path.join(csrc, "obca_quad_model.h")).read()
    body = model.split("OBCA_FN void dyn_g_continuous_jvp(")[1].split("\n}\n")[0]
    assert "sincos_bounded" not in body and "rcp_nr" not in body and "gyro" not in body
