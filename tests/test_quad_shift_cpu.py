"""Receding-horizon restart of the quadcopter batch, without a GPU: (a) the shift text of obca_amd/csrc/obca_quad_shift.h compiled for the host (tests/emu/quad_shift_emu.cpp)
against a numpy statement of its rules, bit for bit; (b) the CPU checker restarted from the host-built shift needs fewer iterations than a cold solve; (c) the entry point is
in the header, the Python binding and the Julia shim."""
import os
import re
import numpy as np
import pytest
from conftest import ROOT
import packing as P
import quad_shift_common as QS


@pytest.mark.parametrize("N,shift", [(2, 0), (2, 2), (5, 3), (63, 1), (64, 64), (65, 7), (128, 127), (128, 128)])
def test_shift_text_matches_numpy_bit_for_bit(N, shift):
    plen, zlen, ox, ot = QS.sizes(N); L = P.quad_layout(N)
    assert (plen, zlen, ox, ot) == (P.quad_problem_len(N), L["len"], L["x"], L["t"])
    rng = np.random.default_rng(1000 * N + shift)
    touched = set(range(P.QPH_X0, P.QPH_X0 + 24)) | {P.QPH_TWS, P.QPH_DWS}
    untouched = [i for i in range(P.QPH_SIZE) if i not in touched]
    for flag in (0.0, 1.0, 2.0):
        for with_x0 in (False, True):
            for with_xF in (False, True):
                prob = rng.normal(size=plen); prob[P.QPH_DWS] = 0.0; z = rng.normal(size=zlen) * 10
                info = rng.normal(size=8); info[7] = flag
                x0n = rng.normal(size=12) if with_x0 else None; xFn = rng.normal(size=12) if with_xF else None
                p0, z0, i0 = prob.copy(), z.copy(), info.copy()
                got = QS.emu_shift(N, shift, prob, z, info, x0n, xFn); want = QS.numpy_shift(N, shift, prob, z, info, x0n, xFn)
                tag = (N, shift, flag, with_x0, with_xF)
                assert np.array_equal(got, want), tag
                assert np.array_equal(prob, p0) and np.array_equal(z, z0) and np.array_equal(info, i0), tag      # the inputs are read only
                assert np.array_equal(got[untouched], p0[untouched]), tag
                ws = got[P.QPH_SIZE:].reshape(N + 1, 12); x = z[ox:ox + 12 * (N + 1)].reshape(N + 1, 12)
                if flag == 0.0:      # a failed instance keeps its warm start, timeWS and dual_ws; x0 only moves with x0_new
                    assert np.array_equal(got[P.QPH_SIZE:], p0[P.QPH_SIZE:]) and got[P.QPH_TWS] == p0[P.QPH_TWS] and got[P.QPH_DWS] == 0.0, tag
                    assert np.array_equal(got[P.QPH_X0:P.QPH_X0 + 12], x0n if with_x0 else p0[P.QPH_X0:P.QPH_X0 + 12]), tag
                else:                # spot checks independent of numpy_shift's indexing
                    assert np.array_equal(ws[0], x[shift]) and np.array_equal(ws[N - shift], x[N]) and got[P.QPH_TWS] == z[ot] and got[P.QPH_DWS] == 1.0, tag
                    assert np.array_equal(ws[N], xFn if (with_xF and shift > 0) else x[N]), tag
                    assert np.array_equal(got[P.QPH_X0:P.QPH_X0 + 12], x0n if with_x0 else x[shift]), tag
                assert np.array_equal(got[P.QPH_XF:P.QPH_XF + 12], xFn if with_xF else p0[P.QPH_XF:P.QPH_XF + 12]), tag
    # a failed instance whose iterate is all NaN: nothing is read from it
    prob = rng.normal(size=plen); info = np.zeros(8); z = np.full(zlen, np.nan)
    for x0n in (None, rng.normal(size=12)):
        got = QS.emu_shift(N, shift, prob, z, info, x0n, None)
        assert np.isfinite(got).all() and np.array_equal(got, QS.numpy_shift(N, shift, prob, z, info, x0n, None))


def test_restart_from_the_shifted_solution_needs_fewer_iterations_on_the_checker():
    """make_quad_batch(4, 60), shift 4, throughput options: cold solves, then restarts from the host-built shift with the warm option values (mu_init = bound_push = bound_frac
    = 1e-4: what obca_amd.quad_warm_restart_opts sets).  All exit flags 1, and the restarts take less than 0.75 of the cold iterations (measured: 158 / 393 = 0.40)."""
    import oracle_quad as Q
    from obca_amd import scenarios as S
    B, N, shift = 4, 60, 4
    bt = S.make_quad_batch(B, N)
    warm = Q.default_opts(); warm.mu_init = warm.bound_push = warm.bound_frac = 1e-4
    cold_it, warm_it = [], []
    for i in range(B):
        r = Q.quadcopter_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], 1.0)
        assert r["exitflag"] == 1, (i, r["exitflag"])
        out = dict(xp=r["xp"][None], timeScale=r["timeScale"][None], info=np.array([[r["status"], r["iters"], r["obj"], r["pinf"], r["dinf"], r["mu"], r["nreg"], r["exitflag"]]], float))
        s = QS.shifted_problem(N, shift, bt["x0"][i], bt["xF"][i], bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], 1.0, 1, out, 0)
        assert np.array_equal(s["x0"], r["xp"][:, shift]) and np.array_equal(s["xWS"][N - shift:], np.tile(r["xp"][:, N], (shift + 1, 1))) and s["timeWS"] == r["t"] and s["dual_ws"] == 1
        r2 = Q.quadcopter_signed_dist(s["x0"], s["xF"], N, bt["Ts"], bt["R"], bt["ob"], s["xWS"], s["timeWS"], opts=warm, dual_ws=s["dual_ws"])
        assert r2["exitflag"] == 1, (i, r2["exitflag"])
        cold_it.append(r["iters"]); warm_it.append(r2["iters"])
    print("iterations cold %s -> shifted restart %s" % (cold_it, warm_it))
    assert sum(warm_it) < 0.75 * sum(cold_it), (cold_it, warm_it)


def test_entry_point_is_in_the_header_the_binding_and_the_shim():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "obca_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+obca_quad_batch_shift_warm_start\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m and [p.strip() for p in m.group(1).split(",")] == ["obca_quad_batch *bt", "int shift", "const double *x0_new", "const double *xF_new"]
    import obca_amd
    from obca_amd.api import EXPORTS
    assert "obca_quad_batch_shift_warm_start" in EXPORTS and hasattr(obca_amd.QuadBatch, "shift_warm_start") and "quad_warm_restart_opts" in obca_amd.__all__
    jl = open(os.path.join(ROOT, "julia", "OBCAHip.jl")).read()
    for s in ("ccall((:obca_quad_batch_shift_warm_start, LIB)", "ccall((:obca_batch_shift_warm_start, LIB)", "mutable struct QuadBatch", "function shift_warm_start!(", "function batch_shift_warm_start!("):
        assert s in jl, s
    for sym in ("create", "destroy", "upload", "solve", "sync", "download", "validate"):
        assert "ccall((:obca_quad_batch_%s, LIB)" % sym in jl, sym
