"""What tests/test_refine_cpu.py and tests/test_gpu_refine.py share: the host build of the kernel text of obca_amd/csrc/obca_refine.h (tests/emu/refine_emu.cpp,
buildflags.build("refine_emu")); the trajectories both suites run -- the never-solved warm starts of clearance_common.parking_cases --; a source instance packed as a resident
batch holds it (problem record, last iterate, start iterate, info) with the numpy statement validate.refine_parking of what its refinement must be; the comparison rules.

Tolerances.  x' at a sub-step s > 0 is ONE val::park_step: about twenty fp64 operations and three libm calls (tan, cos, sin) on numbers of size <= 100, where one rounding
is 1e-14: 1e-12 max(1, |v|), the bound clearance_common reasons out for its fp64 path.  numpy against g++ -O1 differ in how s / r * ts * Ts associates, the device library's
sin / cos / tan against libm by a few ulps; both stay inside.  Everything copied or interpolated is expected to the bit: u', Ts / r, the reference (one product kept from
contracting into one sum), lam', mu', every copied header word, every cleared word, and x' at s = 0 and at the last node."""
import ctypes as C
import functools
import numpy as np
import packing as P
import clearance_common as K
from obca_amd import buildflags, validate as V

D = C.POINTER(C.c_double)
TOL_X = 1e-12
SHAPES = ((2, 2), (5, 3), (33, 2), (64, 2), (4, 32), (7, 1))      # (N, r): fewer than 64 nodes, 67 nodes in two rounds, 129 nodes at the limit, the largest factor, the copy
SENTINEL = -7.25
dp = K.dp


@functools.lru_cache(None)
def emu():
    lib = C.CDLL(buildflags.build("refine_emu"))
    lib.emu_refine_last_error.restype = C.c_char_p
    lib.emu_refine_check_args.argtypes = [C.c_int] * 4
    lib.emu_refine_host.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, D, D, D, C.c_int, D, D, D]
    lib.emu_refine_record.argtypes = [C.c_int, C.c_int, C.c_int, D, D, D, D, C.c_int, D, D, C.c_int, C.POINTER(C.c_int)]
    a, b, c = (C.c_int(0) for _ in range(3))
    lib.emu_refine_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (32, 128, P.OB_HDR)
    return lib


def cases(N):
    """clearance_common.parking_cases(N): BACKWARDS with timeScale 1 and 1 + 0.1 sin k, mixed batches with 3-8 and 3-4 rows per obstacle and ragged obstacle counts"""
    return K.parking_cases(N)


def close_x(a, ref):
    return bool((np.abs(a - ref) <= TOL_X * np.maximum(1.0, np.abs(ref))).all())


# ---------------------------------------------------------------- the host-pointer form
def emu_host(c, r, rev=0, ts="own"):
    """one instance through refine_host_instance: (rc, Ts', x' (4, rN+1), u' (2, rN))"""
    N = c["N"]; Nf = N * r
    x = np.ascontiguousarray(c["x"].T); u = np.ascontiguousarray(c["u"].T); t = None if ts is None else np.ascontiguousarray(c["ts"] if isinstance(ts, str) else ts, float)
    Tsf = np.full(1, SENTINEL); xf = np.full((Nf + 1, 4), SENTINEL); uf = np.full((Nf, 2), SENTINEL)
    rc = emu().emu_refine_host(N, int(r), float(c["Ts"]), float(c["L"]), dp(x), dp(u), dp(t), int(rev), dp(Tsf), dp(xf), dp(uf))
    assert rc in (0, 1), emu().emu_refine_last_error()
    return rc, Tsf[0], xf.T.copy(), uf.T.copy()


# ---------------------------------------------------------------- the resident form
def source(c, seed=0, t=None, fixTime=0, dist=0):
    """instance c as a solved resident batch holds it: problem record, last iterate z (x, u of the case, one t, positive multipliers, everything behind them noise that must
    not travel), start iterate z0 (another trajectory, multipliers of its own), info with exit flag 1.  `parts` keeps the arrays the numpy statement takes."""
    rng = np.random.default_rng(1000 + seed); N, vOb = c["N"], c["vOb"]; nOb, M = len(vOb), int(vOb.sum())
    ref = c["x"][:3] + 0.01 * rng.standard_normal((3, N + 1))
    x0 = c["x"][:, 0].copy(); xF = c["x"][:, -1].copy()
    prob = P.pack_problem(x0, xF, N, c["Ts"], c["L"], c["ego"], np.array([-21.0, 22.0, -3.0, 13.0]), vOb, c["A"], c["b"], ref[0], ref[1], ref[2], fixTime, dist)
    lay = P.layout(N, nOb, M); t = float(c["ts"][1] if t is None else t)
    lam = rng.uniform(0.0, 2.0, (M, N + 1)); mu = rng.uniform(0.0, 2.0, (4 * nOb, N + 1))
    z = P.pack_start(N, nOb, M, c["x"].T, c["u"].T, lam.T, mu.T); z[lay["t"]] = t; z[lay["sl"]:] = rng.standard_normal(lay["len"] - lay["sl"])
    x0s = c["x"] + 0.05 * rng.standard_normal((4, N + 1)); u0s = 0.5 * c["u"]; lam0 = rng.uniform(0.0, 1.0, (M, N + 1)); mu0 = rng.uniform(0.0, 1.0, (4 * nOb, N + 1))
    z0 = P.pack_start(N, nOb, M, x0s.T, u0s.T, lam0.T, mu0.T)
    info = np.array([0.0, 23.0, 1.5, 1e-9, 1e-7, 1e-9, 0.0, 1.0])
    return dict(c=c, N=N, nOb=nOb, M=M, prob=prob, z=z, z0=z0, info=info, lay=lay, fix=fixTime,
                parts=dict(sol=(c["x"], c["u"], t, lam, mu), start=(x0s, u0s, 1.0, lam0, mu0), ref=ref))


def emu_record(src, r, duals, rev=0, pad=37):
    """the instance through refine_record into a sentinel-filled destination whose row is `pad` doubles longer than its layout: (status, pd, zd)"""
    N, Nf = src["N"], src["N"] * r
    ld = P.layout(Nf, src["nOb"], src["M"]); zlen = ld["len"] + pad
    pd = np.full(P.OB_HDR + 3 * (Nf + 1) + 5, SENTINEL); zd = np.full(zlen + 5, SENTINEL); st = C.c_int(99)
    rc = emu().emu_refine_record(N, int(r), int(duals), dp(src["prob"]), dp(src["z"]), dp(src["z0"]), dp(src["info"]), int(rev), dp(pd), dp(zd), zlen, C.byref(st))
    assert rc == 0, emu().emu_refine_last_error()
    assert (pd[-5:] == SENTINEL).all() and (zd[-5:] == SENTINEL).all()      # nothing behind the record and behind the row's stride
    return st.value, pd[:-5], zd[:-5]


def expected_record(src, r, duals, status):
    """(pd, zd_exact, xmask): the destination the numpy statement asks for.  zd_exact holds the bit-exact expectation with the interpolated poses (xmask) left to TOL_X."""
    N, Nf, nOb, M = src["N"], src["N"] * r, src["nOb"], src["M"]; ld = P.layout(Nf, nOb, M); c = src["c"]
    pd = np.zeros(P.OB_HDR + 3 * (Nf + 1)); pd[:P.OB_HDR] = src["prob"][:P.OB_HDR]; pd[P.PH["TS"]] = c["Ts"] / r
    zd = np.zeros(ld["len"]); zd[ld["t"]] = 1.0
    x, u, t, lam, mu = src["parts"]["sol" if status == 0 else "start"]
    f = V.refine_parking(x, u, 1.0 if src["fix"] else t, c["Ts"], c["L"], r, ref=src["parts"]["ref"], lam=lam, mu=mu)
    pd[P.OB_HDR:] = f["ref"].reshape(-1)
    if status >= 0:
        zd[ld["x"]:ld["x"] + 4 * (Nf + 1)] = f["x"].T.reshape(-1); zd[ld["u"]:ld["u"] + 2 * Nf] = f["u"].T.reshape(-1)
        if duals:
            zd[ld["lam"]:ld["lam"] + M * (Nf + 1)] = f["lam"].T.reshape(-1); zd[ld["mu"]:ld["mu"] + 4 * nOb * (Nf + 1)] = f["mu"].T.reshape(-1)
    xmask = np.zeros(ld["len"], bool)
    if status >= 0:
        q = np.arange(Nf + 1); inter = (q % r != 0) & (q < Nf)
        xmask[ld["x"]:ld["x"] + 4 * (Nf + 1)] = np.repeat(inter, 4)
    return pd, zd, xmask


def check_record(src, r, duals, status, pd, zd, what):
    epd, ezd, xm = expected_record(src, r, duals, status); n = len(ezd)
    assert np.array_equal(pd, epd), (what, np.flatnonzero(pd != epd)[:8])
    assert np.array_equal(zd[:n][~xm], ezd[~xm]), (what, np.flatnonzero((zd[:n] != ezd) & ~xm)[:8])
    assert close_x(zd[:n][xm], ezd[xm]), what
    assert (zd[n:] == 0.0).all(), what      # cleared up to the row's stride


# ---------------------------------------------------------------- the resident pipeline through the host builds (solver emulation + this kernel text)
def emu_dualws_into(solver, z, prob, N, v, A, b):
    """DualMultWS of the reference stored in `prob` into the iterate z, as a solve without a dual warm start does first (emu_solver.parking_signed_dist_batch does the same)"""
    nOb, M = len(v), int(v.sum()); lay = P.layout(N, nOb, M); rl = P.row_lengths(A); An = A / rl[:, None]; bn = b / rl
    g = prob[P.PH["G"]:P.PH["G"] + 4].copy(); off = prob[P.PH["OFF"]]
    rx, ry, rw = (prob[P.OB_HDR + a * (N + 1):P.OB_HDR + (a + 1) * (N + 1)] for a in range(3))
    for k in range(N + 1):
        cs, sn = np.cos(rw[k]), np.sin(rw[k]); r0 = 0
        for j, vj in enumerate(v):
            a1, a2, bj = (np.ascontiguousarray(q) for q in (An[r0:r0 + vj, 0], An[r0:r0 + vj, 1], bn[r0:r0 + vj])); lam = np.zeros(8); mu = np.zeros(4); d = C.c_double(0)
            solver.emu_dualws(C.c_int(int(vj)), dp(a1), dp(a2), dp(bj), dp(g), C.c_double(rx[k] + off * cs), C.c_double(ry[k] + off * sn), C.c_double(cs), C.c_double(sn), dp(lam), dp(mu), C.byref(d))
            z[lay["lam"] + k * M + r0:lay["lam"] + k * M + r0 + vj] = lam[:vj]; z[lay["mu"] + 4 * (k * nOb + j):lay["mu"] + 4 * (k * nOb + j) + 4] = mu; r0 += vj


def emu_pipeline(bt, i, r, duals):
    """instance i of the batch dict bt: upload, solve, refine x r, solve -- what a resident batch does, through the host builds.  Returns (coarse, status, fine, start) with
    coarse / fine = dict(x, u, t, lp, np, exitflag, iters), lambda in the caller's row scaling, and start = the numpy statement's refinement of the coarse solution."""
    import emu_solver as E
    solver = E.load(); per = isinstance(bt["vOb"], list)
    v, A, b = (np.asarray(bt[k][i] if per else bt[k]) for k in ("vOb", "A", "b")); v = v.astype(int); A = A.astype(float).reshape(-1, 2); b = b.astype(float)
    N = bt["N"]; Nf = r * N; nOb, M = len(v), int(v.sum()); xWS = bt["xWS"][i].copy(); xWS[0] = bt["x0"][i]
    prob = P.pack_problem(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], v, A, b, xWS[:, 0], xWS[:, 1], xWS[:, 2], 0)
    z0 = P.pack_start(N, nOb, M, xWS, bt["uWS"][i], np.zeros((N + 1, M)), np.zeros((N + 1, 4 * nOb)))

    def solve(n, p, z, opts):
        zo = np.zeros_like(z); info = np.zeros(8)
        solver.emu_solve(C.c_int(n), dp(p), dp(z), C.c_int(len(z)), C.byref(opts), dp(zo), dp(info))
        x, u, t, lp, npp, _ = P.unpack_solution(zo, n, nOb, M, A=A)
        return zo, info, dict(x=x, u=u, t=t, lp=lp, np=npp, exitflag=int(info[7]), iters=int(info[1]))
    zs = z0.copy(); emu_dualws_into(solver, zs, prob, N, v, A, b)
    zo, info, coarse = solve(N, prob, zs, E.default_opts())
    st, pd, zd = emu_record(dict(N=N, nOb=nOb, M=M, prob=prob, z=zo, z0=z0, info=info), r, duals, pad=0)
    pd = pd.copy(); zd = zd.copy(); opts = E.default_opts()
    if duals:
        opts.mu_init = opts.bound_push = opts.bound_frac = 1e-4      # api.warm_restart_opts()
    else:
        emu_dualws_into(solver, zd, pd, Nf, v, A, b)
    _, _, fine = solve(Nf, pd, zd, opts)
    start = V.refine_parking(coarse["x"], coarse["u"], coarse["t"], bt["Ts"][i], bt["L"], r, ref=xWS[:, :3].T, lam=coarse["lp"], mu=coarse["np"])
    return coarse, st, fine, dict(start, vOb=v, A=A, b=b)
