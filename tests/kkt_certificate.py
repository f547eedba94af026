"""TEST INFRASTRUCTURE: the independent optimality certificate of a primal-dual point, and the one map from the solvers' iterate layouts to the variable order of the flat
restatements oracle/nlp_ref.py / nlp_ref_quad.py (torch autograd derivatives: nothing shared with the closed-form derivatives, the condensation or the Riccati recursion of the
kernels and the C oracle but the problem statement).

  first order   r = sigma grad f + J'y - zL + zU with the SOLVER's multipliers and the AUTOGRAD gradient and Jacobian; |r|_inf, the constraint violation |c|_inf and the
                complementarity max z_i * dist_i are held against IPOPT's termination thresholds by the tests; all multipliers of bounds >= 0;
  second order  the AUTOGRAD Hessian of the Lagrangian reduced to the null space of the Jacobian of the equality rows and the active bounds (z_i > dist_i): its extreme eigenvalues.

Used by tests/golden/make_kkt_pin.py, tests/golden/make_kkt_classes.py, tests/test_pin_cpu.py, tests/test_kkt_classes_cpu.py and the direction tests of tests/test_oracle_cpu.py."""
import numpy as np
import packing as P


def certificate(nlp, v, y, zL, zU, sigma=1.0):
    """v, y: primal point and equality multipliers in the ordering of `nlp`; zL, zU: bound multipliers per variable (0 where there is no bound),
    already multiplied by the bound's multiplicity (timeScale stands for N+1 copies); sigma: the factor on the objective the multipliers belong to
    (obj_scaling: the solve ran on sigma f).  `obj` of the result is f itself."""
    import torch
    g = sigma * torch.autograd.functional.jacobian(nlp.f, torch.tensor(v)).numpy()
    cval = nlp.c(torch.tensor(v)).numpy()
    J = torch.autograd.functional.jacobian(nlp.c, torch.tensor(v), vectorize=True).numpy()
    lb, ub = nlp.lb, nlp.ub; n = len(v); mult = getattr(nlp, "mult", np.ones(n))
    r = g + J.T @ y - zL + zU
    hasL = np.isfinite(lb) & (ub > lb); hasU = np.isfinite(ub) & (ub > lb)
    dL = np.where(hasL, v - lb, np.inf); dU = np.where(hasU, ub - v, np.inf)
    with np.errstate(invalid="ignore"):      # (0 * inf where there is no bound: masked)
        compl = max(np.where(hasL, zL * dL / mult, 0).max(), np.where(hasU, zU * dU / mult, 0).max())
    act = np.flatnonzero((hasL & (zL / mult > dL)) | (hasU & (zU / mult > dU)))
    yt = torch.tensor(y)
    H = torch.autograd.functional.hessian(lambda w: sigma * nlp.f(w) + (yt * nlp.c(w)).sum(), torch.tensor(v), vectorize=True).numpy()
    Ea = np.zeros((len(act), n)); Ea[np.arange(len(act)), act] = 1.0
    Jall = np.vstack([J, Ea])
    U, s, Vt = np.linalg.svd(Jall, full_matrices=True)
    rank = int((s > 1e-9 * s[0]).sum())
    Z = Vt[rank:].T
    ev = np.linalg.eigvalsh(Z.T @ H @ Z)
    return dict(obj=float(nlp.f(torch.tensor(v)).item()), cviol=float(np.abs(cval).max()), kkt=float(np.abs(r).max()), y_inf=float(np.abs(y).max()),
                z_min=float(min(zL[hasL].min(), zU[hasU].min() if hasU.any() else np.inf)), compl_max=float(compl), bound_viol=float(max((-dL[hasL]).max(), (-dU[hasU]).max() if hasU.any() else -1)),
                n=n, m=int(J.shape[0]), n_active=int(len(act)), rank=rank, redhess_min=float(ev.min()), redhess_max=float(ev.max()))


def first_order(nlp, v, y, zL, zU, sigma=1.0):
    """(|sigma grad f + J'y - zL + zU|_inf, |c|_inf, complementarity): the first-order part of `certificate` alone (no Hessian, no SVD)"""
    import torch
    g = sigma * torch.autograd.functional.jacobian(nlp.f, torch.tensor(v)).numpy()
    J = torch.autograd.functional.jacobian(nlp.c, torch.tensor(v), vectorize=True).numpy()
    lb, ub = nlp.lb, nlp.ub; mult = getattr(nlp, "mult", np.ones(len(v)))
    hasL = np.isfinite(lb) & (ub > lb); hasU = np.isfinite(ub) & (ub > lb)
    dL = np.where(hasL, v - lb, np.inf); dU = np.where(hasU, ub - v, np.inf)
    with np.errstate(invalid="ignore"):      # (0 * inf where there is no bound: masked)
        compl = max(np.where(hasL, zL * dL / mult, 0).max(), np.where(hasU, zU * dU / mult, 0).max())
    return float(np.abs(g + J.T @ y - zL + zU).max()), float(np.abs(nlp.c(torch.tensor(v)).numpy()).max()), float(compl)


def parking_point(z, N, vOb, nlp, dist, multiplicity=True):
    """iterate z in the layout of packing.layout (= oracle.layout) -> (v, y, zL, zU) in the variable order of oracle/nlp_ref.py: x_0 dropped, multipliers of infinite
    bounds (psi; the penetration slack of ParkingSignedDist) zeroed, zs1 -- the multiplier of the norm-row slack's bound -- only in the ParkingDist formulation.
    multiplicity: the time scale's bound multipliers times N + 1 (one t stands for the reference's N + 1 copies), as `certificate` takes them; False leaves them per copy
    (the direction tests apply nlp.mult themselves).  A direction d in the same layout maps the same way: its primal and multiplier parts are v and y."""
    v_ = np.ravel(vOb).astype(int); nOb = len(v_); M = int(v_.sum()); N1 = N + 1
    assert int(nlp.dist) == int(bool(dist)) and nlp.N == N and nlp.M == M
    Lz = P.layout(N, nOb, M); z = np.asarray(z, float)
    seg = lambda k, cnt: z[Lz[k]:Lz[k] + cnt]
    v = np.zeros(nlp.n); zL = np.zeros(nlp.n); zU = np.zeros(nlp.n)
    v[nlp.ix] = seg("x", 4 * N1)[4:]; v[nlp.it] = z[Lz["t"]]; v[nlp.iu] = seg("u", 2 * N); v[nlp.il] = seg("lam", M * N1); v[nlp.im] = seg("mu", 4 * nOb * N1)
    v[nlp.isl] = seg("sl", nOb * N1); v[nlp.iss] = seg("ss", N); v[nlp.iso] = seg("so", nOb * N1)
    zL[nlp.ix] = seg("zxL", 4 * N1)[4:]; zU[nlp.ix] = seg("zxU", 4 * N1)[4:]
    k = N1 if multiplicity else 1
    zL[nlp.it] = k * z[Lz["ztL"]]; zU[nlp.it] = k * z[Lz["ztU"]]
    zL[nlp.iu] = seg("zuL", 2 * N); zU[nlp.iu] = seg("zuU", 2 * N); zL[nlp.il] = seg("zlam", M * N1); zL[nlp.im] = seg("zmu", 4 * nOb * N1)
    zL[nlp.iss] = seg("zssL", N); zU[nlp.iss] = seg("zssU", N); zL[nlp.iso] = seg("zso", nOb * N1)
    if dist:
        zL[nlp.isl] = seg("zs1", nOb * N1)
    zL[~np.isfinite(nlp.lb)] = 0; zU[~np.isfinite(nlp.ub)] = 0
    y = np.concatenate([seg("pi", 4 * N), seg("nu", 4), seg("yg", N), seg("yo", 4 * nOb * N1)])
    return v, y, zL, zU


DIRECTION_CASES = ("shipped", "rows_5_to_8", "rows_5_to_8_as_emitted", "16_obstacles")


def direction_obstacles(case):
    """(vOb, A, b) of the obstacle sets the direction tests run on, one per instantiation of the kernels' obstacle block:
      shipped                  the backwards scenario, rows 2, 2, 1: the 2-row class, whose Householder-reduced Hessian is 1 x 1, 15 block items at N = 4;
      rows_5_to_8              rows 2, 2, 1, 5, 6, 7, 7: the widest class (LDL' of up to 6 x 6), 35 items at N = 4; rows at unit length -- the iterate holds lambda of unit rows;
      rows_5_to_8_as_emitted   the same rows as obst_hrep emits them (up to 9.7 long): for the oracle's hooks alone, which take rows as they come;
      16_obstacles             16 obstacles of 3-4 rows: the middle class, 80 items at N = 4 -- two rounds of 64 lanes in the kernels; unit rows."""
    from obca_amd import scenarios as S
    if case == "shipped":
        A, b, v = S.scenario_hrep(S.BACKWARDS)
        return np.ravel(v).astype(int), np.asarray(A, float), np.asarray(b, float)
    if case.startswith("rows_5_to_8"):
        bt = S.make_mixed_batch(24, 40, seed=11, rows=(5, 8), max_extra=4); i = 3
        assert np.ravel(bt["vOb"][i]).tolist() == [2, 2, 1, 5, 6, 7, 7]
    else:
        assert case == "16_obstacles", case
        bt = S.make_mixed_batch(40, 40, seed=5, max_extra=13, rows=(3, 4), max_rows=64)
        i = [k for k, v in enumerate(bt["vOb"]) if len(v) == 16][0]
        assert 3 <= np.min(bt["vOb"][i][3:]) and np.max(bt["vOb"][i]) == 4
    v = np.ravel(bt["vOb"][i]).astype(int); A = np.asarray(bt["A"][i], float).reshape(-1, 2); b = np.ravel(np.asarray(bt["b"][i], float))
    if case.endswith("as_emitted"):
        assert P.row_lengths(A).max() > 5
        return v, A, b
    rl = P.row_lengths(A)
    return v, A / rl[:, None], b / rl


def quad_point(z, N, nlp):
    """iterate z = v | y | zL | zU of packing.quad_layout (the kernels' and the oracle's: x with x_0 first | u | t | lam | s | so) -> (v, y, zL, zU) in the variable order of
    oracle/nlp_ref_quad.py: x_0 dropped, the time scale's bound multipliers times N + 1, multipliers of infinite bounds zeroed"""
    L = P.quad_layout(N); n, m = L["n"], L["m"]; z = np.asarray(z, float)
    assert len(z) == L["len"] and nlp.n == n - 12 and nlp.m == m
    keep = np.arange(12, n)
    v = z[:n][keep].copy(); y = z[n:n + m].copy(); zL = z[L["zL"]:L["zL"] + n][keep].copy(); zU = z[L["zU"]:L["zU"] + n][keep].copy()
    zL[nlp.it] *= N + 1; zU[nlp.it] *= N + 1
    zL[~np.isfinite(nlp.lb)] = 0; zU[~np.isfinite(nlp.ub)] = 0
    return v, y, zL, zU
