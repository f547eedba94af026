"""TEST INFRASTRUCTURE of tests/golden/make_kkt_classes.py, tests/test_kkt_classes_cpu.py and the GPU tests on tests/golden/kkt_classes.npz: which solves the fixture records, how the
host build of the kernel text (tests/emu_solver.py) and the C oracle run them, and how a record's final iterate is certified with the autograd derivatives of oracle/nlp_ref*.py
(tests/kkt_certificate.py).  Every record is at N = 20: the smallest horizon at which these instances still solve in 20-90 iterations, and
with at least 4 obstacles it has more than 64 (stage, obstacle) block items."""
import numpy as np
import packing as P
from kkt_certificate import certificate, first_order, parking_point, quad_point
from obca_amd import scenarios as S

N = 20
TOL, CVIOL, COMPL = 1e-5, 1e-4, 1e-4          # tol, constr_viol_tol, compl_inf_tol of the reference's IPOPT call, as in tests/test_pin_cpu.py


def specs():
    """(tag, instance, dist, ref, restoration) of every record: ref = 0 the throughput defaults, 1 the reference configuration (parking: max_soc = 4, recalc_y, lsq_init and the
    block restoration; quadcopter: max_soc = 4, lsq_init, obj_scaling)"""
    out = [("backwards", 0, d, r, r) for d in (0, 1) for r in (0, 1)]
    out += [("wide", i, d, r, r) for d in (0, 1) for i, r in ((3, 0), (3, 1), (6, 0))]
    out += [("corridor", 0, 0, 1, 1), ("corridor", 2, 0, 1, 1), ("corridor", 3, 0, 1, 1), ("corridor", 3, 0, 1, 2), ("corridor", 2, 1, 1, 1)]
    # quadcopter: both instances of make_quad_batch(2, N).  One swap: instance 0 (the shipped scenario) under QuadcopterSignedDist with the reference options spends its
    # last 40 of 82 iterations at mu = 1e-6 with an inertia correction in every one, and two roundings of the same iteration (host build, C oracle: same 82 iterations) end
    # 1.0e-3 apart in the states, 6.7e-5 in the inputs -- outside the tolerances a fixed array is compared at.  Instance 3 of make_quad_batch(6, N) stands in (53 iterations,
    # the two agree to 3e-13), so that two records still carry sigma = 100 / 2100.
    out += [("quad6", 3, d, r, 0) if (i, d, r) == (0, 0, 1) else ("quad", i, d, r, 0) for i in (0, 1) for d in (0, 1) for r in (0, 1)]
    return out


def is_quad(r):
    return r["tag"].startswith("quad")


def name(r):
    return "%s-%d-%s-%s" % (r["tag"], r["idx"], "dist" if r["dist"] else "signed_dist", ("reference" + ("" if r["restoration"] == r["ref"] or is_quad(r) else "_restoration_%d" % r["restoration"])) if r["ref"] else "defaults")


def yardstick_is_the_oracle(r):
    """second order: signed-distance parking records keep the rule of tests/test_pin_cpu.py (their slack curvature of 1e4 sets the scale); ParkingDist and both quadcopter
    formulations have flat directions that end at -2e-4 .. -9e-4 against a largest eigenvalue of 0.7 .. 2, and are measured against the oracle's iterate of the same instance"""
    return is_quad(r) or bool(r["dist"])


_BATCHES = {}


def inputs(tag, i):
    """the inputs of instance i of the batch behind `tag`, as the fixture stores them"""
    if tag not in _BATCHES:
        _BATCHES[tag] = (S.make_batch(S.BACKWARDS, 2, N) if tag == "backwards" else S.make_mixed_batch(24, N, seed=11, rows=(5, 8), max_extra=4) if tag == "wide"
                         else S.make_corridor_batch(8, N, seed=11, clearance=(-0.15, 0.2)) if tag == "corridor" else S.make_quad_batch({"quad": 2, "quad6": 6}[tag], N))
    bt = _BATCHES[tag]
    if tag.startswith("quad"):
        return dict(x0=np.asarray(bt["x0"][i], float), xF=np.asarray(bt["xF"][i], float), Ts=float(bt["Ts"]), R=float(bt["R"]), ob=np.asarray(bt["ob"], float), xWS=np.asarray(bt["xWS"][i], float).reshape(N + 1, 12))
    ragged = isinstance(bt["vOb"], list)
    v, A, b = (bt["vOb"][i], bt["A"][i], bt["b"][i]) if ragged else (bt["vOb"], bt["A"], bt["b"])
    xWS = np.array(bt["xWS"][i], float); xWS[0] = bt["x0"][i]
    return dict(x0=np.asarray(bt["x0"][i], float), xF=np.asarray(bt["xF"][i], float), Ts=float(bt["Ts"][i]), xWS=xWS, uWS=np.asarray(bt["uWS"][i], float)[:N],
                vOb=np.ravel(v).astype(int), A=np.asarray(A, float).reshape(-1, 2), b=np.ravel(np.asarray(b, float)))


def _unit_rows(q):
    rl = P.row_lengths(q["A"])
    return q["A"] / rl[:, None], q["b"] / rl, rl


# ---------------------------------------------------------------- parking
def _parking_switches(ref):
    return dict(max_soc=4, recalc_y=1, lsq_init=1) if ref else {}


def emu_parking(q, dist, ref, restoration):
    """the host build of the kernel text (its own DualMultWS start): full iterate z (packing.layout, lambda of unit rows), info record, the start's lambda"""
    import emu_solver as E
    xWS = q["xWS"]
    r = E.parking_signed_dist_batch(q["x0"][None], q["xF"][None], N, [q["Ts"]], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, q["vOb"], q["A"], q["b"], xWS[None, :, 0], xWS[None, :, 1], xWS[None, :, 2], 0,
                                    xWS[None], q["uWS"][None], dist=bool(dist), restoration=restoration, **_parking_switches(ref))
    info = r["info"][0]
    return dict(z=r["z"][0], status=int(info[0]), iters=int(info[1]), obj=float(info[2]), nreg=int(info[6]), exitflag=int(info[7]), lWS=r["lWS"][0])


def oracle_parking(q, dist, ref, restoration, full=False):
    """the C oracle with the same options; with full, z is its final iterate brought to the kernels' convention (lambda and its bound multipliers of unit rows)"""
    import oracle as O
    oo = O.default_opts()
    for k, v in _parking_switches(ref).items():
        setattr(oo, k, v)
    oo.restoration = restoration
    xWS = q["xWS"]
    r = O.parking_signed_dist(q["x0"], q["xF"], N, q["Ts"], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, q["vOb"], q["A"], q["b"], xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, q["uWS"], opts=oo, dist=dist, full=full)
    if full:
        M = int(np.sum(q["vOb"])); L = P.layout(N, len(q["vOb"]), M); rl = P.row_lengths(q["A"]); z = r["zfull"].copy()
        z[L["lam"]:L["lam"] + M * (N + 1)] = (z[L["lam"]:L["lam"] + M * (N + 1)].reshape(N + 1, M) * rl).reshape(-1)
        z[L["zlam"]:L["zlam"] + M * (N + 1)] = (z[L["zlam"]:L["zlam"] + M * (N + 1)].reshape(N + 1, M) / rl).reshape(-1)
        r["z"] = z
    return r


def parking_nlp(q, dist):
    from nlp_ref import ParkingNLP
    An, bn, _ = _unit_rows(q); xWS = q["xWS"]
    return ParkingNLP(q["x0"], q["xF"], N, q["Ts"], S.L_WHEELBASE, S.EGO, S.XYBOUNDS, q["vOb"], An, bn, xWS[:, 0], xWS[:, 1], xWS[:, 2], dist=dist)


def degenerate_blocks(q, lWS):
    """(stage, obstacle) blocks of a DualMultWS start with |A'lambda|^2 < 1/4 (the start-of-solve trigger of the block restoration): lambda = 0 on a penetrating pose"""
    An, _, _ = _unit_rows(q); off = np.r_[0, np.cumsum(q["vOb"])]; lWS = np.asarray(lWS, float).reshape(N + 1, -1)
    return int(sum((((lWS[:, off[j]:off[j + 1]] @ An[off[j]:off[j + 1]]) ** 2).sum(1) < 0.25).sum() for j in range(len(q["vOb"]))))


def pushing_lambda(q, z, rows=None):
    """index into z of one lambda, for the mutation checks: in the (stage, obstacle) block whose separation row carries the largest multiplier -- where the obstacle pushes on
    the car, and A'lambda enters the stationarity of the pose with that weight -- the largest lambda.  rows: among the obstacles of that many rows only"""
    v = q["vOb"]; nOb = len(v); M = int(v.sum()); L = P.layout(N, nOb, M); off = np.r_[0, np.cumsum(v)]
    y4 = np.abs(z[L["yo"]:L["yo"] + 4 * nOb * (N + 1)].reshape(N + 1, nOb, 4)[:, :, 3])
    if rows is not None:
        y4[:, v != rows] = -1.0
    k, j = np.unravel_index(np.argmax(y4), y4.shape)
    r = int(np.argmax(z[L["lam"] + k * M + off[j]:L["lam"] + k * M + off[j + 1]]))
    return L["lam"] + k * M + off[j] + r


# ---------------------------------------------------------------- quadcopter
def _quad_switches(ref):
    return dict(max_soc=4, lsq_init=1, obj_scaling=1) if ref else {}


def emu_quad(q, dist, ref):
    import emu_solver as E
    r = E.quadcopter_signed_dist_batch(q["x0"][None], q["xF"][None], N, q["Ts"], q["R"], q["ob"], q["xWS"][None], 1.0, dist=bool(dist), **_quad_switches(ref))
    info = r["info"][0]
    return dict(z=r["z"][0], status=int(info[0]), iters=int(info[1]), obj=float(info[2]), nreg=int(info[6]), exitflag=int(info[7]))


def oracle_quad(q, dist, ref):
    """the C oracle with the same options; z = v | y | zL | zU of its final iterate (the layout of packing.quad_layout)"""
    import oracle_quad as Q
    oo = Q.default_opts()
    for k, v in _quad_switches(ref).items():
        setattr(oo, k, v)
    r = Q.quadcopter_signed_dist_full(q["x0"], q["xF"], N, q["Ts"], q["R"], q["ob"], q["xWS"], 1.0, opts=oo, dist=dist)
    r["z"] = r["full"]
    return r


def quad_nlp(q, dist):
    from nlp_ref_quad import QuadNLP
    return QuadNLP(q["x0"], q["xF"], N, q["Ts"], q["R"], q["ob"], dist=bool(dist))


def quad_start(q, dist, nlp):
    """the point the quadcopter kernel starts from, in the variable order of oracle/nlp_ref_quad.py: x = xWS, u at hover, t = timeWS = 1, slack 1 (none in QuadcopterDist), lambda the
    closed-form dual of the point-to-box distance at the warm-start position (unit vector from the box to the point; inside a box the normal of its nearest face)"""
    v = np.zeros(nlp.n); v[nlp.ix] = q["xWS"][1:].reshape(-1); v[nlp.iu] = nlp.wH; v[nlp.it] = 1.0; v[nlp.isl] = 0.0 if dist else 1.0
    lam = np.zeros((N + 1, 5, 6)); hi = q["ob"][:, :3]; lo = -q["ob"][:, 3:]
    for k in range(N + 1):
        p = q["xWS"][k, :3]
        for j in range(5):
            d = p - np.clip(p, lo[j], hi[j]); u = np.zeros(3)
            if d @ d > 1e-16:
                u = d / np.sqrt(d @ d)
            else:
                gap = np.concatenate([hi[j] - p, p - lo[j]]); f = int(np.argmin(gap)); u[f % 3] = 1.0 if f < 3 else -1.0
            lam[k, j] = np.concatenate([np.maximum(u, 0), np.maximum(-u, 0)])
    v[nlp.il] = lam.reshape(-1)
    return v


def quad_sigma(q, dist, ref, nlp):
    """obj_scaling (IPOPT's gradient-based scaling, nlp_scaling_max_gradient = 100): the solve runs on sigma f with sigma = min(1, 100 / |grad f(start)|_inf over the variables of the
    reference's model -- each of its N + 1 time-scale variables carries 1 / (N + 1) of the one t here --, from the AUTOGRAD gradient; the multipliers returned belong to sigma f"""
    if not ref:
        return 1.0
    import torch
    g = torch.autograd.functional.jacobian(nlp.f, torch.tensor(quad_start(q, dist, nlp))).numpy() / nlp.mult
    return float(min(1.0, 100.0 / np.abs(g).max()))


# ---------------------------------------------------------------- one record
def solve_emu(r, q=None, restoration=None):
    q = r if q is None else q
    return emu_quad(q, r["dist"], r["ref"]) if is_quad(r) else emu_parking(q, r["dist"], r["ref"], r["restoration"] if restoration is None else restoration)


def solve_oracle(r, q=None, full=False):
    q = r if q is None else q
    return oracle_quad(q, r["dist"], r["ref"]) if is_quad(r) else oracle_parking(q, r["dist"], r["ref"], r["restoration"], full=full)


def point(r, z, q=None):
    """(nlp, sigma, (v, y, zL, zU)) of the iterate z of record r"""
    q = r if q is None else q
    if is_quad(r):
        nlp = quad_nlp(q, r["dist"])
        return nlp, quad_sigma(q, r["dist"], r["ref"], nlp), quad_point(z, N, nlp)
    nlp = parking_nlp(q, r["dist"])
    return nlp, 1.0, parking_point(z, N, q["vOb"], nlp, r["dist"])


def certify(r, z, q=None):
    nlp, sigma, pt = point(r, z, q)
    return dict(certificate(nlp, *pt, sigma=sigma), sigma=sigma)


def returned(r, z):
    """what the solvers hand back of the iterate z: xp, up, t"""
    if is_quad(r):
        L = P.quad_layout(N)
        return z[L["x"]:L["u"]].reshape(N + 1, 12).T.copy(), z[L["u"]:L["t"]].reshape(N, 4).T.copy(), float(z[L["t"]])
    v = r["vOb"]
    return P.unpack_solution(z, N, len(v), int(np.sum(v)))[:3]


__all__ = ["N", "TOL", "CVIOL", "COMPL", "specs", "name", "inputs", "solve_emu", "solve_oracle", "point", "certify", "first_order", "returned", "degenerate_blocks", "pushing_lambda",
           "yardstick_is_the_oracle"]
