"""
Generates tests/golden/kkt_classes.npz: independent optimality certificates of the KERNEL TEXT's own optima, in the classes tests/golden/kkt_pin.npz does not reach.

kkt_pin.npz certifies the C oracle's multipliers on signed-distance solutions of the shipped scenarios.  Here every record is the final primal-dual iterate of the host build of
the kernel text (tests/emu_solver.py: emu_solve / emu_quad_solve) at N = 20, certified with the autograd derivatives of oracle/nlp_ref.py / nlp_ref_quad.py
(tests/kkt_certificate.py), for (tests/kkt_classes_common.py: specs)

  backwards   the shipped scenario, ParkingSignedDist and ParkingDist, throughput defaults and the reference configuration;
  wide        obstacles of 5-8 rows (rows 2, 2, 1, 5, 6, 7, 7 and 2, 2, 1, 7, 7): the widest instantiation of the obstacle block, both formulations;
  corridor    wedges intruding 0.15 m into the warm start's swept body: the DualMultWS start has degenerate blocks (|A'lambda|^2 < 1/4) and the block restoration fires -- the
              generator asserts that it did (the start is degenerate, and the run with restoration = 0 takes another number of iterations); instance 1 is left out: its
              ParkingDist runs end at max_iter;
  quad        both quadcopter instances, QuadcopterSignedDist and QuadcopterDist, throughput options and the reference options; with obj_scaling the multipliers belong to
              sigma f and the certificate is that of sigma f (sigma from the autograd gradient at the kernel's starting point).  One of the eight solves is taken from
              another batch, because two roundings of its iteration end 1e-3 apart (kkt_classes_common.specs says which and why).

Second order: for ParkingDist and both quadcopter formulations the smallest eigenvalue of the reduced Hessian is measured against the same figure of the ORACLE's full iterate of
the same instance (stored beside it); signed-distance parking records keep the rule of tests/test_pin_cpu.py.
Stored per record: inputs, the full iterate, xp / up / t as returned (lambda, mu and the slacks are slices of the iterate), status, exit flag, iteration and regularisation
counts, the certificate, the oracle's exit flag / iteration count / eigenvalues, and for the corridor records the start's degenerate blocks and the run with restoration = 0.
The certificate is that of the iterate as the host build left it, every bit (the test re-runs the host build and certifies that iterate again, live).  The STORED copy of the
iterate -- what re-runs, the oracle and the HIP path are compared with -- is in fixed point with 36 fractional bits: 1.5e-11 apart, two orders below the 1e-9 it is compared
at.  Full doubles do not compress, and the 23 iterates (62 000 numbers) would make this file half again as large as kkt_pin.npz.  (Certifying the stored copy instead moves
the first-order residual of the signed-distance records from 1e-12 to 1.4e-7: the slack's curvature of 2e4 times 7e-12.)
The file is written with fixed time stamps: a second run reproduces it bit for bit.
Run from the repo root (about 15 s on 8 cores):  python tests/golden/make_kkt_classes.py
"""
import os
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):      # one thread per worker process: the same sums in the same order, run after run
    os.environ[_v] = "1"
import io
import sys
import time
import zipfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.dirname(os.path.abspath(__file__))

import kkt_classes_common as K      # noqa: E402

FRACTION_BITS = 36


def job(spec):
    import torch
    torch.set_num_threads(1)
    tag, idx, dist, ref, restoration = spec
    t0 = time.time()
    q = K.inputs(tag, idx)
    r = dict(tag=tag, idx=idx, dist=dist, ref=ref, restoration=restoration, N=K.N, **q)
    e = K.solve_emu(r)
    assert e["status"] == 0 and e["exitflag"] == 1, (spec, e["status"], e["exitflag"])
    z = np.rint(e["z"] * 2.0 ** FRACTION_BITS) / 2.0 ** FRACTION_BITS
    assert np.abs(e["z"]).max() < 2.0 ** 16 and np.abs(z - e["z"]).max() <= 2.0 ** -(FRACTION_BITS + 1)
    xp, up, t = K.returned(r, z)
    r.update(z=z, status=e["status"], exitflag=e["exitflag"], iters=e["iters"], nreg=e["nreg"], solver_obj=e["obj"], xp=xp, up=up, t=t)
    r.update(K.certify(r, e["z"]))      # of the iterate as the host build left it, every bit
    o = K.solve_oracle(r, full=True)
    oxp, oup, ot = K.returned(r, o["z"])
    r.update(oracle_exitflag=int(o["exitflag"]), oracle_iters=int(o["iters"]), oracle_dx=float(np.abs(oxp - xp).max()), oracle_du=float(np.abs(oup - up).max()), oracle_dt=abs(ot - t),
             oracle_dobj=abs(o["obj"] - e["obj"]) / max(1.0, abs(e["obj"])))
    if K.yardstick_is_the_oracle(r):
        c = K.certify(r, o["z"])
        r.update(oracle_redhess_min=c["redhess_min"], oracle_redhess_max=c["redhess_max"], oracle_kkt=c["kkt"])
    if tag == "corridor":
        e0 = K.solve_emu(r, restoration=0)
        r.update(deg_start=K.degenerate_blocks(q, e["lWS"]), rest0_status=e0["status"], rest0_exitflag=e0["exitflag"], rest0_iters=e0["iters"], rest0_obj=e0["obj"])
        assert r["deg_start"] >= 1 and r["rest0_iters"] != r["iters"], (spec, r["deg_start"], r["rest0_iters"], r["iters"])
    r["seconds"] = time.time() - t0
    return r


def table(recs):
    lines = ["record | rows | status ef iters nreg | objective | first order: |r| |c| compl | min z | bound viol | solver obj rel. | reduced Hessian min / max | oracle's min / max | oracle: ef iters |dx| |"
             " restoration: degenerate blocks at the start, run with restoration = 0"]
    for r in recs:
        rows = "-" if K.is_quad(r) else ",".join(map(str, r["vOb"]))
        s = "%s | %s | %d %d %d %d | %.6f | %.2e %.2e %.2e | %.1e | %.1e | %.1e | %.3e / %.3e | " % (
            K.name(r), rows, r["status"], r["exitflag"], r["iters"], r["nreg"], r["solver_obj"], r["kkt"], r["cviol"], r["compl_max"], r["z_min"], r["bound_viol"],
            abs(r["obj"] - r["solver_obj"]) / max(1.0, abs(r["obj"])), r["redhess_min"], r["redhess_max"])
        s += ("%.3e / %.3e" % (r["oracle_redhess_min"], r["oracle_redhess_max"])) if "oracle_redhess_min" in r else "-"
        s += " | %d %d %.1e" % (r["oracle_exitflag"], r["oracle_iters"], r["oracle_dx"])
        if r["tag"] == "corridor":
            s += " | %d, %d iterations (status %d, objective %.6g)" % (r["deg_start"], r["rest0_iters"], r["rest0_status"], r["rest0_obj"])
        if K.is_quad(r) and r["ref"]:
            s += " | sigma %.6f" % r["sigma"]
        lines.append(s)
    return "\n".join(lines)


def save(path, recs):
    """np.savez_compressed with fixed time stamps: the same records give the same bytes"""
    buf = io.BytesIO(); np.lib.format.write_array(buf, np.array(recs, dtype=object), allow_pickle=True)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        zi = zipfile.ZipInfo("records.npy", date_time=(1980, 1, 1, 0, 0, 0)); zi.compress_type = zipfile.ZIP_DEFLATED; zi.external_attr = 0o600 << 16
        zf.writestr(zi, buf.getvalue())


def dist_restoration_census():
    """for the record (no assertion): what restoration = 1 costs on the corridor instances in the ParkingDist formulation, where no block needs it"""
    out = []
    for i in (0, 2, 3):
        q = K.inputs("corridor", i)
        out.append(tuple(K.emu_parking(q, 1, 1, rest)["iters"] for rest in (1, 0)))
    return out


def main():
    import multiprocessing as mp
    import emu_solver, oracle as O, oracle_quad as Q
    emu_solver.load(); O.build(); Q.lib()      # build once, before the workers start
    specs = K.specs()
    with mp.get_context("fork").Pool(min(8, len(specs))) as pool:
        recs = pool.map(job, specs, chunksize=1)
        census = pool.apply(dist_restoration_census)
    print(table(recs))
    print("corridor instances 0, 2, 3 in the ParkingDist formulation, reference configuration: iterations with restoration = 1 against restoration = 0: %s"
          % ", ".join("%d against %d" % c for c in census))
    print("seconds per record: %s" % " ".join("%.0f" % r.pop("seconds") for r in recs))
    save(os.path.join(OUT, "kkt_classes.npz"), recs)
    print("wrote kkt_classes.npz: %d records, %d bytes" % (len(recs), os.path.getsize(os.path.join(OUT, "kkt_classes.npz"))))


if __name__ == "__main__":
    main()
