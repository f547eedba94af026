"""
Generates tests/golden/quad_refine_cases.npz (run from the repo root:  python tests/golden/make_quad_refine_cases.py): what refining a solved quadcopter batch onto a finer
horizon buys, with the CPU oracle (oracle/oracle_quad.py, default options), numpy and the host build of the refinement text only.

  make_quad_batch(16, 20) and make_quad_batch(8, 60), QuadcopterSignedDist, solved by the oracle           -> N<N>_x, _t, _exitflag, _iters
  their clearance record (validate.quad_clearance, need 0) at 8 samples per interval                       -> N<N>_rec
  for every case (N, factor r, margin) of quad_refine_common.FIXTURE_CASES: the refined problem (Ts / r, R + margin, warm start = the refined solution, timeWS = its t,
  closed-form duals) solved by the oracle, and the clearance record of that solution at 8 / r samples per fine interval -- the same sample density -- against R + margin with
  need = -margin, which is the true radius with need 0                                                     -> <case>_exitflag, _iters, _rec
The fine trajectories are not stored: tests/test_quad_refine_cpu.py solves again and compares the records.

The script asserts what the margin cases are there to show -- every instance ends with exit flag 1, no sample under the true R, the smallest clearance above 0 -- so a fixture
that does not show it cannot be written.  It prints one line per case; the test pins them.
"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)
from obca_amd import scenarios as S, validate as V   # noqa: E402
import oracle_quad as Q                              # noqa: E402
import quad_refine_common as R                       # noqa: E402
OUT = os.path.dirname(os.path.abspath(__file__))


def summary(rec):
    return "samples under 0: %d in %d instances, worst clearance %.6g" % (rec[:, 4].sum(), (rec[:, 4] > 0).sum(), rec[:, 0].min())


def main():
    out = {}; coarse = {}
    for N, B in sorted({(c[0], c[1]) for c in R.FIXTURE_CASES}):
        bt = S.make_quad_batch(B, N)
        sol = [Q.quadcopter_signed_dist(bt["x0"][i], bt["xF"][i], N, bt["Ts"], bt["R"], bt["ob"], bt["xWS"][i], bt["timeWS"]) for i in range(B)]
        rec = np.array([V.quad_clearance(s["xp"], s["t"], bt["Ts"], bt["ob"], bt["R"], R.S_COARSE) for s in sol])
        coarse[N] = (bt, sol)
        out.update({"N%d_x" % N: np.array([s["xp"] for s in sol]), "N%d_t" % N: np.array([s["t"] for s in sol]), "N%d_exitflag" % N: np.array([s["exitflag"] for s in sol]),
                    "N%d_iters" % N: np.array([s["iters"] for s in sol]), "N%d_rec" % N: rec})
        assert (out["N%d_exitflag" % N] == 1).all()
        print("make_quad_batch(%d, %d), no refinement: %s; iterations %s" % (B, N, summary(rec), out["N%d_iters" % N].tolist()))
    for N, B, r, margin in R.FIXTURE_CASES:
        bt, sol = coarse[N]
        fine = [R.oracle_fine(Q, bt, i, sol[i]["xp"], sol[i]["t"], r, margin) for i in range(B)]
        ef = np.array([q["exitflag"] for q, _ in fine]); it = np.array([q["iters"] for q, _ in fine]); rec = np.array([c for _, c in fine])
        key = R.case_key(N, r, margin)
        out.update({key + "_exitflag": ef, key + "_iters": it, key + "_rec": rec})
        print("make_quad_batch(%d, %d), factor %d, margin %g: exit flags %s, %s (against the true R: %.6g); iterations %s"
              % (B, N, r, margin, ef.tolist(), summary(rec), rec[:, 0].min() + margin, it.tolist()))
        if margin:
            assert (ef == 1).all() and (rec[:, 4] == 0).all() and rec[:, 0].min() + margin > 0, key
    np.savez_compressed(os.path.join(OUT, "quad_refine_cases.npz"), cases=np.array(R.FIXTURE_CASES), substeps_coarse=R.S_COARSE, **out)


if __name__ == "__main__":
    main()
