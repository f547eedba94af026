"""What the NLP makes of the device planner's paths, by bucket width: the host build of the device search (tests/emu/hybrid_emu.cpp) against the host planner on config-3 poses
(parallel scenario, goal jitter), both judged by the oracle.  CPU only; minutes of oracle time.

    python tools/hybrid_quality.py [--out profiles/hybrid_quality_cpu.json] [--instances 256] [--N 80] [--widths 0.025 0.05 0.1 0.2] [--workers 8]

Per bucket width: paths found, path cost (length in metres and direction switches, mean), expansions and rounds (mean / max), and the oracle's solved count and mean
iterations from the plans' warm starts at the throughput options; the same for the host planner.  VERDICT's criterion: mean iterations at most 1.10 x the host planner's;
the default width (OBCA_HYBRID_DEFAULT_WIDTH) is the largest swept width that keeps it."""
import argparse
import json
import multiprocessing as mp
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from obca_amd import planner as PL, scenarios as S


def solve(job):
    import oracle as O
    x0, xF, path, dirs, N, v_nom = job
    v, A, b = _FIELD
    Ts, xWS, uWS = PL.path_to_warm_start(path, dirs, N, xF, v_nom=v_nom)
    xWS = xWS.copy(); xWS[0] = x0
    r = O.parking_signed_dist(x0, xF, N, Ts, S.L_WHEELBASE, S.EGO, S.XYBOUNDS, v, A, b, xWS[:, 0], xWS[:, 1], xWS[:, 2], 0, xWS, uWS, opts=O.default_opts())
    return int(r["exitflag"]), int(r["iters"])


def stats(paths, dirs, cnt, nexp, rounds, x0, xF, N, v_nom, pool):
    ok = np.flatnonzero(cnt > 0)
    length = [float(np.hypot(np.diff(paths[i, :cnt[i], 0]), np.diff(paths[i, :cnt[i], 1])).sum()) for i in ok]
    sw = [int(np.count_nonzero(np.diff(dirs[i, :cnt[i]]))) for i in ok]
    res = pool.map(solve, [(x0[i], xF[i], paths[i, :cnt[i]].copy(), dirs[i, :cnt[i]].copy(), N, v_nom) for i in ok])
    flags = np.array([r[0] for r in res]); its = np.array([r[1] for r in res])
    e = dict(with_path=int(len(ok)), length_mean=float(np.mean(length)), switches_mean=float(np.mean(sw)), expansions_mean=float(nexp[ok].mean()), expansions_max=int(nexp[ok].max()),
             oracle_solved=int((flags == 1).sum()), oracle_iterations_mean=float(its.mean()), oracle_iterations_mean_solved=float(its[flags == 1].mean()), oracle_iterations_max=int(its.max()))
    if rounds is not None:
        e.update(rounds_mean=float(rounds[ok].mean()), rounds_max=int(rounds[ok].max()))
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/hybrid_quality_cpu.json")
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--N", type=int, default=80)
    ap.add_argument("--widths", type=float, nargs="+", default=[0.025, 0.05, 0.1, 0.2])
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    import hybrid_common as H
    import oracle as O
    O.build()
    global _FIELD
    sc = S.PARALLEL; kw, v_nom = PL.SCENARIO_OPTS["parallel"]
    _FIELD = H.field(sc)
    x0, xF = S.sample_poses(sc, a.instances, np.random.default_rng(3), goal_jitter=True)
    out = dict(scenario="parallel, goal jitter (config 3)", instances=a.instances, N=a.N, options=kw, criterion="oracle_iterations_mean <= 1.10 x host planner's", entries=[])
    with mp.get_context("fork").Pool(a.workers) as pool:
        h = PL._hybrid_astar_dense(x0, xF, *_FIELD, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, 0, H.CAP, kw)
        host = stats(h[2], h[3], h[4], h[5], None, x0, xF, a.N, v_nom, pool); host["planner"] = "host"
        out["entries"].append(host); print(json.dumps(host), flush=True)
        for bw in a.widths:
            r = H.run_emu(sc, x0, xF, kw, bw=bw, nodes=1 << 20)
            e = stats(r["paths"], r["dirs"], r["counts"], r["expansions"], r["rounds"], x0, xF, a.N, v_nom, pool)
            e.update(planner="device design (host build)", bucket_width=bw, limit_hits=int((r["counts"] == -3).sum()), iterations_ratio_to_host=e["oracle_iterations_mean"] / host["oracle_iterations_mean"],
                     keeps_criterion=bool(e["oracle_iterations_mean"] <= 1.10 * host["oracle_iterations_mean"] and e["oracle_solved"] >= host["oracle_solved"]))
            out["entries"].append(e); print(json.dumps(e), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


_FIELD = None
if __name__ == "__main__":
    main()
