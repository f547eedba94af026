"""Cost of the closed-loop ensemble (Batch.ensemble / QuadBatch.ensemble, include/obca_ensemble.h: one wavefront per instance, one member per lane, one launch) against the
only way to the same answer without it -- M calls of track() on the same batch, each of which recomputes the same gains with one integrating lane --, beside the solve it
follows; and what the ensemble shows on those solved batches: the distribution of the members' smallest clearance and of members_hit, the basis for choosing a
refine(margin=...).

    python tools/ensemble_rate.py [--out profiles/ensemble_device_vs_host.json] [--batches 1024 16384] [--quad-batches 256 1024] [--members 1 8 64] [--substeps 8]
                                  [--repeats 5] [--diffs FILE] [--step-timeout 600]

Config 2 (backwards parking, N = 80; 1 024 planned instances, repeated for the larger batch) and make_quad_batch(B, 60).  Every batch is measured by a child process of its
own under `--step-timeout` seconds (`--only KIND:B` is that child); the first one that fails or runs out of time ends the run.  Per batch and number of members M: the
ensemble kernel's time from HIP events and the wall time of ensemble() (medians of `repeats` after a warm-up call), the track kernel's time of the same batch (the kernel of
the parent commit, unchanged here) and M times it, ipm_ms; the wall time of ensemble_members() / ensemble_final().  The offsets are ensemble_offsets(B, M, SIGMA, seed=0):
parking (0.05 m, 0.05 m, 0.02 rad, 0.05 m/s); quadcopter 0.05 m, 0.01 rad, 0.05 m/s, 0.01 rad/s per axis; no input bias.  --diffs: the file tests/test_gpu_ensemble.py
leaves its largest differences in (OBCA_ENSEMBLE_DIFFS)."""
import argparse
import json
import os
import subprocess
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import obca_amd                                                     # noqa: E402
from obca_amd import scenarios as S                                 # noqa: E402
from rollout_rate import timed                                      # noqa: E402

SIGMA = {4: np.array([0.05, 0.05, 0.02, 0.05]), 12: np.r_[np.full(3, 0.05), np.full(3, 0.01), np.full(3, 0.05), np.full(3, 0.01)]}
PCT = (0, 1, 5, 25, 50, 75, 95, 99, 100)


def entries(b, cfg, B, N, nx, need, ipm_ms, solved, members, S_, repeats):
    out = []
    _, track_ms, t = timed(lambda: b.track(S_), b.track_ms, repeats)
    for M in members:
        dx0 = obca_amd.ensemble_offsets(B, M, SIGMA[nx], seed=0)
        wall_ms, kernel_ms, r = timed(lambda: b.ensemble(M, S_, dx0), b.ensemble_ms, repeats)
        t0 = time.perf_counter(); mem = b.ensemble_members(); mem_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter(); b.ensemble_final(); fin_ms = (time.perf_counter() - t0) * 1e3
        ok = r["finite"] & (r["members_bad"] == 0); good = mem[..., 0] == 0
        nominal = mem[:, 0, 7][good[:, 0]]; spread = (mem[:, :, 7] - mem[:, :1, 7])[good & good[:, :1]]      # a member's smallest clearance minus the nominal closed loop's
        e = dict(config=cfg, B=B, N=N, substeps=S_, members=M, ensemble_kernel_ms=kernel_ms, ensemble_wall_ms=wall_ms, track_kernel_ms=track_ms, members_times_track_kernel_ms=M * track_ms,
                 ensemble_over_members_times_track=kernel_ms / (M * track_ms), ensemble_over_one_track=kernel_ms / track_ms, ipm_ms=ipm_ms, ensemble_over_ipm=kernel_ms / ipm_ms,
                 members_download_wall_ms=mem_ms, final_download_wall_ms=fin_ms, solved=solved, instances_finite=int(r["finite"].sum()), members_bad=int(np.maximum(r["members_bad"], 0).sum()),
                 sigma=SIGMA[nx].tolist(), need=need,
                 member_min_percentiles=dict(zip(map(str, PCT), np.percentile(mem[:, :, 7][good], PCT).tolist())) if good.any() else None,
                 member_min_minus_nominal_percentiles=dict(zip(map(str, PCT), np.percentile(spread, PCT).tolist())) if spread.size else None,
                 nominal_min_percentiles=dict(zip(map(str, PCT), np.percentile(nominal, PCT).tolist())) if nominal.size else None,
                 members_hit_histogram=np.bincount(r["members_hit"][ok], minlength=M + 1).tolist(), instances_with_a_hit=int((r["members_hit"][ok] > 0).sum()),
                 nominal_hits=int((mem[:, 0, 10][good[:, 0]] > 0).sum()),
                 end_pos_median_max=(float(np.median(r["end_pos"][ok])), float(r["end_pos"][ok].max())) if ok.any() else None,
                 dev_pos_median_max=(float(np.median(r["dev_pos"][ok])), float(r["dev_pos"][ok].max())) if ok.any() else None,
                 members_sat_instances=int((r["members_sat"][ok] > 0).sum()), track_finite=int(t["finite"].sum()))
        out.append(e); print(json.dumps(e), flush=True)
    return out


def parking_entries(ctx, B, members, S_, repeats):
    N = 80; base = S.make_batch(S.BACKWARDS, min(B, 1024), N); sel = np.arange(B) % len(base["Ts"])
    bt = dict(base, x0=base["x0"][sel], xF=base["xF"][sel], Ts=base["Ts"][sel], xWS=base["xWS"][sel], uWS=base["uWS"][sel])
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = obca_amd.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    b.solve(); ipm_ms, _ = b.kernel_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    out = entries(b, 2, B, N, 4, 0.05, ipm_ms, solved, members, S_, repeats)
    b.close()
    return out


def quad_entries(ctx, B, members, S_, repeats):
    N = 60; bt = S.make_quad_batch(B, N)
    b = obca_amd.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    b.solve(); ipm_ms = b.kernel_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    out = entries(b, "quad60", B, N, 12, 0.0, ipm_ms, solved, members, S_, repeats)
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 16384])
    ap.add_argument("--quad-batches", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--substeps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--diffs", default=None)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--only", default=None, help="KIND:B -- measure this one batch and print its entries as one JSON line (the child of a run)")
    a = ap.parse_args()
    if a.only:
        kind, B = a.only.split(":"); ctx = obca_amd.Context(0)
        e = (parking_entries if kind == "parking" else quad_entries)(ctx, int(B), a.members, a.substeps, a.repeats)
        print("ENTRIES " + json.dumps(dict(device=ctx.name(), entries=e)), flush=True)
        ctx.close()
        return
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec.update(what="tools/ensemble_rate.py: M disturbed closed loops per instance in one launch, against M times the track kernel of the same batch, beside the solve")
    if a.diffs and os.path.exists(a.diffs):
        rec["device_differences"] = dict(json.load(open(a.diffs)), what="largest relative differences over tests/test_gpu_ensemble.py: device - host build, ensemble - device track call")
    rec["entries"] = []
    for kind, B in [("parking", B) for B in a.batches] + [("quad", B) for B in a.quad_batches]:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "%s:%d" % (kind, B), "--members", *map(str, a.members), "--substeps", str(a.substeps), "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)      # (a step that hangs raises TimeoutExpired: nothing more is started)
        sys.stdout.write(p.stdout); sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            raise SystemExit("%s:%d ended with status %d: stopping" % (kind, B, p.returncode))
        got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ENTRIES ")][-1][8:])
        rec["device"] = got["device"]; rec["entries"] += got["entries"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
