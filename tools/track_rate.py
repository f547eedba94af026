"""Cost of the closed-loop rollout (Batch.track / QuadBatch.track, include/obca_track.h: one wavefront per instance, one launch: linearisation, Riccati recursion, closed
loop) beside the solve it follows, beside the chain rollout() of the same batch -- whose work it contains -- and against doing the same on the host; and what tracking shows
on those solved batches.

    python tools/track_rate.py [--out profiles/track_device_vs_host.json] [--batches 1024 16384] [--quad-batches 256 1024] [--substeps 1 8] [--host-sample 32]
                               [--repeats 5] [--diffs FILE] [--step-timeout 300]

Config 2 (backwards parking, N = 80; 1 024 planned instances, repeated for the larger batch) and make_quad_batch(B, 60).  Every batch is measured by a child process of its
own under `--step-timeout` seconds (`--only KIND:B` is that child); the first one that fails or runs out of time ends the run.  Per batch and number of sub-steps: the track
kernel's time from HIP events and the wall time of track() (medians of `repeats` after a warm-up call), with feedback and -- the same launch without the loop's feedback --
the kernel's time with feedback=False, beside the chain rollout() kernel and ipm_ms of the same batch; track_states() / track_gains() wall time; deviations median / worst
closed against open loop, how many instances the clamp touches, the smallest clearance of the driven path.  With dx0: the same from a start 0.1 m (and 0.1 m/s, quadcopter)
off.  The host route -- download() and the numpy statement (validate.track_parking / track_quad, the sample clearances left out) at 8 sub-steps -- is timed on
`host_sample` instances on one core and scaled.  --diffs: the file tests/test_gpu_track.py leaves its largest device-to-host-build differences in (OBCA_TRACK_DIFFS)."""
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
from obca_amd import scenarios as S, validate as V                  # noqa: E402
from rollout_rate import timed                                      # noqa: E402

DX0 = {4: np.array([0.1, 0.1, 0.05, 0.0]), 12: np.r_[np.full(3, 0.1), np.zeros(3), np.full(3, 0.1), np.zeros(3)]}


def stats(r, key):
    f = r["finite"]
    return (float(np.median(r[key][f])), float(r[key][f].max())) if f.any() else (None, None)


def entries(b, cfg, B, N, nx, ipm_ms, solved, substeps, repeats, host):
    out = []
    for S_ in substeps:
        roll_wall, roll_ms, op = timed(lambda: b.rollout(S_, False), b.rollout_ms, repeats)
        wall_ms, kernel_ms, r = timed(lambda: b.track(S_), b.track_ms, repeats)
        _, open_ms, _ = timed(lambda: b.track(S_, feedback=False, clamp=False), b.track_ms, repeats)
        t0 = time.perf_counter(); b.track_states(); states_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter(); b.track_gains(); gains_ms = (time.perf_counter() - t0) * 1e3
        off = b.track(S_, DX0[nx]); off_open = b.track(S_, DX0[nx], feedback=False, clamp=False)
        e = dict(config=cfg, B=B, N=N, substeps=S_, track_kernel_ms=kernel_ms, track_wall_ms=wall_ms, track_kernel_without_feedback_ms=open_ms, rollout_chain_kernel_ms=roll_ms,
                 track_over_rollout=kernel_ms / roll_ms, ipm_ms=ipm_ms, track_over_ipm=kernel_ms / ipm_ms, states_download_wall_ms=states_ms, gains_download_wall_ms=gains_ms,
                 solved=solved, finite_closed=int(r["finite"].sum()), finite_open=int(op["finite"].sum()),
                 dev_pos_median_max_closed=stats(r, "dev_pos"), dev_pos_median_max_open=stats(op, "dev_pos"), end_pos_median_max_closed=stats(r, "end_pos"),
                 end_pos_median_max_open=stats(op, "end_pos"), clamp_touches=int((r["saturated"] > 0).sum()), du_max_largest=float(np.nanmax(r["du_max"])),
                 clearance_min_smallest_closed=float(np.nanmin(r["clearance"]["min"])), clearance_min_smallest_open=float(np.nanmin(op["clearance"]["min"])),
                 below_instances_closed=int((r["clearance"]["below"][r["finite"]] > 0).sum()), below_instances_open=int((op["clearance"]["below"][op["finite"]] > 0).sum()),
                 from_dx0=dict(dx0=DX0[nx].tolist(), end_pos_median_max_closed=stats(off, "end_pos"), end_pos_median_max_open=stats(off_open, "end_pos"),
                               finite_closed=int(off["finite"].sum()), finite_open=int(off_open["finite"].sum()), clamp_touches=int((off["saturated"] > 0).sum())))
        if S_ == 8 and host is not None:
            e.update(host())
        out.append(e); print(json.dumps(e), flush=True)
    return out


def parking_entries(ctx, B, substeps, repeats, host_sample):
    N = 80; base = S.make_batch(S.BACKWARDS, min(B, 1024), N); sel = np.arange(B) % len(base["Ts"])
    bt = dict(base, x0=base["x0"][sel], xF=base["xF"][sel], Ts=base["Ts"][sel], xWS=base["xWS"][sel], uWS=base["uWS"][sel])
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = obca_amd.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    b.solve(); ipm_ms, _ = b.kernel_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    m = min(host_sample, B)

    def host():
        t0 = time.perf_counter(); o = b.download(); down_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for i in range(m):
            V.track_parking(o["xp"][i], o["up"][i], o["timeScale"][i], bt["Ts"][i], bt["L"], 8)
        return dict(host_download_wall_ms=down_ms, host_numpy_loop_wall_ms=(time.perf_counter() - t0) * 1e3 / m * B, host_loop_sampled_on=m)
    out = entries(b, 2, B, N, 4, ipm_ms, solved, substeps, repeats, host if m > 0 else None)
    b.close()
    return out


def quad_entries(ctx, B, substeps, repeats, host_sample):
    N = 60; bt = S.make_quad_batch(B, N)
    b = obca_amd.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    b.solve(); ipm_ms = b.kernel_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    m = min(host_sample, B)

    def host():
        t0 = time.perf_counter(); o = b.download(); down_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for i in range(m):
            V.track_quad(o["xp"][i], o["up"][i], o["timeScale"][i], bt["Ts"], 8)
        return dict(host_download_wall_ms=down_ms, host_numpy_loop_wall_ms=(time.perf_counter() - t0) * 1e3 / m * B, host_loop_sampled_on=m)
    out = entries(b, "quad60", B, N, 12, ipm_ms, solved, substeps, repeats, host if m > 0 else None)
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 16384])
    ap.add_argument("--quad-batches", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--substeps", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--host-sample", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--diffs", default=None)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--only", default=None, help="KIND:B -- measure this one batch and print its entries as one JSON line (the child of a run)")
    a = ap.parse_args()
    if a.only:
        kind, B = a.only.split(":"); ctx = obca_amd.Context(0)
        e = (parking_entries if kind == "parking" else quad_entries)(ctx, int(B), a.substeps, a.repeats, a.host_sample)
        print("ENTRIES " + json.dumps(dict(device=ctx.name(), entries=e)), flush=True)
        ctx.close()
        return
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec.update(what="tools/track_rate.py: TVLQR gains and closed-loop rollout on the device, beside the chain rollout and the solve of the same batch and the host route")
    if a.diffs and os.path.exists(a.diffs):
        rec["device_vs_host_build"] = dict(json.load(open(a.diffs)), what="largest relative |device - host build| over tests/test_gpu_track.py (gains: relative to the instance's largest)")
    rec["entries"] = []
    for kind, B in [("parking", B) for B in a.batches] + [("quad", B) for B in a.quad_batches]:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "%s:%d" % (kind, B), "--substeps", *map(str, a.substeps), "--host-sample", str(a.host_sample), "--repeats", str(a.repeats)]
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
