"""Cost of checking a solved batch: on the device (Batch.validate / QuadBatch.validate: one kernel, 16 / 10 doubles per instance downloaded) against the numpy
checkers of obca_amd/validate.py on the downloaded solution, for BASELINE configs 2 (parking, 1 024 instances, N = 80) and 4 (quadcopter, N = 60).

    python tools/validate_rate.py [--out profiles/validate_device_vs_host.json] [--batch2 1024] [--batch4 256] [--numpy-sample 128]

Every entry records the validate-kernel time from HIP events, the validate() wall time (result download included, minimum of `repeats`), the numpy time for the same
batch on the same host (measured on `numpy_sample` instances, scaled to the batch; one core, one instance at a time, as bench.py runs it), the interior-point kernel
time of the solve, and the bytes each route brings over PCIe."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import obca_amd as OA                                  # noqa: E402
from obca_amd import scenarios as S, validate as V     # noqa: E402


def timed(fn, repeats):
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter(); r = fn(); dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, r


def parking(ctx, B, N, repeats, sample):
    bt = S.make_batch(S.BACKWARDS, B, N)
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = OA.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    b.solve(opts=OA.ipopt_opts()); ipm_ms = b.kernel_ms()[0]
    b.validate()
    wall_ms, res = timed(b.validate, repeats); kern_ms = b.validate_ms()
    dl_ms, out = timed(b.download, repeats)
    n = min(sample, B); t0 = time.perf_counter(); ok = 0
    for i in range(n):
        ts = out["timeScale"][i]
        ok += V.validate_parking(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], out["xp"][i], out["up"][i], ts,
                                 out["lp"][i], out["np"][i], out["sl"][i])[0]
        V.parking_constraints_ref(bt["x0"][i], bt["xF"][i], N, bt["Ts"][i], bt["L"], bt["ego"], bt["XYbounds"], len(bt["vOb"]), bt["vOb"], bt["A"], bt["b"], out["xp"][i], out["up"][i],
                                  out["lp"][i], out["np"][i], ts, 0, 1)
    np_ms = (time.perf_counter() - t0) * 1e3 / n * B
    nOb, M = len(bt["vOb"]), int(np.sum(bt["vOb"])); per = 4 * (N + 1) + 2 * N + (N + 1) + (M + 4 * nOb + nOb) * (N + 1) + 8
    b.close()
    return dict(config=2, workload="reverse parking, N = %d, %d obstacles / %d rows, reference options" % (N, nOb, M), batch=B, ipm_ms=ipm_ms, validate_kernel_ms=kern_ms,
                validate_wall_ms=wall_ms, download_wall_ms=dl_ms, numpy_ms=np_ms, numpy_sample=n, numpy_checks="validate_parking + parking_constraints_ref",
                device_ok=int(res["ok"].sum()), device_ref_ok=int(res["ref_ok"].sum()), numpy_ok_in_sample=int(ok),
                bytes_downloaded_device_route=B * 16 * 8, bytes_downloaded_host_route=B * per * 8, repeats=repeats)


def quad(ctx, B, N, repeats, sample):
    q = S.make_quad_batch(B, N, random_endpoints=True)
    b = OA.QuadBatch(ctx, B, N)
    b.upload(q["x0"], q["xF"], q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"], dual_ws=True)
    b.solve(opts=OA.quadcopter_ipopt_opts()); ipm_ms = b.kernel_ms()
    b.validate()
    wall_ms, res = timed(b.validate, repeats); kern_ms = b.validate_ms()
    dl_ms, out = timed(b.download, repeats)
    n = min(sample, B); t0 = time.perf_counter(); ok = 0
    for i in range(n):
        ok += V.validate_quadcopter(out["xp"][i], out["up"][i], out["timeScale"][i], q["x0"][i], q["xF"][i], q["Ts"], out["lp"][i], q["ob"], q["R"])[0]
    np_ms = (time.perf_counter() - t0) * 1e3 / n * B
    per = 12 * (N + 1) + 4 * N + (N + 1) + 30 * (N + 1) + 5 * (N + 1) + 8
    b.close()
    return dict(config=4, workload="quadcopter, 5 boxes, N = %d, 3-D A* warm starts, reference options" % N, batch=B, ipm_ms=ipm_ms, validate_kernel_ms=kern_ms, validate_wall_ms=wall_ms,
                download_wall_ms=dl_ms, numpy_ms=np_ms, numpy_sample=n, numpy_checks="validate_quadcopter", device_ok=int(res["ok"].sum()), numpy_ok_in_sample=int(ok),
                bytes_downloaded_device_route=B * 10 * 8, bytes_downloaded_host_route=B * per * 8, repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_device_vs_host.json"))
    ap.add_argument("--batch2", type=int, default=1024); ap.add_argument("--batch4", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--numpy-sample", type=int, default=128)
    a = ap.parse_args()
    ctx = OA.Context(0)
    res = dict(device=ctx.name(), entries=[parking(ctx, a.batch2, 80, a.repeats, a.numpy_sample), quad(ctx, a.batch4, 60, a.repeats, a.numpy_sample)])
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
