"""Cost of the clearance check between the nodes (Batch.clearance / QuadBatch.clearance, include/obca_clearance.h: one wavefront per instance) beside the solve it follows,
and against doing the same on the host: download() plus a DualMultWS distance per sample pose in a loop.

    python tools/clearance_rate.py [--out profiles/clearance_device_vs_host.json] [--batches 1024 16384] [--quad-batch 256] [--substeps 1 8 32] [--host-sample 64] [--repeats 5] [--diffs FILE]

Config 2 (backwards parking, N = 80; 1 024 planned instances, repeated for the larger batch) and config 4 (quadcopter, N = 60): per batch size and number of sub-steps the
kernel's time from HIP events and the wall time of clearance() (kernel + 24 doubles per instance down; minimum of `repeats`), beside dualws_ms and ipm_ms of the same batch's
solve; the smallest clearances found.  The host route of the parking check -- download(), numpy validate.parking_samples, the CPU checker's DualMultWS on the sample poses --
is timed on `host_sample` instances on one core and scaled.  --diffs: the file tests/test_gpu_clearance.py leaves its largest device-to-host-build differences in
(OBCA_CLEARANCE_DIFFS); they are copied into the profile as "device_vs_host_build"."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import obca_amd                                                     # noqa: E402
from obca_amd import scenarios as S, validate as V                  # noqa: E402


def timed(fn, repeats):
    best = None; r = None
    for _ in range(repeats):
        t0 = time.perf_counter(); r = fn(); dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, r


def host_route_ms(b, bt, B, S_, m):
    """download() + the oracle loop on the first m instances, scaled to B"""
    import oracle as O
    t0 = time.perf_counter(); o = b.download(); down_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for i in range(m):
        p = V.parking_samples(o["xp"][i], o["up"][i], o["timeScale"][i], bt["Ts"][i], bt["L"], S_)
        _, _, d = O.dualmult_ws(len(p) - 1, bt["vOb"], bt["A"], bt["b"], p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), bt["ego"])
        V.clearance_record(np.where(d < V.CLR_TOUCH, 0.0, d), S_, V.DMIN)
    return down_ms, (time.perf_counter() - t0) * 1e3 / m * B


def parking_entries(ctx, B, substeps, repeats, host_sample):
    N = 80; base = S.make_batch(S.BACKWARDS, min(B, 1024), N); sel = np.arange(B) % len(base["Ts"])
    bt = dict(base, x0=base["x0"][sel], xF=base["xF"][sel], Ts=base["Ts"][sel], xWS=base["xWS"][sel], uWS=base["uWS"][sel])
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = obca_amd.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    b.solve(); ipm_ms, dualws_ms = b.kernel_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    out = []
    for S_ in substeps:
        b.clearance(S_)
        wall_ms, r = timed(lambda: b.clearance(S_), repeats)
        down_ms, loop_ms = host_route_ms(b, bt, B, S_, min(host_sample, B))
        out.append(dict(config=2, B=B, N=N, substeps=S_, kernel_ms=b.clearance_ms(), clearance_wall_ms=wall_ms, dualws_ms=dualws_ms, ipm_ms=ipm_ms, solved=solved,
                        kernel_over_dualws=b.clearance_ms() / dualws_ms, host_download_wall_ms=down_ms, host_oracle_loop_wall_ms=loop_ms, host_loop_sampled_on=min(host_sample, B),
                        min_nodes_smallest=float(r["min_nodes"].min()), min_smallest=float(r["min"].min()), instances_below_need_between_nodes=int(((r["min"] < V.DMIN - 1e-6) & (r["min_nodes"] >= V.DMIN - 1e-6)).sum())))
    b.close()
    return out


def quad_entries(ctx, B, substeps, repeats):
    N = 60; bt = S.make_quad_batch(B, N)
    b = obca_amd.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    b.solve(); ipm_ms = b.kernel_ms(); ok = b.download()["exitflag"] == 1
    out = []
    for S_ in substeps:
        b.clearance(S_)
        wall_ms, r = timed(lambda: b.clearance(S_), repeats)
        out.append(dict(config=4, B=B, N=N, substeps=S_, kernel_ms=b.clearance_ms(), clearance_wall_ms=wall_ms, ipm_ms=ipm_ms, solved=int(ok.sum()),
                        min_nodes_smallest=float(r["min_nodes"][ok].min()) if ok.any() else None, min_smallest=float(r["min"][ok].min()) if ok.any() else None))
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--quad-batch", type=int, default=256)
    ap.add_argument("--substeps", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--diffs", default=None)
    a = ap.parse_args()
    ctx = obca_amd.Context(0)
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec.update(device=ctx.name(), what="tools/clearance_rate.py: clearance between the nodes on the device, beside the solve of the same batch and the host route", entries=[])
    if a.diffs and os.path.exists(a.diffs):
        rec["device_vs_host_build"] = dict(json.load(open(a.diffs)), what="largest |device - host build| and |resident - host-pointer call| over tests/test_gpu_clearance.py")
    for B in a.batches:
        for e in parking_entries(ctx, B, a.substeps, a.repeats, a.host_sample):
            rec["entries"].append(e); print(json.dumps(e), flush=True)
    for e in quad_entries(ctx, a.quad_batch, a.substeps, a.repeats):
        rec["entries"].append(e); print(json.dumps(e), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
