"""Cost of the clearance certificate (Batch.certify / QuadBatch.certify, include/obca_certify.h: one wavefront per instance, conservative advancement per (interval, obstacle))
beside the sampling it replaces and the solve it follows.

    python tools/certify_rate.py [--out profiles/certify_device_vs_host.json] [--batches 1024 16384] [--quad-batch 256] [--slacks 0.01 0.002] [--repeats 5] [--diffs FILE]

The batches of tools/clearance_rate.py: config 2 (backwards parking, N = 80; 1 024 planned instances, repeated for the larger batch) and config 4 (quadcopter, N = 60).  Per
batch, in ONE run: the certify kernel's time from HIP events at every slack (median of `repeats` after a warm-up), the clearance() kernel at 8 and 32 sub-steps the same way,
ipm_ms of the batch's solve; samples per item (mean / max), the share of instances certified, violated and undecided, and how many instances clearance(8) calls clean at
`need` that certify does not.  The comparison that matters is certify against clearance(32).  --diffs: the file tests/test_gpu_certify.py leaves its largest
device-to-host-build difference in (OBCA_CERTIFY_DIFFS); it is copied into the profile as "device_vs_host_build"."""
import argparse
import json
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import obca_amd                                                     # noqa: E402
from obca_amd import scenarios as S, validate as V                  # noqa: E402


def median_ms(call, ms, repeats):
    """the median of the kernel time over `repeats` calls after one warm-up, and the last result"""
    r = call(); t = []
    for _ in range(repeats):
        r = call(); t.append(ms())
    return float(np.median(t)), r


def entries(b, config, B, N, nOb, need, slacks, repeats, ipm_ms, solved):
    c8_ms, c8 = median_ms(lambda: b.clearance(8, need), b.clearance_ms, repeats)
    c32_ms, c32 = median_ms(lambda: b.clearance(32, need), b.clearance_ms, repeats)
    out = []
    for slack in slacks:
        ms, r = median_ms(lambda: b.certify(need, slack), b.certify_ms, repeats)
        f = r["finite"]; items = (N + 1) * nOb
        out.append(dict(config=config, B=B, N=N, need=need, slack=slack, certify_kernel_ms=ms, clearance8_kernel_ms=c8_ms, clearance32_kernel_ms=c32_ms, ipm_ms=ipm_ms, solved=solved,
                        certify_over_clearance32=ms / c32_ms, certify_over_ipm=ms / ipm_ms, finite=int(f.sum()),
                        samples_per_item_mean=float(r["samples"][f].mean() / items) if f.any() else None, samples_per_item_max=int(r["samples_max"][f].max()) if f.any() else None,
                        samples_per_instance_mean=float(r["samples"][f].mean()) if f.any() else None, samples_per_instance_clearance32=32 * N + 1,
                        certified_share=float(r["certified"].mean()), violated_instances=int((r["violated"][f] > 0).sum()), undecided_instances=int((r["undecided"][f] > 0).sum()),
                        clean_for_clearance8_not_certified=int((f & c8["finite"] & (c8["below"] == 0) & ~r["certified"]).sum()),
                        clean_for_clearance32_not_certified=int((f & c32["finite"] & (c32["below"] == 0) & ~r["certified"]).sum()),
                        lb_smallest=float(r["lb"][f].min()) if f.any() else None, seen_smallest=float(r["seen"][f].min()) if f.any() else None,
                        clearance32_min_smallest=float(c32["min"][f].min()) if f.any() else None, lipschitz_largest=float(r["lipschitz"][f].max()) if f.any() else None))
    return out


def parking_entries(ctx, B, slacks, repeats):
    N = 80; base = S.make_batch(S.BACKWARDS, min(B, 1024), N); sel = np.arange(B) % len(base["Ts"])
    bt = dict(base, x0=base["x0"][sel], xF=base["xF"][sel], Ts=base["Ts"][sel], xWS=base["xWS"][sel], uWS=base["uWS"][sel])
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    b = obca_amd.Batch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
    b.solve(); ipm_ms, _ = b.kernel_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    out = entries(b, 2, B, N, int(b.nObs.max()), V.DMIN, slacks, repeats, ipm_ms, solved)
    b.close()
    return out


def quad_entries(ctx, B, slacks, repeats):
    N = 60; bt = S.make_quad_batch(B, N)
    b = obca_amd.QuadBatch(ctx, B, N)
    b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
    b.solve(); ipm_ms = b.kernel_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    out = entries(b, 4, B, N, 5, 0.0, slacks, repeats, ipm_ms, solved)
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certify_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--quad-batch", type=int, default=256)
    ap.add_argument("--slacks", type=float, nargs="+", default=[0.01, 0.002])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--diffs", default=None)
    a = ap.parse_args()
    ctx = obca_amd.Context(0)
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec.update(device=ctx.name(), what="tools/certify_rate.py: the clearance certificate on the device beside clearance() at 8 and 32 sub-steps and the solve of the same batch; "
                                       "kernel times are medians of %d HIP-event readings after a warm-up" % a.repeats, entries=[])
    if a.diffs and os.path.exists(a.diffs):
        rec["device_vs_host_build"] = dict(json.load(open(a.diffs)), what="largest |device - host build| of lb, seen and the interval bounds over tests/test_gpu_certify.py (parking; the quadcopter is bit-equal)")
    for B in a.batches:
        for e in parking_entries(ctx, B, a.slacks, a.repeats):
            rec["entries"].append(e); print(json.dumps(e), flush=True)
    for e in quad_entries(ctx, a.quad_batch, a.slacks, a.repeats):
        rec["entries"].append(e); print(json.dumps(e), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
