"""Cost of the clearance of a held plan against obstacles that move (Batch.predict_clearance / QuadBatch.predict_clearance, include/obca_predict.h: one wavefront per
instance, one launch) beside clearance() of the same batch at the same sub-steps, beside the solve, and beside the only other route -- download() and the numpy statement.

    python tools/predict_rate.py [--out profiles/predict_device_vs_host.json] [--batches 1024 16384] [--quad-batches 256 1024] [--substeps 1 8 32] [--repeats 5]
                                 [--host-sample 32] [--step-timeout 900]

Config 2 (backwards parking, N = 80; 1 024 planned instances, repeated for the larger batch) and make_quad_batch(B, 60).  Every batch is measured by a child process of its
own under `--step-timeout` seconds (`--only KIND:B` is that child); the first one that fails or runs out of time ends the run.  Per sub-step count the routes alternate --
clearance(), predict without rotation, predict with rotation, predict without rotation keeping the profile --, one warm-up each, medians of `repeats`.  The parking rates
move the left kerb onto the paths at 0.215 m per horizon and let every margin grow by 1 mm/s; the rotation turns every obstacle at 2 mrad/s about its pivot.  The host
route is download() plus validate.predict_parking / predict_quad + predict_record on `host-sample` instances on one core (parking: the exact polygon distance of
tests/polygon_distance.py as the per-pose distance), scaled to the batch.  `clearance_kernel_ms_parent` is the figure of profiles/clearance_device_vs_host.json for the
same batch and sub-steps, where that file has one."""
import argparse
import json
import os
import subprocess
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import obca_amd                                                     # noqa: E402
from obca_amd import scenarios as S, validate as V                  # noqa: E402


def _parent(cfg, B, S_):
    try:
        for e in json.load(open(os.path.join(ROOT, "profiles", "clearance_device_vs_host.json")))["entries"]:
            if e.get("config") == cfg and e.get("B") == B and e.get("substeps") == S_:
                return e.get("kernel_ms")
    except (OSError, ValueError, KeyError):
        pass
    return None


class Parking:
    kind, cfg, N, need = "parking", 2, 80, 0.05

    def __init__(self, ctx, B):
        base = S.make_batch(S.BACKWARDS, min(B, 1024), self.N); sel = np.arange(B) % len(base["Ts"]); self.bt = base; self.B = B
        xWS = base["xWS"][sel].copy(); xWS[:, 0, :] = base["x0"][sel]
        self.b = obca_amd.Batch(ctx, B, self.N)
        self.b.upload(base["x0"][sel], base["xF"][sel], base["Ts"][sel], base["L"], base["ego"], base["XYbounds"], base["vOb"], base["A"], base["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS,
                      base["uWS"][sel])
        self.Ts = base["Ts"][sel]; self.nOb = len(base["vOb"])

    def ipm_ms(self):
        return self.b.kernel_ms()[0]

    def rates(self, horizon, rotate):
        r = np.zeros((self.B, self.nOb, 3)); r[:, 0, 0] = 0.215 / horizon
        if rotate:
            r[:, :, 2] = 0.002
        return dict(rates=r.reshape(-1, 3), pivot=np.tile([[-1.3, 5.0], [1.3, 5.0], [0.0, 11.0]], (self.B, 1)), grow=0.001)

    def host(self, o, kw, S_, n):
        import polygon_distance as PD
        bt = self.bt; A, b = np.asarray(bt["A"], float), np.asarray(bt["b"], float); nr = np.hypot(A[:, 0], A[:, 1]); A = A / nr[:, None]; b = b / nr
        rt = np.c_[kw["rates"], kw["pivot"], np.full(len(kw["rates"]), kw["grow"])].reshape(self.B, self.nOb, 6)
        dist = lambda pose, Aj, bj: PD.polygon_distance(pose[0], pose[1], pose[2], bt["ego"], Aj, bj)
        t0 = time.perf_counter()
        for i in range(n):
            c, tau, ok = V.predict_parking(o["xp"][i], o["up"][i], o["timeScale"][i], float(self.Ts[i]), bt["L"], bt["vOb"], A, b, rt[i], dist, S_)
            V.predict_record(c, tau, rt[i], S_, self.need, ok)
        return (time.perf_counter() - t0) * 1e3


class Quad:
    kind, cfg, N, need = "quad", "quad60", 60, 0.0

    def __init__(self, ctx, B):
        self.bt = bt = S.make_quad_batch(B, self.N); self.B = B; self.b = obca_amd.QuadBatch(ctx, B, self.N)
        self.b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])

    def ipm_ms(self):
        return self.b.kernel_ms()

    def rates(self, horizon, rotate):
        r = np.zeros((self.B, 5, 3)); r[:, 0, 0] = 0.2 / horizon
        return dict(rates=r, grow=0.001)

    def host(self, o, kw, S_, n):
        bt = self.bt; ob = np.broadcast_to(np.asarray(bt["ob"], float).reshape(-1, 5, 6), (self.B, 5, 6)); Ts = float(np.ravel(bt["Ts"])[0])
        rt = np.concatenate([kw["rates"], np.full((self.B, 5, 1), kw["grow"])], axis=2)
        t0 = time.perf_counter()
        for i in range(n):
            c, tau, ok = V.predict_quad(o["xp"][i], o["timeScale"][i], Ts, ob[i], bt["R"], rt[i], S_)
            V.predict_record(c, tau, rt[i], S_, self.need, ok)
        return (time.perf_counter() - t0) * 1e3


def measure(v, substeps, repeats, host_sample):
    b = v.b; b.solve() if v.kind == "parking" else b.solve(obca_amd.quadcopter_default_opts())
    t0 = time.perf_counter(); o = b.download(); dl = (time.perf_counter() - t0) * 1e3
    ipm = v.ipm_ms(); solved = int((o["exitflag"] == 1).sum()); out = []
    horizon = b.predict_clearance(substeps=1, need=v.need)["horizon"]
    routes = [("clearance", None), ("predict", dict(rotate=False, profile=False))] + ([("predict_rot", dict(rotate=True, profile=False))] if v.kind == "parking" else []) + \
             [("predict_profile", dict(rotate=False, profile=True))]
    for S_ in substeps:
        k = {n: [] for n, _ in routes}; w = {n: [] for n, _ in routes}; last = None
        for rep in range(repeats + 1):      # (rep 0: the warm-up of every route)
            for name, opt in routes:
                t0 = time.perf_counter()
                if opt is None:
                    b.clearance(S_, need=v.need); ms = b.clearance_ms()
                else:
                    last = b.predict_clearance(substeps=S_, need=v.need, profile=opt["profile"], **v.rates(horizon, opt["rotate"])); ms = b.predict_clearance_ms()
                wall = (time.perf_counter() - t0) * 1e3
                if rep:
                    k[name].append(ms); w[name].append(wall)
        n = min(host_sample, v.B); kw = v.rates(horizon, False)
        host = v.host(o, kw, S_, n) * v.B / n
        e = dict(config=v.cfg, B=v.B, N=v.N, substeps=S_, ipm_ms=ipm, solved=solved, repeats=repeats, clearance_kernel_ms_parent=_parent(v.cfg, v.B, S_),
                 host_download_wall_ms=dl, host_numpy_wall_ms=host, host_sampled_on=n, profile_bytes=8 * v.B * (v.N * S_ + 1),
                 instances_with_finite_t_first=int(np.isfinite(last["t_first"]).sum()))
        for name, _ in routes:
            e[name + "_kernel_ms"] = float(np.median(k[name])); e[name + "_wall_ms"] = float(np.median(w[name]))
        e["predict_over_clearance_kernel"] = e["predict_kernel_ms"] / e["clearance_kernel_ms"]
        print(json.dumps(e), flush=True); out.append(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 16384])
    ap.add_argument("--quad-batches", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--substeps", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=32)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--only", default=None, help="KIND:B -- measure this one batch and print its entries as one JSON line (the child of a run)")
    a = ap.parse_args()
    if a.only:
        kind, B = a.only.split(":"); ctx = obca_amd.Context(0)
        v = (Parking if kind == "parking" else Quad)(ctx, int(B))
        print("ENTRIES " + json.dumps(dict(device=ctx.name(), entries=measure(v, a.substeps, a.repeats, a.host_sample))), flush=True)
        v.b.close(); ctx.close()
        return
    rec = dict(what="tools/predict_rate.py: predict_clearance() on the device beside clearance() of the same batch in the same process, the solve, and download() + the numpy "
                    "statement on one core (sampled, scaled to the batch)", entries=[])
    for kind, B in [("parking", B) for B in a.batches] + [("quad", B) for B in a.quad_batches]:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "%s:%d" % (kind, B), "--repeats", str(a.repeats), "--host-sample", str(a.host_sample), "--substeps"] + [str(s) for s in a.substeps]
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
