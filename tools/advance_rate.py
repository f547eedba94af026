"""Cost of one closed-loop step on the device (Batch.advance / QuadBatch.advance, include/obca_advance.h: the plant over the first `shift` intervals of the solution and the
restart from where it got, one launch) against the route the parent commit offers for the same step -- rollout() over the whole horizon, rollout_states(), the slice
[:, shift], shift_warm_start(x0_new) --, beside the solve it follows; and what a closed loop of such steps shows.

    python tools/advance_rate.py [--out profiles/advance_device_vs_host.json] [--batches 1024 16384] [--quad-batches 256 1024] [--shifts 1 4] [--substeps 8] [--repeats 5]
                                 [--loop-steps 20] [--step-timeout 600]

Config 2 (backwards parking, N = 80; 1 024 planned instances, repeated for the larger batch) and make_quad_batch(B, 60).  Every batch is measured by a child process of its
own under `--step-timeout` seconds (`--only KIND:B` is that child); the first one that fails or runs out of time ends the run.  Both routes need a solved batch and leave
it unsolved, so every timed call follows a fresh upload and cold solve of the same batch (not timed): the routes alternate, one warm-up each, medians of `repeats`.  Bytes
are computed from the array sizes of the calls, not measured.  The loop: `loop-steps` steps of shift 2 with a seeded kick of 0.02 on the positions, the first solve cold,
the later ones with the restart options (warm_restart_opts(); quad_warm_restart_opts(reference=True)), on the smallest batch of each kind."""
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


class Parking:
    kind, cfg, N, nx, npos, need = "parking", 2, 80, 4, 2, 0.05

    def __init__(self, ctx, B):
        base = S.make_batch(S.BACKWARDS, min(B, 1024), self.N); sel = np.arange(B) % len(base["Ts"])
        self.bt = dict(base, x0=base["x0"][sel], xF=base["xF"][sel], Ts=base["Ts"][sel], xWS=base["xWS"][sel], uWS=base["uWS"][sel])
        self.B = B; self.b = obca_amd.Batch(ctx, B, self.N)

    def upload(self):
        bt = self.bt; xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
        self.b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])

    def ipm_ms(self):
        return self.b.kernel_ms()[0]

    restart_opts = staticmethod(obca_amd.warm_restart_opts)


class Quad:
    kind, cfg, N, nx, npos, need = "quad", "quad60", 60, 12, 3, 0.0

    def __init__(self, ctx, B):
        self.bt = S.make_quad_batch(B, self.N); self.B = B; self.b = obca_amd.QuadBatch(ctx, B, self.N)

    def upload(self):
        bt = self.bt
        self.b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])

    def ipm_ms(self):
        return self.b.kernel_ms()

    restart_opts = staticmethod(lambda: obca_amd.quad_warm_restart_opts(reference=True))


def fresh(v):
    v.upload(); v.b.solve()


def step_cost(v, shift, S_, repeats):
    b = v.b; adv_wall, adv_kern, host_wall, host_parts = [], [], [], []
    for rep in range(repeats + 1):      # (rep 0: the warm-up of both routes)
        fresh(v)
        t0 = time.perf_counter(); b.advance(shift, S_, need=v.need); w = (time.perf_counter() - t0) * 1e3
        k = b.advance_ms()
        fresh(v)
        t0 = time.perf_counter(); b.rollout(S_, False, v.need); t1 = time.perf_counter(); X = b.rollout_states(); t2 = time.perf_counter()
        x0 = np.ascontiguousarray(X[:, shift]); t3 = time.perf_counter(); b.shift_warm_start(shift, x0_new=x0); t4 = time.perf_counter()
        if rep:
            adv_wall.append(w); adv_kern.append(k); host_wall.append((t4 - t0) * 1e3)
            host_parts.append([(t1 - t0) * 1e3, b.rollout_ms(), (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3])
    fresh(v); ipm = v.ipm_ms(); solved = int((b.download()["exitflag"] == 1).sum())
    hp = np.median(np.array(host_parts), axis=0).tolist(); aw, ak, hw = (float(np.median(a)) for a in (adv_wall, adv_kern, host_wall))
    B, N, nx = v.B, v.N, v.nx
    e = dict(config=v.cfg, B=B, N=N, shift=shift, substeps=S_, advance_kernel_ms=ak, advance_wall_ms=aw, host_route_wall_ms=hw, rollout_wall_ms=hp[0], rollout_kernel_ms=hp[1],
             rollout_states_wall_ms=hp[2], slice_wall_ms=hp[3], shift_warm_start_wall_ms=hp[4], advance_wall_over_host_route=aw / hw, advance_kernel_over_rollout_kernel=ak / hp[1],
             ipm_ms=ipm, advance_wall_over_ipm=aw / ipm, solved=solved,
             bytes_advance=dict(d2h=8 * 40 * B, h2d=0, what="the 40-double records; no kick in this measurement (a kick adds 8 nx B up)"),
             bytes_host_route=dict(d2h=8 * 40 * B + 8 * (N + 1) * nx * B, h2d=8 * nx * B, what="the rollout's records and all (N + 1) nx node states down, x0_new up"),
             bytes_computed_from="array sizes of the calls, not measured")
    print(json.dumps(e), flush=True)
    return e


def closed_loop(v, steps, S_, shift=2, sigma=0.02, seed=0):
    b = v.b; rng = np.random.default_rng(seed); rows = []
    v.upload(); b.advance_log(steps * shift)
    for k in range(steps):
        b.solve(v.restart_opts() if k else None); o = b.download(); ipm = v.ipm_ms()
        kick = np.zeros((v.B, v.nx)); kick[:, :v.npos] = sigma * rng.standard_normal((v.B, v.npos))
        r = b.advance(shift, S_, kick=kick, need=v.need); ok = r["finite"]
        it = o["iters"].astype(float)
        rows.append(dict(step=k, solved=int((o["exitflag"] == 1).sum()), exitflag_2=int((o["exitflag"] == 2).sum()), iters_mean=float(it.mean()), iters_max=int(it.max()), ipm_ms=ipm,
                         advance_kernel_ms=b.advance_ms(), advanced=int(ok.sum()), dev_pos_median=float(np.median(r["dev_pos"][ok])) if ok.any() else None,
                         dev_pos_max=float(r["dev_pos"][ok].max()) if ok.any() else None, min_clearance=float(r["clearance"]["min"][ok].min()) if ok.any() else None,
                         below_need=int((r["clearance"]["below"][ok] > 0).sum()), goal_dist_median=float(np.median(r["goal_dist"][ok])) if ok.any() else None))
        print(json.dumps(rows[-1]), flush=True)
    log = b.advance_log_states()
    return dict(config=v.cfg, B=v.B, N=v.N, shift=shift, substeps=S_, kick_sigma=sigma, seed=seed, steps=rows, logged_nodes=int(log.shape[1]),
                restart_opts="warm_restart_opts()" if v.kind == "parking" else "quad_warm_restart_opts(reference=True)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "advance_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 16384])
    ap.add_argument("--quad-batches", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--shifts", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--substeps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-steps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--only", default=None, help="KIND:B[:loop] -- measure this one batch and print its entries as one JSON line (the child of a run)")
    a = ap.parse_args()
    if a.only:
        kind, B, *loop = a.only.split(":"); ctx = obca_amd.Context(0)
        v = (Parking if kind == "parking" else Quad)(ctx, int(B))
        got = dict(device=ctx.name(), entries=[step_cost(v, s, a.substeps, a.repeats) for s in a.shifts], loop=closed_loop(v, a.loop_steps, a.substeps) if loop else None)
        print("ENTRIES " + json.dumps(got), flush=True)
        v.b.close(); ctx.close()
        return
    rec = dict(what="tools/advance_rate.py: one closed-loop step on the device (advance) against rollout() + rollout_states() + slice + shift_warm_start(x0_new) of the same "
                    "batch in the same process, beside the solve; closed loops of advance() steps", entries=[], loops=[])
    todo = [("parking", B, B == min(a.batches)) for B in a.batches] + [("quad", B, B == min(a.quad_batches)) for B in a.quad_batches]
    for kind, B, loop in todo:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "%s:%d%s" % (kind, B, ":loop" if loop else ""), "--shifts", *map(str, a.shifts), "--substeps", str(a.substeps),
               "--repeats", str(a.repeats), "--loop-steps", str(a.loop_steps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)      # (a step that hangs raises TimeoutExpired: nothing more is started)
        sys.stdout.write(p.stdout); sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            raise SystemExit("%s:%d ended with status %d: stopping" % (kind, B, p.returncode))
        got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ENTRIES ")][-1][8:])
        rec["device"] = got["device"]; rec["entries"] += got["entries"]
        if got["loop"]:
            rec["loops"].append(got["loop"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
