"""Cost of moving the obstacles of a resident batch on the device (Batch.move_obstacles / QuadBatch.move_obstacles, include/obca_scene_edit.h: the obstacle words of the
problem records edited in place, one launch) against the only other route to a changed scene -- upload() of host-moved obstacles, which also forgets the solution --, and
what a closed loop with one drifting obstacle shows with and without it.

    python tools/scene_edit_rate.py [--out profiles/scene_edit_device_vs_host.json] [--batches 1024 16384] [--quad-batches 256 1024] [--repeats 5] [--loop-steps 20]
                                    [--step-timeout 600]

Config 2 (backwards parking, N = 80; 1 024 planned instances, repeated for the larger batch) and make_quad_batch(B, 60).  Every batch is measured by a child process of its
own under `--step-timeout` seconds (`--only KIND:B` is that child); the first one that fails or runs out of time ends the run.  The two routes alternate, one warm-up each,
medians of `repeats`; the host-moved rows of the upload route are made outside the timed region (only upload() is timed).  Bytes are computed from the array sizes of the
calls, not measured.  The loop, on the smallest batch of each kind: `loop-steps` steps of advance(2) + move_obstacles (one obstacle drifting 1 cm per step: the far side of
the aisle towards the road / the first wall along x) + a solve with the restart options, beside a second batch of the same instances that is given what a user without the
call has: a download, the plant state and the primal start shifted on the host, a re-upload with the host-moved obstacles and a cold solve (default options; DualMultWS)."""
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


class Parking:
    kind, cfg, N, nx, need = "parking", 2, 80, 4, 0.05

    def __init__(self, ctx, B):
        base = S.make_batch(S.BACKWARDS, min(B, 1024), self.N); sel = np.arange(B) % len(base["Ts"])
        self.bt = dict(base, x0=base["x0"][sel], xF=base["xF"][sel], Ts=base["Ts"][sel], xWS=base["xWS"][sel], uWS=base["uWS"][sel])
        self.B = B; self.ctx = ctx; self.b = obca_amd.Batch(ctx, B, self.N)
        self.A = np.asarray(base["A"], float); self.bb = np.asarray(base["b"], float); self.nOb = len(base["vOb"])

    def upload(self, b=None, rows=None, x0=None, xWS=None, uWS=None):
        bt = self.bt; A, bb = rows or (self.A, self.bb); x0 = bt["x0"] if x0 is None else x0
        xWS = (bt["xWS"] if xWS is None else xWS).copy(); xWS[:, 0, :] = x0
        (b or self.b).upload(x0, bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], A, bb, xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"] if uWS is None else uWS)

    def motion(self, sign):
        m = np.zeros((self.nOb, 3)); m[2] = [0.0, -0.01 * sign, 0.0]      # the far side of the aisle, 1 cm towards the road
        return m

    def move(self, sign):
        return self.b.move_obstacles(np.tile(self.motion(sign), (self.B, 1)))

    def host_rows(self, rows, sign):
        A, bb, _ = V.move_obstacles_parking(rows[0], rows[1], self.bt["vOb"], self.motion(sign))
        return A, bb

    def ipm_ms(self, b=None):
        return (b or self.b).kernel_ms()[0]

    def bytes(self):
        N1 = self.N + 1; nt = self.nOb * self.B
        return dict(move=dict(h2d=8 * 6 * self.nOb * self.B, d2h=8 * self.B, caller_arrays=8 * 3 * nt, what="6 doubles per obstacle staged up (the caller passes 3: no pivot, no inflation), one status word per instance down"),
                    upload=dict(h2d=8 * self.B * ((252 + 3 * N1) + (4 * N1 + 2 * self.N + 1)), d2h=0, what="the problem records (252-double header + reference) and the primal start x, u, t"))

    restart_opts = staticmethod(obca_amd.warm_restart_opts)


class Quad:
    kind, cfg, N, nx, need = "quad", "quad60", 60, 12, 0.0

    def __init__(self, ctx, B):
        self.bt = S.make_quad_batch(B, self.N); self.B = B; self.ctx = ctx; self.b = obca_amd.QuadBatch(ctx, B, self.N)
        self.ob = np.broadcast_to(np.asarray(self.bt["ob"], float).reshape(-1, 5, 6), (B, 5, 6)).copy()

    def upload(self, b=None, rows=None, x0=None, xWS=None, uWS=None):
        bt = self.bt
        (b or self.b).upload(bt["x0"] if x0 is None else x0, bt["xF"], bt["Ts"], bt["R"], self.ob if rows is None else rows, bt["xWS"] if xWS is None else xWS, bt["timeWS"])

    def motion(self, sign):
        m = np.zeros((5, 3)); m[0] = [0.01 * sign, 0.0, 0.0]      # the first wall, 1 cm along x
        return m

    def move(self, sign):
        return self.b.move_obstacles(self.motion(sign))

    def host_rows(self, rows, sign):
        return np.stack([V.move_obstacles_quad(o, self.motion(sign))[0] for o in rows])

    def ipm_ms(self, b=None):
        return (b or self.b).kernel_ms()

    def bytes(self):
        return dict(move=dict(h2d=8 * 4 * 5 * self.B, d2h=8 * self.B, caller_arrays=8 * 3 * 5 * self.B, what="4 doubles per box staged up, one status word per instance down"),
                    upload=dict(h2d=8 * self.B * (64 + 12 * (self.N + 1)), d2h=0, what="the problem records: 64-double header and the warm start"))

    restart_opts = staticmethod(lambda: obca_amd.quad_warm_restart_opts(reference=True))


def move_cost(v, repeats):
    """move_obstacles() against upload() of host-moved obstacles, alternating; the scene swings 1 cm back and forth"""
    v.upload(); rows = (v.A, v.bb) if v.kind == "parking" else v.ob
    mw, mk, uw = [], [], []
    for rep in range(repeats + 1):      # (rep 0: the warm-up of both routes)
        sign = 1 if rep % 2 == 0 else -1
        t0 = time.perf_counter(); st = v.move(sign); w = (time.perf_counter() - t0) * 1e3; k = v.b.move_obstacles_ms()
        assert not st.any()
        rows = v.host_rows(rows, sign)
        t0 = time.perf_counter(); v.upload(rows=rows); v.b.sync(); u = (time.perf_counter() - t0) * 1e3
        if rep:
            mw.append(w); mk.append(k); uw.append(u)
    v.upload(); v.b.solve(); ipm = v.ipm_ms(); solved = int((v.b.download()["exitflag"] == 1).sum())
    a, k, u = (float(np.median(x)) for x in (mw, mk, uw))
    e = dict(config=v.cfg, B=v.B, N=v.N, move_kernel_ms=k, move_wall_ms=a, upload_wall_ms=u, move_wall_over_upload=a / u, ipm_ms=ipm, solved=solved, bytes=v.bytes(),
             bytes_computed_from="array sizes of the calls, not measured", repeats=repeats)
    print(json.dumps(e), flush=True)
    return e


def _shift_host(o, shift, N):
    """the primal start a user can make on the host from a download: states and inputs advanced by `shift`, the tail repeated"""
    ks = np.minimum(np.arange(N + 1) + shift, N); ku = np.minimum(np.arange(N) + shift, N - 1)
    return np.ascontiguousarray(np.transpose(o["xp"][:, :, ks], (0, 2, 1))), np.ascontiguousarray(np.transpose(o["up"][:, :, ku], (0, 2, 1)))


def closed_loop(v, steps, shift=2, S_=8):
    b = v.b; other = type(b)(v.ctx, v.B, v.N); rows = (v.A, v.bb) if v.kind == "parking" else v.ob; out = []
    v.upload(); b.solve(); o = b.download()
    cold0 = dict(solved=int((o["exitflag"] == 1).sum()), iters_mean=float(o["iters"].mean()), iters_max=int(o["iters"].max()), ipm_ms=v.ipm_ms())
    for k in range(steps):
        r = b.advance(shift, S_, need=v.need); st = b.advance_state(); ok = r["finite"]
        t0 = time.perf_counter(); ms = v.move(1); mv_wall = (time.perf_counter() - t0) * 1e3
        rows = v.host_rows(rows, 1)
        # the route without the call: the same plant state and the same primal start, a re-upload in the moved scene, a cold solve
        xs, us = _shift_host(o, shift, v.N); x0 = np.where(ok[:, None], st, o["xp"][:, :, min(shift, v.N)])
        t0 = time.perf_counter()
        if v.kind == "parking":
            v.upload(other, rows=rows, x0=x0, xWS=xs, uWS=us)
        else:
            v.upload(other, rows=rows, x0=x0, xWS=xs)
        other.sync(); up_wall = (time.perf_counter() - t0) * 1e3
        other.solve(); oc = other.download(); ipm_c = v.ipm_ms(other)
        b.solve(v.restart_opts()); o = b.download(); ipm_w = v.ipm_ms()
        c = b.clearance(S_, need=v.need)
        out.append(dict(step=k, advanced=int(ok.sum()), moved=int((ms == 0).sum()), move_kernel_ms=b.move_obstacles_ms(), move_wall_ms=mv_wall, reupload_wall_ms=up_wall,
                        warm=dict(solved=int((o["exitflag"] == 1).sum()), iters_mean=float(o["iters"].mean()), iters_max=int(o["iters"].max()), ipm_ms=ipm_w),
                        cold=dict(solved=int((oc["exitflag"] == 1).sum()), iters_mean=float(oc["iters"].mean()), iters_max=int(oc["iters"].max()), ipm_ms=ipm_c),
                        min_clearance_warm=float(np.nanmin(c["min"])), below_need_warm=int((c["below"] > 0).sum())))
        print(json.dumps(out[-1]), flush=True)
    other.close()
    return dict(config=v.cfg, B=v.B, N=v.N, shift=shift, substeps=S_, drift="1 cm per step: " + ("obstacle 2 (the far side of the aisle) towards the road" if v.kind == "parking" else "box 0 along +x"),
                first_solve=cold0, steps=out, restart_opts="warm_restart_opts()" if v.kind == "parking" else "quad_warm_restart_opts(reference=True)",
                cold_route="download + host shift of the primal start + upload(host-moved obstacles, x0 = the plant state) + solve with default options")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_edit_device_vs_host.json"))
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 16384])
    ap.add_argument("--quad-batches", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-steps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--only", default=None, help="KIND:B[:loop] -- measure this one batch and print its entries as one JSON line (the child of a run)")
    a = ap.parse_args()
    if a.only:
        kind, B, *loop = a.only.split(":"); ctx = obca_amd.Context(0)
        v = (Parking if kind == "parking" else Quad)(ctx, int(B))
        got = dict(device=ctx.name(), entries=[move_cost(v, a.repeats)], loop=closed_loop(v, a.loop_steps) if loop else None)
        print("ENTRIES " + json.dumps(got), flush=True)
        v.b.close(); ctx.close()
        return
    rec = dict(what="tools/scene_edit_rate.py: move_obstacles() on the device against upload() of host-moved obstacles of the same batch in the same process, beside the solve; "
                    "closed loops with one drifting obstacle, advance + move + warm re-solve against re-upload + cold solve", entries=[], loops=[])
    todo = [("parking", B, B == min(a.batches)) for B in a.batches] + [("quad", B, B == min(a.quad_batches)) for B in a.quad_batches]
    for kind, B, loop in todo:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "%s:%d%s" % (kind, B, ":loop" if loop else ""), "--repeats", str(a.repeats), "--loop-steps", str(a.loop_steps)]
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
