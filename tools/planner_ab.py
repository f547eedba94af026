"""A/B of the parking planners' native code between two builds of the libraries: the same calls through the same Python, the outputs compared as raw bytes.

    python tools/planner_ab.py host   PARENT NEW [--out profiles/planner_geom_fold_ab.json] [--time]
    python tools/planner_ab.py device PARENT NEW [--out ...]
    python tools/planner_ab.py asm    PARENT.s NEW.s [--out ...]
    python tools/planner_ab.py bound  NAME PARENT_FIRST_MS NEW_MS PARENT_SECOND_MS [OUT]

PARENT, NEW: directories that hold the libraries of one build each, flat or laid out as the tree (obca_amd/csrc, tests/emu).  Every build is called in a child process of
its own (each under its own time limit; the second starts only if the first ended well), which writes what the calls returned into an .npz; this process compares the two
files item by item and writes, per check, how many items there are and how many differ into the section of --out named after the mode.
  host:   libobca_plan.so -- obca_plan_hybrid_astar_batch2 on the 16 backwards and 16 parallel poses of tests/hybrid_common.py with their SCENARIO_OPTS, 4 each with the
          analytic expansion off, the Reeds-Shepp heuristic on and the lattice heuristic on; obca_plan_reeds_shepp on 10 000 seeded queries; obca_plan_collides on 100 000
          seeded poses per field; both on poses with a NaN or an infinity in them, which the host planner does not refuse.  The host builds of the device planner
          (hybrid_emu, scenes_emu, plan_resident_emu) on the 8-instance cases of their *_common.py in loop orders 0, 1, 2.  --time: the 32 searches on 16 threads, five timed runs per build after one that warms up.
  device: libobca_hip.so through OBCA_HIP_LIBRARY -- hybrid_astar_batch and scene_astar_batch on 8 backwards + 8 parallel poses, Batch.plan_warm_start + plan_paths at B = 8.
  asm:    two `hipcc -save-temps` / `-S` assemblies of obca_hip.hip, kernel by kernel: identical, identical up to block-label numbers, or different.
  bound:  where planner kernels differ, the search-kernel milliseconds (the median `kernel_ms` that tools/hybrid_rate.py, scene_rate.py or plan_resident_rate.py prints
          for B = 1 024, 256 slots) of three runs on one box, parent, new, parent, each tool run with OBCA_HIP_LIBRARY on that build: the parent's spread, the bound (the
          parent's two values widened by their difference on either side) and whether the new value lies within, into device_search_kernel_ms.runs[NAME].
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = dict(host=900, time=300, device=240)      # seconds a child may take


def find(libdir, name):
    for sub in ("", os.path.join("obca_amd", "csrc"), os.path.join("tests", "emu")):
        p = os.path.join(libdir, sub, name)
        if os.path.exists(p):
            return os.path.abspath(p)
    raise SystemExit("no %s under %s" % (name, libdir))


# ---------------------------------------------------------------- the children
def _setup(mode, libdir):
    """this tree's Python over the libraries of `libdir`: nothing is compiled here.  (device: the product library comes through OBCA_HIP_LIBRARY; the host libraries that
    draw the inputs are this tree's)"""
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    if mode == "device":
        return
    from obca_amd import buildflags as BF
    table = {**BF.EMU_PIECES, **BF.CHECK_PIECES, **BF.TEST_PIECES, **BF.PIECES}
    BF.build = lambda name, *a, **k: find(libdir, os.path.basename(table[name].out))


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def _searches(which, B, **more):
    import hybrid_common as H
    from obca_amd import planner as PL, scenarios as S
    sc, x0, xF, kw = H.poses(which, 16)
    v, A, b = H.field(sc)
    _, _, paths, dirs, cnt, nexp = PL._hybrid_astar_dense(x0[:B], xF[:B], v, A, b, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, 16, H.CAP, dict(kw, **more))
    return dict(paths=paths, dirs=dirs, counts=cnt, expansions=nexp)


NOT_FINITE = [(np.nan, 0.0, 0.0), (5.0, np.nan, 1.0), (5.0, 5.0, np.nan), (5.0, 5.0, np.inf), (5.0, 5.0, -np.inf), (np.inf, 5.0, 0.0), (5.0, -np.inf, 0.0), (np.nan, np.nan, np.nan)]


def _code(search):
    """what obca_plan_hybrid_astar2 returned, read back from planner.hybrid_astar: the node count, 0 (no path), -1 (bad arguments) or -2 (start or goal collides)"""
    try:
        r = search()
    except ValueError as e:
        return -2 if "collides" in str(e) else -1
    return 0 if r is None else len(r[0])


def child_host(out):
    import ctypes as C
    import hybrid_common as H
    import plan_resident_common as R
    import scenes_common as SC
    from obca_amd import planner as PL, scenarios as S
    res = {}
    for which in ("backwards", "parallel"):
        for tag, B, more in (("", 16, {}), ("_analytic_off", 4, dict(analytic=0.0)), ("_rs_heuristic", 4, dict(rs_heuristic=1)), ("_lattice", 4, dict(nh_res=0.5))):
            for k, a in _searches(which, B, **more).items():
                res["astar_%s%s/%s" % (which, tag, k)] = a
    # Reeds-Shepp: poses up to 30 m apart, three turning radii
    lib = PL._load(); rng = np.random.default_rng(17); n = 10000; cap = 4096
    q = np.concatenate([rng.uniform(-15, 15, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1)), rng.uniform(-15, 15, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], axis=1)
    radius = rng.choice([0.5, 4.0, 30.0], n)
    rs = np.zeros((n, 32), np.uint8)
    for i in range(n):
        path = np.zeros((cap, 3)); dr = np.zeros(cap, np.int32); word = C.create_string_buffer(8); seg = np.zeros(5); tot = C.c_double(0)
        cnt = lib.obca_plan_reeds_shepp(q[i, :3].copy(), q[i, 3:].copy(), float(radius[i]), 0.2, path, dr, cap, word, seg, C.byref(tot))
        rs[i] = _digest(np.int64(cnt), np.frombuffer(word.raw, np.uint8), seg, np.float64(tot.value), path, dr)
    res["reeds_shepp/word_seglen_total_samples"] = rs
    # the car against the two fields, poses in and a little beyond XYbounds
    e = np.ascontiguousarray(S.EGO, float); xy = np.ascontiguousarray(S.XYBOUNDS, float)
    for which in ("backwards", "parallel"):
        sc, x0, xF, kw = H.poses(which, 16)
        v, A, b = H.field(sc); n = 100000
        x = rng.uniform(xy[0] - 1, xy[1] + 1, n); y = rng.uniform(xy[2] - 1, xy[3] + 1, n); yaw = rng.uniform(-4, 4, n); m = rng.choice([0.0, 0.1], n)
        res["collides_%s/answer" % sc["name"]] = np.array([lib.obca_plan_collides(x[i], y[i], yaw[i], len(v), v, A, b, e, xy, m[i]) for i in range(n)], np.int8)
        # poses that are not numbers: the host entry points refuse none, and what they answer stays -- the test's answer, and the search's return code from such a
        # start and to such a goal
        res["collides_%s_not_finite/answer" % sc["name"]] = np.array([lib.obca_plan_collides(*p, len(v), v, A, b, e, xy, 0.1) for p in NOT_FINITE], np.int8)
        res["astar_%s_not_finite/start" % which] = np.array([_code(lambda: PL.hybrid_astar(p, xF[0], v, A, b, **kw)) for p in NOT_FINITE])
        res["astar_%s_not_finite/goal" % which] = np.array([_code(lambda: PL.hybrid_astar(x0[0], p, v, A, b, **kw)) for p in NOT_FINITE])
    # the host builds of the device planner
    for order in (0, 1, 2):
        for which in ("backwards", "parallel"):
            sc, x0, xF, kw = H.poses(which, 8)
            r = H.run_emu(sc, x0, xF, kw, order=order)
            for k in H.FIELDS:
                res["hybrid_emu_%s_order%d/%s" % (which, order, k)] = r[k]
        x0, xF, kw, fields = SC.scenes()
        r = SC.run_scenes(x0[:8], xF[:8], list(fields[:8]), kw, order=order)
        for k in H.FIELDS:
            res["scenes_emu_order%d/%s" % (order, k)] = r[k]
        x0, xF, kw, fields = R.scenes16()
        prob, z0, nObMax, MMax = R.records(x0[:8], xF[:8], list(fields[:8]))
        r = R.plan(prob, z0, nObMax, MMax, kw, order=order)
        for k in H.FIELDS + ("status", "prob", "z0", "inst"):
            res["plan_resident_emu_order%d/%s" % (order, k)] = r[k]
        res["plan_resident_emu_order%d/packed_block" % order] = R.pack_block(prob, nObMax, MMax, order)[None]
    np.savez(out, **res)


def child_time(out):
    ts = []
    for _ in range(6):      # the first run warms up: library load, thread start, the page faults of the cell tables
        t0 = time.perf_counter(); _searches("backwards", 16); _searches("parallel", 16); ts.append(time.perf_counter() - t0)
    np.savez(out, seconds=np.array(ts[1:]))


def child_device(out):
    import hybrid_common as H
    import plan_resident_common as R
    import scenes_common as SC
    import obca_amd
    from obca_amd import api, scenarios as S
    res = {}
    api.hybrid_configure(slots=16, max_nodes=H.NODES)
    x0s, xFs, kws, fields = SC.scenes()
    for which in ("backwards", "parallel"):
        sc, x0, xF, kw = H.poses(which, 8)
        v, A, b = H.field(sc); o = H.opts_array(kw)
        for k, a in zip(H.FIELDS, api.hybrid_astar_batch(x0, xF, v, A, b, S.EGO, S.L_WHEELBASE, S.XYBOUNDS, o, None, H.CAP)):
            res["hybrid_astar_batch_%s/%s" % (which, k)] = a
        # per-instance fields: the backwards poses in the first 8 scenes (these ARE the first 8 poses of the scenes), the parallel ones each in a copy of their field
        fl = list(fields[:8]) if which == "backwards" else [(v, A, b)] * 8
        for k, a in zip(H.FIELDS, api.scene_astar_batch(x0, xF, *SC.lists(fl), S.EGO, S.L_WHEELBASE, S.XYBOUNDS, o, None, H.CAP)):
            res["scene_astar_batch_%s/%s" % (which, k)] = a
    x0, xF, kw, fields = R.scenes16(); x0, xF, fields = x0[:8], xF[:8], list(fields[:8])
    z = np.zeros((8, R.N + 1))
    bt = obca_amd.Batch(api._ctx(0), 8, R.N)
    bt.upload(x0, xF, np.full(8, R.TS), S.L_WHEELBASE, S.EGO, S.XYBOUNDS, *SC.lists(fields), z, z, z, 0, None, None)
    for k, a in zip(("counts", "status", "expansions", "rounds"), bt.plan_warm_start(**kw)):
        res["plan_warm_start/%s" % k] = a
    for k, a in zip(("paths", "dirs", "inst"), bt.plan_paths()):
        res["plan_warm_start/%s" % k] = a
    res["plan_warm_start/packed_block"] = np.frombuffer(np.ascontiguousarray(bt.plan_block()[0]).tobytes(), np.uint8)[None]
    bt.close()
    np.savez(out, **res)


# ---------------------------------------------------------------- the comparison
def run_child(mode, libdir, out):
    env = dict(os.environ)
    if mode == "device":
        env["OBCA_HIP_LIBRARY"] = find(libdir, "libobca_hip.so")
    subprocess.run([sys.executable, os.path.abspath(__file__), "child", mode, libdir, out], check=True, timeout=LIMIT[mode], env=env)
    return np.load(out)


def compare(a, b):
    checks = {}
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    for k in a.files:
        x, y = a[k], b[k]
        n = len(x)
        if x.shape != y.shape or x.dtype != y.dtype:
            differ = n
        else:      # item i of a check: row i of every array, as bytes
            differ = int((np.ascontiguousarray(x).reshape(n, -1).view(np.uint8) != np.ascontiguousarray(y).reshape(n, -1).view(np.uint8)).any(axis=1).sum())
        name, field = k.split("/")
        c = checks.setdefault(name, dict(items=n, differ=0, fields={}))
        c["fields"][field] = "%d differ" % differ; c["differ"] += differ
    for c in checks.values():
        c["differ"] = "%d differ" % c["differ"]
    return checks


def kernels(path):
    """{kernel: its instructions, comments and blank lines dropped} of an assembly file, in the file's order"""
    names = [l.split()[1] for l in open(path) if l.strip().startswith(".amdhsa_kernel")]
    body, name = {}, None
    for line in open(path):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if name is None and m and m.group(1) in names:
            name = m.group(1); body[name] = []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                name = None
            elif line.split(";")[0].strip():
                body[name].append(line.split(";")[0].rstrip())
    return names, body


def asm(parent, new):
    pn, pb = kernels(parent); nn, nb = kernels(new)
    out = dict(kernels_parent=len(pn), kernels_new=len(nn), same_kernel_names=pn == nn, kernels={})
    for k in pn:
        a, b = pb[k], nb.get(k, [])
        strip = lambda ls: [re.sub(r"\.LBB\d+_\d+", ".LBB", l) for l in ls]
        out["kernels"][k] = "identical" if a == b else ("identical up to block labels" if strip(a) == strip(b) else "different (%d / %d instructions and labels)" % (len(a), len(b)))
    return out


def dump(doc, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")


def bound(doc, name, first, new, second):
    """one run of a rate tool per build, in the order parent, new, parent: is the new search-kernel time inside the parent's two, widened by their difference on either side?"""
    spread = abs(first - second)
    lim = [min(first, second) - spread, max(first, second) + spread]
    doc.setdefault("device_search_kernel_ms", {}).setdefault("runs", {})[name] = dict(parent_first_ms=first, new_ms=new, parent_second_ms=second, parent_spread_ms=spread,
                                                                                     bound_ms=lim, within=bool(lim[0] <= new <= lim[1]))
    return doc["device_search_kernel_ms"]["runs"][name]


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        _setup(sys.argv[2], sys.argv[3])
        return dict(host=child_host, time=child_time, device=child_device)[sys.argv[2]](sys.argv[4])
    if len(sys.argv) > 1 and sys.argv[1] == "bound":      # bound NAME PARENT_FIRST_MS NEW_MS PARENT_SECOND_MS [OUT]
        out = sys.argv[6] if len(sys.argv) > 6 else "profiles/planner_geom_fold_ab.json"
        doc = json.load(open(out)) if os.path.exists(out) else {}
        print(json.dumps(bound(doc, sys.argv[2], *map(float, sys.argv[3:6])), indent=1))
        return dump(doc, out)
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("host", "device", "asm"))
    ap.add_argument("parent"); ap.add_argument("new")
    ap.add_argument("--out", default="profiles/planner_geom_fold_ab.json")
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.mode == "asm":
        doc["asm"] = asm(a.parent, a.new)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            doc[a.mode] = compare(run_child(a.mode, a.parent, os.path.join(tmp, "parent.npz")), run_child(a.mode, a.new, os.path.join(tmp, "new.npz")))
            if a.mode == "host" and a.time:
                t = {w: run_child("time", d, os.path.join(tmp, "t_%s.npz" % w))["seconds"].tolist() for w, d in (("parent", a.parent), ("new", a.new))}
                p = np.array(t["parent"])
                doc["host_time_32_searches_16_threads_s"] = dict(t, parent_median=float(np.median(p)), new_median=float(np.median(t["new"])), parent_max_minus_min=float(p.max() - p.min()),
                                                               no_slower=bool(np.median(t["new"]) <= np.median(p) + (p.max() - p.min())))
    dump(doc, a.out)
    print(json.dumps(doc[a.mode] if a.mode in doc else doc, indent=1))
    bad = [k for k, c in doc.get(a.mode, {}).items() if isinstance(c, dict) and c.get("differ", "0 differ") != "0 differ"] if a.mode != "asm" else []
    if bad:
        raise SystemExit("differ: %s" % ", ".join(bad))


if __name__ == "__main__":
    main()
