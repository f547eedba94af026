"""One step of the closed receding-horizon loop on the device (include/obca_advance.h) through the C ABI: against the host build of the same kernel text
(tests/emu/advance_emu.cpp) fed the batch's own download; against the EXISTING route -- rollout(), rollout_states(), the slice, shift_warm_start(x0_new) -- on a second,
identically uploaded and solved batch; a closed loop of five steps against the same loop routed through the host; the refusals; more workgroups than compute units.
Instances, comparison rules and tolerances: tests/advance_common.py."""
import numpy as np
import pytest
import advance_common as A
import rollout_common as R
from obca_amd import scenarios as S, validate as V
from test_gpu_rollout import record as rollout_record

pytestmark = pytest.mark.gpu
WORST = {}
SHIFT, SUB = 2, 8


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.build_library()
    return obca_amd


@pytest.fixture(scope="module")
def ctx(OA):
    c = OA.Context(0)
    yield c
    c.close()


def record(r, i):
    """row i of a returned dict, back in the layout of the C record"""
    out = rollout_record(r, i)
    out[12], out[13], out[14], out[15] = r["shift"][i], r["driven_time"][i], r["goal_dist"][i], r["logged"][i]
    return out


def _bits(a):
    return np.ascontiguousarray(a, float).view(np.uint64)


def _same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b))


def _same_out(a, b):
    """two downloads, every output, bit for bit"""
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, (list, tuple)):
            if not (len(x) == len(y) and all(_same(p, q) for p, q in zip(x, y))):
                return False
        elif isinstance(x, np.ndarray) and x.dtype.kind == "f":
            if not _same(x, y):
                return False
        elif not np.array_equal(x, y):
            return False
    return True


def _tile(bt, B, n):
    """the batch dict with instance i % B in row i, n rows"""
    idx = np.arange(n) % B; out = {}
    for k, v in bt.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B:
            out[k] = v[idx]
        elif isinstance(v, list) and len(v) == B:
            out[k] = [v[j] for j in idx]
        else:
            out[k] = v
    return out


# ---------------------------------------------------------------- the two vehicles behind one interface
class Park:
    nx, need = 4, V.DMIN

    def __init__(self, bt):
        self.bt, self.B, self.N = bt, len(bt["x0"]), bt["N"]

    def batch(self, OA, ctx):
        bt = self.bt; xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
        b = OA.Batch(ctx, self.B, self.N)
        b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])
        return b

    def opts(self, OA, warm, max_iter=None):
        o = OA.warm_restart_opts() if warm else OA.default_opts()
        if max_iter is not None:
            o.max_iter = max_iter
        return o

    def next_start(self, OA, b):
        """the start the next solve begins from, as the shift tests read it: a max_iter = 0 solve and its download"""
        b.solve(self.opts(OA, True, 0))
        return b.download()

    def _obst(self, i):
        bt = self.bt
        return (bt["vOb"][i], bt["A"][i], bt["b"][i]) if isinstance(bt["vOb"], list) else (bt["vOb"], bt["A"], bt["b"])

    def vmax(self):
        return max(int(np.max(self._obst(i)[0])) for i in range(self.B))

    def host(self, o, i, x0, shift, kick):
        """(record, state) of the host build for instance i of the download o, the plant at x0"""
        bt = self.bt; v, Am, bv = self._obst(i)
        c = dict(N=self.N, Ts=float(bt["Ts"][i]), L=bt["L"], ego=bt["ego"], vOb=np.asarray(v, np.int32), A=np.asarray(Am, float), b=np.asarray(bv, float), x=o["xp"][i], u=o["up"][i],
                 ts=o["timeScale"][i])
        e = A.emu_parking([A.park_instance(c, x0=x0, xF=bt["xF"][i])], shift, SUB, kick, self.need, vmax=self.vmax())
        return e["out"][0], e["st"][0]


class Quad:
    nx, need = 12, 0.0

    def __init__(self, bt, B, N):
        self.bt, self.B, self.N = bt, B, N

    def batch(self, OA, ctx):
        bt = self.bt; b = OA.QuadBatch(ctx, self.B, self.N)
        b.upload(bt["x0"], bt["xF"], bt["Ts"], bt["R"], bt["ob"], bt["xWS"], bt["timeWS"])
        return b

    def opts(self, OA, warm, max_iter=None):
        o = OA.quad_warm_restart_opts() if warm else OA.quadcopter_default_opts()
        if max_iter is not None:
            o.max_iter = max_iter
        return o

    def next_start(self, OA, b):
        xws, tws = b.warm_start()
        return dict(xWS=xws, timeWS=tws)

    def host(self, o, i, x0, shift, kick):
        bt = self.bt
        c = dict(N=self.N, Ts=float(bt["Ts"]), R=bt["R"], ob=bt["ob"], x=o["xp"][i], u=o["up"][i], ts=o["timeScale"][i])
        e = A.emu_quad([A.quad_instance(c, x0=x0, xF=bt["xF"][i])], shift, SUB, kick, None, self.need)
        return e["out"][0], e["st"][0]


def _vehicle(name):
    if name == "parking":
        return Park(S.make_batch(S.BACKWARDS, 16, 30))
    if name == "ragged":
        return Park(S.make_mixed_batch(16, 20, seed=5, min_obstacles=1, max_extra=13, rows=(3, 8), max_rows=64))
    return Quad(S.make_quad_batch(16, 20), 16, 20)


VEHICLES = ["parking", "ragged", "quad"]


def _kick(v, seed):
    """a fixed seeded disturbance of 0.02 on the positions"""
    k = np.zeros((v.B, v.nx)); npos = 2 if v.nx == 4 else 3
    k[:, :npos] = 0.02 * np.random.default_rng(seed).standard_normal((v.B, npos))
    return k


# ---------------------------------------------------------------- 1. device against host build
@pytest.mark.parametrize("name", VEHICLES)
def test_device_matches_the_host_build(OA, ctx, name):
    """record and plant state within 1e-9 max(1, |value|) of the host build fed the device's own solution; flags, indices and counts equal.  Measured on an MI355X:
    4.3e-15 (parking), 1.7e-14 (ragged), 1.1e-14 (quadcopter) at most.  shift 2 with a kick, and shift 0 (the plant stands: X0 + kick to the bit)."""
    v = _vehicle(name); b = v.batch(OA, ctx)
    try:
        x0 = np.reshape(v.bt["x0"], (v.B, v.nx)).astype(float)
        for shift, seed in ((SHIFT, 1), (0, 2)):
            b.solve(v.opts(OA, shift == 0)); o = b.download(); kick = _kick(v, seed)
            r = b.advance(shift, SUB, kick=kick, need=v.need); st = b.advance_state()
            assert r["finite"].all() and (r["shift"] == shift).all() and (r["logged"] == -1).all() and (r["substeps"] == SUB).all() and b.advance_ms() > 0
            for i in range(v.B):
                hrec, hst = v.host(o, i, x0[i], shift, kick[i]); dev = record(r, i)
                WORST[name] = max(WORST.get(name, 0.0), R.worst(dev[A.REAL], hrec[A.REAL]), R.worst(st[i], hst))
                A.check_record(dev, hrec, A.TOL_DEV, (name, shift, i))      # (indices and counts equal)
                assert R.close(st[i], hst, A.TOL_DEV), (name, shift, i)
            if shift == 0:
                assert _same(st, x0 + kick)
            x0 = st      # the plant stands where the step left it: X0 of the record
        print("largest difference device - host build, %s: %.3g" % (name, WORST[name]))
    finally:
        b.close()


# ---------------------------------------------------------------- 2. against the existing route
@pytest.mark.parametrize("name", VEHICLES)
def test_the_fused_call_is_the_existing_pipeline(OA, ctx, name):
    """Two identically uploaded and solved batches: a runs advance(shift), b runs shift_warm_start(shift, x0_new=a.advance_state()).  The next starts are bit-equal and
    so is every output of the following full solves.  Separately a.advance_state() against b.rollout(restart=False), rollout_states()[:, shift] taken before b's shift:
    1e-12 relative is asserted.  Measured on an MI355X: bit-equal for all three batches (the solution's node 0 is X0 to the bit, and both kernels run the same
    roll::integrate)."""
    v = _vehicle(name); a = v.batch(OA, ctx); b = v.batch(OA, ctx)
    try:
        a.solve(v.opts(OA, False)); b.solve(v.opts(OA, False))
        assert _same_out(a.download(), b.download())
        b.rollout(SUB, restart=False, need=v.need); Xr = b.rollout_states()[:, SHIFT]
        r = a.advance(SHIFT, SUB, need=v.need); st = a.advance_state()
        assert r["finite"].all() and R.close(st, Xr, 1e-12), R.worst(st, Xr)
        print("advance_state() against rollout_states()[:, shift], %s: worst %.3g, bit-equal %s" % (name, R.worst(st, Xr), _same(st, Xr)))
        b.shift_warm_start(SHIFT, x0_new=st)
        with pytest.raises(OA.ObcaError, match="nothing has been solved"):      # a counts as unsolved, exactly as b does
            a.advance(SHIFT, SUB)
        sa, sb = v.next_start(OA, a), v.next_start(OA, b)
        assert _same_out(sa, sb)
        a.solve(v.opts(OA, True)); b.solve(v.opts(OA, True))
        oa, ob = a.download(), b.download()
        assert _same_out(oa, ob) and _same(np.asarray(oa["xp"])[:, :, 0], st)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------- 3. a closed loop
@pytest.mark.parametrize("name", ["parking", "quad"])
def test_five_closed_loop_steps_equal_the_loop_routed_through_the_host(OA, ctx, name):
    """shift 2, a fixed seeded kick of 0.02 on the positions: batch a advances on the device, batch b is restarted through the host from a's plant state.  Exit flags,
    iteration counts and downloads are equal at every step; the log holds the plant's path -- its last node of a step is the plant state to the bit, the node before
    agrees with b's chain rollout within 1e-12 relative."""
    v = _vehicle(name); a = v.batch(OA, ctx); b = v.batch(OA, ctx); steps = 5
    try:
        a.advance_log(2 * steps); states = []
        for k in range(steps):
            a.solve(v.opts(OA, k > 0)); b.solve(v.opts(OA, k > 0))
            oa, ob = a.download(), b.download()
            assert np.array_equal(oa["exitflag"], ob["exitflag"]) and np.array_equal(oa["iters"], ob["iters"]) and _same_out(oa, ob), (name, k)
            b.rollout(SUB, restart=False, need=v.need); mid = b.rollout_states()[:, 1]
            r = a.advance(SHIFT, SUB, kick=_kick(v, 10 + k), need=v.need); st = a.advance_state()
            ok = r["finite"]
            assert ok.all() and (r["logged"] == 2 * k + 2).all(), (name, k)
            b.shift_warm_start(SHIFT, x0_new=st)
            states += [mid, st]
        log = a.advance_log_states()
        assert log.shape == (v.B, 2 * steps, v.nx)
        for j, X in enumerate(states):
            assert _same(log[:, j], X) if j % 2 else R.close(log[:, j], X, 1e-12), (name, j, R.worst(log[:, j], X))
        with pytest.raises(OA.ObcaError, match="log is full"):
            a.solve(v.opts(OA, True)); a.advance(1, SUB)
        assert _same(a.advance_log_states(), log)
        a.advance_log(0)
        with pytest.raises(OA.ObcaError, match="no log"):
            a.advance_log_states()
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------- 4. the refusals
@pytest.mark.parametrize("name", ["parking", "quad"])
def test_refusals(OA, ctx, name):
    v = _vehicle(name); b = v.batch(OA, ctx)
    try:
        with pytest.raises(OA.ObcaError, match="nothing has been solved"):
            b.advance(SHIFT)
        with pytest.raises(OA.ObcaError, match="no advance has run"):
            b.advance_state()
        b.solve(v.opts(OA, False)); before = v.next_start(OA, b) if name == "quad" else None
        for kw, msg in ((dict(shift=v.N + 1), "shift out of range"), (dict(shift=-1), "shift out of range"), (dict(substeps=0), "substeps"), (dict(substeps=33), "substeps"),
                        (dict(need=np.nan), "finite `need`")):
            with pytest.raises(OA.ObcaError, match=msg):
                b.advance(**dict(dict(shift=SHIFT), **kw))
        if name == "quad":
            xf = np.array(v.bt["xF"], float).reshape(v.B, 12); xf[3, 1] = np.inf
            with pytest.raises(OA.ObcaError, match="xF_new"):
                b.advance(SHIFT, xF_new=xf)
            assert _same_out(v.next_start(OA, b), before)      # nothing was written by a refused call
        assert b.advance(SHIFT)["finite"].all()
        with pytest.raises(OA.ObcaError, match="nothing has been solved"):      # a second advance without a solve in between
            b.advance(SHIFT)
    finally:
        b.close()


# ---------------------------------------------------------------- 5. more workgroups than compute units
@pytest.mark.parametrize("name", ["parking", "quad"])
def test_260_instances_repeat_the_first_16_bit_for_bit(OA, ctx, name):
    v16 = _vehicle(name); n = 260
    v = Park(_tile(v16.bt, 16, n)) if name == "parking" else Quad(_tile(v16.bt, 16, n), n, 20)
    b = v.batch(OA, ctx)
    try:
        b.solve(v.opts(OA, False)); b.advance_log(SHIFT)
        kick = _kick(v16, 3)[np.arange(n) % 16]
        r = b.advance(SHIFT, SUB, kick=kick, need=v.need); st = b.advance_state(); log = b.advance_log_states(); nxt = v.next_start(OA, b)
        assert r["finite"].all() and log.shape == (n, SHIFT, v.nx) and _same(log[:, -1], st)
        for i in range(16, n):
            assert _same(record(r, i), record(r, i % 16)) and _same(st[i], st[i % 16]) and _same(log[i], log[i % 16]), i
        for k, x in nxt.items():
            if isinstance(x, np.ndarray) and x.shape[:1] == (n,):
                assert _same(x[16:], x[np.arange(16, n) % 16]), k
    finally:
        b.close()
