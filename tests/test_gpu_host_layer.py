"""The host layer around the kernels, where the rest of the GPU suite does not pin it (run with -m gpu): the texts of the lifecycle errors both batch families
raise, and the cached batch of a context's worker lane when calls of other shapes replace it -- every result bit for bit what a fresh device-resident batch gives,
for the solves and for the validate entry points that then run on the replaced batch.  Every shape is tiny."""
import re
import numpy as np
import pytest
from obca_amd import scenarios as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def OA():
    import obca_amd
    obca_amd.Context(0).close()      # fails loudly if the HIP library / device is missing
    return obca_amd


@pytest.fixture()
def ctx(OA):
    c = OA.Context(0)                # a context of its own per test: its lanes start without a cached batch
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_bits(a, b, keys, what):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and _bits(x) == _bits(y), (what, k)


def _parking_args(bt, N):
    xWS = bt["xWS"].copy(); xWS[:, 0, :] = bt["x0"]
    return (bt["x0"], bt["xF"]), (bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], xWS[:, :, 0], xWS[:, :, 1], xWS[:, :, 2], 0, xWS, bt["uWS"])


def test_lifecycle_errors_keep_their_texts(OA, ctx):
    """the expected texts are those of obca_batch_solve / quad_solve / obca_[quad_]batch_validate_ms in the C ABI's source before the two families shared a core"""
    B = 2
    pb = OA.Batch(ctx, B, 4); qb = OA.QuadBatch(ctx, B, 4)
    with pytest.raises(OA.ObcaError, match=re.escape("obca_batch_solve: nothing uploaded")):
        pb.solve()
    with pytest.raises(OA.ObcaError, match=re.escape("obca_quad_batch_solve: nothing uploaded")):
        qb.solve()
    with pytest.raises(OA.ObcaError, match=re.escape("obca_batch_validate_ms: no validate call has run on this batch")):
        pb.validate_ms()
    with pytest.raises(OA.ObcaError, match=re.escape("obca_quad_batch_validate_ms: no validate call has run on this batch")):
        qb.validate_ms()
    q = S.make_quad_batch(B, 4)
    qb.upload(q["x0"], q["xF"], q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"])
    o = OA.quadcopter_default_opts(); o.recalc_y = 1
    with pytest.raises(OA.ObcaError, match=re.escape("quadcopter solve: recalc_y is a switch of the parking kernels only")):
        qb.solve(opts=o)
    with pytest.raises(OA.ObcaError, match=re.escape("obca_quad_batch_validate_ms: no validate call has run on this batch")):      # (an upload is no validate)
        qb.validate_ms()
    (x0, xF), rest = _parking_args(S.make_batch(S.BACKWARDS, B, 4, seed=5), 4)
    pb.upload(x0, xF, *rest)
    with pytest.raises(OA.ObcaError, match=re.escape("obca_batch_validate_ms: no validate call has run on this batch")):
        pb.validate_ms()
    pb.close(); qb.close()


PARK_KEYS = ("xp", "up", "timeScale", "exitflag", "lp", "np", "sl", "info")
QUAD_KEYS = ("xp", "up", "timeScale", "exitflag", "lp", "slack", "info")


def test_parking_slot_batch_replacement_is_bit_neutral(OA, ctx):
    """(B, N) = (3, 8), (5, 10), (3, 8) through the host-pointer entry of ONE context: its lane's cached batch is created, replaced by a larger one of another horizon,
    replaced again; every result equals a fresh resident Batch's, and the host-pointer validate on the batch replaced last equals that Batch's resident validate()"""
    fresh = OA.Context(0)
    outs = []
    for B, N in ((3, 8), (5, 10), (3, 8)):
        bt = S.make_batch(S.BACKWARDS, B, N, seed=11)
        (x0, xF), rest = _parking_args(bt, N)
        out = OA.parking_signed_dist_batch(x0, xF, N, *rest, device=ctx)
        b = OA.Batch(fresh, B, N)
        b.upload(x0, xF, *rest); b.solve()
        ref = b.download(); val = b.validate(); b.close()
        _same_bits(out, ref, PARK_KEYS, "parking host-pointer call against a resident batch, B=%d N=%d" % (B, N))
        outs.append(out)
    _same_bits(outs[0], outs[2], PARK_KEYS, "first against third parking call")
    assert np.isfinite(out["xp"]).all() and (out["iters"] > 0).all()
    host = OA.parking_constraints_batch(x0, xF, N, bt["Ts"], bt["L"], bt["ego"], bt["XYbounds"], bt["vOb"], bt["A"], bt["b"], out["xp"], out["up"], out["timeScale"],
                                        out["lp"], out["np"], out["sl"], device=ctx)
    _same_bits(host, val, ("ok", "ref_ok", "viol"), "parking_constraints_batch against Batch.validate")
    fresh.close()


def test_quadcopter_slot_batch_replacement_is_bit_neutral(OA, ctx):
    """the same walk for the quadcopter family: (B, N) = (2, 8), (3, 10), (2, 8)"""
    fresh = OA.Context(0)
    outs = []
    for B, N in ((2, 8), (3, 10), (2, 8)):
        q = S.make_quad_batch(B, N)
        out = OA.quadcopter_signed_dist_batch(q["x0"], q["xF"], N, q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"], device=ctx)
        b = OA.QuadBatch(fresh, B, N)
        b.upload(q["x0"], q["xF"], q["Ts"], q["R"], q["ob"], q["xWS"], q["timeWS"]); b.solve()
        ref = b.download(); val = b.validate(); b.close()
        _same_bits(out, ref, QUAD_KEYS, "quadcopter host-pointer call against a resident batch, B=%d N=%d" % (B, N))
        outs.append(out)
    _same_bits(outs[0], outs[2], QUAD_KEYS, "first against third quadcopter call")
    assert np.isfinite(out["xp"]).all() and (out["iters"] > 0).all()
    host = OA.quadcopter_constr_satisfaction_batch(out["xp"], out["up"], out["timeScale"], q["x0"], q["xF"], q["Ts"], out["lp"], q["ob"], q["R"], device=ctx)
    _same_bits(host, val, ("ok", "viol"), "quadcopter_constr_satisfaction_batch against QuadBatch.validate")
    fresh.close()
