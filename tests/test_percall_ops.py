"""The per-call operators' routes against each other (csrc/pekf_percall.hip: one operator table, read by the
batched kernel k_op<Op>, the n = 1 routes and the host entry points).

Every route runs the table's body on the same operands, so results are compared bit for bit: the
device-pointer entries against the host-pointer ones, a status plane against the unmodified call, the
resident service against a launch per call.  Shapes: n = 1 (the by-value route), 65 (a full wave plus a
one-lane tile) and 257 (a second block holding one item); inputs are tests/golden/kat.npz rows tiled to 512.
"""
from __future__ import annotations

import numpy as np
import pytest

from poseestimationkf_amd._lib import check, lib

pytestmark = pytest.mark.gpu

ROWS = 512
PREDICT = ("pc_gyro", "pc_dt", "pc_X", "pc_P", "pc_Q", "pc_R")
CORRECT = ("pc_mag", "pc_acc", "pc_z", "pc_Pm", "pc_K", "pc_acc0", "pc_mag0")
RK4 = ("rk4_q0", "rk4_dt", "rk4_w")
WAHBA = ("wahba_acc0", "wahba_mag0", "wahba_acc", "wahba_mag", "wahba_ka", "wahba_km")


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    prev = engine.percall_mode()
    yield engine
    engine.percall_mode(prev)


@pytest.fixture(scope="module")
def rows(kat):
    """kat.npz's operands, each tiled to ROWS rows (read-only)."""
    out = {}
    for k in PREDICT + CORRECT + RK4 + WAHBA + ("jac_w", "jac_q", "cmp_q1", "cmp_q2", "r2q_M"):
        a = np.concatenate([kat[k]] * -(-ROWS // len(kat[k])))[:ROWS]
        a.setflags(write=False)
        out[k] = a
    return out


def _dev_call(eng, fn, ins, out_widths, n, status=None):
    """fn(n, device inputs, device outputs[, status plane], stream) on the first n rows of ins -> the outputs
    (and the status plane when status is True; status=False passes NULL, None: the entry takes none)."""
    bi = [eng.DeviceBuffer(a[:n].nbytes).upload(a[:n]) for a in ins]
    bo = [eng.DeviceBuffer(8 * n * w) for w in out_widths]
    tail = []
    if status is not None:
        sb = eng.DeviceBuffer(4 * n).upload(np.full(n, -1, np.int32))
        tail = [sb.ptr if status else None]
    check(fn(n, *[b.ptr for b in bi], *[b.ptr for b in bo], *tail, None))
    got = [b.download((n, w), np.float64) for b, w in zip(bo, out_widths)]
    if status:
        got.append(sb.download((n,), np.int32))
    return got


def _same_rows(dev, host):
    assert len(dev) == len(host)
    for d, h in zip(dev, host):
        assert np.array_equal(d, h.reshape(d.shape), equal_nan=True)


@pytest.mark.parametrize("n", [1, 65, 257])
def test_dev_entries_match_host_entries(eng, rows, n):
    """pekf_rk4_dev / pekf_predict_dev / pekf_correct_dev on DeviceBuffers give the host-pointer entries' rows."""
    rk = [rows[k] for k in RK4]
    _same_rows(_dev_call(eng, lib.pekf_rk4_dev, rk, (4,), n), [eng.rk4(*[a[:n] for a in rk])])
    pc = [rows[k] for k in PREDICT]
    host = eng.predict(*[a[:n] for a in pc])
    _same_rows(_dev_call(eng, lib.pekf_predict_dev, pc, (4, 16, 16), n, status=False), host)
    *got, st = _dev_call(eng, lib.pekf_predict_dev, pc, (4, 16, 16), n, status=True)
    _same_rows(got, host)
    assert not st.any()
    cc = [rows[k] for k in CORRECT]
    _same_rows(_dev_call(eng, lib.pekf_correct_dev, cc, (4, 16), n), eng.correct(*[a[:n] for a in cc]))


def test_predict_dev_status_plane_marks_exactly_the_singular_items(eng, rows):
    n, bad = 257, [0, 64, 256]   # first lane, first lane of the second wave, the second block's only item
    pc = [rows[k][:n].copy() for k in PREDICT]
    *ref, st0 = _dev_call(eng, lib.pekf_predict_dev, pc, (4, 16, 16), n, status=True)
    assert not st0.any()
    for k in (0, 3, 4, 5):       # zero gyro, P = Q = R = 0: S = P^- + R is singular
        pc[k][bad] = 0.0
    z, Pm, K, st = _dev_call(eng, lib.pekf_predict_dev, pc, (4, 16, 16), n, status=True)
    hit = np.zeros(n, bool)
    hit[bad] = True
    assert np.array_equal(st, hit.astype(np.int32))
    assert np.array_equal(np.isnan(K).all(axis=1), hit) and np.array_equal(np.isnan(K).any(axis=1), hit)
    for got, want in zip((z, Pm, K), ref):
        assert np.array_equal(got[~hit], want[~hit])
    with pytest.raises(np.linalg.LinAlgError):
        eng.predict(*pc)


def test_service_response_carries_no_stale_tail(eng, rows):
    """Service mode answers every n = 1 operator as launch mode does right after a predict, whose 36 outputs
    fill more of the response area than any other operator's (wahba_rotation: 9, jacobian_a: 16)."""
    i = 5
    one = lambda keys: [rows[k][i] for k in keys]
    calls = [(eng.wahba_rotation, one(WAHBA)), (eng.jacobian_a, one(("jac_w",))), (eng.correct, one(CORRECT)),
             (eng.wahba_quaternion, one(WAHBA)), (eng.rk4, one(RK4)), (eng.jacobian_b, one(("jac_q",))),
             (eng.comparator, one(("cmp_q1", "cmp_q2"))), (eng.rotmat_to_quat, one(("r2q_M",)))]
    outputs = lambda r: r if isinstance(r, tuple) else (r,)
    eng.percall_mode(eng.PERCALL_LAUNCH)
    want = [outputs(fn(*args)) for fn, args in calls]
    eng.percall_mode(eng.PERCALL_SERVICE)
    for (fn, args), w in zip(calls, want):
        eng.predict(*one(PREDICT))
        got = outputs(fn(*args))
        assert len(got) == len(w)
        for g, x in zip(got, w):
            assert np.array_equal(g, x, equal_nan=True), fn.__name__
