"""The two-arc Wahba quaternion with its weights folded into the core, on the device (pekf_math.hpp:
wahba_product_ref forms (C, S) = T + ka (. - T) and never km = 1 - ka; wahba_toward_from_product sends
!(ka <= 1) to the matrix chain).  tests/test_wahba_folded_cpu.py holds the NumPy restatement.

256 filters x 64 records through pekf_run_dev: one block, both halves of the ping-pong loop.  Final X and P
against the C oracle on the same records to test_gpu_parity's PREC_GUARD, every lane.

Groups of 32 filters, their sensors remounted by a rotation per filter as tests/test_wahba_two_arc.py
remounts them (gyro, acc and mag in FP64, then rounded to f32; the reference pair rotated in FP64), here so
that the first record's acc has |acc_z| / |acc| = 0.04, 0.5 or 1, up in the even lanes and down in the odd
ones.  The streams stay consistent, so every lane is tracked.
  * ka = |acc_z| = 0.04 and 0.5 at the first record: both terms of the blend carry weight.
  * ka = 1 - 2^-24, the f32 next below 1, written into acc_z of the first four records of a group mounted
    at 1 (they hold |acc_z| > 0.99 before it): C is nearly aW a'_x, and T1 cancels in T1 + ka (aW a'_x - T1).
  * ka = 1 + 2^-23, the f32 next above 1, likewise: km < 0, the reflection case, which the product form does
    not serve.  The reference's rotation there is the product form's turned by about half a turn about z
    (asserted on the inputs below), so these lanes agree with the oracle only through the matrix chain.
The other 128 filters run the stream as generated.

The same records give the same bits under the default, PIN and HOIST schedules, in two launches of 32
records against one of 64, and through pekf_run_rec64_dev.  A session (run_session: k_live) makes its own
records from a phone's events -- normalised, then low-passed from zero, so their ka climbs from 0 towards
|acc_z| / |acc| < 1 and the group above 1 cannot be stated there -- so the session runs one event stream
remounted to the same three directions at phase 3's first acc sample, and its state is compared bit for
bit with the split pipeline's (frontend_init -> run_frontend -> BatchedEKF.run) on the same events.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import ekf_numpy as npo
from poseestimationkf_amd import synth

from .test_gpu_parity import PREC_GUARD
from .test_live import _same as _same_tuple
from .test_live import _split
from .test_wahba_folded_cpu import folded
from .test_wahba_two_arc import K, W, _launch, _maxerr, _same, eng  # noqa: F401
from .test_wahba_two_arc_cpu import arc_to, pair_in_own_frame, quat_rotm

pytestmark = pytest.mark.gpu

BELOW = np.nextafter(np.float32(1), np.float32(0))      # 1 - 2^-24
ABOVE = np.nextafter(np.float32(1), np.float32(2))      # 1 + 2^-23
GROUPS = {   # filters, |acc_z| / |acc| the first record is mounted at, the value written into its first records
    "ka 0.04": (range(0, 32), 0.04, None),
    "ka 0.5": (range(32, 64), 0.5, None),
    "ka next below 1": (range(64, 96), 1.0, BELOW),
    "ka next above 1": (range(96, 128), 1.0, ABOVE),
}
EXACT_AT = (0, 1, 2, 3)
PHI = 0.7                       # the mounted acc's azimuth
E2, E3 = 800, 400               # the session's phase-2 and phase-3 events per phone


def _mount(a, z_over_norm):
    """(k, 3, 3): per filter the shortest arc taking a's direction to (s cos PHI, s sin PHI, +-t), t the
    wanted |a_z| / |a| and s = sqrt(1 - t^2); up in the even filters, down in the odd ones."""
    u = a / np.linalg.norm(a, axis=-1, keepdims=True)
    t = float(z_over_norm)
    s = np.sqrt(1.0 - t * t)
    side = np.where(np.arange(len(a)) % 2 == 0, 1.0, -1.0)
    v = np.stack([np.full(len(a), s * np.cos(PHI)), np.full(len(a), s * np.sin(PHI)), side * t], axis=-1)
    return arc_to(u, v)


def folded_stream():
    """(records, X0, P0): the tracked stream with the filters of GROUPS remounted and their exact ka written"""
    rec = synth.generate(np.arange(K), W, seed=47)
    for cols, t, exact in GROUPS.values():
        cols = list(cols)
        M = _mount(rec.acc[0, cols].astype(np.float64), t)
        g, a, m = (np.einsum("kij,wkj->wki", M, arr[:, cols].astype(np.float64))
                   for arr in (rec.gyro, rec.acc, rec.mag))
        rec.gyro[:, cols], rec.acc[:, cols], rec.mag[:, cols] = (v.astype(np.float32) for v in (g, a, m))
        rec.acc0[cols] = np.einsum("kij,kj->ki", M, rec.acc0[cols])
        rec.mag0[cols] = np.einsum("kij,kj->ki", M, rec.mag0[cols])
        if exact is not None:
            for r in EXACT_AT:
                assert (np.abs(rec.acc[r, cols, 2]) > 0.99).all()
                rec.acc[r, cols, 2] = np.copysign(exact, rec.acc[r, cols, 2])
    X0 = np.tile(np.array([1.0, 0, 0, 0]), (K, 1))
    P0 = np.tile(np.eye(4), (K, 1, 1))
    return rec, X0, P0


def assert_inputs(rec):
    """The inputs are what the docstring says they are (NumPy only)."""
    ka = np.abs(rec.acc[..., 2].astype(np.float64))
    for name, (cols, t, exact) in GROUPS.items():
        cols = list(cols)
        if exact is None:
            assert np.abs(ka[0, cols] - t).max() < 1e-6, name
        else:
            assert (ka[list(EXACT_AT)][:, cols] == np.float64(exact)).all(), name
        assert (rec.acc[0, cols[0::2], 2] > 0).all() and (rec.acc[0, cols[1::2], 2] < 0).all()
    assert float(BELOW) == 1 - 2.0 ** -24 and float(ABOVE) == 1 + 2.0 ** -23
    below, above = list(GROUPS["ka next below 1"][0]), list(GROUPS["ka next above 1"][0])
    assert (ka[0, below] <= 1.0).all() and not (ka[0, above] <= 1.0).any()
    # the product form against the reference's rotation at the first record, in the reference frame's basis
    aW, b1W, b2W, Fw = pair_in_own_frame(rec.acc0, rec.mag0)
    a, m = rec.acc[0].astype(np.float64), rec.mag[0].astype(np.float64)
    q = folded(a, m, aW, b1W, b2W)
    Rq = quat_rotm(q / np.sqrt((q * q).sum(-1))[..., None])
    dist = np.empty(K)
    for k in below + above:
        R = npo.svd_rotation(rec.acc0[k], rec.mag0[k], a[k], m[k], ka[0, k], 1 - ka[0, k])
        dist[k] = np.abs(Rq[k] - Fw[k].T @ R).max()
    print("product form against the reference's rotation: ka below 1 max %.3e, ka above 1 min %.3e"
          % (dist[below].max(), dist[above].min()))
    assert dist[below].max() < 1e-6 and dist[above].min() > 1.0


@pytest.fixture(scope="module")
def case(oracle_c):
    """(records, X0, P0, Xo, Po): the stream, checked, and the oracle's final state, checked alone first."""
    rec, X0, P0 = folded_stream()
    assert_inputs(rec)
    Xo, Po, _ = oracle_c.run(rec, X=X0, P=P0)
    assert np.isfinite(Xo).all() and np.isfinite(Po).all()
    assert np.abs(np.linalg.norm(Xo, axis=1) - 1.0).max() < 1e-12
    return rec, X0, P0, Xo, Po


def test_every_group_against_the_oracle(eng, case):
    rec, X0, P0, Xo, Po = case
    X, P = _launch(eng, eng.IMUWindow.from_records(rec), X0, P0)
    for name, (cols, _, _) in GROUPS.items():
        cols = list(cols)
        print("folded core, %s: max |dX| = %.3e, max |dP| = %.3e"
              % (name, _maxerr(X[cols], Xo[cols]), _maxerr(P[cols], Po[cols])))
    print("folded core, all 256 lanes: max |dX| = %.3e, max |dP| = %.3e" % (_maxerr(X, Xo), _maxerr(P, Po)))
    assert _maxerr(X, Xo) < PREC_GUARD and _maxerr(P, Po) < PREC_GUARD
    assert np.abs(np.linalg.norm(X, axis=1) - 1.0).max() < 1e-13


def test_schedules_bit_identical(eng, case, monkeypatch):
    rec, X0, P0, _, _ = case
    win = eng.IMUWindow.from_records(rec)
    monkeypatch.delenv("PEKF_RUN_PIN", raising=False)
    monkeypatch.delenv("PEKF_RUN_HOIST", raising=False)
    Xd, Pd = _launch(eng, win, X0, P0)                  # the library's own choice
    assert np.isfinite(Xd).all() and np.isfinite(Pd).all()
    for pin, hoist in (("0", "0"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("PEKF_RUN_PIN", pin)
        monkeypatch.setenv("PEKF_RUN_HOIST", hoist)
        X, P = _launch(eng, win, X0, P0)
        assert _same(X, Xd) and _same(P, Pd), (pin, hoist)


def test_two_chunks_and_fp64_records_bit_identical(eng, case):
    rec, X0, P0, _, _ = case
    X1, P1 = _launch(eng, eng.IMUWindow.from_records(rec), X0, P0)
    Xa, Pa = _launch(eng, eng.IMUWindow.from_records(rec), X0, P0, ((W // 2, 0), (W // 2, W // 2)))
    w64 = eng.RecordWindow64.from_arrays(rec.gyro.astype(np.float64), rec.dt_ns, rec.acc.astype(np.float64),
                                         rec.mag.astype(np.float64), rec.acc0, rec.mag0)
    X64, P64 = _launch(eng, w64, X0, P0)
    assert np.isfinite(X1).all() and np.isfinite(P1).all()
    assert _same(Xa, X1) and _same(Pa, P1)              # 2 x 32 records against one launch of 64
    assert _same(X64, X1) and _same(P64, P1)            # pekf_run_rec64_dev on the same values


def session_events():
    """(phase2, phase3): one phone stream per filter, split after E2 events, remounted per group so that
    phase 3's first acc sample points where folded_stream mounts the first record's acc."""
    ev = synth.generate_events(np.arange(K), E2 + E3, seed=48)
    vals = ev["values"].astype(np.float64)
    init_acc, init_mag = ev["init_acc"].copy(), ev["init_mag"].copy()
    first = np.argmax(ev["types"][E2:] == synth.EV_ACC, axis=0) + E2    # phase 3's first acc event, per phone
    a1 = vals[first, np.arange(K)]
    for cols, t, _ in GROUPS.values():
        cols = list(cols)
        M = _mount(a1[cols], min(t, 1.0))
        vals[:, cols] = np.einsum("kij,ekj->eki", M, vals[:, cols])
        init_acc[cols] = np.einsum("kij,kj->ki", M, init_acc[cols])
        init_mag[cols] = np.einsum("kij,kj->ki", M, init_mag[cols])
    ev = dict(ev, values=vals.astype(np.float32), init_acc=init_acc, init_mag=init_mag)
    a1 = ev["values"][first, np.arange(K)].astype(np.float64)
    ratio = np.abs(a1[:, 2]) / np.linalg.norm(a1, axis=1)
    for cols, t, _ in GROUPS.values():
        assert np.abs(ratio[list(cols)] - min(t, 1.0)).max() < 1e-6
    cut = lambda lo, hi: dict(ev, types=ev["types"][lo:hi], values=ev["values"][lo:hi], times=ev["times"][lo:hi])  # noqa: E731
    return cut(0, E2), cut(E2, E2 + E3)


def test_session_equals_split_pipeline(eng):
    ph2, ph3 = session_events()
    f = eng.BatchedEKF(K)
    got = eng.run_session(ph2, ph3, f, records="f32")
    assert got["ready"].all() and got["counts"].min() >= 8
    ini = eng.frontend_init(ph2)
    ev3 = dict(ph3, t_init=ini["t_init"], init_acc=ini["init"][:, :3], init_mag=ini["init"][:, 3:])
    X, P = f.get_state()
    assert np.isfinite(X).all() and np.isfinite(P).all()
    print("session: %d..%d records per filter" % (got["counts"].min(), got["counts"].max()))
    _same_tuple((X, P, got["counts"], got["refs"]), _split(eng, ev3, K))
