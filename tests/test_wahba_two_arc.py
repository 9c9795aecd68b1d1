"""Wahba's quaternion from two plane rotations on the device (pekf_math.hpp: wahba_product_ref and
wahba_toward_from_product, the reference-basis measurement of every multi-record kernel).

q' ~ q_theta (x) q_1: q_1 the shortest arc taking the measured plane's normal n = acc x mag to z, q_theta
the best rotation about z, (cos, sin) ~ (C, S).  q_1 is taken as (N + n_z, n_y, -n_x) for n_z >= 0 and as
that times N - n_z, (rho2, w n_y, -w n_x), for n_z < 0; q_theta as (H + C, S) for C >= 0 and (S, H - C)
for C < 0.  tests/test_wahba_two_arc_cpu.py holds the NumPy restatement used here to state the inputs.

256 filters x 64 records through pekf_run_dev: one block, both halves of the ping-pong loop.  Final X and
P against the C oracle on the same records to test_gpu_parity's PREC_GUARD, every lane.

Groups of 32 filters, their sensors remounted by a rotation per filter (applied to gyro, acc and mag in
FP64, then rounded to f32; the reference pair rotated in FP64).  It puts the first record's normal at a
chosen angle from -z or +z, tilted towards y so that arc 1's axis is x, and acc 15 degrees from +x or -x
in the measured plane (k_acc = |acc_z| >= 0.04, so B keeps rank 2).  The streams stay consistent, so
every lane is tracked, and over the first 4 records (the bodies then turn away)
  * normal 10 degrees from -z: 1 + n_z / N < 1/8, arc 1's second form with all lanes of a wave in it
    (theta takes any value there: next to a half turn arc 1's axis follows the normal's small tilt);
  * normal 10 degrees from +z, acc near +x: 1 + n_z / N > 15/8 and C > 0;
  * C < 0 with n_z >= 0 (normal 15 degrees from +z) and with n_z < 0 (60 degrees from -z): acc near -x,
    so theta is next to a half turn, q_theta's second form.
Select boundaries: records overwritten with acc = (+-0, 0, 1/2), mag = (1/2, 0, -sqrt(3)/2), for which
n_z = +0 and -0, and with acc = (+-1e-30, 0, 1/2), mag = (1/2, 1/4, -0.829), n_z = +-2.5e-31: both sides
of arc 1's select at points where both of its forms are valid.
64 filters start at random attitudes, so that lanes fall on both sides of |q'.z| = |q'| / 4 (the matrix
chain and its re-read of the record).
The constructed rank-1 record acc = (1/2, 0, 0), mag = (1/2, -1/2, 0): rho2 = 0 and n_z < 0, the one
input the two-arc form adds to the fallback's (q' = 0).  It sits in 8 filters at record 5; they are
compared with the oracle over the records before it, and after it by tests/test_degenerate_samples.py's
bounds for a rank-1 B: finite, |X| within 1e-12 of 1, back on the oracle within 1e-9 thirty records on.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import ekf_numpy as npo
from poseestimationkf_amd import synth

from .test_gpu_parity import PREC_GUARD
from .test_wahba_two_arc_cpu import arc1_terms, pair_in_own_frame, two_arc

pytestmark = pytest.mark.gpu

K, W = 256, 64
GAMMA = np.deg2rad(15.0)

GROUPS = {   # filters, side of z the normal is put on, its angle from that side, side of x acc is put on
    "arc 1 second form": (range(8, 40), -1.0, 10.0, 1.0),
    "arc 1 first form": (range(40, 72), 1.0, 10.0, 1.0),
    "C < 0, n_z >= 0": (range(72, 104), 1.0, 15.0, -1.0),
    "C < 0, n_z < 0": (range(104, 136), -1.0, 60.0, -1.0),
}
BOUNDARY = range(136, 168)      # records overwritten with the select's boundaries
FAR = range(168, 232)           # started at random attitudes: both sides of the |q'.z| threshold
RANK1 = range(232, 240)         # the constructed rank-1 record at RANK1_AT
RANK1_AT = 5
BOUNDARY_RECORDS = ((5, 0.0, 0.0), (6, -0.0, 0.0), (9, 1e-30, 0.25), (10, -1e-30, 0.25),
                    (33, -0.0, 0.0), (34, 0.0, 0.0), (40, -1e-30, 0.25), (41, 1e-30, 0.25), (63, -0.0, 0.0))


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _maxerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    return float(np.abs(a - b).max())


def _remount(a, m, side, phi, xside):
    """(k, 3, 3): per filter, the rotation taking the triad (a^, n^ x a^, n^) of the pair (a, m) to that of
    n^ = (0, sin phi, side cos phi) and a^ = xside cos GAMMA x + sin GAMMA (n^ x x)."""
    def triad(e, n):
        return np.stack([e, np.cross(n, e), n], axis=-1)
    e = a / np.linalg.norm(a, axis=-1, keepdims=True)
    n = np.cross(a, m)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    x = np.array([1.0, 0.0, 0.0])
    nt = np.array([0.0, np.sin(np.deg2rad(phi)), side * np.cos(np.deg2rad(phi))])
    et = xside * np.cos(GAMMA) * x + np.sin(GAMMA) * np.cross(nt, x)
    return triad(et, nt)[None] @ np.swapaxes(triad(e, n), -1, -2)


def two_arc_stream():
    """(records, X0, P0): the tracked stream with the filters of GROUPS, BOUNDARY, FAR and RANK1 changed."""
    rec = synth.generate(np.arange(K), W, seed=31)
    for cols, *where in GROUPS.values():
        cols = list(cols)
        M = _remount(rec.acc[0, cols].astype(np.float64), rec.mag[0, cols].astype(np.float64), *where)
        g, a, m = (np.einsum("kij,wkj->wki", M, arr[:, cols].astype(np.float64))
                   for arr in (rec.gyro, rec.acc, rec.mag))
        rec.gyro[:, cols], rec.acc[:, cols], rec.mag[:, cols] = (v.astype(np.float32) for v in (g, a, m))
        rec.acc0[cols] = np.einsum("kij,kj->ki", M, rec.acc0[cols])
        rec.mag0[cols] = np.einsum("kij,kj->ki", M, rec.mag0[cols])
    b = list(BOUNDARY)
    for t, ax, my in BOUNDARY_RECORDS:
        rec.acc[t, b] = np.array([ax, 0.0, 0.5], np.float32)
        rec.mag[t, b] = np.array([0.5, my, -0.8291562 if my else -0.8660254037844386], np.float32)
    rec.acc[RANK1_AT, list(RANK1)] = np.array([0.5, 0.0, 0.0], np.float32)
    rec.mag[RANK1_AT, list(RANK1)] = np.array([0.5, -0.5, 0.0], np.float32)
    X0 = np.tile(np.array([1.0, 0, 0, 0]), (K, 1))
    rng = np.random.default_rng(7)
    far = rng.normal(size=(len(FAR), 4))
    X0[list(FAR)] = far / np.linalg.norm(far, axis=1, keepdims=True)
    P0 = np.tile(np.eye(4), (K, 1, 1))
    return rec, X0, P0


def assert_inputs(rec, X0, P0):
    """The inputs are what the docstring says they are (NumPy only)."""
    a, m = rec.acc.astype(np.float64), rec.mag.astype(np.float64)
    n, N, rho2 = arc1_terms(a, m)
    aW, b1W, b2W, _ = pair_in_own_frame(rec.acc0, rec.mag0)
    _, C, _ = two_arc(a, m, aW, b1W, b2W, want_cs=True)
    num = 1.0 + n[..., 2] / N                   # 1 + cos of arc 1 in its first form
    c2, c1, cp, cn = (list(GROUPS[g][0]) for g in GROUPS)
    first = slice(0, 4)
    assert (num[first, c2] < 1 / 8).all()
    assert (num[first, c1] > 15 / 8).all() and (C[first, c1] > 0).all()
    assert (C[first, cp] < 0).all() and (n[first, cp, 2] >= 0).all()
    assert (C[first, cn] < 0).all() and (n[first, cn, 2] < 0).all()
    b = list(BOUNDARY)
    for t, ax, my in BOUNDARY_RECORDS:
        nz = n[t, b, 2]
        assert (np.signbit(nz) == np.signbit(ax)).all() and (np.abs(nz) == abs(float(np.float32(ax))) * my).all()
        assert (rho2[t, b] > 0.01).all()        # both forms of arc 1 are valid there
    assert {np.signbit(ax) for _, ax, my in BOUNDARY_RECORDS if my} == {True, False}
    r = list(RANK1)
    assert (rho2[RANK1_AT, r] == 0).all() and (n[RANK1_AT, r, 2] < 0).all()
    # lanes of FAR on both sides of the threshold at the first record
    far = 0
    for k in FAR:
        g, d, ak, mk = rec.filter(k)
        z, _, _ = npo.predict(g[0], d[0], X0[k], P0[k], np.identity(3), np.identity(4) * 0.1)
        y = npo.wahba_quat(rec.acc0[k], rec.mag0[k], ak[0], mk[0], abs(ak[0][2]), 1 - abs(ak[0][2]))
        far += abs(float(np.dot(y, z))) < 0.25
    assert 16 <= far <= 48


@pytest.fixture(scope="module")
def case(oracle_c):
    """(records, X0, P0, Xo, Po): the stream, checked, and the oracle's final state, checked alone first."""
    rec, X0, P0 = two_arc_stream()
    assert_inputs(rec, X0, P0)
    Xo, Po, _ = oracle_c.run(rec, X=X0, P=P0)
    assert np.isfinite(Xo).all() and np.isfinite(Po).all()
    assert np.abs(np.linalg.norm(Xo, axis=1) - 1.0).max() < 1e-12
    return rec, X0, P0, Xo, Po


def _launch(eng, win, X0, P0, chunks=((W, 0),), counts=None, **kw):
    f = eng.BatchedEKF(K, **kw)
    f.set_state(X0, P0)
    for n, step0 in chunks:
        f.run(win, n_steps=n, step0=step0, counts=None if counts is None else np.full(K, n, np.int32))
    return f.get_state()


def test_every_group_against_the_oracle(eng, case):
    rec, X0, P0, Xo, Po = case
    X, P = _launch(eng, eng.IMUWindow.from_records(rec), X0, P0)
    named = [(n, c[0]) for n, c in GROUPS.items()] + [("boundary", BOUNDARY), ("far", FAR)]
    for name, cols in named:
        cols = list(cols)
        print("two-arc form, %s: max |dX| = %.3e, max |dP| = %.3e"
              % (name, _maxerr(X[cols], Xo[cols]), _maxerr(P[cols], Po[cols])))
    rest = np.setdiff1d(np.arange(K), list(RANK1))      # (the rank-1 lanes: the test below)
    print("two-arc form, all of these and the tracked lanes: max |dX| = %.3e, max |dP| = %.3e"
          % (_maxerr(X[rest], Xo[rest]), _maxerr(P[rest], Po[rest])))
    assert _maxerr(X[rest], Xo[rest]) < PREC_GUARD and _maxerr(P[rest], Po[rest]) < PREC_GUARD
    assert np.abs(np.linalg.norm(X[rest], axis=1) - 1.0).max() < 1e-13


def test_constructed_rank_one_record(eng, case, oracle_c):
    rec, X0, P0, Xo, Po = case
    r = list(RANK1)
    win = eng.IMUWindow.from_records(rec)
    f = eng.BatchedEKF(K)
    f.set_state(X0, P0)
    f.run(win, n_steps=RANK1_AT)                        # the records before it
    Xb, Pb = f.get_state()
    Xob, Pob, _ = oracle_c.run(rec, n_steps=RANK1_AT, X=X0, P=P0)
    print("rank-1 lanes before the record: max |dX| = %.3e, max |dP| = %.3e"
          % (_maxerr(Xb[r], Xob[r]), _maxerr(Pb[r], Pob[r])))
    assert _maxerr(Xb[r], Xob[r]) < PREC_GUARD and _maxerr(Pb[r], Pob[r]) < PREC_GUARD
    f.run(win, n_steps=2, step0=RANK1_AT)               # the record itself and the next (the multi-record loop)
    X1, P1 = f.get_state()
    assert np.isfinite(X1[r]).all() and np.isfinite(P1[r]).all()
    assert np.abs(np.linalg.norm(X1[r], axis=1) - 1.0).max() < 1e-12
    X, P = _launch(eng, win, X0, P0)                    # one launch through it (the multi-record loop)
    assert np.isfinite(X[r]).all() and np.isfinite(P[r]).all()
    assert np.abs(np.linalg.norm(X[r], axis=1) - 1.0).max() < 1e-12
    print("rank-1 lanes %d records after it: max |dX| = %.3e" % (W - 1 - RANK1_AT, _maxerr(X[r], Xo[r])))
    assert W - 1 - RANK1_AT >= 30 and _maxerr(X[r], Xo[r]) < 1e-9


def test_launch_shapes_bit_identical(eng, case):
    rec, X0, P0, _, _ = case
    win = eng.IMUWindow.from_records(rec)
    halves = ((W // 2, 0), (W // 2, W // 2))
    X1, P1 = _launch(eng, win, X0, P0)
    Xa, Pa = _launch(eng, win, X0, P0, halves)
    Xs, Ps = _launch(eng, win, X0, P0, halves, layout="soa")
    Xc, Pc = _launch(eng, win, X0, P0, halves, counts=True)
    assert np.isfinite(X1).all() and np.isfinite(P1).all()
    assert _same(Xa, X1) and _same(Pa, P1)              # 2 x 32 records against one launch of 64
    assert _same(Xa, Xs) and _same(Pa, Ps)
    assert _same(Xa, Xc) and _same(Pa, Pc)


def test_schedules_bit_identical(eng, case, monkeypatch):
    rec, X0, P0, _, _ = case
    win = eng.IMUWindow.from_records(rec)
    monkeypatch.delenv("PEKF_RUN_PIN", raising=False)
    monkeypatch.delenv("PEKF_RUN_HOIST", raising=False)
    Xd, Pd = _launch(eng, win, X0, P0)                  # the library's own choice
    for pin, hoist in (("0", "0"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("PEKF_RUN_PIN", pin)
        monkeypatch.setenv("PEKF_RUN_HOIST", hoist)
        X, P = _launch(eng, win, X0, P0)
        assert _same(X, Xd) and _same(P, Pd), (pin, hoist)


def test_fp64_record_launch_bit_identical(eng, case):
    rec, X0, P0, _, _ = case
    w64 = eng.RecordWindow64.from_arrays(rec.gyro.astype(np.float64), rec.dt_ns, rec.acc.astype(np.float64),
                                         rec.mag.astype(np.float64), rec.acc0, rec.mag0)
    X1, P1 = _launch(eng, eng.IMUWindow.from_records(rec), X0, P0)
    X64, P64 = _launch(eng, w64, X0, P0)
    assert np.isfinite(X1).all() and _same(X64, X1) and _same(P64, P1)
