"""The reference's filter with the covariance side held in a chosen dtype -- TEST INFRASTRUCTURE ONLY.

``run_filter_pt`` is ``oracle.ekf_numpy.run_filter``'s loop, operation for operation, with every
covariance-side operand -- omega_half(gyro), xi_half(X), Q, R, P, P-, S, inv(S), K and P - K P -- in
dtype ``pt``; RK4, Wahba, the hemisphere test, X = z + K (y - z) (K cast up) and the normalisation stay
float64.  With ``pt = np.float64`` it is ``run_filter`` bit for bit; with ``np.float32`` it is "the
reference's own arithmetic with the covariance in f32", the yardstick the mixed-precision kernels
(PEKF_RUN_MIXED_PRECISION) are measured against: it shares no code and no algebra with them.

``run_filter_rminus`` is the same loop with the step in the plain r-minus form, Si = inv(P- + rI),
K = I - r Si, P = rI - r^2 Si: the algebra whose f32 error grows like r / q.  The CPU tests use it to
show that the acceptance rule tells the two apart.

``errors`` / ``accept`` are that rule (tests/test_mixed_precision.py, scripts/fuzz_gpu.py).
"""
from __future__ import annotations

import numpy as np

from oracle import ekf_numpy as npo

FACTOR = 4.0  # a mixed launch may err up to 4x as far from the FP64 oracle as the yardstick does


def omega_half(w, pt):
    """ekf_numpy.omega_half with the entries and the halving in pt."""
    a, b, c = w[0], w[1], w[2]
    rows = [[0.0, -a, -b, -c],
            [a, 0.0, c, -b],
            [b, -c, 0.0, a],
            [c, b, -a, 0.0]]
    return pt(0.5) * np.asarray(rows, dtype=pt)


def xi_half(q, pt):
    """ekf_numpy.xi_half with the entries and the halving in pt."""
    rows = [[-q[1], -q[2], -q[3]],
            [q[0], q[3], -q[2]],
            [-q[3], q[0], q[1]],
            [q[2], -q[1], q[0]]]
    return pt(0.5) * np.asarray(rows, dtype=pt)


def _setup(q, r, pt, X0, P0):
    Q = np.identity(3, dtype=pt)
    Q *= pt(q)
    R = np.identity(4, dtype=pt)
    R *= pt(r)
    X = np.asarray([1., 0., 0., 0.]) if X0 is None else np.asarray(X0, dtype=np.float64)
    P = np.identity(4, dtype=pt) if P0 is None else np.asarray(P0).astype(pt)
    return Q, R, X, P


def _measure(acc, mag, z, acc0, mag0):
    """Correction's float64 half up to the hemisphere test (ekf_numpy.correct): y"""
    y = npo.wahba_quat(acc0, mag0, acc, mag, abs(acc[2]), 1 - (abs(acc[2])))
    if npo.hemisphere_test(y, z)[0] < 0.0:
        y = -y
    return y


def _run(gyro, dt_ns, acc, mag, acc0, mag0, q, r, pt, X0, P0, missing, gain):
    pt = np.dtype(pt).type
    Q, R, X, P = _setup(q, r, pt, X0, P0)
    n = len(dt_ns)
    traj, Ps = np.empty((n, 4)), np.empty((n, 4, 4))
    for i in range(n):
        A = omega_half(gyro[i], pt)
        Jb = xi_half(X, pt)
        Pm = np.matmul(np.matmul(A, P), A.transpose()) + np.matmul(np.matmul(Jb, Q), Jb.transpose())
        z = npo.rk4(X, dt_ns[i], gyro[i])
        K, Pc = gain(Pm, R, pt)
        assert Pm.dtype == pt and K.dtype == pt and Pc.dtype == pt, (Pm.dtype, K.dtype, Pc.dtype)  # NumPy promotes silently
        if missing is not None and missing[i]:
            X, P = z, Pm
        else:
            y = _measure(acc[i], mag[i], z, acc0, mag0)
            X = z + np.matmul(K.astype(np.float64), y - z)
            X, P = X / npo.loop_norm(X), Pc
        assert X.dtype == np.float64 and P.dtype == pt
        traj[i], Ps[i] = X, P
    return traj, Ps


def _gain_reference(Pm, R, pt):
    """K = P- S^-1, P = P- - K P- (ekf_numpy.predict / correct)"""
    S = Pm + R
    K = np.matmul(Pm, np.linalg.inv(S))
    return K, Pm - np.matmul(K, Pm)


def _gain_rminus(Pm, R, pt):
    """Si = (P- + rI)^-1, K = I - r Si, P = rI - r^2 Si"""
    r = R[0, 0]
    Si = np.linalg.inv(Pm + R)
    I = np.identity(4, dtype=pt)
    return I - r * Si, r * I - (r * r) * Si


def run_filter_pt(gyro, dt_ns, acc, mag, acc0, mag0, q, r, pt, X0=None, P0=None, missing=None):
    """One filter over a record sequence as ekf_numpy.run_filter, the covariance side in dtype pt.
    Returns (traj (N, 4) float64, P (N, 4, 4): every record's posterior covariance, cast up to float64)."""
    return _run(gyro, dt_ns, acc, mag, acc0, mag0, q, r, pt, X0, P0, missing, _gain_reference)


def run_filter_rminus(gyro, dt_ns, acc, mag, acc0, mag0, q, r, pt, X0=None, P0=None, missing=None):
    """run_filter_pt with the gain and the posterior in the r-minus form (module docstring)."""
    return _run(gyro, dt_ns, acc, mag, acc0, mag0, q, r, pt, X0, P0, missing, _gain_rminus)


def run_records_pt(rec, q, r, pt, X0=None, P0=None, run=run_filter_pt):
    """Every filter of a synth.Records window through `run`: (traj (K, W, 4), P (K, W, 4, 4))."""
    W, K = rec.dtw.shape
    traj, Ps = np.empty((K, W, 4)), np.empty((K, W, 4, 4))
    miss = rec.missing
    for k in range(K):
        g, d, a, m = rec.filter(k)
        traj[k], Ps[k] = run(g, d, a, m, rec.acc0[k], rec.mag0[k], q, r, pt,
                             None if X0 is None else X0[k], None if P0 is None else P0[k], miss[:, k])
    return traj, Ps


def errors(X, P, Xo, Po):
    """(eX, eP) of the acceptance rule: eX the largest |X - X_oracle| over everything given (filters, and
    records where X is a trajectory), eP the largest over filters of max|P - P_oracle| / max|P_oracle|
    (P, Po: (K, 4, 4) final covariances)."""
    X, P, Xo, Po = (np.asarray(a, np.float64) for a in (X, P, Xo, Po))
    assert X.shape == Xo.shape and P.shape == Po.shape and P.shape[-2:] == (4, 4), (X.shape, Xo.shape, P.shape, Po.shape)
    assert np.isfinite(X).all() and np.isfinite(P).all()
    eX = float(np.abs(X - Xo).max())
    eP = float((np.abs(P - Po).max(axis=(-2, -1)) / np.abs(Po).max(axis=(-2, -1))).max())
    return eX, eP


def accept(e_got, e_ref):
    """The rule: every error of the launch within FACTOR x the yardstick's own, X and P alike."""
    return all(g <= FACTOR * r for g, r in zip(e_got, e_ref))


def conditioning(Po):
    """min over filters of lambda_min / max|P| of the oracle's covariances (K, 4, 4)"""
    Po = np.asarray(Po, np.float64)
    return float((np.linalg.eigvalsh(Po).min(axis=-1) / np.abs(Po).max(axis=(-2, -1))).min())
