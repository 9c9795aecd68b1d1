"""NumPy restatement of phase 1, the server's magnetometer calibration (KFS/Magnetometer_Calibration.cpp), in
the order of operations of k_magcal (csrc/pekf_magcal.hip) -- TEST INFRASTRUCTURE ONLY.

Per phone: the messages are counted as the server counts them (every phase-1 message is a sample, whatever its
type: KFS/Parser.cpp:30-34,144-147); the first n_cal samples are summed in arrival order and divided by n_cal
(setValues, :13-43 -- the bias, bit for bit the reference's computeBias); message n_cal + 1 fires the fit.  With
v = m - bias the normal equations of [x^2, y^2, z^2, 2xy, 2zx, 2yz] . {a..f} = 1 (:65-80) are summed in sample
order and solved by an unpivoted Cholesky factorisation; R = [[a, d, e], [d, b, f], [e, f, c]] (:165-175);
W = V sqrt(D) V^T (:178-200) by cyclic Jacobi over the pairs (0,1), (0,2), (1,2).

All functions are vectorised over phones (leading axis K); only the sample loop is sequential.
"""
from __future__ import annotations

import numpy as np

N_SWEEPS = 6
STATUS_OK, STATUS_FEW, STATUS_NO_QUADRIC, STATUS_NOT_ELLIPSOID = 0, 1, 2, 3


def message_samples(types, values, n_take):
    """The first n_take messages of each phone of an event dict's arrays (types (E, K), values (E, K, 3)):
    (samples (K, n_take, 3) float64 zero-padded, count (K,) messages in all).  Every type 0..3 is a message;
    synth.EV_NONE (4) is none."""
    types = np.asarray(types)
    values = np.asarray(values, np.float64)
    E, K = types.shape
    out = np.zeros((K, n_take, 3))
    cnt = np.zeros(K, np.int64)
    for k in range(K):
        v = values[types[:, k] <= 3, k]
        cnt[k] = len(v)
        out[k, :min(n_take, len(v))] = v[:n_take]
    return out, cnt


def bias_of(samples):
    """samples (K, n, 3): the sequential sum over n divided by n (setValues :20-22,32-34)."""
    s = np.zeros((samples.shape[0], 3))
    for i in range(samples.shape[1]):
        s = s + samples[:, i]
    return s / float(samples.shape[1])


def normal_equations(v):
    """v (K, n, 3) centred samples -> (A^T A (K, 6, 6), A^T 1 (K, 6)), summed in sample order."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    d = np.stack([x * x, y * y, z * z, 2.0 * x * y, 2.0 * z * x, 2.0 * y * z], axis=-1)  # (K, n, 6)
    ata, atb = np.zeros((v.shape[0], 6, 6)), np.zeros((v.shape[0], 6))
    for i in range(v.shape[1]):
        ata = ata + d[:, i, :, None] * d[:, i, None, :]
        atb = atb + d[:, i]
    return ata, atb


def cholesky_solve(ata, atb):
    """Unpivoted Cholesky solve per phone: (x (K, 6), ok (K,) every pivot > 0 and finite)."""
    K = ata.shape[0]
    L = np.zeros((K, 6, 6))
    ok = np.ones(K, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = ata[:, j, j].copy()
            for k in range(j):
                d = d - L[:, j, k] * L[:, j, k]
            ok &= (d > 0.0) & np.isfinite(d)
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                s = ata[:, j, i].copy()
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                L[:, i, j] = s * (1.0 / L[:, j, j])
        x = np.zeros((K, 6))
        for i in range(6):
            s = atb[:, i].copy()
            for k in range(i):
                s = s - L[:, i, k] * x[:, k]
            x[:, i] = s / L[:, i, i]
        for i in range(5, -1, -1):
            s = x[:, i].copy()
            for k in range(i + 1, 6):
                s = s - L[:, k, i] * x[:, k]
            x[:, i] = s / L[:, i, i]
    return x, ok


def r_of(fit):
    a, b, c, d, e, f = (fit[..., i] for i in range(6))
    return np.stack([np.stack([a, d, e], -1), np.stack([d, b, f], -1), np.stack([e, f, c], -1)], -2)


def jacobi_root(R, sweeps=N_SWEEPS):
    """R (K, 3, 3) symmetric -> (W (K, 3, 3) its principal square root with mirrored entries equal, ok (K,)
    every eigenvalue > 0 and finite).  Rotation t = sgn(tau) / (|tau| + sqrt(1 + tau^2)), tau = (aqq - app) /
    (2 apq); a zero apq is skipped; an infinite tau gives t = 0."""
    A = np.array(R, np.float64, copy=True)
    K = A.shape[0]
    V = np.tile(np.eye(3), (K, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = A[:, p, q]
                go = apq != 0.0
                tau = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = np.copysign(1.0, tau) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                t, c, s = np.where(go, t, 0.0), np.where(go, c, 1.0), np.where(go, s, 0.0)
                tapq = np.where(go, t * apq, 0.0)
                A[:, p, p] = A[:, p, p] - tapq
                A[:, q, q] = A[:, q, q] + tapq
                A[:, p, q] = A[:, q, p] = np.where(go, 0.0, apq)
                rp, rq = A[:, r, p].copy(), A[:, r, q].copy()
                A[:, r, p] = A[:, p, r] = np.where(go, c * rp - s * rq, rp)
                A[:, r, q] = A[:, q, r] = np.where(go, s * rp + c * rq, rq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(go[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(go[:, None], s[:, None] * vp + c[:, None] * vq, vq)
        lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], -1)
        ok = np.all((lam > 0.0) & np.isfinite(lam), axis=1)
        rt = np.sqrt(lam)
        W = np.empty((K, 3, 3))
        for i in range(3):
            for j in range(i, 3):
                W[:, i, j] = W[:, j, i] = (rt[:, 0] * V[:, i, 0] * V[:, j, 0] + rt[:, 1] * V[:, i, 1] * V[:, j, 1]) + \
                    rt[:, 2] * V[:, i, 2] * V[:, j, 2]
    return W, ok


def calibrate(types, values, n_cal=100):
    """An event dict's arrays -> dict(bias (K, 3), W (K, 3, 3), fit (K, 6), status (K,) int32), with the
    ABI's conventions for phones that are not calibrated (bias 0, W = I, fit NaN)."""
    samples, cnt = message_samples(types, values, n_cal)
    bias = bias_of(samples)
    ata, atb = normal_equations(samples - bias[:, None, :])
    fit, spd = cholesky_solve(ata, atb)
    W, ell = jacobi_root(r_of(fit))
    status = np.where(~ell, STATUS_NOT_ELLIPSOID, STATUS_OK)
    status = np.where(~spd, STATUS_NO_QUADRIC, status)
    status = np.where(cnt <= n_cal, STATUS_FEW, status).astype(np.int32)
    bad = status != 0
    bias[bad] = 0.0
    W[bad] = np.eye(3)
    fit[bad] = np.nan
    return dict(bias=bias, W=W, fit=fit, status=status)


def fit_error(fit, fit_exact):
    """Per phone max|fit - fit_exact| / max|fit_exact| (the fixture's e_ref is the reference's own)."""
    return np.abs(fit - fit_exact).max(axis=1) / np.abs(fit_exact).max(axis=1)


def root_residual(W, R):
    """Per phone max|W W - R| / max|R| (the fixture's w_ref is that of NumPy's eigh-based root)."""
    return np.abs(W @ W - R).reshape(len(R), -1).max(axis=1) / np.abs(R).reshape(len(R), -1).max(axis=1)


def eigh_root(R):
    """R (K, 3, 3) symmetric positive definite -> NumPy's eigh-based principal root (V sqrt(lam)) V^T, the
    yardstick of the fixture's w_ref."""
    lam, V = np.linalg.eigh(R)
    return (V * np.sqrt(lam)[:, None, :]) @ V.transpose(0, 2, 1)


def scaled_root_residual(W, R):
    """Per phone max_ij |V^T (W W - R) V|_ij / sqrt(lam_i lam_j) in R's own eigenbasis (NumPy's eigh): the
    residual of each eigen-direction relative to that direction's eigenvalue, so an error along the small
    eigenvalue is not hidden behind max|R| when kappa(R) is in the hundreds."""
    lam, V = np.linalg.eigh(R)
    E = V.transpose(0, 2, 1) @ (W @ W - R) @ V
    return (np.abs(E) / np.sqrt(lam[:, :, None] * lam[:, None, :])).reshape(len(R), -1).max(axis=1)


def exact_solve(v):
    """The normal equations (A^T A) x = A^T 1 of the design rows [x^2, y^2, z^2, 2xy, 2zx, 2yz] of the float64
    samples v (n, 3), formed and solved in rationals (fractions.Fraction, Gauss-Jordan): (x, pivots, exchanged)
    -- the six unknowns and the six pivots as Fractions, and whether a row exchange was needed.  Without an
    exchange pivot c is the ratio of the leading minors c + 1 and c, so A^T A is positive definite exactly when
    exchanged is False and every pivot is > 0.  A singular system raises StopIteration."""
    from fractions import Fraction
    rows = []
    for x, y, z in v:
        x, y, z = Fraction(float(x)), Fraction(float(y)), Fraction(float(z))
        rows.append([x * x, y * y, z * z, 2 * x * y, 2 * z * x, 2 * y * z])
    M = [[sum(r[i] * r[j] for r in rows) for j in range(6)] + [sum(r[i] for r in rows)] for i in range(6)]
    pivots, exchanged = [], False
    for c in range(6):  # Gauss-Jordan in rationals
        p = next(r for r in range(c, 6) if M[r][c] != 0)
        exchanged = exchanged or p != c
        M[c], M[p] = M[p], M[c]
        pivots.append(M[c][c])
        M[c] = [e / M[c][c] for e in M[c]]
        for r in range(6):
            if r != c and M[r][c] != 0:
                M[r] = [a - M[r][c] * b for a, b in zip(M[r], M[c])]
    return [M[i][6] for i in range(6)], pivots, exchanged


def exact_fit(v):
    """The exact solution of (A^T A) x = A^T 1 for the design rows of the float64 samples v (n, 3), rounded to
    float64 at the end (tests/golden/magcal.npz's fit_exact)."""
    return np.array([float(e) for e in exact_solve(v)[0]])


def apply(values, types, bias, W, status=None):
    """W (m - bias) for the type-2 events of the calibrated phones: values (E, K, 3) float64 -> a corrected copy."""
    out = np.array(values, np.float64, copy=True)
    sel = np.asarray(types) == 2
    if status is not None:
        sel = sel & (np.asarray(status) == 0)[None, :]
    cor = np.einsum("kij,ekj->eki", W, out - bias[None])
    out[sel] = cor[sel]
    return out
