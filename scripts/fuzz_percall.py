#!/usr/bin/env python3
"""Randomised sweep of the batched per-call operators (pekf_predict / pekf_correct /
pekf_wahba_quaternion: the drop-ins' Prediction, Correction and getQuarternion) against the NumPy
restatement of the reference (oracle/ekf_numpy.py, bit-identical to ExtendedKalmanFilter.py /
Wahba.py), item by item, on the GPU box.

Each case draws 1-3,000 items with random gyro rates, dts of 0-2 s (fractional ns too), quaternions
of norm 0.5-2, covariances that are SPD or general (non-symmetric, as the reference accepts any
4x4), Q and R scalar or full SPD, raw-magnitude or unit acc / mag samples and reference pairs, and
Wahba weights of either sign.  An item passes within 1e-12 x max(1, |value|), or, where the item is
ill-conditioned in the reference's own arithmetic, within 10 x the disagreement between the two
restatements of the reference (the C oracle and the NumPy one differ only in rounding); a Wahba
quaternion also within 100 ulps of B's largest singular value over s2 + s3 (the SVD's own bound).

A quarter of the items are ill conditioned: P = Q1 diag(10^(-k [0, 1/3, 2/3, 1])) Q2^T with k uniform in 0-8 (Q2 = Q1,
symmetric, for half of them) and Q = q I, R = r I a thousandth of A P A^T's smallest singular value, so cond(S) is
about 10^k.  There the gain is judged as tests/test_percall_conditioning.py judges it: against the exact rational
P^- inv(S) of the device's own P^- (tests/percall_families.py), within 8 x the error of the reference's own
np.linalg.inv statement on that item (or eps cond(S), where LAPACK happened to do better than that).

An eighth of the items take their Wahba operands from the families of tests/wahba_families.py (pairs down to 1e-13
rad, weights down to 1e-12, vectors times 2^+-520, optima beside the identity and a half turn), and are judged as
tests/test_wahba_conditioning.py judges them: the quaternion against the exact one of tests/golden/wahba_families.npz,
sign-insensitively, within 8 x the worst error of the reference's own statement on the item's family.  Those of the
filter_weights family (whose weights are Correction's own |acc_z|, 1 - |acc_z|) are Correction's operands too, and X is
held to z + K (y - z) normalised with the exact y, within that bound carried through K and the norm.

usage: python3 scripts/fuzz_percall.py [--cases N] [--seed S]   (exit status 1 on any mismatch)
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ekf_numpy, oracle_c  # noqa: E402  (the checkers)
from tests import percall_families as families  # noqa: E402  (the exact rational gain)
from tests import wahba_families  # noqa: E402  (the Wahba families and their exact optima)
from poseestimationkf_amd import engine  # noqa: E402

TOL = 1e-12
SPREAD = 10.0
ILL = 0.25      # the fraction of ill-conditioned items
FAMILY = 0.125  # the fraction of items whose Wahba operands come from tests/wahba_families.py


def _unit(rng, shape):
    v = rng.normal(size=shape)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _spd(rng, n, k, scalar_p):
    A = rng.normal(scale=0.5, size=(n, k, k))
    M = A @ A.transpose(0, 2, 1) + 0.05 * np.eye(k)
    s = rng.uniform(0.01, 3.0, size=(n, 1, 1)) * np.eye(k)
    return np.where((rng.random(n) < scalar_p)[:, None, None], s, M)


def draw_case(rng):
    n = int(rng.integers(1, 3001))
    gyro = rng.normal(scale=float(rng.choice([0.1, 1.0, 3.0])), size=(n, 3))
    dt = rng.uniform(0, float(rng.choice([2e7, 2e9])), size=n)
    dt = np.where(rng.random(n) < 0.5, np.floor(dt), dt)
    X = _unit(rng, (n, 4)) * rng.uniform(0.5, 2.0, size=(n, 1))
    P = _spd(rng, n, 4, 0.0)
    P = np.where((rng.random(n) < 0.3)[:, None, None], P + rng.normal(scale=0.1, size=(n, 4, 4)), P)
    Q, R = _spd(rng, n, 3, 0.5), _spd(rng, n, 4, 0.5)
    ill = rng.random(n) < ILL
    if ill.any():
        m = int(ill.sum())
        k = rng.uniform(0.0, 8.0, size=m)
        lam = 10.0 ** (-k[:, None] * np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0]))
        q1, q2 = np.linalg.qr(rng.normal(size=(m, 4, 4)))[0], np.linalg.qr(rng.normal(size=(m, 4, 4)))[0]
        q2 = np.where((rng.random(m) < 0.5)[:, None, None], q1, q2)
        P[ill] = (q1 * lam[:, None, :]) @ q2.transpose(0, 2, 1)
        small = 1e-3 * 10.0 ** -k * np.sum(gyro[ill] ** 2, axis=1) / 4.0    # A P A^T = (|w|^2 / 4) (rotated P)
        Q[ill], R[ill] = small[:, None, None] * np.eye(3), small[:, None, None] * np.eye(4)
    raw = rng.random() < 0.5
    sa, sm = (9.8, 45.0) if raw else (1.0, 1.0)
    acc = (_unit(rng, (n, 3)) + rng.normal(scale=0.05, size=(n, 3))) * sa
    mag = (_unit(rng, (n, 3)) + rng.normal(scale=0.05, size=(n, 3))) * sm
    acc0, mag0 = _unit(rng, (n, 3)) * sa, _unit(rng, (n, 3)) * sm
    ka = rng.uniform(-1.0, 2.0, size=n)
    c = dict(n=n, gyro=gyro, dt=dt, X=X, P=P, Q=Q, R=R, acc=acc, mag=mag, acc0=acc0, mag0=mag0, ka=ka, km=1.0 - ka,
             raw=raw, ill=ill)
    # Wahba's own operands: the same samples, but for the items drawn from the families (fam: the item's row there)
    fcat, rows = wahba_families.side_by_side(wahba_families.families())
    fam = np.where(rng.random(n) < FAMILY, rng.integers(0, len(fcat["acc"]), n), -1)
    w = {k: np.array(c[k]) for k in ("acc0", "mag0", "acc", "mag")}
    hit = fam >= 0
    for k in w:
        w[k][hit] = fcat[k][fam[hit]]
    c["ka"][hit], c["km"][hit] = fcat["k_acc"][fam[hit]], fcat["k_mag"][fam[hit]]
    both = hit & (fam >= rows["filter_weights"].start) & (fam < rows["filter_weights"].stop)
    for k in w:
        c[k][both] = w[k][both]
    c.update(w_acc0=w["acc0"], w_mag0=w["mag0"], w_acc=w["acc"], w_mag=w["mag"], fam=fam, both=both)
    return c


def _family_problems(c, i, q, X, z, K):
    """A family item's q (and X, for filter_weights) by tests/test_wahba_conditioning.py's rule"""
    g, j = wahba_families.golden(), c["fam"][i]
    first = j - j % wahba_families.ITEMS
    Yq = wahba_families.yard(g, "f64", slice(first, first + wahba_families.ITEMS))[1]
    out = []
    e = wahba_families.err_quat(q, g["f64_q"][j])[0]
    if not e <= wahba_families.MARGIN * Yq:
        out.append("item %d q_wahba (family row %d): error %.3e against the exact one, bound %.3e" % (i, j, e, 8 * Yq))
    if c["both"][i]:
        y = g["f64_q"][j] * (-1.0 if np.dot(g["f64_q"][j], z) < 0.0 else 1.0)
        x = z + K @ (y - z)
        bound = 2.0 * np.abs(K).sum(axis=1).max() * wahba_families.MARGIN * Yq / np.linalg.norm(x) + TOL
        e = np.abs(X - x / np.linalg.norm(x)).max()
        if not e <= bound:
            out.append("item %d X (family row %d): error %.3e against the exact measurement, bound %.3e" % (i, j, e, bound))
    return out


def _gain_ok(Pm, K, Pn, Kn, R):
    """An ill-conditioned item's K against the exact gain of the device's own P^-: (passes, its error, the bound)."""
    S = Pm + R
    exact = families.gain_exact(Pm, S)
    if exact is None:
        return False, np.inf, 0.0
    e_lu = families.err(Kn, families.gain_exact(Pn, Pn + R))
    sv = np.linalg.svd(S, compute_uv=False)
    bound = max(families.MARGIN * e_lu, families.EPS * sv[0] / sv[-1])
    e = families.err(K, exact)
    return e <= bound, e, bound


def _ok(err, ref, spread):
    scale = np.maximum(1.0, np.abs(ref))
    return bool(np.all(err <= np.maximum(TOL * scale, SPREAD * spread)))


def check(c):
    """Problems (strings) of one case."""
    out = []
    z, Pm, K = engine.predict(c["gyro"], c["dt"], c["X"], c["P"], c["Q"], c["R"])
    Xc, Pc = engine.correct(c["mag"], c["acc"], z, Pm, K, c["acc0"], c["mag0"])
    qw = engine.wahba_quaternion(c["w_acc0"], c["w_mag0"], c["w_acc"], c["w_mag"], c["ka"], c["km"])
    for i in range(c["n"]):
        zn, Pn, Kn = ekf_numpy.predict(c["gyro"][i], c["dt"][i], c["X"][i], c["P"][i], c["Q"][i], c["R"][i])
        Xn, Pcn = ekf_numpy.correct(c["mag"][i], c["acc"][i], z[i], Pm[i], K[i], c["acc0"][i], c["mag0"][i])
        qn = ekf_numpy.wahba_quat(c["w_acc0"][i], c["w_mag0"][i], c["w_acc"][i], c["w_mag"][i], c["ka"][i], c["km"][i])
        if c["fam"][i] >= 0:
            out += _family_problems(c, i, qw[i], Xc[i], z[i], K[i])
        for name, g, e in (("z", z[i], zn), ("P-", Pm[i], Pn), ("K", K[i], Kn), ("X", Xc[i], Xn), ("P", Pc[i], Pcn),
                           ("q_wahba", qw[i], qn)):
            err = np.abs(g - e)
            if c["fam"][i] >= 0 and (name == "q_wahba" or (name == "X" and c["both"][i])):
                continue
            if name == "K" and c["ill"][i]:
                ok, e_k, bound = _gain_ok(Pm[i], K[i], Pn, Kn, c["R"][i])
                if not ok:
                    out.append("item %d K (ill conditioned): error %.3e against the exact gain, bound %.3e" % (i, e_k, bound))
                continue
            if np.all(err <= TOL * np.maximum(1.0, np.abs(e))):
                continue
            # the C restatement on the same inputs: how far the reference's own rounding moves this item
            if name in ("z", "P-", "K"):
                zc, Pcc, Kc = oracle_c.predict(c["gyro"][i], c["dt"][i], c["X"][i], c["P"][i], c["Q"][i], c["R"][i])
                alt = {"z": zc, "P-": Pcc, "K": Kc}[name]
            elif name in ("X", "P"):
                Xo, Po = oracle_c.correct(c["mag"][i], c["acc"][i], z[i], Pm[i], K[i], c["acc0"][i], c["mag0"][i])
                alt = {"X": Xo, "P": Po}[name]
            else:
                alt = oracle_c.wahba_quat(c["w_acc0"][i], c["w_mag0"][i], c["w_acc"][i], c["w_mag"][i], c["ka"][i], c["km"][i])
            spread = np.abs(alt - e)
            if name == "q_wahba":
                # the rotation of an SVD moves by ~ |dB| / (s2 + s3) for a perturbation dB of B
                # (LAPACK's error bound for the singular subspaces); the kernel's closed-form 3x3 SVD
                # and the reference's gesdd round differently, so allow that bound at a few ulps of B
                B = (c["ka"][i] * np.outer(c["w_acc0"][i], c["w_acc"][i]) + c["km"][i] * np.outer(c["w_mag0"][i], c["w_mag"][i]))
                sv = np.linalg.svd(B, compute_uv=False)
                spread = np.maximum(spread, 10 * np.finfo(float).eps * sv[0] / max(sv[1] + sv[2], 1e-300))
            if not _ok(err, e, spread):
                out.append("item %d %s: |d| %.3e (C / NumPy %.3e)" % (i, name, err.max(), np.abs(alt - e).max()))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args(argv)
    oracle_c.lib()
    rng = np.random.default_rng(a.seed)
    fails, items, t0 = 0, 0, time.time()
    for i in range(a.cases):
        c = draw_case(rng)
        items += c["n"]
        problems = check(c)
        if problems:
            fails += 1
            print("MISMATCH case %d (n=%d raw=%s): %s" % (i, c["n"], c["raw"], "; ".join(problems[:4])), flush=True)
        print("%d cases, %d items, %d mismatching cases, %.0f s" % (i + 1, items, fails, time.time() - t0), flush=True)
    print("done: %d cases, %d items, %d mismatching cases" % (a.cases, items, fails))
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
