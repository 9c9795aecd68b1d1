"""Exact results for the items of tests/step_families.py, and the error of the reference's own float64 statements
against them (needs mpmath; no GPU, no reference checkout):

    python tests/golden/make_step_golden.py

Propagation.  The reference's RungeKutta4 (ExtendedKalmanFilter.py:25-41: the four stages with h = T * 1e-09, the
double, and q1 / |q1|) on the item's doubles at DPS = 80 digits, record after record with nothing rounded in between;
the last X is rounded once.  For the sets "f64" and "f32" (step_families.PROP, 288 items each) and the items judged
apart:
  p_<set>_X        (288, 4)  the exact last X
  p_<set>_X_ref    (288, 4)  oracle.ekf_numpy.rk4 chained in float64 over the same records, and
  p_<set>_err      (288,)    max |X_ref - X|, taken at 80 digits (the families' yardstick Y, step_families.prop_yard)
  p_apart_X        (7, 4)    of step_families.prop_apart(): exact where it is finite (the first three), else NaN
Measurement.  The exact optimum of B = k_acc acc0 acc^T + k_mag mag0 mag^T, k_acc = |acc_z| and k_mag = 1 - k_acc as
float64 gives them, by make_wahba_golden's solver: mpmath's SVD, which must agree with the closed form to 1e-40 or the
script stops.  z is the exact RK4 step of the item's X0 by the gain-one record (gyro (2, 0, 0), 1000 ns).  For "f64"
(step_families.MEAS, 320 items) and "f32" (MEAS32, 288 items):
  m_<set>_q        (n, 4)    the reference's branch formula (Wahba.py:19-47) applied to the exact R at 80 digits
  m_<set>_sign     (n,)      int8, the exact sign of q . z
  m_<set>_qz       (n,)      |q . z|
  m_<set>_q_ref    (n, 4)    oracle.ekf_numpy.wahba_quat, and
  m_<set>_err_q    (n,)      min(max |q_ref - q|, max |q_ref + q|) at 80 digits (Y_q, step_families.meas_yard)

Output: tests/golden/step_families.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("PEKF_GOLDEN_OUT") or HERE
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import mpmath as mp  # noqa: E402

import make_wahba_golden as mw  # noqa: E402
from oracle import ekf_numpy as npo  # noqa: E402
from tests import step_families as sf  # noqa: E402
from tests import wahba_families as wf  # noqa: E402

DPS = 80


def _half_omega(w, q):
    a, b, c = w
    return [(-a * q[1] - b * q[2] - c * q[3]) / 2, (a * q[0] + c * q[2] - b * q[3]) / 2,
            (b * q[0] - c * q[1] + a * q[3]) / 2, (c * q[0] + b * q[1] - a * q[2]) / 2]


def exact_chain(X0, gyro, dt, n):
    """the last X of n records, as mpf"""
    x = [mp.mpf(float(v)) for v in X0]
    ns = mp.mpf(float(sf.NS))
    for l in range(n):
        w = [mp.mpf(float(v)) for v in gyro[l]]
        h = mp.mpf(float(dt[l])) * ns
        k1 = _half_omega(w, x)
        k2 = _half_omega(w, [a + h / 2 * b for a, b in zip(x, k1)])
        k3 = _half_omega(w, [a + h / 2 * b for a, b in zip(x, k2)])
        k4 = _half_omega(w, [a + h * b for a, b in zip(x, k3)])
        q1 = [a + h / 6 * (b + 2 * c + 2 * d + e) for a, b, c, d, e in zip(x, k1, k2, k3, k4)]
        nq = mp.sqrt(sum(v * v for v in q1))
        x = [v / nq for v in q1]
    return x


def reference_chain(X0, gyro, dt, n):
    x = np.asarray(X0, dtype=np.float64)
    for l in range(n):
        x = npo.rk4(x, dt[l], gyro[l])
    return x


def solve_prop(cat):
    n = len(cat["n"])
    X, Xr, err = np.empty((n, 4)), np.empty((n, 4)), np.empty(n)
    for i in range(n):
        ex = exact_chain(cat["X0"][i], cat["gyro"][i], cat["dt"][i], int(cat["n"][i]))
        X[i] = [float(v) for v in ex]
        Xr[i] = reference_chain(cat["X0"][i], cat["gyro"][i], cat["dt"][i], int(cat["n"][i]))
        err[i] = float(max(abs(mp.mpf(float(a)) - b) for a, b in zip(Xr[i], ex)))
    return dict(X=X, X_ref=Xr, err=err)


def solve_meas(cat):
    n = len(cat["acc"])
    out = dict(q=np.empty((n, 4)), sign=np.empty(n, np.int8), qz=np.empty(n), q_ref=np.empty((n, 4)), err_q=np.empty(n))
    for i in range(n):
        it = [cat[k][i] for k in wf.FIELDS]
        R, _ = mw.svd_optimum(mw.exact_b(*it))
        R2 = mw.closed_form_optimum(*it)
        worst = max(abs(R[a, b] - R2[a, b]) for a in range(3) for b in range(3))
        if not worst < mw.AGREE:
            raise SystemExit("item %d: the SVD and the closed form differ by %s" % (i, mp.nstr(worst, 5)))
        q = mw.branch_quat(R)[0]
        z = exact_chain(cat["X0"][i], [sf.GAIN_GYRO], [sf.GAIN_DT], 1)
        qz = sum(a * b for a, b in zip(q, z))
        out["q"][i] = [float(v) for v in q]
        out["sign"][i], out["qz"][i] = (1 if qz >= 0 else -1), float(abs(qz))
        out["q_ref"][i] = npo.wahba_quat(*it)
        out["err_q"][i] = float(mw._err_q(out["q_ref"][i], q))
    return out


def main():
    mp.mp.dps = DPS
    store = {}
    for form in ("f64", "f32"):
        cat, _ = sf.prop_side_by_side(sf.prop_families(form))
        for k, v in solve_prop(cat).items():
            store["p_%s_%s" % (form, k)] = v
        cat, _ = sf.meas_side_by_side(sf.meas_families(form))
        for k, v in solve_meas(cat).items():
            store["m_%s_%s" % (form, k)] = v
    ap = sf.prop_apart()
    store["p_apart_X"] = np.full((len(sf.PROP_APART), 4), np.nan)
    for i in range(sf.PROP_APART_FINITE):
        store["p_apart_X"][i] = [float(v) for v in exact_chain(ap["X0"][i], ap["gyro"][i], ap["dt"][i], 1)]
    path = os.path.join(OUT, "step_families.npz")
    np.savez_compressed(path, **store)
    print("step_families.npz %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
