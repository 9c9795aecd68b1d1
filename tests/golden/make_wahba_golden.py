"""Exact Wahba optima for the families of tests/wahba_families.py, and the error of the reference's own float64
statements against them (needs mpmath; no GPU, no reference checkout):

    python tests/golden/make_wahba_golden.py

For each item, B = k_acc acc0 acc^T + k_mag mag0 mag^T is formed exactly from the doubles (rationals), its SVD taken
by mpmath.svd_r at DPS = 80 digits, and R = U diag(1, 1, det U det V) V^T (Wahba.py:14-17).  The same optimum from the
closed form in the same arithmetic (Gram-Schmidt frames and the 2 x 2 polar factor, exact but for 1e-80 roundings)
must agree to 1e-40, or the script stops: the SVD of a rank-2 matrix is not taken on trust.

Stored, for the set "f64" (the nine families, 288 items) and the set "f32" (wahba_families.F32 with every vector
rounded to float32, 192 items), arrays over the items side by side -- the inputs come from the generator and are not
stored:
  <set>_rank1     (n,) bool  a pair of the item is exactly parallel (float32 rounding makes a pair thinner than ~1e-7 so
                             as often as not): B has rank 1, no rotation is the optimum, every other entry is NaN
  <set>_R         (n, 3, 3)  the exact optimum, each entry rounded once
  <set>_q         (n, 4)     the reference's branch formula (Wahba.py:19-47) applied to the exact R at 80 digits
  <set>_t_own     (n,)       the chosen branch's numerator 1 +- R00 +- R11 +- R22 (= 4 x the square of its own entry of q)
  <set>_margin    (n,)       that numerator less the larger of the other two: the exact branch margin
  <set>_w_num     (n,)       |the numerator of q's w entry| in that branch
  <set>_theta     (n, 2)     the exact angles theta_W, theta_V of the two pairs
  <set>_cond      (n,)       sigma_1 / sigma_2 of B
  <set>_R_ref     (n, 3, 3)  oracle.ekf_numpy.svd_rotation in float64 (np.linalg.svd), and
  <set>_q_ref     (n, 4)     oracle.ekf_numpy.wahba_quat: the reference's statements as this NumPy gives them
  <set>_err_R     (n,)       max |R_ref - R| and
  <set>_err_q     (n,)       min(max |q_ref - q|, max |q_ref + q|), both taken at 80 digits
For the pure R -> q operator, per family of wahba_families.matrices() (the float64 matrix as given is the operand):
  mat_<name>_q    (32, 4)    the branch formula at 80 digits
  mat_<name>_err  (32,)      oracle.ekf_numpy.rotm_to_quat's error against it (sign-insensitive, as above)

Output: tests/golden/wahba_families.npz
"""
from __future__ import annotations

import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("PEKF_GOLDEN_OUT") or HERE
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

import mpmath as mp  # noqa: E402

from oracle import ekf_numpy as npo  # noqa: E402
from tests import wahba_families as wf  # noqa: E402

DPS = 80
AGREE = mp.mpf(10) ** -40


def _mpf(x):
    fr = Fraction(x)
    return mp.mpf(fr.numerator) / mp.mpf(fr.denominator)


def exact_b(acc0, mag0, acc, mag, ka, km):
    fr = lambda v: [Fraction(float(x)) for x in v]
    a0, m0, a, m, ka, km = fr(acc0), fr(mag0), fr(acc), fr(mag), Fraction(float(ka)), Fraction(float(km))
    return mp.matrix([[_mpf(ka * a0[i] * a[j] + km * m0[i] * m[j]) for j in range(3)] for i in range(3)])


def svd_optimum(B):
    """R = U diag(1, 1, det U det V) V^T and the singular values"""
    U, S, V = mp.svd_r(B)
    d = mp.det(U) * mp.det(V)
    return U * mp.diag([1, 1, d]) * V, S


def _frame(a, m, sg):
    na = mp.sqrt(sum(x * x for x in a))
    e1 = [x / na for x in a]
    b1 = sum(x * y for x, y in zip(e1, m))
    t = [y - b1 * x for x, y in zip(e1, m)]
    nt = mp.sqrt(sum(x * x for x in t))
    e2 = [sg * x / nt for x in t]
    u3 = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    return e1, e2, u3, na, b1, sg * nt


def closed_form_optimum(acc0, mag0, acc, mag, ka, km):
    """pekf_math.hpp's algebra (wahba_rotation) at DPS digits"""
    v = lambda x: [mp.mpf(float(y)) for y in x]
    ka, km = mp.mpf(float(ka)), mp.mpf(float(km))
    sg = 1 if ka * km >= 0 else -1
    w1, w2, w3, aw, b1w, b2w = _frame(v(acc0), v(mag0), 1)
    v1, v2, v3, av, b1v, b2v = _frame(v(acc), v(mag), sg)
    p = ka * aw * av + km * b1w * b1v + km * b2w * b2v
    s = km * b2w * b1v - km * b1w * b2v
    h = mp.sqrt(p * p + s * s)
    p, s = p / h, s / h
    R = mp.matrix(3, 3)
    for i in range(3):
        g0, g1 = w1[i] * p + w2[i] * s, w2[i] * p - w1[i] * s
        for j in range(3):
            R[i, j] = g0 * v1[j] + g1 * v2[j] + w3[i] * v3[j]
    return R


def branch_quat(M):
    """RotationMatrix2Quart (Wahba.py:19-47) at DPS digits: q, the chosen numerator, its margin, |w's numerator|"""
    t1 = 1 + M[0, 0] - M[1, 1] - M[2, 2]
    t2 = 1 - M[0, 0] + M[1, 1] - M[2, 2]
    t3 = 1 - M[0, 0] - M[1, 1] + M[2, 2]
    if t1 > t2 and t1 > t3:
        s = mp.sqrt(t1) * 2
        q, own, rest, wn = [(M[2, 1] - M[1, 2]) / s, s / 4, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s], t1, max(t2, t3), M[2, 1] - M[1, 2]
    elif t2 > t1 and t2 > t3:
        s = mp.sqrt(t2) * 2
        q, own, rest, wn = [(M[0, 2] - M[2, 0]) / s, (M[0, 1] + M[1, 0]) / s, s / 4, (M[1, 2] + M[2, 1]) / s], t2, max(t1, t3), M[0, 2] - M[2, 0]
    else:
        s = mp.sqrt(t3) * 2
        q, own, rest, wn = [(M[1, 0] - M[0, 1]) / s, (M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, s / 4], t3, max(t1, t2), M[1, 0] - M[0, 1]
    return q, own, own - rest, abs(wn)


def _angle(a, m):
    a, m = [mp.mpf(float(x)) for x in a], [mp.mpf(float(x)) for x in m]
    c = [a[1] * m[2] - a[2] * m[1], a[2] * m[0] - a[0] * m[2], a[0] * m[1] - a[1] * m[0]]
    return mp.atan2(mp.sqrt(sum(x * x for x in c)), sum(x * y for x, y in zip(a, m)))


def _err_q(q, q_exact):
    return min(max(abs(mp.mpf(float(x)) - y) for x, y in zip(q, q_exact)),
               max(abs(mp.mpf(float(x)) + y) for x, y in zip(q, q_exact)))


def solve_set(cat):
    n = len(cat["acc"])
    out = dict(R=np.empty((n, 3, 3)), q=np.empty((n, 4)), t_own=np.empty(n), margin=np.empty(n), w_num=np.empty(n),
               theta=np.empty((n, 2)), cond=np.empty(n), R_ref=np.empty((n, 3, 3)), q_ref=np.empty((n, 4)),
               err_R=np.empty(n), err_q=np.empty(n))
    for v in out.values():
        v.fill(np.nan)
    out["rank1"] = wf.exactly_parallel(cat)
    for i in np.nonzero(~out["rank1"])[0]:
        it = [cat[k][i] for k in wf.FIELDS]
        R, S = svd_optimum(exact_b(*it))
        R2 = closed_form_optimum(*it)
        worst = max(abs(R[a, b] - R2[a, b]) for a in range(3) for b in range(3))
        if not worst < AGREE:
            raise SystemExit("item %d: the SVD and the closed form differ by %s" % (i, mp.nstr(worst, 5)))
        q, own, margin, wn = branch_quat(R)
        out["R"][i] = [[float(R[a, b]) for b in range(3)] for a in range(3)]
        out["q"][i] = [float(x) for x in q]
        out["t_own"][i], out["margin"][i], out["w_num"][i] = float(own), float(margin), float(wn)
        out["theta"][i] = float(_angle(it[0], it[1])), float(_angle(it[2], it[3]))
        out["cond"][i] = float(S[0] / S[1])
        out["R_ref"][i] = npo.svd_rotation(*it)
        out["q_ref"][i] = npo.wahba_quat(*it)
        out["err_R"][i] = float(max(abs(mp.mpf(float(out["R_ref"][i][a, b])) - R[a, b]) for a in range(3) for b in range(3)))
        out["err_q"][i] = float(_err_q(out["q_ref"][i], q))
    return out


def main():
    mp.mp.dps = DPS
    store = {}
    for name, fam in (("f64", wf.families()), ("f32", wf.families32())):
        cat, _ = wf.side_by_side(fam)
        for k, v in solve_set(cat).items():
            store["%s_%s" % (name, k)] = v
    for name, M in wf.matrices().items():
        q, err = np.empty((len(M), 4)), np.empty(len(M))
        for i in range(len(M)):
            exact = branch_quat(mp.matrix([[mp.mpf(float(x)) for x in row] for row in M[i]]))[0]
            q[i] = [float(x) for x in exact]
            err[i] = float(_err_q(npo.rotm_to_quat(M[i]), exact))
        store["mat_%s_q" % name], store["mat_%s_err" % name] = q, err
    path = os.path.join(OUT, "wahba_families.npz")
    np.savez_compressed(path, **store)
    print("wahba_families.npz %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
