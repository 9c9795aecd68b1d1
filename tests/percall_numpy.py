"""NumPy restatements of the per-call gain's two algebras (csrc/pekf_math.hpp inverse4 and its caller
d_predict_gain, csrc/pekf_percall.hip), operation for operation in float64 scalars.  NumPy does not contract a * b + c
to an fma as the device's compiler does, so the figures differ from the device's in the last bits, not in kind.

    inverse4_cofactor   the former inverse4: unpivoted 2x2 cofactors over an unscaled determinant
    inverse4_pivoted    the present one: LU with partial pivoting (one reciprocal per pivot, as LAPACK's getf2
                        scales by it), inv(L) P formed beside it, then four back substitutions.  Its forward error
                        is that of a Gauss-Jordan sweep, but its residual S X - I is the small one, and K = P^- X =
                        (S - R) X feels the residual: Gauss-Jordan (tried here first) reached 16 to 70 x e_lu on
                        spd_10 and general_8 where this form stays below 1.5 x
    gain(Pm, R, inv4)   S = Pm + R, K = Pm inv(S) with matmul<4, 4, 4>'s sums; None where inv4 reports a singular S
"""
import numpy as np


def inverse4_cofactor(S):
    m = [np.float64(x) for x in np.asarray(S, dtype=np.float64).reshape(16)]
    with np.errstate(all="ignore"):
        s0 = m[0] * m[5] - m[4] * m[1]
        s1 = m[0] * m[6] - m[4] * m[2]
        s2 = m[0] * m[7] - m[4] * m[3]
        s3 = m[1] * m[6] - m[5] * m[2]
        s4 = m[1] * m[7] - m[5] * m[3]
        s5 = m[2] * m[7] - m[6] * m[3]
        c5 = m[10] * m[15] - m[14] * m[11]
        c4 = m[9] * m[15] - m[13] * m[11]
        c3 = m[9] * m[14] - m[13] * m[10]
        c2 = m[8] * m[15] - m[12] * m[11]
        c1 = m[8] * m[14] - m[12] * m[10]
        c0 = m[8] * m[13] - m[12] * m[9]
        det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0
        if det == 0.0:
            return None
        d = np.float64(1.0) / det
        inv = [(m[5] * c5 - m[6] * c4 + m[7] * c3) * d, (-m[1] * c5 + m[2] * c4 - m[3] * c3) * d,
               (m[13] * s5 - m[14] * s4 + m[15] * s3) * d, (-m[9] * s5 + m[10] * s4 - m[11] * s3) * d,
               (-m[4] * c5 + m[6] * c2 - m[7] * c1) * d, (m[0] * c5 - m[2] * c2 + m[3] * c1) * d,
               (-m[12] * s5 + m[14] * s2 - m[15] * s1) * d, (m[8] * s5 - m[10] * s2 + m[11] * s1) * d,
               (m[4] * c4 - m[5] * c2 + m[7] * c0) * d, (-m[0] * c4 + m[1] * c2 - m[3] * c0) * d,
               (m[12] * s4 - m[13] * s2 + m[15] * s0) * d, (-m[8] * s4 + m[9] * s2 - m[11] * s0) * d,
               (-m[4] * c3 + m[5] * c1 - m[6] * c0) * d, (m[0] * c3 - m[1] * c1 + m[2] * c0) * d,
               (-m[12] * s3 + m[13] * s1 - m[14] * s0) * d, (m[8] * s3 - m[9] * s1 + m[10] * s0) * d]
    return np.array(inv).reshape(4, 4)


def inverse4_pivoted(S):
    a = [[np.float64(x) for x in row] for row in np.asarray(S, dtype=np.float64).reshape(4, 4)]
    b = [[np.float64(i == j) for j in range(4)] for i in range(4)]
    x, rp, ok = [None] * 4, [None] * 4, True
    with np.errstate(all="ignore"):
        for c in range(4):
            for r in range(c + 1, 4):          # the largest |a[r][c]|, r >= c, comes to row c
                if abs(a[r][c]) > abs(a[c][c]):
                    a[c], a[r] = a[r], a[c]
                    b[c], b[r] = b[r], b[c]
            ok = ok and a[c][c] != 0.0
            rp[c] = np.float64(1.0) / a[c][c]
            for r in range(c + 1, 4):          # a -> U, b -> inv(L) P
                l = a[r][c] * rp[c]
                a[r] = [u - l * v for u, v in zip(a[r], a[c])]
                b[r] = [u - l * v for u, v in zip(b[r], b[c])]
        for r in (3, 2, 1, 0):                 # U X = inv(L) P, from the last row up
            row = b[r]
            for t in range(r + 1, 4):
                row = [u - a[r][t] * v for u, v in zip(row, x[t])]
            x[r] = [u * rp[r] for u in row]
    return np.array(x) if ok else None


def gain(Pm, R, inverse4):
    Pm = np.asarray(Pm, dtype=np.float64).reshape(4, 4)
    inv = inverse4(Pm + np.asarray(R, dtype=np.float64).reshape(4, 4))
    if inv is None:
        return None
    K = np.empty((4, 4))
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                s = np.float64(0.0)
                for t in range(4):
                    s = s + Pm[i, t] * inv[t, j]
                K[i, j] = s
    return K
