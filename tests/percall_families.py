"""Predict operands across the conditioning of S = P^- + R, with their reference quantities, for the per-call gain
K = P^- inv(S) (ExtendedKalmanFilter.py:63-66; csrc/pekf_math.hpp inverse4, behind k_op<OpPredict>, k_call1<OpPredict>
and the resident service).  NumPy and exact rational arithmetic only: nothing here comes from the code under test, so
the conditions of tests/test_percall_conditioning.py rest on the reference (tests/test_percall_conditioning_cpu.py pins
them).

Families of ITEMS = 26 items of (gyro, dt, X, P, Q, R), X a unit quaternion; c = |gyro|^2 / 4 is the factor by which
A P A^T (A = 0.5 Omega(gyro), A A^T = c I) scales P's spectrum:

    trajectory   tests/golden/kat.npz's predict rows 0, 10, .., 250 (one well-conditioned filter run)
    spd_k        k in 0, 2, .., 10: P = Q1 diag(10^(-k [0, 1/3, 2/3, 1])) Q1^T symmetric, Q = q I, R = r I with
                 q = r = 1e-3 lam_min: cond(S) within a decade of 10^k
    general_k    the same k: P = Q1 diag(..) Q2^T (not symmetric), Q and R full and not symmetric, of the same sizes
    graded       S = D S0 D + (Q's term), D = diag(1, 1e-3, 1e3, 1), S0 = P0 + 0.1 I with P0's eigenvalues in [0.5, 2]:
                 cond(S) ~ 1e12, cond(S0) < 10 -- badly scaled, not ill conditioned (gyro = +-2 e_i, so that A is a
                 signed permutation and the grading reaches S exactly)
    scaled_+-j   j in 200, 266, 400: the spd_0 operands with P, Q and R times 2^(+-j).  Every j is kept: the scaling
                 is exact, so np.linalg.inv's error on each is spd_0's own, bit for bit (asserted, within the 2x the
                 families' statement allows).

Reference quantities (reference()):
    Pm        P^- as the reference forms it, matmul(matmul(A, P), A^T) + matmul(matmul(Jb, Q), Jb^T)
    Pm_exact  A P A^T + Jb Q Jb^T in rationals (a list of 4 x 4 Fractions per item)
    S         fl(Pm + R): the reference rounds that sum too
    K_exact   the exact rational Pm inv(S) (Gauss-Jordan on Fractions), each entry rounded once
    err(K)    max|K - K_exact| / max|K_exact| of an item
    e_lu[f]   the worst err of matmul(Pm, np.linalg.inv(S)) over family f: the reference's own statement
    yard[f]   max(e_lu[f], e_lu[general_0]): a family on which LAPACK happens to be exact does not demand the impossible
"""
from fractions import Fraction

import numpy as np

SEED = 20261021
ITEMS = 26
KS = (0, 2, 4, 6, 8, 10)
JS = (200, 266, 400)
EPS = 2.0 ** -52
MARGIN = 8.0        # a device solve over the reference's LU against an exact solution (test_magcal_conditioning.py)
# P^- against the exact one, in ulps of its largest entry: the reference's own arithmetic stays within 1.45 on every
# family (tests/test_percall_conditioning_cpu.py holds it to 1.5), and the device gets the gain's margin over that
PM_ULPS = 1.5 * MARGIN
FIELDS = ("gyro", "dt", "X", "P", "Q", "R")
GRADING = np.array([1.0, 1e-3, 1e3, 1.0])

SPD = ["spd_%d" % k for k in KS]
GENERAL = ["general_%d" % k for k in KS]
SCALED = ["scaled_%+d" % (s * j) for j in JS for s in (1, -1)]
NAMES = ["trajectory"] + SPD + GENERAL + ["graded"] + SCALED

# cond(S) band of each family: within a decade of its nominal figure
BAND = {"trajectory": (1.0, 10.0), "graded": (1e10, 1e14)}
for _k in KS:
    BAND["spd_%d" % _k] = BAND["general_%d" % _k] = (max(1.0, 10.0 ** (_k - 1)), 10.0 ** (_k + 1))
BAND.update({_n: BAND["spd_0"] for _n in SCALED})


def omega_half(w):
    a, b, c = w[0], w[1], w[2]
    return 0.5 * np.asarray([[0.0, -a, -b, -c], [a, 0.0, c, -b], [b, -c, 0.0, a], [c, b, -a, 0.0]])


def xi_half(q):
    return 0.5 * np.asarray([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])


def spectrum(k):
    return 10.0 ** (-k * np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0]))


def _orthogonal(rng, n=4):
    q, r = np.linalg.qr(rng.normal(size=(n, n)))
    return q * np.sign(np.diag(r))


def _common(rng):
    g = rng.normal(size=(ITEMS, 3))
    g *= (rng.uniform(1.0, 3.0, size=ITEMS) / np.linalg.norm(g, axis=1))[:, None]
    X = rng.normal(size=(ITEMS, 4))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return dict(gyro=g, dt=np.floor(rng.uniform(5e6, 2e7, size=ITEMS)), X=X)


def _spd(rng, k):
    f = _common(rng)
    lam, small = spectrum(k), 1e-3 * 10.0 ** -k
    P = np.empty((ITEMS, 4, 4))
    for i in range(ITEMS):
        q1 = _orthogonal(rng)
        m = (q1 * lam) @ q1.T
        P[i] = 0.5 * (m + m.T)
    f.update(P=P, Q=np.tile(small * np.eye(3), (ITEMS, 1, 1)), R=np.tile(small * np.eye(4), (ITEMS, 1, 1)))
    return f


def _general(rng, k):
    f = _common(rng)
    lam, small = spectrum(k), 1e-3 * 10.0 ** -k
    P = np.empty((ITEMS, 4, 4))
    for i in range(ITEMS):
        P[i] = (_orthogonal(rng) * lam) @ _orthogonal(rng).T
    f.update(P=P, Q=small * rng.normal(size=(ITEMS, 3, 3)), R=small * rng.normal(size=(ITEMS, 4, 4)))
    return f


def _graded(rng):
    f = _common(rng)
    f["gyro"] = np.zeros((ITEMS, 3))
    f["gyro"][np.arange(ITEMS), rng.integers(0, 3, ITEMS)] = rng.choice([-2.0, 2.0], ITEMS)
    P, R = np.empty((ITEMS, 4, 4)), np.empty((ITEMS, 4, 4))
    for i in range(ITEMS):
        q1 = _orthogonal(rng)
        p0 = (q1 * rng.uniform(0.5, 2.0, 4)) @ q1.T
        target = GRADING[:, None] * (0.5 * (p0 + p0.T)) * GRADING[None, :]
        A = omega_half(f["gyro"][i])               # a signed permutation: the two products are exact
        P[i] = A.T @ target @ A
        R[i] = np.diag(0.1 * GRADING * GRADING)
    f.update(P=P, Q=np.tile(1e-9 * np.eye(3), (ITEMS, 1, 1)), R=R)
    return f


def _trajectory(kat):
    idx = np.arange(ITEMS) * 10
    return {k: np.array(kat["pc_" + k][idx], dtype=np.float64) for k in FIELDS}


def _scaled(base, e):
    f = {k: v.copy() for k, v in base.items()}
    for k in ("P", "Q", "R"):
        f[k] = np.ldexp(f[k], e)
    return f


_cache = {}


def families(kat):
    """{name: {field: (ITEMS, ...) float64}} in NAMES' order (read-only, built once)."""
    if "families" not in _cache:
        out = {"trajectory": _trajectory(kat)}
        for n, k in enumerate(KS):
            out["spd_%d" % k] = _spd(np.random.default_rng([SEED, 1, n]), k)
        for n, k in enumerate(KS):
            out["general_%d" % k] = _general(np.random.default_rng([SEED, 2, n]), k)
        out["graded"] = _graded(np.random.default_rng([SEED, 3]))
        for j in JS:
            for s in (1, -1):
                out["scaled_%+d" % (s * j)] = _scaled(out["spd_0"], s * j)
        for f in out.values():
            for a in f.values():
                a.setflags(write=False)
        _cache["families"] = {n: out[n] for n in NAMES}
    return _cache["families"]


def side_by_side(fam, names=NAMES):
    """The families' operands in one batch, and {name: slice} of its rows."""
    cat = {k: np.concatenate([fam[n][k] for n in names]) for k in FIELDS}
    return cat, {n: slice(i * ITEMS, (i + 1) * ITEMS) for i, n in enumerate(names)}


# ------------------------------------------------------------------------------------------ reference quantities
def pm_reference(gyro, X, P, Q):
    """P^- in the reference's own arithmetic (ExtendedKalmanFilter.py:59-61)."""
    A, Jb = omega_half(gyro), xi_half(X)
    return np.matmul(np.matmul(A, P), A.transpose()) + np.matmul(np.matmul(Jb, Q), Jb.transpose())


def _fr(m):
    return [[Fraction(float(x)) for x in row] for row in np.asarray(m)]


def _mul(a, b):
    return [[sum(a[i][t] * b[t][j] for t in range(len(b))) for j in range(len(b[0]))] for i in range(len(a))]


def _tr(a):
    return [list(r) for r in zip(*a)]


def pm_exact(gyro, X, P, Q):
    """A P A^T + Jb Q Jb^T in rationals (0.5 w and 0.5 q are exact in float64)."""
    A, Jb = _fr(omega_half(gyro)), _fr(xi_half(X))
    a, b = _mul(_mul(A, _fr(P)), _tr(A)), _mul(_mul(Jb, _fr(Q)), _tr(Jb))
    return [[a[i][j] + b[i][j] for j in range(4)] for i in range(4)]


def pm_error_ulps(pm, exact):
    """max|pm - exact| in units of EPS max|exact|."""
    top = max(abs(x) for row in exact for x in row)
    worst = max(abs(Fraction(float(pm[i][j])) - exact[i][j]) for i in range(4) for j in range(4))
    return float(worst / (top * Fraction(EPS)))


def inverse_exact(S):
    """inv(S) in rationals by Gauss-Jordan (any non-zero pivot will do: the arithmetic is exact); None if singular."""
    n = len(S)
    a = [list(S[i]) + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        p = next((r for r in range(c, n) if a[r][c] != 0), None)
        if p is None:
            return None
        a[c], a[p] = a[p], a[c]
        d = a[c][c]
        a[c] = [x / d for x in a[c]]
        for r in range(n):
            if r != c and a[r][c] != 0:
                f = a[r][c]
                a[r] = [x - f * y for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


def gain_exact(Pm, S):
    """The exact Pm inv(S) of the float64 matrices Pm and S, each entry rounded once; None if S is singular."""
    inv = inverse_exact(_fr(S))
    if inv is None:
        return None
    return np.array([[float(x) for x in row] for row in _mul(_fr(Pm), inv)])


def err(K, K_exact):
    K = np.asarray(K, dtype=np.float64).reshape(4, 4)
    if not np.isfinite(K).all():
        return np.inf
    return float(np.abs(K - K_exact).max() / np.abs(K_exact).max())


def gain_lu(Pm, S):
    """The reference's statement (ExtendedKalmanFilter.py:63-66)."""
    return np.matmul(Pm, np.linalg.inv(S))


def reference_of(f):
    """Of one family's operands: Pm, Pm_exact, S, cond, K_exact, e_lu_item (per item) and e_lu (the worst)."""
    out = dict(Pm=np.empty((ITEMS, 4, 4)), S=np.empty((ITEMS, 4, 4)), K_exact=np.empty((ITEMS, 4, 4)),
               cond=np.empty(ITEMS), e_lu_item=np.empty(ITEMS), Pm_exact=[])
    for i in range(ITEMS):
        pm = pm_reference(f["gyro"][i], f["X"][i], f["P"][i], f["Q"][i])
        S = pm + f["R"][i]
        out["Pm"][i], out["S"][i] = pm, S
        out["Pm_exact"].append(pm_exact(f["gyro"][i], f["X"][i], f["P"][i], f["Q"][i]))
        out["K_exact"][i] = gain_exact(pm, S)
        sv = np.linalg.svd(S, compute_uv=False)
        out["cond"][i] = sv[0] / sv[-1]
        out["e_lu_item"][i] = err(gain_lu(pm, S), out["K_exact"][i])
    out["e_lu"] = float(out["e_lu_item"].max())
    return out


def reference(kat):
    """{name: reference_of(family)} with yard added (built once, read-only)."""
    if "reference" not in _cache:
        ref = {n: reference_of(f) for n, f in families(kat).items()}
        for r in ref.values():
            r["yard"] = max(r["e_lu"], ref["general_0"]["e_lu"])
        _cache["reference"] = ref
    return _cache["reference"]


def singular_items():
    """Two exactly singular predicts (operands as FIELDS), both with R = 0: the all-zero S, and an S with two
    identical rows reached exactly (gyro = 2 e_x makes A a signed permutation, Q = 0, small integer entries; the
    pivot of the identical pair is a power of two, so the elimination leaves an exactly zero row whichever way the
    pivot row is normalised)."""
    z = dict(gyro=np.zeros(3), dt=1e7, X=np.array([1.0, 0, 0, 0]), P=np.zeros((4, 4)), Q=np.zeros((3, 3)),
             R=np.zeros((4, 4)))
    S = np.array([[4.0, 1, 2, 1], [4, 1, 2, 1], [1, 2, 0, 1], [0, 1, 1, 2]])
    g = np.array([2.0, 0, 0])
    A = omega_half(g)
    twin = dict(gyro=g, dt=1e7, X=np.array([0.6, 0, 0.8, 0]), P=A.T @ S @ A, Q=np.zeros((3, 3)), R=np.zeros((4, 4)))
    return [z, twin], [np.zeros((4, 4)), S]
