"""Inputs that isolate the two halves of the fused record step (csrc/pekf_step.hpp ekf_record_step) that do not involve
P: the propagation (pekf_math.hpp rk4_closed / rk4_closed_w with state_norm2's snap, behind k_run, k_run_one, k_update
and k_gyro_chain) and the measurement (wahba_product_ref + wahba_toward_from_product of the loop form,
wahba_quat_toward(const Frame &) of the plain form).  NumPy only, deterministic: nothing here comes from the code
under test.  The exact results and the error of the reference's own float64 statements against them are in
tests/golden/step_families.npz (tests/golden/make_step_golden.py, mpmath); tests/test_step_halves_cpu.py pins both.

The isolations.  A record with the missing-magnetometer bit is X = RK4(X), P = P-: a run of such records is the
gyro chain through the fused kernels' own code.  With P0 = I, a gyro sample of |w| = 2 (A P A^T = I), q = 1 and
r = R_GAIN_ONE = 2^-70 the gain is one to 2r: X is Wahba's quaternion Y, flipped toward z, to 2^-69.

ITEMS = 32 items a family, the kinds of a family taken in turn.  Every set comes as "f64" and as "f32": there the
samples are float32 values and every dt is a whole number of ns, below 2^31 - 1 in the record's word or escaped
to the float64 side plane; the exact result is that of the item as rounded.

Propagation items: X0 (4,), n records (gyro (3,), dt_ns), judged on the last X.  Away from chain an item has 1, 2 or
3 records of its kind (so the multi-record kernels' lazy records, both ping-pong halves, see every kind).
theta = h |w| / 2 is the half angle of a record.

    ordinary  |w| in 0.1 .. 4 rad/s, dt in 5 .. 20 ms
    tiny      |w| = 10^-3k, k = 1 .. 8 (theta down to ~1e-26: a phone at rest)
    roots     theta^2 = (6 - sqrt 12, 6, 6 + sqrt 12) (1 + (0, 1e-3, -1e-6, 1e-9)): the roots of RK4's two coefficients
              1 - x/2 + x^2/24 and 1 - x/6, dt ~ 2^30 ns (dt is chosen after |w| is rounded, so both sets land there)
    huge      dt = 2^31 - 2 - i - 32 l (the top of the word's range), |w| = 10^1 .. 10^6: theta up to 1e6
    longdt    escaped dts in 2^32 .. 2^45 ns, |w| in 0.1 .. 4
    back      negative (escaped) dts, -5 ms .. -20 s
    offunit   |X0| in 2^-40, 1e-3, 0.7, 3, 1e3, 2^40, and |X0|^2 - 1 = +-2.8e-14, +-9e-14, +-1.1e-13: beside
              state_norm2's snap to 1 (2.9e-14; it stood at 1e-13)
    sparse    a one-axis gyro on the basis-vector states, every other one with a second component of 1e-9
    chain     64 records: ordinary ones (even items), and huge ones of |w| in 10 .. 100 (odd items; a covariance
              that grows by |w|^2 / 4 a record stays finite over 64 of them)

prop_apart(): w = 0, dt = 0 and both on exactly representable unit states; NaN, +Inf and -Inf in a gyro component;
X0 = 0 -- there the reference's X is NaN.

Measurement items: (acc0, mag0, acc, mag, X0), weights the filter's own k_acc = |acc_z|, k_mag = 1 - k_acc
(ExtendedKalmanFilter.py:71).  n = a x m is the measured plane's normal, (C, S) the in-plane turn of
wahba_product_ref.

    ordinary        unit pairs, angles in U(0.3, 1.3)
    thin_current    the current pair's angle in THIN = 1e-2 .. 3e-12 and pi - 1e-8 (f32: THIN32, no thinner than 1e-6,
                    so that rounding makes no pair exactly parallel)
    thin_reference  the same for the reference pair
    flat            |acc_z| in 1e-3, 1e-6, 1e-9, 1e-12 (k_acc -> 0)
    upright         1 - |acc_z| in the same steps (k_mag -> 0; f32: 1e-3 .. 1e-6, since 1 - 1e-9 rounds to 1)
    raw_units       |acc| = |acc0| = 9.81, |mag| = |mag0| = 48: k_mag < 0 for most, the matrix chain
    normal_near_z   n within 1e-2, 1e-4, 1e-6, 1e-8 rad of +z and of -z: both forms of arc 1 beside their select
    quarter_turn    C / |(C, S)| = +-1e-2 .. +-1e-8, S of either sign: both forms of q_theta beside their select; and
                    (C, S) within 1e-2 .. 1e-8 rad of (-H, 0), either side: where the first form alone would cancel
    near_optimum    the optimum 1e-2, 1e-4, 1e-6 from the identity, and pi - 1e-4 about x, y and z
    mag_scale       f64 only: mag0 times 2^100 and mag times 2^-100 (even items) or the reverse (odd): the product
                    mag0 mag^T, and B with it, is unchanged, and every intermediate of the product form is not.  (Scaling
                    both by 2^100 would weigh the accelerometer term 2^-200: rank 1 to any float64 statement.)

X0 is a float64 optimum (the closed form below, good to the pair's conditioning) turned about a random axis by one of
TURNS, item by item across the families: 1e-3 and 1 rad, 100, 150 and 152 degrees (|q.z| = cos(turn / 2) either side
of 1/4, the product form's fallback) and, one item in eleven, 170 degrees (the fallback, and |q.z| < 0.2: no sign asked).

meas_apart(): acc_z = +-0 exactly (k_acc = 0) and acc = (0, 0, +-1) exactly (k_mag = 0): B has rank 1, judged by the
optimum tr(R^T B) it attains, as tests/test_degenerate_samples.py does.
"""
import os

import numpy as np

from . import wahba_families as wf
from .wahba_families import FAST_MARGIN, INFORMATIVE, MARGIN, U  # noqa: F401  (the Wahba pin's constants)

SEED = 20261022
ITEMS = 32
NS = 1e-09                         # ExtendedKalmanFilter.py:32
DT_WORD_MAX = 2 ** 31 - 2          # the largest dt the record's word holds (2^31 - 1 is the escape)
R_GAIN_ONE = 2.0 ** -70
GAIN_GYRO, GAIN_DT = (2.0, 0.0, 0.0), 1000.0
SNAP = 2.9e-14                    # state_norm2's kNormSnap
SNAP_STOOD = 1e-13
SIGN_QZ = 0.2

PROP = ["ordinary", "tiny", "roots", "huge", "longdt", "back", "offunit", "sparse", "chain"]
ROOTS = (6.0 - np.sqrt(12.0), 6.0, 6.0 + np.sqrt(12.0))
ROOT_EPS = (0.0, 1e-3, -1e-6, 1e-9)
OFF_SCALE = (2.0 ** -40, 1e-3, 0.7, 3.0, 1e3, 2.0 ** 40)
OFF_DELTA = (2.8e-14, -2.8e-14, 9e-14, -9e-14, 1.1e-13, -1.1e-13)
CHAIN = 64

MEAS = ["ordinary", "thin_current", "thin_reference", "flat", "upright", "raw_units", "normal_near_z", "quarter_turn",
        "near_optimum", "mag_scale"]
MEAS32 = [n for n in MEAS if n != "mag_scale"]
THIN = wf.THIN
THIN32 = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, np.pi - 1e-4)
STEPS = (1e-3, 1e-6, 1e-9, 1e-12)
STEPS32 = (1e-3, 1e-4, 1e-5, 1e-6)
NEAR = (1e-2, 1e-4, 1e-6, 1e-8)
TURNS = (1e-3, 1.0, np.deg2rad(100), np.deg2rad(150), np.deg2rad(152)) * 2 + (np.deg2rad(170),)
MFIELDS = ("acc0", "mag0", "acc", "mag")


def _r32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _unit(rng, shape, d=3):
    v = rng.normal(size=tuple(shape) + (d,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _lengths(nk):
    i = np.arange(ITEMS)
    return 1 + (i + (i // nk if nk % 3 == 0 else 0)) % 3


# ------------------------------------------------------------------------------------------ propagation
def prop_kinds(name):
    k = {"tiny": ["1e-%02d" % (3 * j) for j in range(1, 9)],
         "roots": ["%s %+g" % (r, e) for r in ("6-sqrt12", "6", "6+sqrt12") for e in ROOT_EPS],
         "huge": ["1e%d" % j for j in range(1, 7)],
         "longdt": ["2^%d" % e for e in range(32, 45)],
         "back": ["-%.0e ns" % (5e6 * 4000.0 ** (j / 7.0)) for j in range(8)],
         "offunit": ["|X0| %.3g" % s for s in OFF_SCALE] + ["n2-1 %+.1e" % d for d in OFF_DELTA],
         "sparse": ["e%d" % j for j in range(4)],
         "chain": ["ordinary", "huge"]}.get(name, [name])
    return [k[i % len(k)] for i in range(ITEMS)]


def _prop_family(name, rng, form):
    L = CHAIN if name == "chain" else 3
    i = np.arange(ITEMS)
    nk = len(set(prop_kinds(name)))
    kind = (i % nk)[:, None]
    d = _unit(rng, (ITEMS, L))
    u, u2 = rng.uniform(size=(ITEMS, L)), rng.uniform(size=(ITEMS, L))
    X0 = _unit(rng, (ITEMS,), 4)
    mag = 0.1 * 40.0 ** u
    dt = 5e6 + 15e6 * u2
    n = _lengths(nk)
    lrow = np.arange(L)[None, :]
    top = DT_WORD_MAX - i[:, None] - 32.0 * lrow
    if name == "tiny":
        mag = 10.0 ** (-3.0 * (1 + kind)) * np.ones((1, L))
    elif name == "roots":
        th2 = np.array(ROOTS)[kind // 4] * (1.0 + np.array(ROOT_EPS)[kind % 4])
        mag = 2.0 * np.sqrt(th2) / (2.0 ** 30 * (1.0 + 0.01 * u) * NS)
    elif name == "huge":
        mag, dt = 10.0 ** (1.0 + kind) * np.ones((1, L)), top
    elif name == "longdt":
        dt = 2.0 ** (32 + kind) * (1.0 + u2)
    elif name == "back":
        dt = -5e6 * 4000.0 ** (kind / 7.0) * (1.0 + 0.1 * u2)
    elif name == "offunit":
        s = np.where(kind[:, 0] < 6, np.array(OFF_SCALE)[kind[:, 0] % 6],
                     np.sqrt(1.0 + np.array(OFF_DELTA)[(kind[:, 0] - 6) % 6]))
        X0 = X0 * s[:, None]
    elif name == "sparse":
        X0 = np.eye(4)[i % 4] + np.where((i // 4 % 2 == 1)[:, None], 1e-9 * np.eye(4)[(i + 1) % 4], 0.0)
        d = (np.eye(3)[(i // 4) % 3] * np.where(i % 2 == 0, 1.0, -1.0)[:, None])[:, None, :] * np.ones((1, L, 1))
    elif name == "chain":
        hg = kind == 1
        mag, dt = np.where(hg, 10.0 ** (1.0 + u), mag), np.where(hg, top, dt)
        n = np.full(ITEMS, CHAIN)
    gyro = d * mag[..., None]
    if form == "f32":
        gyro = _r32(gyro)
    if name == "roots":     # dt from the gyro as it is carried, so that theta^2 is the kind's in both sets
        dt = 2.0 * np.sqrt(th2) / (np.linalg.norm(gyro, axis=-1) * NS)
    if form == "f32":
        dt = np.rint(dt)
    return dict(X0=X0, gyro=gyro, dt=dt, n=n.astype(np.int32))


PROP_APART = ["w=0", "dt=0", "w=0 dt=0", "nan", "+inf", "-inf", "X0=0"]
PROP_APART_FINITE = 3


def prop_apart():
    """{X0 (7, 4), gyro (7, 1, 3), dt (7, 1), n}: PROP_APART's items, float32 values and whole dts (both sets)"""
    X0 = np.array([[0, 0, 1.0, 0], [0.5, 0.5, 0.5, 0.5], [-0.5, 0.5, -0.5, 0.5], [1.0, 0, 0, 0], [0, 1.0, 0, 0],
                   [0, 0, 0, 1.0], [0, 0, 0, 0]])
    gyro = np.array([[0, 0, 0], [1.0, 2.0, 3.0], [0, 0, 0], [np.nan, 0.125, 0.25], [0.125, np.inf, 0.25],
                     [0.125, 0.25, -np.inf], [0.125, 0.25, 0.5]])[:, None, :]
    dt = np.array([1e7, 0.0, 0.0, 1e7, 1e7, 1e7, 1e7])[:, None]
    return dict(X0=X0, gyro=gyro, dt=dt, n=np.ones(7, np.int32))


# ------------------------------------------------------------------------------------------ measurement
def meas_kinds(name, form="f64"):
    thin, steps = (THIN32, STEPS32) if form == "f32" else (THIN, STEPS)
    k = {"thin_current": ["%.6g" % t for t in thin], "thin_reference": ["%.6g" % t for t in thin],
         "flat": ["%.0e" % s for s in STEPS], "upright": ["%.0e" % s for s in steps],
         "normal_near_z": ["%sz %.0e" % (s, e) for s in "+-" for e in NEAR],
         "quarter_turn": ["C %s%.0e S %s" % (c, e, s) for s in "+-" for c in "+-" for e in NEAR]
         + ["half turn %.0e S %s" % (e, s) for s in "+-" for e in NEAR],
         "near_optimum": ["%.0e" % p for p in wf.PHI] + ["pi-1e-4 " + a for a in "xyz"],
         "mag_scale": ["mag0 up", "mag0 down"]}.get(name, [name])
    return [k[i % len(k)] for i in range(ITEMS)]


def _basis_of(nrm):
    """(u, v) unit with u x v = nrm for each unit nrm"""
    ax = np.eye(3)[np.argmin(np.abs(nrm), axis=1)]
    u = np.cross(nrm, ax)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u, np.cross(nrm, u)


def _arc_to_z(nrm):
    """the shortest-arc rotations A with A nrm = z (nrm unit, away from -z)"""
    out = np.empty((len(nrm), 3, 3))
    for j, v in enumerate(nrm):
        k = np.cross(v, [0.0, 0.0, 1.0])
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        out[j] = np.eye(3) + K + K @ K / (1.0 + v[2])
    return out


def _meas_family(name, rng, form):
    thin, steps = (THIN32, STEPS32) if form == "f32" else (THIN, STEPS)
    i = np.arange(ITEMS)
    nk = len(set(meas_kinds(name, form)))
    kind = i % nk
    one = np.ones(ITEMS)
    ordinary = lambda: rng.uniform(0.3, 1.3, ITEMS)   # noqa: E731
    thw = np.array(thin)[kind] if name == "thin_reference" else ordinary()
    thv = np.array(thin)[kind] if name == "thin_current" else ordinary()
    if name in ("thin_current", "thin_reference"):
        thw, thv = (thw, one) if name == "thin_reference" else (one, thv)
    acc0, mag0 = wf.pair(rng, thw)
    acc, mag = wf.pair(rng, thv)
    ph, sg = rng.uniform(0.0, 2.0 * np.pi, ITEMS), rng.choice([-1.0, 1.0], ITEMS)
    axes = _unit(rng, (ITEMS,))
    if name in ("flat", "upright"):
        z = np.array(STEPS)[kind] if name == "flat" else 1.0 - np.array(steps)[kind]
        rad = np.sqrt((1.0 - z) * (1.0 + z))
        acc = np.stack([rad * np.cos(ph), rad * np.sin(ph), sg * z], axis=1)
        p = np.cross(acc, axes)
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        mag = np.cos(thv)[:, None] * acc + np.sin(thv)[:, None] * p
    elif name == "raw_units":
        acc0, acc, mag0, mag = 9.81 * acc0, 9.81 * acc, 48.0 * mag0, 48.0 * mag
    elif name == "normal_near_z":
        e, side = np.array(NEAR)[kind % 4], np.where(kind < 4, 1.0, -1.0)
        nrm = np.stack([np.sin(e) * np.cos(ph), np.sin(e) * np.sin(ph), side * np.cos(e)], axis=1)
        uu, vv = _basis_of(nrm)
        al = rng.uniform(0.0, 2.0 * np.pi, ITEMS)
        acc = np.cos(al)[:, None] * uu + np.sin(al)[:, None] * vv
        mag = np.cos(al + thv)[:, None] * uu + np.sin(al + thv)[:, None] * vv
    elif name == "quarter_turn":
        # current pair congruent to the reference pair: after arc 1 its acc lies at the angle phi from x, and
        # (C, S) is along (cos phi, -sin phi)
        e = np.array(NEAR)[kind % 4] * np.where(kind % 8 < 4, 1.0, -1.0)
        phi = np.where(kind < 8, -1.0, 1.0) * (0.5 * np.pi - e)
        phi = np.where(kind < 16, phi, np.where(kind < 20, -1.0, 1.0) * (np.pi - np.array(NEAR)[kind % 4]))
        nrm = _unit(rng, (ITEMS,))
        nrm[:, 2] = np.where(i % 2 == 0, 1.0, -1.0) * np.abs(nrm[:, 2])
        nrm[:, 2] = np.where(np.abs(nrm[:, 2]) > 0.9, 0.5 * nrm[:, 2], nrm[:, 2])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        A = _arc_to_z(nrm)
        ap = np.stack([np.cos(phi), np.sin(phi), 0 * phi], axis=1)
        mp_ = np.stack([np.cos(phi + thw), np.sin(phi + thw), 0 * phi], axis=1)
        acc, mag = np.einsum("nji,nj->ni", A, ap), np.einsum("nji,nj->ni", A, mp_)
    elif name == "near_optimum":
        for j in range(ITEMS):
            T = wf.rodrigues(axes[j], wf.PHI[kind[j]]) if kind[j] < 3 else wf.rodrigues(np.eye(3)[kind[j] - 3], np.pi - 1e-4)
            acc[j], mag[j] = T @ acc0[j], T @ mag0[j]
    elif name == "mag_scale":
        e = np.where(kind == 0, 100, -100)[:, None]
        mag0, mag = np.ldexp(mag0, e), np.ldexp(mag, -e)
    f = dict(acc0=acc0, mag0=mag0, acc=acc, mag=mag)
    if form == "f32":
        f = {k: _r32(v) for k, v in f.items()}
    f["k_acc"] = np.abs(f["acc"][:, 2])
    f["k_mag"] = 1.0 - f["k_acc"]
    f["turn_axis"] = _unit(rng, (ITEMS,))
    return f


def optimum64(f):
    """The optimum's quaternion in float64 by the Gram-Schmidt frames and the 2 x 2 polar factor (plain arithmetic, no
    LAPACK: the same bits everywhere): where X0 starts from, not a yardstick"""
    def frame(a, m, sg):
        na = np.linalg.norm(a, axis=1)
        e1 = a / na[:, None]
        b1 = (e1 * m).sum(1)
        t = m - b1[:, None] * e1
        nt = np.linalg.norm(t, axis=1)
        e2 = sg[:, None] * t / nt[:, None]
        return e1, e2, np.cross(e1, e2), na, b1, sg * nt
    ka, km = f["k_acc"], f["k_mag"]
    sc = np.exp2(-np.round(np.log2(np.linalg.norm(f["mag"], axis=1))))[:, None]     # (mag_scale: an exact factor)
    sg = np.where(ka * km >= 0, 1.0, -1.0)
    w1, w2, w3, aw, b1w, b2w = frame(f["acc0"], f["mag0"] / sc, np.ones(len(ka)))
    v1, v2, v3, av, b1v, b2v = frame(f["acc"], f["mag"] * sc, sg)
    p = ka * aw * av + km * b1w * b1v + km * b2w * b2v
    s = km * b2w * b1v - km * b1w * b2v
    h = np.hypot(p, s)
    p, s = p / h, s / h
    g0, g1 = w1 * p[:, None] + w2 * s[:, None], w2 * p[:, None] - w1 * s[:, None]
    return optimum_quat_of(g0[:, :, None] * v1[:, None, :] + g1[:, :, None] * v2[:, None, :] + w3[:, :, None] * v3[:, None, :])


def optimum_quat_of(R):
    """the unit quaternion of each rotation (n, 3, 3): the column of 4 q q^T with the largest diagonal entry"""
    Q4 = np.empty((len(R), 4, 4))
    Q4[:, 0, 0] = 1 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    Q4[:, 1, 1] = 1 + R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2]
    Q4[:, 2, 2] = 1 - R[:, 0, 0] + R[:, 1, 1] - R[:, 2, 2]
    Q4[:, 3, 3] = 1 - R[:, 0, 0] - R[:, 1, 1] + R[:, 2, 2]
    Q4[:, 0, 1] = Q4[:, 1, 0] = R[:, 2, 1] - R[:, 1, 2]
    Q4[:, 0, 2] = Q4[:, 2, 0] = R[:, 0, 2] - R[:, 2, 0]
    Q4[:, 0, 3] = Q4[:, 3, 0] = R[:, 1, 0] - R[:, 0, 1]
    Q4[:, 1, 2] = Q4[:, 2, 1] = R[:, 0, 1] + R[:, 1, 0]
    Q4[:, 1, 3] = Q4[:, 3, 1] = R[:, 0, 2] + R[:, 2, 0]
    Q4[:, 2, 3] = Q4[:, 3, 2] = R[:, 1, 2] + R[:, 2, 1]
    col = np.argmax(np.einsum("nii->ni", Q4), axis=1)
    q = Q4[np.arange(len(R)), :, col]
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def qmul(a, b):
    """a (x) b, rows"""
    a0, a1, a2, a3 = a.T
    b0, b1, b2, b3 = b.T
    return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                     a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], axis=1)


MEAS_APART = ["acc_z=+0", "acc_z=-0", "acc=+z", "acc=-z"]


def meas_apart():
    """MEAS_APART's items (float32 values), X0 the identity turned by 1 rad"""
    acc0, mag0 = np.tile(wf.ACC0, (4, 1)), np.tile(wf.MAG0, (4, 1))
    acc = np.array([[0.75, -0.5, 0.0], [0.75, -0.5, -0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])
    mag = np.array([[0.5, 0.25, -0.75], [-0.5, 0.25, 0.75], [0.5, 0.25, -0.75], [-0.5, 0.25, 0.75]])
    f = dict(acc0=_r32(acc0), mag0=_r32(mag0), acc=acc, mag=mag)
    f["k_acc"] = np.abs(acc[:, 2])
    f["k_mag"] = 1.0 - f["k_acc"]
    f["X0"] = np.tile([np.cos(0.5), np.sin(0.5) * 0.6, 0.0, np.sin(0.5) * 0.8], (4, 1))
    return f


# ------------------------------------------------------------------------------------------ the sets
_cache = {}


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def prop_families(form="f64"):
    """{name: {X0 (32, 4), gyro (32, L, 3), dt (32, L), n (32,)}} in PROP's order; L = 3, chain's 64 (read-only)"""
    if ("p", form) not in _cache:
        _cache["p", form] = {n: _frozen(_prop_family(n, np.random.default_rng([SEED, 1, j]), form))
                             for j, n in enumerate(PROP)}
    return _cache["p", form]


def meas_families(form="f64"):
    """{name: {acc0, mag0, acc, mag (32, 3), k_acc, k_mag (32,), X0 (32, 4)}} in MEAS' order (MEAS32's for "f32")"""
    if ("m", form) not in _cache:
        out, at = {}, 0
        for j, n in enumerate(MEAS):
            if form == "f32" and n not in MEAS32:
                continue
            f = _meas_family(n, np.random.default_rng([SEED, 2, j]), form)
            half = 0.5 * np.array(TURNS)[(at + np.arange(ITEMS)) % len(TURNS)]
            dq = np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * f.pop("turn_axis")], axis=1)
            f["X0"] = qmul(optimum64(f), dq)
            out[n] = _frozen(f)
            at += ITEMS
        _cache["m", form] = out
    return _cache["m", form]


def prop_side_by_side(fam, names=None, apart=False):
    """The families' items in one batch of CHAIN rows (padded with copies of an item's last record, which its count
    leaves out) -> {X0 (n, 4), gyro (n, 64, 3), dt (n, 64), n}, {name: slice}; apart: prop_apart()'s items last"""
    names = list(fam) if names is None else names
    parts = [fam[n] for n in names] + ([prop_apart()] if apart else [])

    def pad(a):
        return np.concatenate([a, np.repeat(a[:, -1:], CHAIN - a.shape[1], axis=1)], axis=1) if a.shape[1] < CHAIN else a
    cat = dict(X0=np.concatenate([p["X0"] for p in parts]), gyro=np.concatenate([pad(p["gyro"]) for p in parts]),
               dt=np.concatenate([pad(p["dt"]) for p in parts]), n=np.concatenate([p["n"] for p in parts]))
    sl = {n: slice(j * ITEMS, (j + 1) * ITEMS) for j, n in enumerate(names)}
    if apart:
        sl["apart"] = slice(len(names) * ITEMS, len(names) * ITEMS + len(PROP_APART))
    return cat, sl


def meas_side_by_side(fam, names=None):
    names = list(fam) if names is None else names
    cat = {k: np.concatenate([fam[n][k] for n in names]) for k in MFIELDS + ("k_acc", "k_mag", "X0")}
    return cat, {n: slice(j * ITEMS, (j + 1) * ITEMS) for j, n in enumerate(names)}


# ------------------------------------------------------------------------------------------ judging
def golden():
    """tests/golden/step_families.npz (make_step_golden.py says what it holds), read once"""
    if "golden" not in _cache:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_families.npz")) as z:
            _cache["golden"] = {k: z[k] for k in z.files}
    return _cache["golden"]


def prop_yard(g, form, rows):
    """Y of the items rows: the worst error of oracle.ekf_numpy.rk4 chained in float64, in units of U, floored at 1"""
    return max(1.0, float(g["p_%s_err" % form][rows].max()) / U)


def meas_yard(g, form, rows):
    """Y_q of the items rows: the worst sign-insensitive error of oracle.ekf_numpy.wahba_quat"""
    return float(g["m_%s_err_q" % form][rows].max())


def err_state(X, X_exact):
    """max |X - X_exact| per item; inf where X is not finite"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        e = np.abs(X - X_exact).max(axis=1)
    return np.where(np.isfinite(X).all(axis=1), e, np.inf)


def sign_of(X, q_exact):
    """+1 where X is nearer q_exact than -q_exact, else -1"""
    return np.where(wf.same_sign(X, q_exact), 1, -1)
