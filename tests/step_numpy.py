"""NumPy restatements of the two halves of the fused record step that tests/step_families.py isolates, for
tests/test_step_halves_cpu.py: rk4_closed with state_norm2's snap (pekf_math.hpp, pekf_step.hpp) chained as the
one-record kernels (plain) and the multi-record loop (loop) chain it, and Wahba's quaternion as the loop form's product
of two arcs (tests/test_wahba_two_arc_cpu.two_arc is wahba_product_ref as it stands; two_arc_forms below is the same
algebra with either second form switchable).  IEEE float64 with no fma contraction and an exact 1 / sqrt, so the
device's figures differ in the last bits and by its rsqrt's 4.2e-15.  Each fault is one the rule must catch."""
import numpy as np

from . import step_families as sf
from . import wahba_numpy as wn
from .test_wahba_two_arc_cpu import arc1_terms, pair_in_own_frame, two_arc


def state_norm2(x, snap=sf.SNAP):
    n2 = (x * x).sum(-1)
    return np.where(np.abs(n2 - 1.0) < snap, 1.0, n2)


def rk4_closed(x, n2, dt_ns, w, shortcut=False):
    """z of rk4_closed: rows x (n, 4), n2 (n,), dt_ns (n,), w (n, 3) the raw gyro"""
    hw = 0.5 * w
    th2 = hw[:, 0] * hw[:, 0] + hw[:, 1] * hw[:, 1] + hw[:, 2] * hw[:, 2]
    h = dt_ns * sf.NS
    xx = (h * h) * th2
    ca = xx * (xx * (1.0 / 24.0) - 0.5) + 1.0
    cb = h * (1.0 - xx * (1.0 / 6.0))
    if shortcut:    # the fault: the identity for a small angle
        ca, cb = np.where(xx < 1e-16, 1.0, ca), np.where(xx < 1e-16, 0.0, cb)
    kk = ca * ca + (cb * cb) * th2
    inn = 1.0 / np.sqrt(kk * n2)
    a, c = ca * inn, cb * inn
    w0, w1, w2 = c * hw[:, 0], c * hw[:, 1], c * hw[:, 2]
    return np.stack([a * x[:, 0] - w0 * x[:, 1] - w1 * x[:, 2] - w2 * x[:, 3],
                     a * x[:, 1] + w0 * x[:, 0] + w2 * x[:, 2] - w1 * x[:, 3],
                     a * x[:, 2] + w1 * x[:, 0] - w2 * x[:, 1] + w0 * x[:, 3],
                     a * x[:, 3] + w2 * x[:, 0] + w1 * x[:, 1] - w0 * x[:, 2]], axis=1)


def chain(cat, form="plain", snap=sf.SNAP, shortcut=False, dt32=False, n2_one=False):
    """The last X of every item of a side-by-side batch (step_families.prop_side_by_side).
    plain: every record takes state_norm2 of the stored X (k_run_one, k_update, k_gyro_chain's launches of one);
    loop: the launch's first record does, the later ones take |x|^2 as it is, and X is normalised at the end (k_run).
    Faults: shortcut (rk4_closed's), dt32 (an escaped dt taken through float32), n2_one (|X|^2 = 1 whatever X is)."""
    x = np.array(cat["X0"], dtype=np.float64)
    with np.errstate(all="ignore"):
        for l in range(int(cat["n"].max())):
            dt = cat["dt"][:, l]
            if dt32:
                esc = (dt < 0) | (dt > sf.DT_WORD_MAX)
                dt = np.where(esc, dt.astype(np.float32).astype(np.float64), dt)
            n2 = state_norm2(x, snap) if (form == "plain" or l == 0) else (x * x).sum(-1)
            if n2_one and (form == "plain" or l == 0):
                n2 = np.ones(len(x))
            z = rk4_closed(x, n2, dt, cat["gyro"][:, l], shortcut)
            x = np.where((l < cat["n"])[:, None], z, x)
        if form == "loop":
            x = x / np.sqrt((x * x).sum(-1))[:, None]
    return x


def two_arc_forms(a, m, aW, b1W, b2W, arc1_second=True, theta_second=True):
    """two_arc's algebra; arc1_second / theta_second = False: the first form of that arc on both sides of its select"""
    ka = np.abs(a[..., 2])
    km = 1 - ka
    n, N, rho2 = arc1_terms(a, m)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    f1 = (nz >= 0) | (not arc1_second)
    w = N + (np.abs(nz) if arc1_second else nz)
    A0, A1, A2 = np.where(f1, w, rho2), np.where(f1, ny, w * ny), np.where(f1, -nx, -(w * nx))
    ax, ay = A0 * a[..., 0] + A2 * a[..., 2], A0 * a[..., 1] - A1 * a[..., 2]
    mx, my = A0 * m[..., 0] + A2 * m[..., 2], A0 * m[..., 1] - A1 * m[..., 2]
    kaw, kb, kw = ka * aW, km * b1W, km * b2W
    C = kaw * ax + kb * mx + kw * my
    S = kw * mx - kb * my - kaw * ay
    ft = (C >= 0) | (not theta_second)
    wt = np.sqrt(C * C + S * S) + (np.abs(C) if theta_second else C)
    c0, c3 = np.where(ft, wt, S), np.where(ft, S, wt)
    return np.stack([c0 * A0, c0 * A1 - c3 * A2, c0 * A2 + c3 * A1, c3 * A0], axis=-1)


def frame_quat(Fw):
    """the quaternion of each proper frame (n, 3, 3) [e1 e2 u3] (columns)"""
    return sf.optimum_quat_of(Fw)


def fused_quat(f, arc1_second=True, theta_second=True, parallel=0.0):
    """Wahba's quaternion in the world basis as the loop form has it (unit, sign free): q_W (x) q' with q' the two-arc
    product; items of k_mag < 0 by the matrix chain (the closed form of tests/wahba_numpy.py), as the fallback takes
    them.  parallel > 0, the fault: a pair whose Gram-Schmidt remainder is under parallel |m| takes the rank-1 route."""
    aW, b1W, b2W, Fw = pair_in_own_frame(f["acc0"], f["mag0"])
    with np.errstate(all="ignore"):
        if arc1_second and theta_second:
            qp = two_arc(f["acc"], f["mag"], aW, b1W, b2W)
        else:
            qp = two_arc_forms(f["acc"], f["mag"], aW, b1W, b2W, arc1_second, theta_second)
        qp = qp / np.sqrt((qp * qp).sum(-1))[:, None]
        q = sf.qmul(frame_quat(Fw), qp)
        ops = [f[k] for k in ("acc0", "mag0", "acc", "mag", "k_acc", "k_mag")]
        R, _ = wn.wahba_rotation_vectors(*ops, **wn.FIXED)
        q = np.where((f["k_acc"] > 1.0)[:, None], wn.rotm_to_quat(R), q)
        if parallel > 0.0:
            R, deg = wn.wahba_rotation_vectors(*ops, threshold=parallel, scaled=True)
            q = np.where(deg[:, None], wn.rotm_to_quat(R), q)
    return q
