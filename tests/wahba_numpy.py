"""NumPy restatement of the per-call Wahba solve (csrc/pekf_math.hpp: make_frame, wahba_rotation, frame_degenerate,
wahba_rank1_rotation, shortest_arc, normal_of and their caller wahba_rotation_vectors), FAST = 0, operation for
operation in float64 over a batch of items (the device's selects are np.where).  NumPy does not contract a * b + c to
an fma as the device's compiler does, so the figures differ from the device's in the last bits, not in kind.

Two parameters tell the algebra as it stood from the present one:

    threshold   frame_degenerate calls a pair parallel where |t| <= threshold |m| (t Gram-Schmidt's remainder):
                TODAY's 1e-12 (as the code stood), or THRESHOLD = 2^-48 = 32 u, three times the 10 u that rounding
                can leave of an exactly parallel pair (pekf_math.hpp derives it)
    scaled      False: the vectors as given (a . a overflows from 2^512 and underflows from 2^-538); True: each of the
                four vectors times the power of two that brings its largest entry into [1/2, 1), the exponents folded
                into the two weights with their common exponent removed (pow2_normalise, fold_weights)
"""
import numpy as np

THRESHOLD = 2.0 ** -48
TODAY = dict(threshold=1e-12, scaled=False)
FIXED = dict(threshold=THRESHOLD, scaled=True)
NO_WEIGHT = -(1 << 20)      # the exponent of a zero weight: below every other


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def make_frame(a, m, sg=1.0):
    """e1, e2, u3 (n, 3) and alpha, beta1, beta2 (n,) of the pairs (a, m); sg as the device's (only its sign)."""
    sa = _dot(a, a)
    ia = 1.0 / np.sqrt(sa)
    e1 = a * ia[:, None]
    b1 = _dot(e1, m)
    t = m - b1[:, None] * e1
    sb = _dot(t, t)
    ib = np.copysign(1.0 / np.sqrt(sb), sg)
    e2 = t * ib[:, None]
    return dict(e1=e1, e2=e2, u3=_cross(e1, e2), alpha=np.sqrt(sa), beta1=b1, beta2=np.copysign(np.sqrt(sb), sg))


def wahba_sign(ka, km):
    return np.where(ka * km >= 0.0, 1.0, -1.0)


def wahba_rotation(W, V, ka, km):
    kw, kb = km * W["beta2"], km * W["beta1"]
    p = ka * W["alpha"] * V["alpha"] + kb * V["beta1"] + kw * V["beta2"]
    s = kw * V["beta1"] - kb * V["beta2"]
    ih = 1.0 / np.sqrt(p * p + s * s)
    p, s = p * ih, s * ih
    g0 = W["e1"] * p[:, None] + W["e2"] * s[:, None]
    g1 = W["e2"] * p[:, None] - W["e1"] * s[:, None]
    return (g0[:, :, None] * V["e1"][:, None, :] + g1[:, :, None] * V["e2"][:, None, :]
            + W["u3"][:, :, None] * V["u3"][:, None, :])


def frame_degenerate(F, threshold):
    b1, b2 = F["beta1"], F["beta2"]
    return ~(b2 * b2 > (threshold * threshold) * (b1 * b1 + b2 * b2)) | ~(F["e1"][:, 0] == F["e1"][:, 0])


def normal_of(v):
    ax, ay, az = np.abs(v[:, 0]), np.abs(v[:, 1]), np.abs(v[:, 2])
    j0 = (ax <= ay) & (ax <= az)
    j1 = ~j0 & (ay <= az)
    z = np.zeros(len(v))
    return np.stack([np.where(j0, z, np.where(j1, -v[:, 2], v[:, 1])), np.where(j0, v[:, 2], np.where(j1, z, -v[:, 0])),
                     np.where(j0, -v[:, 1], np.where(j1, v[:, 0], z))], axis=-1)


def shortest_arc(v, w):
    c = _dot(v, w)
    k = _cross(v, w)
    sk = _dot(k, k)
    n = normal_of(v)
    use_k = sk > 0.0
    ih = 1.0 / np.sqrt(np.where(use_k, sk, _dot(n, n)))
    h = np.where(use_k[:, None], k, n) * ih[:, None]
    d = 1.0 - c
    R = np.empty((len(v), 3, 3))
    R[:, 0, 0] = c + d * h[:, 0] * h[:, 0]
    R[:, 0, 1] = d * h[:, 0] * h[:, 1] - k[:, 2]
    R[:, 0, 2] = d * h[:, 0] * h[:, 2] + k[:, 1]
    R[:, 1, 0] = d * h[:, 1] * h[:, 0] + k[:, 2]
    R[:, 1, 1] = c + d * h[:, 1] * h[:, 1]
    R[:, 1, 2] = d * h[:, 1] * h[:, 2] - k[:, 0]
    R[:, 2, 0] = d * h[:, 2] * h[:, 0] - k[:, 1]
    R[:, 2, 1] = d * h[:, 2] * h[:, 1] + k[:, 0]
    R[:, 2, 2] = c + d * h[:, 2] * h[:, 2]
    return R


def wahba_rank1_rotation(acc0, mag0, acc, mag, ka, km):
    B = (ka[:, None, None] * (acc0[:, :, None] * acc[:, None, :])
         + km[:, None, None] * (mag0[:, :, None] * mag[:, None, :]))
    rn = B[:, :, 0] * B[:, :, 0] + B[:, :, 1] * B[:, :, 1] + B[:, :, 2] * B[:, :, 2]
    r0 = (rn[:, 0] >= rn[:, 1]) & (rn[:, 0] >= rn[:, 2])
    r1 = ~r0 & (rn[:, 1] >= rn[:, 2])
    iv = 1.0 / np.sqrt(np.where(r0, rn[:, 0], np.where(r1, rn[:, 1], rn[:, 2])))
    v = np.where(r0[:, None], B[:, 0], np.where(r1[:, None], B[:, 1], B[:, 2])) * iv[:, None]
    w = B[:, :, 0] * v[:, None, 0] + B[:, :, 1] * v[:, None, 1] + B[:, :, 2] * v[:, None, 2]
    iw = 1.0 / np.sqrt(_dot(w, w))
    return shortest_arc(v, w * iw[:, None])


def pow2_normalise(v):
    """v 2^-e and e (int), e the frexp exponent of v's largest |entry| (0 for a zero, non-finite or NaN vector)."""
    top = np.fmax(np.fmax(np.abs(v[:, 0]), np.abs(v[:, 1])), np.abs(v[:, 2]))
    e = np.where(np.isfinite(top), np.frexp(np.where(np.isfinite(top), top, 0.0))[1], 0).astype(np.int64)
    return np.ldexp(v, -e[:, None].astype(np.int32)), e


def fold_weights(ka, ea, km, em):
    """ka 2^ea and km 2^em with their common exponent removed: the larger of the two in [1/2, 1), a zero weight
    out of the comparison."""
    fa, xa = np.frexp(np.where(np.isfinite(ka), ka, 0.0))
    fm, xm = np.frexp(np.where(np.isfinite(km), km, 0.0))
    fa, fm = np.where(np.isfinite(ka), fa, ka), np.where(np.isfinite(km), fm, km)
    ta = np.where(fa != 0.0, xa + ea, NO_WEIGHT)
    tm = np.where(fm != 0.0, xm + em, NO_WEIGHT)
    top = np.maximum(ta, tm)
    clip = lambda d: np.maximum(d, -1100).astype(np.int32)     # (ldexp's int; below -1075 everything is 0 already)
    return np.ldexp(fa, clip(ta - top)), np.ldexp(fm, clip(tm - top))


def wahba_rotation_vectors(acc0, mag0, acc, mag, ka, km, threshold=THRESHOLD, scaled=True):
    """R (n, 3, 3) and which items took the rank-1 route (n,) bool."""
    acc0, mag0, acc, mag = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (acc0, mag0, acc, mag))
    ka, km = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (ka, km))
    with np.errstate(all="ignore"):
        if scaled:
            (acc0, e0), (mag0, f0), (acc, e1), (mag, f1) = (pow2_normalise(x) for x in (acc0, mag0, acc, mag))
            ka, km = fold_weights(ka, e0 + e1, km, f0 + f1)
        W = make_frame(acc0, mag0)
        V = make_frame(acc, mag, wahba_sign(ka, km))
        deg = frame_degenerate(W, threshold) | frame_degenerate(V, threshold)
        R = np.where(deg[:, None, None], wahba_rank1_rotation(acc0, mag0, acc, mag, ka, km), wahba_rotation(W, V, ka, km))
    return R, deg


def rotm_to_quat(M):
    """csrc/pekf_math.hpp rotm_to_quat (Wahba.py:19-47) over a batch, by selects"""
    M = np.asarray(M, dtype=np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        t1 = ((1.0 + M[:, 0, 0]) - M[:, 1, 1]) - M[:, 2, 2]
        t2 = ((1.0 - M[:, 0, 0]) + M[:, 1, 1]) - M[:, 2, 2]
        t3 = ((1.0 - M[:, 0, 0]) - M[:, 1, 1]) + M[:, 2, 2]
        b1 = (t1 > t2) & (t1 > t3)
        b2 = ~b1 & (t2 > t1) & (t2 > t3)
        S = np.sqrt(np.where(b1, t1, np.where(b2, t2, t3))) * 2.0
        sxy, sxz, syz = M[:, 0, 1] + M[:, 1, 0], M[:, 0, 2] + M[:, 2, 0], M[:, 1, 2] + M[:, 2, 1]
        w = np.where(b1, M[:, 2, 1] - M[:, 1, 2], np.where(b2, M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1])) / S
        own = 0.25 * S
        x = np.where(b1, own, np.where(b2, sxy / S, sxz / S))
        y = np.where(b2, own, np.where(b1, sxy / S, syz / S))
        z = np.where(b1, sxz / S, np.where(b2, syz / S, own))
    return np.stack([w, x, y, z], axis=-1)
