"""The device front-end's two record algebras (csrc/pekf_phase3.hpp) restated in float64 Python with IEEE division and
sqrt as the hardware seeds -- TEST INFRASTRUCTURE ONLY, for tests/test_frontend_conditioning_cpu.py: what the rule of
tests/test_frontend_conditioning.py passes and what it catches, shown without a GPU.  No fma contraction, so the
device's figures differ in the last bits.

    form "f32"  lpf_record: f = num * recip(den), v = (y2 - y1) * f + y1          (f32 events)
    form "f64"  lerp_scaled: d = |den|, s = den < 0 ? -num : num, v d = (y2 - y1) * s + y1 * d, NaN at d = 0
                                                                                    (FP64 events)
    both        x = v * rsqrt(v.v) (rsqrt_sumsq), l <- beta l + alpha x from zero, beta = 1 - alpha

recip and rsqrt are a seed and one Newton step, as on the device; the seed here is the IEEE quotient, so the step moves
the last bit at most -- but it keeps the device's behaviour at the edges: recip(0) and, as rsqrt stood (`stood=True`),
rsqrt(inf) are NaN (inf * 0 in the residual).

Mutations (`mut`): "sign" -- the sign of a negative denominator dropped (f64: s = num; f32: recip(|den|));
"mean" -- the phase-2 mean not selected where acc_0 / mag_0 still holds it (the slot's zero start is read);
"recip_seed" / "rsqrt_seed" -- the hardware seed's 5.6e-8 relative error left in, the Newton step skipped."""
import math

import numpy as np

SEED_ERROR = 5.6e-8     # v_rcp_f64 / v_rsq_f64, measured (pekf_math.hpp)
DBL_MAX = float(np.finfo(np.float64).max)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def recip(x, mut=None):
    r = _div(1.0, x)
    if mut == "recip_seed":
        return r * (1.0 + SEED_ERROR)
    return r + r * (1.0 - x * r)


def rsqrt(x, mut=None, stood=False):
    with np.errstate(all="ignore"):
        y = float(1.0 / np.sqrt(np.float64(x)))
    if mut == "rsqrt_seed":
        return y * (1.0 + SEED_ERROR)
    e = 1.0 - ((x if stood else min(x, DBL_MAX)) * y) * y if not math.isnan(x) else math.nan
    return y + y * (0.5 * e)


def records(item, tuples, form, mut=None, stood=False):
    """The item's records by the device's algebra -> (R, 2, 3) low-pass outputs {acc, mag}; tuples: the families
    module's (frontend_families.tuples(item))"""
    alpha = item["alpha"]
    beta = 1.0 - alpha
    low = np.zeros((2, 3))
    out = []
    for r, rec in enumerate(tuples):
        for c, (t1, t2, t3, y1, y2) in enumerate(rec[2:]):
            y1, y2 = [float(x) for x in y1], [float(x) for x in y2]
            if mut == "mean" and t1 == item["t_init"] and y1 == [float(x) for x in item[("init_acc", "init_mag")[c]]]:
                y1 = [0.0, 0.0, 0.0]
            num, den = float(t3 - t1), float(t2 - t1)
            if form == "f32":
                f = num * recip(abs(den) if mut == "sign" else den, mut)
                v = [(b - a) * f + a for a, b in zip(y1, y2)]
            else:
                d, s = abs(den), (-num if den < 0.0 and mut != "sign" else num)
                v = [(b - a) * s + a * d for a, b in zip(y1, y2)]
                if d == 0.0:
                    v[0] = math.nan
            inv = rsqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], mut, stood)
            low[c] = [beta * l + alpha * (x * inv) for x, l in zip(v, low[c])]
        out.append(low.copy())
    return np.array(out).reshape(-1, 2, 3)
