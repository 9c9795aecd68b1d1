"""The two-arc Wahba quaternion with its weights folded into the 2x2 core (pekf_math.hpp: wahba_product_ref),
restated in NumPy on the CPU, on the three streams of tests/test_wahba_two_arc_cpu.py.

What changed against the form that file restates (two_arc there), and what is checked of each change:

  * Arc 1 selects its factor, mu = 1 or w, and forms A1 = mu n_y, A2 = -(mu n_x), where it selected between
    n_y and w n_y (n_x and w n_x).  A product with 1.0 is exact, so the values are the same bit for bit:
    compared as bit patterns on every record.
  * The weights sum to one, km = 1 - ka, so the core (C, S) = ka (aW a'_x, -aW a'_y) + km (T1, T2) is formed
    as the blend T + ka (. - T), T1 = b1W m'_x + b2W m'_y, T2 = b2W m'_x - b1W m'_y, and km is not formed.
    The rounding differs; the bound is that file's own, 2e-15 against its np.longdouble yardstick (the
    unfolded two-arc form in extended precision), on every record.  The kernel contracts each of these
    expressions' products into FMAs, NumPy rounds every product; both are within the bound's 6x margin
    over the measured 3e-16.
  * The reflection test reads ka: km = 1 - ka >= 0 exactly when ka <= 1.  A difference of two doubles is
    zero only if they are equal and otherwise has the sign of the exact difference (gradual underflow), and
    NaN fails both comparisons: checked at the f32 and FP64 values next to 1 (the record formats' ka), at
    +-0, the extremes, inf and NaN.
"""
import numpy as np
import pytest

from .test_wahba_two_arc_cpu import (TARGETS, arc1_terms, normal_to, pair_in_own_frame, stream,  # noqa: F401
                                     two_arc, unit_toward)

BOUND = 2e-15   # tests/test_wahba_two_arc_cpu.py's bound for the FP64 form against the yardstick


def folded(a, m, aW, b1W, b2W, dtype=np.float64, want_cs=False):
    """q' unnormalised, as wahba_product_ref forms it now; arguments as two_arc's."""
    a, m = a.astype(dtype), m.astype(dtype)
    aW, b1W, b2W = (np.asarray(v).astype(dtype) for v in (aW, b1W, b2W))
    ka = np.abs(a[..., 2])
    n, N, rho2 = arc1_terms(a, m)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    w = N + np.abs(nz)
    f1 = nz >= 0
    mu = np.where(f1, dtype(1), w)
    A0, A1, B2 = np.where(f1, w, rho2), mu * ny, mu * nx
    ax, ay = A0 * a[..., 0] - B2 * a[..., 2], A0 * a[..., 1] - A1 * a[..., 2]
    mx, my = A0 * m[..., 0] - B2 * m[..., 2], A0 * m[..., 1] - A1 * m[..., 2]
    T1 = b1W * mx + b2W * my
    T2 = b2W * mx - b1W * my
    C = T1 + ka * (aW * ax - T1)
    S = T2 - ka * (aW * ay + T2)
    wt = np.sqrt(C * C + S * S) + np.abs(C)
    ft = C >= 0
    c0, c3 = np.where(ft, wt, S), np.where(ft, S, wt)
    q = np.stack([c0 * A0, c0 * A1 + c3 * B2, c3 * A1 - c0 * B2, c3 * A0], axis=-1)
    return (q, C, S) if want_cs else q


@pytest.fixture(scope="module")
def streams(stream):
    """{name: (a, m)} the stream as generated and under the two remountings, and the pair's own coordinates"""
    a, m, acc0, mag0 = stream
    out = {}
    for name, target in TARGETS.items():
        if target is None:
            out[name] = (a, m)
        else:
            M = normal_to(a, m, target)
            out[name] = (np.einsum("kij,wkj->wki", M, a), np.einsum("kij,wkj->wki", M, m))
    return out, pair_in_own_frame(acc0, mag0)[:3]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("name", list(TARGETS))
def test_selected_factor_equals_selected_products(streams, name):
    a, m = streams[0][name]
    n, N, _ = arc1_terms(a, m)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    w = N + np.abs(nz)
    f1 = nz >= 0
    mu = np.where(f1, 1.0, w)
    second = float((~f1).mean())
    print("%s: %d records, %.1f %% in arc 1's second form" % (name, f1.size, 100 * second))
    if name == "normal at -z":
        assert second > 0.3
    if name == "normal at +z":
        assert second < 0.7
    assert np.array_equal(_bits(mu * ny), _bits(np.where(f1, ny, w * ny)))
    assert np.array_equal(_bits(mu * nx), _bits(np.where(f1, nx, w * nx)))


@pytest.mark.parametrize("name", list(TARGETS))
def test_folded_core_against_the_extended_precision_yardstick(streams, name):
    (a, m), (aW, b1W, b2W) = streams[0][name], streams[1]
    ref = two_arc(a, m, aW, b1W, b2W, np.longdouble)
    ref = (ref / np.sqrt((ref * ref).sum(-1))[..., None]).astype(np.float64)
    assert np.isfinite(ref).all()
    qf = unit_toward(folded(a, m, aW, b1W, b2W), ref)
    q2 = unit_toward(two_arc(a, m, aW, b1W, b2W), ref)
    assert np.isfinite(qf).all() and qf.shape == a.shape[:-1] + (4,)
    df, d2 = float(np.abs(qf - ref).max()), float(np.abs(q2 - ref).max())
    ka = np.abs(a[..., 2])
    print("%s: %d records, ka in [%.3g, %.8f]: max |dq| folded %.3e, unfolded %.3e"
          % (name, ka.size, ka.min(), ka.max(), df, d2))
    assert df <= BOUND


def test_reflection_test_on_ka():
    one32, one64 = np.float32(1), np.float64(1)
    near = [one32, np.nextafter(one32, np.float32(0)), np.nextafter(one32, np.float32(2)),
            np.nextafter(np.nextafter(one32, np.float32(0)), np.float32(0)),
            np.nextafter(np.nextafter(one32, np.float32(2)), np.float32(2)),
            one64, np.nextafter(one64, 0.0), np.nextafter(one64, 2.0),
            np.nextafter(np.nextafter(one64, 0.0), 0.0), np.nextafter(np.nextafter(one64, 2.0), 2.0)]
    rest = [0.0, -0.0, np.finfo(np.float64).tiny, 5e-324, 0.04, 0.5, 2.0, np.finfo(np.float32).max,
            np.finfo(np.float64).max, np.inf, -np.inf, np.nan, -1.0, -np.nextafter(one32, np.float32(2))]
    ka = np.array([np.float64(v) for v in near + rest])
    with np.errstate(invalid="ignore"):
        old, new = (1.0 - ka) >= 0.0, ka <= 1.0
    assert np.array_equal(old, new)
    assert new[:2].all() and not new[2] and new[5:7].all() and not new[7]      # both sides of 1 are there
    assert not new[len(near) + rest.index(np.inf)] and not old[np.isnan(ka)].any()
    # the kernel's ka = |acc_z| of every f32 within 2^-12 of 1, both sides
    bits = np.arange(-(1 << 12), (1 << 12) + 1, dtype=np.int64) + int(np.float32(1).view(np.uint32))
    f = bits.astype(np.uint32).view(np.float32).astype(np.float64)
    assert f.min() < 1 < f.max() and np.array_equal((1.0 - f) >= 0.0, f <= 1.0)
