"""The per-call gain K = P^- inv(P^- + R) on the device (inverse4, csrc/pekf_math.hpp, behind k_op<OpPredict>,
k_call1<OpPredict> and the resident service's svc_predict_wave) against exact solves across the conditioning of S: the
families of tests/percall_families.py, cond(S) from 1 to 1e10, a graded S of cond 1e12 and well-conditioned ones scaled
by 2^+-200, 2^+-266 and 2^+-400 -- where kat.npz's one well-conditioned trajectory, the fuzz's well-conditioned draws
and the route-against-route comparisons of the other per-call tests cannot see an error.  The conditions (the exact
rational gain, np.linalg.inv's error e_lu against it, yard = max(e_lu, e_lu[general_0])) come from the reference
quantities alone; tests/test_percall_conditioning_cpu.py pins them and shows that the rule fails the 2x2-cofactor
inverse this file was written against (eps cond^2; non-finite or falsely singular from 2^+-266).

Shapes: twenty families x 26 items side by side, 520 items in one launch (two full 256-item blocks and a third of 8).

Measured on MI355X: see test_gain_against_the_exact_solution."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from oracle import ekf_numpy as npo
from poseestimationkf_amd._lib import check, lib

from . import percall_families as pf
from . import percall_numpy as pn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = (0, 8, 17, 25)     # of each family, through the n = 1 routes


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    prev = engine.percall_mode()
    yield engine
    engine.percall_mode(prev)


@pytest.fixture(autouse=True)
def _mode_restored(eng):
    prev = eng.percall_mode()
    yield
    eng.percall_mode(prev)


@pytest.fixture(scope="module")
def fam(kat):
    return pf.families(kat)


@pytest.fixture(scope="module")
def ref(kat):
    return pf.reference(kat)


@pytest.fixture(scope="module")
def batch(fam):
    """The 520 items side by side and {family: its rows} (shared, not modified)"""
    return pf.side_by_side(fam)


def _predict_dev(eng, ops, n):
    """pekf_predict_dev with a status plane on n items -> z, Pm, K, status"""
    bi = [eng.DeviceBuffer(a.nbytes).upload(a) for a in (np.ascontiguousarray(ops[k][:n], dtype=np.float64) for k in pf.FIELDS)]
    bo = [eng.DeviceBuffer(8 * n * w) for w in (4, 16, 16)]
    sb = eng.DeviceBuffer(4 * n).upload(np.full(n, -1, np.int32))
    check(lib.pekf_predict_dev(n, *[b.ptr for b in bi], *[b.ptr for b in bo], sb.ptr, None))
    z, Pm, K = (b.download((n, w), np.float64) for b, w in zip(bo, (4, 16, 16)))
    return z, Pm.reshape(n, 4, 4), K.reshape(n, 4, 4), sb.download((n,), np.int32)


@pytest.fixture(scope="module")
def launch(eng, batch):
    """The one engine.predict call over all 520 items: z, Pm, K (no LinAlgError: every status 0)"""
    cat, _ = batch
    return eng.predict(*[cat[k] for k in pf.FIELDS])


@pytest.fixture(scope="module")
def judged(batch, launch):
    """Per item, with the device's own P^- as the input: K_exact of it (S = fl(Pm + R)), the device's err, and the
    err of the pivoted restatement (tests/percall_numpy.py, no fma) on the same P^-."""
    cat, _ = batch
    _, Pm, K = launch
    n = len(Pm)
    e_dev, e_np = np.empty(n), np.empty(n)
    for i in range(n):
        exact = pf.gain_exact(Pm[i], Pm[i] + cat["R"][i])
        restated = pn.gain(Pm[i], cat["R"][i], pn.inverse4_pivoted)
        e_dev[i] = pf.err(K[i], exact)
        e_np[i] = np.inf if restated is None else pf.err(restated, exact)
    return e_dev, e_np


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_device_pointer_route_and_status(eng, batch, launch):
    """pekf_predict_dev with a status plane on the same 520 items: z, Pm, K bit for bit engine.predict's, every
    status 0 -- no false "singular" on the scaled families -- and every K finite."""
    cat, sl = batch
    z, Pm, K, st = _predict_dev(eng, cat, 520)
    assert not st.any(), {n: np.nonzero(st[s])[0] for n, s in sl.items() if st[s].any()}
    for got, want in zip((z, Pm, K), launch):
        assert np.array_equal(_bits(got), _bits(want).reshape(got.shape))
    assert np.isfinite(K).all() and np.isfinite(Pm).all()


def test_state_prediction(batch, launch):
    """z within 1e-14 of the reference's RK4 (oracle/ekf_numpy.rk4) on every item"""
    cat, _ = batch
    want = np.array([npo.rk4(cat["X"][i], cat["dt"][i], cat["gyro"][i]) for i in range(520)])
    assert np.abs(launch[0] - want).max() <= 1e-14


def test_prior_covariance(batch, launch, ref):
    """Pm within PM_ULPS = 12 ulp of the largest entry of the exact A P A^T + Jb Q Jb^T, item by item: 8x the 1.5 ulp
    that the reference's own arithmetic is held to (1.45 measured, test_percall_conditioning_cpu.py).
    Measured on MI355X: at most 1.45 ulp (spd_8), every family's figure the reference arithmetic's own."""
    _, sl = batch
    for name, s in sl.items():
        worst = max(pf.pm_error_ulps(pm, ex) for pm, ex in zip(launch[1][s], ref[name]["Pm_exact"]))
        print("k_predict %-12s Pm within %.2f ulp of its largest entry" % (name, worst))
        assert worst <= pf.PM_ULPS, name


def test_gain_against_the_exact_solution(batch, ref, judged):
    """err(K) <= 8 yard[family] for every item, K_exact the exact rational Pm inv(fl(Pm + R)) of the device's own Pm;
    yard = max(e_lu, e_lu[general_0]), e_lu the worst error of the reference's np.linalg.inv statement on the family;
    the 8 is test_magcal_conditioning's margin of a device solve over the reference's LU.
    Measured on MI355X, the worst error as a ratio to e_lu, next to the NumPy restatement's on the same Pm (which
    does not contract to fma), and the same ratio of the 2x2-cofactor inverse4 this one replaced, on the same box:
        family        cond(S) to  e_lu      device  restatement  cofactor form
        trajectory    3.5e0       4.27e-16  1.000   1.000        1.05
        spd_0         1.0e0       3.33e-16  1.000   1.003        1
        spd_2         1.0e2       6.22e-15  0.696   0.795        2.24
        spd_4         1.0e4       4.94e-13  0.973   1.331        74.3
        spd_6         1.0e6       3.67e-11  1.152   1.089        1.5e+03
        spd_8         1.0e8       5.56e-9   0.984   1.304        1.71e+04
        spd_10        1.0e10      5.29e-7   0.730   0.921        9.47e+05
        general_0     1.0e0       3.33e-16  0.676   1.000        1.33
        general_2     1.0e2       3.65e-15  1.103   1.181        4.28
        general_4     1.0e4       5.10e-13  1.205   1.695        47.2
        general_6     1.0e6       6.85e-11  0.739   0.639        529
        general_8     1.0e8       4.92e-9   0.975   1.205        2.14e+04
        general_10    1.0e10      4.74e-7   1.035   1.110        5.17e+05
        graded        2.8e12      6.40e-15  0.553   0.595        0.889
        scaled_+200   1.0e0       3.33e-16  1.000   1.003        1
        scaled_-200   1.0e0       3.33e-16  1.000   1.003        1
        scaled_+266   1.0e0       3.33e-16  1.000   1.003        3e+15
        scaled_-266   1.0e0       3.33e-16  1.000   1.003        not finite (26)
        scaled_+400   1.0e0       3.33e-16  1.000   1.003        not finite (26)
        scaled_-400   1.0e0       3.33e-16  1.000   1.003        singular (26)
    (the cofactor form's status plane called all 26 items of scaled_-400 singular, and engine.predict raised.)"""
    _, sl = batch
    e_dev, e_np = judged
    for name, s in sl.items():
        r = ref[name]
        print("k_predict %-12s cond(S) to %.1e: e_lu %.2e, K error %.3e = %.3f e_lu (restatement %.3f)"
              % (name, r["cond"].max(), r["e_lu"], e_dev[s].max(), e_dev[s].max() / r["e_lu"], e_np[s].max() / r["e_lu"]))
    for name, s in sl.items():
        assert e_dev[s].max() <= pf.MARGIN * ref[name]["yard"], name


def test_exactly_singular_items_still_raise(eng, batch, launch):
    """An exactly singular S -- all zero; two identical rows with R = 0 (percall_families.singular_items) -- at items
    64 and 256 of a 257-item call (a wave's first lane; the second block's only item): status 1 and an all-NaN K for
    exactly those, every other row the 520-item launch's, LinAlgError through engine.predict; and through both n = 1
    routes for each of the two."""
    cat, _ = batch
    ops = {k: np.array(cat[k][:257]) for k in pf.FIELDS}
    items, _ = pf.singular_items()
    for at, it in zip((64, 256), items):
        for k in pf.FIELDS:
            ops[k][at] = it[k]
    z, Pm, K, st = _predict_dev(eng, ops, 257)
    hit = np.zeros(257, bool)
    hit[[64, 256]] = True
    assert np.array_equal(st, hit.astype(np.int32))
    assert np.array_equal(np.isnan(K).all(axis=(1, 2)), hit) and np.array_equal(np.isnan(K).any(axis=(1, 2)), hit)
    for got, want in zip((z, Pm, K), launch):
        assert np.array_equal(_bits(got[~hit]), _bits(want[:257][~hit]).reshape(got[~hit].shape))
    with pytest.raises(np.linalg.LinAlgError):
        eng.predict(*[ops[k] for k in pf.FIELDS])
    for mode in (eng.PERCALL_LAUNCH, eng.PERCALL_SERVICE):
        eng.percall_mode(mode)
        for it in items:
            with pytest.raises(np.linalg.LinAlgError):
                eng.predict(*[it[k] for k in pf.FIELDS])


def test_n1_routes_give_the_batched_rows(eng, batch, launch):
    """Items 0, 8, 17 and 25 of every family one at a time, through k_call1 (PERCALL_LAUNCH) and through the resident
    service (PERCALL_SERVICE, svc_predict_wave): z, Pm and K bit for bit the 520-item launch's rows."""
    cat, sl = batch
    for mode in (eng.PERCALL_LAUNCH, eng.PERCALL_SERVICE):
        eng.percall_mode(mode)
        for name, s in sl.items():
            for i in (s.start + j for j in SAMPLE):
                got = eng.predict(*[cat[k][i] for k in pf.FIELDS])
                for g, want in zip(got, launch):
                    assert np.array_equal(_bits(g).reshape(-1), _bits(want[i]).reshape(-1)), (mode, name, i)


def test_dropin_prediction_on_an_ill_conditioned_item(eng, batch, launch, ref, judged, monkeypatch):
    """dropin.ExtendedKalmanFilter.KalmanFilter.Prediction with P, Q, R of one spd_6 item (cond(S) 1e6) set on the
    object: z, P^- and K bit for bit the batched row, so K is within 8 yard of the exact gain there too."""
    monkeypatch.syspath_prepend(os.path.join(ROOT, "poseestimationkf_amd", "dropin"))
    for m in ("ExtendedKalmanFilter", "Wahba", "UtilityFunctions", "_bootstrap"):
        sys.modules.pop(m, None)
    from ExtendedKalmanFilter import KalmanFilter
    cat, sl = batch
    i = sl["spd_6"].start + 5
    kf = KalmanFilter(0.0, [0.5, 0.0, -0.86], [0.0, 0.1, 0.99], 0.5)
    kf.Q, kf.R = np.array(cat["Q"][i]), np.array(cat["R"][i])
    z, Pm, K = kf.Prediction(cat["gyro"][i], cat["dt"][i], cat["X"][i], cat["P"][i])
    for g, want in zip((z, Pm, K), launch):
        assert np.array_equal(_bits(g).reshape(-1), _bits(want[i]).reshape(-1))
    assert kf.previousT == cat["dt"][i] and judged[0][i] <= pf.MARGIN * ref["spd_6"]["yard"]
    for m in ("ExtendedKalmanFilter", "Wahba", "UtilityFunctions", "_bootstrap"):
        sys.modules.pop(m, None)
