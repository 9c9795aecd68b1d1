"""Phase 1 on the device (k_magcal, csrc/pekf_magcal.hip; k_magcal_resume, csrc/pekf_magcal_resume.hip with
csrc/pekf_magcal.hpp) against exact solves across cloud conditioning: the families of tests/magcal_clouds.py, from
cond(A^T A) of 3 to 3e7 and kappa(R) to 4.8e4, where the unpivoted Cholesky, the fixed six Jacobi sweeps and the two
hand-kept statements of the solve could go wrong unseen by the one-regime clouds of the other magcal tests.  The
conditions (the exact rational fit, np.linalg.solve's error e_lu against it, the exact classification) come from
the reference quantities alone; tests/test_magcal_conditioning_cpu.py pins them.

Shapes: eleven families x 24 phones side by side, 264 phones x 101 messages in 104 rows (four full waves and a
partial one, the last 8 phones in a second 256-lane block); ncal9 and ncal6 at 70 phones in launches of their own.

Measured on MI355X (FP64 events; the f32 form bit for bit the same): the tables in
test_fit_against_the_exact_solution and test_root -- the fit at most 1.49x the error of np.linalg.solve (band03),
both root residuals at or below those of NumPy's eigh root on every family."""
import numpy as np
import pytest

from . import magcal_clouds as cl
from . import magcal_numpy as mc

pytestmark = pytest.mark.gpu

BIG = [f.name for f in cl.BIG]
SMALL = [f.name for f in cl.SMALL]
NAMES = BIG + SMALL


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


@pytest.fixture(scope="module")
def ref():
    return cl.reference()


@pytest.fixture(scope="module")
def planes():
    """{launch: (event dict, n_cal, {family: its phones})}: "big" the eleven 100-sample families in 104 rows,
    ncal9 and ncal6 by themselves (10 and 7 rows).  Shared, not modified."""
    ev, sl = cl.family_events(BIG, rows=104)
    out = {"big": (ev, 100, sl)}
    for f in cl.SMALL:
        out[f.name] = (cl.family_events([f.name])[0], f.n_cal, {f.name: slice(0, f.K)})
    return out


@pytest.fixture(scope="module")
def launches(eng, planes):
    """The one launch of each plane with FP64 events (shared, not modified)"""
    return {key: eng.calibrate_magnetometer(ev, n_cal=n_cal, events="f64") for key, (ev, n_cal, _) in planes.items()}


@pytest.fixture(scope="module")
def device(planes, launches):
    """{family: dict(bias, W, fit, status) of its phones} from the shared launches"""
    out = {}
    for key, (_, _, sl) in planes.items():
        for name, s in sl.items():
            out[name] = {k: launches[key][k][s] for k in ("bias", "W", "fit", "status")}
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(got, want, phones=slice(None)):
    assert np.array_equal(got["status"], want["status"][phones])
    for key in ("bias", "W", "fit"):
        assert np.array_equal(_bits(got[key]), _bits(want[key][phones])), key


def test_fit_against_the_exact_solution(ref, device):
    """For the calibrated phones of every family: bias bit for bit mc.bias_of of the float64 samples
    (server_doubles: genuine doubles), and the fit within 8 e_lu[family] of the exact rational solution -- e_lu
    the worst error of np.linalg.solve, the reference model's method, on the same normal equations; the 8 is
    test_magcal_fixture_parity's margin over the reference's own LU.  Also within 8x e_lu over the ellipsoids
    alone, the smaller figure in the mixed families.
    Measured on MI355X, the fit error as a ratio to e_lu, next to the NumPy restatement's (which does not contract
    to fma):
        family            cond(A^T A) to  e_lu      device   restatement
        generator         1.5e1           2.51e-15  0.977    0.977
        sphere            4.1e0           1.46e-15  1.156    1.156
        sphere_noiseless  4.2e0           2.25e-15  1.000    1.176
        ratio5            1.5e3           1.80e-13  0.987    0.994
        ratio20           2.9e5           6.98e-11  0.817    1.058
        band03            3.9e3           3.77e-14  1.492    1.361
        band005           5.1e6           1.62e-11  0.725    0.704
        cap90             2.0e2           1.20e-14  1.058    1.014
        cap45             5.3e3           1.14e-14  0.673    1.248
        hard3000          1.9e1           2.45e-15  1.083    1.083
        server_doubles    1.7e1           2.57e-15  1.000    1.000
        ncal9             9.3e3           3.34e-13  0.041    0.054   (of the ellipsoids' 2.72e-14: 0.500, 0.662)
        ncal6             3.1e7           6.78e-10  0.0003   0.0002  (of the ellipsoids' 2.20e-13: 1.014, 0.753)"""
    for name in NAMES:
        r, got = ref[name], device[name]
        ok = got["status"] == 0
        assert ok.any()
        assert np.array_equal(_bits(got["bias"][ok]), _bits(r["bias"][ok])), name
        e = mc.fit_error(got["fit"][ok], r["exact"][ok]).max()
        print("k_magcal %-16s cond(A^T A) to %.1e: fit error %.3e = %.3f e_lu (%.3f e_lu of the ellipsoids)"
              % (name, r["cond"].max(), e, e / r["e_lu"], e / r["e_lu_ell"]))
        assert e <= 8 * r["e_lu"], name
        assert e <= 8 * r["e_lu_ell"], name


def test_event_forms_agree(eng, planes, launches):
    """The f32 form of the ten families whose samples are float32-exact: bias, fit, W and status bit for bit the
    FP64 form's."""
    names = [n for n in BIG if n != "server_doubles"]
    ev, sl = cl.family_events(names, rows=104)
    assert np.array_equal(ev["values64"], planes["big"][0]["values64"][:, :240])
    got = eng.calibrate_magnetometer(ev, n_cal=100, events="f32")
    _same(got, launches["big"], slice(0, 240))


def test_status(ref, device):
    """Status 0 where the exact R is positive definite and 3 where it is not, for every phone (each one's margin
    is at least 64 cond eps: test_magcal_conditioning_cpu.py); no status 2 (every A^T A is positive definite in
    rationals), none excluded.  Not calibrated: bias 0, W = I, fit NaN.  band005 holds 21 ellipsoids of 24, ncal9
    49 of 70, ncal6 13 of 70."""
    for name in NAMES:
        got, want = device[name], np.where(ref[name]["ellipsoid"], 0, 3)
        assert np.array_equal(got["status"], want), (name, np.nonzero(got["status"] != want)[0])
        bad = want != 0
        assert np.all(got["bias"][bad] == 0.0) and np.all(got["W"][bad] == np.eye(3)) and np.isnan(got["fit"][bad]).all()
        assert np.isfinite(got["fit"][~bad]).all() and np.isfinite(got["W"]).all()
    assert all((device[n]["status"] == 3).sum() >= 3 and (device[n]["status"] == 0).sum() >= 3 for n in cl.MIXED)


def test_root(device):
    """For the calibrated phones, with R of the device's own fit: W symmetric bit for bit, every eigenvalue of W
    > 0 (the principal root), and max|W W - R| / max|R| and the scaled max_ij |V^T (W W - R) V|_ij / sqrt(lam_i
    lam_j) each within 8x the same residual of NumPy's eigh root of the same R (family maxima).
    Measured on MI355X, Jacobi / eigh:
        family            kappa(R) to  W W - R            scaled
        generator         2.83         1.73e-15/2.45e-15  1.76e-15/2.23e-15
        sphere            1.25         2.15e-15/2.37e-15  2.17e-15/2.79e-15
        sphere_noiseless  1.16         1.88e-15/2.82e-15  2.08e-15/2.08e-15
        ratio5            27.6         1.95e-15/3.12e-15  2.21e-15/6.82e-15
        ratio20           426          1.55e-15/1.66e-15  3.26e-14/1.09e-13
        band03            5.17         1.76e-15/2.38e-15  1.75e-15/3.07e-15
        band005           155          2.17e-15/2.37e-15  2.18e-15/2.78e-14
        cap90             6.64         1.73e-15/2.53e-15  1.72e-15/3.46e-15
        cap45             36.3         1.62e-15/2.00e-15  1.99e-15/7.18e-15
        hard3000          2.67         1.63e-15/2.78e-15  2.05e-15/2.95e-15
        server_doubles    2.86         1.54e-15/4.09e-15  2.54e-15/3.49e-15
        ncal9             137          1.60e-15/2.79e-15  5.00e-15/8.37e-15
        ncal6             4.78e4       1.26e-15/1.66e-15  2.78e-13/6.63e-13

    The Jacobi root is at or below the eigh root in both metrics on every family; on the restatement five, four and
    six sweeps give the same verdict and three fail ten families."""
    for name in NAMES:
        got = device[name]
        ok = got["status"] == 0
        lam = np.linalg.eigvalsh(mc.r_of(got["fit"][ok]))
        fig = cl.check_roots(got["W"][ok], got["fit"][ok])
        print("k_magcal %-16s kappa(R) to %.3g: W W - R %.2e (eigh %.2e), scaled %.2e (eigh %.2e)"
              % ((name, (lam[:, -1] / lam[:, 0]).max()) + fig))


@pytest.mark.parametrize("k", [-20, 10])
def test_power_of_two_scaling(eng, planes, launches, k):
    """The generator and ratio20 planes with every sample times 2^k (k = -20: about tesla; +10: about raw counts;
    both stay float32-exact): bias 2^k, fit 2^-2k, W 2^-k times the unscaled launch's, and the same status, bit
    for bit -- sums, fma, divide, the square root of an even power and the tau ratio all commute with the
    scaling, and an absolute tolerance or constant in the pivot test or the rotation would not.  (Tried on MI355X:
    with `fabs(apq) < 1e-20` for jacobi_rot's `apq == 0.0` and `d > 1e-12` for the pivot test's `d > 0.0`, in both
    statements, these two cases fail and every other magcal test passes.)"""
    ev, sl = cl.family_events(["generator", "ratio20"], rows=104)
    scaled = cl.scaled_by(ev, k)
    assert np.array_equal(scaled["values"].astype(np.float64), scaled["values64"])
    for form in ("f64", "f32"):
        got = eng.calibrate_magnetometer(scaled, n_cal=100, events=form)
        base = {key: np.concatenate([launches["big"][key][planes["big"][2][n]] for n in ("generator", "ratio20")])
                for key in ("bias", "fit", "W", "status")}
        assert np.all(base["status"] == 0)
        cl.check_scaled(got, base, k)


def test_rotation_skip_path(eng):
    """magcal_clouds.reflected_points (8 phones, n_cal = 96): every sum is an exact integer, so the bias and
    fit[3:6] are exactly 0 and R is diagonal -- jacobi_rot returns at apq == 0 all 18 times -- and W is bit for
    bit diag(sqrt a, sqrt b, sqrt c); fit[:3] within 8 e_lu of the exact solution.
    Measured on MI355X (both event forms): fit 0.437 e_lu (e_lu 9.37e-16; the restatement 0.364)."""
    p = cl.reflected_points()
    r = cl.reference_of(p, 96)
    assert r["definite"].all() and r["ellipsoid"].all() and np.all(r["exact"][:, 3:] == 0.0) and r["e_lu"] > 0.0
    ev = cl.events(p, rows=104)
    for form in ("f64", "f32"):
        cl.check_reflected(eng.calibrate_magnetometer(ev, n_cal=96, events=form), r)


@pytest.mark.parametrize("key", ["big", "ncal6"])
def test_both_statements_of_the_solve(eng, planes, launches, key):
    """The same planes through engine.CalibrationSession in chunks of 7 rows (k_magcal_resume: the solve as
    csrc/pekf_magcal.hpp states it): cal, fit and status bit for bit the one launch's (k_magcal's own statement),
    test_magcal_resume.py's invariant on inputs where a difference between the two would show.  (Tried on MI355X:
    with `d > 1e-6 * ata[sym6(j, j)]` as the pivot test of pekf_magcal.hpp alone, ncal6 fails here and every test
    of test_magcal_resume.py passes.)"""
    ev, n_cal, _ = planes[key]
    E, K = ev["types"].shape
    s = eng.CalibrationSession(K, n_cal, "f64")
    for a in range(0, E, 7):
        s.feed({k: ev[k][a:a + 7] for k in ("types", "values", "values64", "times")})
    got, one = s.result(), launches[key]
    assert sorted(np.unique(got["status"])) == [0, 3]
    _same(got, one)
    c = got["cal"].download((K, 12), np.float64)
    assert np.array_equal(c[:, :3], got["bias"]) and np.array_equal(c[:, 3:].reshape(K, 3, 3), got["W"])
