"""The calibration clouds of tests/magcal_clouds.py without a GPU: what the families themselves are -- the
conditioning they span, that every system is positive definite and every phone's status decidable, that the mixed
families hold both kinds of quadric -- from the exact rational solution and NumPy alone, so the conditions of
tests/test_magcal_conditioning.py rest on the reference and not on the code under test; and the NumPy restatement
of k_magcal (tests/magcal_numpy.py) held to the same bounds as the device.

Measured (the restatement; fit error as a ratio to e_lu, the family's worst error of np.linalg.solve against the
exact solution; root residuals Jacobi / NumPy's eigh root):

    family            cond(A^T A)       kappa(R)  e_lu      fit / e_lu  W W - R          scaled
    generator         7.3e0 .. 1.5e1    2.8       2.51e-15  0.98        1.9e-15/3.9e-15  1.8e-15/2.5e-15
    sphere            2.6e0 .. 4.1e0    1.2       1.46e-15  1.16        2.2e-15/2.2e-15  2.2e-15/2.1e-15
    sphere_noiseless  2.7e0 .. 4.2e0    1.2       2.25e-15  1.18        1.7e-15/1.9e-15  2.0e-15/1.8e-15
    ratio5            3.6e2 .. 1.5e3    28        1.80e-13  0.99        1.9e-15/2.9e-15  3.4e-15/3.5e-15
    ratio20           1.5e5 .. 2.9e5    426       6.98e-11  1.06        2.3e-15/2.3e-15  5.1e-14/7.8e-14
    band03            2.5e2 .. 3.9e3    5.2       3.77e-14  1.36        1.3e-15/2.0e-15  2.4e-15/2.2e-15
    band005           3.9e5 .. 5.1e6    155       1.62e-11  0.70        1.4e-15/1.7e-15  1.9e-15/2.8e-14
    cap90             2.1e1 .. 2.0e2    6.6       1.20e-14  1.01        1.5e-15/1.7e-15  1.7e-15/2.4e-15
    cap45             4.4e2 .. 5.3e3    36        1.14e-14  1.25        1.8e-15/2.1e-15  2.5e-15/5.2e-15
    hard3000          6.7e0 .. 1.9e1    2.7       2.45e-15  1.08        2.0e-15/2.3e-15  2.3e-15/2.2e-15
    server_doubles    5.1e0 .. 1.7e1    2.9       2.57e-15  1.00        2.1e-15/2.1e-15  2.4e-15/2.1e-15
    ncal9             1.4e1 .. 9.3e3    138       3.34e-13  0.05        2.2e-15/2.0e-15  2.4e-15/7.7e-15
    ncal6             3.1e1 .. 3.1e7    4.8e4     6.78e-10  0.0002      1.5e-15/4.0e-15  6.1e-13/4.5e-12

(kappa(R) and the fit error over the ellipsoids only: 21 of 24 in band005, 49 of 70 in ncal9, 13 of 70 in ncal6,
whose worst-conditioned phones are other quadrics.)  The smallest margin |lam|min / |lam|max of an exact R is
3,450 x its 64 cond eps (an ncal6 phone), 1.2e5 x in the 100-sample families."""
import numpy as np
import pytest

from poseestimationkf_amd import wire  # noqa: F401  (server_doubles: the server's parse, a host function of libpekf)

from . import magcal_clouds as cl
from . import magcal_numpy as mc

NAMES = [f.name for f in cl.FAMILIES]


@pytest.fixture(scope="module")
def ref():
    return cl.reference()


@pytest.fixture(scope="module")
def model():
    """The restatement's calibration of every family's float64 samples (shared, not modified)."""
    out = {}
    for f in cl.FAMILIES:
        ev = cl.events(cl.samples(f.name)[1])
        out[f.name] = mc.calibrate(ev["types"], ev["values64"], n_cal=f.n_cal)
    return out


def test_cloud_generator():
    """cloud()'s own statement: float32 and repeatable; the noiseless cloud lies on the quadric A^-2 / field^2,
    whose eigenvalues give back `lam`; the band and the cap bound the direction's z (seen with A = I); the
    offset and the noise are within their bounds, the noise scaling with the field."""
    lam = np.array([0.4, 1.0, 2.0])
    m = cl.cloud(5, 400, 3, lam=lam, hard=0.0, noise=0.0)
    assert m.shape == (5, 400, 3) and m.dtype == np.float32
    assert np.array_equal(m, cl.cloud(5, 400, 3, lam=lam, hard=0.0, noise=0.0))
    ata, atb = mc.normal_equations(m.astype(np.float64))
    ev = np.linalg.eigvalsh(mc.r_of(np.linalg.solve(ata, atb[..., None])[..., 0]))
    assert np.allclose(np.sort(1.0 / np.sqrt(2500.0 * ev), axis=1), lam, rtol=1e-5)
    for kw, zlo, zhi in ((dict(zmax=0.3), -0.3, 0.3), (dict(zmax=0.05), -0.05, 0.05), (dict(cap=np.pi / 2), 0.0, 1.0),
                         (dict(cap=np.pi / 4), np.sqrt(0.5), 1.0), ({}, -1.0, 1.0)):
        c = cl.cloud(3, 2000, 4, lam=(1.0, 1.0, 1.0), hard=0.0, noise=0.0, **kw).astype(np.float64) / 50.0
        z, edge = c[..., 2], 0.02 * (zhi - zlo)
        assert np.abs(np.linalg.norm(c, axis=2) - 1.0).max() < 1e-6
        assert zlo - 1e-6 <= z.min() < zlo + edge and zhi - edge < z.max() <= zhi + 1e-6
        assert np.abs(np.arctan2(c[..., 1], c[..., 0])).max() > 3.0          # the whole azimuth
    h = cl.cloud(200, 1, 5, lam=(1.0, 1.0, 1.0), hard=3000.0)[:, 0].astype(np.float64)
    assert 2900.0 < np.abs(h).max() <= 3000.0 + 50.0 + 0.05 + 1e-3
    n = cl.cloud(4, 50, 6, field=5e-5, lam=(1.0, 1.0, 1.0), hard=0.0).astype(np.float64)
    dev = np.abs(np.linalg.norm(n, axis=2) / 5e-5 - 1.0).max()
    assert 1e-5 < dev < 2 * 0.05 / 50.0                                     # noise 0.05 at 50: 1e-3 of the field


def test_family_planes():
    """264 phones x 101 messages in 104 rows: four full waves and a partial one, the last 8 phones in a second
    256-lane block; server_doubles' FP64 samples are not float32-exact, every other family's are."""
    ev, sl = cl.family_events([f.name for f in cl.BIG], rows=104)
    assert ev["types"].shape == (104, 264) and sl["server_doubles"] == slice(240, 264)
    assert np.all(ev["types"][:101] == 2) and np.all(ev["types"][101:] == 4)
    exact32 = ev["values64"] == ev["values"].astype(np.float64)
    assert exact32[:, :240].all() and not exact32[:101, 240:].all(axis=(0, 2)).any()
    assert [(f.name, f.K, f.n_cal) for f in cl.SMALL] == [("ncal9", 70, 9), ("ncal6", 70, 6)]


@pytest.mark.parametrize("name", NAMES)
def test_conditioning_spread(ref, name):
    """The family's worst cond(A^T A) lies in the decade range written next to it in magcal_clouds.FAMILIES:
    `generator` within DESIGN's former claim (<= 240), band005 and ncal6 at 1e5 and beyond."""
    f, worst = cl.BY_NAME[name], ref[name]["cond"].max()
    print("%s: cond(A^T A) %.2e .. %.2e, e_lu %.3e" % (name, ref[name]["cond"].min(), worst, ref[name]["e_lu"]))
    assert f.cond_lo <= worst <= f.cond_hi
    assert cl.BY_NAME["generator"].cond_hi <= 240.0
    assert cl.BY_NAME["band005"].cond_lo >= 1e5 and cl.BY_NAME["ncal6"].cond_lo >= 1e5


@pytest.mark.parametrize("name", NAMES)
def test_every_system_is_definite_and_every_status_decidable(ref, name):
    """A^T A is positive definite in rationals for every phone, so status 2 is expected for none; and every
    exact R's |lam|min / |lam|max is at least 64 cond eps, so a fit within a few cond eps of the exact one has
    the exact one's classification: the device's status test excludes nobody."""
    r = ref[name]
    assert r["definite"].all()
    room = r["margin"] / (64.0 * r["cond"] * cl.EPS)
    print("%s: smallest margin %.3e, %.1f x its 64 cond eps" % (name, r["margin"].min(), room.min()))
    assert np.all(room >= 1.0)


@pytest.mark.parametrize("name", NAMES)
def test_mixed_status_families(ref, name):
    """band005, ncal9 and ncal6 hold at least 3 ellipsoids and 3 other quadrics each; the other families'
    phones are all ellipsoids."""
    ell = ref[name]["ellipsoid"]
    if name in cl.MIXED:
        assert ell.sum() >= 3 and (~ell).sum() >= 3
    else:
        assert ell.all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_on_the_family(ref, model, name):
    """The NumPy restatement under the device's conditions: status the exact classification (0 or 3), the
    not-calibrated outputs as the ABI says, fit within 8 e_lu of the exact solution -- and within 8x the worst
    error of np.linalg.solve over the ellipsoids alone, which in the mixed families is the smaller figure (ncal6:
    2.2e-13 against 6.8e-10) -- and the root checks."""
    r, got = ref[name], model[name]
    assert np.array_equal(got["status"], np.where(r["ellipsoid"], 0, 3))
    ok = got["status"] == 0
    assert np.all(got["bias"][~ok] == 0.0) and np.all(got["W"][~ok] == np.eye(3)) and np.isnan(got["fit"][~ok]).all()
    assert np.array_equal(got["bias"][ok], r["bias"][ok])
    e = mc.fit_error(got["fit"][ok], r["exact"][ok]).max()
    fig = cl.check_roots(got["W"][ok], got["fit"][ok])
    lam = np.linalg.eigvalsh(mc.r_of(got["fit"][ok]))
    print("%s (restatement): kappa(R) %.3g, fit / e_lu %.3f (/ e_lu of the ellipsoids %.3f), W W - R %.2e (eigh "
          "%.2e), scaled %.2e (eigh %.2e)" % ((name, (lam[:, -1] / lam[:, 0]).max(), e / r["e_lu"], e / r["e_lu_ell"]) + fig))
    assert e <= 8 * r["e_lu"]
    assert e <= 8 * r["e_lu_ell"]     # the same yardstick over the phones compared: no room lent by the others


@pytest.mark.parametrize("k", [-100, -20, 10, 60])
def test_restatement_commutes_with_a_power_of_two(model, k):
    """Samples times 2^k: bias 2^k, fit 2^-2k, W 2^-k times the unscaled ones and the same status, bit for bit."""
    for name in ("generator", "ratio20", "band005"):
        f = cl.BY_NAME[name]
        ev = cl.scaled_by(cl.events(cl.samples(name)[1]), k)
        cl.check_scaled(mc.calibrate(ev["types"], ev["values64"], n_cal=f.n_cal), model[name], k)


def test_restatement_on_reflected_integer_points():
    """magcal_clouds.reflected_points: every sum exact, so bias 0, fit[3:6] 0 (in the exact solution too), W
    diag(sqrt a, sqrt b, sqrt c) bit for bit, and fit[:3] within 8 e_lu of the exact solution."""
    p = cl.reflected_points()
    r = cl.reference_of(p, 96)
    assert r["definite"].all() and r["ellipsoid"].all() and np.all(r["exact"][:, 3:] == 0.0) and r["e_lu"] > 0.0
    ev = cl.events(p)
    got = mc.calibrate(ev["types"], ev["values64"], n_cal=96)
    cl.check_reflected(got, r)
