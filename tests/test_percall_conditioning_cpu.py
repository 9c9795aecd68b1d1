"""The predict families of tests/percall_families.py without a GPU: what the families themselves are -- the
conditioning of S = P^- + R they span, the error e_lu of the reference's own K = P^- np.linalg.inv(S) against the exact
rational gain, how exactly P^- is formed -- from NumPy and rationals alone, so the conditions of
tests/test_percall_conditioning.py rest on the reference and not on the code under test; and the rule err(K) <= 8 yard
shown to tell the two algebras of csrc/pekf_math.hpp's inverse4 apart on their NumPy restatements
(tests/percall_numpy.py: no fma contraction, so the device's figures differ in the last bits).

Measured (26 items a family; e_lu the worst error of the reference's statement; the two restatements' worst error as a
ratio to yard = max(e_lu, e_lu[general_0]); P^- of the reference's arithmetic against the exact one in ulps of its
largest entry):

    family        cond(S)             e_lu      cofactor  pivoted LU  P^- ulps
    trajectory    1.3e0 .. 3.5e0      4.27e-16  1.00      1.00        0.70
    spd_0         1.0e0               3.33e-16  1.33      1.00        1.37
    spd_2         1.0e2               6.22e-15  2.46      0.80        1.18
    spd_4         1.0e4               4.94e-13  67.4      1.33        1.01
    spd_6         1.0e6               3.67e-11  2.41e3    1.09        1.25
    spd_8         1.0e8               5.56e-9   4.62e4    1.30        1.45
    spd_10        1.0e10              5.29e-7   7.49e5    0.92        0.97
    general_0     1.0e0               3.33e-16  1.33      1.00        1.13
    general_2     1.0e2               3.65e-15  5.81      1.18        0.94
    general_4     1.0e4               5.10e-13  47.7      1.69        0.95
    general_6     1.0e6               6.85e-11  749       0.64        0.82
    general_8     1.0e8               4.92e-9   3.11e4    1.21        1.37
    general_10    1.0e10              4.74e-7   8.80e5    1.11        0.98
    graded        5.6e11 .. 2.8e12    6.40e-15  1.53      0.60        0.35
    scaled_+-200  1.0e0               3.33e-16  1.33      1.00        1.37
    scaled_+-266  1.0e0               3.33e-16  inf       1.00        1.37
    scaled_+-400  1.0e0               3.33e-16  inf / singular  1.00  1.37

The cofactor form passes 8 yard on trajectory, spd_0/2 and general_0/2, fails every spd_k / general_k from k = 4 (by
eps cond^2 against LAPACK's eps cond) and, its determinant being a product of four entries, gives a non-finite K at
2^+-266 and 2^+400 and a false "singular" at 2^-400.  The pivoted LU passes everywhere, at most 1.69 yard.  All six
scaled families are kept: e_lu on each is spd_0's bit for bit."""
import numpy as np
import pytest

from oracle import ekf_numpy as npo

from . import percall_families as pf
from . import percall_numpy as pn


@pytest.fixture(scope="module")
def fam(kat):
    return pf.families(kat)


@pytest.fixture(scope="module")
def ref(kat):
    return pf.reference(kat)


@pytest.fixture(scope="module")
def restated(fam, ref):
    """{algebra: {family: worst err}} of the two restatements on the reference's own P^- (inf: singular or not
    finite), and which items the cofactor form calls singular."""
    out = {"cofactor": {}, "pivoted": {}, "singular": {}}
    for name in pf.NAMES:
        f, r = fam[name], ref[name]
        for key, inv4 in (("cofactor", pn.inverse4_cofactor), ("pivoted", pn.inverse4_pivoted)):
            K = [pn.gain(r["Pm"][i], f["R"][i], inv4) for i in range(pf.ITEMS)]
            out[key][name] = max(np.inf if k is None else pf.err(k, r["K_exact"][i]) for i, k in enumerate(K))
            if key == "cofactor":
                out["singular"][name] = sum(k is None for k in K)
    return out


def test_families(fam):
    """Twenty families of 26 items, 520 side by side (a third 256-item block); repeatable; X unit; the spd families'
    P symmetric and the general ones' P, Q and R not; the scaled families spd_0 times an exact power of two."""
    assert len(pf.NAMES) == 20 and list(fam) == pf.NAMES
    cat, sl = pf.side_by_side(fam)
    assert cat["P"].shape == (520, 4, 4) and sl["scaled_-400"] == slice(494, 520)
    for name, f in fam.items():
        assert [f[k].shape for k in pf.FIELDS] == [(26, 3), (26,), (26, 4), (26, 4, 4), (26, 3, 3), (26, 4, 4)]
        assert np.abs(np.linalg.norm(f["X"], axis=1) - 1.0).max() < 1e-15 or name == "trajectory"
    for name in pf.SPD:
        assert np.array_equal(fam[name]["P"], fam[name]["P"].transpose(0, 2, 1))
    for name in pf.GENERAL:
        for k in ("P", "Q", "R"):       # every item's far from symmetric, R with no zero entry
            m = fam[name][k]
            skew = np.abs(m - m.transpose(0, 2, 1)).max(axis=(1, 2))
            assert np.all(skew > 0.1 * np.abs(m).max(axis=(1, 2))) and np.all(fam[name]["R"] != 0.0)
    for j in pf.JS:
        for s in (1, -1):
            f = fam["scaled_%+d" % (s * j)]
            for k in ("P", "Q", "R"):
                assert np.array_equal(np.ldexp(f[k], -s * j), fam["spd_0"][k])
            assert all(np.array_equal(f[k], fam["spd_0"][k]) for k in ("gyro", "dt", "X"))


@pytest.mark.parametrize("name", pf.NAMES)
def test_conditioning_band(ref, name):
    """Every item's cond(S) lies in its family's band: within a decade of 10^k for spd_k and general_k; graded at
    1e10 .. 1e14 while D^-1 S D^-1 stays below 100 (badly scaled, not ill conditioned)."""
    r, (lo, hi) = ref[name], pf.BAND[name]
    print("%-12s cond(S) %.2e .. %.2e, e_lu %.3e, yard %.3e" % (name, r["cond"].min(), r["cond"].max(), r["e_lu"], r["yard"]))
    assert lo <= r["cond"].min() and r["cond"].max() <= hi
    if name == "graded":
        inner = r["S"] / pf.GRADING[:, None] / pf.GRADING[None, :]
        assert np.linalg.cond(inner).max() < 100.0


def test_reference_error_grows_with_cond(ref):
    """e_lu rises along both ladders (by eps cond: more than 1e7 from k = 0 to 10) and is positive everywhere; the
    scaled families' e_lu is spd_0's, so every j stays (within the 2x their statement allows)."""
    for ladder in (pf.SPD, pf.GENERAL):
        e = [ref[n]["e_lu"] for n in ladder]
        assert all(b > 4.0 * a for a, b in zip(e, e[1:])), e
        assert e[-1] > 1e7 * e[0]
    assert all(r["e_lu"] > 0.0 and r["yard"] >= ref["general_0"]["e_lu"] for r in ref.values())
    for name in pf.SCALED:
        assert ref[name]["e_lu"] <= 2.0 * ref["spd_0"]["e_lu"]
        assert np.array_equal(ref[name]["e_lu_item"], ref["spd_0"]["e_lu_item"])


@pytest.mark.parametrize("name", pf.NAMES)
def test_prior_covariance_is_formed_to_a_few_ulp(fam, ref, name):
    """P^- as the reference's arithmetic forms it (bit for bit oracle/ekf_numpy.predict's) is within PM_ULPS / 8 =
    1.5 ulp of the largest entry of the exact A P A^T + Jb Q Jb^T; the device gets the 8x margin of the gain."""
    f, r = fam[name], ref[name]
    worst = 0.0
    for i in range(pf.ITEMS):
        assert np.array_equal(npo.predict(*[f[k][i] for k in pf.FIELDS])[1], r["Pm"][i])
        worst = max(worst, pf.pm_error_ulps(r["Pm"][i], r["Pm_exact"][i]))
    print("%-12s P^- within %.2f ulp of its largest entry" % (name, worst))
    assert worst <= pf.PM_ULPS / pf.MARGIN


def test_exact_gain_is_exact(ref):
    """gain_exact against an independent route: K_exact S = Pm to the rounding of K_exact alone, in rationals."""
    for name in ("spd_10", "general_10", "graded", "scaled_-400"):
        r = ref[name]
        for i in (0, 25):
            K, S, Pm = pf._fr(r["K_exact"][i]), pf._fr(r["S"][i]), pf._fr(r["Pm"][i])
            inv = pf.inverse_exact(S)
            true = pf._mul(Pm, inv)
            top = max(abs(x) for row in true for x in row)
            assert max(abs(K[a][b] - true[a][b]) for a in range(4) for b in range(4)) <= top * pf.EPS / 2
            assert pf._mul(S, inv) == [[int(a == b) for b in range(4)] for a in range(4)]


PASSES = ["trajectory", "spd_0", "spd_2", "general_0", "general_2"]


@pytest.mark.parametrize("name", pf.NAMES)
def test_rule_tells_the_algebras_apart(ref, restated, name):
    """err <= 8 yard on the restatements: the pivoted LU passes on every family; the cofactor form passes on the
    well-conditioned five (graded and 2^+-200 are not held against it either way), fails from k = 4, and from |j| = 266 returns singular or a non-finite K."""
    yard = ref[name]["yard"]
    cof, piv = restated["cofactor"][name], restated["pivoted"][name]
    print("%-12s cofactor %.3g yard (%d singular), pivoted %.3g yard" % (name, cof / yard, restated["singular"][name], piv / yard))
    assert piv <= pf.MARGIN * yard
    if name in PASSES:
        assert cof <= pf.MARGIN * yard
    elif name in pf.SPD + pf.GENERAL:
        assert cof > pf.MARGIN * yard and np.isfinite(cof)
    elif name in pf.SCALED and abs(int(name.split("_")[1])) >= 266:
        assert cof == np.inf


def test_singular_items():
    """The two exactly singular predicts: S is what singular_items says (all zero; rows 0 and 1 identical) with R = 0,
    the reference raises on both, both restatements report singular, and so does the exact inverse."""
    items, want = pf.singular_items()
    for it, S in zip(items, want):
        Pm = pf.pm_reference(it["gyro"], it["X"], it["P"], it["Q"])
        assert np.array_equal(Pm + it["R"], S) and not it["R"].any()
        with pytest.raises(np.linalg.LinAlgError):
            npo.predict(*[it[k] for k in pf.FIELDS])
        assert pn.inverse4_pivoted(S) is None and pn.inverse4_cofactor(S) is None
        assert pf.inverse_exact(pf._fr(S)) is None
    assert np.array_equal(want[1][0], want[1][1]) and np.linalg.matrix_rank(want[1]) == 3
