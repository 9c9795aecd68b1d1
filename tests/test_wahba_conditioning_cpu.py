"""The Wahba families of tests/wahba_families.py without a GPU: what the families are -- the pairs' exact angles,
sigma_1 / sigma_2 of B, the error Y of the reference's own float64 statements (oracle.ekf_numpy.svd_rotation,
wahba_quat) against the exact optimum of tests/golden/wahba_families.npz -- so that the conditions of
tests/test_wahba_conditioning.py rest on the reference and not on the code under test; and the rule shown to tell the
closed form as it stood (frame_degenerate at 1e-12 |m|, vectors as given) from the present one (2^-48 |m|, vectors
brought to unit scale by powers of two) on their NumPy restatement (tests/wahba_numpy.py: no fma contraction, so the
device's figures differ in the last bits).

The rule, per family: the worst error over its items (max |R - R_exact|; for q, min(|q - q_e|, |q + q_e|)) is at most
8 Y for the IEEE routes and 8 (4.2e-15 / 2^-53) Y ~ 303 Y for the FAST route, Y the worst error of the reference's
statement over the same items; a family counts only where that bound is below 0.5.

Measured (32 items a family; theta the thinner pair's angle; the restatements' worst error as a ratio to Y):

    family           theta            cond(B)           Y_R       Y_q       as it stood (R, q)   present (R, q)
    ordinary         0.31 .. 1.3      2.1 .. 19         1.61e-15  2.55e-15  0.62   0.26          0.62   0.26
    thin_current     3e-12 .. 1e-2    3.7e2 .. 1.2e12   9.80e-5   4.15e-5   0.68   0.58          0.68   0.58
    thin_reference   3e-12 .. 1e-2    3.7e2 .. 1.2e12   7.52e-5   3.57e-5   1.56   0.81          1.56   0.81
    both_thin        1e-4 .. 1e-2     4.0e4 .. 4.0e8    2.72e-8   1.18e-8   1.5e-4 3.8e-4        1.5e-4 3.8e-4
    under_threshold  1e-13 .. 5e-13   7.3e12 .. 3.7e13  3.61e-3   2.27e-3   520    491           0.92   0.56
    filter_weights   1e-8 .. 1        3.6 .. 2.4e9      9.85e-8   4.23e-8   0.36   0.38          0.36   0.38
    lopsided         0.31 .. 1.3      1.2e4 .. 5.4e12   4.41e-4   1.87e-4   1.4e-12 3.0e-12      1.4e-12 3.0e-12
    scale            0.31 .. 1.3      2.7 .. 25         1.65e-15  7.86e-16  not finite (10)      0.47   3.53
    near_optimum     0.31 .. 1.3      1.8 .. 31         1.75e-15  2.05e-4   0.45   4.54          0.45   4.54

As it stood the closed form fails exactly under_threshold (all 32 items took the shortest arc: an error of 1.9, 520
Y) and scale (the ten items at 2^+520 and 2^-540 are NaN, those at 2^-520 1e-11); the present one fails none.  Where a
weight is tiny or both pairs are thin the closed form is far better than the SVD, which loses sigma_2's digits."""
import numpy as np
import pytest

from oracle import ekf_numpy as npo

from . import wahba_families as wf
from . import wahba_numpy as wn

NOMINAL = {  # (theta_W, theta_V) of each kind; None: drawn from U(0.3, 1.3)
    "thin_current": lambda k: (1.0, np.pi - 1e-8 if k == "pi-1e-8" else float(k)),
    "thin_reference": lambda k: (np.pi - 1e-8 if k == "pi-1e-8" else float(k), 1.0),
    "both_thin": lambda k: (float(k), float(k)),
    "under_threshold": lambda k: (1.0, float(k[2:])) if k[0] == "V" else (float(k[2:]), 1.0),
    "filter_weights": lambda k: (1.0, float(k.split()[1])),
}
COND = {"ordinary": (1.0, 1e2), "thin_current": (1e2, 1e13), "thin_reference": (1e2, 1e13), "both_thin": (1e4, 1e9),
        "under_threshold": (1e12, 1e14), "filter_weights": (1.0, 1e10), "lopsided": (1e3, 1e13), "scale": (1.0, 1e2),
        "near_optimum": (1.0, 1e2)}
FAILS_AS_IT_STOOD = ["under_threshold", "scale"]


@pytest.fixture(scope="module")
def g():
    return wf.golden()


@pytest.fixture(scope="module")
def batch():
    return wf.side_by_side(wf.families())


@pytest.fixture(scope="module")
def restated(batch, g):
    """{algebra: (err_R, err_q, rank-1 route taken) per item} of the restatement as it stood and as it is"""
    cat, _ = batch
    out = {}
    for key, kw in (("stood", wn.TODAY), ("present", wn.FIXED)):
        R, deg = wn.wahba_rotation_vectors(*[cat[k] for k in wf.FIELDS], **kw)
        out[key] = (wf.err_rotation(R, g["f64_R"]), wf.err_quat(wn.rotm_to_quat(R), g["f64_q"]), deg)
    return out


def test_families(batch, g):
    """Nine families of 32 items, 288 side by side; repeatable; unit vectors but for filter_weights' raw half and
    scale, whose items are ordinary ones times an exact power of two; no pair exactly parallel; the stacked batch
    adds rank1_by_weight's 16 and parallels' 1004 items: 1308, 20 full waves and one of 28 lanes."""
    cat, sl = batch
    assert len(wf.NAMES) == 9 and list(sl) == wf.NAMES and cat["acc"].shape == (288, 3)
    again = wf._family("lopsided", np.random.default_rng([wf.SEED, 7, wf.NAMES.index("lopsided")]))
    assert all(np.array_equal(again[k], wf.families()["lopsided"][k]) for k in wf.FIELDS)
    for name, f in wf.families().items():
        assert [f[k].shape for k in wf.FIELDS] == [(32, 3)] * 4 + [(32,)] * 2 and len(wf.kinds(name)) == 32
        if name not in ("filter_weights", "scale"):
            assert all(np.abs(np.linalg.norm(f[k], axis=1) - 1.0).max() < 1e-15 for k in wf.FIELDS[:4]), name
    assert not g["f64_rank1"].any() and not wf.exactly_parallel(cat).any()
    f = wf.families()["scale"]
    for i, k in enumerate(wf.kinds("scale")):
        which, e = k.split()
        for key in (("acc", "mag") if which == "current" else ("acc0", "mag0")):
            assert abs(np.linalg.norm(np.ldexp(f[key][i], -int(e))) - 1.0) < 1e-15
    fw = wf.families()["filter_weights"]
    raw = np.array([k.startswith("raw") for k in wf.kinds("filter_weights")])
    assert np.abs(np.linalg.norm(fw["acc"][raw], axis=1) - 9.81).max() < 1e-14
    assert np.abs(np.linalg.norm(fw["mag0"][raw], axis=1) - 48.0).max() < 1e-13 and (fw["k_mag"][raw] < 0).sum() >= 12
    assert np.array_equal(fw["k_acc"], np.abs(fw["acc"][:, 2])) and np.array_equal(fw["k_mag"], 1.0 - fw["k_acc"])
    lo = wf.families()["lopsided"]
    assert (lo["k_mag"] < 0).sum() >= 9 and np.abs(lo["k_acc"] + lo["k_mag"] - 1.0).max() < 1e-15
    scat, ssl = wf.stacked()
    assert len(scat["acc"]) == 1308 and ssl["parallels"] == slice(304, 1308) and ssl["rank1_by_weight"] == slice(288, 304)


@pytest.mark.parametrize("name", wf.NAMES)
def test_geometry(batch, g, name):
    """The exact angles of the doubles are the nominal ones (to the 4e-16 that rounding m moves them) and every item's
    sigma_1 / sigma_2 lies in its family's band."""
    _, sl = batch
    th, cond = g["f64_theta"][sl[name]], g["f64_cond"][sl[name]]
    print("%-16s theta_W %.3g .. %.3g, theta_V %.3g .. %.3g, cond %.2e .. %.2e" % (
        name, th[:, 0].min(), th[:, 0].max(), th[:, 1].min(), th[:, 1].max(), cond.min(), cond.max()))
    assert COND[name][0] <= cond.min() and cond.max() <= COND[name][1]
    if name in NOMINAL:
        want = np.array([NOMINAL[name](k) for k in wf.kinds(name)])
        assert np.all(np.abs(th - want) <= 4e-16 + 1e-9 * want), name
    else:
        assert 0.3 <= th[:, 0].min() and th[:, 0].max() <= 1.3


def test_exact_optima_are_rotations_that_beat_the_reference(batch, g):
    """R of the fixture is orthogonal to its rounding, q is unit and is R's quaternion, and tr(R^T B) is no smaller
    than the reference's own rotation attains (away from scale, where B's size is not 1)."""
    cat, sl = batch
    R, q = g["f64_R"], g["f64_q"]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-15 and np.abs(np.linalg.det(R) - 1).max() < 1e-15
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-15 and np.abs(wf.quat_rotm(q) - R).max() < 1e-15
    B = wf.wahba_b(cat)
    keep = np.ones(288, bool)
    keep[sl["scale"]] = False
    gain = np.einsum("nij,nij->n", R - g["f64_R_ref"], B)[keep]
    assert gain.min() > -1e-15 * np.abs(B[keep]).max()


def test_share_of_items_that_pin_the_sign(g):
    """At least 90 % of the items qualify for the sign check (wahba_families.sign_qualifies): every item but the
    near-identity and near-half-turn optima below 1e-2, where a numerator is under 1e-3 by construction."""
    ok = wf.sign_qualifies(g, "f64")
    print("sign: %d of %d items qualify" % (ok.sum(), len(ok)))
    assert ok.mean() >= 0.9
    assert np.array_equal(wf.same_sign(g["f64_q_ref"], g["f64_q"])[ok], np.ones(ok.sum(), bool))


def test_every_family_is_informative(batch, g):
    """8 Y < 0.5 for R and q on every family (the IEEE routes); 303 Y < 0.5 on every family the stream takes, on the
    float64 items and on those rounded to float32, under_threshold with its 5e-13 items alone (~0.2)."""
    _, sl = batch
    for name in wf.NAMES:
        YR, Yq = wf.yard(g, "f64", sl[name])
        print("%-16s Y_R %.3e Y_q %.3e: IEEE bounds %.3g %.3g" % (name, YR, Yq, wf.MARGIN * YR, wf.MARGIN * Yq))
        assert 0.0 < wf.MARGIN * YR < wf.INFORMATIVE and 0.0 < wf.MARGIN * Yq < wf.INFORMATIVE, name
    _, sl32 = wf.side_by_side(wf.families32())
    for which, names, rows in (("f64", wf.STREAM, sl), ("f32", wf.F32, sl32)):
        for name in names:
            Yq = wf.yard(g, which, rows[name], wf.stream_pick(name))[1]
            print("%s %-16s Y_q %.3e: FAST bound %.3g" % (which, name, Yq, wf.FAST_MARGIN * Yq))
            assert wf.FAST_MARGIN * Yq < wf.INFORMATIVE, (which, name)
    assert abs(wf.FAST_MARGIN - 8 * 4.2e-15 / 2.0 ** -53) < 1e-9 and 300 < wf.FAST_MARGIN < 305


def test_float32_items(g):
    """Rounded to float32, every pair meant to be thinner than 1e-6 is either exactly parallel (rank 1: judged by the
    optimum) or some angle of the order of float32's rounding; the rest keep their angles to 1e-6."""
    cat, sl = wf.side_by_side(wf.families32())
    assert np.array_equal(g["f32_rank1"], wf.exactly_parallel(cat)) and g["f32_rank1"].sum() == 23
    for name in ("thin_current", "thin_reference"):
        col = 1 if name == "thin_current" else 0
        for i, k in enumerate(wf.kinds(name)):
            th = g["f32_theta"][sl[name]][i, col]
            if g["f32_rank1"][sl[name]][i]:
                assert k in ("1e-08", "1e-10", "3e-12", "pi-1e-8") and np.isnan(th)
            elif k in ("1e-02", "1e-04", "1e-06"):
                assert abs(th - float(k)) < 2e-7
            else:
                assert 1e-9 < min(th, np.pi - th) < 1e-6
    assert not g["f32_rank1"][sl["ordinary"]].any() and not g["f32_rank1"][sl["both_thin"]].any()


@pytest.mark.parametrize("name", wf.NAMES)
def test_rule_tells_the_algebras_apart(batch, g, restated, name):
    """The present restatement meets 8 Y on every family, R and q; as it stood it fails exactly under_threshold (every
    item on the shortest arc, an O(1) error) and scale (NaN at 2^+520 and 2^-540), and meets the rule elsewhere."""
    _, sl = batch
    s = sl[name]
    YR, Yq = wf.yard(g, "f64", s)
    for key in ("stood", "present"):
        eR, eq, deg = restated[key]
        print("%-16s %-8s R %.3g Y_R, q %.3g Y_q, %d items by the rank-1 route, %d not finite" % (
            name, key, eR[s].max() / YR, eq[s].max() / Yq, deg[s].sum(), np.isinf(eR[s]).sum()))
    eR, eq, deg = restated["present"]
    assert eR[s].max() <= wf.MARGIN * YR and eq[s].max() <= wf.MARGIN * Yq and not deg[s].any()
    eR, eq, deg = restated["stood"]
    if name in FAILS_AS_IT_STOOD:
        assert eR[s].max() > wf.MARGIN * YR and eq[s].max() > wf.MARGIN * Yq
    else:
        assert eR[s].max() <= wf.MARGIN * YR and eq[s].max() <= wf.MARGIN * Yq and not deg[s].any()
    if name == "under_threshold":
        assert deg[s].all() and np.median(eR[s]) > 1.0      # (an arbitrary turn about the parallel direction)
    if name == "scale":
        big = np.array([k in ("current +520", "current -540", "reference +520") for k in wf.kinds(name)])
        assert np.array_equal(np.isinf(eR[s]), big), np.nonzero(np.isinf(eR[s]))


def test_sign_of_the_restatement(g, restated, batch):
    """The present restatement's q carries the reference's sign on every qualifying item."""
    cat, _ = batch
    R, _ = wn.wahba_rotation_vectors(*[cat[k] for k in wf.FIELDS], **wn.FIXED)
    ok = wf.sign_qualifies(g, "f64")
    assert wf.same_sign(wn.rotm_to_quat(R), g["f64_q_ref"])[ok].all()


def test_rank1_groups():
    """parallels(): every item takes the rank-1 route under both thresholds, the present one at its margin (the
    remainder is at most 8 u |m|, a quarter of 2^-48); the rotation is proper to 1e-12 and attains the optimum to 1e-12
    sigma_1 (test_degenerate_samples' criterion).  rank1_by_weight(): healthy frames, so the closed form itself, and
    the same criterion.  In float32 the current-pair parallels are exactly parallel too."""
    par = wf.parallels()
    assert len(par["acc"]) == 1004 and par["current"].sum() == 503
    for kw in (wn.TODAY, wn.FIXED):
        R, deg = wn.wahba_rotation_vectors(*[par[k] for k in wf.FIELDS], **kw)
        orth, short = wf.optimum_shortfall(R, par)
        assert deg.all() and orth.max() < 1e-12 and np.abs(short).max() < 1e-12
    with np.errstate(all="ignore"):
        for a, m in ((par["acc"][par["current"]], par["mag"][par["current"]]), (par["acc0"][~par["current"]], par["mag0"][~par["current"]])):
            F = wn.make_frame(a, m)
            noise = np.abs(F["beta2"]) / np.hypot(F["beta1"], F["beta2"])
            assert np.nanmax(noise) <= 8 * wf.U and 8 * wf.U * 4 == wn.THRESHOLD
    by = wf.rank1_by_weight()
    assert np.array_equal(by["k_acc"] == 0.0, by["k_mag"] == 1.0) and (by["k_acc"] == 0.0).sum() == 8
    R, deg = wn.wahba_rotation_vectors(*[by[k] for k in wf.FIELDS], **wn.FIXED)
    orth, short = wf.optimum_shortfall(R, by)
    assert not deg.any() and orth.max() < 1e-12 and np.abs(short).max() < 1e-12
    assert np.linalg.matrix_rank(wf.wahba_b(by), tol=1e-12).max() == 1


def test_overflow_group_is_the_references_failure():
    """Both pairs times 2^520: B is not finite and np.linalg.svd raises, which the operators report as status 1."""
    f = wf.overflow()
    for i in range(4):
        with np.errstate(all="ignore"):
            assert not np.isfinite(wf.wahba_b(f, i)).any()
            with pytest.raises(np.linalg.LinAlgError):
                npo.svd_rotation(*[f[k][i] for k in wf.FIELDS])


@pytest.mark.parametrize("name", ["near_identity", "near_half_turn"])
def test_matrix_families(g, name):
    """R -> q alone on the float64 matrix as given: the yardstick is the reference formula's float64 error against the
    same formula at 80 digits (1.6e-4 near the identity at phi = 1e-6, 1e-16 near a half turn); the restated selects
    give the reference's q bit for bit."""
    M = wf.matrices()[name]
    Y = g["mat_%s_err" % name].max()
    print("%-14s Y_q %.3e" % (name, Y))
    assert 0.0 < wf.MARGIN * Y < wf.INFORMATIVE
    ref = np.array([npo.rotm_to_quat(m) for m in M])
    assert np.array_equal(wn.rotm_to_quat(M), ref)
    assert wf.err_quat(ref, g["mat_%s_q" % name]).max() <= Y * (1 + 1e-12) + 2e-16
