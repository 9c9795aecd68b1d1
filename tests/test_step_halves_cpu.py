"""The items of tests/step_families.py without a GPU: what the families are, the yardsticks of
tests/golden/step_families.npz -- the error Y of the reference's own float64 statements (oracle.ekf_numpy.rk4 chained,
wahba_quat) against results exact to 80 digits -- so that the conditions of tests/test_step_halves.py rest on the
reference and not on the code under test; and the rule shown to have teeth on NumPy restatements of the device's two
halves (tests/step_numpy.py; no fma contraction and an exact 1 / sqrt, so the device's figures differ).

The rule.  Propagation: max |X - X_exact| of a family <= 303 Y u on the fused routes (FAST_MARGIN = 8 x 4.2e-15 / u, the
rsqrt's class), Y the reference's worst error over the family in units of u = 2^-53, floored at 1.  Measurement: the
sign-insensitive max |X -+ q_exact| <= 303 Y_q.

Measured here (the restatements' worst error as a ratio to the yardstick; "f32" set for the propagation, "f64" for the
measurement):

    propagation  Y (f64, f32)  plain  loop   as it stood (snap 1e-13)   fault that must fail here
    ordinary     1.20  1.31    3.8    1.5    3.8
    tiny         1.28  1.28    1.6    1.2    1.6                        identity under xx < 1e-16: 5.6e7
    roots        13.8  15.7    0.92   0.92   0.92
    huge         3.51  2.83    0.71   0.71   0.71
    longdt       6.47  5.38    2.2    2.4    2.2                        escaped dt through float32: 3.6e8
    back         2.54  2.48    1.6    1.0    1.6                        the same: 2.7e8
    offunit      1.81  1.27    80     1.6    316 (> 303)                |X|^2 = 1 whatever X: 6.6e27
    sparse       0.97  1.27    3.1    0.78   3.1
    chain        13.4  18.3    2.6    0.44   2.6

    measurement     Y_q       present   fault that must fail here
    ordinary        2.04e-15  0.18
    thin_current    7.78e-5   9.4e-3    a pair called parallel under 1e-11 |m|: 1.1e4
    thin_reference  4.87e-5   0.46      the same: 2.5e4
    flat            8.35e-5   4.0e-12
    upright         4.32e-10  7.7e-7
    raw_units       1.08e-14  0.028
    normal_near_z   2.90e-8   8.6e-9    arc 1 without its second form: 2.7e7
    quarter_turn    6.24e-15  0.14      q_theta without its second form: 3.3e6
    near_optimum    4.72e-4   4.7e-13
    mag_scale       2.51e-15  0.11

Three findings about the conditions themselves.
 - Y of roots and chain is above MARGIN = 8, as it has to be: at theta^2 = 6 the reference's stage sum cancels from
   terms of 1, 3 and 1.5 to |q1| = 1/2, an amplification of 11, and 64 records of ~1.3 u each walk to ~10 u, the worst of
   sixteen chains twice that.  They are held to [1, 3 MARGIN); every other family to [1, MARGIN).
 - q_theta's first form alone does not fail beside C = 0, where both forms are sound (the select is where they are
   equally good); it cancels at C = -H.  quarter_turn therefore carries half-turn kinds too, and fails on those.
 - The thinnest pair is 3e-12 rad, above a threshold of 1e-12 |m|, which therefore calls no item parallel; the fault is
   shown at 1e-11 |m|.
With the snap at 1e-13 the restatement of the one-record routes misses the bound on the |X|^2 - 1 = -9e-14 kind of the
f32 set: 4.5e-14 = 405 u, which is 316 Y u at that set's Y = 1.27, against 303 Y u (the f64 set, Y = 1.81, passes at
224 Y u).  state_norm2 snaps at 2.9e-14; test_snap_is_the_headers ties step_families.SNAP to the header's kNormSnap."""
from fractions import Fraction

import numpy as np
import pytest

from . import step_families as sf
from . import step_numpy as sn
from . import wahba_families as wf
from .test_wahba_two_arc_cpu import arc1_terms, pair_in_own_frame, two_arc

WIDE_Y = ("roots", "chain")     # see the docstring
PROP_FAULTS = {"shortcut": ["tiny"], "dt32": ["longdt", "back"], "n2_one": ["offunit"]}
MEAS_FAULTS = {"arc1": (dict(arc1_second=False), ["normal_near_z"]), "theta": (dict(theta_second=False), ["quarter_turn"]),
               "parallel": (dict(parallel=1e-11), ["thin_current", "thin_reference"])}


@pytest.fixture(scope="module")
def g():
    return sf.golden()


def _prop_ratio(g, form, X):
    cat, sl = sf.prop_side_by_side(sf.prop_families(form))
    e = sf.err_state(X, g["p_%s_X" % form])
    return {n: e[s].max() / (sf.prop_yard(g, form, s) * sf.U) for n, s in sl.items()}


def _meas_ratio(g, form, q):
    cat, sl = sf.meas_side_by_side(sf.meas_families(form))
    e = wf.err_quat(q, g["m_%s_q" % form])
    return {n: e[s].max() / sf.meas_yard(g, form, s) for n, s in sl.items()}


def test_propagation_families():
    """Nine families of 32 items in both sets, repeatable; the f32 set holds float32 samples and whole dts, escaped
    exactly on longdt and back; the kinds are what their labels say (theta^2 at the roots to 1e-8 in both sets,
    |X0|^2 - 1 of offunit to 5e-16 in exact arithmetic)."""
    for form in ("f64", "f32"):
        fam = sf.prop_families(form)
        assert list(fam) == sf.PROP and len(sf.PROP) == 9
        again = sf._prop_family("roots", np.random.default_rng([sf.SEED, 1, sf.PROP.index("roots")]), form)
        assert all(np.array_equal(again[k], fam["roots"][k]) for k in again)
        for name, f in fam.items():
            L = sf.CHAIN if name == "chain" else 3
            assert f["X0"].shape == (32, 4) and f["gyro"].shape == (32, L, 3) and f["dt"].shape == (32, L), name
            assert len(sf.prop_kinds(name)) == 32 and f["n"].min() >= 1 and f["n"].max() == L
            if name != "chain":
                assert set(f["n"]) == {1, 2, 3}
            esc = (f["dt"] < 0) | (f["dt"] > sf.DT_WORD_MAX)
            assert esc.all() == (name in ("longdt", "back")) and esc.any() == (name in ("longdt", "back")), name
            if form == "f32":
                assert np.array_equal(sf._r32(f["gyro"]), f["gyro"]) and np.array_equal(np.rint(f["dt"]), f["dt"])
        th2 = (fam["roots"]["dt"] * sf.NS * np.linalg.norm(fam["roots"]["gyro"], axis=-1) / 2) ** 2
        want = np.array([sf.ROOTS[j // 4] * (1 + sf.ROOT_EPS[j % 4]) for j in np.arange(32) % 12])[:, None]
        assert np.abs(th2 / want - 1).max() < 1e-8
        assert fam["huge"]["dt"].max() == sf.DT_WORD_MAX and np.linalg.norm(fam["huge"]["gyro"], axis=-1).max() > 9e5
        assert np.linalg.norm(fam["tiny"]["gyro"], axis=-1).min() < 2e-24
        assert fam["longdt"]["dt"].max() > 2.0 ** 44 and fam["back"]["dt"].min() < -1.9e10
        for k, x in zip(sf.prop_kinds("offunit"), fam["offunit"]["X0"]):
            n2 = sum(Fraction(float(v)) ** 2 for v in x)
            if k.startswith("n2-1"):
                d = float(n2 - 1)
                assert abs(d - float(k.split()[1])) < 5e-16
                assert (abs(d) < sf.SNAP) == (abs(d) < 5e-14) and (abs(d) < sf.SNAP_STOOD) == (abs(d) < 1e-13)
            else:
                assert abs(float(n2) ** 0.5 / float(k.split()[1]) - 1) < 1e-2
        sp = fam["sparse"]
        assert ((sp["gyro"] != 0).sum(-1) == 1).all() and ((sp["X0"] != 0).sum(-1) <= 2).all()
        assert ((sp["X0"] != 0).sum(-1) == 2).sum() == 16
        # 64 huge records: the covariance grows by |w|^2 / 4 a record and stays finite
        ch = np.linalg.norm(fam["chain"]["gyro"], axis=-1)
        assert (np.log10(ch * ch / 4).sum(1) < 300).all() and ch.max() > 50
    ap = sf.prop_apart()
    assert len(sf.PROP_APART) == 7 and np.isfinite(ap["gyro"][:sf.PROP_APART_FINITE]).all()
    assert np.array_equal(sf._r32(ap["gyro"]), ap["gyro"], equal_nan=True)


def test_measurement_families(g):
    """Ten families (nine in f32), the filter's own weights; no pair exactly parallel in either set; n and (C, S) are
    where normal_near_z and quarter_turn say; raw_units has k_mag < 0 for most; and at least 90 % of the items have
    |q . z| >= 0.2, where the sign is asked."""
    for form, names in (("f64", sf.MEAS), ("f32", sf.MEAS32)):
        fam = sf.meas_families(form)
        cat, sl = sf.meas_side_by_side(fam)
        assert list(fam) == names and not wf.exactly_parallel(cat).any()
        assert np.array_equal(cat["k_acc"], np.abs(cat["acc"][:, 2])) and np.array_equal(cat["k_mag"], 1 - cat["k_acc"])
        assert np.abs(np.linalg.norm(cat["X0"], axis=1) - 1).max() < 1e-15
        if form == "f32":
            assert all(np.array_equal(sf._r32(cat[k]), cat[k]) for k in sf.MFIELDS)
        assert (fam["raw_units"]["k_mag"] < 0).sum() >= 20
        f = fam["normal_near_z"]
        n, N, _ = arc1_terms(f["acc"], f["mag"])
        for k, nz, nn in zip(sf.meas_kinds("normal_near_z"), n[:, 2], N):
            off = np.arccos(min(1.0, abs(nz) / nn)) if float(k.split()[1]) > 1e-7 or form == "f64" else 0.0
            assert (nz > 0) == (k[0] == "+")
            if float(k.split()[1]) >= 1e-4:
                assert abs(off / float(k.split()[1]) - 1) < 1e-2, k
        f = fam["quarter_turn"]
        aW, b1W, b2W, _ = pair_in_own_frame(f["acc0"], f["mag0"])
        _, C, S = two_arc(f["acc"], f["mag"], aW, b1W, b2W, want_cs=True)
        for k, c, s in zip(sf.meas_kinds("quarter_turn", form), C / np.hypot(C, S), S):
            assert (s > 0) == k.endswith("+"), k
            if k.startswith("C"):
                e = float(k.split()[1])
                assert abs(c - e) < 2e-7 + 1e-3 * abs(e), (k, c)
            else:
                assert c < -0.9999
        qz = g["m_%s_qz" % form]
        print("%s: |q.z| >= 0.2 on %d of %d items" % (form, (qz >= sf.SIGN_QZ).sum(), len(qz)))
        assert (qz >= sf.SIGN_QZ).mean() >= 0.9 and (qz < 0.25).sum() >= 2 * len(names)
    assert "mag_scale" not in sf.MEAS32 and len(sf.MEAS) == 10
    ap = sf.meas_apart()
    assert np.linalg.matrix_rank(wf.wahba_b(ap), tol=1e-12).max() == 1 and len(sf.MEAS_APART) == 4


def test_yardsticks_are_the_references_own_error(g):
    """Propagation: 1 <= Y < MARGIN on every family but roots and chain, which stay under 3 MARGIN (the docstring says
    why); measurement: MARGIN Y_q < INFORMATIVE.  The exact states are unit, the exact q is unit, and the apart items'
    exact X is X0 itself."""
    for form in ("f64", "f32"):
        _, sl = sf.prop_side_by_side(sf.prop_families(form))
        for name, s in sl.items():
            Y = float(g["p_%s_err" % form][s].max()) / sf.U
            print("%s propagation %-9s Y %.3g u" % (form, name, Y))
            assert 0.9 <= Y and 1.0 <= sf.prop_yard(g, form, s) < (3 if name in WIDE_Y else 1) * sf.MARGIN, name
        assert np.abs(np.linalg.norm(g["p_%s_X" % form], axis=1) - 1).max() < 1e-15
        _, sl = sf.meas_side_by_side(sf.meas_families(form))
        for name, s in sl.items():
            Yq = sf.meas_yard(g, form, s)
            print("%s measurement %-15s Y_q %.3e: bounds %.3g, %.3g" % (form, name, Yq, sf.MARGIN * Yq, sf.FAST_MARGIN * Yq))
            assert 0.0 < sf.MARGIN * Yq < sf.INFORMATIVE, name
        assert np.abs(np.linalg.norm(g["m_%s_q" % form], axis=1) - 1).max() < 1e-15
    ap = sf.prop_apart()
    k = sf.PROP_APART_FINITE
    assert np.array_equal(g["p_apart_X"][:k], ap["X0"][:k]) and np.isnan(g["p_apart_X"][k:]).all()


@pytest.mark.parametrize("form", ["f64", "f32"])
def test_restated_device_meets_the_rule(g, form):
    """rk4_closed chained as the one-record routes chain it (state_norm2 every record), as the multi-record loop does
    (the first record alone, X normalised at the end) and as k_gyro_chain does (no snap), and the two-arc product:
    within 303 Y on every family of both sets."""
    cat, _ = sf.prop_side_by_side(sf.prop_families(form))
    for key, kw in (("plain", {}), ("loop", dict(form="loop")), ("no snap", dict(snap=0.0))):
        r = _prop_ratio(g, form, sn.chain(cat, **kw))
        print(form, key, " ".join("%s %.3g" % kv for kv in r.items()))
        assert max(r.values()) <= sf.FAST_MARGIN, (key, r)
    mcat, _ = sf.meas_side_by_side(sf.meas_families(form))
    r = _meas_ratio(g, form, sn.fused_quat(mcat))
    print(form, "two-arc", " ".join("%s %.3g" % kv for kv in r.items()))
    assert max(r.values()) <= sf.FAST_MARGIN, r


@pytest.mark.parametrize("fault", list(PROP_FAULTS))
def test_rule_catches_a_wrong_propagation(g, fault):
    """Each fault misses the bound on its families and on no other (f32 set: the one with escaped dts)."""
    cat, _ = sf.prop_side_by_side(sf.prop_families("f32"))
    r = _prop_ratio(g, "f32", sn.chain(cat, **{fault: True}))
    print(fault, " ".join("%s %.3g" % kv for kv in r.items()))
    assert [n for n in sf.PROP if r[n] > sf.FAST_MARGIN] == PROP_FAULTS[fault]


@pytest.mark.parametrize("fault", list(MEAS_FAULTS))
def test_rule_catches_a_wrong_measurement(g, fault):
    kw, fails = MEAS_FAULTS[fault]
    mcat, _ = sf.meas_side_by_side(sf.meas_families("f64"))
    r = _meas_ratio(g, "f64", sn.fused_quat(mcat, **kw))
    print(fault, " ".join("%s %.3g" % kv for kv in r.items()))
    assert [n for n in sf.MEAS if r[n] > sf.FAST_MARGIN] == fails
    if fault == "parallel":     # 1e-12 |m| is under the thinnest pair: it calls nothing parallel
        same = sn.fused_quat(mcat, parallel=1e-12)
        assert np.array_equal(same, sn.fused_quat(mcat))


def test_snap_as_it_stood_misses_the_bound(g):
    """state_norm2 at 1e-13: the one-record routes store z normalised by the snapped |X|^2, 4.5e-14 off on the
    |X|^2 - 1 = -9e-14 kind, above 303 Y u; at 2.9e-14 the worst is the 2.8e-14 kinds' 1.4e-14.  The multi-record loop
    normalises at the launch's end and never showed it."""
    for form in ("f64", "f32"):
        cat, sl = sf.prop_side_by_side(sf.prop_families(form))
        stood = _prop_ratio(g, form, sn.chain(cat, snap=sf.SNAP_STOOD))
        now = _prop_ratio(g, form, sn.chain(cat))
        loop = _prop_ratio(g, form, sn.chain(cat, form="loop", snap=sf.SNAP_STOOD))
        print("%s offunit: stood %.3g, present %.3g, loop %.3g (x Y u)" % (form, stood["offunit"], now["offunit"], loop["offunit"]))
        assert now["offunit"] <= sf.FAST_MARGIN / 2 and loop["offunit"] <= sf.MARGIN
        e = sf.err_state(sn.chain(cat, snap=sf.SNAP_STOOD), g["p_%s_X" % form])[sl["offunit"]]
        worst = sf.prop_kinds("offunit")[int(e.argmax())]
        assert worst.startswith("n2-1") and "9.0e-14" in worst and 4.0e-14 < e.max() < 5.0e-14
    assert stood["offunit"] > sf.FAST_MARGIN    # (f32 set: Y = 1.27)


def test_snap_is_the_headers():
    """step_families.SNAP, which the restatement and the offunit kinds' labels go by, is state_norm2's kNormSnap as
    csrc/pekf_step.hpp states it."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "poseestimationkf_amd", "csrc", "pekf_step.hpp")
    with open(path) as fh:
        m = re.search(r"constexpr double kNormSnap = ([0-9.eE+-]+);", fh.read())
    assert m and float(m.group(1)) == sf.SNAP
