"""The front-end families of tests/frontend_families.py without a GPU: what the families are -- their kinds, slots and
channels, the judged channel's kappa, the error Y of the reference's own float64 statement
(oracle.frontend_numpy.run_frontend, held bit for bit to the compiled Parser.cpp by tests/test_parser_golden.py)
against the exact chain of tests/golden/frontend_families.npz -- so that the conditions of
tests/test_frontend_conditioning.py rest on the reference and not on the code under test; and the rule shown to have
teeth on a NumPy restatement of the device's two algebras (tests/phase3_numpy.py).

The rule, per family: max over its items of |out - exact|_max / (kappa U) on the last record's judged channel is at
most FAST_MARGIN Y ~ 303 Y, Y the reference statement's own largest such ratio on the family (at least 1); an item is
asserted only where FAST_MARGIN Y kappa U < INFORMATIVE.  Every other stored value (the other channel, the earlier
records) is held to the same bound with its own kappa.

Measured (32 items a family; the restated device algebras' worst ratio in units of Y, FP64 / f32 event form on the
float64 / float32 items, with exact seeds, so without the device's rsqrt error):

    family       kappa (f64 items)   Y (f64, f32 items)   restated device
    ordinary     1.0 .. 1.08         1.20  1.17           1.07  1.39
    extrapolate  1.0 .. 1.8          1.04  1.00           0.98  1.31
    cancel       2e2 .. 2e8          1.00  1.00           0.56  0.82
    clock_back   1.0 .. 1.17         1.19  1.00           1.15  1.21
    one_ns       1.0 .. 1.83         1.00  1.00           1.13  1.42
    long_pause   1.0 .. 1.59         1.46  1.09           0.79  1.35
    scale        1.0 .. 1.09         1.05  1.00           1.26  1.15
    mixed_scale  1.0 .. 11.8         1.00  1.09           1.24  0.86
    lowpass      1.05 .. 1.07        5.16  5.34           1.18  1.00

The largest bound an item is asserted under is cancel's at kappa 2e8: 303 x 2e8 x 2^-53 = 6.7e-6.  The mutations on
the families named for them: a dropped sign 1.3e15 and more (bound ~303), a zero for the mean 1.8e11 (lowpass) to
1.8e16, a seed left in rsqrt 4.7e8 to 5.0e8, in recip 1.7e7 and 7.9e7."""
import numpy as np
import pytest

from oracle import frontend_numpy as fe

from . import frontend_families as ff
from . import phase3_numpy as p3

SETS = ("f64", "f32")
MUTATIONS = {"sign": ("clock_back", "one_ns"), "mean": tuple(ff.NAMES), "rsqrt_seed": ("ordinary", "scale", "lowpass"),
             "recip_seed": ("ordinary", "long_pause")}      # the families named to catch each


@pytest.fixture(scope="module")
def g():
    return ff.golden()


def _reference(item):
    _, _, a, m = fe.run_frontend(item["types"], item["values"], item["times"], item["init_acc"], item["init_mag"],
                                 item["t_init"], item["alpha"])
    return np.stack([a, m], axis=1)


def _ratios(g, which, outputs):
    """outputs: per item (R, 2, 3) -> (rho per item on the last record's judged channel, the worst ratio of every
    other stored value to its own kappa U per item); NaN rho for the items judged apart"""
    items, sl = ff.stacked(which)
    rho, rest = np.full(len(items), np.nan), np.zeros(len(items))
    for i, (it, out) in enumerate(zip(items, outputs)):
        rows, recs = ff.rows_of(g, which, i)
        err = ff.error(out[recs], g, which, rows).max(axis=2)              # (rows, 2)
        with np.errstate(invalid="ignore"):
            each = err / (g[which + "_kappa_row"][rows].astype(np.float64) * ff.U)
        if i < sl["apart"].start:
            rho[i] = err[-1, it["ch"]] / (g[which + "_kappa"][i] * ff.U)
        rest[i] = np.nanmax(each)
    return rho, rest


def _family_ratio(g, which, rho, name):
    sl = ff.stacked(which)[1][name]
    return float(np.max(np.where(np.isfinite(rho[sl]), rho[sl], np.inf)))


def test_families(g):
    """Nine families of 32 items in the given order, none dropped; repeatable; every kind of a family meets at least
    two slot kinds and both channels wherever it has two items; times within the FP64 events' 2^51 ns; the float32 set
    leaves out exactly scale's 1e-80 and 1e80 items; the list judged apart is fixed at eight."""
    fam = ff.families()
    assert list(fam) == ff.NAMES and ff.NAMES[:2] == ["ordinary", "extrapolate"] and len(ff.NAMES) == 9
    assert set(ff.NAMES) >= {"ordinary", "extrapolate", "cancel", "clock_back", "one_ns", "long_pause", "scale", "mixed_scale", "lowpass"}
    again = ff._family("cancel", np.random.default_rng([ff.SEED, 13, ff.NAMES.index("cancel")]))
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(again, fam["cancel"]) for k in ("types", "values", "times", "init_acc"))
    for name, items in fam.items():
        ks, ss = ff.kinds(name), ff.slots(name)
        assert len(items) == ff.ITEMS == len(ks) == len(ss)
        for k in set(ks):
            mine = [i for i in range(ff.ITEMS) if ks[i] == k]
            if len(mine) > 1:
                assert len({ss[i] for i in mine}) >= 2 and len({items[i]["ch"] for i in mine}) == 2, (name, k)
        assert {s for s in ss} == set(ff.SLOTS)
        for it, s in zip(items, ss):
            n = len(ff.tuples(it))
            assert it["alpha"] == (1.0 if name != "lowpass" else it["alpha"]) and np.abs(it["times"]).max() < ff.T_LIMIT
            assert n == (ff.LOWPASS_RECORDS + (s == "second") if name == "lowpass" else 1 + (s == "second"))
    assert sorted({it["alpha"] for it in fam["lowpass"]}) == [1e-3, 1e-2, 0.1]
    assert [len(v) for v in ff.families32().values()] == [32] * 6 + [32 - 8, 32, 32] and ff.in_f32("scale").sum() == 24
    assert len(ff.apart()) == len(ff.APART) == 8
    for which, n in (("f64", 296), ("f32", 288)):
        items, sl = ff.stacked(which)
        assert len(items) == n == len(g[which + "_count"]) and sl["apart"] == slice(n - 8, n)
        assert np.array_equal(g[which + "_count"], [len(ff.tuples(it)) for it in items])


def test_geometry(g):
    """The exact kappa of the doubles is what each family was built for: near 1 where the family is well conditioned,
    2 / eps on cancel's float64 items; clock_back's denominators are negative, one_ns's are +-1 ns with numerators up
    to 1e9, long_pause's lie in 2^31 .. 2^45 ns, scale's samples span 1e-80 .. 1e80."""
    items, sl = ff.stacked("f64")
    k = g["f64_kappa"]
    for name, hi in (("ordinary", 1.2), ("extrapolate", 2.0), ("clock_back", 1.3), ("one_ns", 2.0), ("long_pause", 2.0), ("scale", 1.2),
                     ("mixed_scale", 20.0), ("lowpass", 1.2)):
        assert 1.0 <= k[sl[name]].min() and k[sl[name]].max() <= hi, name
    eps = np.array([float(c.split()[0]) for c in ff.kinds("cancel")])
    assert np.all(np.abs(k[sl["cancel"]] * eps / 2.0 - 1.0) < 0.02)
    last = lambda it: ff.tuples(it)[-1][2 + it["ch"]]
    den = lambda name: np.array([last(it)[1] - last(it)[0] for it in items[sl[name]]])
    num = lambda name: np.array([last(it)[2] - last(it)[0] for it in items[sl[name]]])
    assert (den("clock_back") < 0).all() and {"below", "between", "above"} == set(ff.kinds("clock_back"))
    lam = num("clock_back") / den("clock_back")
    assert (lam > 1).sum() >= 10 and (lam < 0).sum() >= 10 and ((lam > 0) & (lam < 1)).sum() >= 10
    assert set(den("one_ns")) == {1, -1} and np.abs(num("one_ns")).max() == 10 ** 9
    assert den("long_pause").min() >= 2 ** 31 and den("long_pause").max() <= 2 ** 45
    assert max(it["times"].max() for it in items[sl["long_pause"]]) > ff.T_LIMIT - 2 ** 47
    lam = np.abs(num("extrapolate") / den("extrapolate"))
    assert lam.min() == 1e2 and lam.max() == 1e8
    mags = np.array([np.abs(last(it)[4]).max() for it in items[sl["scale"]]])
    assert mags.min() < 1e-79 and mags.max() > 1e79
    mix = [(np.linalg.norm(last(it)[3]), np.linalg.norm(last(it)[4])) for it in items[sl["mixed_scale"]]]
    assert {(round(np.log10(a)), round(np.log10(b))) for a, b in mix} == {(-30, 30), (30, -30)}


def test_tuples_are_the_ones_the_reference_interpolates():
    """The tuples the exact chain was given, put through the reference's _interp and _normalise, are fe.records bit
    for bit -- gyro, gyro time, acc, mag of every record of every item of both sets, NaN for NaN."""
    for which in SETS:
        for it in ff.stacked(which)[0]:
            theirs = list(fe.records(it["types"], it["values"], it["times"], it["init_acc"], it["init_mag"], it["t_init"]))
            mine = ff.tuples(it)
            assert len(theirs) == len(mine) > 0
            for (g1, t1, a1, m1), (g2, t2, ta, tm) in zip(theirs, mine):
                assert list(g1) == list(g2) and t1 == t2
                for want, (p, q, r, y1, y2) in ((a1, ta), (m1, tm)):
                    got = fe._normalise(fe._interp(p, q, r, list(map(float, y1)), list(map(float, y2))))
                    assert np.array_equal(np.array(got).view(np.uint64), np.array(want, np.float64).view(np.uint64))


@pytest.mark.parametrize("which", SETS)
def test_the_restatements_y_is_the_fixtures(g, which):
    """run_frontend's error against the stored exact chain, taken here in float64 from the double and its residual, is
    the fixture's rho per item (to the residual's float32: 1e-6) and its Y per family; Y is at least 1 and below 8."""
    items, sl = ff.stacked(which)
    rho, rest = _ratios(g, which, [_reference(it) for it in items])
    fam = slice(0, sl["apart"].start)
    assert np.allclose(rho[fam], g[which + "_rho"][fam], rtol=1e-5, atol=1e-6)
    for j, name in enumerate(ff.NAMES):
        Y = g[which + "_Y"][j]
        print("%s %-12s kappa %.3g .. %.3g  Y %.3g  every other value %.3g" % (
            which, name, g[which + "_kappa"][sl[name]].min(), g[which + "_kappa"][sl[name]].max(), Y, rest[sl[name]].max()))
        assert 1.0 <= Y < ff.MARGIN and abs(max(1.0, rho[sl[name]].max()) - Y) <= 1e-5 * Y
        assert rest[sl[name]].max() <= ff.MARGIN * Y          # (the statement itself, on every other stored value)
    assert np.isnan(g[which + "_rho"][sl["apart"]]).all() and not g[which + "_nan"][g[which + "_row_item"] < sl["apart"].start].any()


@pytest.mark.parametrize("which", SETS)
def test_every_item_is_asserted_under_an_informative_bound(g, which):
    """FAST_MARGIN Y kappa U < INFORMATIVE for every item of every family: none is skipped, and what is not asserted
    is the fixed list judged apart.  The largest bound is cancel's, 6.7e-6 at kappa 2e8."""
    items, sl = ff.stacked(which)
    worst = 0.0
    for j, name in enumerate(ff.NAMES):
        bound = ff.FAST_MARGIN * g[which + "_Y"][j] * g[which + "_kappa"][sl[name]] * ff.U
        assert np.isfinite(bound).all() and (bound < ff.INFORMATIVE).all(), name
        rows = np.isin(g[which + "_row_item"], np.arange(sl[name].start, sl[name].stop))
        every = ff.FAST_MARGIN * g[which + "_Y"][j] * g[which + "_kappa_row"][rows].astype(np.float64) * ff.U
        assert np.isfinite(every).all() and (every < ff.INFORMATIVE).all(), name
        worst = max(worst, bound.max(), every.max())
    print("%s: the largest asserted bound %.3g" % (which, worst))
    assert worst < 1e-5 and sl["apart"].stop == len(items) and sl["apart"].start == sum(len(v) for v in (ff.families() if which == "f64" else ff.families32()).values())
    assert abs(ff.FAST_MARGIN - ff.MARGIN * ff.RSQRT / ff.U) < 1e-9 and 300 < ff.FAST_MARGIN < 305


@pytest.fixture(scope="module")
def restated(g):
    """{(set, mutation): rho per item, rest per item} of the restated device algebra of that set's event form"""
    out = {}
    for which in SETS:
        items, _ = ff.stacked(which)
        tups = [ff.tuples(it) for it in items]
        for mut in (None,) + tuple(MUTATIONS):
            if mut == "recip_seed" and which == "f64":
                continue                          # (lerp_scaled takes no reciprocal)
            out[which, mut] = _ratios(g, which, [p3.records(it, t, which, mut) for it, t in zip(items, tups)])
    return out


@pytest.mark.parametrize("which", SETS)
def test_the_rule_passes_the_restated_device(g, restated, which):
    """Unmutated, both algebras meet FAST_MARGIN Y on every family, on the judged value and on every other one."""
    _, sl = ff.stacked(which)
    rho, rest = restated[which, None]
    for j, name in enumerate(ff.NAMES):
        r = _family_ratio(g, which, rho, name)
        print("%s %-12s restated device %.3g Y (every other value %.3g)" % (which, name, r / g[which + "_Y"][j], rest[sl[name]].max()))
        assert r <= ff.FAST_MARGIN * g[which + "_Y"][j] and rest[sl[name]].max() <= ff.FAST_MARGIN * g[which + "_Y"][j], name


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_the_rule_has_teeth(g, restated, mut):
    """Each mutation fails every family named for it, in every event form that has the mutated operation: a dropped
    sign for den < 0 fails clock_back and one_ns; a mean not selected fails every family (a third of each is "mean"
    or "second" slots); a seed without its Newton step fails the well-conditioned families by a factor of 1e2 or more."""
    for which in SETS:
        if (which, mut) not in restated:
            continue
        rho, _ = restated[which, mut]
        for name in MUTATIONS[mut]:
            j = ff.NAMES.index(name)
            r = _family_ratio(g, which, rho, name)
            print("%s %-10s %-12s %.3g (bound %.3g)" % (which, mut, name, r, ff.FAST_MARGIN * g[which + "_Y"][j]))
            assert r > ff.FAST_MARGIN * g[which + "_Y"][j], (which, mut, name)


@pytest.mark.parametrize("which", SETS)
def test_the_list_judged_apart(g, which):
    """The reference on the fixed list: the first record's judged channel is NaN in every component -- for an infinite
    newer sample in that component alone, 0 in the others -- every later record of that channel is NaN wherever the one
    before was, and the other channel is finite; the stored NaN pattern is the reference's.  The restated device gives
    that pattern and keeps the other channel within the ordinary family's bound; with rsqrt as it stood (the Newton
    residual inf * 0 at a sum of squares of +inf) the two infinite newer samples come out NaN in all three."""
    items, sl = ff.stacked(which)
    Y = g[which + "_Y"][0]
    differ = []
    for i in range(sl["apart"].start, sl["apart"].stop):
        it, label = items[i], ff.APART[i - sl["apart"].start]
        ref = _reference(it)
        rows, recs = ff.rows_of(g, which, i)
        nan = np.isnan(ref)
        assert len(ref) == 3 and np.array_equal(recs, [0, 1, 2]) and np.array_equal(nan, g[which + "_nan"][rows]), label
        ch = it["ch"]
        assert not nan[:, 1 - ch].any() and nan[:, ch].any(axis=1).all() and (nan[1:, ch] >= nan[:-1, ch]).all(), label
        assert nan[0, ch].sum() == (1 if "inf in" in label and "newer" in label else 3), label
        assert np.array_equal(ref[0, ch][~nan[0, ch]], np.zeros(3)[~nan[0, ch]]), label
        for stood in (False, True):
            out = p3.records(it, ff.tuples(it), which, stood=stood)
            err = ff.error(out, g, which, rows)[:, 1 - ch].max(axis=1)
            assert (err <= ff.FAST_MARGIN * Y * g[which + "_kappa_row"][rows, 1 - ch] * ff.U).all(), label
            if stood:
                if not np.array_equal(np.isnan(out), nan):
                    differ.append(label)
            else:
                assert np.array_equal(np.isnan(out), nan), label
    assert differ == ["+inf in acc's newer sample", "-inf in mag's newer sample"]
