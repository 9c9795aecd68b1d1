"""The phase-3 front-end on the device (csrc/pekf_phase3.hpp lerp_scaled, lpf_record, normalised, normalised_fma,
rsqrt_sumsq, recip; behind k_frontend, k_live and every chunked session) against exact chains across interpolation
geometry, clock behaviour and sample scale: the families of tests/frontend_families.py -- gyro times up to 1e8 gaps
outside their pair, interpolants that cancel to 1e-8, clocks stepping back, 1 ns denominators under 1 s numerators,
pauses of 2^45 ns at times near 2^51, samples from 1e-80 to 1e80, alpha = 1 so that nothing is scaled away -- where
synth.generate_events (gravity-sized vectors, regular gaps, the gyro inside its pair, alpha = 0.1) and parser.npz's
handful of time edges cannot see an error.  The conditions (the exact chain of tests/golden/frontend_families.npz, the
error Y of the reference's own float64 statement against it, the device held to FAST_MARGIN Y kappa U ~ 303 Y kappa
2^-53, for f32 records beside half a float32 ulp of the exact value) come from the reference quantities alone;
tests/test_frontend_conditioning_cpu.py pins them and shows that the rule has teeth.

Shapes: alpha is one number a launch, so each event form runs as four batches: alpha = 1 (264 columns -- 256 for f32
events -- of 3 to 15 events: the eight alpha = 1 families and the eight items judged apart; four full waves and a
partial one) and lowpass's three alphas (10 or 11 columns of 603 to 608 events each).  The first 65 columns of the
alpha = 1 batch run alone too.

Measured on MI355X: see test_fp64_records_against_the_exact_chain and test_f32_records_against_the_exact_chain."""
from __future__ import annotations

import numpy as np
import pytest

from poseestimationkf_amd import synth

from . import frontend_families as ff

pytestmark = pytest.mark.gpu

FORMS = {"f64": "f64", "f32": "f32"}     # the fixture's set -> engine.run_frontend's events


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


@pytest.fixture(scope="module")
def g():
    return ff.golden()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _batches(which):
    """[(alpha, item indices, the batch's event dict)] of a set, built once"""
    items, _ = ff.stacked(which)
    return [(a, ix, ff.events([items[i] for i in ix], float32=which == "f32")) for a, ix in ff.by_alpha(items).items()]


def _frontend(eng, ev, alpha, which):
    """run_frontend on a batch -> per column (gyro (R, 3), dt (R,), out (R, 2, 3) float64, dt words (R,) or None)"""
    win, counts = eng.run_frontend(ev, alpha=alpha, events=FORMS[which])
    K = len(counts)
    cols = []
    if which == "f64":
        gy, dt, a, m, _ = win.download_filters(np.arange(K))
        word = None
    else:
        rec = win.download_filters(np.arange(K))
        gy, dt, a, m, word = rec.gyro, rec.dt_ns, rec.acc, rec.mag, rec.dtw
    for k in range(K):
        r = int(counts[k])
        cols.append((gy[:r, k], dt[:r, k], np.stack([a[:r, k], m[:r, k]], axis=1).astype(np.float64),
                     None if word is None else word[:r, k]))
    return cols


@pytest.fixture(scope="module")
def runs(eng):
    """{set: per item (gyro, dt, out, dt words)}: both event forms through engine.run_frontend, a launch per alpha"""
    out = {}
    for which in FORMS:
        items, _ = ff.stacked(which)
        got = [None] * len(items)
        for alpha, ix, ev in _batches(which):
            for i, col in zip(ix, _frontend(eng, ev, alpha, which)):
                got[i] = col
        out[which] = got
    return out


def _expected_header(it):
    """(gyro (R, 3), dt (R,)) of the item's records: the gyro samples as given and the exact integer time differences"""
    tups = ff.tuples(it)
    t = np.array([it["t_init"]] + [r[1] for r in tups], np.int64)
    return np.array([r[0] for r in tups], np.float64).reshape(-1, 3), np.diff(t)


def _judge(g, which, runs, half_ulp32):
    """Per family the worst |dev - exact| / (kappa U) on the judged value (f32 records: after half a float32 ulp of
    the exact value is taken off the error), and per item whether every other stored value meets its own bound"""
    items, sl = ff.stacked(which)
    rho, rest_ok = np.full(len(items), np.nan), np.ones(len(items), bool)
    for i, it in enumerate(items[:sl["apart"].start]):
        rows, recs = ff.rows_of(g, which, i)
        gy, dt, out, _ = runs[which][i]
        assert len(out) == g[which + "_count"][i], (which, i)
        err = ff.error(out[recs], g, which, rows)
        if half_ulp32:
            err = np.maximum(err - 0.5 * ff.ulp32(g[which + "_out"][rows]), 0.0)
        err = np.where(np.isfinite(out[recs]), err, np.inf).max(axis=2)
        j = [n for n in ff.NAMES if sl[n].start <= i < sl[n].stop][0]
        bound = ff.FAST_MARGIN * g[which + "_Y"][ff.NAMES.index(j)] * g[which + "_kappa_row"][rows].astype(np.float64) * ff.U
        rest_ok[i] = (err <= bound).all()
        rho[i] = err[-1, it["ch"]] / (g[which + "_kappa"][i] * ff.U)
    return rho, rest_ok


def _assert_families(g, which, rho, rest_ok, label):
    _, sl = ff.stacked(which)
    for j, name in enumerate(ff.NAMES):
        Y = g[which + "_Y"][j]
        print("%s %-12s Y %.3g: %.3g Y (bound %.3g Y)" % (label, name, Y, rho[sl[name]].max() / Y, ff.FAST_MARGIN))
    for j, name in enumerate(ff.NAMES):
        Y = g[which + "_Y"][j]
        assert (ff.FAST_MARGIN * Y * g[which + "_kappa"][sl[name]] * ff.U < ff.INFORMATIVE).all(), name
        assert rho[sl[name]].max() <= ff.FAST_MARGIN * Y, name
        assert rest_ok[sl[name]].all(), name


def test_fp64_records_against_the_exact_chain(g, runs):
    """FP64 events -> FP64 records: per family max_i |dev - exact| / (kappa_i U) <= FAST_MARGIN Y on the last record's
    judged channel, every other stored value under the same bound with its own kappa; gyro, dt and counts exact.
    Measured on MI355X, the worst ratio in units of Y (bound 303):
        ordinary 4.47, extrapolate 2.29, cancel 0.34, clock_back 4.33, one_ns 24.5, long_pause 2.16, scale 8.55,
        mixed_scale 3.61, lowpass 0.96
    -- the same before and after rsqrt_sumsq took the place of rsqrt<true> (the bits are the same for finite sums).
    one_ns's 24.5 is rsqrt's own error class (19 ulp measured over 1e-6 .. 1e6) beside the interpolation's few."""
    items, sl = ff.stacked("f64")
    for i, it in enumerate(items):
        gy, dt, out, _ = runs["f64"][i]
        want_g, want_dt = _expected_header(it)
        assert np.array_equal(_bits(gy), _bits(want_g)) and np.array_equal(dt, want_dt.astype(np.float64)), i
    rho, rest_ok = _judge(g, "f64", runs, half_ulp32=False)
    _assert_families(g, "f64", rho, rest_ok, "k_frontend FP64 records")


def test_f32_records_against_the_exact_chain(g, runs):
    """f32 events -> 40 B records: |dev - exact| <= ulp32(exact) / 2 + FAST_MARGIN Y kappa U per value (reported as
    the excess over half an ulp in units of kappa U Y); the gyro is the float32 sample; the dt word is the dt, or
    PEKF_DT_ESCAPE with the dt in the side plane where it is negative or 2^31 - 1 ns and more (clock_back,
    extrapolate, one_ns and long_pause have both kinds).
    Measured on MI355X, the worst excess in units of Y (bound 303): 0 on every family -- each value is the exact
    one rounded to float32 -- but cancel (0.45), whose values near zero have float32 ulps below kappa U."""
    items, sl = ff.stacked("f32")
    escaped = 0
    for i, it in enumerate(items):
        gy, dt, out, word = runs["f32"][i]
        want_g, want_dt = _expected_header(it)
        assert gy.dtype == np.float32 and np.array_equal(gy.astype(np.float64), want_g), i
        assert np.array_equal(dt, want_dt.astype(np.float64)), i
        esc = (want_dt < 0) | (want_dt >= synth.DT_ESCAPE)
        assert np.array_equal(word & synth.DT_MASK, np.where(esc, synth.DT_ESCAPE, want_dt).astype(np.uint32)), i
        escaped += esc.sum()
    assert escaped >= 40
    rho, rest_ok = _judge(g, "f32", runs, half_ulp32=True)
    _assert_families(g, "f32", rho, rest_ok, "k_frontend f32 records")


@pytest.mark.parametrize("which", list(FORMS))
def test_the_list_judged_apart(g, runs, which):
    """An exactly zero interpolant, t2 == t1, an infinite or NaN sample: NaN in the components where the reference's
    record is NaN -- of that record and of every later record of that channel -- and nowhere else; the other channel
    finite and within the ordinary family's bound; gyro, dt and counts as for any item.  With rsqrt<true> in the
    normalisation (its Newton residual is inf * 0 at a sum of squares of +inf) the two items with an infinite newer
    sample gave NaN in all three components of that channel on MI355X, in both event forms, and every other item
    passed."""
    items, sl = ff.stacked(which)
    Y = g[which + "_Y"][0]
    for i in range(sl["apart"].start, sl["apart"].stop):
        it, label = items[i], ff.APART[i - sl["apart"].start]
        rows, recs = ff.rows_of(g, which, i)
        gy, dt, out, _ = runs[which][i]
        want_g, want_dt = _expected_header(it)
        assert len(out) == 3 and np.array_equal(gy.astype(np.float64), want_g) and np.array_equal(dt, want_dt.astype(np.float64)), label
        assert np.array_equal(np.isnan(out), g[which + "_nan"][rows]), (label, np.isnan(out).astype(int).tolist())
        o = 1 - it["ch"]
        err = ff.error(out, g, which, rows)[:, o]
        if which == "f32":
            err = np.maximum(err - 0.5 * ff.ulp32(g[which + "_out"][rows][:, o]), 0.0)
        assert np.isfinite(out[:, o]).all(), label
        assert (err.max(axis=1) <= ff.FAST_MARGIN * Y * g[which + "_kappa_row"][rows, o] * ff.U).all(), label


def _trajectory_rows(tj, counts):
    """the written rows of a (R, K, 4) trajectory as bits, column by column"""
    return [_bits(tj[:c, k]) for k, c in enumerate(counts)]


def test_one_arithmetic_two_kernels(eng, runs):
    """k_live and k_frontend round their records identically: on every batch of the FP64 items, the poses of
    BatchedEKF.run_events(events="f64", records="f64", trajectory=True) are those of run_frontend + the FP64-record
    run (pekf_run_rec64_dev) row by row in their bits, NaN rows included, and so are those of a LiveSession fed the
    same rows in chunks of 1 and of 7."""
    feeds = 0
    for alpha, ix, ev in _batches("f64"):
        K = len(ix)
        win, counts = eng.run_frontend(ev, alpha=alpha, events="f64")
        n = max(2, int(counts.max()))
        split = _trajectory_rows(eng.BatchedEKF(K).run(win, n_steps=n, want_traj=True), counts)
        fused = eng.BatchedEKF(K)
        c, _, tj = fused.run_events(ev, alpha=alpha, records="f64", events="f64", trajectory=True)
        assert np.array_equal(c, counts) and np.array_equal(tj["record_dt_ns"][0], [runs["f64"][i][1][0] for i in ix])
        live = _trajectory_rows(tj["trajectory"], counts)
        assert all(np.array_equal(a, b) for a, b in zip(split, live)), alpha
        E = ev["types"].shape[0]
        for step in (1, 7):
            f = eng.BatchedEKF(K)
            s = eng.LiveSession(f, ev["init_acc"], ev["init_mag"], ev["t_init"], alpha=alpha, events="f64")
            got = [[] for _ in range(K)]
            for a in range(0, E, step):
                chunk = {k: ev[k][a:a + step] for k in ("types", "values", "times", "values64")}
                cc, ct = s.feed(chunk, trajectory=True)
                feeds += 1
                for k in np.flatnonzero(cc):
                    got[k].append(_bits(ct["trajectory"][:cc[k], k]))
            assert np.array_equal(s.total_counts, counts), (alpha, step)
            for k in range(K):
                rows = np.concatenate(got[k]) if got[k] else np.zeros((0, 4), np.uint64)
                assert np.array_equal(rows, live[k]), (alpha, step, k)
            assert np.array_equal(_bits(f.get_state()[0]), _bits(fused.get_state()[0])), (alpha, step)
    print("k_live against k_frontend + the FP64-record run: 4 batches, %d chunks fed" % feeds)
    assert feeds == sum(-(-b[2]["types"].shape[0] // step) for b in _batches("f64") for step in (1, 7))


@pytest.mark.parametrize("which", list(FORMS))
def test_launch_shape(eng, runs, which):
    """The first 65 columns of the alpha = 1 batch -- a full wave and one lane of the next -- run alone give the
    full batch's bits, record for record."""
    items, _ = ff.stacked(which)
    alpha, ix, _ = _batches(which)[0]
    assert alpha == 1.0 and len(ix) >= 256
    ix = ix[:65]
    cols = _frontend(eng, ff.events([items[i] for i in ix], float32=which == "f32"), alpha, which)
    for i, (gy, dt, out, word) in zip(ix, cols):
        full = runs[which][i]
        assert np.array_equal(_bits(gy), _bits(full[0])) and np.array_equal(dt, full[1]) and np.array_equal(_bits(out), _bits(full[2])), i
