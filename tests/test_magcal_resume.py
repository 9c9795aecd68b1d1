"""Chunked phase 1 on the device (csrc/pekf_magcal_resume.hip: pekf_magcal_resume_dev; engine.CalibrationSession)
against the one launch (pekf_magcal_dev, engine.calibrate_magnetometer): any cutting of a phase-1 plane into
chunks gives the one launch's cal, fit and status bit for bit (NaN bits included), after every chunk, on both
event forms.

Shapes: 70 phones (one wave and a 6-lane tail) with n_cal = 20 unless said otherwise; chunk sizes 1, 3, 7, 8, 9
(the last three bracket the 8-row event ring), random ones with empty chunks, and one chunk."""
import numpy as np
import pytest

from poseestimationkf_amd import synth

from . import magcal_numpy as mc
from .test_magcal import _ragged, _with_values64
from .test_magcal_cpu import hyperboloid_samples

pytestmark = pytest.mark.gpu

K, N_CAL, E = 70, 20, 60
FORMS = ("f32", "f64")


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


def _rows(ev, a, b):
    return {k: ev[k][a:b] for k in ("types", "values", "values64", "times")}


def _out(d):
    """A calibration dict's device outputs as bits: (cal (K, 12), fit (K, 6)) uint64 and status"""
    Kk = len(d["status"])
    cal = d["cal"].download((Kk, 12), np.float64)
    assert np.array_equal(cal[:, :3], d["bias"]) and np.array_equal(cal[:, 3:].reshape(Kk, 3, 3), d["W"])
    return cal.view(np.uint64), np.ascontiguousarray(d["fit"]).view(np.uint64), d["status"].copy()


def _same(got, want, what=""):
    for g, w, key in zip(got, want, ("cal", "fit", "status")):
        assert np.array_equal(g, w), "%s: %s differs for phones %s" % (what, key, np.unique(np.nonzero(g != w)[0])[:8])


def _uncalibrated(out, phones):
    cal, fit, status = out
    assert np.all(status[phones] == 1)
    assert np.array_equal(cal[phones].view(np.float64), np.tile(np.r_[np.zeros(3), np.eye(3).ravel()], (len(phones), 1)))
    assert np.isnan(fit[phones].view(np.float64)).all()


def _scattered():
    """60 rows x 70 phones with no-message rows scattered in: 15..40 messages per phone, so phones 15..20 never fire
    and the rest fire at different rows; every fifth phone sends messages of types 0..3."""
    rng = np.random.default_rng(2019)
    src = synth.generate_calibration_events(K, 40, seed=19)
    types = np.full((E, K), synth.EV_NONE, np.uint32)
    vals = np.zeros((E, K, 3), np.float32)
    n_msg = 15 + (np.arange(K) * 7) % 26
    n_msg[[0, 64, 69]] = (15, 40, 21)
    for k in range(K):
        rows = np.sort(rng.choice(E, n_msg[k], replace=False))
        types[rows, k] = rng.integers(0, 4, n_msg[k]) if k % 5 == 3 else synth.EV_MAG
        vals[rows, k] = src["values"][:n_msg[k], k]
    times = src["t_init"][None, :] + 10_000_000 * (1 + np.arange(E))[:, None]
    return dict(types=types, values=vals, values64=vals.astype(np.float64), times=times, t_init=src["t_init"]), n_msg


def _fire_rows(ev, n_cal):
    """per phone the row of its message n_cal + 1 (the plane's row count if it has none)"""
    seen = np.cumsum(ev["types"] != synth.EV_NONE, axis=0)
    return np.where(seen[-1] > n_cal, np.argmax(seen > n_cal, axis=0), len(seen))


@pytest.fixture(scope="module")
def scattered(eng):
    """The plane, and the one launch on its first r rows for every r and both event forms (shared, not modified)"""
    ev, n_msg = _scattered()
    fire = _fire_rows(ev, N_CAL)
    assert n_msg.min() == 15 and n_msg.max() == 40 and (n_msg <= N_CAL).sum() >= 6
    assert len(np.unique(fire[n_msg > N_CAL])) >= 20 and (ev["types"][:, 3::5] != synth.EV_MAG).any()
    refs = {}
    for form in FORMS:
        refs[form] = [None] + [_out(eng.calibrate_magnetometer(_rows(ev, 0, r), n_cal=N_CAL, events=form))
                               for r in range(1, E + 1)]
        refs[form][0] = refs[form][1]                # no phone has fired after one row
        _uncalibrated(refs[form][0], np.arange(K))
        assert sorted(np.unique(refs[form][E][2])) == [0, 1]
    assert synth.has_time_events(synth.pack_events(ev))   # the f32 form has time events inside
    return ev, refs


def _cuts(name):
    if name == "one":
        return [0, E]
    if name == "random":
        rng = np.random.default_rng(5)
        inner = np.sort(rng.integers(0, E + 1, 14))
        inner[3] = inner[2]                           # empty chunks, one of them the first
        return [0, 0] + inner.tolist() + [E, E]
    return list(range(0, E, int(name))) + [E]


@pytest.mark.parametrize("events", FORMS)
@pytest.mark.parametrize("cutting", ["1", "3", "7", "8", "9", "random", "one"])
def test_any_cutting_equals_the_one_launch(eng, scattered, cutting, events):
    """After every chunk cal / fit / status are the one launch's on the rows so far, bit for bit."""
    ev, refs = scattered
    s = eng.CalibrationSession(K, N_CAL, events)
    _same(_out(s.result()), refs[events][0], "before any row")
    cuts = _cuts(cutting)
    for a, b in zip(cuts[:-1], cuts[1:]):
        s.feed(_rows(ev, a, b))
        _same(_out(s.result()), refs[events][b], "after rows %d..%d" % (a, b))
    assert cuts[-1] == E


@pytest.fixture(scope="module")
def dense(eng):
    """25 rows, a message in every row, so message n_cal + 1 is row 20 for every phone but phone 33, which stops
    after exactly n_cal messages.  With the one launch on every prefix."""
    ev = _with_values64(synth.generate_calibration_events(K, 25, seed=23))
    ev["types"][N_CAL:, 33] = synth.EV_NONE
    refs = {form: {r: _out(eng.calibrate_magnetometer(_rows(ev, 0, r), n_cal=N_CAL, events=form))
                   for r in (20, 21, 25)} for form in FORMS}
    return ev, refs


@pytest.mark.parametrize("events", FORMS)
@pytest.mark.parametrize("cuts", [[0, 20, 25], [0, 21, 25], [0, 20, 21, 25]], ids=["first", "last", "alone"])
def test_the_firing_message_at_chunk_edges(eng, dense, cuts, events):
    """Message n_cal + 1 as a chunk's first row, as its last row and alone in a one-row chunk; a phone with exactly
    n_cal messages stays not calibrated."""
    ev, refs = dense
    others = np.delete(np.arange(K), 33)
    assert np.all(refs[events][20][2] == 1) and np.all(refs[events][21][2][others] == 0)
    s = eng.CalibrationSession(K, N_CAL, events)
    for a, b in zip(cuts[:-1], cuts[1:]):
        s.feed(_rows(ev, a, b))
        got = _out(s.result())
        _same(got, refs[events][b], "after rows %d..%d" % (a, b))
        _uncalibrated(got, np.array([33]) if b > 20 else np.arange(K))


@pytest.mark.parametrize("events", FORMS)
def test_degenerate_phones_through_the_chunked_path(eng, dense, events):
    """test_magcal.py's flat, still and hyperboloid phones at n_cal = 20, in lanes 5, 40 and 66 (the tail): status
    2, 2 and 3, equal to the one launch bit for bit, and the other lanes unchanged."""
    ev, refs = dense
    flat, still, hyper = 5, 40, 66
    vals = ev["values"].copy()
    vals[:21, flat, 2] = 17.0
    vals[:21, still] = [12.5, -3.25, 40.0]
    vals[:21, hyper] = hyperboloid_samples(21)
    ev = _with_values64(dict(ev, values=vals))
    one = _out(eng.calibrate_magnetometer(_rows(ev, 0, 25), n_cal=N_CAL, events=events))
    want = np.zeros(K, np.int32)
    want[[flat, still]], want[hyper], want[33] = 2, 3, 1
    assert np.array_equal(one[2], want)
    assert np.array_equal(want, mc.calibrate(ev["types"], vals, n_cal=N_CAL)["status"])
    s = eng.CalibrationSession(K, N_CAL, events)
    for a, b in ((0, 7), (7, 19), (19, 22), (22, 25)):
        s.feed(_rows(ev, a, b))
    got = _out(s.result())
    _same(got, one)
    rest = np.delete(np.arange(K), [flat, still, hyper])
    _same([g[rest] for g in got], [r[rest] for r in refs[events][25]], "the other lanes")
    bad = np.array([flat, still, hyper])
    assert np.all(got[0][bad].view(np.float64)[:, :3] == 0.0) and np.isnan(got[1][bad].view(np.float64)).all()


@pytest.mark.parametrize("events", FORMS)
def test_a_fired_phone_is_not_written_again(eng, dense, events):
    """30 more messages after every phone has fired (other samples: a second fit would give other numbers), then a
    launch without rows: no bit of the outputs moves.  Phone 33, at exactly n_cal messages, fires on the first of
    them, as the one launch over all the rows says."""
    ev, refs = dense
    more = _with_values64(synth.generate_calibration_events(K, 30, seed=29))
    more["types"][0, 33] = synth.EV_NONE
    s = eng.CalibrationSession(K, N_CAL, events)
    s.feed(_rows(ev, 0, 25))
    before = _out(s.result())
    _same(before, refs[events][25])
    s.feed(_rows(more, 0, 1))                        # no message for phone 33 yet
    _same(_out(s.result()), before, "one more row")
    s.feed(_rows(more, 1, 30))
    after = _out(s.result())
    others = np.delete(np.arange(K), 33)
    _same([g[others] for g in after], [b[others] for b in before], "30 more messages")
    both = {k: np.concatenate([ev[k], more[k]]) for k in ("types", "values", "values64", "times")}
    _same(after, _out(eng.calibrate_magnetometer(both, n_cal=N_CAL, events=events)), "against the one launch")
    assert after[2][33] == 0
    s.feed_planes(None, 0)
    _same(_out(s.result()), after, "a launch without rows")


@pytest.mark.parametrize("events", FORMS)
def test_block_edge_and_the_references_size(eng, events):
    """300 phones (past the 256-thread block) with n_cal = 100: test_magcal.py's ragged plane of 171 rows, its 200
    phones and the first 100 of them again, in chunks of 50.  The one launch's bits, and the restatement's bias."""
    ev200, _ = _ragged()
    ev = {k: np.concatenate([ev200[k], ev200[k][:, :100]], axis=1) for k in ("types", "values", "values64", "times")}
    one = eng.calibrate_magnetometer(ev, n_cal=100, events=events)
    s = eng.CalibrationSession(300, 100, events)
    for a in range(0, 171, 50):
        s.feed(_rows(ev, a, min(a + 50, 171)))
    got = s.result()
    _same(_out(got), _out(one))
    assert sorted(np.unique(got["status"])) == [0, 1]
    model = mc.calibrate(ev["types"], ev["values"], n_cal=100)
    assert np.array_equal(got["status"], model["status"])
    assert np.array_equal(got["bias"].view(np.uint64), model["bias"].view(np.uint64))


@pytest.mark.parametrize("events", FORMS)
def test_calibration_session_planes_and_its_result_in_a_session(eng, scattered, events):
    """feed_planes on row ranges of one resident plane equals feed on dict chunks; result()["cal"] is what
    run_session takes as calibration."""
    ev, refs = scattered
    if events == "f64":
        planes = synth.pack_events64(ev, ev["values64"])
    else:
        planes = synth.pack_events(ev)
    rows, row_bytes = planes.shape[0], planes[0].nbytes
    buf = eng.DeviceBuffer(planes.nbytes).upload(planes)
    s = eng.CalibrationSession(K, N_CAL, events)
    for a in range(0, rows, 11):
        s.feed_planes(buf, min(11, rows - a), offset=a * row_bytes)
    got = s.result()
    _same(_out(got), refs[events][E])
    with pytest.raises(ValueError, match="outside the planes buffer"):
        s.feed_planes(buf, rows + 1)
    with pytest.raises(ValueError, match="outside the planes buffer"):
        s.feed_planes(buf, 1, offset=8)
    # as run_session's calibration: the same session as with the one launch's dict
    ph2 = synth.generate_events(np.arange(K), 80, seed=31)
    ph3 = synth.generate_events(np.arange(K), 40, seed=37)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    one = eng.calibrate_magnetometer(ev, n_cal=N_CAL, events=events)
    fa, fb = eng.BatchedEKF(K), eng.BatchedEKF(K)
    oa = eng.run_session(ph2, ph3, fa, n_avg=10, events="f64", calibration=got)
    ob = eng.run_session(ph2, ph3, fb, n_avg=10, events="f64", calibration=one)
    assert oa["ready"].sum() > K // 2 and oa["counts"][oa["ready"]].min() > 0
    assert oa["calibrated"].any() and not oa["calibrated"].all()
    for key in ob:
        assert np.array_equal(oa[key], ob[key], equal_nan=key == "refs"), key   # (a phone that is not ready: NaN)
    for a, b in zip(fa.get_state(), fb.get_state()):
        assert np.array_equal(a, b)
