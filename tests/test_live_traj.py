"""A pose per record from the fused live launch (pekf_live_traj_dev; run_events / run_session /
run_wire_session with trajectory=...): the server's X_k of every phase-3 record (Parser::ExecuteKalmanFilter,
KFS/Parser.cpp:248-267), row r of filter k being its X after its own r-th record.

Checked bit for bit against routes that exist without it -- the same launch without a trajectory (X, P, counts,
refs), the launch's final X (the last row), the split pipeline's trajectory (run_frontend + BatchedEKF.run with
want_traj) for f32 records and for FP64 events, the front-end's record dt -- and, for the default FP64 records on
f32 events, against the NumPy restatement of the reference's loop within tests/test_live.py's ATOL_F64_CHAIN."""
import numpy as np
import pytest

from poseestimationkf_amd import synth, wire

from .test_frontend import _events, _oracle_records
from .test_live import ATOL_F64_CHAIN, _fused, _same

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 1500, 21), (64, 37, 22)]   # ragged counts, a partial last wave; a last event block padded with nulls
FORMS = {"f32 records": dict(records="f32", events="f32"), "FP64 records": dict(records="f64", events="f32"),
         "FP64 events": dict(records="f64", events="f64")}
G31 = (1 << 31) + 12345
# pauses of 2^31 ns and more and a clock stepping back (tests/test_live.py's clock-step stream): with f32 events
# these go through time events and escaped record dts, with FP64 events they are just the next event's time
CLOCK_STEPS = [(synth.EV_ACC, 1_000_000), (synth.EV_MAG, 1_000_000)] + [
    (synth.EV_GYRO, 1000), (synth.EV_ACC, G31), (synth.EV_MAG, 10), (synth.EV_GYRO, -5_000_000),
    (synth.EV_ACC, 700), (synth.EV_MAG, 0), (synth.EV_GYRO, 3 * G31), (synth.EV_ACC, 10), (synth.EV_MAG, 10)] * 4
# the clock steps back between two records (a negative record dt), then pauses for 2^31 ns and more
BACKWARDS = [(synth.EV_ACC, 1_000_000), (synth.EV_MAG, 1_000_000)] + [
    (synth.EV_GYRO, 1000), (synth.EV_ACC, 10), (synth.EV_MAG, 10), (synth.EV_GYRO, -5_000_000), (synth.EV_ACC, 700),
    (synth.EV_MAG, 10), (synth.EV_GYRO, G31), (synth.EV_ACC, 10), (synth.EV_MAG, 10)] * 4
# records 3 x (2^30 - 1) ns apart: every gap fits an f32 event, every record's dt is escaped
ESCAPED = [(synth.EV_GYRO, (1 << 30) - 1)] * 3 + [(synth.EV_ACC, 10), (synth.EV_MAG, 10)]


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


@pytest.fixture(scope="module")
def streams():
    made = {}

    def get(K, E, seed):
        if (K, E, seed) not in made:
            made[K, E, seed] = synth.generate_events(np.arange(K), E, seed=seed)
        return made[K, E, seed]
    return get


@pytest.fixture(scope="module")
def runs(eng, streams):
    """(X, P, counts, refs, trajectory dict) of run_events(trajectory=True) on a generated stream, made once"""
    made = {}

    def get(form, K, E, seed):
        if (form, K, E, seed) not in made:
            made[form, K, E, seed] = _traj_run(eng, streams(K, E, seed), K, **FORMS[form])
        return made[form, K, E, seed]
    return get


def _traj_run(eng, ev, K, trajectory=True, X0=None, P0=None, **form):
    f = eng.BatchedEKF(K)
    if X0 is not None:
        f.set_state(X0, P0)
    counts, refs, tj = f.run_events(ev, trajectory=trajectory, **form)
    X, P = f.get_state()
    return X, P, counts, refs, tj


def _mask(counts, rows):
    return np.arange(rows)[:, None] < np.asarray(counts)[None, :]


def _written_rows_equal(a, b, counts):
    """rows < counts[k] of two (R, K, ...) arrays, bit for bit (their R may differ)"""
    n = min(len(a), len(b))
    assert counts.max(initial=0) <= n
    m = _mask(counts, n)
    assert np.array_equal(a[:n][m], b[:n][m])


def _unwritten_rows_are_nan(tj, counts):
    R = len(tj["trajectory"])
    m = _mask(counts, R)
    assert np.isnan(tj["trajectory"][~m]).all() and np.isfinite(tj["trajectory"][m]).all()
    assert np.isnan(tj["record_dt_ns"][~m]).all() and np.isfinite(tj["record_dt_ns"][m]).all()
    assert np.isnan(tj["record_times_ns"][~m]).all() and np.isfinite(tj["record_times_ns"][m]).all()


def _resumed(K, seed):
    rng = np.random.default_rng(seed)
    X0 = rng.standard_normal((K, 4))
    X0 /= np.linalg.norm(X0, axis=1, keepdims=True)
    return X0, np.tile(np.eye(4) * 0.4, (K, 1, 1))


# ------------------------------------------------------------------ 1, 2. the filter is left alone

@pytest.mark.parametrize("K,E,seed", SHAPES)
@pytest.mark.parametrize("form", list(FORMS))
def test_trajectory_leaves_the_filter_alone_and_ends_at_the_final_state(eng, streams, runs, form, K, E, seed):
    X, P, counts, refs, tj = runs(form, K, E, seed)
    _same((X, P, counts, refs), _fused(eng, streams(K, E, seed), K, **FORMS[form]))
    assert tj["trajectory"].shape == (E // 3, K, 4) and tj["record_dt_ns"].shape == (E // 3, K)
    assert counts.max() > 0 and counts.max() <= E // 3
    has = counts >= 1
    assert np.array_equal(tj["trajectory"][counts[has] - 1, np.flatnonzero(has)], X[has])
    _unwritten_rows_are_nan(tj, counts)
    assert np.array_equal(tj["record_times_ns"], eng.record_times_ns(streams(K, E, seed)["t_init"], tj["record_dt_ns"]),
                          equal_nan=True)


@pytest.mark.parametrize("records", ["f32", "f64"])
def test_trajectory_with_time_events_leaves_the_filter_alone(eng, records):
    """f32 events whose planes hold time events (the TE kernels), both record precisions, from a resumed state"""
    K = 64
    ev = _events(K, CLOCK_STEPS)
    X0, P0 = _resumed(K, 44)
    X, P, counts, refs, tj = _traj_run(eng, ev, K, X0=X0, P0=P0, records=records)
    _same((X, P, counts, refs), _fused(eng, ev, K, X0, P0, records=records))
    assert np.all(counts == 12)
    assert np.array_equal(tj["trajectory"][11], X)
    _unwritten_rows_are_nan(tj, counts)


# ------------------------------------------------------------------ 3, 4. the split pipeline's trajectory

@pytest.mark.parametrize("K,E,seed", SHAPES)
@pytest.mark.parametrize("form", ["f32 records", "FP64 events"])
def test_trajectory_equals_the_split_pipeline(eng, streams, runs, form, K, E, seed):
    """f32 records: run_frontend + BatchedEKF.run(want_traj=True); FP64 events: the same over FP64 records"""
    X, P, counts, refs, tj = runs(form, K, E, seed)
    win, c = eng.run_frontend(streams(K, E, seed), events=FORMS[form]["events"])
    assert np.array_equal(c, counts)
    f = eng.BatchedEKF(K)
    split = f.run(win, n_steps=max(2, int(counts.max())), want_traj=True)
    _written_rows_equal(tj["trajectory"], split, counts)
    _same((X, P), f.get_state())


# ------------------------------------------------------------------ 5. FP64 records on f32 events: the oracle

@pytest.mark.parametrize("K,E,seed,every", [(1000, 1500, 21, 97), (64, 37, 22, 7)])
def test_fp64_record_trajectory_follows_the_oracle(streams, runs, K, E, seed, every):
    """Sampled filters, every row against ekf_numpy.run_filter(record=True) on the restatement's float64
    records.  Measured worst |row - oracle| (printed): 2.6e-14 at 1,000 x 1,500, 5.1e-14 at 64 x 37."""
    from oracle import ekf_numpy
    ev = streams(K, E, seed)
    _, _, counts, refs, tj = runs("FP64 records", K, E, seed)
    worst = 0.0
    for k in range(0, K, every):
        g, dt, a, m = _oracle_records(ev, k)
        assert counts[k] == len(dt)
        _, _, want = ekf_numpy.run_filter(g, dt.astype(np.float64), a, m, refs[k, :3], refs[k, 3:], record=True)
        if len(dt):
            worst = max(worst, float(np.abs(tj["trajectory"][:len(dt), k] - want).max()))
            assert np.array_equal(tj["record_dt_ns"][:len(dt), k], dt.astype(np.float64))
    print("FP64-record trajectory, %d x %d: worst row vs the oracle chain %.3e" % (K, E, worst))
    assert worst < ATOL_F64_CHAIN


# ------------------------------------------------------------------ 6. the records' dt

def _frontend_dt(eng, ev, events):
    """(dt (r_max, K) float64 ns of run_frontend's records, counts)"""
    win, counts = eng.run_frontend(ev, events=events)
    R, K = win.window, win.batch
    if events == "f64":
        return win.gd.download((R, K, 4), np.float64)[..., 3], counts
    word = np.ascontiguousarray(win.gd.download((R, K, 4), np.float32)[..., 3]).view(np.uint32) & 0x7FFFFFFF
    dt = word.astype(np.float64)
    if win.dtx is not None:
        dt = np.where(word == 0x7FFFFFFF, win.dtx.download((R, K), np.float64), dt)
    else:
        assert not (word[_mask(counts, R)] == 0x7FFFFFFF).any()
    return dt, counts


@pytest.mark.parametrize("K,E,seed", SHAPES)
@pytest.mark.parametrize("form", list(FORMS))
def test_record_dt_is_the_frontends(eng, streams, runs, form, K, E, seed):
    _, _, counts, _, tj = runs(form, K, E, seed)
    dt, c = _frontend_dt(eng, streams(K, E, seed), FORMS[form]["events"])
    assert np.array_equal(c, counts)
    _written_rows_equal(tj["record_dt_ns"], dt, counts)


@pytest.mark.parametrize("spec,n_rec", [(CLOCK_STEPS, 12), (BACKWARDS, 12), (ESCAPED * 5, 5)])
@pytest.mark.parametrize("form", list(FORMS))
def test_record_dt_across_long_pauses_and_a_clock_step(eng, form, spec, n_rec):
    """Pauses of 2^31 ns or more and a clock stepping back: the dt word's escape (f32 events: the queue's side
    entry or register), the FP64 event's float64 difference -- the dt the front-end writes, bit for bit, and the
    trajectory still ends at the final X"""
    K = 64
    ev = _events(K, spec)
    X0, P0 = _resumed(K, 9)
    X, _, counts, _, tj = _traj_run(eng, ev, K, X0=X0, P0=P0, **FORMS[form])
    assert np.all(counts == n_rec)
    dt, c = _frontend_dt(eng, ev, FORMS[form]["events"])
    assert np.array_equal(c, counts)
    _written_rows_equal(tj["record_dt_ns"], dt, counts)
    got = tj["record_dt_ns"][:n_rec]
    assert (np.abs(got) >= 2.0**31).any()
    if spec is BACKWARDS:     # (the restatement's record dts of this stream: 2001000, -4999980, 2147496703, 1020, ...)
        assert (got < 0).any()
    assert np.array_equal(tj["trajectory"][n_rec - 1], X)
    _unwritten_rows_are_nan(tj, counts)


# ------------------------------------------------------------------ 7. nothing else is written

@pytest.mark.parametrize("form", list(FORMS))
def test_a_row_cap_keeps_the_first_rows_and_the_counts(runs, eng, streams, form):
    K, E, seed = SHAPES[0]
    X, P, counts, refs, tj = runs(form, K, E, seed)
    Xc, Pc, cc, rc, tc = _traj_run(eng, streams(K, E, seed), K, trajectory=5, **FORMS[form])
    _same((Xc, Pc, cc, rc), (X, P, counts, refs))
    assert counts.max() > 5 and tc["trajectory"].shape == (5, K, 4)
    for key in ("trajectory", "record_dt_ns", "record_times_ns"):
        assert np.array_equal(tc[key], tj[key][:5], equal_nan=True), key


@pytest.mark.parametrize("flags_of", ["f32 records", "FP64 records", "FP64 events"])
def test_rows_past_the_cap_keep_their_bytes(eng, streams, flags_of):
    """pekf_live_traj_dev on the caller's own buffers: 5 rows asked for, two guard rows behind them and every
    row a filter does not reach keep the bytes the caller put there; counts report every record"""
    K, E, seed = SHAPES[0]
    ev = dict(streams(K, E, seed))
    ev["types"] = ev["types"].copy()
    ev["types"][:, [5, 70, 999]] = synth.EV_ACC        # no record at all
    ev["types"][30:, [6, 64, 500]] = synth.EV_ACC      # one or two records (the restatement: 1, 2, 1), below the cap
    form = FORMS[flags_of]
    evb, En, flags = eng._event_planes(ev, form["events"])
    flags |= eng._record_flags(form["records"], form["events"])
    init = eng.DeviceBuffer(48 * K).upload(np.concatenate([ev["init_acc"], ev["init_mag"]], axis=1).astype(np.float64))
    tib = eng.DeviceBuffer(8 * K).upload(np.ascontiguousarray(ev["t_init"], np.int64))
    cnt, refs = eng.DeviceBuffer(4 * K), eng.DeviceBuffer(48 * K)
    cap, guard = 5, 2
    fill_t = np.full((cap + guard, K, 4), -12345.678)
    fill_d = np.full((cap + guard, K), -8765.4321)
    tb, db = eng.DeviceBuffer(fill_t.nbytes).upload(fill_t), eng.DeviceBuffer(fill_d.nbytes).upload(fill_d)
    f = eng.BatchedEKF(K)
    f.run_events_async(evb, En, init, tib, cnt, refs, flags=flags, traj=tb, traj_dt=db, traj_rows=cap)
    f2 = eng.BatchedEKF(K)
    cnt2, tb2 = eng.DeviceBuffer(4 * K), eng.DeviceBuffer(fill_t.nbytes).upload(fill_t)
    f2.run_events_async(evb, En, init, tib, cnt2, refs, flags=flags, traj=tb2, traj_dt=None, traj_rows=cap)
    eng.check(eng.lib.pekf_device_sync())
    counts = cnt.download((K,), np.int32)
    got_t, got_d = tb.download(fill_t.shape, np.float64), db.download(fill_d.shape, np.float64)
    _, _, tj = eng.BatchedEKF(K).run_events(ev, trajectory=True, **form)
    assert counts.max() > cap + guard and np.all(counts[[5, 70, 999]] == 0)
    assert np.all((counts[[6, 64, 500]] > 0) & (counts[[6, 64, 500]] < cap))
    assert np.array_equal(counts, cnt2.download((K,), np.int32))
    m = np.concatenate([_mask(counts, cap), np.zeros((guard, K), bool)])
    assert np.array_equal(got_t[m], tj["trajectory"][:cap][m[:cap]])
    assert np.array_equal(got_d[m], tj["record_dt_ns"][:cap][m[:cap]])
    assert np.array_equal(got_t[~m], fill_t[~m]) and np.array_equal(got_d[~m], fill_d[~m])
    assert np.array_equal(tb2.download(fill_t.shape, np.float64), got_t)      # without traj_dt: the same rows


# ------------------------------------------------------------------ 8. idle filters

def test_filters_that_never_got_ready_have_no_rows(eng):
    """tests/test_live.py's session whose phase 2 leaves about a third of the filters not ready"""
    K = 384
    ph2 = synth.generate_events(np.arange(K), 520, seed=36)
    ph3 = synth.generate_events(np.arange(K), 400, seed=37)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    X0, P0 = _resumed(K, 38)
    f, g = eng.BatchedEKF(K), eng.BatchedEKF(K)
    f.set_state(X0, P0)
    g.set_state(X0, P0)
    got = eng.run_session(ph2, ph3, f, records="f32", trajectory=True)
    plain = eng.run_session(ph2, ph3, g, records="f32")
    assert sorted(plain) == ["counts", "ready", "refs"]
    assert sorted(got) == ["counts", "ready", "record_dt_ns", "record_times_ns", "refs", "trajectory"]
    _same(f.get_state() + (got["counts"], got["refs"], got["ready"]),
          g.get_state() + (plain["counts"], plain["refs"], plain["ready"]))
    ready = got["ready"]
    assert 0 < ready.sum() < K and np.all(got["counts"][~ready] == 0) and np.all(got["counts"][ready] > 0)
    for key in ("trajectory", "record_dt_ns", "record_times_ns"):
        assert np.isnan(got[key][:, ~ready]).all(), key
    _unwritten_rows_are_nan(got, got["counts"])
    X = f.get_state()[0]
    assert np.array_equal(got["trajectory"][got["counts"][ready] - 1, np.flatnonzero(ready)], X[ready])
    ini = eng.frontend_init(ph2)
    assert np.array_equal(got["record_times_ns"],
                          eng.record_times_ns(ini["t_init"], got["record_dt_ns"]), equal_nan=True)


@pytest.mark.parametrize("form", list(FORMS))
def test_streams_without_records_have_no_rows(eng, streams, form):
    K, E = 130, 300
    ev = dict(streams(K, E, 29))
    idle = [3, 64, 129]
    ev["types"] = ev["types"].copy()
    ev["types"][:, idle] = synth.EV_ACC              # no gyro, no mag: no record
    X0, P0 = _resumed(K, 6)
    X, P, counts, _, tj = _traj_run(eng, ev, K, X0=X0, P0=P0, **FORMS[form])
    assert np.all(counts[idle] == 0) and np.all(np.delete(counts, idle) > 0)
    assert np.array_equal(X[idle], X0[idle]) and np.array_equal(P[idle], P0[idle])
    for key in ("trajectory", "record_dt_ns", "record_times_ns"):
        assert np.isnan(tj[key][:, idle]).all(), key
    _unwritten_rows_are_nan(tj, counts)
    # every filter idle: nothing at all is written
    none = _events(70, [(synth.EV_ACC, 10), (synth.EV_MAG, 10)] * 5)
    _, _, c0, _, t0 = _traj_run(eng, none, 70, **FORMS[form])
    assert np.all(c0 == 0) and t0["trajectory"].shape == (3, 70, 4) and np.isnan(t0["trajectory"]).all()
    assert np.isnan(t0["record_dt_ns"]).all()


# ------------------------------------------------------------------ 9. the wire session

def _session_texts(K, n1=0):
    ph2 = synth.generate_events(np.arange(K), 700, seed=63)
    ph3 = synth.generate_events(np.arange(K), 400, seed=64)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    ph1 = synth.generate_calibration_events(K, n1, seed=84) if n1 else None
    texts = []
    for k in range(K):
        n2, n3 = 640 + 4 * (k % 13), 400 - 9 * (k % 5)    # phase-2 parts of different lengths: phase-3 rows drift
        t = wire.events_text(ph1["types"][:, k], ph1["values"][:, k], ph1["times"][:, k], phase=1) if n1 else ""
        texts.append(t + wire.events_text(ph2["types"][:n2, k], ph2["values"][:n2, k], ph2["times"][:n2, k], phase=2) +
                     wire.events_text(ph3["types"][:n3, k], ph3["values"][:n3, k], ph3["times"][:n3, k], phase=3))
    return texts, ph2["times"][0]


def _sessions_equal(a, fa, b, fb):
    for key in ("ready", "counts", "refs"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    _same(fa.get_state(), fb.get_state())
    counts = a["counts"]
    n = min(len(a["trajectory"]), len(b["trajectory"]))       # (True: a third of the rows each launch reads)
    assert counts.max() <= n
    for key in ("trajectory", "record_dt_ns", "record_times_ns"):
        assert np.array_equal(a[key][:n], b[key][:n], equal_nan=True), key
        assert np.isnan(a[key][n:]).all() and np.isnan(b[key][n:]).all(), key
    _unwritten_rows_are_nan(a, counts)


@pytest.mark.parametrize("frame_rows", [True, False])
def test_wire_session_trajectory_equals_the_event_sessions(eng, frame_rows):
    K = 96
    texts, t0 = _session_texts(K)
    f_dev, f_host, f_plain = eng.BatchedEKF(K), eng.BatchedEKF(K), eng.BatchedEKF(K)
    dev = eng.run_wire_session(wire.frames(texts), f_dev, frame_rows=frame_rows, trajectory=True)
    e2 = wire.events_from_wire(texts, np.zeros((K, 3)), np.zeros((K, 3)), t0, phase=2)
    e3 = wire.events_from_wire(texts, np.zeros((K, 3)), np.zeros((K, 3)), t0, phase=3)
    host = eng.run_session(e2, e3, f_host, events="f64", trajectory=True)
    assert dev["ready"].sum() > K // 2 and dev["counts"][dev["ready"]].min() > 0
    _sessions_equal(dev, f_dev, host, f_host)
    plain = eng.run_wire_session(wire.frames(texts), f_plain, frame_rows=frame_rows)
    assert sorted(plain) == ["counts", "ready", "refs"]
    _same(f_plain.get_state() + (plain["counts"],), f_dev.get_state() + (dev["counts"],))
    has = dev["counts"] >= 1
    assert np.array_equal(dev["trajectory"][dev["counts"][has] - 1, np.flatnonzero(has)], f_dev.get_state()[0][has])


def test_wire_session_trajectory_with_a_calibration_from_its_frames(eng):
    """calibration="frames" against calibration=<the same fit as a dict>: the same trajectory"""
    K, n_cal = 70, 20
    texts, _ = _session_texts(K, n1=30)
    fr = wire.frames(texts)
    e1 = wire.events_from_wire(texts, np.zeros((K, 3)), np.zeros((K, 3)), np.zeros(K, np.int64), phase=1)
    cal = eng.calibrate_magnetometer(e1, n_cal=n_cal, events="f64")
    f_a, f_b = eng.BatchedEKF(K), eng.BatchedEKF(K)
    a = eng.run_wire_session(fr, f_a, calibration="frames", n_cal=n_cal, trajectory=True)
    b = eng.run_wire_session(fr, f_b, calibration=cal, trajectory=True)
    assert a["calibrated"].all() and a["counts"].max() > 0
    _sessions_equal(a, f_a, b, f_b)
