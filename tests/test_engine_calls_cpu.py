"""The C calls behind engine.py's public functions: which entries, in which order, with which scalar arguments.

Every call that reaches the library goes to a recording fake (tests/fake_libpekf.py's host fake: device
memory is host memory, copies are memmoves) that computes nothing and returns 0.  A call is recorded as
(name, arguments) with each pointer into the fake's device memory written D, a ctypes reference "ref", and
every scalar and every null pointer as it is.  The expected sequences are written out here by hand from
include/pekf.h's signatures; they are what engine.py has to keep doing however its code is arranged."""
import numpy as np
import pytest

from poseestimationkf_amd import synth

D = "dev"
K, E = 4, 30
R_MAX = E // 3 + 1   # run_frontend's default window
ROWS = E // 3        # trajectory=True
SYNC = ("pekf_device_sync", ())


@pytest.fixture
def fake(monkeypatch):
    from . import fake_libpekf

    class Fake(fake_libpekf.FakeLib):
        COUNTS_ARG = {"pekf_run_dev": 13, "pekf_filter_run_ext": 9}

        def __init__(self):
            super().__init__(1)
            self.counts_seen = []   # the per-filter counts a run was launched with

        def _norm(self, a):
            if a is None or isinstance(a, (bool, float)):
                return a
            if isinstance(a, (int, np.integer)):
                a = int(a)
                return D if any(p <= a < p + len(b) for p, b in self.mem.items()) else a
            return "ref"

        def _record(self, name, a):
            self.calls.append((name, tuple(self._norm(v) for v in a)))
            i = self.COUNTS_ARG.get(name)
            if i is not None and a[i] is not None:
                self.counts_seen.append(self._view(a[i], 4 * K, np.int32).copy())
            return 0

        def __getattr__(self, name):
            if name.startswith("pekf_"):
                return lambda *a: self._record(name, a)
            raise AttributeError("fake libpekf has no %s" % name)

        def pekf_device_sync(self):
            return self._record("pekf_device_sync", ())

        def pekf_run_dev(self, *a):
            return self._record("pekf_run_dev", a)

        def pekf_filter_create(self, *a):
            self.create_flags = a[6]
            fake_libpekf._set(a[-1], 77)
            return 0

        # the error word: a record's dt escaped (bit 1) while there is no side plane, stored there (bit 4) once
        # there is one; FP64 events escape nothing
        def pekf_frontend_ext_dev(self, *a):
            self._view(a[14], 4, np.int32)[0] = 0 if a[13] & 4 else (1 if a[10] is None else 4)
            return self._record("pekf_frontend_ext_dev", a)

    from poseestimationkf_amd import _lib, engine
    f = Fake()
    for mod in (_lib, engine):
        monkeypatch.setattr(mod, "lib", f)
    return f


@pytest.fixture
def engine(fake):
    from poseestimationkf_amd import engine
    return engine


def _events(seed=3):
    ev = synth.generate_events(np.arange(K), E, seed=seed)
    return dict(ev, values64=ev["values"].astype(np.float64))   # (the server's values: any doubles do here)


def _session():
    ph2, ph3 = _events(3), _events(4)
    return ph2, dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])


def _live(flags):
    return ("pekf_live_ext_dev", (K, E, D, D, D, 0.1, D, D, 1.0, 0.1, D, D, flags, None, None))


def _live_traj(flags, rows):
    return [("pekf_memset", (D, 0xFF, 32 * rows * K, None)), ("pekf_memset", (D, 0xFF, 8 * rows * K, None)),
            ("pekf_live_traj_dev", (K, E, D, D, D, 0.1, D, D, 1.0, 0.1, D, D, flags, D, D, rows, None, None))]


def _phase2(flags, stats=None):
    return ("pekf_frontend_init_ext_dev", (K, E, D, D, 100, D, D, stats, D, flags, None))


def test_run_events(fake, engine):
    f = engine.BatchedEKF(K)
    fake.calls.clear()
    counts, refs = f.run_events(_events())
    assert fake.calls == [_live(0), SYNC]
    assert counts.shape == (K,) and counts.dtype == np.int32 and refs.shape == (K, 6)
    fake.calls.clear()
    f.run_events(_events(), records="f32")
    assert fake.calls == [_live(2), SYNC]
    fake.calls.clear()
    assert len(f.run_events(_events(), events="f64")) == 2
    assert fake.calls == [_live(4), SYNC]
    fake.calls.clear()
    out = f.run_events(_events(), events="f64", trajectory=True)
    assert fake.calls == _live_traj(4, ROWS) + [SYNC]
    assert out[2]["trajectory"].shape == (ROWS, K, 4)
    fake.calls.clear()
    out = f.run_events(_events(), trajectory=0)    # a cap of no rows: the plain launch, the empty trajectory
    assert fake.calls == [_live(0), SYNC]
    assert out[2]["trajectory"].shape == (0, K, 4) and out[2]["record_times_ns"].shape == (0, K)


def test_run_session(fake, engine):
    ph2, ph3 = _session()
    f = engine.BatchedEKF(K)
    fake.calls.clear()
    out = engine.run_session(ph2, ph3, f)
    assert fake.calls == [_phase2(0), _live(0), SYNC]
    assert sorted(out) == ["counts", "ready", "refs"] and out["ready"].dtype == bool


def test_run_session_refuses_f32_records_of_f64_events(fake, engine):
    ph2, ph3 = _session()
    with pytest.raises(ValueError, match="FP64 events make FP64 records"):
        engine.run_session(ph2, ph3, engine.BatchedEKF(K), records="f32", events="f64")


def test_run_session_with_calibration_and_trajectory(fake, engine):
    ph2, ph3 = _session()
    f = engine.BatchedEKF(K)
    calib = dict(status=np.zeros(K, np.int32), calibrated=np.array([True, False, True, True]),
                 cal=engine.DeviceBuffer(96 * K), status_dev=engine.DeviceBuffer(4 * K))
    apply = ("pekf_magcal_apply_dev", (K, E, D, D, D, 0, None))
    fake.calls.clear()
    out = engine.run_session(ph2, ph3, f, calibration=calib)
    assert fake.calls == [apply, apply, _phase2(0), _live(0), SYNC]
    assert sorted(out) == ["calibrated", "counts", "ready", "refs"]
    assert out["calibrated"].tolist() == [True, False, True, True]
    fake.calls.clear()
    out = engine.run_session(ph2, ph3, f, n_avg=7, alpha=0.25, events="f64", calibration=calib)
    assert fake.calls == [("pekf_magcal_apply_dev", (K, E, D, D, D, 4, None))] * 2 + [
        ("pekf_frontend_init_ext_dev", (K, E, D, D, 7, D, D, None, D, 4, None)),
        ("pekf_live_ext_dev", (K, E, D, D, D, 0.25, D, D, 1.0, 0.1, D, D, 4, None, None)), SYNC]
    fake.calls.clear()
    out = engine.run_session(ph2, ph3, f, trajectory=True)
    assert fake.calls == [_phase2(0)] + _live_traj(0, ROWS) + [SYNC]
    assert sorted(out) == ["counts", "ready", "record_dt_ns", "record_times_ns", "refs", "trajectory"]
    assert out["trajectory"].shape == (ROWS, K, 4) and out["record_dt_ns"].shape == (ROWS, K)
    fake.calls.clear()
    out = engine.run_session(ph2, ph3, f, records="f32", trajectory=3, calibration=calib)
    assert fake.calls == [apply, apply, _phase2(0)] + _live_traj(2, 3) + [SYNC]
    assert sorted(out) == ["calibrated", "counts", "ready", "record_dt_ns", "record_times_ns", "refs", "trajectory"]


def _frontend(flags, dtx):
    return ("pekf_frontend_ext_dev", (K, E, D, D, D, 0.1, R_MAX, D, D, D, dtx, D, D, flags, D, None))


def test_run_frontend(fake, engine):
    fake.calls.clear()
    win, counts = engine.run_frontend(_events())   # the fake escapes a dt: one retry with the side plane
    assert fake.calls == [_frontend(0, None), SYNC, _frontend(0, D), SYNC]
    assert isinstance(win, engine.IMUWindow) and (win.batch, win.window) == (K, R_MAX)
    assert win.dtx is not None and win.dtx.nbytes == 8 * K * R_MAX and counts is win.counts
    fake.calls.clear()
    win, counts = engine.run_frontend(_events(), events="f64")
    assert fake.calls == [_frontend(4, None), SYNC]
    assert isinstance(win, engine.RecordWindow64) and (win.batch, win.window) == (K, R_MAX) and counts is win.counts
    fake.calls.clear()
    win, _ = engine.run_frontend(_events(), alpha=0.5, r_max=20, events="f64")
    assert fake.calls == [("pekf_frontend_ext_dev", (K, E, D, D, D, 0.5, 20, D, D, D, None, D, D, 4, D, None)), SYNC]
    assert win.window == 20


def test_frontend_init(fake, engine):
    fake.calls.clear()
    out = engine.frontend_init(_events())
    assert fake.calls == [_phase2(0, stats=D), SYNC]
    assert sorted(out) == ["gyro_mean", "init", "ready", "t_init", "var_acc", "var_gyro", "var_mag"]
    fake.calls.clear()
    out = engine.frontend_init(_events(), stats=False)
    assert fake.calls == [_phase2(0), SYNC]
    assert sorted(out) == ["init", "ready", "t_init"]
    fake.calls.clear()
    engine.frontend_init(_events(), n_avg=5, events="f64")
    assert fake.calls == [("pekf_frontend_init_ext_dev", (K, E, D, D, 5, D, D, D, D, 4, None)), SYNC]


def _windows(engine):
    rec = synth.generate(np.arange(K), E, seed=5)
    rng = np.random.default_rng(5)
    g, a, m = rng.standard_normal((3, E, K, 3))
    return (engine.IMUWindow.from_records(rec),
            engine.RecordWindow64.from_arrays(g, np.full((E, K), 1e6), a, m, rec.acc0, rec.mag0))


def test_window_side_outputs(fake, engine):
    win, win64 = _windows(engine)
    fake.calls.clear()
    q, traj = win.gyro_chain()
    assert fake.calls == [("pekf_gyro_chain_ext_dev", (K, E, E, 0, D, None, D, None, None)), SYNC]
    assert q.shape == (K, 4) and traj is None
    win.dtx = engine.DeviceBuffer(8 * E * K)
    fake.calls.clear()
    q, traj = win.gyro_chain(n_steps=7, step0=2, want_traj=True)
    assert fake.calls == [("pekf_gyro_chain_ext_dev", (K, 7, E, 2, D, D, D, D, None)), SYNC]
    assert traj.shape == (7, K, 4)
    fake.calls.clear()
    assert win.wahba_quaternions().shape == (E, K, 4)
    assert fake.calls == [("pekf_wahba_stream_dev", (K, E, E, 0, D, D, D, 0.5, 0.5, D, None)), SYNC]
    fake.calls.clear()
    assert win.wahba_quaternions(7, 2, 0.25, 0.75).shape == (7, K, 4)
    assert fake.calls == [("pekf_wahba_stream_dev", (K, 7, E, 2, D, D, D, 0.25, 0.75, D, None)), SYNC]

    fake.calls.clear()
    q, traj = win64.gyro_chain()
    assert fake.calls == [("pekf_gyro_chain_rec64_dev", (K, E, E, 0, D, D, None, None)), SYNC]
    assert q.shape == (K, 4) and traj is None
    fake.calls.clear()
    q, traj = win64.gyro_chain(n_steps=7, step0=2, want_traj=True)
    assert fake.calls == [("pekf_gyro_chain_rec64_dev", (K, 7, E, 2, D, D, D, None)), SYNC]
    assert traj.shape == (7, K, 4)
    fake.calls.clear()
    assert win64.wahba_quaternions().shape == (E, K, 4)
    assert fake.calls == [("pekf_wahba_stream_rec64_dev", (K, E, E, 0, D, D, D, 0.5, 0.5, D, None)), SYNC]
    fake.calls.clear()
    assert win64.wahba_quaternions(7, 2, 0.25, 0.75).shape == (7, K, 4)
    assert fake.calls == [("pekf_wahba_stream_rec64_dev", (K, 7, E, 2, D, D, D, 0.25, 0.75, D, None)), SYNC]
    assert win.nbytes == 40 * E * K and win64.nbytes == 80 * E * K


def test_runs_with_ragged_counts(fake, engine):
    """win.counts, shifted by step0 and clipped to the launch, is what both runs hand the kernel."""
    win, win64 = _windows(engine)
    win.counts = win64.counts = np.array([30, 5, 2, 1], np.int32)
    f = engine.BatchedEKF(K)
    fake.calls.clear()
    assert f.run(win, n_steps=20, step0=2) is None
    assert fake.calls == [("pekf_run_dev", (K, 20, E, 2, D, D, D, D, D, D, 1.0, 0.1, None, D, 0, None)), SYNC]
    assert fake.counts_seen.pop().tolist() == [20, 3, 0, 0]
    fake.calls.clear()
    assert f.run(win64, n_steps=20, step0=2, want_traj=True).shape == (20, K, 4)
    assert fake.calls == [("pekf_run_rec64_dev", (K, 20, E, 2, D, D, D, D, D, D, 1.0, 0.1, D, D, None)), SYNC]
    fake.calls.clear()
    f.run(win, n_steps=20, step0=2, counts=[1, 2, 3, 4])   # given counts are taken as they are
    assert fake.counts_seen.pop().tolist() == [1, 2, 3, 4]
    win.counts = None
    fake.calls.clear()
    f.run(win)
    assert fake.calls == [("pekf_run_dev", (K, E, E, 0, D, D, D, D, D, D, 1.0, 0.1, None, None, 0, None)), SYNC]
    assert fake.counts_seen == []

    rec = synth.generate(np.arange(K), 1, seed=5)
    h = engine.FilterHandle(rec.acc0, rec.mag0)
    try:
        win.counts = np.array([30, 5, 2, 1], np.int32)
        fake.calls.clear()
        assert h.run(win, n_steps=20, step0=2) is None
        assert fake.calls == [("pekf_filter_run_ext", (77, 20, E, 2, D, D, D, None, None, D, None)), SYNC]
        assert fake.counts_seen.pop().tolist() == [20, 3, 0, 0]
        win.counts, win.dtx = None, engine.DeviceBuffer(8 * E * K)
        fake.calls.clear()
        assert h.run(win, want_traj=True).shape == (E, K, 4)
        assert fake.calls == [("pekf_filter_run_ext", (77, E, E, 0, D, D, D, D, D, None, None)), SYNC]
    finally:
        h.close()


def test_flags_of_precision_and_layout(fake, engine):
    """The run flags both constructors derive: RUN_MIXED_PRECISION 1, RUN_STATE_SOA 2."""
    for precision, layout, flags in (("f64", "aos", 0), ("mixed", "aos", 1), ("f64", "soa", 2), ("mixed", "soa", 3)):
        assert engine.BatchedEKF(K, precision=precision, layout=layout).flags == flags
        fake.calls.clear()
        h = engine.FilterHandle(np.ones((K, 3)), np.ones((K, 3)), precision=precision, layout=layout)
        h.close()
        assert fake.create_flags == flags and fake.calls == [("pekf_filter_destroy", (77,))]
