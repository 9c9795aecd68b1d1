"""Phase 1 from wire frames without a GPU: pekf_wire_events_p1_dev's argument checks against the real library
(they return before any device call) and the call sequences of engine.wire_events(phase1=...) and
engine.run_wire_session(calibration="frames") with a recording fake of the library."""
import numpy as np
import pytest

from poseestimationkf_amd import wire  # noqa: F401  (binds the real library before any fake is installed)


@pytest.fixture(scope="module")
def lib():
    from poseestimationkf_amd import _lib
    return _lib


P = 4096  # a non-null, 16-byte aligned address; every call below returns before anything reads it
ROWS = 1  # PEKF_WIRE_FRAME_ROWS


def _args(batch=8, n_frames=8, frames=P, e1=8, e2=8, e3=8, ev1=P, ev2=P, ev3=P, first_t2=P, n1=P, n2=P, n3=P,
          bad=P, err=P, bounds=P, flags=0):
    return (batch, n_frames, frames, e1, e2, e3, ev1, ev2, ev3, first_t2, n1, n2, n3, bad, err, bounds, flags, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(batch=-1), "negative size"),
    (dict(n_frames=-1), "negative size"),
    (dict(e1=-1), "negative size"),
    (dict(e3=-1), "negative size"),
    (dict(flags=0x2), "unknown flags"),
    (dict(flags=0x80000000), "unknown flags"),
    (dict(ev1=None), "null pointer"),
    (dict(n1=None), "null pointer"),
    (dict(ev2=None), "null pointer"),
    (dict(n3=None), "null pointer"),
    (dict(frames=None), "null pointer"),
    (dict(ev1=P + 8), "misaligned"),
    (dict(ev3=P + 8), "misaligned"),
    (dict(frames=P + 2), "misaligned"),
    (dict(flags=ROWS, e1=7), "PEKF_WIRE_FRAME_ROWS"),
    (dict(flags=ROWS, e2=7), "PEKF_WIRE_FRAME_ROWS"),
    (dict(e1=1 << 31), "2^31"),
    (dict(n_frames=1 << 31, e1=1 << 31, e2=1 << 31, e3=1 << 31, flags=ROWS), "2^31"),
])
def test_wire_events_p1_arguments_are_checked(lib, kw, msg):
    assert lib.lib.pekf_wire_events_p1_dev(*_args(**kw)) == lib.PEKF_ERR_INVALID
    assert msg in lib.last_error()


def test_wire_events_p1_empty_batch_is_ok(lib):
    assert lib.lib.pekf_wire_events_p1_dev(*_args(batch=0, frames=None, ev1=None, ev2=None, ev3=None, first_t2=None,
                                                  n1=None, n2=None, n3=None, bad=None, err=None,
                                                  bounds=None)) == lib.PEKF_OK
    # compacted planes may be shorter than the frames (the extra messages are dropped and reported on the device)
    assert lib.lib.pekf_wire_events_p1_dev(*_args(batch=0, e1=3, e2=2, e3=1)) == lib.PEKF_OK


def test_the_older_entries_take_no_phase1_plane(lib):
    """pekf_wire_events_ext_dev's checks are what they were: its planes alone, in the same order."""
    L = lib.lib
    assert L.pekf_wire_events_ext_dev(8, 8, P, 8, 8, P, P, P, P, P, P, P, P, 0x2, None) == lib.PEKF_ERR_INVALID
    assert "unknown flags" in lib.last_error()
    assert L.pekf_wire_events_ext_dev(8, 8, P, 7, 8, P, P, P, P, P, P, P, P, ROWS, None) == lib.PEKF_ERR_INVALID
    assert "PEKF_WIRE_FRAME_ROWS" in lib.last_error()
    assert L.pekf_wire_events_ext_dev(8, 8, P, 8, 8, P, P, P, None, P, P, P, P, 0, None) == lib.PEKF_ERR_INVALID
    assert "null pointer" in lib.last_error()
    assert L.pekf_wire_events_ext_dev(0, 8, None, 8, 8, None, None, None, None, None, None, None, None, 0,
                                      None) == lib.PEKF_OK


# ------------------------------------------------------------------ the call sequences

RECORDED = ("pekf_frontend_init_ext_dev", "pekf_live_ext_dev", "pekf_magcal_dev", "pekf_magcal_apply_dev",
            "pekf_wire_events_ext_dev", "pekf_wire_events_p1_dev")


def _recording_fake(monkeypatch):
    """tests/fake_libpekf.py's host fake with the session's entry points recorded (they compute nothing)."""
    from . import fake_libpekf

    class Fake(fake_libpekf.FakeLib):
        def _rec(self, name):
            def f(*a):
                self.calls.append(name)
                return 0
            return f

        def __getattr__(self, name):
            if name in RECORDED:
                return self._rec(name)
            raise AttributeError("fake libpekf has no %s" % name)

    from poseestimationkf_amd import _lib, engine, shard
    fake = Fake(1)
    for mod in (_lib, engine, shard):
        monkeypatch.setattr(mod, "lib", fake)
    return fake, engine


@pytest.mark.parametrize("frame_rows", [False, True])
def test_session_calibrated_from_its_frames_is_one_chain_of_launches(monkeypatch, frame_rows):
    """calibration="frames": the parse with the phase-1 plane, the fit, one correction per plane, phase 2, the
    fused phase 3 -- and nothing else; the result carries calibrate_magnetometer's dict."""
    fake, engine = _recording_fake(monkeypatch)
    K = 8
    frames = np.full((4, K, 100), ord(" "), np.uint8)
    out = engine.run_wire_session(frames, engine.BatchedEKF(K), frame_rows=frame_rows, calibration="frames")
    assert fake.calls == ["pekf_wire_events_p1_dev", "pekf_magcal_dev", "pekf_magcal_apply_dev",
                          "pekf_magcal_apply_dev", "pekf_frontend_init_ext_dev", "pekf_live_ext_dev"]
    assert sorted(out) == ["calibrated", "calibration", "counts", "ready", "refs"]
    cal = out["calibration"]
    assert sorted(cal) == ["W", "bias", "cal", "calibrated", "fit", "status", "status_dev"]
    assert cal["bias"].shape == (K, 3) and cal["W"].shape == (K, 3, 3) and cal["fit"].shape == (K, 6)
    assert cal["status"].shape == (K,) and np.array_equal(out["calibrated"], cal["calibrated"])


def test_an_unknown_calibration_string_is_refused_before_any_launch(monkeypatch):
    fake, engine = _recording_fake(monkeypatch)
    frames = np.full((4, 8, 100), ord(" "), np.uint8)
    with pytest.raises(ValueError, match="calibration"):
        engine.run_wire_session(frames, engine.BatchedEKF(8), calibration="nonsense")
    assert fake.calls == []


def test_wire_events_without_phase1_is_the_older_entry(monkeypatch):
    fake, engine = _recording_fake(monkeypatch)
    frames = np.full((4, 8, 100), ord(" "), np.uint8)
    for rows in (False, True):
        fake.calls.clear()
        w = engine.wire_events(frames, frame_rows=rows)
        assert fake.calls == ["pekf_wire_events_ext_dev"]
        assert not {"ev1", "E1", "n1"} & set(w)
        fake.calls.clear()
        w = engine.wire_events(frames, frame_rows=rows, phase1=True)
        assert fake.calls == ["pekf_wire_events_p1_dev"]
        assert {"ev1", "E1", "n1"} <= set(w) and w["n1"].shape == (8,)


def test_calibrate_magnetometer_is_one_fit_launch(monkeypatch):
    """The event-dict path goes through the same launch helper: one pekf_magcal_dev, the same dict."""
    from poseestimationkf_amd import synth
    fake, engine = _recording_fake(monkeypatch)
    ev = synth.generate_calibration_events(5, 101, seed=3)
    for form in ("f32", "f64"):
        fake.calls.clear()
        got = engine.calibrate_magnetometer(ev, events=form)
        assert fake.calls == ["pekf_magcal_dev"]
        assert sorted(got) == ["W", "bias", "cal", "calibrated", "fit", "status", "status_dev"]
