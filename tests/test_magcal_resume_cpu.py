"""Chunked phase 1 (pekf_magcal_resume_dev, pekf_magcal_state_bytes, engine.CalibrationSession, PhoneSession's
n_cal), the parts a CPU can check: the entries are declared, bound and exported; the state's size; the arguments
refused before any device call; the calibrating PhoneSession's launches per chunk and its two refusals; and that
a session without n_cal makes exactly the calls it made."""
import re

import numpy as np
import pytest

from .test_capi import HEADER
from .test_phone_session_cpu import _Recorder, _chunk

P = 16  # a non-null, 16-byte aligned "pointer": every case is refused before anything is read or launched
TE, F32R, EV64 = 0x1, 0x2, 0x4


@pytest.fixture(scope="module")
def lib():
    from poseestimationkf_amd import _lib
    return _lib


def _args(batch=8, n_events=8, ev=P, n_cal=20, cal=P, fit=P, status=P, flags=0, state=P, resume=0):
    return batch, n_events, ev, n_cal, cal, fit, status, flags, state, resume, None


def _names(text, entry, prefix="int "):
    m = re.search(r"^%s%s\(([^;]*)\);" % (prefix, entry), text, re.M | re.S)
    assert m, "include/pekf.h does not declare %s" % entry
    return [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]


def test_entries_are_declared_bound_and_exported(lib):
    text = open(HEADER).read()
    resume, one = _names(text, "pekf_magcal_resume_dev"), _names(text, "pekf_magcal_dev")
    # pekf_magcal_dev's arguments, plus state and resume before the stream
    assert resume == one[:-1] + ["state", "resume", "stream"]
    assert len(resume) == 11 == len(lib.SIGNATURES["pekf_magcal_resume_dev"])
    sig = list(lib.SIGNATURES["pekf_magcal_resume_dev"])
    assert sig[:8] + sig[10:] == lib.SIGNATURES["pekf_magcal_dev"]
    size = _names(text, "pekf_magcal_state_bytes", prefix="long long\nint ")   # 64 bits
    assert size == ["batch", "n_cal", "flags"] and len(lib.SIGNATURES["pekf_magcal_state_bytes"]) == 3
    for name in ("pekf_magcal_resume_dev", "pekf_magcal_state_bytes"):
        assert hasattr(lib.lib, name)
    assert lib.lib.pekf_magcal_state_bytes.restype is lib._i64
    assert lib.lib.pekf_abi_version() == 1
    # the header says what a caller must keep fixed, and cites the reference's state
    assert "n_cal MUST BE THE SAME" in text and "KFS/Magnetometer_Calibration.cpp:13-43" in text


def test_state_bytes(lib):
    size = lib.lib.pekf_magcal_state_bytes
    for flags in (0, TE, EV64, EV64 | TE):
        for n_cal in (6, 7, 20, 99, 100, 101, 1000, (1 << 30) - 1):
            one = size(1, n_cal, flags)
            assert one > 0 and one % 16 == 0
            # the sums and the count, n_cal samples of three doubles; at most a whole 32 B event per sample
            assert 24 * n_cal + 28 <= one <= 32 * n_cal + 64
            for batch in (2, 70, 1000, 1 << 20):
                assert size(batch, n_cal, flags) == batch * one
            assert size(0, n_cal, flags) == 0
        assert size(1, 100, flags) == size(1, 100, 0)          # both event forms keep doubles
    assert size(1 << 27, 1 << 20, 0) > 1 << 32                 # 64 bits
    for bad in (F32R, F32R | TE, 0x8, 0x100, EV64 | F32R):
        assert size(64, 100, bad) < 0
    for n_cal in (5, 0, -1, 1 << 30):
        assert size(64, n_cal, 0) < 0 and size(64, n_cal, EV64) < 0
    assert size(-1, 100, 0) < 0 and size(-1, 100, EV64) < 0


def test_arguments_are_refused_before_any_device_call(lib):
    L, bad = lib.lib, lib.PEKF_ERR_INVALID
    f = L.pekf_magcal_resume_dev
    for resume in (0, 1):
        assert f(*_args(state=None, resume=resume)) == bad and "state must be" in lib.last_error()
        assert f(*_args(state=P + 8, resume=resume)) == bad and "state must be" in lib.last_error()
        assert f(*_args(n_cal=5, resume=resume)) == bad and "n_cal" in lib.last_error()
        assert f(*_args(n_cal=1 << 30, resume=resume)) == bad and "n_cal" in lib.last_error()
        for flags in (F32R, 0x8, EV64 | F32R):
            assert f(*_args(flags=flags, resume=resume)) == bad and "unknown flags" in lib.last_error()
        assert f(*_args(batch=-1, resume=resume)) == bad and "negative size" in lib.last_error()
        assert f(*_args(n_events=-1, resume=resume)) == bad and "negative size" in lib.last_error()
        assert f(*_args(n_events=1 << 30, resume=resume)) == bad and "2^30" in lib.last_error()
        assert f(*_args(ev=P + 8, resume=resume)) == bad and "misaligned event planes" in lib.last_error()
        assert f(*_args(ev=None, resume=resume)) == bad and "null pointer" in lib.last_error()
        assert f(*_args(cal=None, resume=resume)) == bad and "null pointer" in lib.last_error()
        assert f(*_args(status=None, resume=resume)) == bad and "null pointer" in lib.last_error()
        assert f(*_args(batch=0, flags=EV64, resume=resume)) == lib.PEKF_OK
        assert f(*_args(batch=0, n_events=0, ev=None, fit=None, resume=resume)) == lib.PEKF_OK
        # a state is required even where nothing would be launched
        assert f(*_args(batch=0, state=None, resume=resume)) == bad and "state must be" in lib.last_error()
    # pekf_magcal_dev is what it was
    assert L.pekf_magcal_dev(0, 8, P, 20, P, P, P, EV64, None) == lib.PEKF_OK
    assert L.pekf_magcal_dev(8, 8, P, 5, P, P, P, 0, None) == bad


class _CalRecorder:
    """test_phone_session_cpu's recording fake with phase 1's entries: the resume launch and the correction record
    what they were handed"""

    def __new__(cls):
        Base = type(_Recorder())

        class Fake(Base):
            replies = []

            def pekf_magcal_state_bytes(self, batch, n_cal, flags):
                return batch * (32 + 24 * n_cal + 8 * (n_cal & 1)) if n_cal >= 6 else -1

            def pekf_magcal_resume_dev(self, batch, n, ev, n_cal, cal, fit, status, flags, state, resume, stream):
                self.calls.append(dict(entry="magcal_resume", n=n, flags=flags, resume=resume, n_cal=n_cal, ev=ev,
                                       cal=cal, fit=fit, status=status, state=state,
                                       planes=self._view(ev, n * batch * 32).copy() if n else None))
                return 0

            def pekf_magcal_apply_dev(self, batch, n, ev, cal, status, flags, stream):
                self.calls.append(dict(entry="apply", n=n, flags=flags, ev=ev, cal=cal, status=status))
                return 0
        return Fake(1)


def _install(monkeypatch, fake):
    from poseestimationkf_amd import _lib, engine
    for mod in (_lib, engine):
        monkeypatch.setattr(mod, "lib", fake)


def _replies(K, n):
    return [(np.zeros(K, np.int64), [0] * K, np.zeros(K, np.int32), None) for _ in range(n)]


def test_calibrating_session_launches_phase1_then_apply_phase2_and_the_join(monkeypatch):
    from poseestimationkf_amd import engine, synth
    fake = _CalRecorder()
    _install(monkeypatch, fake)
    K, E = 4, 12
    ev = dict(synth.generate_events(np.arange(K), E, seed=3))
    p1 = dict(synth.generate_calibration_events(K, 9, seed=5))
    s = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5, n_cal=7)
    assert s.n_cal == 7
    fake.calls.clear()
    fake.replies[:] = _replies(K, 5)
    empty = dict(types=ev["types"][:0], values=ev["values"][:0], times=ev["times"][:0])
    s.feed(None, None, phase1=_chunk(p1, 0, 5))                    # phase 1 alone
    s.feed(_chunk(ev, 0, 5), None, phase1=_chunk(p1, 5, 9))        # phase 1 and phase 2
    s.feed(_chunk(ev, 5, 12), _chunk(ev, 0, 4))                    # no phase-1 rows: no phase-1 launch
    s.feed(None, _chunk(ev, 4, 12), phase1=empty)                  # an empty phase-1 chunk is none
    s.feed(None, empty, phase1=_chunk(p1, 0, 1))                   # late phase-1 rows are still fed
    calls = fake.calls
    assert [c["entry"] for c in calls] == ["magcal_resume", "phase2", "join",
                                           "magcal_resume", "apply", "phase2", "join",
                                           "apply", "apply", "phase2", "join",
                                           "apply", "phase2", "join",
                                           "magcal_resume", "phase2", "join"]
    m = [c for c in calls if c["entry"] == "magcal_resume"]
    assert [c["resume"] for c in m] == [0, 1, 1] and [c["n"] for c in m] == [5, 4, 1]
    assert all(c["n_cal"] == 7 and c["flags"] == EV64 for c in m)
    assert len({(c["cal"], c["fit"], c["status"], c["state"]) for c in m}) == 1    # the session's own buffers
    for c, (a, b) in zip(m, ((0, 5), (5, 9), (0, 1))):
        want = synth.pack_events64(_chunk(p1, a, b), engine.server_event_values(_chunk(p1, a, b)))
        assert c["planes"].tobytes() == want.tobytes()
    ap = [c for c in calls if c["entry"] == "apply"]
    assert [c["n"] for c in ap] == [5, 7, 4, 8]
    assert all((c["cal"], c["status"]) == (m[0]["cal"], m[0]["status"]) and c["flags"] == EV64 for c in ap)
    # the correction is handed the rows phase 2 / the join then read
    later = {id(c): calls[i + 1:] for i, c in enumerate(calls)}
    for c in ap:
        assert any(x["entry"] in ("phase2", "join") and x["ev"] == c["ev"] and x["n"] == c["n"] for x in later[id(c)][:3])
    assert [c["resume"] for c in calls if c["entry"] == "phase2"] == [0, 1, 1, 1, 1]


def test_first_chunk_without_phase1_rows_still_launches_phase1(monkeypatch):
    from poseestimationkf_amd import engine, synth
    fake = _CalRecorder()
    _install(monkeypatch, fake)
    K = 4
    ev = dict(synth.generate_events(np.arange(K), 6, seed=3))
    s = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5, n_cal=7)
    fake.calls.clear()
    fake.replies[:] = _replies(K, 2)
    s.feed(_chunk(ev, 0, 3), None)
    s.feed(_chunk(ev, 3, 6), None)
    assert [c["entry"] for c in fake.calls] == ["magcal_resume", "apply", "phase2", "join", "apply", "phase2", "join"]
    assert fake.calls[0]["n"] == 0 and fake.calls[0]["resume"] == 0 and not fake.calls[0]["ev"]


def test_the_two_refusals_launch_nothing(monkeypatch):
    from poseestimationkf_amd import engine, synth
    fake = _CalRecorder()
    _install(monkeypatch, fake)
    K = 4
    ev = dict(synth.generate_events(np.arange(K), 6, seed=3))
    p1 = dict(synth.generate_calibration_events(K, 9, seed=5))
    buf = engine.DeviceBuffer(32 * K * 6)
    frames = np.full((3, K, 100), ord(" "), np.uint8)
    cal = dict(cal=buf, status_dev=buf)
    calibrating = engine.PhoneSession(engine.BatchedEKF(K), n_cal=7)
    plain = engine.PhoneSession(engine.BatchedEKF(K))
    assert plain.n_cal is None and plain.calibration is None
    fake.calls.clear()
    for call in (lambda: calibrating.feed(_chunk(ev, 0, 6), None, calibration=cal),
                 lambda: calibrating.feed(None, None, calibration=cal, phase1=_chunk(p1, 0, 9)),
                 lambda: calibrating.feed_planes(buf, 6, None, 0, calibration=cal),
                 lambda: calibrating.feed_frames(frames, calibration=cal),
                 lambda: calibrating.feed_frames(frames, calibration="frames")):
        with pytest.raises(ValueError, match="takes no calibration="):
            call()
    for call in (lambda: plain.feed(_chunk(ev, 0, 6), None, phase1=_chunk(p1, 0, 9)),
                 lambda: plain.feed_planes(buf, 6, None, 0, planes1=buf, n1=6),
                 lambda: plain.feed_planes(buf, 6, None, 0, n1=1)):
        with pytest.raises(ValueError, match="construct the session with n_cal="):
            call()
    with pytest.raises(ValueError, match="not chunked"):
        plain.feed_frames(frames, calibration="frames")
    with pytest.raises(ValueError, match="outside the planes buffer"):
        calibrating.feed_planes(None, 0, None, 0, planes1=buf, n1=7)
    with pytest.raises(ValueError, match="phase1 is of"):
        calibrating.feed(None, None, phase1=_chunk(dict(synth.generate_calibration_events(K + 1, 3, seed=5)), 0, 3))
    with pytest.raises(ValueError, match="n_cal"):
        engine.PhoneSession(engine.BatchedEKF(K), n_cal=5)
    assert fake.calls == []                                     # nothing was launched


def test_a_session_without_n_cal_makes_the_calls_it_made(monkeypatch):
    """The plain recorder has no phase-1 entry at all: a session without n_cal that touched one would raise."""
    from poseestimationkf_amd import engine, synth
    fake = _Recorder()
    _install(monkeypatch, fake)
    assert not hasattr(type(fake), "pekf_magcal_state_bytes")
    K, E = 4, 12
    ev = dict(synth.generate_events(np.arange(K), E, seed=3))
    s = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5)
    fake.calls.clear()
    fake.replies[:] = _replies(K, 2)
    applied = []
    fake.pekf_magcal_apply_dev = lambda *a: applied.append(a[1]) or 0
    buf = engine.DeviceBuffer(96 * K)
    s.feed(_chunk(ev, 0, 5), _chunk(ev, 0, 4))
    s.feed(_chunk(ev, 5, 12), _chunk(ev, 4, 12), calibration=dict(cal=buf, status_dev=buf))
    assert [c["entry"] for c in fake.calls] == ["phase2", "join"] * 2 and applied == [7, 8]
    assert [c["resume"] for c in fake.calls[0::2]] == [0, 1]
    snap = s.snapshot()
    assert sorted(snap) == sorted(["batch", "q", "r", "X", "P", "book", "n_avg", "alpha", "p2state", "state", "t_start",
                                   "init", "t_init", "ready", "refs"])
    # and the calibrating session's snapshot adds phase 1's state, outputs and n_cal
    fake2 = _CalRecorder()
    _install(monkeypatch, fake2)
    c = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5, n_cal=7)
    snap2 = c.snapshot()
    assert sorted(set(snap2) - set(snap)) == ["cal", "fit", "n_cal", "p1state", "status"] and snap2["n_cal"] == 7
    assert snap2["p1state"].nbytes == fake2.pekf_magcal_state_bytes(K, 7, EV64)
    r = engine.PhoneSession.restore(engine.BatchedEKF(K), snap2)
    assert r.n_cal == 7 and sorted(r.snapshot()) == sorted(snap2)
