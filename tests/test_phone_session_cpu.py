"""Live sessions from a phone's first message (pekf_frontend_init_resume_dev, pekf_frontend_init_state_bytes,
pekf_live_join_dev, engine.PhoneSession), the parts a CPU can check: the entries are declared, bound and
exported; the phase-2 state's size; the arguments refused before any device call; PhoneSession's refusals and
its host bookkeeping (the two launches per chunk and what they are handed, the record times)."""
import re

import numpy as np
import pytest

from .test_capi import HEADER

P = 16  # a non-null, 16-byte aligned "pointer": every case is refused before anything is read or launched
TE, F32R, EV64 = 0x1, 0x2, 0x4


@pytest.fixture(scope="module")
def lib():
    from poseestimationkf_amd import _lib
    return _lib


def _init_args(batch=8, n_events=8, ev=P, t_start=P, n_avg=5, init=P, t_init=P, ready=P, flags=0, state=P, resume=0):
    return batch, n_events, ev, t_start, n_avg, init, t_init, ready, flags, state, resume, None


def _join_args(batch=8, n_events=8, ev=P, flags=EV64, state=P, traj=P, traj_dt=P, traj_rows=4, r=0.1):
    return batch, n_events, ev, P, P, 0.1, P, P, 1.0, r, P, P, flags, state, traj, traj_dt, traj_rows, None, None


def test_entries_are_declared_bound_and_exported(lib):
    text = open(HEADER).read()
    m = re.search(r"^int pekf_frontend_init_resume_dev\(([^;]*)\);", text, re.M | re.S)
    assert m, "include/pekf.h does not declare pekf_frontend_init_resume_dev"
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["batch", "n_events", "ev_planes", "t_start", "n_avg", "init", "t_init", "ready", "flags", "state",
                      "resume", "stream"]
    assert "stats" not in params and len(params) == len(lib.SIGNATURES["pekf_frontend_init_resume_dev"])
    m = re.search(r"^long long\nint pekf_frontend_init_state_bytes\(([^;]*)\);", text, re.M | re.S)   # 64 bits
    assert m and len(m.group(1).split(",")) == 2 == len(lib.SIGNATURES["pekf_frontend_init_state_bytes"])
    # pekf_live_join_dev: pekf_live_resume_dev's arguments minus resume
    join = re.search(r"^int pekf_live_join_dev\(([^;]*)\);", text, re.M | re.S)
    resume = re.search(r"^int pekf_live_resume_dev\(([^;]*)\);", text, re.M | re.S)
    assert join and resume
    names = [[p.strip().split()[-1].lstrip("*") for p in g.group(1).replace("\n", " ").split(",")] for g in (join, resume)]
    assert names[0] == [n for n in names[1] if n != "resume"] and len(names[1]) == 20
    assert len(names[0]) == 19 == len(lib.SIGNATURES["pekf_live_join_dev"])
    sig = list(lib.SIGNATURES["pekf_live_resume_dev"])
    del sig[names[1].index("resume")]
    assert lib.SIGNATURES["pekf_live_join_dev"] == sig
    for name in ("pekf_frontend_init_resume_dev", "pekf_frontend_init_state_bytes", "pekf_live_join_dev"):
        assert hasattr(lib.lib, name)
    assert lib.lib.pekf_abi_version() == 1
    # the restrictions are stated where a user meets them
    assert "NO VARIANCES" in text and "FP64 events only" in text


def test_phase2_state_bytes(lib):
    size = lib.lib.pekf_frontend_init_state_bytes
    for flags in (0, TE, EV64, EV64 | TE):         # what pekf_frontend_init_ext_dev takes
        one = size(1, flags)
        assert one > 0 and one % 16 == 0           # whole 16-byte planes per phone
        for batch in (2, 70, 1000, 1 << 20):
            assert size(batch, flags) == batch * one
        assert size(0, flags) == 0
        # 9 doubles (the sums), 2 clocks, 3 counts and the 4 flags
        assert one >= 9 * 8 + 2 * 8 + 3 * 4 + 1
    for bad in (F32R, F32R | TE, 0x8, 0x100, EV64 | F32R):
        assert size(64, bad) < 0
    assert size(-1, 0) < 0 and size(-1, EV64) < 0


def test_phase2_arguments_are_refused_before_any_device_call(lib):
    L, bad = lib.lib, lib.PEKF_ERR_INVALID
    f = L.pekf_frontend_init_resume_dev
    assert f(*_init_args(state=None)) == bad and "state must be" in lib.last_error()
    assert f(*_init_args(state=P + 8)) == bad and "state must be" in lib.last_error()
    assert f(*_init_args(state=None, resume=1)) == bad and "state must be" in lib.last_error()
    assert f(*_init_args(n_avg=1)) == bad and "n_avg" in lib.last_error()
    assert f(*_init_args(n_avg=0, resume=1)) == bad and "n_avg" in lib.last_error()
    for flags in (F32R, 0x8, EV64 | F32R):
        assert f(*_init_args(flags=flags)) == bad and "unknown flags" in lib.last_error()
    assert f(*_init_args(batch=-1)) == bad and "negative size" in lib.last_error()
    assert f(*_init_args(n_events=-1)) == bad and "negative size" in lib.last_error()
    assert f(*_init_args(n_events=1 << 30)) == bad and "2^30" in lib.last_error()
    assert f(*_init_args(batch=1 << 28)) == bad and "batch must be" in lib.last_error()
    assert f(*_init_args(ev=None)) == bad and "null pointer" in lib.last_error()
    assert f(*_init_args(init=None)) == bad and "null pointer" in lib.last_error()
    assert f(*_init_args(t_start=None)) == bad and "null pointer" in lib.last_error()   # read when a session starts
    assert f(*_init_args(ev=P + 8)) == bad and "misaligned event planes" in lib.last_error()
    assert f(*_init_args(batch=0)) == lib.PEKF_OK
    assert f(*_init_args(batch=0, flags=EV64, resume=1, t_start=None)) == lib.PEKF_OK


def test_join_arguments_are_refused_before_any_device_call(lib):
    L, bad = lib.lib, lib.PEKF_ERR_INVALID
    f = L.pekf_live_join_dev
    for flags in (0, TE, F32R, EV64 | TE, EV64 | F32R):    # FP64 events only
        assert f(*_join_args(flags=flags)) == bad
        assert "PEKF_EV_F64_EVENTS" in lib.last_error(), flags
    assert f(*_join_args(flags=0x8)) == bad and "unknown flags" in lib.last_error()
    assert f(*_join_args(state=None)) == bad and "state must be" in lib.last_error()
    assert f(*_join_args(state=P + 8)) == bad and "state must be" in lib.last_error()
    # pekf_live_traj_dev's own checks, as pekf_live_resume_dev has them
    assert f(*_join_args(batch=-1)) == bad and "negative size" in lib.last_error()
    assert f(*_join_args(traj_rows=-1)) == bad and "traj_rows" in lib.last_error()
    assert f(*_join_args(traj=None)) == bad and "traj must be" in lib.last_error()
    assert f(*_join_args(traj_dt=P + 4)) == bad and "traj_dt" in lib.last_error()
    assert f(*_join_args(batch=1 << 28)) == bad and "batch must be" in lib.last_error()
    assert f(*_join_args(n_events=1 << 30)) == bad and "n_events must be" in lib.last_error()
    assert f(*_join_args(ev=None)) == bad and "null pointer" in lib.last_error()
    assert f(*_join_args(ev=P + 8)) == bad and "misaligned event planes" in lib.last_error()
    assert f(*_join_args(r=0.0, traj=None, traj_dt=None, traj_rows=0)) == bad and "r must be > 0" in lib.last_error()
    assert f(*_join_args(batch=0)) == lib.PEKF_OK
    # pekf_live_resume_dev is what it was: 20 parameters, resume 0 / nonzero, FP64 events among its forms
    assert L.pekf_live_resume_dev(0, 8, P, P, P, 0.1, P, P, 1.0, 0.1, P, P, EV64, P, 1, None, None, 0, None,
                                  None) == lib.PEKF_OK


class _Recorder:
    """fake_libpekf with the session's entries: the two launches record their arguments and play back the phase-2
    outputs, counts and dts the test queued for them"""

    def __new__(cls):
        from . import fake_libpekf

        class Fake(fake_libpekf.FakeLib):
            replies = []

            def pekf_live_state_bytes(self, batch, flags):
                return batch * 336 if flags == EV64 else -1

            def pekf_frontend_init_state_bytes(self, batch, flags):
                return batch * 112

            def pekf_memset(self, p, value, n, stream):
                self._view(p, n)[:] = value
                return 0

            def pekf_frontend_init_resume_dev(self, batch, n, ev, t_start, n_avg, init, t_init, ready, flags, state,
                                              resume, stream):
                self.calls.append(dict(entry="phase2", n=n, flags=flags, resume=resume, n_avg=n_avg, ev=ev,
                                       planes=self._view(ev, n * batch * 32).copy() if n else None))
                self.reply = self.replies.pop(0)
                self._view(t_init, 8 * batch, np.int64)[:] = self.reply[0]
                self._view(ready, 4 * batch, np.int32)[:] = self.reply[1]
                return 0

            def pekf_live_join_dev(self, batch, n, ev, init, t_init, alpha, X, Pm, q, r, counts, refs, flags, state,
                                   traj, traj_dt, rows, err, stream):
                zeroed = not self._view(state, 336 * batch).any()
                self.calls.append(dict(entry="join", n=n, flags=flags, rows=rows, zeroed=zeroed, ev=ev,
                                       planes=self._view(ev, n * batch * 32).copy() if n else None))
                c, dt = self.reply[2], self.reply[3]
                self._view(counts, 4 * batch, np.int32)[:] = c
                if rows and dt is not None:
                    self._view(traj_dt, 8 * rows * batch, np.float64).reshape(rows, batch)[:len(dt)] = dt
                return 0
        return Fake(1)


def _chunk(ev, a, b):
    return dict(types=ev["types"][a:b], values=ev["values"][a:b], times=ev["times"][a:b],
                values64=ev["values"][a:b].astype(np.float64))   # (the server's parse is not what is checked here)


def test_feed_launches_phase2_then_the_join_and_chains_the_record_times(monkeypatch):
    from poseestimationkf_amd import _lib, engine, synth
    fake = _Recorder()
    for mod in (_lib, engine):
        monkeypatch.setattr(mod, "lib", fake)
    K, E = 4, 12
    ev = dict(synth.generate_events(np.arange(K), E, seed=3))
    s = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5)
    fake.calls.clear()
    nan = np.nan
    t0, t1, t2 = np.array([10, 20, 30, 40]), np.array([11, 21, 31, 41]), np.array([12, 22, 32, 42])
    fake.replies[:] = [(t0, [1, 0, 1, 0], np.array([1, 0, 0, 0], np.int32), np.array([[5.0, nan, nan, nan]])),
                       (t1, [1, 1, 1, 0], np.zeros(K, np.int32), None),
                       (t2, [1, 1, 1, 0], np.array([2, 1, 0, 0], np.int32), np.array([[1.0, 7.0, nan, nan],
                                                                                       [2.0, nan, nan, nan]]))]
    outs = [s.feed(_chunk(ev, 0, 5), _chunk(ev, 0, 4), trajectory=True),
            s.feed(None, dict(types=ev["types"][:0], values=ev["values"][:0], times=ev["times"][:0]), trajectory=True),
            s.feed(_chunk(ev, 5, 12), _chunk(ev, 4, 12), trajectory=True)]
    calls = fake.calls
    assert [c["entry"] for c in calls] == ["phase2", "join"] * 3
    assert [c["n"] for c in calls] == [5, 4, 0, 0, 7, 8]
    assert all(c["flags"] == EV64 for c in calls)
    assert [c["resume"] for c in calls[0::2]] == [0, 1, 1] and all(c["n_avg"] == 5 for c in calls[0::2])
    assert [c["rows"] for c in calls[1::2]] == [2, 0, 3]
    assert calls[1]["zeroed"]                                   # the caller zeroes the state before the first call
    assert calls[3]["ev"]                                       # no rows: still a valid pointer
    for c, (a, b) in zip((calls[0], calls[1], calls[4], calls[5]), ((0, 5), (0, 4), (5, 12), (4, 12))):
        want = synth.pack_events64(_chunk(ev, a, b), engine.server_event_values(_chunk(ev, a, b)))
        assert c["planes"].tobytes() == want.tobytes()
    assert [np.array_equal(o[1], r) for o, r in zip(outs, ([1, 0, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0]))] == [True] * 3
    assert np.array_equal(s.total_counts, [3, 1, 0, 0])
    # a phone's record times start from the t_init of the chunk in which it applied its first record
    assert np.array_equal(outs[0][2]["record_times_ns"][:, 0], [15.0, nan], equal_nan=True)
    assert np.array_equal(outs[2][2]["record_times_ns"][:2, 0], [16.0, 18.0])
    assert np.array_equal(outs[2][2]["record_times_ns"][:, 1], [29.0, nan, nan], equal_nan=True)
    assert all(np.isnan(o[2]["record_times_ns"][:, 2:]).all() for o in outs)


def test_phone_session_refusals(monkeypatch):
    from poseestimationkf_amd import _lib, engine, synth
    fake = _Recorder()
    for mod in (_lib, engine):
        monkeypatch.setattr(mod, "lib", fake)
    K = 4
    fake.pekf_state_layout_dev = lambda *a: 0
    with pytest.raises(ValueError, match="AoS"):
        engine.PhoneSession(engine.BatchedEKF(K, layout="soa"))
    with pytest.raises(ValueError, match="FP64 filter"):
        engine.PhoneSession(engine.BatchedEKF(K, precision="mixed"))
    s = engine.PhoneSession(engine.BatchedEKF(K))
    fake.calls.clear()
    frames = np.full((3, K, 100), ord(" "), np.uint8)
    with pytest.raises(ValueError, match="not chunked"):
        s.feed_frames(frames, calibration="frames")
    with pytest.raises(ValueError, match="5 phones"):
        s.feed_frames(np.full((3, K + 1, 100), ord(" "), np.uint8))
    ev = synth.generate_events(np.arange(K + 1), 6, seed=3)
    with pytest.raises(ValueError, match="phase2 is of"):
        s.feed(_chunk(ev, 0, 6), None)
    with pytest.raises(ValueError, match="phase3 is of"):
        s.feed(None, _chunk(ev, 0, 6))
    buf = engine.DeviceBuffer(32 * K * 6)
    with pytest.raises(ValueError, match="outside the planes buffer"):
        s.feed_planes(buf, 7, buf, 6)
    with pytest.raises(ValueError, match="outside the planes buffer"):
        s.feed_planes(buf, 6, buf, 6, offset3=8)
    with pytest.raises(ValueError, match="outside the planes buffer"):
        s.feed_planes(None, 1, buf, 6)
    assert fake.calls == []                                     # nothing was launched
