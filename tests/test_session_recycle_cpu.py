"""Column recycling (pekf_session_recycle_dev, engine.PhoneSession.recycle, engine.CalibrationSession.recycle), the
parts a CPU can check: the entry is declared, bound and exported; every refusal of its arguments comes before any
device call and names the argument; the sessions' own refusals; what the launch is handed; and the host
bookkeeping of the recycled columns (the summed counts, the running record times)."""
import re

import numpy as np
import pytest

from .test_capi import HEADER

P = 16  # a non-null, 16-byte aligned "pointer": every case is refused before anything is read or launched
TE, F32R, EV64 = 0x1, 0x2, 0x4
PARAMS = ["batch", "n_cols", "cols", "flags", "live_state", "X", "P", "refs", "X0", "P0", "final_X", "final_P",
          "init_state", "t_start", "init", "t_init", "ready", "t_start_new", "magcal_state", "n_cal", "cal", "fit",
          "status", "stream"]


@pytest.fixture(scope="module")
def lib():
    from poseestimationkf_amd import _lib
    return _lib


def _args(batch=8, n_cols=3, cols=P, flags=EV64, live=(P, P, P, P), X0=None, P0=None, final_X=None, final_P=None,
          p2=(P, P, P, P, P), t_new=None, p1=(P, 20, P, P, P)):
    return (batch, n_cols, cols, flags) + tuple(live) + (X0, P0, final_X, final_P) + tuple(p2) + (t_new,) + tuple(p1) + (None,)


NO_LIVE, NO_P2, NO_P1 = (None,) * 4, (None,) * 5, (None, 0, None, None, None)


def test_entry_is_declared_bound_and_exported(lib):
    text = open(HEADER).read()
    m = re.search(r"^int pekf_session_recycle_dev\(([^;]*)\);", text, re.M | re.S)
    assert m, "include/pekf.h does not declare pekf_session_recycle_dev"
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    assert params == PARAMS
    assert len(params) == len(lib.SIGNATURES["pekf_session_recycle_dev"]) == len(_args())
    assert hasattr(lib.lib, "pekf_session_recycle_dev")
    assert lib.lib.pekf_abi_version() == 1
    # the comment says what it replaces: the reference's per-connection construction
    comment = text[:m.start()].rsplit("/*", 1)[1]
    for cite in ("KFS/Server.cpp:58", ":93", "KFS/Parser.h:93", "KFS/Magnetometer_Calibration.cpp:7-12"):
        assert cite in comment, cite


def test_arguments_are_refused_before_any_device_call(lib):
    bad = lib.PEKF_ERR_INVALID
    f = lib.lib.pekf_session_recycle_dev

    def refused(word, **kw):
        assert f(*_args(**kw)) == bad, kw
        assert word in lib.last_error(), (kw, lib.last_error())

    refused("negative size", batch=-1)
    refused("negative size", n_cols=-1)
    refused("batch must be", batch=1 << 28)
    refused("live_state must be", live=(P + 8, P, P, P))
    refused("init_state must be", p2=(P + 8, P, P, P, P))
    refused("magcal_state must be", p1=(P + 8, 20, P, P, P))
    # a half-given group, whichever pointer is missing -- the state's included
    for k in range(4):
        refused("filter group", live=tuple(None if j == k else P for j in range(4)))
    for k in range(5):
        refused("phase-2 group", p2=tuple(None if j == k else P for j in range(5)))
    for k in (0, 2, 3, 4):
        refused("phase-1 group", p1=tuple(None if j == k else v for j, v in enumerate((P, 20, P, P, P))))
    for n_cal in (5, 0, -1, 1 << 30):
        refused("n_cal", p1=(P, n_cal, P, P, P))
    for flags in (0, TE, F32R, EV64 | TE, EV64 | F32R, 0x8):
        refused("PEKF_EV_F64_EVENTS", flags=flags)
    refused("final_X and final_P", final_X=P)
    refused("final_X and final_P", final_P=P)
    refused("need the filter group", final_X=P, final_P=P, live=NO_LIVE)
    refused("X0 and P0", X0=P)
    refused("X0 and P0", P0=P)
    refused("need the filter group", X0=P, P0=P, live=NO_LIVE)
    refused("needs the phase-2 group", t_new=P, p2=NO_P2)
    refused("null pointer", cols=None)
    refused("n_cols must be <= batch", n_cols=9)


def test_what_needs_no_launch_is_ok(lib):
    f = lib.lib.pekf_session_recycle_dev
    assert f(*_args(n_cols=0)) == lib.PEKF_OK
    assert f(*_args(n_cols=0, cols=None)) == lib.PEKF_OK
    assert f(*_args(batch=0, n_cols=0)) == lib.PEKF_OK
    assert f(*_args(batch=0)) == lib.PEKF_OK
    # the phase-1 group does not depend on the event form; n_cal is checked only with it
    assert f(*_args(n_cols=0, flags=0, live=NO_LIVE, p2=NO_P2)) == lib.PEKF_OK
    assert f(*_args(n_cols=0, flags=TE, live=NO_LIVE, p2=NO_P2)) == lib.PEKF_OK
    assert f(*_args(n_cols=0, p1=NO_P1)) == lib.PEKF_OK
    assert f(*_args(live=NO_LIVE, p2=NO_P2, p1=NO_P1, flags=0)) == lib.PEKF_OK   # no group: nothing to do


class _Recorder:
    """fake_libpekf with the sessions' entries: the launches record their arguments; phase 2 and the join play back
    the outputs, counts and dts the test queued; the recycle launch does what the kernel does to X / P"""

    def __new__(cls):
        from . import fake_libpekf

        class Fake(fake_libpekf.FakeLib):
            replies = []

            def pekf_live_state_bytes(self, batch, flags):
                return batch * 336 if flags == EV64 else -1

            def pekf_frontend_init_state_bytes(self, batch, flags):
                return batch * 112

            def pekf_magcal_state_bytes(self, batch, n_cal, flags):
                return batch * (32 + 24 * n_cal + 8 * (n_cal % 2))

            def pekf_memset(self, p, value, n, stream):
                self._view(p, n)[:] = value
                return 0

            def pekf_magcal_resume_dev(self, batch, n, ev, n_cal, cal, fit, status, flags, state, resume, stream):
                self.calls.append(dict(entry="phase1", n=n, resume=resume, flags=flags))
                return 0

            def pekf_frontend_init_resume_dev(self, batch, n, ev, t_start, n_avg, init, t_init, ready, flags, state,
                                              resume, stream):
                self.calls.append(dict(entry="phase2", n=n, resume=resume))
                self.reply = self.replies.pop(0)
                self._view(t_init, 8 * batch, np.int64)[:] = self.reply[0]
                self._view(ready, 4 * batch, np.int32)[:] = self.reply[1]
                return 0

            def pekf_live_join_dev(self, batch, n, ev, init, t_init, alpha, X, Pm, q, r, counts, refs, flags, state,
                                   traj, traj_dt, rows, err, stream):
                self.calls.append(dict(entry="join", n=n, rows=rows))
                c, dt = self.reply[2], self.reply[3]
                self._view(counts, 4 * batch, np.int32)[:] = c
                if rows and dt is not None:
                    self._view(traj_dt, 8 * rows * batch, np.float64).reshape(rows, batch)[:len(dt)] = dt
                return 0

            def pekf_session_recycle_dev(self, *a):
                assert len(a) == len(PARAMS)
                c = dict(zip(PARAMS, a), entry="recycle")
                c["cols_host"] = cols = self._view(c["cols"], 4 * c["n_cols"], np.int32).copy()
                self.calls.append(c)
                if c["live_state"]:
                    X = self._view(c["X"], 32 * c["batch"], np.float64).reshape(-1, 4)
                    Pv = self._view(c["P"], 128 * c["batch"], np.float64).reshape(-1, 16)
                    if c["final_X"]:
                        self._view(c["final_X"], 32 * len(cols), np.float64).reshape(-1, 4)[:] = X[cols]
                        self._view(c["final_P"], 128 * len(cols), np.float64).reshape(-1, 16)[:] = Pv[cols]
                    X[cols] = self._view(c["X0"], 32 * len(cols), np.float64).reshape(-1, 4) if c["X0"] else [1, 0, 0, 0]
                    Pv[cols] = (self._view(c["P0"], 128 * len(cols), np.float64).reshape(-1, 16) if c["P0"]
                                else np.eye(4).ravel())
                if c["t_start_new"]:
                    c["t_new_host"] = self._view(c["t_start_new"], 8 * len(cols), np.int64).copy()
                return 0
        return Fake(1)


def _install(monkeypatch):
    from poseestimationkf_amd import _lib, engine
    fake = _Recorder()
    for mod in (_lib, engine):
        monkeypatch.setattr(mod, "lib", fake)
    return fake, engine


def _chunk(ev, a, b):
    return dict(types=ev["types"][a:b], values=ev["values"][a:b], times=ev["times"][a:b],
                values64=ev["values"][a:b].astype(np.float64))   # (the server's parse is not what is checked here)


def test_sessions_refuse_bad_columns_before_any_launch(monkeypatch):
    fake, engine = _install(monkeypatch)
    K = 4
    s = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5, n_cal=8)
    c = engine.CalibrationSession(K, n_cal=8)
    fake.calls.clear()
    for session in (s, c):
        for columns in ([4], [-1], [0, K], [1, -2]):
            with pytest.raises(ValueError, match=r"lie in \[0, 4\)"):
                session.recycle(columns)
        for columns in ([1, 1], [0, 3, 0]):
            with pytest.raises(ValueError, match="twice"):
                session.recycle(columns)
        for columns in ([[0, 1]], 2, [0.0, 1.0]):
            with pytest.raises(ValueError, match="1-D sequence of integer"):
                session.recycle(columns)
    I2 = np.broadcast_to(np.eye(4), (2, 4, 4))
    X2 = np.tile([1.0, 0, 0, 0], (2, 1))
    with pytest.raises(ValueError, match="t_start must have shape"):
        s.recycle([0, 1], t_start=[1, 2, 3])
    with pytest.raises(ValueError, match="t_start must have shape"):
        s.recycle([0, 1], t_start=5)
    with pytest.raises(ValueError, match="X0 must have shape"):
        s.recycle([0, 1], X0=np.zeros((2, 3)), P0=I2)
    with pytest.raises(ValueError, match="X0 must have shape"):
        s.recycle([0, 1], X0=np.zeros((3, 4)), P0=I2)
    with pytest.raises(ValueError, match="P0 must have shape"):
        s.recycle([0, 1], X0=X2, P0=np.zeros((2, 16)))
    with pytest.raises(ValueError, match="X0 needs P0"):
        s.recycle([0, 1], X0=X2)
    with pytest.raises(ValueError, match="P0 needs X0"):
        s.recycle([0, 1], P0=I2)
    # an empty list launches nothing and changes nothing -- not even the session's first, zero-row launch
    assert s.recycle([]) is None and c.recycle([]) is None
    assert s.recycle(np.zeros(0, np.int64), final=True)["X"].shape == (0, 4)
    assert fake.calls == [] and not s._book["started"] and not c.started


def test_recycle_hands_the_launch_its_groups_and_resets_the_book(monkeypatch):
    from poseestimationkf_amd import synth
    fake, engine = _install(monkeypatch)
    K, E = 4, 15
    ev = dict(synth.generate_events(np.arange(K), E, seed=3))
    f = engine.BatchedEKF(K)
    s = engine.PhoneSession(f, n_avg=5)
    nan = np.nan
    t0, t1, t2 = np.array([10, 20, 30, 40]), np.array([11, 21, 31, 41]), np.array([1000, 22, 32, 42])
    fake.replies[:] = [(t0, [1, 1, 0, 0], np.array([2, 1, 0, 0], np.int32), np.array([[5.0, 7.0, nan, nan],
                                                                                       [6.0, nan, nan, nan]])),
                       (t1, [1, 1, 1, 0], np.array([1, 1, 0, 0], np.int32), np.array([[1.0, 2.0, nan, nan]])),
                       (t2, [1, 1, 1, 0], np.array([2, 1, 0, 0], np.int32), np.array([[3.0, 4.0, nan, nan],
                                                                                       [9.0, nan, nan, nan]]))]
    out0 = s.feed(_chunk(ev, 0, 6), _chunk(ev, 0, 6), trajectory=True)
    out1 = s.feed(_chunk(ev, 6, 9), _chunk(ev, 6, 9), trajectory=True)
    assert np.array_equal(out0[2]["record_times_ns"][:, 0], [15.0, 21.0])
    assert np.array_equal(out1[2]["record_times_ns"][0, :2], [22.0, 29.0])        # 10 + 5 + 6 + 1; 20 + 7 + 2
    assert np.array_equal(s.total_counts, [3, 2, 0, 0])
    X = np.arange(4.0 * K).reshape(K, 4)
    Pm = np.arange(16.0 * K).reshape(K, 4, 4)
    f.set_state(X, Pm)
    fake.calls.clear()

    got = s.recycle([2, 0], t_start=[300, 100], final=True)
    (c,) = fake.calls                                                             # one launch, nothing else
    assert c["entry"] == "recycle" and (c["batch"], c["n_cols"], c["flags"]) == (K, 2, EV64)
    assert c["cols_host"].dtype == np.int32 and c["cols_host"].tolist() == [2, 0]   # int32, the caller's order
    assert c["t_new_host"].tolist() == [300, 100]
    assert (c["live_state"], c["X"], c["P"], c["refs"]) == (s._state.ptr, f.X.ptr, f.P.ptr, s._refs.ptr)
    assert (c["init_state"], c["t_start"], c["init"], c["t_init"], c["ready"]) == (
        s._p2state.ptr, s._t_start.ptr, s._init.ptr, s._t_init.ptr, s._ready.ptr)
    assert c["X0"] is None and c["P0"] is None and c["final_X"] and c["final_P"]
    # no n_cal: no phase-1 group
    assert (c["magcal_state"], c["cal"], c["fit"], c["status"]) == (None,) * 4
    # the departing phones, in the order of `columns`; the counts from the book as they were
    assert np.array_equal(got["X"], X[[2, 0]]) and np.array_equal(got["P"], Pm[[2, 0]])
    assert got["total_counts"].tolist() == [0, 3]
    # the listed columns' book is reset, the others' is untouched
    assert s.total_counts.tolist() == [0, 2, 0, 0]
    assert s._book["dt_sum"].tolist() == [0.0, 9.0, 0.0, 0.0]
    assert s._book["t_init"].tolist() == [100, 20, 300, 0]
    Xn, Pn = f.get_state()
    assert np.array_equal(Xn[[0, 2]], np.tile([1.0, 0, 0, 0], (2, 1))) and np.array_equal(Xn[[1, 3]], X[[1, 3]])
    assert np.array_equal(Pn[[0, 2]], np.broadcast_to(np.eye(4), (2, 4, 4))) and np.array_equal(Pn[[1, 3]], Pm[[1, 3]])

    # the new phone in column 0 applies its first record from ITS t_init (1000), not the old phone's (10); phone 1
    # goes on from its own running time
    out2 = s.feed(_chunk(ev, 9, 15), _chunk(ev, 9, 15), trajectory=True)
    assert np.array_equal(out2[2]["record_times_ns"][:, 0], [1003.0, 1012.0])
    assert np.array_equal(out2[2]["record_times_ns"][:, 1], [33.0, nan], equal_nan=True)
    assert s.total_counts.tolist() == [2, 3, 0, 0]
    assert s.recycle([1]) is None                                                 # final=False returns nothing
    assert fake.calls[-1]["final_X"] is None and fake.calls[-1]["t_start_new"] is None
    assert s._book["t_init"][1] == 0


def test_recycle_passes_the_phase1_group_only_with_n_cal(monkeypatch):
    fake, engine = _install(monkeypatch)
    K = 4
    f = engine.BatchedEKF(K)
    s = engine.PhoneSession(f, n_avg=5, n_cal=8)
    z = np.zeros(K, np.int32)
    fake.replies[:] = [(np.zeros(K, np.int64), z, z, None)]
    fake.calls.clear()
    X0, P0 = np.full((3, 4), 0.5), np.broadcast_to(0.4 * np.eye(4), (3, 4, 4))
    assert s.recycle(np.array([3, 1, 2]), X0=X0, P0=P0) is None
    # before the first chunk: the zero-row launches first, so that the buffers exist in their started form
    assert [c["entry"] for c in fake.calls] == ["phase1", "phase2", "join", "recycle"]
    assert [c["n"] for c in fake.calls[:3]] == [0, 0, 0] and fake.calls[0]["resume"] == 0 and s._book["started"]
    c = fake.calls[-1]
    assert c["cols_host"].tolist() == [3, 1, 2] and c["cols_host"].dtype == np.int32
    assert (c["magcal_state"], c["n_cal"], c["cal"], c["fit"], c["status"]) == (
        s._p1state.ptr, 8, s._cal.ptr, s._fit.ptr, s._status.ptr)
    assert c["live_state"] == s._state.ptr and c["init_state"] == s._p2state.ptr
    assert c["X0"] and c["P0"] and c["final_X"] is None and c["t_start_new"] is None
    Xn, Pn = f.get_state()
    assert np.array_equal(Xn[[3, 1, 2]], X0) and np.array_equal(Pn[[3, 1, 2]], P0) and Xn[0].tolist() == [1, 0, 0, 0]

    # CalibrationSession: the phase-1 group alone, on either event form
    for events, form in (("f32", 0), ("f64", EV64)):
        cs = engine.CalibrationSession(K, n_cal=8, events=events)
        fake.calls.clear()
        cs.recycle([2, 0])
        assert [c["entry"] for c in fake.calls] == ["phase1", "recycle"] and fake.calls[0]["flags"] == form
        c = fake.calls[-1]
        assert c["cols_host"].tolist() == [2, 0] and c["flags"] == 0
        assert (c["magcal_state"], c["n_cal"], c["cal"], c["fit"], c["status"]) == (
            cs._state.ptr, 8, cs._cal.ptr, cs._fit.ptr, cs._status.ptr)
        assert all(c[k] is None for k in PARAMS[4:18])
        cs.recycle([1])
        assert [c["entry"] for c in fake.calls] == ["phase1", "recycle", "recycle"]   # started: no zero-row launch
