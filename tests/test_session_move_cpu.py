"""Moving live phones between session columns (pekf_session_export_dev, pekf_session_import_dev,
pekf_session_columns_bytes; engine.PhoneSession.export_columns / import_columns / move, engine.SessionColumns,
engine.CalibrationSession.export_columns / import_columns), the parts a CPU can check: the entries are declared,
bound and exported; every refusal of their arguments comes before any device call and names the argument; the
pack's size; the sessions' own refusals, before any launch; what the launches are handed; and the host book of
the moved columns."""
import re

import numpy as np
import pytest

from . import test_session_recycle_cpu as rc
from .test_capi import HEADER

P = 16  # a non-null, 16-byte aligned "pointer": every case is refused before anything is read or launched
TE, F32R, EV64 = 0x1, 0x2, 0x4
GROUPS = ["live_state", "X", "P", "refs", "init_state", "t_start", "init", "t_init", "ready", "magcal_state", "n_cal",
          "cal", "fit", "status"]
PARAMS = ["batch", "n_cols", "cols", "flags"] + GROUPS + ["pack", "stream"]
ENTRIES = ("pekf_session_export_dev", "pekf_session_import_dev")
# per column: the filter (LiveState<true>'s 21 planes, X, P, refs), phase 2 (InitState's 7 planes, the two times,
# init, ready), and the phase-1 outputs (cal, fit, status), in 16 B plane entries
SESSION_BYTES, P1_OUT_BYTES = 16 * (21 + 2 + 8 + 3) + 16 * (7 + 1 + 3 + 1), 16 * (6 + 3 + 1)


@pytest.fixture(scope="module")
def lib():
    from poseestimationkf_amd import _lib
    return _lib


def _args(batch=8, n_cols=3, cols=P, flags=EV64, live=(P, P, P, P), p2=(P, P, P, P, P), p1=(P, 20, P, P, P), pack=P):
    return (batch, n_cols, cols, flags) + tuple(live) + tuple(p2) + tuple(p1) + (pack, None)


NO_LIVE, NO_P2, NO_P1 = (None,) * 4, (None,) * 5, (None, 0, None, None, None)


def test_entries_are_declared_bound_and_exported(lib):
    text = open(HEADER).read()
    for name in ENTRIES:
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M | re.S)
        assert m, "include/pekf.h does not declare %s" % name
        params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
        assert params == PARAMS, name
        assert len(params) == len(lib.SIGNATURES[name]) == len(_args())
        assert hasattr(lib.lib, name)
        # export reads the session and writes the pack; import the other way round
        consts = [p.strip().startswith("const ") for p in m.group(1).replace("\n", " ").split(",")]
        session = [c for c, p in zip(consts, params) if p in GROUPS and p != "n_cal"]
        assert all(session) == (name == ENTRIES[0]) and any(session) == (name == ENTRIES[0])
        assert consts[params.index("pack")] == (name == ENTRIES[1]) and consts[params.index("cols")]
    m = re.search(r"^int pekf_session_columns_bytes\(([^;]*)\);", text, re.M | re.S)
    assert m and [p.split()[-1] for p in m.group(1).split(",")] == ["n_cols", "n_cal", "flags"]
    assert len(lib.SIGNATURES["pekf_session_columns_bytes"]) == 3 and hasattr(lib.lib, "pekf_session_columns_bytes")
    assert lib.lib.pekf_abi_version() == 1
    # the header states the caller's preconditions
    comment = text[:text.index("int pekf_session_export_dev(")].rsplit("/*", 1)[1]
    for word in ("DISTINCT", "inside [0, batch)", "carries the groups it was exported with", "KFS/Server.cpp:58"):
        assert word in comment, word


@pytest.mark.parametrize("entry", ENTRIES)
def test_arguments_are_refused_before_any_device_call(lib, entry):
    bad = lib.PEKF_ERR_INVALID
    f = getattr(lib.lib, entry)

    def refused(word, **kw):
        assert f(*_args(**kw)) == bad, kw
        assert word in lib.last_error(), (kw, lib.last_error())

    refused("negative size", batch=-1)
    refused("negative size", n_cols=-1)
    refused("batch must be", batch=1 << 28)
    refused("live_state must be", live=(P + 8, P, P, P))
    refused("init_state must be", p2=(P + 8, P, P, P, P))
    refused("magcal_state must be", p1=(P + 8, 20, P, P, P))
    refused("pack must be", pack=P + 8)
    # the order is pekf_session_recycle_dev's: sizes, then alignment, then the groups
    refused("negative size", batch=-1, live=(P + 8, P, P, P), pack=P + 8)
    refused("live_state must be", live=(P + 8, None, P, P), pack=P + 8)
    # a half-given group, whichever pointer is missing -- the state's included
    for k in range(4):
        refused("filter group", live=tuple(None if j == k else P for j in range(4)))
    for k in range(5):
        refused("phase-2 group", p2=tuple(None if j == k else P for j in range(5)))
    for k in (0, 2, 3, 4):
        refused("phase-1 group", p1=tuple(None if j == k else v for j, v in enumerate((P, 20, P, P, P))))
    for n_cal in (5, 0, -1, 1 << 30):
        refused("n_cal", p1=(P, n_cal, P, P, P))
    refused("n_cal", p1=(None, 20, None, None, None))           # it sizes the pack: 0 without the group
    for flags in (0, TE, F32R, EV64 | TE, EV64 | F32R, 0x8):
        refused("PEKF_EV_F64_EVENTS", flags=flags)
        refused("PEKF_EV_F64_EVENTS", flags=flags, p2=NO_P2, p1=NO_P1)
        refused("PEKF_EV_F64_EVENTS", flags=flags, live=NO_LIVE, p1=NO_P1)   # the pack of flags 0 has no room for it
    for flags in (TE, F32R, 0x8):                                # a pack is a joining session's, or phase 1 alone
        refused("PEKF_EV_F64_EVENTS", flags=flags, live=NO_LIVE, p2=NO_P2)
    refused("null pointer", cols=None)
    refused("null pointer", pack=None)
    refused("n_cols must be <= batch", n_cols=9)


@pytest.mark.parametrize("entry", ENTRIES)
def test_what_needs_no_launch_is_ok(lib, entry):
    f = getattr(lib.lib, entry)
    assert f(*_args(n_cols=0)) == lib.PEKF_OK
    assert f(*_args(n_cols=0, cols=None, pack=None)) == lib.PEKF_OK
    assert f(*_args(batch=0, n_cols=0)) == lib.PEKF_OK
    assert f(*_args(batch=0)) == lib.PEKF_OK
    # the phase-1 group alone travels on either pack; n_cal is checked only with it
    assert f(*_args(n_cols=0, flags=0, live=NO_LIVE, p2=NO_P2)) == lib.PEKF_OK
    assert f(*_args(n_cols=0, flags=EV64, live=NO_LIVE, p2=NO_P2)) == lib.PEKF_OK
    assert f(*_args(n_cols=0, p1=NO_P1)) == lib.PEKF_OK
    assert f(*_args(live=NO_LIVE, p2=NO_P2, p1=NO_P1, flags=0)) == lib.PEKF_OK   # no group: nothing to do


def test_columns_bytes(lib):
    f = lib.lib.pekf_session_columns_bytes
    assert f(0, 0, EV64) == 0 and f(0, 20, 0) == 0
    assert f(5, 0, 0) == 0                                       # neither a session's groups nor phase 1
    for n in (1, 3, 70, 1 << 20):
        assert f(n, 0, EV64) == n * SESSION_BYTES
        for n_cal in (6, 7, 20, 21, 100, 101, (1 << 30) - 1):
            # per column the phase-1 state's own size -- two header planes and 24 B per sample, rounded up to
            # 16 -- and the phase-1 outputs
            grow = 32 + ((24 * n_cal + 15) & ~15) + P1_OUT_BYTES
            assert f(n, n_cal, EV64) - f(n, 0, EV64) == n * grow, (n, n_cal)
            assert f(n, n_cal, 0) == n * grow
            assert f(n, n_cal, EV64) % 16 == 0 and f(n, n_cal, 0) % 16 == 0
            assert n * (32 + ((24 * n_cal + 15) & ~15)) == lib.lib.pekf_magcal_state_bytes(n, n_cal, 0)
    for n_cal in (-1, 1, 5, 1 << 30):
        assert f(3, n_cal, EV64) == -1 and f(3, n_cal, 0) == -1
    for flags in (TE, F32R, EV64 | TE, 0x8):
        assert f(3, 20, flags) == -1
    assert f(-1, 20, EV64) == -1 and f(1 << 28, 0, EV64) == -1


# ------------------------------------------------------------------ the engine, on a fake library

def _install(monkeypatch):
    """test_session_recycle_cpu's recorder (it fails on any call it does not know) with the three new entries:
    export and import record what they are handed and move X as the kernel does, entry i <-> column cols[i]"""
    fake, engine = rc._install(monkeypatch)
    cls = type(fake)

    def columns_bytes(self, n, n_cal, flags):
        if n_cal != 0 and n_cal < 6:
            return -1
        return n * ((SESSION_BYTES if flags == EV64 else 0) + (32 + 24 * n_cal + 8 * (n_cal % 2) + P1_OUT_BYTES if n_cal else 0))

    def move(entry):
        def call(self, *a):
            assert len(a) == len(PARAMS)
            c = dict(zip(PARAMS, a), entry=entry)
            c["cols_host"] = cols = self._view(c["cols"], 4 * c["n_cols"], np.int32).copy()
            self.calls.append(c)
            if c["live_state"]:
                X = self._view(c["X"], 32 * c["batch"], np.float64).reshape(-1, 4)
                packed = self._view(c["pack"], 32 * len(cols), np.float64).reshape(-1, 4)
                if entry == "export":
                    packed[:] = X[cols]
                else:
                    X[cols] = packed
            return 0
        return call

    def join_noise(self, batch, n, ev, init, t_init, alpha, X, Pm, noise, counts, refs, flags, state, traj, traj_dt,
                   rows, err, stream):
        return self.pekf_live_join_dev(batch, n, ev, init, t_init, alpha, X, Pm, None, None, counts, refs, flags,
                                       state, traj, traj_dt, rows, err, stream)

    cls.pekf_session_columns_bytes = columns_bytes
    cls.pekf_session_export_dev = move("export")
    cls.pekf_session_import_dev = move("import")
    cls.pekf_live_join_noise_dev = join_noise
    return fake, engine


def _quiet(K):
    z = np.zeros(K, np.int32)
    return (np.zeros(K, np.int64), z, z, None)


def test_sessions_refuse_before_any_launch(monkeypatch):
    fake, engine = _install(monkeypatch)
    K = 4
    s = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5, n_cal=8)
    c = engine.CalibrationSession(K, n_cal=8)
    fake.replies[:] = [_quiet(K)]
    pack, cpack = s.export_columns([1, 3], release=False), c.export_columns([0, 2], release=False)
    assert isinstance(pack, engine.SessionColumns) and (pack.n, pack.n_avg, pack.alpha, pack.n_cal) == (2, 5, 0.1, 8)
    assert (cpack.n, cpack.n_cal, cpack.kind, cpack.events) == (2, 8, "calibration", "f32")
    fake.calls.clear()
    for session, good in ((s, pack), (c, cpack)):
        for columns in ([4, 0], [-1, 0], [0, K], [1, -2]):
            with pytest.raises(ValueError, match=r"lie in \[0, 4\)"):
                session.export_columns(columns)
            with pytest.raises(ValueError, match=r"lie in \[0, 4\)"):
                session.import_columns(columns, good)
        for columns in ([1, 1], [0, 3, 0]):
            with pytest.raises(ValueError, match="twice"):
                session.export_columns(columns)
        with pytest.raises(ValueError, match="twice"):
            session.import_columns([1, 1], good)
        for columns in ([[0, 1]], 2, [0.0, 1.0]):
            with pytest.raises(ValueError, match="1-D sequence of integer"):
                session.export_columns(columns)
            with pytest.raises(ValueError, match="1-D sequence of integer"):
                session.import_columns(columns, good)
        # a pack of another length
        for columns in ([0], [0, 1, 2], []):
            with pytest.raises(ValueError, match="columns listed for a pack of 2"):
                session.import_columns(columns, good)
    # the other class's pack
    with pytest.raises(ValueError, match="of this class"):
        s.import_columns([0, 1], cpack)
    with pytest.raises(ValueError, match="of this class"):
        c.import_columns([0, 1], pack)
    with pytest.raises(ValueError, match="of this class"):
        s.import_columns([0, 1], dict(n=2))
    # move: src and dst disjoint, of one length, each by recycle's rule
    for src, dst in (([0, 1], [1, 2]), ([0], [0]), ([3, 2], [0, 3])):
        with pytest.raises(ValueError, match="overlap"):
            s.move(src, dst)
    with pytest.raises(ValueError, match="columns listed for a pack of"):
        s.move([0, 1], [2])
    with pytest.raises(ValueError, match="twice"):
        s.move([0, 0], [1, 2])
    with pytest.raises(ValueError, match=r"lie in \[0, 4\)"):
        s.move([0, 1], [2, 4])
    # n_avg, alpha, n_cal: the session's -- phase 1 on one side only included
    f = engine.BatchedEKF(K)
    for kw, name in ((dict(n_avg=6, n_cal=8), "n_avg"), (dict(n_avg=5, alpha=0.2, n_cal=8), "alpha"),
                     (dict(n_avg=5, n_cal=9), "n_cal"), (dict(n_avg=5), "n_cal")):
        other = engine.PhoneSession(f, **kw)
        with pytest.raises(ValueError, match="the pack's %s is" % name):
            other.import_columns([0, 1], pack)
    bare = engine.PhoneSession(f, n_avg=5)
    fake.replies[:] = [_quiet(K)]
    bare_pack = bare.export_columns([0, 1], release=False)
    fake.calls.clear()
    with pytest.raises(ValueError, match="the pack's n_cal is None"):
        s.import_columns([0, 1], bare_pack)
    with pytest.raises(ValueError, match="the pack's n_cal is"):
        engine.CalibrationSession(K, n_cal=9).import_columns([0, 1], cpack)
    with pytest.raises(ValueError, match="the pack's events is"):
        engine.CalibrationSession(K, n_cal=8, events="f64").import_columns([0, 1], cpack)
    # noise that does not fit: a scalar filter takes only its own q and r
    for q, r in ((2.0, 0.1), (1.0, 0.2)):
        other = engine.PhoneSession(engine.BatchedEKF(K, q=q, r=r), n_avg=5, n_cal=8)
        with pytest.raises(ValueError, match="scalar-noise"):
            other.import_columns([0, 1], pack)
    mixed = engine.SessionColumns.from_host(dict(pack.to_host(), q=np.array([1.0, 3.0])))
    with pytest.raises(ValueError, match="scalar-noise"):
        s.import_columns([0, 1], mixed)
    # ... and a per-filter-noise filter only pairs a filter can have
    pf = engine.PhoneSession(engine.BatchedEKF(K, q=np.ones(K), r=np.full(K, 0.1)), n_avg=5, n_cal=8)
    for bad in (dict(r=np.array([0.1, 0.0])), dict(q=np.array([-1.0, 1.0])), dict(r=np.array([np.nan, 0.1]))):
        with pytest.raises(ValueError, match="every [qr] must be"):
            pf.import_columns([0, 1], engine.SessionColumns.from_host(dict(pack.to_host(), **bad)))
    # an empty list launches nothing and changes nothing -- not even a session's first, zero-row launch
    fresh, cfresh = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5, n_cal=8), engine.CalibrationSession(K, n_cal=8)
    fake.calls.clear()
    empty, cempty = fresh.export_columns([]), cfresh.export_columns(np.zeros(0, np.int64))
    assert empty.n == 0 and cempty.n == 0 and empty.pack.nbytes == 0
    assert fresh.import_columns([], empty) is None and cfresh.import_columns([], cempty) is None
    assert fresh.move([], []) is None
    assert fake.calls == [] and not fresh._book["started"] and not cfresh.started


def test_export_and_import_hand_the_launches_their_groups_and_move_the_book(monkeypatch):
    from poseestimationkf_amd import synth
    fake, engine = _install(monkeypatch)
    K, E = 4, 15
    ev = dict(synth.generate_events(np.arange(K), E, seed=3))
    f = engine.BatchedEKF(K)
    s = engine.PhoneSession(f, n_avg=5)
    nan = np.nan
    t0, t1 = np.array([10, 20, 30, 40]), np.array([11, 21, 31, 41])
    fake.replies[:] = [(t0, [1, 1, 0, 0], np.array([2, 1, 0, 0], np.int32), np.array([[5.0, 7.0, nan, nan],
                                                                                       [6.0, nan, nan, nan]])),
                       (t1, [1, 1, 1, 0], np.array([1, 1, 0, 0], np.int32), np.array([[1.0, 2.0, nan, nan]]))]
    s.feed(rc._chunk(ev, 0, 6), rc._chunk(ev, 0, 6), trajectory=True)
    s.feed(rc._chunk(ev, 6, 9), rc._chunk(ev, 6, 9), trajectory=True)
    assert s.total_counts.tolist() == [3, 2, 0, 0] and s._book["dt_sum"].tolist() == [12.0, 9.0, 0.0, 0.0]
    X = np.arange(4.0 * K).reshape(K, 4)
    f.set_state(X, np.broadcast_to(np.eye(4), (K, 4, 4)))
    fake.calls.clear()

    # a fork: one launch, the book as it was
    fork = s.export_columns([1, 0], release=False)
    (c,) = fake.calls
    assert c["entry"] == "export" and (c["batch"], c["n_cols"], c["flags"]) == (K, 2, EV64)
    assert c["cols_host"].dtype == np.int32 and c["cols_host"].tolist() == [1, 0]      # int32, the caller's order
    assert (c["live_state"], c["X"], c["P"], c["refs"]) == (s._state.ptr, f.X.ptr, f.P.ptr, s._refs.ptr)
    assert (c["init_state"], c["t_start"], c["init"], c["t_init"], c["ready"]) == (
        s._p2state.ptr, s._t_start.ptr, s._init.ptr, s._t_init.ptr, s._ready.ptr)
    assert (c["magcal_state"], c["n_cal"], c["cal"], c["fit"], c["status"]) == (None, 0, None, None, None)   # no n_cal
    assert c["pack"] == fork.pack.ptr and fork.pack.nbytes == 2 * SESSION_BYTES
    assert s.total_counts.tolist() == [3, 2, 0, 0]
    assert (fork.n, fork.n_avg, fork.alpha, fork.n_cal) == (2, 5, 0.1, None)
    assert fork.q.tolist() == [1.0, 1.0] and fork.r.tolist() == [0.1, 0.1]             # the filter's scalars, repeated
    assert fork.book["total_counts"].tolist() == [2, 3] and fork.book["dt_sum"].tolist() == [9.0, 12.0]
    assert fork.book["t_init"].tolist() == [20, 10]

    # a move: export, recycle (the book reset), import (the book rows of the pack), nothing else
    fake.calls.clear()
    assert s.move([0, 1], [3, 2]) is None
    assert [c["entry"] for c in fake.calls] == ["export", "recycle", "import"]
    ex, re_, im = fake.calls
    assert ex["cols_host"].tolist() == re_["cols_host"].tolist() == [0, 1] and im["cols_host"].tolist() == [3, 2]
    assert re_["X0"] is None and re_["final_X"] is None and re_["t_start_new"] is None
    assert im["pack"] == ex["pack"] and (im["batch"], im["n_cols"], im["flags"]) == (K, 2, EV64)
    for key in GROUPS:
        assert im[key] == ex[key], key
    assert s.total_counts.tolist() == [0, 0, 2, 3]
    assert s._book["dt_sum"].tolist() == [0.0, 0.0, 9.0, 12.0] and s._book["t_init"].tolist() == [0, 0, 20, 10]
    Xn, _ = f.get_state()
    assert np.array_equal(Xn[[3, 2]], X[[0, 1]]) and np.array_equal(Xn[[0, 1]], np.tile([1.0, 0, 0, 0], (2, 1)))

    # the moved phones' record times go on from their own book: 20 + 9 + 4 in column 2, 10 + 12 + 3 in column 3
    fake.replies[:] = [(np.array([1000, 22, 32, 42]), [0, 0, 1, 1], np.array([0, 0, 1, 1], np.int32),
                        np.array([[nan, nan, 4.0, 3.0]]))]
    out = s.feed(rc._chunk(ev, 9, 15), rc._chunk(ev, 9, 15), trajectory=True)
    assert np.array_equal(out[2]["record_times_ns"][0], [nan, nan, 33.0, 25.0], equal_nan=True)
    assert s.total_counts.tolist() == [0, 0, 3, 4]

    # into a session that has not started, of another batch: its zero-row launches first; through the host
    f2 = engine.BatchedEKF(6)
    s2 = engine.PhoneSession(f2, n_avg=5)
    fake.replies[:] = [_quiet(6)]
    fake.calls.clear()
    host = fork.to_host()
    assert all(isinstance(v, np.ndarray) for v in host.values()) and host["pack"].dtype == np.uint8
    again = engine.SessionColumns.from_host(host)
    assert (again.n, again.n_avg, again.alpha, again.n_cal, again.kind) == (2, 5, 0.1, None, "phone")
    assert again.pack.ptr != fork.pack.ptr and np.array_equal(again.to_host()["pack"], host["pack"])
    s2.import_columns([5, 2], again)
    assert [c["entry"] for c in fake.calls] == ["phase2", "join", "import"] and s2._book["started"]
    assert fake.calls[-1]["batch"] == 6 and fake.calls[-1]["cols_host"].tolist() == [5, 2]
    assert s2.total_counts.tolist() == [0, 0, 3, 0, 0, 2] and s2._book["t_init"].tolist() == [0, 0, 10, 0, 0, 20]
    assert np.array_equal(f2.get_state()[0][[5, 2]], X[[1, 0]])
    with pytest.raises(ValueError, match="does not hold|bytes are not"):
        engine.SessionColumns.from_host(dict(host, pack=host["pack"][:-16]))


def test_phase1_travels_only_with_n_cal_and_noise_goes_into_the_plane(monkeypatch):
    fake, engine = _install(monkeypatch)
    K = 4
    q, r = np.array([1.0, 0.37, 4.0, 1e-3]), np.array([0.1, 2.5, 0.01, 1.0])
    f = engine.BatchedEKF(K, q=q, r=r)
    s = engine.PhoneSession(f, n_avg=5, n_cal=8)
    fake.replies[:] = [_quiet(K)]
    fake.calls.clear()
    pack = s.export_columns(np.array([3, 1]))
    # before the first chunk: the zero-row launches first, then the export, then release's recycle
    assert [c["entry"] for c in fake.calls] == ["phase1", "phase2", "join", "export", "recycle"]
    c = fake.calls[3]
    assert (c["magcal_state"], c["n_cal"], c["cal"], c["fit"], c["status"]) == (
        s._p1state.ptr, 8, s._cal.ptr, s._fit.ptr, s._status.ptr)
    assert c["live_state"] == s._state.ptr and c["init_state"] == s._p2state.ptr
    assert pack.pack.nbytes == 2 * (SESSION_BYTES + 32 + 24 * 8 + P1_OUT_BYTES)
    assert pack.q.tolist() == [1e-3, 0.37] and pack.r.tolist() == [1.0, 2.5]           # the columns' own pairs
    # a per-filter-noise destination takes the pairs into its arrays and its plane
    f2 = engine.BatchedEKF(K, q=np.ones(K), r=np.full(K, 0.1))
    s2 = engine.PhoneSession(f2, n_avg=5, n_cal=8)
    fake.replies[:] = [_quiet(K)]
    s2.import_columns([0, 2], pack)
    assert f2.q.tolist() == [1e-3, 1.0, 0.37, 1.0] and f2.r.tolist() == [1.0, 0.1, 2.5, 0.1]
    plane = f2.noise.download((K, 2), np.float64)
    assert np.array_equal(plane, np.stack([f2.q, f2.r], axis=1))
    assert fake.calls[-1]["entry"] == "import" and fake.calls[-1]["magcal_state"] == s2._p1state.ptr
    # a scalar filter accepts a pack whose pairs all are its own
    s3 = engine.PhoneSession(engine.BatchedEKF(K, q=1.0, r=0.1), n_avg=5, n_cal=8)
    fake.replies[:] = [_quiet(K)]
    own = s2.export_columns([1, 3], release=False)
    s3.import_columns([0, 1], own)
    assert fake.calls[-1]["entry"] == "import"

    # CalibrationSession: the phase-1 group alone, on either event form; the f32 form's last times travel
    for events, form in (("f32", 0), ("f64", EV64)):
        cs, cd = (engine.CalibrationSession(K, n_cal=8, events=events) for _ in range(2))
        cs._last_times[:] = [5, 6, 7, 8]
        cs.started = True
        fake.calls.clear()
        cp = cs.export_columns([2, 0])
        assert [c["entry"] for c in fake.calls] == ["export", "recycle"]               # started: no zero-row launch
        c = fake.calls[0]
        assert c["cols_host"].tolist() == [2, 0] and c["flags"] == 0
        assert (c["magcal_state"], c["n_cal"], c["cal"], c["fit"], c["status"]) == (
            cs._state.ptr, 8, cs._cal.ptr, cs._fit.ptr, cs._status.ptr)
        assert all(c[k] is None for k in GROUPS[:9])
        assert cp.pack.nbytes == 2 * (32 + 24 * 8 + P1_OUT_BYTES) and cp.book["last_times"].tolist() == [7, 5]
        fake.calls.clear()
        cd.import_columns([1, 3], engine.SessionColumns.from_host(cp.to_host()))
        assert [c["entry"] for c in fake.calls] == ["phase1", "import"] and fake.calls[0]["flags"] == form
        c = fake.calls[-1]
        assert c["cols_host"].tolist() == [1, 3] and c["flags"] == 0 and c["magcal_state"] == cd._state.ptr
        assert all(c[k] is None for k in GROUPS[:9])
        assert cd._last_times.tolist() == [0, 7, 0, 5]
        fake.calls.clear()
        fork = cs.export_columns([1], release=False)
        assert [c["entry"] for c in fake.calls] == ["export"] and fork.n == 1
