"""Chunked sessions that hand out their records (pekf_live_resume_rec_dev, pekf_live_join_rec_dev, the `records`
keyword of LiveSession / PhoneSession, engine.SessionLog), the parts a CPU can check: the entries are declared,
bound and exported; what they refuse before any device call; with a recorder in place of the library, which entry
a chunk calls and with what; and SessionLog's bytes and refusals on hand-made chunk dicts."""
import io
import re

import numpy as np
import pytest

from .test_capi import HEADER

P = 32  # a non-null "pointer" aligned for every plane: every case is refused before anything is read or launched
TE, F32R, EV64 = 0x1, 0x2, 0x4


@pytest.fixture(scope="module")
def lib():
    from poseestimationkf_amd import _lib
    return _lib


def _resume(batch=8, n_events=8, ev=P, r=0.1, noise=None, flags=0, state=P, resume=0, traj=P, traj_dt=P, traj_rows=4,
            gd=P, am=P, my=P):
    return (batch, n_events, ev, P, P, 0.1, P, P, 1.0, r, noise, P, P, flags, state, resume, traj, traj_dt, traj_rows,
            gd, am, my, None, None)


def _join(flags=EV64, **kw):
    a = _resume(flags=flags, **kw)
    return a[:15] + a[16:]      # no `resume` word


def test_entries_are_declared_bound_and_exported(lib):
    text = open(HEADER).read()
    for name, n in (("pekf_live_resume_rec_dev", 24), ("pekf_live_join_rec_dev", 23)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M | re.S)
        assert m, "include/pekf.h does not declare " + name
        params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
        assert len(params) == n == len(lib.SIGNATURES[name])
        assert params[8:11] == ["q", "r", "noise"]
        assert params[-7:] == ["traj_dt", "traj_rows", "rec_gd", "rec_am", "rec_my", "dev_error", "stream"]
        assert hasattr(lib.lib, name)
    # the entries they extend are what they were
    for name, n in (("pekf_live_resume_dev", 20), ("pekf_live_join_dev", 19), ("pekf_live_resume_noise_dev", 19),
                    ("pekf_live_join_noise_dev", 18)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M | re.S)
        assert len(m.group(1).split(",")) == n == len(lib.SIGNATURES[name])
    assert lib.lib.pekf_abi_version() == 1


@pytest.mark.parametrize("which", ["resume", "join"])
def test_arguments_are_refused_before_any_device_call(lib, which):
    entry = getattr(lib.lib, "pekf_live_%s_rec_dev" % which)
    args = _resume if which == "resume" else _join
    form = {} if which == "resume" else dict(flags=EV64)
    bad = lib.PEKF_ERR_INVALID

    def refused(message, **kw):
        assert entry(*args(**dict(form, **kw))) == bad
        assert message in lib.last_error(), lib.last_error()

    # a record comes beside its pose
    refused("traj_rows must be > 0", traj_rows=0)
    refused("traj_rows must be > 0", traj_dt=None)
    refused("traj must be", traj=None)
    # the three planes: non-null, 32 / 32 / 16 bytes
    for plane in ("gd", "am", "my"):
        refused("null record plane", **{plane: None})
    refused("misaligned record planes", gd=P + 16)
    refused("misaligned record planes", am=P + 16)
    refused("misaligned record planes", my=P + 8)
    assert entry(*args(**dict(form, my=P + 16, batch=0))) == lib.PEKF_OK     # rec_my: 16 bytes do
    # flags
    refused("PEKF_EV_F32_RECORDS" if which == "resume" else "PEKF_EV_F64_EVENTS", flags=F32R)
    if which == "join":
        refused("PEKF_EV_F64_EVENTS", flags=0)
        refused("PEKF_EV_F64_EVENTS", flags=TE)
    else:
        refused("PEKF_EV_F32_RECORDS", flags=F32R | TE, resume=1)
    # the parents' checks
    refused("state must be", state=None)
    refused("state must be", state=P + 8)
    refused("negative size", batch=-1)
    refused("traj_rows", traj_rows=1 << 31)
    refused("traj_dt", traj_dt=P + 4)
    refused("batch must be", batch=1 << 28)
    refused("null pointer", ev=None)
    refused("r must be > 0", r=0.0)
    refused("noise must be", noise=P + 8, r=0.0)       # a plane: q and r are ignored, the plane's alignment is not
    # an empty batch is fine, and before that every check above still holds
    assert entry(*args(**dict(form, batch=0))) == lib.PEKF_OK
    assert entry(*args(**dict(form, batch=0, noise=P))) == lib.PEKF_OK
    refused("null record plane", batch=0, gd=None)


# ------------------------------------------------------------------ which entry a chunk calls, and with what

def _fake():
    from . import fake_libpekf

    class Fake(fake_libpekf.FakeLib):
        def pekf_live_state_bytes(self, batch, flags):
            return batch * (336 if flags & EV64 else 288)

        def pekf_frontend_init_state_bytes(self, batch, flags):
            return batch * 64

        def pekf_memset(self, p, value, n, stream):
            self._view(p, n)[:] = value
            return 0

        def _sizes(self):
            return {a: len(b) for a, b in self.mem.items()}

        def _log(self, name, args):
            self.calls.append((name, args, self._sizes()))
            return 0

        def pekf_frontend_init_resume_dev(self, *a):
            return 0

        def pekf_live_resume_dev(self, *a):
            return self._log("resume", a)

        def pekf_live_resume_noise_dev(self, *a):
            return self._log("resume_noise", a)

        def pekf_live_resume_rec_dev(self, *a):
            return self._log("resume_rec", a)

        def pekf_live_join_dev(self, *a):
            return self._log("join", a)

        def pekf_live_join_noise_dev(self, *a):
            return self._log("join_noise", a)

        def pekf_live_join_rec_dev(self, *a):
            return self._log("join_rec", a)
    return Fake(1)


def _install(monkeypatch):
    from poseestimationkf_amd import _lib, engine
    fake = _fake()
    for mod in (_lib, engine):
        monkeypatch.setattr(mod, "lib", fake)
    return fake, engine


def _stream(K, E):
    from poseestimationkf_amd import synth
    return synth.generate_events(np.arange(K), E, seed=3)


def _rows(ev, a, b):
    return dict(types=ev["types"][a:b], values=ev["values"][a:b], times=ev["times"][a:b],
                values64=ev["values"][a:b].astype(np.float64))


@pytest.mark.parametrize("per_filter", [False, True])
@pytest.mark.parametrize("events", ["f32", "f64"])
def test_live_session_calls(monkeypatch, per_filter, events):
    fake, engine = _install(monkeypatch)
    K, E = 5, 12
    ev = _stream(K, E)
    q, r = (np.linspace(0.5, 1.5, K), np.linspace(0.1, 0.2, K)) if per_filter else (1.0, 0.1)

    def session():
        f = engine.BatchedEKF(K, q, r)
        return f, engine.LiveSession(f, ev["init_acc"], ev["init_mag"], ev["t_init"], events=events)

    # without records: the parent's call, argument for argument (same entry, same count and values)
    f, s = session()
    fake.calls.clear()
    s.feed(_rows(ev, 0, 7), trajectory=True)
    s.feed(_rows(ev, 7, E))
    plain = "resume_noise" if per_filter else "resume"
    assert [c[0] for c in fake.calls] == [plain, plain]
    a = fake.calls[0][1]
    assert len(a) == (19 if per_filter else 20)
    noise = (f.noise.ptr,) if per_filter else (1.0, 0.1)
    form = EV64 if events == "f64" else 0
    assert a[:8] == (K, 7, a[2], s._init.ptr, s._t_init.ptr, 0.1, f.X.ptr, f.P.ptr)
    assert a[8:8 + len(noise)] == noise
    tail = a[8 + len(noise):]
    assert tail[:5] == (s._cnt.ptr, s._refs.ptr, form, s._state.ptr, 0) and tail[7:] == (3, None, None)
    b = fake.calls[1][1]
    assert b[8 + len(noise):][4:] == (1, None, None, 0, None, None)         # resumed, no trajectory

    # with records: the _rec entry, three planes of rows x K x 32 / 32 / 16 bytes, every byte 0xFF
    f, s = session()
    fake.calls.clear()
    counts, out = s.feed(_rows(ev, 0, 7), records=True)                       # a trajectory is implied: 3 rows
    (name, a, sizes), = fake.calls
    assert name == "resume_rec" and len(a) == 24
    assert a[:8] == (K, 7, a[2], s._init.ptr, s._t_init.ptr, 0.1, f.X.ptr, f.P.ptr)
    assert a[8:11] == ((0.0, 0.0, f.noise.ptr) if per_filter else (1.0, 0.1, None))
    assert a[11:16] == (s._cnt.ptr, s._refs.ptr, form, s._state.ptr, 0)
    rows = a[18]
    assert rows == 3 and a[22:] == (None, None)
    assert [sizes[p] for p in a[16:18]] == [32 * rows * K, 8 * rows * K]
    assert [sizes[p] for p in a[19:22]] == [32 * rows * K, 32 * rows * K, 16 * rows * K]
    win = out["records"]
    assert isinstance(win, engine.RecordWindow64) and (win.batch, win.window) == (K, rows)
    assert (win.gd.ptr, win.am.ptr, win.my.ptr) == a[19:22]
    for plane in (win.gd, win.am, win.my):
        assert (plane.download((plane.nbytes,), np.uint8) == 0xFF).all()
    assert np.array_equal(win.counts, np.zeros(K)) and np.array_equal(win.chunk_counts, counts)
    assert set(out) == {"trajectory", "record_dt_ns", "record_times_ns", "records"}
    # an explicit cap holds for poses and records alike; a resumed chunk says so
    fake.calls.clear()
    _, out = s.feed(_rows(ev, 7, E), trajectory=1, records=True)
    (name, a, sizes), = fake.calls
    assert name == "resume_rec" and a[15] == 1 and a[18] == 1 and sizes[a[21]] == 16 * K
    assert out["records"].window == 1 and out["trajectory"].shape == (1, K, 4)
    # no rows: nothing to export, the launch is the parent's and the window is empty
    fake.calls.clear()
    _, out = s.feed(_rows(ev, E, E), records=True)
    assert [c[0] for c in fake.calls] == [plain] and out["records"].window == 0


@pytest.mark.parametrize("per_filter", [False, True])
def test_phone_session_calls(monkeypatch, per_filter):
    fake, engine = _install(monkeypatch)
    K, E = 5, 12
    ev = _stream(K, E)
    q, r = (np.linspace(0.5, 1.5, K), np.linspace(0.1, 0.2, K)) if per_filter else (1.0, 0.1)
    f = engine.BatchedEKF(K, q, r)
    s = engine.PhoneSession(f, n_avg=5)
    fake.calls.clear()
    out = s.feed(_rows(ev, 0, 6), _rows(ev, 0, 6), trajectory=True)
    plain = "join_noise" if per_filter else "join"
    (name, a, _), = fake.calls
    assert name == plain and len(a) == (18 if per_filter else 19) and len(out) == 3
    assert a[-5:] == (a[-5], a[-4], 2, None, None)
    fake.calls.clear()
    counts, ready, out = s.feed(_rows(ev, 6, E), _rows(ev, 6, E), records=True)
    (name, a, sizes), = fake.calls
    assert name == "join_rec" and len(a) == 23
    assert a[:2] == (K, 6) and a[3:8] == (s._init.ptr, s._t_init.ptr, 0.1, f.X.ptr, f.P.ptr)
    assert a[8:11] == ((0.0, 0.0, f.noise.ptr) if per_filter else (1.0, 0.1, None))
    assert a[11:15] == (s._cnt.ptr, s._refs.ptr, EV64, s._state.ptr)
    rows = a[17]
    assert rows == 2 and [sizes[p] for p in a[18:21]] == [32 * rows * K, 32 * rows * K, 16 * rows * K]
    assert (out["records"].gd.ptr, out["records"].am.ptr, out["records"].my.ptr) == a[18:21]
    assert out["records"].window == rows and a[21:] == (None, None)


# ------------------------------------------------------------------ SessionLog

class _Window:
    """A chunk's records as SessionLog reads them, from host arrays"""

    def __init__(self, gyro, dt, acc, mag, refs, counts, chunk_counts, wahba, q_rows):
        self.window, self.batch = gyro.shape[:2]
        self.a = gyro, dt, acc, mag, refs
        self.counts, self.chunk_counts, self.wahba, self.q_rows = counts, chunk_counts, wahba, q_rows
        self.q0 = None

    def wahba_quaternions(self):
        return self.wahba

    def gyro_chain(self, q0, want_traj):
        assert want_traj
        self.q0 = np.array(q0)
        return self.q_rows[-1], self.q_rows

    def download_filters(self, cols):
        g, dt, a, m, refs = self.a
        return g[:, cols], dt[:, cols], a[:, cols], m[:, cols], refs[cols]


class _Session:
    def __init__(self, K, t_init):
        self.batch, self._book = K, dict(t_init=t_init)


def test_session_log_writes_write_logs_bytes(tmp_path):
    from poseestimationkf_amd import engine, logformat
    rng = np.random.default_rng(5)
    K, R = 4, 9
    counts_all = np.array([9, 0, 5, 7])                     # column 1 never has a record: no file
    gyro, acc, mag = (rng.standard_normal((R, K, 3)) for _ in range(3))
    dt = rng.integers(1, 10**7, (R, K)).astype(np.float64)
    traj, wahba, qg = (rng.standard_normal((R, K, 4)) for _ in range(3))
    refs = rng.standard_normal((K, 6))
    t_init = np.array([10**15, 5, 10**15 + 77, 123456789], np.int64)
    times = engine.record_times_ns(t_init, dt)
    cols = [3, 1, 0, 2]
    paths = [tmp_path / ("log%d.txt" % k) for k in cols]
    log = engine.SessionLog(_Session(K, t_init), cols, paths)
    pos = np.zeros(K, np.int64)
    seen_q0 = []
    for n in ([2, 0, 0, 3], [0, 0, 0, 0], [4, 0, 5, 1], [3, 0, 0, 3]):     # rows of each column per chunk
        n = np.array(n)
        rows = max(1, int(n.max()))

        def cut(a):
            out = np.full((rows,) + a.shape[1:], np.nan)
            for k in range(K):
                out[:n[k], k] = a[pos[k]:pos[k] + n[k], k]
            return out
        win = _Window(cut(gyro), cut(dt), cut(acc), cut(mag), refs, n, n, cut(wahba), cut(qg))
        log.append(dict(trajectory=cut(traj), record_dt_ns=cut(dt), record_times_ns=cut(times), records=win))
        if win.q0 is not None:
            seen_q0.append((pos.copy(), win.q0))
        pos += n
    assert np.array_equal(pos, counts_all)
    for k, path in zip(cols, paths):
        n = counts_all[k]
        if n == 0:
            assert not path.exists()
            continue
        want = io.StringIO()
        logformat.write_log(want, np.concatenate([[t_init[k]], times[:n, k]]), gyro[:n, k], acc[:n, k], mag[:n, k],
                            refs[k, :3], refs[k, 3:], qg[:n, k], traj[:n, k], wahba[:n, k])
        assert path.read_text() == want.getvalue()
    # q_gyro continues from the column's own last row so far: the identity at first, never another column's row
    for at, q0 in seen_q0:
        for k in cols:
            assert np.array_equal(q0[k], qg[at[k] - 1, k] if at[k] else [1.0, 0.0, 0.0, 0.0])


def test_write_log_continued_leaves_the_default_alone():
    from poseestimationkf_amd import logformat
    rng = np.random.default_rng(6)
    n = 5
    g, a, m = (rng.standard_normal((n, 3)) for _ in range(3))
    q = rng.standard_normal((n, 4))
    t = np.arange(n + 1) * 1000 + 7
    whole, parts = io.StringIO(), io.StringIO()
    logformat.write_log(whole, t, g, a, m, [1, 2, 3], [4, 5, 6], q, q + 1, q + 2)
    logformat.write_log(parts, t[:3], g[:2], a[:2], m[:2], [1, 2, 3], [4, 5, 6], q[:2], q[:2] + 1, q[:2] + 2)
    logformat.write_log(parts, t[3:], g[2:], a[2:], m[2:], None, None, q[2:], q[2:] + 1, q[2:] + 2, continued=True)
    assert parts.getvalue() == whole.getvalue()
    assert whole.getvalue().startswith("mag_0 : 4.000000,5.000000,6.000000\nacc_0 : 1.000000,2.000000,3.000000\n")


def test_session_log_refusals(tmp_path):
    from poseestimationkf_amd import engine
    K = 3
    s = _Session(K, np.zeros(K, np.int64))
    with pytest.raises(ValueError, match="paths"):
        engine.SessionLog(s, [0, 1], [tmp_path / "a"])
    with pytest.raises(ValueError, match="twice"):
        engine.SessionLog(s, [1, 1], [tmp_path / "a", tmp_path / "b"])
    log = engine.SessionLog(s, [0, 2], [tmp_path / "a", tmp_path / "b"])
    z = np.zeros((2, K, 4))
    plain = dict(trajectory=z, record_dt_ns=z[..., 0], record_times_ns=z[..., 0])
    with pytest.raises(ValueError, match="records=True"):
        log.append(plain)                                   # a chunk fed without records
    with pytest.raises(ValueError, match="records=True"):
        log.append(np.zeros(K, np.int32))                   # ... or without a trajectory at all: counts alone
    full = np.array([2, 5, 3], np.int32)                    # column 2 applied 3 records, the cap kept 2 rows
    win = _Window(z[..., :3], z[..., 0], z[..., :3], z[..., :3], np.zeros((K, 6)), np.minimum(full, 2), full, z, z)
    with pytest.raises(ValueError, match="row cap"):
        log.append(dict(plain, records=win))
    assert not (tmp_path / "a").exists() and not (tmp_path / "b").exists()
    # a cut column that is not listed does not matter
    log = engine.SessionLog(s, [0], [tmp_path / "a"])
    log.append(dict(plain, records=win))
    assert (tmp_path / "a").exists()
