"""Chunked sessions hand out their records (pekf_live_resume_rec_dev, pekf_live_join_rec_dev; records=True of
LiveSession / PhoneSession; engine.SessionLog): what the filter was fed, row for row beside its poses.

The yardsticks are existing paths whose kernels are not under test: the one-shot front-end (engine.run_frontend,
k_frontend) for the records themselves, the same session fed without `records` for everything else a launch
writes, the multi-record run (BatchedEKF.run on a RecordWindow64) for the replay, and logformat.write_log on
one-shot arrays for the log.  K = 130 phones: lanes 63, 64 and K - 1 are there and the batch ends inside a wave."""
import io

import numpy as np
import pytest

from poseestimationkf_amd import logformat, synth, wire

from .test_live import ATOL_F64_CHAIN
from .test_live_resume import _ragged_clock
from .test_live_traj import _resumed
from .test_noise_per_filter import PAIRS

pytestmark = pytest.mark.gpu

K, E, EP, N_AVG, N_CAL, ALPHA = 130, 100, 120, 10, 20, 0.1   # (E: a LiveSession's event rows, EP: a PhoneSession's)
LANES = [0, 63, 64, K - 1]
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
FIELDS = (("traj", (4,)), ("dt", ()), ("times", ()), ("gyro", (3,)), ("rdt", ()), ("acc", (3,)), ("mag", (3,)))
RECORD = ("gyro", "rdt", "acc", "mag")


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _cuts(n, seed=0):
    """name -> [(first row, end row)] covering 0 .. n: one chunk, single rows, 3s, 7s, random sizes with empty chunks"""
    def by(m):
        return [(a, min(a + m, n)) for a in range(0, n, m)]
    rng = np.random.default_rng(3000 + seed)
    sizes = [0]
    while sum(sizes) < n:
        sizes.append(int(rng.integers(0, 30)))
        if len(sizes) == 2 or rng.random() < 0.2:
            sizes.append(0)
    edges = np.minimum(np.cumsum([0] + sizes + [0]), n)
    out = {"one": [(0, n)], "1": by(1), "3": by(3), "7": by(7), "random": list(zip(edges[:-1], edges[1:]))}
    assert sum(a == b for a, b in out["random"]) >= 3
    return out


class Got:
    """What a session's chunks gave, put together per filter in order: poses, dts, times and -- from the chunks
    fed with records -- the records.  Every chunk's window is checked as it comes: its shape, its counts, and that
    nothing but a filter's own rows was written (every other byte is still 0xFF)."""

    def __init__(self, rows, batch=K):
        self.f = {name: np.full((rows, batch) + shape, np.nan) for name, shape in FIELDS}
        self.pos, self.batch, self.windows = np.zeros(batch, np.int64), batch, 0

    def add(self, counts, out):
        R = len(out["trajectory"])
        n = np.minimum(counts, R)
        arrays = dict(traj=out["trajectory"], dt=out["record_dt_ns"], times=out["record_times_ns"])
        win = out.get("records")
        if win is not None:
            assert (win.batch, win.window) == (self.batch, R)
            assert np.array_equal(win.counts, n) and np.array_equal(win.chunk_counts, counts)
            self.windows += 1
            if R:
                gd, am, my = (b.download((R, self.batch, w), np.float64) for b, w in ((win.gd, 4), (win.am, 4), (win.my, 2)))
                free = ~(np.arange(R)[:, None] < n[None, :])
                for plane in (gd, am, my):
                    assert (_bits(plane)[free] == ONES).all()
                assert not np.isnan(gd[~free]).any() and not np.isnan(am[~free]).any() and not np.isnan(my[~free]).any()
                arrays.update(gyro=gd[..., :3], rdt=gd[..., 3], acc=am[..., :3],
                              mag=np.concatenate([am[..., 3:], my], axis=-1))
        for r in range(int(n.max(initial=0))):
            k = np.flatnonzero(n > r)
            for name, a in arrays.items():
                self.f[name][self.pos[k] + r, k] = a[r, k]
        self.pos += n

    def equal(self, other, names, cols=slice(None), other_cols=None):
        oc = cols if other_cols is None else other_cols
        n = min(len(self.f["dt"]), len(other.f["dt"]))         # (the two may have room for different numbers of rows)
        return all(_same(self.f[name][:n, cols], other.f[name][:n, oc]) and np.isnan(self.f[name][n:, cols]).all() and
                   np.isnan(other.f[name][n:, oc]).all() for name in names)


def _window_arrays(win, cols=None):
    """(gyro, dt, acc, mag) (W, K, ..) float64 of a RecordWindow64"""
    cols = np.arange(win.batch) if cols is None else cols
    g, dt, a, m, _ = win.download_filters(cols)
    return dict(gyro=g, rdt=dt, acc=a, mag=m)


def _rows_equal(got, want, counts, names=RECORD, cols=None):
    """rows [:counts[k]] of got.f equal those of the arrays `want`, bit for bit, column by column"""
    for k in (range(len(counts)) if cols is None else cols):
        n = int(counts[k])
        for name in names:
            assert _same(got.f[name][:n, k], want[name][:n, k]), (name, k)
        assert np.isnan(got.f["gyro"][n:, k]).all()


# ------------------------------------------------------------------ LiveSession

def _live_stream():
    """every third filter pauses for seconds (2^31 ns and more: f32 events need time events, the record's dt is
    escaped), another third's clock steps back"""
    return _ragged_clock(K, E, 22)


def _pack(eng, ev, form):
    return synth.pack_events64(ev, eng.server_event_values(ev)) if form == "f64" else synth.pack_events(ev)


def _live(eng, ev, form, cuts, records, q=1.0, r=0.1, trajectory=True, state=None, planes=None):
    planes = _pack(eng, ev, form) if planes is None else planes
    buf = eng.DeviceBuffer(planes.nbytes).upload(planes)
    row = planes[0].nbytes
    f = eng.BatchedEKF(K, q, r)
    if state is not None:
        f.set_state(*state)
    s = eng.LiveSession(f, ev["init_acc"], ev["init_mag"], ev["t_init"], alpha=ALPHA, events=form)
    got = Got(planes.shape[0] // 3 + 2)
    full = np.zeros(K, np.int64)
    for a, b in cuts:
        a, b = int(a), int(b)
        te = eng.EV_TIME_EVENTS if form == "f32" and a < b and synth.has_time_events(planes[a:b]) else 0
        counts, out = s.feed_planes(buf, b - a, te, trajectory=trajectory, offset=a * row, records=records)
        got.add(counts, out)
        full += counts
    X, P = f.get_state()
    assert np.array_equal(s.total_counts, full)
    return dict(X=X, P=P, refs=s.refs, total=full, got=got, session=s)


def _launch_outputs_equal(a, b, label=""):
    """everything a launch writes without `records`: X, P, refs, counts, every trajectory row and its dt"""
    assert np.array_equal(a["total"], b["total"]), label
    for key in ("X", "P", "refs"):
        assert _same(a[key], b[key]), (label, key)
    assert a["got"].equal(b["got"], ("traj", "dt", "times")), label


@pytest.fixture(scope="module")
def live(eng):
    """per event form: the stream, its packed planes, the filters' start, the one-shot front-end's window"""
    made = {}

    def get(form):
        if form not in made:
            ev = _live_stream()
            planes = _pack(eng, ev, form)
            win, counts = eng.run_frontend(ev, ALPHA, events=form)
            made[form] = dict(ev=ev, planes=planes, state=_resumed(K, 45), win=win, counts=counts, runs={})
        return made[form]
    return get


def _live_run(eng, live, form, name):
    w = live(form)
    if name not in w["runs"]:
        cuts = _cuts(w["planes"].shape[0])[name]
        w["runs"][name] = _live(eng, w["ev"], form, cuts, True, state=w["state"], planes=w["planes"])
    return w["runs"][name]


@pytest.mark.parametrize("name", ["one", "1", "3", "7", "random"])
def test_fp64_event_session_exports_the_frontends_records(eng, live, name):
    w = live("f64")
    t = w["ev"]["times"]
    assert (np.diff(t, axis=0) < 0).any() and (np.diff(t, axis=0) > 2**31).any()     # a step back, a pause of seconds
    assert w["counts"].max() > 10 and len(set(w["counts"])) > 5 and w["counts"][LANES].min() > 0
    run = _live_run(eng, live, "f64", name)
    assert np.array_equal(run["total"], w["counts"])
    _rows_equal(run["got"], _window_arrays(w["win"]), w["counts"])
    assert _same(run["refs"], w["win"].refs.download((K, 6), np.float64))
    # the export does not disturb the launch: the same session fed without records
    cuts = _cuts(w["planes"].shape[0])[name]
    plain = _live(eng, w["ev"], "f64", cuts, False, state=w["state"], planes=w["planes"])
    assert plain["got"].windows == 0 and run["got"].windows == len(cuts)
    _launch_outputs_equal(run, plain, name)
    assert _same(run["got"].f["rdt"], run["got"].f["dt"])        # the record's dt is the dt its pose was applied with


@pytest.mark.parametrize("name", ["one", "1", "3", "7", "random"])
def test_f32_event_session_exports_what_the_filter_was_fed(eng, live, name):
    w = live("f32")
    rec = w["win"].download_filters(np.arange(K))                   # the 40 B records, f32 gyro / acc / mag
    t = w["ev"]["times"]
    assert synth.has_time_events(w["planes"]) and (np.diff(t, axis=0) < 0).any()
    assert w["win"].dtx is not None and (rec.dt_ns[np.arange(rec.dtw.shape[0])[:, None] < w["counts"]] >= 2.0**31).any()
    run = _live_run(eng, live, "f32", name)
    got = run["got"]
    assert np.array_equal(run["total"], w["counts"])
    for k in range(K):
        n = int(w["counts"][k])
        assert _same(got.f["gyro"][:n, k], rec.gyro[:n, k].astype(np.float64)), k     # the f32 gyro, widened
        assert _same(got.f["rdt"][:n, k], rec.dt_ns[:n, k]), k                        # the dt word or its dtx entry
        assert _same(got.f["acc"][:n, k].astype(np.float32), rec.acc[:n, k]), k       # Rec = float32(RecLpf)
        assert _same(got.f["mag"][:n, k].astype(np.float32), rec.mag[:n, k]), k
        assert np.isnan(got.f["gyro"][n:, k]).all()
    assert np.abs(got.f["acc"] - got.f["acc"].astype(np.float32))[np.isfinite(got.f["acc"])].max() > 0   # FP64 kept
    # all cuttings agree in the FP64 values, and with the session fed without records in the rest
    assert got.equal(_live_run(eng, live, "f32", "7")["got"], [n for n, _ in FIELDS])
    cuts = _cuts(w["planes"].shape[0])[name]
    _launch_outputs_equal(run, _live(eng, w["ev"], "f32", cuts, False, state=w["state"], planes=w["planes"]), name)


def _replay(eng, got, refs, total, state, q=1.0, r=0.1):
    """the concatenated records of a whole session through the multi-record run, from the session's X0 / P0"""
    rows = max(2, int(total.max()))
    a = {name: np.nan_to_num(got.f[name][:rows]) for name in RECORD}
    ok = np.isfinite(refs).all(axis=1)
    safe = np.where(ok[:, None], refs, [0.0, 0.0, 1.0, 1.0, 0.0, 0.0])       # (a phone that is not ready: 0 records)
    win = eng.RecordWindow64.from_arrays(a["gyro"], a["rdt"], a["acc"], a["mag"], safe[:, :3], safe[:, 3:])
    f = eng.BatchedEKF(K, q, r)
    f.set_state(*state)
    traj = f.run(win, n_steps=rows, want_traj=True, counts=total)
    return f.get_state() + (traj,)


@pytest.mark.parametrize("form", ["f64", "f32"])
def test_replay_of_a_live_sessions_records(eng, live, form):
    """On FP64 events bit for bit (P too, as tests/test_live.py's FP64 split pipeline: array_equal).  On f32 events
    within ATOL_F64_CHAIN; measured on an MI355X: 0.0 (the same ekf_record_step on the same doubles)."""
    w = live(form)
    run = _live_run(eng, live, form, "7")
    X, P, traj = _replay(eng, run["got"], run["refs"], run["total"], w["state"])
    m = np.arange(len(traj))[:, None] < run["total"][None, :]
    mine = run["got"].f["traj"][:len(traj)]
    assert run["total"].min() > 0
    worst = max(float(np.abs(traj[m] - mine[m]).max()), float(np.abs(X - run["X"]).max()))
    print("replay of the %s-event session's records vs the session: max |dX| = %.3e" % (form, worst))
    if form == "f64":
        assert _same(traj[m], mine[m]) and _same(X, run["X"]) and _same(P, run["P"])
    else:
        assert worst <= ATOL_F64_CHAIN


def test_row_cap(eng, live):
    w = live("f64")
    full = _live_run(eng, live, "f64", "one")
    f = eng.BatchedEKF(K)
    f.set_state(*w["state"])
    s = eng.LiveSession(f, w["ev"]["init_acc"], w["ev"]["init_mag"], w["ev"]["t_init"], alpha=ALPHA, events="f64")
    buf = eng.DeviceBuffer(w["planes"].nbytes).upload(w["planes"])
    counts, out = s.feed_planes(buf, w["planes"].shape[0], trajectory=5, records=True)
    win = out["records"]
    assert win.window == 5 and out["trajectory"].shape == (5, K, 4)
    assert np.array_equal(counts, w["counts"]) and counts.max() > 5                           # the full counts
    assert np.array_equal(win.counts, np.minimum(counts, 5))                                  # the window's: capped
    got = Got(5)
    got.add(counts, out)                                        # (rows >= the capped counts are 0xFF: checked there)
    for name, _ in FIELDS:
        assert _same(got.f[name], full["got"].f[name][:5]), name
    assert _same(f.get_state()[0], full["X"])                   # records past the cap are applied, not stored


def test_rows_past_the_cap_keep_their_bytes(eng, live, monkeypatch):
    """The planes made four rows longer than the cap the launch is given: rows >= 5 are still 0xFF"""
    w = live("f64")
    full = _live_run(eng, live, "f64", "one")
    make = eng._chunk_records
    monkeypatch.setattr(eng, "_chunk_records", lambda rows, batch: make(rows + 4, batch))
    f = eng.BatchedEKF(K)
    f.set_state(*w["state"])
    s = eng.LiveSession(f, w["ev"]["init_acc"], w["ev"]["init_mag"], w["ev"]["t_init"], alpha=ALPHA, events="f64")
    buf = eng.DeviceBuffer(w["planes"].nbytes).upload(w["planes"])
    counts, out = s.feed_planes(buf, w["planes"].shape[0], trajectory=5, records=True)
    win = out["records"]
    assert win.window == 9 and out["trajectory"].shape == (5, K, 4) and counts.max() > 9
    g, dt, a, m, _ = win.download_filters(np.arange(K))
    for name, arr in (("gyro", g), ("rdt", dt), ("acc", a), ("mag", m)):
        assert (_bits(arr[5:]) == ONES).all(), name
        written = np.arange(5)[:, None] < counts[None, :]
        assert _same(arr[:5][written], full["got"].f[name][:5][written]), name


# ------------------------------------------------------------------ PhoneSession

def _phone_planes(n, seed, frac=(0.5, 0.62), late=0.8):
    """(phase2, phase3) of n rows on one timeline (tests/test_phone_session.py's, with phase 2 long enough for
    n_avg = 10): phones out of step; k % 7 == 2 never ready (8 messages); k % 7 == 4 ready long before its first
    phase-3 message; k % 11 == 5 phase 2 to the end."""
    gen = synth.generate_events(np.arange(K), n, seed=seed)
    rng = np.random.default_rng(seed)
    k = np.arange(K)
    s = rng.integers(0, n // 10, K)
    L2 = rng.integers(int(frac[0] * n), int(frac[1] * n), K)
    L2[k % 7 == 4] = int(late * n)
    L2[k % 11 == 5] = n
    L2[k % 7 == 2] = 8
    rows = np.arange(n)[:, None]
    in2, in3 = (rows >= s) & (rows < s + L2), rows >= s + L2
    common = dict(values=gen["values"], values64=wire.server_values(gen["values"]), times=gen["times"],
                  t_init=gen["t_init"])
    return (dict(common, types=np.where(in2, gen["types"], synth.EV_NONE).astype(np.uint32)),
            dict(common, types=np.where(in3, gen["types"], synth.EV_NONE).astype(np.uint32)))


KEYS = ("types", "values", "values64", "times")
DEAD = 2            # a phone that never gets ready


def _rows(ev, a, b):
    return {key: ev[key][a:b] for key in KEYS}


def _phone_session(eng, t_start, state, q=1.0, r=0.1, n_cal=None):
    f = eng.BatchedEKF(K, q, r)
    f.set_state(*state)
    return f, eng.PhoneSession(f, n_avg=N_AVG, alpha=ALPHA, t_start=t_start, n_cal=n_cal)


def _feed(s, got, p2, p3, cuts, records=True, between=None):
    ready = None
    for a, b in cuts:
        if between:
            between(int(a))
        counts, ready, out = s.feed(_rows(p2, int(a), int(b)), _rows(p3, int(a), int(b)), trajectory=True,
                                    records=records)
        got.add(counts, out)
    return ready


def _phone(eng, p2, p3, cuts, state, records=True, q=1.0, r=0.1):
    f, s = _phone_session(eng, p2["t_init"], state, q, r)
    got = Got(len(p3["types"]) // 3 + 2)
    ready = _feed(s, got, p2, p3, cuts, records)
    X, P = f.get_state()
    return dict(X=X, P=P, refs=s.refs, total=s.total_counts, got=got, ready=ready, session=s)


@pytest.fixture(scope="module")
def phones(eng):
    """The planes, the one-shot front-end on them (phase 2's outputs handed to run_frontend on the phase-3 plane),
    and the session fed in chunks of 7 with records"""
    p2, p3 = _phone_planes(EP, 41)
    state = _resumed(K, 48)
    init = eng.frontend_init(p2, N_AVG, stats=False, events="f64")
    ready = init["ready"]
    k = np.arange(K)
    assert not ready[k % 7 == 2].any() and ready[LANES].all() and ready.sum() > K // 2 and not ready[DEAD]
    ev3 = dict(p3, init_acc=init["init"][:, :3], init_mag=init["init"][:, 3:], t_init=init["t_init"])
    win, counts = eng.run_frontend(ev3, ALPHA, events="f64")
    assert counts[LANES].min() > 0 and len(set(counts[ready])) > 2
    first3 = np.argmax(p3["types"] != synth.EV_NONE, axis=0)
    assert len(set(first3[ready])) > 10                                   # out of step: they join in different chunks
    assert (p3["types"][:, ~ready] != synth.EV_NONE).any(axis=0).all()   # never ready, with phase-3 messages
    base = _phone(eng, p2, p3, _cuts(EP)["7"], state)
    return dict(p2=p2, p3=p3, state=state, init=init, ready=ready, win=win, counts=counts, base=base)


def _phone_records_are_the_frontends(run, w):
    ready = w["ready"]
    assert np.array_equal(run["ready"], ready)
    assert np.array_equal(run["total"][ready], w["counts"][ready]) and np.all(run["total"][~ready] == 0)
    _rows_equal(run["got"], _window_arrays(w["win"]), w["counts"], cols=np.flatnonzero(ready))
    # a phone that is never ready: no row written (Got.add saw 0xFF everywhere), nothing collected
    for name in RECORD:
        assert np.isnan(run["got"].f[name][:, ~ready]).all()


@pytest.mark.parametrize("name", ["1", "3", "7", "random"])
def test_phone_session_exports_the_frontends_records(eng, phones, name):
    w = phones
    run = w["base"] if name == "7" else _phone(eng, w["p2"], w["p3"], _cuts(EP)[name], w["state"])
    _phone_records_are_the_frontends(run, w)
    assert run["got"].equal(w["base"]["got"], [n for n, _ in FIELDS])
    if name == "7":     # the export does not disturb the launch
        plain = _phone(eng, w["p2"], w["p3"], _cuts(EP)["7"], w["state"], records=False)
        _launch_outputs_equal(run, plain)
        # ... and the replay of the whole session's records is the session
        X, P, traj = _replay(eng, run["got"], run["refs"], run["total"], w["state"])
        m = np.arange(len(traj))[:, None] < run["total"][None, :]
        ran = run["total"] > 0
        assert _same(traj[m], run["got"].f["traj"][:len(traj)][m])
        assert _same(X[ran], run["X"][ran]) and _same(P[ran], run["P"][ran])


def test_frames_with_records_equal_the_parsed_dicts(eng):
    n2, n3 = 70, 36
    ph2 = synth.generate_events(np.arange(K), n2, seed=65)
    ph3 = synth.generate_events(np.arange(K), n3, seed=66)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    texts, lens = [], []
    for k in range(K):
        m2, m3 = (9 if k % 9 == 4 else n2 - 2 * (k % 6)), n3 - 5 * (k % 4)
        lens.append((m2, m3))
        texts.append(wire.events_text(ph2["types"][:m2, k], ph2["values"][:m2, k], ph2["times"][:m2, k], phase=2) +
                     wire.events_text(ph3["types"][:m3, k], ph3["values"][:m3, k], ph3["times"][:m3, k], phase=3))
    fr = wire.frames(texts)
    F = fr.shape[0]
    # the same frames as parsed dicts: row f of each plane is frame f's message of that phase
    d2, d3 = (dict(types=np.full((F, K), synth.EV_NONE, np.uint32), values=np.zeros((F, K, 3), np.float32),
                   times=np.zeros((F, K), np.int64)) for _ in range(2))
    for k, (m2, m3) in enumerate(lens):
        for key in ("types", "values", "times"):
            d2[key][:m2, k] = ph2[key][:m2, k]
            d3[key][m2:m2 + m3, k] = ph3[key][:m3, k]
    for d in (d2, d3):
        d["values64"] = wire.server_values(d["values"])
    state = _resumed(K, 52)
    cuts = _cuts(F)["7"]
    by_frames, by_dicts = Got(F // 3 + 2), Got(F // 3 + 2)
    f1, s1 = _phone_session(eng, None, state)
    f2, s2 = _phone_session(eng, None, state)
    for a, b in cuts:
        counts, ready, out = s1.feed_frames(fr[a:b], trajectory=True, records=True)
        by_frames.add(counts, out)
        counts2, ready2, out2 = s2.feed(_rows(d2, a, b), _rows(d3, a, b), trajectory=True, records=True)
        by_dicts.add(counts2, out2)
        assert np.array_equal(counts, counts2) and np.array_equal(ready, ready2)
    assert by_frames.pos.max() > 1 and (by_frames.pos > 0).sum() > K // 2
    assert by_frames.equal(by_dicts, [n for n, _ in FIELDS])
    assert _same(f1.get_state()[0], f2.get_state()[0])


def test_calibrating_session_replays_its_corrected_records(eng):
    """n_cal = 20, phones in the client's order: the records are the corrected ones (the server's Mag_1), so their
    replay is the session's trajectory bit for bit, and they differ from the uncalibrated session's."""
    n1, n2, n3 = N_CAL + 1, 70, 36
    ph1 = synth.generate_calibration_events(K, n1, seed=91)
    A, h = ph1["soft"], ph1["hard"]
    ph2 = synth.generate_events(np.arange(K), n2, seed=92)
    ph3 = synth.generate_events(np.arange(K), n3, seed=93)
    t1 = ph1["times"][-1]
    ph2 = dict(ph2, times=ph2["times"] - ph2["t_init"][None, :] + t1[None, :], t_init=t1)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    for ph in (ph2, ph3):
        m = np.einsum("kij,ekj->eki", A, ph["values"].astype(np.float64)) + h[None]
        ph["values"] = np.where((ph["types"] == synth.EV_MAG)[..., None], m.astype(np.float32), ph["values"])
    ph1, ph2, ph3 = (dict(p, values64=wire.server_values(p["values"])) for p in (ph1, ph2, ph3))
    state = _resumed(K, 94)
    none = dict(types=np.zeros((0, K), np.uint32), values=np.zeros((0, K, 3), np.float32),
                values64=np.zeros((0, K, 3)), times=np.zeros((0, K), np.int64))
    runs = []
    for n_cal in (N_CAL, None):
        f, s = _phone_session(eng, ph2["t_init"], state, n_cal=n_cal)
        got = Got((n2 + n3) // 3 + 2)
        if n_cal:
            for a, b in _cuts(n1)["7"]:
                counts, ready, out = s.feed(none, none, trajectory=True, records=True, phase1=_rows(ph1, a, b))
                got.add(counts, out)
        for p2, p3, n in ((ph2, none, n2), (none, ph3, n3)):
            for a, b in _cuts(n)["7"]:
                counts, ready, out = s.feed(_rows(p2, a, b) if p2 is not none else none,
                                            _rows(p3, a, b) if p3 is not none else none, trajectory=True, records=True)
                got.add(counts, out)
        X, P = f.get_state()
        runs.append(dict(X=X, P=P, refs=s.refs, total=s.total_counts, got=got, ready=ready, session=s))
    cal, raw = runs
    assert cal["session"].calibration["calibrated"].sum() > K // 2
    assert cal["ready"].sum() > K // 2 and cal["total"][cal["ready"]].min() > 0
    X, P, traj = _replay(eng, cal["got"], cal["refs"], cal["total"], state)
    m = np.arange(len(traj))[:, None] < cal["total"][None, :]
    ran = cal["total"] > 0
    assert _same(traj[m], cal["got"].f["traj"][:len(traj)][m])
    assert _same(X[ran], cal["X"][ran]) and _same(P[ran], cal["P"][ran])
    both = np.flatnonzero((cal["total"] > 0) & (raw["total"] > 0))
    assert len(both) > K // 2
    assert all(np.abs(cal["got"].f["mag"][0, k] - raw["got"].f["mag"][0, k]).max() > 1e-3 for k in both)
    assert cal["got"].equal(raw["got"], ("gyro", "rdt"), both)       # the correction touches the magnetometer alone


# ------------------------------------------------------------------ per-filter noise

def _noise():
    deal = np.arange(K) % 4
    return np.array([PAIRS[d][0] for d in deal]), np.array([PAIRS[d][1] for d in deal])


@pytest.mark.parametrize("kind", ["live f64", "live f32", "phone"])
def test_per_filter_noise(eng, live, phones, kind):
    q, r = _noise()
    if kind == "phone":
        w = phones
        scalar = w["base"]
        cuts = _cuts(EP)["7"]
        noisy = _phone(eng, w["p2"], w["p3"], cuts, w["state"], True, q, r)
        plain = _phone(eng, w["p2"], w["p3"], cuts, w["state"], False, q, r)
    else:
        form = kind.split()[1]
        w = live(form)
        scalar = _live_run(eng, live, form, "7")
        cuts = _cuts(w["planes"].shape[0])["7"]
        noisy = _live(eng, w["ev"], form, cuts, True, q, r, state=w["state"], planes=w["planes"])
        plain = _live(eng, w["ev"], form, cuts, False, q, r, state=w["state"], planes=w["planes"])
    assert noisy["got"].equal(scalar["got"], RECORD + ("dt", "times"))    # records do not depend on the noise
    _launch_outputs_equal(noisy, plain, kind)                               # poses: the noise session's, undisturbed
    pair0 = np.flatnonzero((np.arange(K) % 4 == 0) & (scalar["total"] > 0))  # PAIRS[0] is the scalar filter's (1, 0.1)
    other = np.flatnonzero((np.arange(K) % 4 != 0) & (scalar["total"] > 1))
    assert noisy["got"].equal(scalar["got"], ("traj",), pair0)
    assert len(other) > K // 5 and (np.abs(noisy["X"] - scalar["X"])[other].max(axis=1) > 1e-9).mean() > 0.9


# ------------------------------------------------------------------ recycle and move

def test_a_recycled_column_exports_a_new_sessions_records(eng, phones):
    w = phones
    R = 21                                                    # three chunks of 7: the phones are still in phase 2
    C = np.array([64, 3, 69, 9, 63, 2, 44, 129, 0, 1, 6, 7, 8, 10, 12])
    g2, g3 = _phone_planes(EP - R, 77, frac=(0.6, 0.7), late=0.85)         # the next phones' rows
    fresh = _phone(eng, g2, g3, _cuts(EP - R)["7"], w["state"])             # ... in a new session
    assert (fresh["total"][C] > 0).sum() >= 4
    p2, p3 = ({key: w[p][key].copy() for key in KEYS} for p in ("p2", "p3"))
    for mine, theirs in ((p2, g2), (p3, g3)):
        for key in KEYS:
            mine[key][R:, C] = theirs[key][:, C]
    f, s = _phone_session(eng, w["p2"]["t_init"], w["state"])
    before, after = Got(EP // 3 + 2), Got(EP // 3 + 2)
    _feed(s, before, p2, p3, _cuts(EP)["7"][:R // 7])
    X0, P0 = w["state"]
    s.recycle(C, t_start=g2["t_init"][C], X0=X0[C], P0=P0[C])
    _feed(s, after, p2, p3, _cuts(EP)["7"][R // 7:])
    assert after.equal(fresh["got"], [n for n, _ in FIELDS], C)            # a new session's records, bit for bit
    assert np.all(before.pos[C] == 0)
    # every other column: the never-recycled session's records, before and after the recycle
    others = np.setdiff1d(np.arange(K), C)
    base = w["base"]["got"]
    for k in others:
        nb, na = int(before.pos[k]), int(after.pos[k])
        assert nb + na == w["base"]["total"][k]
        for name, _ in FIELDS:
            assert _same(np.concatenate([before.f[name][:nb, k], after.f[name][:na, k]]), base.f[name][:nb + na, k])
    assert _same(f.get_state()[0][others], w["base"]["X"][others])


def test_a_moved_phone_exports_the_never_moved_sessions_records(eng, phones):
    w = phones
    R = 98                                                    # fourteen chunks of 7: phones in every stage
    k = np.arange(K)
    dst = np.flatnonzero(k % 7 == 2)[:6]                      # free for the test: phones that never get ready
    src = np.array([63, 64, 0, 129, 11, 46])                  # lanes of both waves' edges; 11 % 7 == 4: ready, waiting
    assert not w["ready"][dst].any() and w["ready"][src].all()
    p2, p3 = ({key: w[p][key].copy() for key in KEYS} for p in ("p2", "p3"))
    for plane in (p2, p3):
        for key in KEYS:
            plane[key][R:, dst] = plane[key][R:, src]
        plane["types"][R:, src] = synth.EV_NONE
    f, s = _phone_session(eng, w["p2"]["t_init"], w["state"])
    before, after = Got(EP // 3 + 2), Got(EP // 3 + 2)
    _feed(s, before, p2, p3, _cuts(EP)["7"][:R // 7])
    assert 0 < (before.pos[src] > 0).sum() and (w["base"]["total"][src] > before.pos[src]).sum() >= 4
    s.move(src, dst)
    _feed(s, after, p2, p3, _cuts(EP)["7"][R // 7:])
    base = w["base"]["got"]
    others = np.setdiff1d(k, np.concatenate([src, dst]))
    for a, b in list(zip(src, dst)) + [(c, c) for c in others]:
        nb, na = int(before.pos[a]), int(after.pos[b])
        assert nb + na == w["base"]["total"][a], (a, b)
        for name, _ in FIELDS:
            assert _same(np.concatenate([before.f[name][:nb, a], after.f[name][:na, b]]), base.f[name][:nb + na, a])
    assert np.all(after.pos[src] == 0)
    X = f.get_state()[0]
    assert _same(X[dst], w["base"]["X"][src]) and _same(X[others], w["base"]["X"][others])


# ------------------------------------------------------------------ the log

def test_session_log_is_write_log_of_the_one_shot_arrays(eng, phones, tmp_path):
    w = phones
    cols = LANES + [DEAD]
    paths = [tmp_path / ("phone%d.txt" % c) for c in cols]
    f, s = _phone_session(eng, w["p2"]["t_init"], w["state"])
    log = eng.SessionLog(s, cols, paths)
    for a, b in _cuts(EP)["7"]:
        out = s.feed(_rows(w["p2"], a, b), _rows(w["p3"], a, b), records=True)
        log.append(out[-1])
    # the one-shot arrays: run_frontend's records and side outputs, the one-launch trajectory and record times
    one = eng.BatchedEKF(K)
    one.set_state(*w["state"])
    out = eng.run_session(w["p2"], w["p3"], one, n_avg=N_AVG, alpha=ALPHA, events="f64", trajectory=True)
    rec = _window_arrays(w["win"])
    refs = w["win"].refs.download((K, 6), np.float64)
    q_gyro = w["win"].gyro_chain(want_traj=True)[1]
    wahba = w["win"].wahba_quaternions()
    assert np.array_equal(out["counts"], s.total_counts)
    for c, path in zip(cols, paths):
        n = int(out["counts"][c])
        if c == DEAD:
            assert n == 0 and not path.exists()
            continue
        assert n > 0
        want = io.StringIO()
        logformat.write_log(want, [w["init"]["t_init"][c]] + list(out["record_times_ns"][:n, c]), rec["gyro"][:n, c],
                            rec["acc"][:n, c], rec["mag"][:n, c], refs[c, :3], refs[c, 3:], q_gyro[:n, c],
                            out["trajectory"][:n, c], wahba[:n, c])
        assert path.read_text() == want.getvalue(), c
    back = eng.RecordWindow64.from_logs(paths[:-1])
    assert np.array_equal(back.counts, s.total_counts[LANES])
    # what SessionLog refuses on a live session: a chunk without records, a chunk whose cap cut a listed column
    f2, s2 = _phone_session(eng, w["p2"]["t_init"], w["state"])
    log2 = eng.SessionLog(s2, LANES, [tmp_path / ("x%d.txt" % c) for c in LANES])
    with pytest.raises(ValueError, match="records=True"):
        log2.append(s2.feed(_rows(w["p2"], 0, EP), _rows(w["p3"], 0, 91), trajectory=True)[-1])
    with pytest.raises(ValueError, match="row cap"):
        log2.append(s2.feed(None, _rows(w["p3"], 91, EP), trajectory=1, records=True)[-1])
