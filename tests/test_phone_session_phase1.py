"""Live sessions that calibrate from their own stream (engine.PhoneSession(..., n_cal=): per chunk
pekf_magcal_resume_dev on the phase-1 rows, pekf_magcal_apply_dev on the phase-2 / phase-3 rows, phase 2 resumed,
the join launch) against the one-shot sessions, whose kernels are not under test:
run_wire_session(frames, filters, calibration="frames", n_cal=...) and
run_session(..., calibration=calibrate_magnetometer(phase1, n_cal, events="f64")).

The contract: the session equals the one-shot bit for bit for every phone that has no phase-2 / phase-3
magnetometer message in a chunk before the chunk its fit fires in (the client's own order), and for every phone
that never fires; a phone outside that order keeps the magnetometer messages of those earlier chunks as they came.

70 phones (one wave and a 6-lane tail), n_cal = 20, n_avg = 10; phase 1 of 21 messages (phone 7: 20, never
calibrated), phase 2 of 60 rows, phase 3 of 40 rows with ragged lengths; a soft- and hard-iron distortion in all
three phases, as tests/test_wire_phase1.py's session_texts."""
import numpy as np
import pytest

from oracle import ekf_numpy
from oracle import frontend_numpy as fe
from poseestimationkf_amd import synth, wire

from . import magcal_numpy as mc
from .test_live import ATOL_F64_CHAIN
from .test_live_traj import _resumed
from .test_phone_session import Fed, _cuttings, _equals_one_shot, _rows

pytestmark = pytest.mark.gpu

K, N_CAL, N_AVG, E2, E3 = 70, 20, 10, 60, 40
SHORT = 7            # the phone with n_cal messages only
CAL_KEYS = ("bias", "W", "fit", "status", "calibrated")


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


def _with64(ev):
    return dict(ev, values64=wire.server_values(ev["values"]))


@pytest.fixture(scope="module")
def phases():
    """The three phases as event dicts on one timeline (values64: the server's parse of the phone's text)"""
    ph1 = synth.generate_calibration_events(K, N_CAL + 1, seed=91)
    A, h = ph1["soft"], ph1["hard"]
    ph2 = synth.generate_events(np.arange(K), E2, seed=92)
    ph3 = synth.generate_events(np.arange(K), E3, seed=93)
    t1 = ph1["times"][-1]
    ph2 = dict(ph2, times=ph2["times"] - ph2["t_init"][None, :] + t1[None, :], t_init=t1)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    for ph in (ph2, ph3):   # what the distorted magnetometer reports
        m = np.einsum("kij,ekj->eki", A, ph["values"].astype(np.float64)) + h[None]
        ph["values"] = np.where((ph["types"] == synth.EV_MAG)[..., None], m.astype(np.float32), ph["values"])
    n1 = np.where(np.arange(K) == SHORT, N_CAL, N_CAL + 1)
    n3 = E3 - 3 * (np.arange(K) % 4)
    ph1["types"][N_CAL, SHORT] = synth.EV_NONE
    ph3["types"] = np.where(np.arange(E3)[:, None] < n3[None, :], ph3["types"], synth.EV_NONE).astype(np.uint32)
    X0, P0 = _resumed(K, 94)
    return dict(ph1=_with64(ph1), ph2=_with64(ph2), ph3=_with64(ph3), n1=n1, n3=n3, X0=X0, P0=P0)


def _cal_bits_equal(got, want, label=""):
    for key in CAL_KEYS:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), "%s calibration[%s]" % (label, key)


def _chunk_of(row, edges):
    """the chunk (a, b) of `edges` = [(a, b), ...] that holds row `row` (the first non-empty one)"""
    return next(c for c, (a, b) in enumerate(edges) if a <= row < b)


# ------------------------------------------------------------------ frames

@pytest.fixture(scope="module")
def wired(eng, phases):
    """The phones' frames, where each phone's message n_cal + 1 and first magnetometer message of phases 2 / 3 sit
    among them, the one-shot wire session with calibration="frames" and the uncalibrated one"""
    p = phases
    texts = []
    for k in range(K):
        n1, n3 = int(p["n1"][k]), int(p["n3"][k])
        texts.append("".join(wire.events_text(ph["types"][:n, k], ph["values"][:n, k], ph["times"][:n, k], phase=i)
                             for i, ph, n in ((1, p["ph1"], n1), (2, p["ph2"], E2), (3, p["ph3"], n3))))
    fr = wire.frames(texts)
    fire = np.where(p["n1"] > N_CAL, N_CAL, -1)                       # the frame of message n_cal + 1
    mag23 = np.concatenate([p["ph2"]["types"], p["ph3"]["types"]]) == synth.EV_MAG
    first_mag = p["n1"] + np.argmax(mag23, axis=0)                    # the frame of the first one to be corrected
    assert mag23.any(axis=0).all()
    runs = []
    for calibration in ("frames", None):
        f = eng.BatchedEKF(K)
        f.set_state(p["X0"], p["P0"])
        out = eng.run_wire_session(fr, f, n_avg=N_AVG, calibration=calibration, n_cal=N_CAL, trajectory=True)
        runs.append(f.get_state() + (out,))
    cal = runs[0][2]["calibration"]
    assert cal["status"].tolist() == [1 if k == SHORT else 0 for k in range(K)]
    ready = runs[0][2]["ready"]                   # (60 rows hold more than n_avg magnetometer samples for two in three)
    assert K // 2 < ready.sum() < K and ready[SHORT] and runs[0][2]["counts"][ready].min() > 0
    return fr, fire, first_mag, runs[0], runs[1]


@pytest.mark.parametrize("name", ["7", "random", "one"])
def test_frames_in_chunks_equal_the_calibrating_wire_session(eng, phases, wired, name):
    fr, fire, first_mag, single, plain = wired
    F = fr.shape[0]
    cuts = {"7": [(a, min(a + 7, F)) for a in range(0, F, 7)], "random": _cuttings(F, 4)["random"],
            "one": [(0, F)]}[name]
    # every phone of the fixture meets the contract's condition under this cutting: none is exempt
    for k in range(K):
        assert fire[k] < 0 or _chunk_of(first_mag[k], cuts) >= _chunk_of(fire[k], cuts), k
    f = eng.BatchedEKF(K)
    f.set_state(phases["X0"], phases["P0"])
    s = eng.PhoneSession(f, n_avg=N_AVG, n_cal=N_CAL)
    fed = Fed(K, F // 3 + 1)
    for a, b in cuts:
        fed.add(s.feed_frames(fr[int(a):int(b)], trajectory=True))
    X, P = f.get_state()
    _equals_one_shot((X, P, s.refs, fed, s), single, "frames in chunks of " + name)
    _cal_bits_equal(s.calibration, single[2]["calibration"], name)
    # the phone with n_cal messages ends where the uncalibrated session ends; the others do not
    assert np.array_equal(X[SHORT], plain[0][SHORT]) and np.array_equal(P[SHORT], plain[1][SHORT])
    others = (np.arange(K) != SHORT) & single[2]["ready"]
    assert np.abs(X - plain[0]).max(axis=1)[others].min() > 1e-9


# ------------------------------------------------------------------ planes

def _feed(s, fed, p1, p2, p3, schedule, calibrations=None):
    """schedule: per chunk the row ranges ((a1, b1), (a2, b2), (a3, b3)) of the three planes"""
    for c, (r1, r2, r3) in enumerate(schedule):
        kw = dict(phase1=_rows(p1, *r1)) if calibrations is None else dict(calibration=calibrations[c])
        fed.add(s.feed(_rows(p2, *r2), _rows(p3, *r3), trajectory=True, **kw))


def _session(eng, phases, n_cal):
    f = eng.BatchedEKF(K)
    f.set_state(phases["X0"], phases["P0"])
    return f, eng.PhoneSession(f, n_avg=N_AVG, t_start=phases["ph2"]["t_init"], n_cal=n_cal), Fed(K, E3 // 3 + 1)


ON_TIME = [((0, 6), (0, 0), (0, 0)), ((6, 6), (0, 0), (0, 0)), ((6, 12), (0, 0), (0, 0)), ((12, 20), (0, 0), (0, 0)),
           ((20, 21), (0, 13), (0, 0)), ((21, 21), (13, 40), (0, 0)), ((21, 21), (40, 60), (0, 9)),
           ((21, 21), (60, 60), (9, 40)), ((21, 21), (60, 60), (40, 40))]


@pytest.fixture(scope="module")
def one_shot(eng, phases):
    p = phases
    calib = eng.calibrate_magnetometer(p["ph1"], n_cal=N_CAL, events="f64")
    f = eng.BatchedEKF(K)
    f.set_state(p["X0"], p["P0"])
    out = eng.run_session(p["ph2"], p["ph3"], f, n_avg=N_AVG, events="f64", calibration=calib, trajectory=True)
    assert K // 2 < out["ready"].sum() < K and out["ready"][SHORT] and out["counts"][out["ready"]].min() > 0
    return f.get_state() + (out,), calib


@pytest.fixture(scope="module")
def on_time(eng, phases):
    """The calibrating session over ON_TIME's chunks (shared: the planes route and the oracle check)"""
    f, s, fed = _session(eng, phases, N_CAL)
    _feed(s, fed, phases["ph1"], phases["ph2"], phases["ph3"], ON_TIME)
    return f.get_state() + (s.refs, fed, s)


def test_dict_chunks_with_phase1_equal_the_calibrated_one_shot(phases, one_shot, on_time):
    single, calib = one_shot
    # the contract's condition, for every phone: its fit fires in chunk 4, which holds phase 2's first rows
    fire = np.where(phases["n1"] > N_CAL, N_CAL, -1)
    assert all(fire[k] < 0 or _chunk_of(fire[k], [c[0] for c in ON_TIME]) == 4 for k in range(K))
    assert all(a == b for c in ON_TIME[:4] for a, b in c[1:])
    _equals_one_shot(on_time, single, "dict chunks")
    _cal_bits_equal(on_time[4].calibration, calib)
    assert calib["status"].tolist() == [1 if k == SHORT else 0 for k in range(K)]


def _late_plane(phases):
    """Phase 1 in 30 rows: the even phones' messages in rows 0..20; the odd phones send 15, pause, and send their
    last 6 from row 21 (k % 4 == 1) or row 24 (k % 4 == 3) on, after phase 2 has begun.  Phone 7 has 20 messages."""
    src = phases["ph1"]
    types = np.full((30, K), synth.EV_NONE, np.uint32)
    vals, v64 = np.zeros((30, K, 3), np.float32), np.zeros((30, K, 3))
    for k in range(K):
        n = int(phases["n1"][k])
        rows = np.arange(n) if k % 2 == 0 else np.r_[np.arange(15), (21 if k % 4 == 1 else 24) + np.arange(n - 15)]
        types[rows, k], vals[rows, k], v64[rows, k] = synth.EV_MAG, src["values"][:n, k], src["values64"][:n, k]
    times = src["t_init"][None, :] + 10_000_000 * (1 + np.arange(30))[:, None]
    return dict(types=types, values=vals, values64=v64, times=times)


LATE = [((0, 10), (0, 0), (0, 0)), ((10, 21), (0, 0), (0, 0)), ((21, 24), (0, 20), (0, 0)),
        ((24, 27), (20, 40), (0, 0)), ((27, 30), (40, 60), (0, 10)), ((30, 30), (60, 60), (10, 40))]


@pytest.fixture(scope="module")
def late(eng, phases):
    """The late plane, each phone's firing chunk worked out from its message counts, and the uninterrupted
    calibrating session over LATE's chunks"""
    p1 = _late_plane(phases)
    seen = np.cumsum(p1["types"] != synth.EV_NONE, axis=0)
    fire_row = np.where(seen[-1] > N_CAL, np.argmax(seen > N_CAL, axis=0), -1)
    fire_chunk = np.array([_chunk_of(r, [c[0] for c in LATE]) if r >= 0 else len(LATE) for r in fire_row])
    k = np.arange(K)
    assert np.all(fire_chunk[k % 2 == 0] == 1) and np.all(fire_chunk[(k % 4 == 1)] == 3)
    assert np.all(fire_chunk[(k % 4 == 3) & (k != SHORT)] == 4) and fire_chunk[SHORT] == len(LATE)
    f, s, fed = _session(eng, phases, N_CAL)
    _feed(s, fed, p1, phases["ph2"], phases["ph3"], LATE)
    return p1, fire_chunk, f.get_state() + (s.refs, fed, s)


def test_late_phones_keep_their_earlier_messages_as_they_came(eng, phases, one_shot, late):
    """Expected, from the machinery that exists: a session without n_cal fed the same chunks, each with the one-shot
    cal and a status that reads 1 for a phone until its firing chunk and its one-shot status from then on."""
    p1, fire_chunk, got = late
    calib = eng.calibrate_magnetometer(p1, n_cal=N_CAL, events="f64")
    _cal_bits_equal(calib, one_shot[1], "the late plane holds the same samples:")
    # the late phones are outside the contract's condition: magnetometer messages in chunks before their fit fires
    mag2 = phases["ph2"]["types"] == synth.EV_MAG
    for k in range(1, K, 2):
        if k != SHORT:
            assert mag2[:LATE[fire_chunk[k] - 1][1][1], k].any()
    calibrations = []
    for c in range(len(LATE)):
        status = np.where(c < fire_chunk, 1, calib["status"]).astype(np.int32)
        calibrations.append(dict(cal=calib["cal"], status=status,
                                 status_dev=eng.DeviceBuffer(4 * K).upload(status)))
    f, s, fed = _session(eng, phases, None)
    _feed(s, fed, None, phases["ph2"], phases["ph3"], LATE, calibrations)
    want = f.get_state() + (s.refs, fed, s)
    X, P, refs, gfed, gs = got
    assert np.array_equal(X, want[0]) and np.array_equal(P, want[1])
    assert np.array_equal(refs, want[2], equal_nan=True) and np.array_equal(gfed.ready, fed.ready)
    assert np.array_equal(gfed.total, fed.total)
    for a, b in ((gfed.got.traj, fed.got.traj), (gfed.got.dt, fed.got.dt), (gfed.got.times, fed.got.times)):
        assert np.array_equal(a, b, equal_nan=True)
    _cal_bits_equal(gs.calibration, calib)
    # and that is where the session differs from the one-shot one, which corrects every message: the late phones
    # averaged raw samples into mag0; the phones in the client's order equal the one-shot bit for bit
    single = one_shot[0]
    even = np.arange(K) % 2 == 0
    assert np.array_equal(X[even], single[0][even])
    assert np.array_equal(refs[even], single[2]["refs"][even], equal_nan=True)   # (NaN: a phone that is not ready)
    odd = ~even & (np.arange(K) != SHORT) & single[2]["ready"] & gfed.ready
    assert odd.sum() > 10 and np.all(np.abs(refs[odd] - single[2]["refs"][odd]).max(axis=1) > 1e-6)
    assert np.array_equal(X[SHORT], single[0][SHORT])


def test_snapshot_and_restore_carry_phase1(eng, phases, late):
    """A snapshot after chunk 2: the even phones have fired, the odd ones are mid-store (15 of their 20 samples in
    the state), phase 2 has begun.  Restored on other filters, the rest of the chunks give the uninterrupted bits."""
    p1, fire_chunk, whole = late
    f, s, fed = _session(eng, phases, N_CAL)
    _feed(s, fed, p1, phases["ph2"], phases["ph3"], LATE[:3])
    snap = s.snapshot()
    assert snap["n_cal"] == N_CAL and 0 < (snap["status"].view(np.int32) == 0).sum() < K - 1
    f.set_state(*_resumed(K, 95))                                   # the old session goes its own way
    _feed(s, Fed(K, E3 // 3 + 1), p1, phases["ph2"], phases["ph3"], LATE[3:4])
    f2 = eng.BatchedEKF(K)
    s2 = eng.PhoneSession.restore(f2, snap)
    assert s2.n_cal == N_CAL
    _feed(s2, fed, p1, phases["ph2"], phases["ph3"], LATE[3:])
    X, P = f2.get_state()
    assert np.array_equal(X, whole[0]) and np.array_equal(P, whole[1])
    assert np.array_equal(s2.refs, whole[2], equal_nan=True) and np.array_equal(fed.total, whole[3].total)
    for a, b in ((fed.got.traj, whole[3].got.traj), (fed.got.dt, whole[3].got.dt), (fed.got.times, whole[3].got.times)):
        assert np.array_equal(a, b, equal_nan=True)
    _cal_bits_equal(s2.calibration, whole[4].calibration)


def test_calibrating_session_follows_the_oracle_chain(phases, on_time):
    """The final X of the calibrated chunked session against the restatement end to end: magcal_numpy.calibrate /
    apply on the server's values, frontend_numpy (phase 2, phase 3) and ekf_numpy.run_filter from X0 / P0.  The
    bound is the project's for this chain, ATOL_F64_CHAIN = 1e-12; the worst distance is printed: 3.6e-14
    over 140 records on an MI355X."""
    p = phases
    X, _, refs, fed, _ = on_time
    ph1, ph2, ph3 = p["ph1"], p["ph2"], p["ph3"]
    cal = mc.calibrate(ph1["types"], ph1["values64"], n_cal=N_CAL)
    assert cal["status"].tolist() == [1 if k == SHORT else 0 for k in range(K)]
    v2 = mc.apply(ph2["values64"], ph2["types"], cal["bias"], cal["W"], cal["status"])
    v3 = mc.apply(ph3["values64"], ph3["types"], cal["bias"], cal["W"], cal["status"])
    worst, records = 0.0, 0
    for k in range(K):
        m3 = ph3["types"][:, k] != synth.EV_NONE
        iv = fe.initial_values(ph2["types"][:, k], v2[:, k], ph2["times"][:, k], n_avg=N_AVG)
        assert iv["ready"] == fed.ready[k]
        if not iv["ready"]:
            continue
        g, dt, a, m = fe.run_frontend(ph3["types"][m3, k], v3[m3, k], ph3["times"][m3, k], iv["acc"], iv["mag"],
                                      iv["t_init"])
        assert fed.total[k] == len(dt) > 0
        Xo, _, _ = ekf_numpy.run_filter(g, dt.astype(np.float64), a, m, refs[k, :3], refs[k, 3:], X0=p["X0"][k],
                                        P0=p["P0"][k], record=False)
        worst = max(worst, float(np.abs(X[k] - Xo).max()))
        records += len(dt)
    print("calibrating phone session vs the oracle chain: %.3e over %d records" % (worst, records))
    assert records > K and worst < ATOL_F64_CHAIN
