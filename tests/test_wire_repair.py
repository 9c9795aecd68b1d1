"""A refused wire frame is its phone's business, on the device: engine.wire_events / run_wire_session /
PhoneSession.feed_frames with refused="repair" against (1) the reference parser's recorded parse of every number
and message form (tests/golden/parser.npz), (2) the project's own clean path on twin frames -- the same messages
with the odd token printed as repr of the double it parses to --, (3) the batch whose stopped phones' frames are
blank from the frame that stopped them, (4) the one-shot repaired session for sessions fed in chunks; and (5) the
patch entry alone.  Every comparison is of bits.

Shapes: 73 phones x 3 frames for the forms; for the sessions K = 130 (lanes 0, 63, 64 and 129 = K - 1; three
waves) and F = 98 frames -- 22 phase-1 (n_cal = 20: with fewer samples most six-parameter fits fail), 40 phase-2
(n_avg = 3) and up to 36 phase-3 messages, about the fewest with which most phones calibrate, get ready and apply
records; frame rows are also parsed in 3 and 7
chunks (PEKF_WIRE_CHUNKS), so that k_wire_rows_finalize finds the stop in a later chunk."""
import numpy as np
import pytest

from poseestimationkf_amd import synth, wire

from .test_parser_golden import OBS_TIME, OBS_TYPE, OBS_VALUES, OK, THREW, load_golden, same_bits
from .test_phone_session import Fed, _equals_one_shot

pytestmark = pytest.mark.gpu

NONE_W = np.uint64(synth.EV64_NONE_W)
K, N_CAL, N_AVG = 130, 20, 3
E1, E2, E3 = 22, 40, 36
F = E1 + E2 + E3
P2, P3 = E1, E1 + E2     # the first phase-2 and the first phase-3 frame


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _plane(w, name, n_frames, batch):
    return _bits(w[name].download((n_frames, batch, 4), np.float64))


def _none_rows(n):
    out = np.zeros((n, 4), np.uint64)
    out[:, 3] = NONE_W
    return out


def _event(ty, values, t):
    out = np.empty(4, np.uint64)
    out[:3] = _bits(values)
    out[3] = _bits([float(t)])[0] | np.uint64(ty)
    return out


def _raw_bad(eng, fr, rows):
    """bad_frame of a raw pekf_wire_events_ext_dev call: the frames the device parser itself refuses"""
    from poseestimationkf_amd._lib import check, lib
    Fr, Kc = fr.shape[:2]
    b = [eng.DeviceBuffer(n) for n in (fr.nbytes, 32 * Fr * Kc, 32 * Fr * Kc, 8 * Kc, 4 * Kc, 4 * Kc, 4 * Kc, 4, 8)]
    b[0].upload(np.ascontiguousarray(fr))
    b[7].upload(np.zeros(1, np.int32))
    check(lib.pekf_wire_events_ext_dev(Kc, Fr, b[0].ptr, Fr, Fr, b[1].ptr, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr,
                                       b[6].ptr, b[7].ptr, b[8].ptr if rows else None, 1 if rows else 0, None))
    check(lib.pekf_device_sync())
    return b[6].download((Kc,), np.int32)


# ------------------------------------------------------------------ 1. every form

@pytest.mark.parametrize("phase1", [False, True])
@pytest.mark.parametrize("rows", [False, True])
def test_every_form_is_the_reference_parsers_message_or_stops_its_phone(eng, golden, rows, phase1):
    """Phone k sends a client frame, forms_frames[k], a client frame.  Where the reference threw, or the time is
    outside +-2^51 ns, the phone stops at frame 1 with one message; otherwise nothing stops it and its planes hold
    the reference's values and time in the right rows.  repaired: exactly the phones whose middle frame the device
    refused and the host took.  With refused="raise" the same call still raises."""
    z = golden
    names = list(z["forms_names"])
    N = len(names)
    assert N == 73
    t_plain = int(z["forms_time"][names.index("last_plain")])
    first = np.frombuffer(wire.message(3, 0, [0.5, 0.25, 4.0], 1000).encode(), np.uint8)
    fr = np.stack([np.tile(first, (N, 1)), z["forms_frames"],
                   np.tile(z["forms_frames"][names.index("last_plain")], (N, 1))])
    head, tail = _event(0, [0.5, 0.25, 4.0], 1000), _event(1, [1.0, 2.0, 3.0], t_plain)
    with pytest.raises(ValueError, match="not in the client's message form"):
        eng.wire_events(fr, frame_rows=rows, phase1=phase1, refused="raise")
    w = eng.wire_events(fr, frame_rows=rows, phase1=phase1, refused="repair")
    bad_raw = _raw_bad(eng, fr, rows)
    ev = {2: _plane(w, "ev2", 3, N), 3: _plane(w, "ev3", 3, N)}
    counts = {2: w["n2"], 3: w["n3"]}
    if phase1:
        ev[1], counts[1] = _plane(w, "ev1", 3, N), w["n1"]
    stopped = []
    for k, name in enumerate(names):
        out, obs = int(z["forms_outcome"][k]), int(z["forms_obs"][k])
        ph = int(z["forms_phase"][k]) - ord("0") if out == OK else 0
        too_late = out == OK and ph in (2, 3) and abs(int(z["forms_time"][k])) >= 2 ** 51 and obs & OBS_TIME
        want = {p: [] for p in ev}      # per plane: (row, event or None for "whatever the reference does not show")
        want[3].append((0, head))
        if out == THREW or too_late:
            assert w["bad_frame"][k] == 1 and not w["repaired"][k] and bad_raw[k] == 1, name
            stopped.append(name)
        else:
            assert w["bad_frame"][k] == -1, name
            assert w["repaired"][k] == (bad_raw[k] == 1), name
            if out == OK and ph in ev:
                want[ph].append((1, None))
            want[3].append((2, tail))
        for p, plane in ev.items():
            assert counts[p][k] == len(want[p]), (name, p)
            col = plane[:, k]
            held = {}
            for i, (f, e) in enumerate(want[p]):
                held[f if rows else i] = e
            for r in range(3):
                if r not in held:
                    assert np.array_equal(col[r], _none_rows(1)[0]), (name, p, r)
                elif held[r] is not None:
                    assert np.array_equal(col[r], held[r]), (name, p, r)
                else:           # the form's own message: the reference's fields where its state shows them
                    e = col[r]
                    want_type = int(z["forms_type"][k]) - ord("0") if obs & OBS_TYPE else synth.EV_OTHER
                    if p == 3 or obs & OBS_TYPE:   # (a Type the reference's state does not show in phase 3: no sensor's)
                        assert int(e[3] & np.uint64(3)) == (want_type if 0 <= want_type <= 2 else 3), name
                    if obs & OBS_VALUES:
                        assert same_bits(e[:3].view(np.float64), z["forms_values"][k]), name
                    if obs & OBS_TIME and p != 1:
                        assert (e[3:4] & ~np.uint64(3)).view(np.float64)[0] == float(z["forms_time"][k]), name
    assert {"x_huge", "missing_comma", "t_above_int64", "t_2pow51"} <= set(stopped)
    assert w["repaired"].sum() >= 14 and all(w["repaired"][names.index(n)] for n in ("x_hex", "x_blanks", "x_digits20"))
    if not rows:
        assert w["E3"] == int(w["n3"].max()) and w["ev3_from"] == 0


# ------------------------------------------------------------------ the sessions' batches

def _messages():
    """K phones' client messages as text, per phone a list of F frames' texts (99 characters and the newline):
    22 phase-1, 40 phase-2 and 36 - (k % 3) phase-3 messages, blank frames after them"""
    ph1 = synth.generate_calibration_events(K, E1, seed=91)
    A, h = ph1["soft"], ph1["hard"]
    ph2 = synth.generate_events(np.arange(K), E2, seed=92)
    ph3 = synth.generate_events(np.arange(K), E3, seed=93)
    t1 = ph1["times"][-1]
    ph2 = dict(ph2, times=ph2["times"] - ph2["t_init"][None, :] + t1[None, :])
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    for ph in (ph2, ph3):   # what the distorted magnetometer reports
        m = np.einsum("kij,ekj->eki", A, ph["values"].astype(np.float64)) + h[None]
        ph["values"] = np.where((ph["types"] == synth.EV_MAG)[..., None], m.astype(np.float32), ph["values"])
    out = []
    for k in range(K):
        msgs = [wire.message(p, ph["types"][i, k], ph["values"][i, k], ph["times"][i, k])
                for p, ph, n in ((1, ph1, E1), (2, ph2, E2), (3, ph3, E3 - k % 3)) for i in range(n)]
        out.append(msgs + [" " * 99 + "\n"] * (F - len(msgs)))
    return out


def _with_token(msg, token, text):
    """the client message with value token 0..2 replaced by text"""
    head, rest = msg.rstrip().split(":", 1)
    parts = rest.split(",")
    parts[token] = text
    out = (head + ":" + ",".join(parts)).ljust(99) + "\n"
    assert len(out) == 100
    return out


def _frames_of(msgs):
    return wire.frames(["".join(m) for m in msgs])


# (phone, frame, value token, the odd form): lanes 0, 63, 64 and 129, two phones of one wave (0 and 5, phone 5
# twice), every phase (frames below P2: phase 1; below P3: phase 2; then phase 3), frame 0 and the last frame
ODD = [(0, 0, 0, "0x1p3"), (5, 3, 1, "  2.5"), (5, P3 + 12, 0, "0x1p-1"), (63, P2 + 2, 2, "1.5abc"),
       (64, P2 + 4, 0, "1.2345678901234567890"), (129, F - 1, 1, "0x1p3"), (100, P3 + 2, 2, "\t3.25"),
       (70, P3 + 4, 0, "+1.5"), (71, P3 + 5, 1, "7"), (72, P3 + 6, 2, ".5"), (73, P3 + 7, 0, "5."),
       (74, P3 + 8, 1, "1e5")]
ODD_VALUE = {"0x1p3": 8.0, "  2.5": 2.5, "0x1p-1": 0.5, "1.5abc": 1.5, "1.2345678901234567890": 1.2345678901234567890,
             "\t3.25": 3.25, "+1.5": 1.5, "7": 7.0, ".5": 0.5, "5.": 5.0, "1e5": 1e5}
# what the device parser leaves to the host among them (tests/test_parser_golden_gpu.py, REFUSED_FORMS)
HOST_FORMS = {"0x1p3", "  2.5", "0x1p-1", "1.5abc", "1.2345678901234567890", "\t3.25"}


@pytest.fixture(scope="module")
def batches():
    """(plain messages, the batch with the odd forms, its twin): frames [F][K][100]"""
    plain = _messages()
    assert len(plain[129]) == F and plain[129][F - 1].startswith("#3")
    odd, twin = [list(m) for m in plain], [list(m) for m in plain]
    for k, f, token, form in ODD:
        assert plain[k][f][0] == "#" and plain[k][f][1] == ("1" if f < E1 else "2" if f < E1 + E2 else "3")
        odd[k][f] = _with_token(plain[k][f], token, form)
        twin[k][f] = _with_token(plain[k][f], token, repr(ODD_VALUE[form]))
    fo, ft = _frames_of(odd), _frames_of(twin)
    # the twin carries the same doubles, in the client's own form
    a, b = wire.parse_frames(fo.reshape(-1, 100)), wire.parse_frames(ft.reshape(-1, 100))
    for key in ("status", "phase", "types", "times"):
        assert np.array_equal(a[key], b[key])
    assert np.array_equal(_bits(a["values"]), _bits(b["values"]))
    return plain, fo, ft


def _same_wire_events(eng, got, want, phase1, label):
    """every plane row below its E, the counts, first_t2, the E's and ev3_from"""
    for key in ("E2", "E3", "ev3_from") + (("E1",) if phase1 else ()):
        assert got[key] == want[key], (label, key, got[key], want[key])
    for key in ("n2", "n3") + (("n1",) if phase1 else ()):
        assert np.array_equal(got[key], want[key]), (label, key)
    assert np.array_equal(got["first_t2"].download((K,), np.int64), want["first_t2"].download((K,), np.int64)), label
    for name, lo, n in (("ev2", 0, want["E2"]), ("ev3", want["ev3_from"], want["E3"])) + \
            ((("ev1", 0, want["E1"]),) if phase1 else ()):
        a, b = _plane(got, name, F, K), _plane(want, name, F, K)
        assert np.array_equal(a[lo:lo + n], b[lo:lo + n]), (label, name)


SESSION_KEYS = ("ready", "counts", "refs", "trajectory", "record_dt_ns", "record_times_ns")


def _session(eng, fr, rows=True, cal=None, **kw):
    f = eng.BatchedEKF(K)
    out = eng.run_wire_session(fr, f, n_avg=N_AVG, frame_rows=rows, calibration=cal, n_cal=N_CAL, trajectory=True, **kw)
    X, P = f.get_state()
    return X, P, out


def _same_sessions(a, b, label, phones=slice(None)):
    (Xa, Pa, oa), (Xb, Pb, ob) = a, b
    assert np.array_equal(_bits(Xa[phones]), _bits(Xb[phones])), label
    assert np.array_equal(_bits(Pa[phones]), _bits(Pb[phones])), label
    for key in SESSION_KEYS:
        x, y = np.asarray(oa[key], np.float64), np.asarray(ob[key], np.float64)
        assert x.shape == y.shape, (label, key, x.shape, y.shape)
        x, y = (x[:, phones], y[:, phones]) if key in SESSION_KEYS[3:] else (x[phones], y[phones])
        assert np.array_equal(_bits(x), _bits(y)), (label, key)
    if "calibration" in ob:
        for key in ("bias", "W", "fit", "status"):
            assert np.array_equal(_bits(oa["calibration"][key][phones].astype(np.float64)),
                                  _bits(ob["calibration"][key][phones].astype(np.float64))), (label, key)


# ------------------------------------------------------------------ 2. twins

@pytest.mark.parametrize("phase1", [False, True])
@pytest.mark.parametrize("rows,chunks", [(False, None), (True, None), (True, "3"), (True, "7")])   # (chunks: frame rows only)
def test_repaired_planes_equal_the_twins(eng, batches, rows, phase1, chunks, monkeypatch):
    if chunks:
        monkeypatch.setenv("PEKF_WIRE_CHUNKS", chunks)
    _, fo, ft = batches
    want = eng.wire_events(ft, frame_rows=rows, phase1=phase1)          # raises nothing
    # the phones the host has to take: those with a form the device parser leaves to it (HOST_FORMS), no others
    host_takes = np.zeros(K, bool)
    host_takes[[k for k, _, _, form in ODD if form in HOST_FORMS]] = True
    got = eng.wire_events(fo, frame_rows=rows, phase1=phase1, refused="repair")
    assert (got["bad_frame"] == -1).all() and np.array_equal(got["repaired"], host_takes)
    _same_wire_events(eng, got, want, phase1, "host frames")
    dev = (eng.DeviceBuffer(fo.nbytes).upload(fo), F, K)
    got_dev = eng.wire_events(dev, frame_rows=rows, phase1=phase1, refused="repair")
    assert (got_dev["bad_frame"] == -1).all() and np.array_equal(got_dev["repaired"], host_takes)
    _same_wire_events(eng, got_dev, want, phase1, "device frames")


@pytest.mark.parametrize("cal", [None, "frames"])
@pytest.mark.parametrize("rows", [True, False])
def test_repaired_session_equals_the_twins(eng, batches, rows, cal):
    _, fo, ft = batches
    want = _session(eng, ft, rows, cal)
    assert want[2]["ready"].sum() > K // 2 and (want[2]["counts"] > 0).sum() > K // 2
    if cal:
        assert want[2]["calibrated"].sum() > K // 2
    with pytest.raises(ValueError, match="phone 0, frame 0"):
        _session(eng, fo, rows, cal)
    got = _session(eng, fo, rows, cal, refused="repair")
    assert (got[2]["bad_frame"] == -1).all() and got[2]["repaired"].sum() == 6
    _same_sessions(got, want, "rows=%s cal=%s" % (rows, cal))


# ------------------------------------------------------------------ 3. stopped phones

def _throwing(msg, how):
    head, rest = msg.rstrip().split(":", 1)
    x, y, z, t = rest.split(",")
    rest = {"x_huge": ",".join(["1e999", y, z, t]), "missing_comma": x + " " + ",".join([y, z, t]),
            "t_above_int64": ",".join([x, y, z, "t:9223372036854775808"])}[how]
    return (head + ":" + rest).ljust(99) + "\n"


STOPS = [(3, P2 + 12, "x_huge"), (64, P3 - 1, "missing_comma"), (129, P3 + 22, "t_above_int64")]   # phase 2, its last frame, phase 3


def _stopped_batch(plain, stops):
    thrown, blank = [list(m) for m in plain], [list(m) for m in plain]
    for k, f, how in stops:
        thrown[k][f] = _throwing(plain[k][f], how)
        blank[k][f:] = [" " * 99 + "\n"] * (F - f)
    return _frames_of(thrown), _frames_of(blank)


@pytest.mark.parametrize("chunks", [None, "3"])
@pytest.mark.parametrize("cal", [None, "frames"])
def test_a_stopped_phone_is_a_stream_that_ended(eng, batches, cal, chunks, monkeypatch):
    if chunks:
        monkeypatch.setenv("PEKF_WIRE_CHUNKS", chunks)
    plain, _, _ = batches
    thrown, blank = _stopped_batch(plain, STOPS)
    want, whole = _session(eng, blank, True, cal), _session(eng, _frames_of(plain), True, cal)
    got = _session(eng, thrown, True, cal, refused="repair")
    bad = np.full(K, -1)
    for k, f, _ in STOPS:
        bad[k] = f
    assert np.array_equal(got[2]["bad_frame"], bad) and not got[2]["repaired"].any()
    _same_sessions(got, want, "stopped")
    others = np.array([k for k in range(K) if bad[k] < 0])
    for key in ("ready", "counts", "refs"):
        assert np.array_equal(_bits(got[2][key][others].astype(np.float64)),
                              _bits(whole[2][key][others].astype(np.float64))), key
    assert np.array_equal(_bits(got[0][others]), _bits(whole[0][others]))
    assert np.array_equal(_bits(got[1][others]), _bits(whole[1][others]))
    assert whole[2]["ready"][129] and got[2]["counts"][129] <= whole[2]["counts"][129]
    # compacted planes too
    got_c, want_c = _session(eng, thrown, False, cal, refused="repair"), _session(eng, blank, False, cal)
    _same_sessions(got_c, want_c, "stopped, compacted")


@pytest.mark.parametrize("chunks", [None, "7"])
def test_every_phone_refused_at_once_and_none(eng, batches, chunks, monkeypatch):
    if chunks:
        monkeypatch.setenv("PEKF_WIRE_CHUNKS", chunks)
    plain, _, _ = batches
    kinds = ("x_huge", "missing_comma", "t_above_int64")
    stops = [(k, (7 * k) % (F - 3), kinds[k % 3]) for k in range(K)]
    thrown, blank = _stopped_batch(plain, stops)
    got, want = _session(eng, thrown, True, "frames", refused="repair"), _session(eng, blank, True, "frames")
    assert got[2]["bad_frame"].tolist() == [f for _, f, _ in stops]
    _same_sessions(got, want, "every phone stopped")
    fr = _frames_of(plain)
    a, b = _session(eng, fr, True, "frames", refused="repair"), _session(eng, fr, True, "frames")
    assert (a[2]["bad_frame"] == -1).all() and not a[2]["repaired"].any()
    _same_sessions(a, b, "no refusal")


# ------------------------------------------------------------------ 4. chunked

def _fed_in_chunks(eng, fr, size, n_cal, between=None):
    f = eng.BatchedEKF(K)
    s = eng.PhoneSession(f, n_avg=N_AVG, n_cal=n_cal)
    fed = Fed(K, F // 3 + 1)
    bad, repaired = np.full(K, -1), np.zeros(K, bool)
    for a in range(0, F, size):
        out = s.feed_frames(fr[a:a + size], trajectory=True, refused="repair")
        assert len(out) == 5
        fed.add(out[:3])
        assert ((out[3] < 0) | (bad < 0)).all()              # a phone stops once
        bad = np.where(out[3] >= 0, a + out[3], bad)
        repaired |= out[4]
        assert np.array_equal(s.stopped, bad >= 0)
        if between:
            between(s, a + size)
    X, P = f.get_state()
    return (X, P, s.refs, fed, s), bad, repaired


@pytest.mark.parametrize("n_cal", [None, N_CAL])
@pytest.mark.parametrize("size", [1, 3, 7])
def test_sessions_fed_in_chunks_equal_the_one_shot_repair(eng, batches, size, n_cal):
    """The odd forms and the throwing frames together, fed in chunks: the one-shot repaired session bit for bit.
    The stopped phones' later frames are valid client frames and change nothing."""
    plain, _, _ = batches
    msgs = [list(m) for m in plain]
    for k, f, token, form in ODD:
        msgs[k][f] = _with_token(plain[k][f], token, form)
    for k, f, how in STOPS[:2] + [(5, P2 + 32, "x_huge")]:
        msgs[k][f] = _throwing(plain[k][f], how)
    fr = _frames_of(msgs)
    cal = "frames" if n_cal else None
    single = _session(eng, fr, True, cal, refused="repair")
    want_bad = np.full(K, -1)
    want_bad[[3, 64, 5]] = [P2 + 12, P3 - 1, P2 + 32]
    assert np.array_equal(single[2]["bad_frame"], want_bad)
    chunked, bad, repaired = _fed_in_chunks(eng, fr, size, n_cal)
    assert np.array_equal(bad, want_bad) and np.array_equal(repaired, single[2]["repaired"])
    assert np.array_equal(chunked[4].total_counts, chunked[3].total)
    _equals_one_shot(chunked, single, "chunks of %d" % size)
    if n_cal:
        for key in ("bias", "W", "fit", "status"):
            assert np.array_equal(_bits(chunked[4].calibration[key].astype(np.float64)),
                                  _bits(single[2]["calibration"][key].astype(np.float64))), key


def test_a_recycled_column_takes_the_next_phone(eng, batches):
    """Phone 5 stops at frame 24 (phase 2); its column is recycled at frame 28 and fed phone 7's whole stream from there: the
    column ends as a new session fed that stream does, and session.stopped follows."""
    plain, _, _ = batches
    msgs = [list(m) for m in plain]
    msgs[5][24] = _throwing(plain[5][24], "x_huge")
    fr = _frames_of(msgs)
    late = np.full((28 + F, K, 100), ord(" "), np.uint8)
    late[:F] = fr
    late[28:, 5] = _frames_of(plain)[:, 7]
    f = eng.BatchedEKF(K)
    s = eng.PhoneSession(f, n_avg=N_AVG)
    total = np.zeros(K, np.int64)
    for a in range(0, late.shape[0], 7):
        if a == 28:
            assert s.stopped.tolist() == [k == 5 for k in range(K)]
            s.recycle([5])
            assert not s.stopped.any()
            total[5] = 0
        out = s.feed_frames(late[a:a + 7], refused="repair")
        total += out[0]
        assert (out[2][5] == 3 if a == 21 else out[2][5] == -1) and (np.delete(out[2], 5) == -1).all()
    X, P = f.get_state()
    Xw, Pw, want = _session(eng, _frames_of(plain), True, None)
    assert not s.stopped.any() and want["counts"][7] > 0
    assert np.array_equal(_bits(X[5]), _bits(Xw[7])) and np.array_equal(_bits(P[5]), _bits(Pw[7]))
    assert total[5] == want["counts"][7] and np.array_equal(_bits(s.refs[5]), _bits(want["refs"][7]))
    keep = np.array([k for k in range(K) if k != 5])
    assert np.array_equal(_bits(X[keep]), _bits(Xw[keep])) and np.array_equal(total[keep], want["counts"][keep])


# ------------------------------------------------------------------ 5. the patch entry alone

def _patch(eng, Kp, rows_max, recs, cells, ev1=True, bounds=False, misalign=0, marker=0x7ff8dead0000beef):
    """Planes of rows_max rows filled with a marker, patched: (planes {1, 2, 3} (rows, Kp, 4) uint64, n1, n2, n3,
    first_t2, bad_frame, status, row bounds)"""
    from poseestimationkf_amd._lib import lib
    fill = np.full((rows_max, Kp, 4), marker, np.uint64)
    planes = [eng.DeviceBuffer(fill.nbytes).upload(fill) for _ in range(3)]
    small = [eng.DeviceBuffer(4 * Kp).upload(np.full(Kp, -7, np.int32)) for _ in range(4)]   # n1, n2, n3, bad
    t2 = eng.DeviceBuffer(8 * Kp).upload(np.full(Kp, -7, np.int64))
    bw = eng.DeviceBuffer(12).upload(np.full(3, -7, np.int32))
    cb = eng.DeviceBuffer(max(cells.nbytes, 16))
    if cells.nbytes:
        cb.upload(np.ascontiguousarray(cells))
    rb = eng.DeviceBuffer(max(recs.nbytes, 8))
    if recs.nbytes:
        rb.upload(np.ascontiguousarray(recs))
    st = lib.pekf_wire_patch_dev(Kp, len(recs), recs.ctypes.data, rb.ptr, cells.shape[1], cb.ptr if cells.shape[1] else None,
                                 rows_max if ev1 else 0, rows_max, rows_max, planes[0].ptr + misalign if ev1 else None,
                                 planes[1].ptr, planes[2].ptr, t2.ptr, small[0].ptr if ev1 else None, small[1].ptr,
                                 small[2].ptr, small[3].ptr, rows_max if bounds else 0, bw.ptr if bounds else None, None)
    lib.pekf_device_sync()
    got = {p + 1: planes[p].download((rows_max, Kp, 4), np.float64).view(np.uint64) for p in range(3)}
    return (got, [b.download((Kp,), np.int32) for b in small], t2.download((Kp,), np.int64), st,
            bw.download((3,), np.int32), fill)


@pytest.mark.parametrize("ev1", [True, False])
@pytest.mark.parametrize("Kp", [65, 130])
def test_the_patch_writes_the_listed_columns_rows_and_nothing_else(eng, Kp, ev1):
    from poseestimationkf_amd._lib import PEKF_ERR_INVALID, PEKF_OK
    rows_max = 9
    cols = [0, 63, 64, Kp - 1] if Kp > 65 else [0, 1, 63, 64]
    recs = np.zeros(4, eng._PATCH_COL)
    recs["col"] = cols
    recs["from_row"] = [[0, 0, 0], [3, 4, 5], [8, 8, 8], [9, 2, 0]]       # (9: no row of that plane at all)
    recs["n_cells"] = [[2, 0, 3], [1, 1, 1], [1, 0, 0], [0, 3, 0]]
    recs["n"] = [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]
    recs["bad_frame"] = [-1, 4, -1, 0]
    recs["first_t2"] = [11, 22, 33, 44]
    rng = np.random.default_rng(7)
    cells = rng.integers(1, 2 ** 62, (3, 3, 4, 4)).astype(np.uint64)
    got, small, t2, st, _, fill = _patch(eng, Kp, rows_max, recs, cells, ev1=ev1)
    assert st == PEKF_OK
    none = _none_rows(1)[0]
    for p in (1, 2, 3):
        want = fill.copy()
        if p > 1 or ev1:
            for i, c in enumerate(cols):
                r0, n = int(recs["from_row"][i, p - 1]), int(recs["n_cells"][i, p - 1])
                for r in range(r0, rows_max):
                    want[r, c] = cells[p - 1, r - r0, i] if r - r0 < n else none
        assert np.array_equal(got[p], want), p              # byte for byte: the other columns and rows are the marker
    listed = np.zeros(Kp, bool)
    listed[cols] = True
    for j, b in enumerate(small):    # n1, n2, n3, bad_frame
        want = np.full(Kp, -7, np.int32)
        if j or ev1:
            want[cols] = recs["bad_frame"] if j == 3 else recs["n"][:, j]
        assert np.array_equal(b, want), j
    assert np.array_equal(t2[cols], recs["first_t2"]) and (t2[~listed] == -7).all()
    # no column: nothing is written
    got, small, t2, st, _, fill = _patch(eng, Kp, rows_max, recs[:0], cells[:, :0, :0], ev1=ev1)
    assert st == PEKF_OK and all(np.array_equal(got[p], fill) for p in got) and (t2 == -7).all()
    # refused before any launch: misaligned planes, a column >= batch, a negative row
    if ev1:
        got, _, _, st, _, fill = _patch(eng, Kp, rows_max, recs, cells, misalign=8)
        assert st == PEKF_ERR_INVALID and all(np.array_equal(got[p], fill) for p in got)
    for field, value in (("col", Kp), ("from_row", -1)):
        bad = recs.copy()
        bad[field][2] = value
        got, _, t2, st, _, fill = _patch(eng, Kp, rows_max, bad, cells, ev1=ev1)
        assert st == PEKF_ERR_INVALID and all(np.array_equal(got[p], fill) for p in got) and (t2 == -7).all()


def test_the_patch_entrys_row_bounds_are_the_planes(eng):
    """row_bounds afresh: 1 + the last row with a phase-2 (phase-1) message, n_rows - the first with a phase-3 one"""
    Kp, rows_max = 130, 9
    recs = np.zeros(Kp, eng._PATCH_COL)     # every column blank, then messages in three of them
    recs["col"] = np.arange(Kp)
    recs["bad_frame"] = -1
    recs["n_cells"][[0, 64, 129]] = [[0, 0, 7], [6, 0, 0], [0, 4, 0]]
    cells = np.tile(_none_rows(1)[0], (3, 7, Kp, 1))
    cells[2, 6, 0] = cells[0, 5, 64] = cells[1, 3, 129] = _event(1, [1.0, 2.0, 3.0], 5)
    got, _, _, st, bw, _ = _patch(eng, Kp, rows_max, recs, cells, bounds=True)
    assert st == 0 and bw.tolist() == [4, rows_max - 6, 6]
    assert (got[3][6, 0] == cells[2, 6, 0]).all() and (got[3][:6, :, 3] == NONE_W).all()
    got, _, _, st, bw, _ = _patch(eng, Kp, rows_max, recs, cells[:, :0], bounds=True)    # n_cells above cell_rows
    assert st != 0
    recs["n_cells"] = 0
    got, _, _, st, bw, _ = _patch(eng, Kp, rows_max, recs, cells[:, :0], bounds=True)
    assert st == 0 and bw.tolist() == [0, 0, 0]
