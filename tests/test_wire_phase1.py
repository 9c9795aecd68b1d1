"""Phase 1 from wire frames on the device (csrc/pekf_wire_dev.hip's P1 kernels behind pekf_wire_events_p1_dev;
engine.wire_events(phase1=True), engine.run_wire_session(calibration="frames")): the phase-1 plane against the
host parse of the same text and against the reference's own parser (tests/golden/parser.npz), bit for bit, the
other planes against the parse without it, and the calibrated session against the route through the host parse.

Shapes: 150 / 129 / 70 / 65 phones (two full waves and a partial one, a ragged last 8-lane group), one to a few
frame indices for the two-slot DMA ring's edges."""
import numpy as np
import pytest

from poseestimationkf_amd import synth, wire

from .test_parser_golden import load_golden, same_bits

pytestmark = pytest.mark.gpu

NONE_W = np.uint64(synth.EV64_NONE_W)
T_2POW51 = 2251799813685248


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


def _frame(tokens, t, phase=1, ty=2):
    s = "#%s,%s:%s,%s,%s,t:%s" % (phase, ty, tokens[0], tokens[1], tokens[2], t)
    assert len(s) <= 99
    return s.ljust(99) + "\n"


def _fast_form(rng):
    """A number of the device's fast form: [-]D{1,8}.D+(E[-]D{1,2})? with at most 15 digits."""
    nI = int(rng.integers(1, 9))
    nF = int(rng.integers(1, 16 - nI))
    s = ("-" if rng.random() < 0.5 else "") + "".join(str(d) for d in rng.integers(0, 10, nI)) + "." + \
        "".join(str(d) for d in rng.integers(0, 10, nF))
    if rng.random() < 0.5:
        s += "E" + ("-" if rng.random() < 0.5 else "") + str(int(rng.integers(0, 23 if rng.random() < 0.5 else 60)))
    return s


def _host_planes(texts, phase, E):
    """The host parse's messages of one phase as [E][K] FP64 events, padded with the no-message event."""
    ev = wire.events_from_wire(texts, np.zeros((len(texts), 3)), np.zeros((len(texts), 3)),
                               np.zeros(len(texts), np.int64), phase=phase)
    p = synth.pack_events64(ev)
    out = np.empty((E, len(texts), 4))
    out[...] = NONE_W.view(np.float64)
    out[..., :3] = 0.0
    n = min(E, p.shape[0])
    out[:n] = p[:n]
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _plane(w, name, F, K):
    return w[name].download((F, K, 4), np.float64)


def _compact(planes, K):
    """[F][K] frame-row planes -> each phone's rows that are not the no-message event, in order."""
    w = _bits(planes[..., 3])
    return [planes[w[:, k] != NONE_W, k] for k in range(K)]


def _phase1_rows(fr):
    """[F][K] bool: the frames that are phase-1 messages (every '#' frame of these tests is a whole message)."""
    return (fr[:, :, 0] == ord("#")) & (fr[:, :, 1] == ord("1"))


# ------------------------------------------------------------------ 1. the plane equals the host parse

@pytest.fixture(scope="module")
def ragged(eng):
    """150 ragged phones: 0-130 phase-1 messages interleaved at random among 0-60 phase-2 and 0-90 phase-3 ones,
    Types 0 / 1 / 2 / '7', every kind of float the client prints, blank frames and frames without '#'; the
    compacted parse with and without the phase-1 plane, and the host's planes (shared, not modified)."""
    rng = np.random.default_rng(41)
    K = 150
    texts = []
    for k in range(K):
        n1, n2, n3 = int(rng.integers(0, 131)), int(rng.integers(0, 61)), int(rng.integers(0, 91))
        n = n1 + n2 + n3
        phases = rng.permutation(np.repeat([1, 2, 3], [n1, n2, n3]))
        vals = (rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-40, 38, (n, 3))).astype(np.float32)
        vals[rng.random(vals.shape) < 0.01] = np.nan
        vals[rng.random(vals.shape) < 0.01] = np.inf
        vals[rng.random(vals.shape) < 0.01] = -np.inf
        vals[rng.random(vals.shape) < 0.01] = np.float32(1.4e-45)
        t = 10 ** 12 + np.cumsum(rng.integers(0, 3_000_000, n))
        types = rng.integers(0, 3, n).astype(str).astype(object)
        types[rng.random(n) < 0.05] = "7"
        msgs = [wire.message(phases[i], types[i], vals[i], t[i]) for i in range(n)]
        if k % 5 == 0:
            msgs.insert(int(rng.integers(0, len(msgs) + 1)), " " * 99 + "\n")
        if k % 7 == 0:
            msgs.insert(int(rng.integers(0, len(msgs) + 1)), "x" * 99 + "\n")
        texts.append("".join(msgs))
    fr = wire.frames(texts)
    F = fr.shape[0]
    return dict(K=K, F=F, texts=texts, fr=fr, without=eng.wire_events(fr), with1=eng.wire_events(fr, phase1=True),
                host={ph: _host_planes(texts, ph, F) for ph in (1, 2, 3)})


def _same_other_planes(a, b, F, K):
    """Everything the parse gave before the phase-1 plane existed, bit for bit."""
    assert a["E2"] == b["E2"] and a["E3"] == b["E3"] and a["ev3_from"] == b["ev3_from"]
    assert np.array_equal(a["n2"], b["n2"]) and np.array_equal(a["n3"], b["n3"])
    assert np.array_equal(a["first_t2"].download((K,), np.int64), b["first_t2"].download((K,), np.int64))
    assert _same(_plane(a, "ev2", F, K), _plane(b, "ev2", F, K))
    assert _same(_plane(a, "ev3", F, K), _plane(b, "ev3", F, K))


def test_phase1_plane_equals_the_host_parse(ragged):
    """Compacted: ev1 is pack_events64 of wire.events_from_wire(..., phase=1) padded with the no-message event,
    n1 the host's counts, E1 the most of any phone; ev2 / ev3 / n2 / n3 / first_t2 / E2 / E3 of the same call
    equal those of the parse without the plane (and the host's)."""
    r = ragged
    K, F, w = r["K"], r["F"], r["with1"]
    assert _same(_plane(w, "ev1", F, K), r["host"][1])
    n1 = np.array([(wire.parse(tx)["phase"] == 1).sum() for tx in r["texts"]])
    assert np.array_equal(w["n1"], n1) and w["n1"].dtype == np.int32
    assert w["E1"] == n1.max() > 100
    types = _bits(_plane(w, "ev1", F, K)[..., 3]) & np.uint64(3)
    assert {0, 1, 2, 3} == set(np.unique(types[_bits(_plane(w, "ev1", F, K)[..., 3]) != NONE_W]).tolist())
    _same_other_planes(w, r["without"], F, K)
    assert _same(_plane(w, "ev2", F, K), r["host"][2]) and _same(_plane(w, "ev3", F, K), r["host"][3])


@pytest.mark.parametrize("chunks", [None, "3", "7"])
def test_phase1_frame_rows(eng, ragged, chunks, monkeypatch):
    """PEKF_WIRE_FRAME_ROWS: row f of ev1 is frame f's phase-1 message or the no-message event -- each column,
    compacted, is the compacted plane's, and the rows that hold a message are exactly the phase-1 frames';
    E1 = 1 + the last such row of any phone; the other planes, counts and bounds are those of the frame-row
    parse without the plane.  Also with the frames split into chunks parsed by separate waves."""
    if chunks:
        monkeypatch.setenv("PEKF_WIRE_CHUNKS", chunks)
    r = ragged
    K, F, fr = r["K"], r["F"], r["fr"]
    assert F > 7 * 8                                    # "7" splits into chunks of several frame indices
    a = eng.wire_events(fr, frame_rows=True)
    w = eng.wire_events(fr, frame_rows=True, phase1=True)
    _same_other_planes(w, a, F, K)
    assert np.array_equal(w["n1"], r["with1"]["n1"])
    rows1 = _plane(w, "ev1", F, K)
    is1 = _phase1_rows(fr)
    assert np.array_equal(_bits(rows1[..., 3]) != NONE_W, is1)
    assert w["E1"] == 1 + int(np.nonzero(is1.any(axis=1))[0].max())
    comp = _plane(r["with1"], "ev1", F, K)
    for k, got in enumerate(_compact(rows1, K)):
        assert got.shape[0] == w["n1"][k] and _same(got, comp[:w["n1"][k], k]), k
    none = rows1[~is1]
    assert np.all(_bits(none[:, :3]) == 0)             # the whole no-message event: {0, 0, 0, w}


# ------------------------------------------------------------------ 2. ring and batch edges

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("K,F", [(1, 1), (65, 1), (65, 2), (64, 3), (129, 5)])
def test_phase1_ring_edges(eng, K, F, rows):
    """The two-slot LDS ring at its ends -- one or two frame indices, a last block of one phone -- with phase-1
    frames only (some blank, some for the general parser): ev1 and n1 equal the host parse's, the other planes
    hold no message."""
    rng = np.random.default_rng(K * 10 + F)
    texts = []
    for k in range(K):
        frames = []
        for i in range(F):
            if rng.random() < 0.15:
                frames.append(" " * 99 + "\n")
                continue
            toks = [_fast_form(rng) for _ in range(3)]
            if k % 3 == 1 and i == F // 2:
                toks[1] = "+1.5e3"                      # not the fast form: the general parser takes it
            frames.append(_frame(toks, int(rng.integers(0, 10 ** 12)), ty=str(rng.choice(["0", "1", "2", "7"]))))
        texts.append("".join(frames))
    fr = wire.frames(texts)
    w = eng.wire_events(fr, frame_rows=rows, phase1=True)
    host = _host_planes(texts, 1, F)
    n1 = (_bits(host[..., 3]) != NONE_W).sum(axis=0)
    assert np.array_equal(w["n1"], n1) and not w["n2"].any() and not w["n3"].any()
    got = _plane(w, "ev1", F, K)
    if rows:
        is1 = _phase1_rows(fr)
        assert np.array_equal(_bits(got[..., 3]) != NONE_W, is1)
        assert w["E1"] == (1 + int(np.nonzero(is1.any(axis=1))[0].max()) if is1.any() else 0)
        for k, col in enumerate(_compact(got, K)):
            assert _same(col, host[:n1[k], k]), k
    else:
        assert _same(got, host) and w["E1"] == n1.max(initial=0)
    for name in ("ev2", "ev3"):
        p = _plane(w, name, F, K)
        assert np.all(_bits(p[..., 3]) == NONE_W) and np.all(_bits(p[..., :3]) == 0)
    assert w["E2"] == 0 and w["E3"] == 0


# ------------------------------------------------------------------ 3. the general parser and the time rule

def _raw_p1(eng, fr, rows):
    """pekf_wire_events_p1_dev past engine.wire_events' refusal of a bad frame: (ev1 [F][K][4], n1, n2, n3,
    bad_frame, error word)."""
    from poseestimationkf_amd._lib import check, lib
    F, K = fr.shape[:2]
    sizes = (fr.nbytes, 32 * F * K, 32 * F * K, 32 * F * K, 8 * K, 4 * K, 4 * K, 4 * K, 4 * K, 4, 12)
    fb, e1, e2, e3, t2, n1, n2, n3, bad, err, bounds = (eng.DeviceBuffer(n) for n in sizes)
    fb.upload(np.ascontiguousarray(fr))
    err.upload(np.zeros(1, np.int32))
    check(lib.pekf_wire_events_p1_dev(K, F, fb.ptr, F, F, F, e1.ptr, e2.ptr, e3.ptr, t2.ptr, n1.ptr, n2.ptr, n3.ptr,
                                      bad.ptr, err.ptr, bounds.ptr if rows else None, 1 if rows else 0, None))
    check(lib.pekf_device_sync())
    return (e1.download((F, K, 4), np.float64), n1.download((K,), np.int32), n2.download((K,), np.int32),
            n3.download((K,), np.int32), bad.download((K,), np.int32), int(err.download((1,), np.int32)[0]))


GOOD = ["1.0", "2.0", "3.0"]


@pytest.mark.parametrize("rows", [False, True])
def test_phase1_general_parser_and_the_time_rule(eng, rows):
    """A phase-1 frame in a form only the general parser takes lands in ev1 with the host's value; a phase-1
    frame with a time of 2^51 ns -- which std::stoll accepts, the server never reads and the event cannot
    hold -- is a message with its values and type and time 0, counted in n1, and the phone's later phase-2
    and phase-3 frames are parsed."""
    forms = ["+1.5e3", "9007199254740993", "1e23", "-0.0", "1e-80", "9e80", "00000001.5", "5", "1.5E+5"]
    phone0 = "".join(_frame([forms[i], forms[i + 1], forms[i + 2]], 100 + i, ty=i % 3) for i in range(0, 9, 3))
    def phone1(t_big, t_neg):
        return (_frame(GOOD, 5, phase=1, ty=0) + _frame(["-7.25", "0.5", "1.5E3"], t_big, phase=1, ty=1) +
                _frame(["4.0", "5.0", "6.0"], t_neg, phase=1, ty=7) + _frame(GOOD, 7, phase=2, ty=1) +
                _frame(GOOD, 8, phase=3, ty=2) + _frame(GOOD, T_2POW51 - 1, phase=1))
    texts = [phone0, phone1(T_2POW51, -T_2POW51 - 5)]   # (also past the limit below 0)
    as_stored = [phone0, phone1(0, 0)]                  # what the plane holds: the same messages at time 0
    fr = wire.frames(texts)
    F = fr.shape[0]
    w = eng.wire_events(fr, frame_rows=rows, phase1=True)
    ev1 = _compact(_plane(w, "ev1", F, 2), 2)
    host = _host_planes(as_stored, 1, F)
    assert w["n1"].tolist() == [3, 4] and w["n2"].tolist() == [0, 1] and w["n3"].tolist() == [0, 1]
    assert _same(ev1[0], host[:3, 0]) and _same(ev1[1], host[:4, 1])
    assert ev1[1][1, :3].tolist() == [-7.25, 0.5, 1500.0] and int(_bits(ev1[1][1, 3:])[0]) == 1   # time 0 | type 1
    assert ev1[1][2, :3].tolist() == [4.0, 5.0, 6.0] and int(_bits(ev1[1][2, 3:])[0]) == 3
    for ph, name in ((2, "ev2"), (3, "ev3")):           # the frames after them: the host's
        got = _compact(_plane(w, name, F, 2), 2)[1]
        assert _same(got, _host_planes(as_stored, ph, F)[:1, 1])


@pytest.mark.parametrize("rows", [False, True])
def test_phase1_refusals_stop_the_phone_as_before(eng, rows):
    """A form the device refuses ("0x1p3") in a phase-1 frame stops the phone at that frame, and so does a time
    of 2^51 ns in a phase-2 frame, with or without the phase-1 plane."""
    ok = _frame(GOOD, 7)
    texts = [ok * 4,
             ok + _frame(["0x1p3", "2.0", "3.0"], 8) + ok + _frame(GOOD, 9, phase=3),
             ok + ok + _frame(GOOD, T_2POW51, phase=2) + ok]
    fr = wire.frames(texts)
    with pytest.raises(ValueError, match="phone 1, frame 1"):
        eng.wire_events(fr, frame_rows=rows, phase1=True)
    for phase1 in (True, False):
        with pytest.raises(ValueError, match="phone 1, frame 2"):
            eng.wire_events(fr[:, [0, 2]].copy(), frame_rows=rows, phase1=phase1)   # (texts[2] as phone 1)
    ev1, n1, n2, n3, bad, err = _raw_p1(eng, fr, rows)
    assert bad.tolist() == [-1, 1, 2] and err & 1
    assert n1.tolist() == [4, 1, 2] and not n2.any() and not n3.any()
    w1 = _bits(ev1[..., 3]) != NONE_W
    assert w1[:, 0].all() and w1[:, 1].tolist() == [True, False, False, False]
    assert w1[:, 2].tolist() == [True, True, False, False]


# ------------------------------------------------------------------ 4. pinned by the reference's own parser

K_GOLD = 70


def _tiled_frames(z, phones):
    """[F][70][100] frames, column c from phone phones[c % len(phones)], shorter phones padded with blank frames."""
    F = max(len(z[p + "_frames"]) for p in phones)
    fr = np.full((F, K_GOLD, 100), ord(" "), np.uint8)
    for c in range(K_GOLD):
        a = z[phones[c % len(phones)] + "_frames"]
        fr[:len(a), c] = a
    return fr


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.mark.parametrize("rows", [False, True])
def test_phase1_plane_equals_the_reference_parser(eng, golden, rows):
    """Phone `phase1` of tests/golden/parser.npz (1,257 frames, 157 phase-1 messages, each traced into the
    reference's setValues) in 70 columns: every column's ev1 values, in order, are the reference's own bit for
    bit, n1 = 157; phones without a phase-1 message have n1 = 0."""
    z = golden
    want = z["phase1_values"][z["phase1_phase"] == ord("1")]
    assert want.shape == (157, 3) and len(z["phase1_frames"]) == 1257 and np.isfinite(want).all()
    fr = _tiled_frames(z, ["phase1"])
    F = fr.shape[0]
    w = eng.wire_events(fr, frame_rows=rows, phase1=True)
    assert (w["n1"] == 157).all()
    for c, col in enumerate(_compact(_plane(w, "ev1", F, K_GOLD), K_GOLD)):
        assert col.shape == (157, 4) and same_bits(col[:, :3], want), c
    fr0 = _tiled_frames(z, ["plain", "other"])
    w0 = eng.wire_events(fr0, frame_rows=rows, phase1=True)
    assert not w0["n1"].any() and w0["E1"] == 0
    assert np.all(_bits(_plane(w0, "ev1", fr0.shape[0], K_GOLD)[..., 3]) == NONE_W)


# ------------------------------------------------------------------ 5. the session against today's route

N_CAL = 100


@pytest.fixture(scope="module")
def session_texts():
    """64 phones with a soft- and hard-iron distortion in all three phases, as wire text (phase-3 parts of
    different lengths); phone 7 stops after 100 calibration messages."""
    Ks = 64
    ph1 = synth.generate_calibration_events(Ks, N_CAL + 1, seed=81)
    A, h = ph1["soft"], ph1["hard"]
    ph2 = synth.generate_events(np.arange(Ks), 700, seed=82)
    ph3 = synth.generate_events(np.arange(Ks), 300, seed=83)
    t1 = ph1["times"][-1]
    ph2 = dict(ph2, times=ph2["times"] - ph2["t_init"][None, :] + t1[None, :], t_init=t1)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    for ph in (ph2, ph3):   # what the distorted magnetometer reports
        m = np.einsum("kij,ekj->eki", A, ph["values"].astype(np.float64)) + h[None]
        ph["values"] = np.where((ph["types"] == synth.EV_MAG)[..., None], m.astype(np.float32), ph["values"])
    texts = []
    for k in range(Ks):
        n1 = N_CAL if k == 7 else N_CAL + 1
        n3 = 300 - 7 * (k % 4)
        texts.append(wire.events_text(ph1["types"][:n1, k], ph1["values"][:n1, k], ph1["times"][:n1, k], phase=1) +
                     wire.events_text(ph2["types"][:, k], ph2["values"][:, k], ph2["times"][:, k], phase=2) +
                     wire.events_text(ph3["types"][:n3, k], ph3["values"][:n3, k], ph3["times"][:n3, k], phase=3))
    return texts


def _host_route(eng, texts, n_cal):
    """Today's route to a calibration from wire text: the host parse of phase 1, then the device's fit."""
    K = len(texts)
    e1 = wire.events_from_wire(texts, np.zeros((K, 3)), np.zeros((K, 3)), np.zeros(K, np.int64), phase=1)
    return eng.calibrate_magnetometer(e1, n_cal=n_cal, events="f64")


def _sessions_are_identical(eng, fr, cal_w, frame_rows, **kw):
    """run_wire_session(calibration="frames") against run_wire_session(calibration=cal_w): the same k_magcal
    reads the same messages in the same order (skipped rows add nothing), so every result is bit-equal."""
    K = fr.shape[1]
    f_dev, f_host = eng.BatchedEKF(K), eng.BatchedEKF(K)
    got = eng.run_wire_session(fr, f_dev, frame_rows=frame_rows, calibration="frames", **kw)
    kw.pop("n_cal", None)
    want = eng.run_wire_session(fr, f_host, frame_rows=frame_rows, calibration=cal_w, **kw)
    assert sorted(got) == ["calibrated", "calibration", "counts", "ready", "refs"]
    for key in ("ready", "counts", "refs", "calibrated"):
        assert np.array_equal(_bits(got[key].astype(np.float64)), _bits(want[key].astype(np.float64))), key
    for key in ("bias", "W", "fit", "status"):
        assert np.array_equal(_bits(got["calibration"][key].astype(np.float64)),
                              _bits(cal_w[key].astype(np.float64))), key
    assert np.array_equal(got["calibration"]["calibrated"], cal_w["calibrated"])
    for a, b in zip(f_dev.get_state(), f_host.get_state()):
        assert np.array_equal(_bits(a), _bits(b))
    return got, f_dev


@pytest.fixture(scope="module")
def session_cal(eng, session_texts):
    return _host_route(eng, session_texts, N_CAL)


@pytest.mark.parametrize("frame_rows", [True, False])
def test_session_calibrated_from_its_frames_equals_the_host_route(eng, session_texts, session_cal, frame_rows):
    """The 64 phones' frames through run_wire_session(calibration="frames") and through today's route (host parse
    of phase 1 -> calibrate_magnetometer -> run_wire_session(calibration=dict)): X, P, ready, counts, refs,
    calibrated and the calibration's bias / W / fit / status identical; phone 7, with 100 messages, is the one
    left uncalibrated."""
    fr = wire.frames(session_texts)
    got, _ = _sessions_are_identical(eng, fr, session_cal, frame_rows)
    assert got["calibration"]["status"].tolist() == [1 if k == 7 else 0 for k in range(64)]
    assert got["ready"].all() and got["counts"].min() > 0
    assert np.isfinite(got["calibration"]["fit"][got["calibrated"]]).all()


# ------------------------------------------------------------------ 6. interleaved, small

@pytest.mark.parametrize("frame_rows", [True, False])
def test_interleaved_phase1_messages_calibrate_the_whole_session(eng, frame_rows):
    """70 phones, n_cal = 20: 30 phase-1 messages spread through 120 phase-2 and 40 phase-3 ones.  The fit uses
    each phone's first 20 wherever they sit, and the whole of phases 2 and 3 is corrected: identical to the host
    route.  The phone without a phase-1 frame has status 1 and ends where the session without a calibration
    does, bit for bit."""
    K, n_cal, n_avg, lone = 70, 20, 10, 0
    rng = np.random.default_rng(51)
    ph1 = synth.generate_calibration_events(K, 30, seed=84)
    ph2 = synth.generate_events(np.arange(K), 120, seed=85)
    ph3 = synth.generate_events(np.arange(K), 40, seed=86)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    texts = []
    for k in range(K):
        msgs = [wire.message(2, ph2["types"][i, k], ph2["values"][i, k], ph2["times"][i, k]) for i in range(120)] + \
               [wire.message(3, ph3["types"][i, k], ph3["values"][i, k], ph3["times"][i, k]) for i in range(40)]
        if k != lone:
            at = np.sort(rng.integers(0, len(msgs) + 1, 30))
            for j in range(29, -1, -1):                 # from the back: phase 1's own order is kept
                msgs.insert(int(at[j]), wire.message(1, ph1["types"][j, k], ph1["values"][j, k], ph1["times"][j, k]))
        texts.append("".join(msgs))
    fr = wire.frames(texts)
    cal_w = _host_route(eng, texts, n_cal)
    got, f_dev = _sessions_are_identical(eng, fr, cal_w, frame_rows, n_cal=n_cal, n_avg=n_avg)
    status = got["calibration"]["status"]
    assert status[lone] == 1 and (np.delete(status, lone) == 0).all()
    ran = got["counts"] > 0                              # (40 phase-3 messages: a handful of records, or none)
    assert got["ready"].all() and ran.sum() > K // 2 and ran[lone]
    f_none = eng.BatchedEKF(K)
    eng.run_wire_session(fr, f_none, frame_rows=frame_rows, n_avg=n_avg)
    for a, b in zip(f_dev.get_state(), f_none.get_state()):
        assert np.array_equal(_bits(a[lone]), _bits(b[lone]))
    X, X0 = f_dev.get_state()[0], f_none.get_state()[0]
    ran[lone] = False
    assert (np.abs(X - X0).max(axis=1)[ran] > 0).all()  # the correction reached every other phone that applied a record
