"""The device wire parse, the phase-2 and phase-3 kernels and the whole wire session against the
REFERENCE's own C++ Parser, through tests/golden/parser.npz (see tests/test_parser_golden.py, which holds
the restatement and the host parse to the same fixture on the CPU).  Only the committed fixture is read.

The fixture's phones are tiled to K = 70 columns -- a second wave, and a partial 8-lane group at its end --
and every column must give what its source phone gave the reference."""
import numpy as np
import pytest

from oracle import frontend_numpy as fe
from poseestimationkf_amd import synth

from .test_live import ATOL_F32_ROUNDING, ATOL_F64_CHAIN
from .test_parser_golden import (NOHASH, OBS_TIME, OBS_TYPE, OBS_VALUES, OK, PHASE3, SESSIONS, SHORT, THREW,
                                 load_golden, phase_events, same_bits, trace_records)

pytestmark = pytest.mark.gpu

K = 70
NONE_W = np.uint64(synth.EV64_NONE_W)


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def events(golden):
    """{phone: {2: (types, values, times), 3: ...}}: each phone's messages as the reference parsed them."""
    return {p: {ph: phase_events(golden, p, ph) for ph in (2, 3)} for p in SESSIONS}


def _tiled_frames(z, phones):
    """[F][K][100] frames, column c from phone phones[c % len(phones)], shorter phones padded with blank
    frames (no message)."""
    F = max(len(z[p + "_frames"]) for p in phones)
    fr = np.full((F, K, 100), ord(" "), np.uint8)
    for c in range(K):
        a = z[phones[c % len(phones)] + "_frames"]
        fr[:len(a), c] = a
    return fr


def _wire_raw(eng, fr, rows):
    """pekf_wire_events_ext_dev past engine.wire_events' refusal of a bad frame: (ev2, ev3 [F][K][4] as
    uint64 bits, n2, n3, bad_frame, first_t2)."""
    from poseestimationkf_amd._lib import check, lib
    F, Kc = fr.shape[:2]
    bufs = [eng.DeviceBuffer(n) for n in (fr.nbytes, 32 * F * Kc, 32 * F * Kc, 8 * Kc, 4 * Kc, 4 * Kc, 4 * Kc, 4, 8)]
    bufs[0].upload(np.ascontiguousarray(fr))
    bufs[7].upload(np.zeros(1, np.int32))
    check(lib.pekf_wire_events_ext_dev(Kc, F, bufs[0].ptr, F, F, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr,
                                       bufs[5].ptr, bufs[6].ptr, bufs[7].ptr, bufs[8].ptr if rows else None,
                                       1 if rows else 0, None))
    check(lib.pekf_device_sync())
    ev2 = bufs[1].download((F, Kc, 4), np.float64).view(np.uint64)
    ev3 = bufs[2].download((F, Kc, 4), np.float64).view(np.uint64)
    return (ev2, ev3, bufs[4].download((Kc,), np.int32), bufs[5].download((Kc,), np.int32),
            bufs[6].download((Kc,), np.int32), bufs[3].download((Kc,), np.int64))


def _event_bits(ty, va, ti):
    """(n, 4) uint64: the FP64 events {x, y, z, bits(t) | type} of parsed messages (include/pekf.h)."""
    out = np.empty((len(ty), 4), np.uint64)
    out[:, :3] = np.asarray(va, np.float64).reshape(-1, 3).view(np.uint64)
    out[:, 3] = np.asarray(ti, np.int64).astype(np.float64).view(np.uint64) | np.asarray(ty, np.uint64)
    return out


def _none_rows(n):
    out = np.zeros((n, 4), np.uint64)
    out[:, 3] = NONE_W
    return out


@pytest.mark.parametrize("rows", [False, True])
def test_device_parse_of_the_sessions_equals_the_reference_parser(eng, golden, events, rows):
    """eng.wire_events' kernel on the session phones' frames, compact and frame-row planes: every message's
    type bits, values and time bit-equal to the reference's parse, n2 / n3 its counts, phase-1 frames and
    padding no messages, and no frame refused."""
    z = golden
    fr = _tiled_frames(z, SESSIONS)
    F = fr.shape[0]
    ev2, ev3, n2, n3, bad, t2 = _wire_raw(eng, fr, rows)
    w = eng.wire_events(fr, frame_rows=rows)   # the engine's entry agrees with the raw call
    assert np.array_equal(w["n2"], n2) and np.array_equal(w["n3"], n3)
    assert (bad == -1).all()
    for c in range(K):
        p = SESSIONS[c % len(SESSIONS)]
        e2, e3 = _event_bits(*events[p][2]), _event_bits(*events[p][3])
        assert n2[c] == len(e2) and n3[c] == len(e3), (c, p)
        assert t2[c] == (events[p][2][2][0] if len(e2) else 0)
        if rows:  # row f: frame f's message in its phase's plane, the no-message event in the other
            ph = np.zeros(F, np.uint8)
            ph[:len(z[p + "_phase"])] = z[p + "_phase"]
            x2, x3 = _none_rows(F), _none_rows(F)
            x2[ph == ord("2")] = e2
            x3[ph == ord("3")] = e3
        else:     # the messages in order, then no-message events
            x2, x3 = np.concatenate([e2, _none_rows(F - len(e2))]), np.concatenate([e3, _none_rows(F - len(e3))])
        assert np.array_equal(ev2[:, c], x2), (c, p)
        assert np.array_equal(ev3[:, c], x3), (c, p)


@pytest.mark.parametrize("rows", [False, True])
def test_device_parse_of_every_form_follows_the_reference_parser(eng, golden, rows):
    """One form per phone (frame 0), then a plain client message (frame 1), so that what a form does to its
    phone shows.  A frame the server skips -- no '#', 30 characters or fewer, also where a NUL cut it -- is no
    message and stops nothing; one its std::stod / std::stoll throws on is refused (bad_frame); one in the
    client's own form (also NUL-cut) that the server processes gives the server's values, time and type bit
    for bit; any other form is either refused or equals the server's parse bit for bit, never anything
    else.  Phase-3 messages count in n3, other phases in nothing."""
    z = golden
    names = list(z["forms_names"])
    N = len(names)
    assert N > 64                                  # a second wave, as K = 70 gives the sessions
    plain = z["forms_frames"][names.index("last_plain")]
    fr = np.stack([z["forms_frames"], np.tile(plain, (N, 1))])
    ev2, ev3, n2, n3, bad, _ = _wire_raw(eng, fr, rows)
    tail = _event_bits([1], [[1.0, 2.0, 3.0]], [z["forms_time"][names.index("last_plain")]])[0]
    assert (n2 == 0).all() and (ev2[..., 3] == NONE_W).all()
    refused = []
    for c, name in enumerate(names):
        out, obs, own = int(z["forms_outcome"][c]), int(z["forms_obs"][c]), bool(z["forms_client"][c])
        phase3 = out == OK and z["forms_phase"][c] == ord("3")
        if out == THREW or (bad[c] == 0 and out == OK and not own):
            assert bad[c] == 0 and n3[c] == 0, name
            assert (ev3[:, c, 3] == NONE_W).all(), name
            refused.append(name)
            continue
        assert bad[c] == -1, name
        assert n3[c] == 1 + phase3, name
        first = ev3[0, c]
        if not phase3:                              # skipped by the server, or of no phase the device takes
            assert out in (NOHASH, SHORT) or chr(z["forms_phase"][c]) not in "23", name
            first, second = (ev3[1, c], ev3[0, c]) if rows else (ev3[0, c], ev3[1, c])
            assert np.array_equal(first, tail) and second[3] == NONE_W, name
            continue
        assert np.array_equal(ev3[1, c], tail), name
        want_type = int(z["forms_type"][c]) - ord("0") if obs & OBS_TYPE else synth.EV_OTHER
        assert int(first[3] & np.uint64(3)) == want_type, name
        if obs & OBS_VALUES:
            assert same_bits(first[:3].view(np.float64), z["forms_values"][c]), name
        if obs & OBS_TIME:
            assert (first[3:4] & ~np.uint64(3)).view(np.float64)[0] == float(z["forms_time"][c]), name
    # Exactly these are refused -- no other form may start to be, none of them may start to be taken:
    print("refused forms:", " ".join(refused))
    assert sorted(refused) == sorted(REFUSED_FORMS)


# The forms pekf_wire_events_dev leaves to the host parse (include/pekf.h: it takes the decimals the client
# prints and their plain variants -- a sign, no fraction, an exponent -- and "NaN" / "[-]Infinity"):
REFUSED_FORMS = (
    # what the server's std::stod / std::stoll throw on
    "x_huge", "x_subnormal", "x_min_subnormal", "x_underflow", "x_empty", "x_dot", "missing_comma", "missing_t",
    "t_blanks_only", "t_above_int64", "no_colon", "nul_32",
    # numbers strtod reads in forms no client prints: blanks before, hex, text after, more than 19 digits,
    # other spellings of inf / nan, an exponent without digits
    "x_blanks", "x_tab", "x_hex", "x_trailing", "x_digits20", "x_digits25", "x_frac25", "x_inf_word",
    "x_nan_lower", "x_minus_nan", "x_lone_e", "y_hex", "z_blanks", "z_trailing",
    # times std::stoll reads in forms no client prints (blanks, '+', not right after the third value), and
    # times of 2^51 ns or more, which an FP64 event cannot hold
    "t_blanks_digits", "t_plus", "t_later", "t_int64_max", "t_2pow51",
)


def _event_dict(streams, init_acc, init_mag, t_init):
    """Per-column (types, values, times) -> the engine's event dict, shorter streams padded with no-message
    events."""
    E = max(len(s[0]) for s in streams)
    Kc = len(streams)
    types = np.full((E, Kc), synth.EV_NONE, np.uint32)
    vals = np.zeros((E, Kc, 3))
    times = np.zeros((E, Kc), np.int64)
    for c, (ty, va, ti) in enumerate(streams):
        n = len(ty)
        types[:n, c], vals[:n, c], times[:n, c] = ty, va, ti
        times[n:, c] = ti[-1] if n else t_init[c]
    return dict(types=types, values64=vals, values=vals.astype(np.float32), times=times,
                init_acc=np.asarray(init_acc, np.float64), init_mag=np.asarray(init_mag, np.float64),
                t_init=np.asarray(t_init, np.int64))


def test_phase2_kernel_equals_the_reference_parser(eng, golden, events):
    """eng.frontend_init on FP64 events of the messages the reference parsed: ready, t_init, the means and
    the variances bit for bit against what its InitialValues / Parser ended phase 2 with (the phone that
    never got ready: not ready, NaN means)."""
    z = golden
    phones = [SESSIONS[c % len(SESSIONS)] for c in range(K)]
    streams = [events[p][2] for p in phones]
    ev = _event_dict(streams, np.zeros((K, 3)), np.zeros((K, 3)), [s[2][0] for s in streams])
    got = eng.frontend_init(ev, events="f64")
    for c, p in enumerate(phones):
        assert got["ready"][c] == bool(z[p + "_ready"][0]), (c, p)
        if not got["ready"][c]:
            assert p == "short" and np.isnan(got["init"][c]).all()
            continue
        assert got["t_init"][c] == z[p + "_t_init"][0], (c, p)
        assert same_bits(got["init"][c], np.concatenate([z[p + "_avg"][0], z[p + "_avg"][1]])), (c, p)
        assert same_bits(got["gyro_mean"][c], z[p + "_avg"][2]), (c, p)
        for row, name in enumerate(("acc", "mag", "gyro")):
            assert same_bits(got["var_" + name][c], z[p + "_var"][row]), (c, p, name)


def test_phase3_kernel_equals_the_reference_parser(eng, golden, events):
    """eng.run_frontend on FP64 events of the messages the reference parsed, from the averages and time its
    phase 2 ended with: the record count, gyro and dt exactly; acc / mag against fe.lpf of the normalised
    interpolated vectors the reference handed its filter, within 1e-15 (the kernel's rsqrt / reciprocal with
    a Newton step against IEEE division, as test_frontend_fp64_events_records_vs_oracle).  Where a zero
    time gap makes the reference's vector NaN (and its low-pass from there on), the kernel's is NaN too,
    and the finite values are compared (test_frontend_zero_time_gaps_follow_ieee_like_the_cpp).

    Measured: worst distance 4.44e-16 over the finite values, 270 NaN values agreeing (7 phones x 10 columns)."""
    z = golden
    phones = [PHASE3[c % len(PHASE3)] for c in range(K)]
    ev = _event_dict([events[p][3] for p in phones], [z[p + "_avg"][0] for p in phones],
                     [z[p + "_avg"][1] for p in phones], [z[p + "_t_init"][0] for p in phones])
    win, counts = eng.run_frontend(ev, events="f64")
    g, dt, a, m, refs = win.download_filters(np.arange(K))
    worst = 0.0
    n_nan = 0
    for c, p in enumerate(phones):
        rg, rdt, ra, rm = trace_records(z, p)
        r = len(rdt)
        assert counts[c] == r, (c, p)
        if not r:
            continue
        assert same_bits(g[:r, c], rg) and np.array_equal(dt[:r, c], rdt.astype(np.float64)), (c, p)
        for got, want in ((a[:r, c], fe.lpf(ra)), (m[:r, c], fe.lpf(rm))):
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (c, p)
            n_nan += int(nan.sum())
            worst = max(worst, float(np.abs(got[~nan] - want[~nan]).max()))
        ctor = z[p + "_ctor"]   # the reference's filter got the normalised means: mag0, acc0
        assert np.abs(refs[c] - np.concatenate([ctor[3:], ctor[:3]])).max() < 1e-15, (c, p)
    print("FP64-event records vs the reference parser's: worst |d| = %.2e (%d NaN values agree)" % (worst, n_nan))
    assert n_nan > 0 and worst < 1e-15


@pytest.mark.parametrize("rows", [True, False])
def test_wire_session_end_to_end_against_the_reference_parser(eng, oracle_c, golden, rows):
    """eng.run_wire_session on the session phones' frames: ready and the record counts as the reference's,
    and the final X against the C oracle run over the records assembled from the reference's trace (gyro,
    dt from the gyro times, fe.lpf of the vectors it handed its filter; references: the constructor's).
    oracle_c.run itself takes the f32 stream records, so its own loop is run on the float64 records
    (oracle_c.run_records64) for ATOL_F64_CHAIN, and oracle_c.run on the rounded ones for ATOL_F32_ROUNDING.

    Measured: FP64 chain 5.413e-14, f32-record oracle_c.run 1.877e-08 (both plane layouts)."""
    z = golden
    phones = [p for p in SESSIONS if p != "tedge"]   # (its zero time gaps leave the filter NaN)
    fr = _tiled_frames(z, phones)
    filt = eng.BatchedEKF(K)
    out = eng.run_wire_session(fr, filt, frame_rows=rows)
    X, _ = filt.get_state()
    want = {}
    for p in phones:
        g, dt, ra, rm = trace_records(z, p)
        if not len(dt):
            want[p] = (np.array([1.0, 0, 0, 0]),) * 2
            continue
        a, m = fe.lpf(ra), fe.lpf(rm)
        acc0, mag0 = z[p + "_ctor"][3:], z[p + "_ctor"][:3]
        rec = synth.Records(g[:, None].astype(np.float32), a[:, None].astype(np.float32),
                            m[:, None].astype(np.float32), dt[:, None].astype(np.uint32), acc0[None], mag0[None])
        want[p] = (oracle_c.run_records64(g, dt.astype(np.float64), a, m, acc0, mag0)[0], oracle_c.run(rec)[0][0])
    worst64 = worst32 = 0.0
    for c in range(K):
        p = phones[c % len(phones)]
        assert out["ready"][c] == bool(z[p + "_ready"][0]), (c, p)
        assert out["counts"][c] == len(z[p + "_rec_time"]), (c, p)
        worst64 = max(worst64, float(np.abs(X[c] - want[p][0]).max()))
        worst32 = max(worst32, float(np.abs(X[c] - want[p][1]).max()))
    print("wire session vs the C oracle over the reference parser's records: FP64 chain %.3e, "
          "f32-record oracle_c.run %.3e" % (worst64, worst32))
    assert worst64 < ATOL_F64_CHAIN
    assert worst32 < ATOL_F32_ROUNDING
