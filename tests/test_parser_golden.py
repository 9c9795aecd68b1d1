"""The front-end restatement and the host wire parse against the REFERENCE's own C++ Parser.

tests/golden/parser.npz (made by tests/golden/make_parser_golden.py) holds wire frames and what the
reference server's Parser.cpp / InitialValues.cpp -- compiled unchanged behind stand-in headers,
oracle/ref_parser/ -- made of them: per frame whether Parser::run / ProcessString took it and what its
state shows of the parse, every call it made on the filter (the constructor, SetAngularVelocity,
SetAccelerometerMeasurements, SetMagnetometerMeasurements, UpdateLatestPreviousTime), and the phase-2
averages and variances at the end.  oracle/frontend_numpy.py is the checker of every GPU test of phase 2
and phase 3, and wire.parse that of the device parser: here both are held to the binary, bit for bit.

The phones: sessions (plain; exact: phase 2 stops at the message that builds the filter; short: never
ready; phase1: calibration messages interleaved; other: messages of a Type no sensor takes), phase 3's
time edges (tedge) and state-machine orders (orders, acconly), and number / message forms (forms).
These tests read only the committed fixture; the last ones regenerate it where the reference is present.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from oracle import frontend_numpy as fe
from poseestimationkf_amd import synth

from .conftest import GOLDEN, ROOT

NOHASH, SHORT, THREW, OK = 0, 1, 2, 3          # P_outcome
OBS_VALUES, OBS_TIME, OBS_TYPE = 1, 2, 4       # P_obs
SESSIONS = ("plain", "exact", "short", "phase1", "other", "tedge", "orders", "acconly")
PHASE3 = tuple(p for p in SESSIONS if p != "short")   # the phones whose filter is built


def load_golden():
    with np.load(os.path.join(GOLDEN, "parser.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def same_bits(a, b):
    """Float arrays equal bit for bit, any NaN equal to any NaN (the trace prints NaNs without payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def client_fields(frame):
    """A frame in the client's form "#p,T:x,y,z,t:ns" read with Python's own float() / int() (correctly
    rounded, as strtod is): (phase, type, [x, y, z], t).  Independent of the code under test; used where
    the parser's state does not show a field (most of phase 2), and checked against it where it does."""
    s = bytes(frame).decode("latin-1")
    assert s[0] == "#" and s[2] == "," and s[4] == ":", s
    x, y, z, t = s[5:].split(",")
    assert t.startswith("t:")
    return int(s[1]), int(s[3]), [float(x), float(y), float(z)], int(t[2:])


def phase_events(z, p, phase):
    """Phone p's messages of one phase, in order, as (types, values (n, 3), times): what the trace shows,
    and client_fields for what it does not (the two compared wherever the trace shows a field).  A Type
    no sensor takes is synth.EV_OTHER."""
    ty, va, ti = [], [], []
    for f in np.nonzero((z[p + "_outcome"] == OK) & (z[p + "_phase"] == ord("0") + phase))[0]:
        _, t_py, v_py, time_py = client_fields(z[p + "_frames"][f])
        obs = int(z[p + "_obs"][f])
        if obs & OBS_TYPE:
            assert int(z[p + "_type"][f]) == ord("0") + t_py, (p, f)
        if obs & OBS_VALUES:
            assert same_bits(z[p + "_values"][f], v_py), (p, f)
        if obs & OBS_TIME:
            assert int(z[p + "_time"][f]) == time_py, (p, f)
        if phase == 3:  # every sensor message shows in the parser's state
            assert (obs == (OBS_VALUES | OBS_TIME | OBS_TYPE)) == (t_py <= 2), (p, f)
        ty.append(t_py if t_py <= 2 else synth.EV_OTHER)
        va.append(v_py)
        ti.append(time_py)
    return np.array(ty, np.uint32), np.array(va, np.float64).reshape(-1, 3), np.array(ti, np.int64)


def trace_records(z, p):
    """Phone p's records as the reference hands them to its filter: gyro (R, 3), dt (R,) int64 from the gyro
    times and t_init (KalmanFilter.cpp:306-308), and the normalised interpolated acc / mag (R, 3) before
    the filter's low-pass."""
    t = z[p + "_rec_time"]
    dt = np.diff(np.concatenate([z[p + "_t_init"], t]))
    return z[p + "_rec_gyro"], dt, z[p + "_rec_acc"], z[p + "_rec_mag"]


# ------------------------------------------------------------------ the fixture itself

def test_fixture_holds_the_cases_it_is_for(golden):
    z = golden
    assert list(z["phones"]) == list(SESSIONS) + ["forms"]
    assert os.path.getsize(os.path.join(GOLDEN, "parser.npz")) < 400_000
    for p in SESSIONS:
        assert (z[p + "_outcome"] == OK).all() and z[p + "_client"].all()
    assert not z["short_ready"][0] and len(z["short_frames"]) == 520 and not z["short_initialized"].all()
    for p in PHASE3:
        assert z[p + "_ready"][0] and z[p + "_initialized"].all()
    assert z["exact_t_init"][0] == z["exact_t_ctor"][0] and z["plain_t_init"][0] > z["plain_t_ctor"][0]
    assert (z["phase1_phase"] == ord("1")).sum() > 100 and (z["phase1_obs"][z["phase1_phase"] == ord("1")] == 1).all()
    for p in ("plain", "exact", "phase1", "other"):
        assert len(z[p + "_rec_time"]) >= 25
    assert len(z["acconly_rec_time"]) == 0 and (z["acconly_phase"] == ord("3")).sum() == 30
    # time edges: a negative dt, pauses of seconds, and the NaN the zero gaps make of acc / mag
    _, dt, a, m = trace_records(z, "tedge")
    assert dt.min() < 0 and dt.max() > 3_000_000_000
    assert np.isnan(a).any() and np.isnan(m).any() and np.isfinite(a[:10]).all() and np.isfinite(m[:10]).all()
    assert np.abs(z["tedge_time"]).max() < 2 ** 51
    # forms: every outcome occurs
    assert sorted(set(z["forms_outcome"].tolist())) == [NOHASH, SHORT, THREW, OK]
    names = list(z["forms_names"])
    out = dict(zip(names, z["forms_outcome"]))
    assert out["chars_30"] == SHORT and out["chars_31"] == OK and out["nul_10"] == SHORT and out["nul_31"] == SHORT
    assert out["nul_2"] == SHORT and out["nul_phase"] == SHORT and out["nul_type"] == SHORT
    assert out["nul_60"] == OK and out["x_huge"] == THREW and out["x_subnormal"] == THREW and out["no_hash"] == NOHASH


# ------------------------------------------------------------------ phase 3: the restatement's state machine

@pytest.mark.parametrize("p", PHASE3)
def test_restatement_phase3_equals_the_reference_parser(golden, p):
    """fe.records / fe.run_frontend on the messages the binary parsed, from the averages and time its
    phase 2 ended with: the record count, gyro, dt and the normalised interpolated acc / mag before the
    low-pass, bit for bit (NaN where the reference's division by a zero time gap gives NaN); and
    run_frontend's acc / mag are fe.lpf of those."""
    z = golden
    ty, va, ti = phase_events(z, p, 3)
    t_init = int(z[p + "_t_init"][0])
    init_acc, init_mag = z[p + "_avg"][0], z[p + "_avg"][1]
    rg, rdt, ra, rm = trace_records(z, p)
    units = list(fe.records(ty, va, ti, init_acc, init_mag, t_init))
    assert len(units) == len(rdt)
    g, dt, a, m = fe.run_frontend(ty, va, ti, init_acc, init_mag, t_init)
    assert len(dt) == len(rdt)
    if len(rdt):
        assert same_bits([u[0] for u in units], rg) and same_bits(g, rg)
        assert [u[1] for u in units] == z[p + "_rec_time"].tolist()
        assert np.array_equal(dt, rdt)
        assert same_bits([u[2] for u in units], ra)
        assert same_bits([u[3] for u in units], rm)
        assert same_bits(fe.lpf(ra), a) and same_bits(fe.lpf(rm), m)


# ------------------------------------------------------------------ phase 2: the restatement's initial values

@pytest.mark.parametrize("p", SESSIONS)
def test_restatement_phase2_equals_the_reference_parser(golden, p):
    """fe.initial_values on the phone's phase-2 messages: ready, t_init (the last UpdateLatestPreviousTime,
    or the constructor's time), the raw means and the variances, bit for bit; the constructor got the
    normalised means."""
    z = golden
    ty, va, ti = phase_events(z, p, 2)
    o = fe.initial_values(ty, va, ti)
    assert o["ready"] == bool(z[p + "_ready"][0])
    if not o["ready"]:
        assert p == "short" and o["t_init"] is None
        return
    assert o["t_init"] == int(z[p + "_t_init"][0])
    for row, name in enumerate(("acc", "mag", "gyro")):
        assert same_bits(o[name], z[p + "_avg"][row]), name
        assert same_bits(o["var_" + name], z[p + "_var"][row]), name
    assert same_bits(fe._normalise(o["mag"]) + fe._normalise(o["acc"]), z[p + "_ctor"])


# ------------------------------------------------------------------ the host wire parse

def _host_parse(frame_bytes):
    from poseestimationkf_amd import wire
    from poseestimationkf_amd._lib import PekfError
    try:
        return wire.parse(frame_bytes)
    except PekfError:
        return None


def _check_message(z, p, f, got, i):
    """Message i of a host parse against frame f of phone p's trace, where the trace shows the field."""
    assert int(got["phase"][i]) == (int(z[p + "_phase"][f]) - ord("0")) % 256, (p, f)
    obs = int(z[p + "_obs"][f])
    if obs & OBS_TYPE:
        assert int(got["types"][i]) == int(z[p + "_type"][f]) - ord("0"), (p, f)
    if obs & OBS_VALUES:
        assert same_bits(got["values"][i], z[p + "_values"][f]), (p, f)
    if obs & OBS_TIME:
        assert int(got["times"][i]) == int(z[p + "_time"][f]), (p, f)


@pytest.mark.parametrize("p", SESSIONS)
def test_host_parse_of_a_session_equals_the_reference_parser(golden, p):
    """wire.parse (pekf_wire_parse) on a phone's whole stream: one message per frame the binary processed,
    its phase, and the type, the three values' bits and the time wherever the binary's state shows them."""
    z = golden
    got = _host_parse(z[p + "_frames"].tobytes())
    taken = np.nonzero(z[p + "_outcome"] == OK)[0]
    assert got is not None and len(got["types"]) == len(taken)
    n_values = 0
    for i, f in enumerate(taken):
        _check_message(z, p, f, got, i)
        n_values += bool(z[p + "_obs"][f] & OBS_VALUES)
    assert n_values >= 250  # phase 2 alone shows up to 99 samples of each sensor


def test_host_parse_of_every_form_equals_the_reference_parser(golden):
    """Frame by frame over the number and message forms: taken / skipped / error as the binary's processed /
    (no '#' or 30 characters or fewer, a NUL ending the message) / threw, and the parsed fields where
    shown.  The host parse is line-oriented, so the one frame with a newline inside (a '\\n' Type,
    type_newline) is outside what it can express: it reads two short lines and skips both, where the server
    processes one message that no sensor takes; the device parser, which takes frames (wire.frames), is
    held to it in the GPU tests."""
    z = golden
    seen = 0
    for f, name in enumerate(z["forms_names"]):
        got = _host_parse(z["forms_frames"][f].tobytes())
        out = int(z["forms_outcome"][f])
        if name == "type_newline":
            assert out == OK and z["forms_obs"][f] == 0 and got is not None and len(got["types"]) == 0
            continue
        if out == THREW:
            assert got is None, name
        elif out in (NOHASH, SHORT):
            assert got is not None and len(got["types"]) == 0, name
        else:
            assert got is not None and len(got["types"]) == 1, name
            _check_message(z, "forms", f, got, 0)
            seen += int(z["forms_obs"][f]) == 7
    assert seen >= 35


def test_server_values_equal_the_reference_parse_of_the_clients_text(golden):
    """wire.server_values(f32) against the binary's std::stod of wire.message's text, over Float.toString's
    shapes (1.0E7, 9.999E-4, 1.4E-45, 3.4028235E38, -0.0, NaN, Infinity, -Infinity, ...)."""
    from poseestimationkf_amd import wire
    z = golden
    fr = z["forms_f32_frame"]
    assert (z["forms_outcome"][fr] == OK).all() and (z["forms_obs"][fr] == 7).all()
    texts = [z["forms_frames"][f].tobytes().decode() for f in fr]
    assert any("E-45" in t for t in texts) and any("E38" in t for t in texts) and any("-Infinity" in t for t in texts)
    assert [wire.message(3, 1, v, t) for v, t in zip(z["forms_f32"], z["forms_time"][fr])] == texts
    assert same_bits(wire.server_values(z["forms_f32"]), z["forms_values"][fr])


# ------------------------------------------------------------------ run_wire_session's batch check

@pytest.mark.parametrize("batch", [3, 5])
def test_run_wire_session_refuses_a_batch_that_is_not_the_frames(batch):
    """The event planes are laid out for the frames' phone count: filters of any other batch would read
    past them or mix phones, so it is refused before anything is allocated or launched (the filters here
    are no device object at all)."""
    from poseestimationkf_amd import engine
    frames = np.full((2, 4, 100), ord(" "), np.uint8)
    with pytest.raises(ValueError, match="4 phones"):
        engine.run_wire_session(frames, types.SimpleNamespace(batch=batch))
    with pytest.raises(ValueError, match="4 phones"):
        engine.run_wire_session((None, 2, 4), types.SimpleNamespace(batch=batch))


# ------------------------------------------------------------------ regeneration

# the reference's place, as oracle/Makefile takes it (REFERENCE, from the environment too)
REF_DIR = os.path.join(os.environ.get("REFERENCE") or "/root/reference", "Kalman Filter Server", "PoseEstimator")
REF_PARSER = os.path.join(ROOT, "oracle", "_ref", "ref_parser")
needs_reference = pytest.mark.skipif(not (os.path.isdir(REF_DIR) and os.path.exists(REF_PARSER)),
                                     reason="the reference or oracle/_ref/ref_parser is not present here")


def _tree(top):
    return sorted(os.path.join(d, f) for d, _, files in os.walk(top) for f in files)


@needs_reference
def test_make_parser_golden_regenerates_the_committed_fixture(tmp_path):
    """The generator, through the binary built from the reference, reproduces parser.npz array for array,
    and leaves nothing new under the reference."""
    before = _tree(os.path.dirname(os.path.dirname(REF_DIR)))
    env = dict(os.environ, PEKF_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_parser_golden.py")], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(os.path.join(GOLDEN, "parser.npz")) as a, np.load(os.path.join(tmp_path, "parser.npz")) as b:
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    assert _tree(os.path.dirname(os.path.dirname(REF_DIR))) == before
