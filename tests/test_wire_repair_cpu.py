"""A refused wire frame is its phone's business, without a GPU: wire.parse_frames (pekf_wire_parse_frames, the
frame-wise host parse) against the reference parser's recorded outcomes and values (tests/golden/parser.npz); the
call sequences of engine.wire_events / run_wire_session / PhoneSession.feed_frames with refused="raise" and
refused="repair" on a recording fake of the library (a clean error word: the launches of before; a refused frame:
at most one gather, exactly one patch, before phase 2); what the host hands the patch launch; the session's
stopped mark in its host book; the new entries' argument checks against the real library (they return before any
device call); and the host entry under AddressSanitizer / UndefinedBehaviorSanitizer in a program of its own."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from poseestimationkf_amd import synth, wire  # noqa: F401  (binds the real library before any fake is installed)

from .conftest import ROOT
from .test_parser_golden import NOHASH, OBS_TIME, OBS_TYPE, OBS_VALUES, OK, SHORT, THREW, load_golden, same_bits

NONE_W = np.uint64(synth.EV64_NONE_W)


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def lib():
    from poseestimationkf_amd import _lib
    return _lib


# ------------------------------------------------------------------ wire.parse_frames against the fixture

def test_parse_frames_statuses_are_the_reference_parsers_outcomes(golden):
    """All 73 number and message forms: no '#' / short / threw / processed as the reference's Parser, type_newline
    (a '\\n' Type: one message no sensor takes, which the line parse reads as two short lines) included; the parsed
    fields where the reference's state shows them, bit for bit; zeros for every frame that is no message."""
    z = golden
    assert (wire.NO_HASH, wire.SHORT, wire.THROWS, wire.MESSAGE) == (NOHASH, SHORT, THREW, OK)
    got = wire.parse_frames(z["forms_frames"])
    names = list(z["forms_names"])
    assert len(names) == 73 and got["status"].dtype == np.uint8
    wrong = [(n, int(g), int(w)) for n, g, w in zip(names, got["status"], z["forms_outcome"]) if g != w]
    assert not wrong, wrong
    f = names.index("type_newline")
    assert got["status"][f] == OK and got["phase"][f] == 3 and got["types"][f] == (ord("\n") - ord("0")) % 256
    shown = 0
    for f, name in enumerate(names):
        if z["forms_outcome"][f] != OK:
            assert not got["phase"][f] and not got["types"][f] and not got["times"][f], name
            assert (got["values"][f].view(np.uint64) == 0).all(), name
            continue
        assert int(got["phase"][f]) == (int(z["forms_phase"][f]) - ord("0")) % 256, name
        obs = int(z["forms_obs"][f])
        if obs & OBS_TYPE:
            assert int(got["types"][f]) == int(z["forms_type"][f]) - ord("0"), name
        if obs & OBS_VALUES:   # (the trace prints NaNs without their sign bit: any NaN equals any NaN)
            assert same_bits(got["values"][f], z["forms_values"][f]), name
        if obs & OBS_TIME:
            assert int(got["times"][f]) == int(z["forms_time"][f]), name
        shown += obs == 7
    assert shown >= 35


@pytest.mark.parametrize("p", ["plain", "tedge", "phase1"])
def test_parse_frames_of_client_streams_equals_the_line_parse(golden, p):
    """The client's own frames: every one processed, and field for field wire.parse of the same text (which
    test_parser_golden holds to the reference)."""
    fr = golden[p + "_frames"]
    got, want = wire.parse_frames(fr), wire.parse(fr.tobytes())
    assert (got["status"] == OK).all() and len(want["types"]) == len(fr)
    for key in ("phase", "types", "times"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["values"].view(np.uint64), want["values"].view(np.uint64))


def test_parse_frames_goes_on_after_a_frame_that_throws(golden):
    z = golden
    names = list(z["forms_names"])
    fr = np.stack([z["forms_frames"][names.index(n)] for n in ("x_huge", "last_plain", "missing_comma", "x_hex")])
    got = wire.parse_frames(fr)
    assert got["status"].tolist() == [THREW, OK, THREW, OK]
    assert got["values"][1].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        wire.parse_frames(np.zeros((2, 99), np.uint8))
    assert len(wire.parse_frames(np.zeros((0, 100), np.uint8))["status"]) == 0


# ------------------------------------------------------------------ the new entries' argument checks

P = 4096  # a non-null, 16-byte aligned address; every call below returns before anything reads it


def _records(*rows):
    """pekf_wire_patch_col records from (col, from_row, n_cells) triples"""
    from poseestimationkf_amd.engine import _PATCH_COL
    rec = np.zeros(len(rows), _PATCH_COL)
    for r, (col, from_row, n_cells) in zip(rec, rows):
        r["col"], r["from_row"], r["n_cells"], r["bad_frame"] = col, from_row, n_cells, -1
    return rec


def _patch_args(batch=8, rec=None, cell_rows=2, cells=P, e=(8, 8, 8), ev1=P, ev2=P, ev3=P, t2=P, n1=P, n2=P, n3=P, bad=P,
                n_rows=0, bounds=None, rec_dev=P):
    rec = _records((1, 0, 1)) if rec is None else rec
    return (batch, len(rec), rec.ctypes.data, rec_dev, cell_rows, cells, e[0], e[1], e[2], ev1, ev2, ev3, t2, n1, n2, n3, bad,
            n_rows, bounds, None), rec


@pytest.mark.parametrize("kw,msg", [
    (dict(ev2=P + 8), "misaligned"),
    (dict(ev1=P + 4), "misaligned"),
    (dict(cells=P + 8), "misaligned"),
    (dict(rec=(8, 0, 1)), "column 8 outside"),
    (dict(rec=(-1, 0, 1)), "column -1 outside"),
    (dict(rec=(1, -1, 1)), "negative from_row"),
    (dict(rec=(1, 0, -1)), "negative from_row"),
    (dict(rec=(1, 0, 3)), "n_cells above cell_rows"),
    (dict(batch=-1), "negative size"),
    (dict(cell_rows=-1), "negative size"),
    (dict(e=(8, -1, 8)), "negative size"),
    (dict(ev1=None), "ev1 and n1 together"),
    (dict(cells=None), "null pointer"),
    (dict(rec_dev=None), "null pointer"),
    (dict(rec_dev=P + 4), "misaligned"),
    (dict(n2=None), "null pointer"),
    (dict(n_rows=9, bounds=P), "row_bounds"),
])
def test_patch_arguments_are_refused_before_any_launch(lib, kw, msg):
    if "rec" in kw:
        kw = dict(kw, rec=_records(kw["rec"]))
    args, keep = _patch_args(**kw)
    assert lib.lib.pekf_wire_patch_dev(*args) == lib.PEKF_ERR_INVALID
    assert msg in lib.last_error(), lib.last_error()


def test_patch_and_gather_without_work_launch_nothing(lib):
    L = lib.lib
    args, keep = _patch_args(rec=_records())          # n_cols = 0, no row bounds
    assert L.pekf_wire_patch_dev(*args) == lib.PEKF_OK
    args, keep = _patch_args(batch=0)
    assert L.pekf_wire_patch_dev(*args) == lib.PEKF_OK
    assert L.pekf_wire_gather_frames_dev(8, 4, P, 0, P, 0, P, None) == lib.PEKF_OK       # no column
    assert L.pekf_wire_gather_frames_dev(8, 4, P, 2, P, 4, P, None) == lib.PEKF_OK       # no frame from frame0 on
    for bad, msg in (((8, 4, P + 2, 2, P, 0, P, None), "misaligned"), ((8, 4, P, 2, P, 5, P, None), "frame0"),
                     ((8, 4, P, -1, P, 0, P, None), "negative size"), ((8, 4, P, 2, None, 0, P, None), "null pointer"),
                     ((8, 4, P, 9, P, 0, P, None), "n_cols must be <= batch")):
        assert L.pekf_wire_gather_frames_dev(*bad) == lib.PEKF_ERR_INVALID
        assert msg in lib.last_error(), lib.last_error()
    assert lib.lib.pekf_abi_version() == 1
    assert ctypes.sizeof(ctypes.c_int32) * 12 + 8 == 56   # pekf_wire_patch_col, as engine._PATCH_COL packs it


# ------------------------------------------------------------------ the call sequences

RECORDED = ("pekf_frontend_init_ext_dev", "pekf_live_ext_dev", "pekf_live_traj_dev", "pekf_magcal_dev",
            "pekf_magcal_apply_dev", "pekf_magcal_resume_dev", "pekf_frontend_init_resume_dev", "pekf_live_join_dev",
            "pekf_session_recycle_dev", "pekf_session_export_dev", "pekf_session_import_dev")
EV64 = 0x4


def _recording_fake(monkeypatch):
    """tests/fake_libpekf.py's host fake with the wire session's entry points: the session's launches are recorded
    and compute nothing; the parse entries write zero counts, and for the phones of `refuse` ({phone: frame}) the
    bad_frame plane and the error word, as the kernel reports a refused frame; the gather copies; the patch keeps
    what it was handed."""
    from . import fake_libpekf

    class Fake(fake_libpekf.FakeLib):
        refuse = {}
        patches = []

        def _rec(self, name):
            def f(*a):
                self.calls.append(name)
                return 0
            return f

        def __getattr__(self, name):
            if name in RECORDED:
                return self._rec(name)
            raise AttributeError("fake libpekf has no %s" % name)

        def pekf_live_state_bytes(self, batch, flags):
            return batch * 336 if flags == EV64 else -1

        def pekf_frontend_init_state_bytes(self, batch, flags):
            return batch * 112

        def pekf_magcal_state_bytes(self, batch, n_cal, flags):
            return batch * (((24 * n_cal + 15) & ~15) + 32)

        def pekf_session_columns_bytes(self, n, n_cal, flags):
            return 16 * n

        def pekf_memset(self, p, value, n, stream):
            self._view(p, n)[:] = value
            return 0

        def _parse(self, name, K, F, planes, counts, t2, bad, err):
            self.calls.append(name)
            for ev in planes:
                v = self._view(ev, 32 * F * K, np.uint64).reshape(F, K, 4)
                v[:] = 0
                v[..., 3] = NONE_W
            for c in counts:
                self._view(c, 4 * K, np.int32)[:] = 0
            self._view(t2, 8 * K, np.int64)[:] = 0
            b = self._view(bad, 4 * K, np.int32)
            b[:] = -1
            for k, f in self.refuse.items():
                b[k] = f
            self._view(err, 4, np.int32)[0] = 1 if self.refuse else 0
            return 0

        def pekf_wire_events_ext_dev(self, K, F, frames, e2, e3, ev2, ev3, t2, n2, n3, bad, err, bounds, flags, stream):
            return self._parse("pekf_wire_events_ext_dev", K, F, (ev2, ev3), (n2, n3), t2, bad, err)

        def pekf_wire_events_p1_dev(self, K, F, frames, e1, e2, e3, ev1, ev2, ev3, t2, n1, n2, n3, bad, err, bounds,
                                    flags, stream):
            return self._parse("pekf_wire_events_p1_dev", K, F, (ev1, ev2, ev3), (n1, n2, n3), t2, bad, err)

        def pekf_wire_gather_frames_dev(self, K, F, frames, n, cols, f0, out, stream):
            self.calls.append("pekf_wire_gather_frames_dev")
            src = self._view(frames, 100 * F * K).reshape(F, K, 100)
            c = self._view(cols, 4 * n, np.int32)
            self._view(out, 100 * n * (F - f0)).reshape(n, F - f0, 100)[:] = src[f0:, c].transpose(1, 0, 2)
            return 0

        def pekf_wire_patch_dev(self, K, n, cols, cols_dev, cell_rows, cells, e1, e2, e3, ev1, ev2, ev3, t2, n1, n2, n3, bad,
                                n_rows, bounds, stream):
            from poseestimationkf_amd.engine import _PATCH_COL
            self.calls.append("pekf_wire_patch_dev")
            rec = self._view(cols_dev, 56 * n).view(_PATCH_COL).copy()   # (what the kernel reads)
            assert rec.tobytes() == self._view(cols, 56 * n).tobytes()
            cl = (self._view(cells, 96 * cell_rows * n, np.uint64).reshape(3, cell_rows, n, 4).copy()
                  if cell_rows else np.zeros((3, 0, n, 4), np.uint64))
            self.patches.append(dict(rec=rec, cells=cl, e=(e1, e2, e3), ev1=ev1, n1=n1, n_rows=n_rows,
                                     bounds=bounds is not None))
            if bounds is not None:
                self._view(bounds, 12, np.int32)[:] = 0
            return 0

    from poseestimationkf_amd import _lib, engine, shard
    fake = Fake(1)
    fake.refuse, fake.patches = {}, []
    for mod in (_lib, engine, shard):
        monkeypatch.setattr(mod, "lib", fake)
    return fake, engine


def _blank(F, K):
    return np.full((F, K, 100), ord(" "), np.uint8)


def _frame(text):
    return np.frombuffer(text.ljust(99).encode("latin-1") + b"\n", np.uint8)


PARSE, PARSE1 = "pekf_wire_events_ext_dev", "pekf_wire_events_p1_dev"
SESSION = ["pekf_frontend_init_ext_dev", "pekf_live_ext_dev"]
CALIBRATED = ["pekf_magcal_dev", "pekf_magcal_apply_dev", "pekf_magcal_apply_dev"] + SESSION
CHUNK = ["pekf_frontend_init_resume_dev", "pekf_live_join_dev"]


@pytest.mark.parametrize("refused", ["raise", "repair"])
def test_a_clean_error_word_makes_todays_calls(monkeypatch, refused):
    """No refused frame: wire_events, run_wire_session (both layouts, with and without calibration="frames") and
    feed_frames (with and without n_cal) make exactly the launches of before, whichever `refused` is; only the
    repair mode's results carry bad_frame / repaired."""
    fake, engine = _recording_fake(monkeypatch)
    K, F = 8, 4
    fr = _blank(F, K)
    for rows in (False, True):
        for p1 in (False, True):
            fake.calls.clear()
            w = engine.wire_events(fr, frame_rows=rows, phase1=p1, refused=refused)
            assert fake.calls == [PARSE1 if p1 else PARSE]
            assert ("bad_frame" in w) == ("repaired" in w) == (refused == "repair")
        for cal, want in ((None, [PARSE] + SESSION), ("frames", [PARSE1] + CALIBRATED)):
            fake.calls.clear()
            out = engine.run_wire_session(fr, engine.BatchedEKF(K), frame_rows=rows, calibration=cal, refused=refused)
            assert fake.calls == want
            extra = ["bad_frame", "repaired"] if refused == "repair" else []
            base = ["counts", "ready", "refs"] + (["calibrated", "calibration"] if cal else [])
            assert sorted(out) == sorted(base + extra)
            if extra:
                assert (out["bad_frame"] == -1).all() and not out["repaired"].any()
    for n_cal, want in ((None, [PARSE] + CHUNK), (6, [PARSE1, "pekf_magcal_resume_dev"] + CHUNK)):
        s = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5, n_cal=n_cal)
        fake.calls.clear()
        out = s.feed_frames(fr, refused=refused)
        assert fake.calls == want
        assert len(out) == (4 if refused == "repair" else 2)
        assert not s.stopped.any() and ("stopped" in s._book) == (refused == "repair")
    assert fake.patches == []


def test_the_default_is_raise_and_its_message_is_todays(monkeypatch):
    fake, engine = _recording_fake(monkeypatch)
    fake.refuse = {5: 2, 3: 1}
    fr = _blank(4, 8)
    for call in (lambda: engine.wire_events(fr), lambda: engine.wire_events(fr, refused="raise"),
                 lambda: engine.run_wire_session(fr, engine.BatchedEKF(8)),
                 lambda: engine.PhoneSession(engine.BatchedEKF(8), n_avg=5).feed_frames(fr)):
        fake.calls.clear()
        with pytest.raises(ValueError, match=r"phone 3, frame 1: not in the client's message form \(wire.parse reads it\)"):
            call()
        assert fake.calls == [PARSE]


def test_an_unknown_refused_string_is_refused_before_any_launch(monkeypatch):
    fake, engine = _recording_fake(monkeypatch)
    fr = _blank(4, 8)
    s = engine.PhoneSession(engine.BatchedEKF(8), n_avg=5)
    fake.calls.clear()
    for call in (lambda: engine.wire_events(fr, refused="ignore"),
                 lambda: engine.run_wire_session(fr, engine.BatchedEKF(8), refused="Repair"),
                 lambda: s.feed_frames(fr, refused=None)):
        with pytest.raises(ValueError, match="refused must be"):
            call()
    assert fake.calls == []


def _refusing_frames(F=6, K=8):
    """Phone 2: "+1.5" at frame 1 (a form std::stod reads), then a phase-2 and a phase-3 client frame; phone 5:
    a hex value at frame 3, then a frame std::stod throws on at frame 4 and a valid one after it; phone 6: a
    phase-3 time of 2^51 at frame 0."""
    fr = _blank(F, K)
    fr[1, 2] = _frame("#3,1:+1.5,7,.5,t:1000")
    fr[2, 2] = _frame("#2,0:0.25,0.5,1.0,t:2000")
    fr[4, 2] = _frame("#3,2:1.0,2.0,3.0,t:3000")
    fr[3, 5] = _frame("#2,1:0x1p3,2.5,1e5,t:500")
    fr[4, 5] = _frame("#3,1:1e999,2.0,3.0,t:600")
    fr[5, 5] = _frame("#3,1:1.0,2.0,3.0,t:700")
    fr[0, 6] = _frame("#3,1:1.0,2.0,3.0,t:%d" % 2 ** 51)
    return fr, {2: 1, 5: 3, 6: 0}


def _cell(ty, v, t):
    out = np.empty(4, np.uint64)
    out[:3] = np.asarray(v, np.float64).view(np.uint64)
    out[3] = np.array([float(t)]).view(np.uint64)[0] | np.uint64(ty)
    return out


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("rows", [False, True])
def test_a_refused_frame_is_one_patch_before_phase_2(monkeypatch, rows, device):
    """The error word set: at most one gather (frames on the device only), exactly one patch, then the session's
    launches; and what the patch is handed -- per refused phone its rows, cells, counts, first phase-2 time and
    the frame that stopped it for good."""
    fake, engine = _recording_fake(monkeypatch)
    fr, fake.refuse = _refusing_frames()
    F, K = fr.shape[:2]
    frames = (engine.DeviceBuffer(fr.nbytes).upload(fr), F, K) if device else fr
    out = engine.run_wire_session(frames, engine.BatchedEKF(K), frame_rows=rows, refused="repair")
    gather = ["pekf_wire_gather_frames_dev"] if device else []
    assert fake.calls == [PARSE] + gather + ["pekf_wire_patch_dev"] + SESSION
    assert out["bad_frame"].tolist() == [-1, -1, -1, -1, -1, 4, 0, -1]
    assert out["repaired"].tolist() == [False, False, True, False, False, True, False, False]
    (patch,) = fake.patches
    rec, cells = patch["rec"], patch["cells"]
    assert rec["col"].tolist() == [2, 5, 6] and rec["bad_frame"].tolist() == [-1, 4, 0]
    assert patch["ev1"] is None and patch["n1"] is None and patch["e"] == (0, F, F)
    assert patch["bounds"] == rows and patch["n_rows"] == (F if rows else 0)
    assert rec["n"].tolist() == [[0, 1, 2], [0, 1, 0], [0, 0, 0]]
    assert rec["first_t2"].tolist() == [2000, 500, 0]
    a = _cell(1, [1.5, 7.0, 0.5], 1000)
    b = _cell(0, [0.25, 0.5, 1.0], 2000)
    c = _cell(2, [1.0, 2.0, 3.0], 3000)
    d = _cell(1, [8.0, 2.5, 1e5], 500)
    none = _cell(3, [0, 0, 0], -0.0)
    assert none[3] == NONE_W
    if rows:   # from the refused frame on, row f; cells up to the phone's last message of the plane
        assert rec["from_row"].tolist() == [[0, 1, 1], [0, 3, 3], [0, 0, 0]]
        assert rec["n_cells"].tolist() == [[0, 2, 4], [0, 1, 0], [0, 0, 0]]
        assert np.array_equal(cells[1, :2, 0], [none, b]) and np.array_equal(cells[2, :4, 0], [a, none, none, c])
        assert np.array_equal(cells[1, 0, 1], d)
    else:      # the phone's next compacted rows (the fake's counts before the refused frame are 0)
        assert rec["from_row"].tolist() == [[0, 0, 0]] * 3
        assert rec["n_cells"].tolist() == [[0, 1, 2], [0, 1, 0], [0, 0, 0]]
        assert np.array_equal(cells[1, 0, 0], b) and np.array_equal(cells[2, :2, 0], [a, c])
        assert np.array_equal(cells[1, 0, 1], d)
    assert (cells[0, ..., 3] == NONE_W).all() and (cells[:, :, 2, 3] == NONE_W).all()   # no plane 1; phone 6: none


def test_phase1_messages_are_patched_into_their_plane(monkeypatch):
    """With the phase-1 plane a phase-1 message is kept whatever its Type, and a time the event cannot hold is
    stored as 0; without it the message is skipped."""
    fake, engine = _recording_fake(monkeypatch)
    fr = _blank(3, 4)
    fr[0, 1] = _frame("#1,7: 2.5,1.5abc,00000000000000000001.0,t:%d" % 2 ** 60)
    fr[2, 1] = _frame("#1,1:1.0,2.0,3.0,t:9")
    fake.refuse = {1: 0}
    w = engine.wire_events(fr, frame_rows=True, phase1=True, refused="repair")
    assert fake.calls == [PARSE1, "pekf_wire_patch_dev"] and w["bad_frame"][1] == -1 and w["repaired"][1]
    (patch,) = fake.patches
    assert patch["rec"]["n"].tolist() == [[2, 0, 0]] and patch["rec"]["n_cells"].tolist() == [[3, 0, 0]]
    assert patch["e"] == (3, 3, 3) and patch["ev1"] is not None and w["n1"].tolist() == [0, 2, 0, 0]
    assert np.array_equal(patch["cells"][0, 0, 0], _cell(3, [2.5, 1.5, 1.0], 0))
    assert np.array_equal(patch["cells"][0, 2, 0], _cell(1, [1.0, 2.0, 3.0], 9))
    fake.patches.clear()
    w = engine.wire_events(fr, frame_rows=True, refused="repair")
    assert fake.patches[0]["rec"]["n"].tolist() == [[0, 0, 0]] and w["repaired"][1]


# ------------------------------------------------------------------ the session's host book

def _stopping_chunks(K=8):
    a = _blank(3, K)
    a[1, 3] = _frame("#3,1:1e999,2.0,3.0,t:600")        # std::stod throws: phone 3 stops at frame 1 of the chunk
    a[2, 3] = _frame("#3,1:1.0,2.0,3.0,t:700")
    b = _blank(2, K)
    b[0, 3] = _frame("#3,1:1.0,2.0,3.0,t:800")          # what a stopped phone goes on sending changes nothing
    return a, b


@pytest.mark.parametrize("n_cal", [None, 6])
def test_a_stopped_column_is_blanked_until_it_is_recycled(monkeypatch, n_cal):
    fake, engine = _recording_fake(monkeypatch)
    K = 8
    a, b = _stopping_chunks(K)
    s = engine.PhoneSession(engine.BatchedEKF(K), n_avg=5, n_cal=n_cal)
    assert not s.stopped.any() and "stopped" not in s.snapshot()["book"]
    fake.refuse = {3: 1}
    out = s.feed_frames(a, refused="repair")
    assert out[-2].tolist() == [-1, -1, -1, 1, -1, -1, -1, -1] and not out[-1].any()
    assert s.stopped.tolist() == [False] * 3 + [True] + [False] * 4
    got = s.stopped
    got[:] = True
    assert s.stopped.sum() == 1                                       # a copy
    # the next chunks: the error word is clean, and the stopped column is still patched blank -- in either mode
    fake.refuse = {}
    for mode in ("repair", "raise"):
        fake.calls.clear()
        fake.patches.clear()
        out = s.feed_frames(b, refused=mode)
        assert fake.calls.count("pekf_wire_patch_dev") == 1 and "pekf_wire_gather_frames_dev" not in fake.calls
        assert fake.calls.index("pekf_wire_patch_dev") == 1 and fake.calls[-2:] == CHUNK
        rec = fake.patches[0]["rec"]
        assert rec["col"].tolist() == [3] and not rec["from_row"].any() and not rec["n_cells"].any()
        assert not rec["n"].any() and rec["bad_frame"].tolist() == [-1] and fake.patches[0]["cells"].shape[1] == 0
        if mode == "repair":
            assert (out[-2] == -1).all() and not out[-1].any()
    # a refused frame of a stopped phone raises nothing, another phone's does
    fake.refuse = {3: 0}
    s.feed_frames(b)
    fake.refuse = {3: 0, 4: 1}
    with pytest.raises(ValueError, match="phone 4, frame 1"):
        s.feed_frames(b)
    fake.refuse = {}
    # snapshot / restore carry the mark; a snapshot from before it existed restores with none stopped
    snap = s.snapshot()
    assert snap["book"]["stopped"].tolist() == s.stopped.tolist()
    again = engine.PhoneSession.restore(engine.BatchedEKF(K), snap)
    assert again.stopped.tolist() == s.stopped.tolist()
    del snap["book"]["stopped"]
    assert not engine.PhoneSession.restore(engine.BatchedEKF(K), snap).stopped.any()
    # export / import / move carry it with the rest of the host book
    fork = s.export_columns([3, 0], release=False)
    assert fork.book["stopped"].tolist() == [True, False] and s.stopped[3]
    back = engine.SessionColumns.from_host(fork.to_host())
    other = engine.PhoneSession(engine.BatchedEKF(4), n_avg=5, n_cal=n_cal)
    other.import_columns([1, 2], back)
    assert other.stopped.tolist() == [False, True, False, False]
    s.move([3], [6])
    assert s.stopped.tolist() == [False] * 6 + [True, False]
    # recycle clears it: the column's next phone starts afresh, and nothing is patched any more
    s.recycle([6])
    assert not s.stopped.any()
    fake.calls.clear()
    s.feed_frames(b, refused="repair")
    assert "pekf_wire_patch_dev" not in fake.calls


# ------------------------------------------------------------------ the host entry under the sanitizers

@pytest.fixture(scope="module")
def frames_harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("asan_frames") / "wire_frames_harness"
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "wire_frames_harness.cpp"),
           os.path.join(ROOT, "poseestimationkf_amd", "csrc", "pekf_wire.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


def test_parse_frames_under_sanitizers(frames_harness, golden, tmp_path):
    """tests/native/wire_frames_harness.cpp, run directly: the fixture's frames (every form, and a client's
    stream) and 4,000 frames of random bytes, NULs included, without a sanitizer report; the statuses it prints
    are the fixture's outcomes."""
    z = golden
    paths = []
    for name in ("forms", "plain"):
        p = tmp_path / (name + ".frames")
        p.write_bytes(z[name + "_frames"].tobytes())
        paths.append(str(p))
    r = subprocess.run([frames_harness] + paths, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                UBSAN_OPTIONS="print_stacktrace=1"))
    report = r.stdout + r.stderr
    assert r.returncode == 0 and "Sanitizer" not in report and "runtime error" not in report, report[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 5
    fields = [dict(kv.split("=", 1) for kv in line.split()[1:]) for line in lines[:4]]
    assert all(f["rc"] == "0" for f in fields)
    assert fields[0]["st"] == "".join(str(int(o)) for o in z["forms_outcome"])
    assert fields[1]["st"] == "3" * len(z["plain_frames"])
    assert fields[1]["t"] == str(int(wire.parse_frames(z["plain_frames"])["times"].astype(np.uint64).sum()))
    noise = fields[2]["st"]
    assert fields[2]["n"] == "4000" and set(noise) == set("0123") and fields[3]["n"] == "0"
    assert lines[4] == "null rc=1 negative rc=1"
