"""Live sessions from a phone's first message (engine.PhoneSession: pekf_frontend_init_resume_dev and
pekf_live_join_dev per chunk): however a session's rows are cut into chunks, every output has the bits of the
one-shot session.

The yardstick is the existing one-shot path, whose kernels are not under test: engine.run_session(phase2,
phase3, filters, events="f64", trajectory=True) -- for frames engine.run_wire_session -- X, P, refs, ready,
counts, every trajectory row, its dt and its time.  Phone k's phase-2 messages sit in rows [s_k, s_k + L2_k) of
the phase-2 plane and its phase-3 messages in the following rows of the phase-3 plane, s_k and L2_k differing
from phone to phone, so that in one chunk some phones still average, some get ready and some already filter:
they join the fused session in different chunks, some never get ready (their phase-3 messages are dropped),
some are ready long before their first phase-3 message while their t_init moves, some never send one."""
import numpy as np
import pytest

from oracle import frontend_numpy as fe
from poseestimationkf_amd import synth, wire

from .test_live import ATOL_F64_CHAIN
from .test_live_resume import Collected
from .test_live_traj import _resumed

pytestmark = pytest.mark.gpu

N_AVG = 5


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


def _planes_of(K, E, seed):
    """(phase2, phase3) event dicts of E rows on one timeline, synth.EV_NONE where a phone has no message"""
    gen = synth.generate_events(np.arange(K), E, seed=seed)
    rng = np.random.default_rng(seed)
    k = np.arange(K)
    s = rng.integers(0, E // 7, K)
    L2 = rng.integers(int(0.35 * E), int(0.55 * E), K)
    L2[k % 7 == 4] = int(0.65 * E)          # ready long before the first phase-3 message: t_init keeps moving
    L2[k % 11 == 5] = E                     # phase 2 to the end: ready, no phase-3 message at all
    L2[k % 7 == 2] = 8                      # too few messages: never ready, with phase-3 messages after
    L3 = np.where(k % 5 == 1, E // 4, E)    # some stop early
    rows = np.arange(E)[:, None]
    in2 = (rows >= s) & (rows < s + L2)
    in3 = (rows >= s + L2) & (rows < s + L2 + L3)
    v64 = wire.server_values(gen["values"])
    common = dict(values=gen["values"], values64=v64, times=gen["times"], t_init=gen["t_init"])
    phase2 = dict(common, types=np.where(in2, gen["types"], synth.EV_NONE).astype(np.uint32))
    phase3 = dict(common, types=np.where(in3, gen["types"], synth.EV_NONE).astype(np.uint32))
    return phase2, phase3


def _one_shot(eng, phase2, phase3, K, X0, P0, calibration=None):
    f = eng.BatchedEKF(K)
    f.set_state(X0, P0)
    out = eng.run_session(phase2, phase3, f, n_avg=N_AVG, events="f64", trajectory=True, calibration=calibration)
    X, P = f.get_state()
    return X, P, out


def _rows(ev, a, b):
    return {key: ev[key][a:b] for key in ("types", "values", "values64", "times")}


def _cuttings(E, seed=0, most=30):
    def by(n):
        return [(a, min(a + n, E)) for a in range(0, E, n)]
    rng = np.random.default_rng(2000 + seed)
    sizes = [0]
    while sum(sizes) < E:
        sizes.append(int(rng.integers(0, most)))
        if len(sizes) == 2 or rng.random() < 0.2:
            sizes.append(0)
    edges = np.minimum(np.cumsum([0] + sizes + [0]), E)
    out = {"1": by(1), "2": by(2), "3": by(3), "4": by(4), "random": list(zip(edges[:-1], edges[1:]))}
    assert sum(a == b for a, b in out["random"]) >= 3
    return out


class Fed:
    """What a chunked session gave, put together"""

    def __init__(self, K, rows):
        self.got, self.total, self.ready = Collected(K, rows), np.zeros(K, np.int64), None

    def add(self, out):
        counts, self.ready, tj = out
        self.got.add(counts, tj)
        self.total += counts


def _chunked(eng, phase2, phase3, K, X0, P0, cuts, how="planes", calibration=None, between=None):
    E = phase3["types"].shape[0]
    f = eng.BatchedEKF(K)
    f.set_state(X0, P0)
    s = eng.PhoneSession(f, n_avg=N_AVG, t_start=phase2["t_init"])
    fed = Fed(K, E // 3 + 1)
    if how == "planes":
        p2 = synth.pack_events64(phase2, phase2["values64"])
        p3 = synth.pack_events64(phase3, phase3["values64"])
        b2, b3 = eng.DeviceBuffer(p2.nbytes).upload(p2), eng.DeviceBuffer(p3.nbytes).upload(p3)
        row = p2[0].nbytes
    for a, b in cuts:
        a, b = int(a), int(b)
        if how == "planes":
            fed.add(s.feed_planes(b2, b - a, b3, b - a, trajectory=True, offset2=a * row, offset3=a * row))
        else:
            fed.add(s.feed(_rows(phase2, a, b), _rows(phase3, a, b), trajectory=True, calibration=calibration))
        if between:
            between(s, fed)
    X, P = f.get_state()
    assert np.array_equal(s.total_counts, fed.total)
    return X, P, s.refs, fed, s


def _equals_one_shot(chunked, single, label=""):
    X, P, refs, fed, _ = chunked
    Xs, Ps, out = single
    assert np.array_equal(fed.ready, out["ready"]), label
    assert np.array_equal(fed.total, out["counts"]), label
    assert np.array_equal(np.isnan(refs), np.isnan(out["refs"])), label
    assert np.array_equal(refs, out["refs"], equal_nan=True), label
    assert np.array_equal(X, Xs) and np.array_equal(P, Ps), label
    got = fed.got
    R = min(len(got.traj), len(out["trajectory"]))
    assert out["counts"].max(initial=0) <= R
    for mine, theirs in ((got.traj, out["trajectory"]), (got.dt, out["record_dt_ns"]),
                         (got.times, out["record_times_ns"])):
        assert np.array_equal(mine[:R], theirs[:R], equal_nan=True), label
        assert np.isnan(mine[R:]).all() and np.isnan(theirs[R:]).all(), label


@pytest.fixture(scope="module")
def small(eng):
    """K = 70 (one full wave plus six lanes, ending inside an 8-lane group) x 100 rows and its one-shot session"""
    K, E = 70, 100
    phase2, phase3 = _planes_of(K, E, 41)
    X0, P0 = _resumed(K, 48)
    single = _one_shot(eng, phase2, phase3, K, X0, P0)
    _phones_are_out_of_step(K, phase3, X0, P0, single)
    return K, E, phase2, phase3, X0, P0, single


def _phones_are_out_of_step(K, phase3, X0, P0, single):
    """the small session is what the tests below need it to be"""
    Xs, Ps, out = single
    ready, counts = out["ready"], out["counts"]
    k = np.arange(K)
    assert 0 < ready.sum() < K and not ready[k % 7 == 2].any()
    silent = (k % 11 == 5) & (k % 7 != 2)
    assert (counts[ready & ~silent] > 0).mean() > 0.9 and len(set(counts)) > 5
    assert np.all(counts[~ready] == 0) and np.all(counts[silent] == 0) and ready[silent].all()
    # the never-ready phones have phase-3 messages, and their filters stay as they were
    assert (phase3["types"][:, ~ready] != synth.EV_NONE).any(axis=0).all()
    assert np.array_equal(Xs[~ready], X0[~ready]) and np.array_equal(Ps[~ready], P0[~ready])
    # phones join in different chunks: their first phase-3 message is spread over the rows
    first3 = np.argmax(phase3["types"] != synth.EV_NONE, axis=0)
    assert len(set(first3[ready])) > 10


@pytest.mark.parametrize("name", ["1", "2", "3", "4", "random"])
def test_any_cutting_gives_the_one_shot_session(eng, small, name):
    K, E, phase2, phase3, X0, P0, single = small
    ready = single[2]["ready"]
    moved = []

    def between(s, fed):
        """a never-ready phone's filter is untouched after every chunk; a ready phone's t_init moves while it
        has no phase-3 message yet"""
        X, P = s.filters.get_state()
        dead = ~fed.ready
        assert np.all(fed.total[dead] == 0)
        assert np.array_equal(X[dead], X0[dead]) and np.array_equal(P[dead], P0[dead])
        moved.append(s._t_init.download((K,), np.int64))

    chunked = _chunked(eng, phase2, phase3, K, X0, P0, _cuttings(E)[name], between=between if name != "1" else None)
    _equals_one_shot(chunked, single, "chunks of " + name)
    assert np.array_equal(chunked[0][~ready], X0[~ready]) and np.array_equal(chunked[1][~ready], P0[~ready])
    if moved:
        waiting = np.flatnonzero(np.arange(K) % 7 == 4)
        assert all(len(set(m[k] for m in moved)) > 2 for k in waiting)   # (its start value, then a move per chunk)


def test_feed_of_dict_chunks_equals_feed_planes(eng, small):
    K, E, phase2, phase3, X0, P0, single = small
    cuts = [(0, 0), (0, 13), (13, 13), (13, 14), (14, 50), (50, 77), (77, E), (E, E)]
    _equals_one_shot(_chunked(eng, phase2, phase3, K, X0, P0, cuts, how="dicts"), single)
    # chunks that carry one phase only: phase 2's rows of a range, then phase 3's, is the same session
    f = eng.BatchedEKF(K)
    f.set_state(X0, P0)
    s = eng.PhoneSession(f, n_avg=N_AVG)
    fed = Fed(K, E // 3 + 1)
    for a, b in _cuttings(E)["random"]:
        fed.add(s.feed(phase2=_rows(phase2, a, b), trajectory=True))
        fed.add(s.feed(phase3=_rows(phase3, a, b), trajectory=True))
    X, P = f.get_state()
    _equals_one_shot((X, P, s.refs, fed, s), single)
    # without a trajectory: counts and ready only
    f2 = eng.BatchedEKF(K)
    f2.set_state(X0, P0)
    s2 = eng.PhoneSession(f2, n_avg=N_AVG)
    total = 0
    for a, b in _cuttings(E)["4"]:
        counts, ready = s2.feed(_rows(phase2, a, b), _rows(phase3, a, b))
        total = total + counts
    assert np.array_equal(total, single[2]["counts"]) and np.array_equal(ready, single[2]["ready"])
    assert np.array_equal(f2.get_state()[0], single[0]) and np.array_equal(f2.get_state()[1], single[1])


def test_a_larger_batch_in_random_chunks(eng):
    K, E = 1000, 400
    phase2, phase3 = _planes_of(K, E, 42)
    X0, P0 = _resumed(K, 49)
    single = _one_shot(eng, phase2, phase3, K, X0, P0)
    assert 0 < single[2]["ready"].sum() < K and single[2]["counts"].max() > 20
    for seed in (1, 2):
        cuts = _cuttings(E, seed, most=98)["random"]
        _equals_one_shot(_chunked(eng, phase2, phase3, K, X0, P0, cuts), single, "random cutting %d" % seed)


def test_snapshot_and_restore_continue_the_session(eng, small):
    K, E, phase2, phase3, X0, P0, single = small
    f = eng.BatchedEKF(K)
    f.set_state(X0, P0)
    s = eng.PhoneSession(f, n_avg=N_AVG)
    fed = Fed(K, E // 3 + 1)
    for a, b in ((0, 30), (30, 47)):
        fed.add(s.feed(_rows(phase2, a, b), _rows(phase3, a, b), trajectory=True))
    snap = s.snapshot()
    assert 0 < (fed.total > 0).sum() < single[2]["ready"].sum()     # mid-session: some have joined, some not yet
    f.set_state(*_resumed(K, 50))                                   # the old filters go their own way
    s.feed(_rows(phase2, 47, 60), _rows(phase3, 47, 60))
    f2 = eng.BatchedEKF(K)
    s2 = eng.PhoneSession.restore(f2, snap)
    assert np.array_equal(s2.total_counts, fed.total)
    for a, b in ((47, 48), (48, 80), (80, E)):
        fed.add(s2.feed(_rows(phase2, a, b), _rows(phase3, a, b), trajectory=True))
    X, P = f2.get_state()
    _equals_one_shot((X, P, s2.refs, fed, s2), single)


def test_calibrated_session(eng):
    """calibration: calibrate_magnetometer's dict, applied to both chunks of every feed, against
    run_session(calibration=...)"""
    K, E = 70, 100
    phase2, phase3 = _planes_of(K, E, 43)
    ph1 = synth.generate_calibration_events(K, 101, seed=44)
    ph1["types"][100, 7] = synth.EV_NONE                     # phone 7 is not calibrated: its samples stay raw
    calib = eng.calibrate_magnetometer(ph1, n_cal=100, events="f64")
    assert calib["calibrated"].sum() > K // 2 and not calib["calibrated"][7]
    X0, P0 = _resumed(K, 51)
    single = _one_shot(eng, phase2, phase3, K, X0, P0, calibration=calib)
    plain = _one_shot(eng, phase2, phase3, K, X0, P0)
    assert not np.array_equal(single[0], plain[0])
    chunked = _chunked(eng, phase2, phase3, K, X0, P0, _cuttings(E)["random"], how="dicts", calibration=calib)
    _equals_one_shot(chunked, single)


# ------------------------------------------------------------------ the wire

@pytest.fixture(scope="module")
def wired(eng):
    """The frames of a small session, built as tests/test_wire_dev.py builds its own: phones whose phase-2
    parts differ in length (one too short to get ready), so that their phase-3 frames drift apart"""
    K = 40
    ph2 = synth.generate_events(np.arange(K), 70, seed=65)
    ph3 = synth.generate_events(np.arange(K), 80, seed=66)
    ph3 = dict(ph3, times=ph3["times"] - ph3["t_init"][None, :] + ph2["times"][-1][None, :])
    texts = []
    for k in range(K):
        n2, n3 = (9 if k % 9 == 4 else 50 + 2 * (k % 11)), 80 - 9 * (k % 5)
        texts.append(wire.events_text(ph2["types"][:n2, k], ph2["values"][:n2, k], ph2["times"][:n2, k], phase=2) +
                     wire.events_text(ph3["types"][:n3, k], ph3["values"][:n3, k], ph3["times"][:n3, k], phase=3))
    fr = wire.frames(texts)
    f = eng.BatchedEKF(K)
    out = eng.run_wire_session(fr, f, n_avg=N_AVG, trajectory=True)
    X, P = f.get_state()
    assert 0 < out["ready"].sum() < K and (out["counts"][out["ready"]] > 0).mean() > 0.9
    return K, fr, (X, P, out)


@pytest.mark.parametrize("name", ["1", "5", "random"])
def test_frames_in_chunks_equal_the_wire_session(eng, wired, name):
    K, fr, single = wired
    F = fr.shape[0]
    cuts = {"1": [(a, a + 1) for a in range(F)], "5": [(a, min(a + 5, F)) for a in range(0, F, 5)],
            "random": _cuttings(F, 3)["random"]}[name]
    f = eng.BatchedEKF(K)
    s = eng.PhoneSession(f, n_avg=N_AVG)
    fed = Fed(K, F // 3 + 1)
    for a, b in cuts:
        fed.add(s.feed_frames(fr[int(a):int(b)], trajectory=True))
    X, P = f.get_state()
    _equals_one_shot((X, P, s.refs, fed, s), single, "frames in chunks of " + name)


# ------------------------------------------------------------------ the oracle chain

def test_chunked_session_follows_the_oracle_chain(eng, small):
    """Every ready phone of the small session, fed in chunks of 3, against the restatement end to end: phase 2
    (frontend_numpy.initial_values), phase 3 (run_frontend) and ekf_numpy.run_filter from X0 / P0, on the phone's
    own messages with the server's values.  The worst distance is printed: 5.4e-13 over 176 records on an MI355X
    (from X0 / P0 = 0.4 I, not from reset); the bound is the project's for this chain, ATOL_F64_CHAIN = 1e-12."""
    from oracle import ekf_numpy
    K, E, phase2, phase3, X0, P0, single = small
    X, _, refs, fed, _ = _chunked(eng, phase2, phase3, K, X0, P0, _cuttings(E)["3"])
    worst, records = 0.0, 0
    for k in range(K):
        m2, m3 = phase2["types"][:, k] != synth.EV_NONE, phase3["types"][:, k] != synth.EV_NONE
        iv = fe.initial_values(phase2["types"][m2, k], phase2["values64"][m2, k], phase2["times"][m2, k], n_avg=N_AVG)
        assert iv["ready"] == fed.ready[k]
        if not iv["ready"]:
            continue
        g, dt, a, m = fe.run_frontend(phase3["types"][m3, k], phase3["values64"][m3, k], phase3["times"][m3, k],
                                      iv["acc"], iv["mag"], iv["t_init"])
        assert fed.total[k] == len(dt)
        if len(dt):
            Xo, _, _ = ekf_numpy.run_filter(g, dt.astype(np.float64), a, m, refs[k, :3], refs[k, 3:], X0=X0[k],
                                            P0=P0[k], record=False)
            worst = max(worst, float(np.abs(X[k] - Xo).max()))
            records += len(dt)
    print("chunked phone session vs the oracle chain: %.3e over %d records" % (worst, records))
    assert records > K and worst < ATOL_F64_CHAIN
