"""A live session fed in chunks (pekf_live_resume_dev, engine.LiveSession): however a session's events are cut
into launches, every output has the bits of the single launch.

The yardstick is the existing one-shot launch, whose kernels are not under test: BatchedEKF.run_events(...,
trajectory=True) -- final X and P, refs, counts, every trajectory row and its dt.  The chunked sessions feed row
ranges of one packed event plane (feed_planes) in several cuttings and must equal it and the session fed
everything as one chunk with np.array_equal; between chunks X[k] is the server's X_k of filter k's latest record.
Forms: the default FP64 records on f32 events, and FP64 events."""
import numpy as np
import pytest

from poseestimationkf_amd import synth

from .test_frontend import _events
from .test_live import ATOL_F64_CHAIN, _oracle_chain_f64
from .test_live_traj import BACKWARDS, CLOCK_STEPS, ESCAPED, _resumed

pytestmark = pytest.mark.gpu

SHAPES = [(64, 37, 22), (1000, 1500, 21)]   # a partial last wave, ragged counts, E no multiple of the 3-event ring
FORMS = ["f32", "f64"]                      # the session's event form (records are FP64 in both)


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


def _pack(eng, ev, form):
    if form == "f64":
        return synth.pack_events64(ev, eng.server_event_values(ev))
    return synth.pack_events(ev)


def _cuttings(E, seed=0):
    """name -> list of (first row, end row) covering 0 .. E"""
    def by(n):
        return [(a, min(a + n, E)) for a in range(0, E, n)]
    rng = np.random.default_rng(1000 + seed)
    sizes = [0]                                    # an empty first chunk
    while sum(sizes) < E:
        sizes.append(int(rng.integers(0, 98)))
        if len(sizes) == 2 or rng.random() < 0.2:
            sizes.append(0)                        # empty chunks between others
    sizes += [0]                                   # and an empty last one
    edges = np.minimum(np.cumsum([0] + sizes), E)
    out = {"2": by(2), "3": by(3), "4": by(4), "random": list(zip(edges[:-1], edges[1:]))}
    assert sum(a == b for a, b in out["random"]) >= 3
    if E <= 64:
        out["1"] = by(1)
    return out


class Collected:
    """What a session's chunks gave, put together: per filter the trajectory rows and dts in order"""

    def __init__(self, K, rows):
        self.traj, self.dt = np.full((rows, K, 4), np.nan), np.full((rows, K), np.nan)
        self.times = np.full((rows, K), np.nan)
        self.pos = np.zeros(K, np.int64)

    def add(self, counts, tj):
        assert counts.max(initial=0) <= len(tj["trajectory"])
        # nothing but a filter's own rows is written
        m = np.arange(len(tj["trajectory"]))[:, None] < counts[None, :]
        assert np.isnan(tj["trajectory"][~m]).all() and np.isnan(tj["record_dt_ns"][~m]).all()
        for r in range(int(counts.max(initial=0))):
            k = np.flatnonzero(counts > r)
            self.traj[self.pos[k] + r, k] = tj["trajectory"][r, k]
            self.dt[self.pos[k] + r, k] = tj["record_dt_ns"][r, k]
            self.times[self.pos[k] + r, k] = tj["record_times_ns"][r, k]
        self.pos += counts


def _chunked(eng, ev, form, cuts, K, between=None, X0=None, P0=None, planes=None, init=None):
    """The session over row ranges `cuts` of the packed plane -> (X, P, refs, total counts, Collected).
    between(session, filters, counts, X before, P before): called after every chunk with the state downloaded."""
    planes = _pack(eng, ev, form) if planes is None else planes
    E = planes.shape[0]
    buf = eng.DeviceBuffer(planes.nbytes).upload(planes)
    row = planes[0].nbytes if E else 0
    f = eng.BatchedEKF(K)
    if X0 is not None:
        f.set_state(X0, P0)
    ia, im = (ev["init_acc"], ev["init_mag"]) if init is None else init
    s = eng.LiveSession(f, ia, im, ev["t_init"], events=form)
    got = Collected(K, E // 3 + 1)
    Xb, Pb = f.get_state() if between else (None, None)
    for a, b in cuts:
        te = eng.EV_TIME_EVENTS if form == "f32" and a < b and synth.has_time_events(planes[a:b]) else 0
        counts, tj = s.feed_planes(buf, b - a, te, trajectory=True, offset=int(a) * row)
        got.add(counts, tj)
        if between:
            Xa, Pa = f.get_state()
            between(s, counts, (Xb, Pb), (Xa, Pa))
            Xb, Pb = Xa, Pa
    X, P = f.get_state()
    return X, P, s.refs, s.total_counts, got


def _one_launch(eng, ev, form, K, X0=None, P0=None):
    f = eng.BatchedEKF(K)
    if X0 is not None:
        f.set_state(X0, P0)
    counts, refs, tj = f.run_events(ev, events=form, trajectory=True)
    X, P = f.get_state()
    return X, P, refs, counts, tj


def _equals_one_launch(chunked, single, label=""):
    X, P, refs, total, got = chunked
    Xs, Ps, refs_s, counts_s, tj = single
    assert np.array_equal(total, counts_s), label
    assert np.array_equal(refs, refs_s, equal_nan=True), label   # (NaN: a filter whose init is not finite)
    assert np.array_equal(X, Xs, equal_nan=True) and np.array_equal(P, Ps, equal_nan=True), label
    R = min(len(got.traj), len(tj["trajectory"]))
    assert counts_s.max(initial=0) <= R
    assert np.array_equal(got.traj[:R], tj["trajectory"][:R], equal_nan=True), label
    assert np.array_equal(got.dt[:R], tj["record_dt_ns"][:R], equal_nan=True), label
    assert np.array_equal(got.times[:R], tj["record_times_ns"][:R], equal_nan=True), label
    assert np.isnan(got.traj[R:]).all() and np.isnan(tj["trajectory"][R:]).all()


@pytest.fixture(scope="module")
def singles(eng):
    """The one-shot launch on a generated stream, made once and left unchanged"""
    made = {}

    def get(form, K, E, seed):
        if (form, K, E, seed) not in made:
            ev = synth.generate_events(np.arange(K), E, seed=seed)
            made[form, K, E, seed] = ev, _one_launch(eng, ev, form, K)
        return made[form, K, E, seed]
    return get


# ------------------------------------------------------------------ 1, 2. any cutting; the pose between chunks

@pytest.mark.parametrize("K,E,seed", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_any_cutting_gives_the_single_launch(eng, singles, form, K, E, seed):
    ev, single = singles(form, K, E, seed)
    assert single[3].max() > 0 and len(set(single[3])) > 1
    traj_s, counts_s = single[4]["trajectory"], single[3]

    def between(s, counts, before, after):
        """X[k] is the server's X_k of filter k's latest record; without a record X[k] and P[k] stay"""
        tot = s.total_counts
        k = np.flatnonzero(counts > 0)
        assert np.array_equal(after[0][k], traj_s[tot[k] - 1, k])
        idle = counts == 0
        assert np.array_equal(after[0][idle], before[0][idle]) and np.array_equal(after[1][idle], before[1][idle])

    whole = _chunked(eng, ev, form, [(0, E)], K)
    _equals_one_launch(whole, single, "one chunk")
    for name, cuts in _cuttings(E, seed).items():
        # (at 1000 x 1500 the state is downloaded between chunks in the random cutting only: seconds, not minutes)
        chunked = _chunked(eng, ev, form, cuts, K, between if E <= 64 or name == "random" else None)
        _equals_one_launch(chunked, single, "chunks of " + name)
        _equals_one_launch(chunked, whole[:4] + (single[4],), "chunks of %s against one chunk" % name)
        assert np.array_equal(chunked[4].traj, whole[4].traj, equal_nan=True)
    assert counts_s.sum() == whole[3].sum()


def test_a_session_continues_a_given_filter_state(eng):
    """Not from reset: the first chunk starts from the BatchedEKF's X / P as the one-shot launch does"""
    K, E, seed = 64, 37, 22
    ev = synth.generate_events(np.arange(K), E, seed=seed)
    X0, P0 = _resumed(K, 45)
    for form in FORMS:
        single = _one_launch(eng, ev, form, K, X0, P0)
        _equals_one_launch(_chunked(eng, ev, form, _cuttings(E)["3"], K, X0=X0, P0=P0), single, form)


# ------------------------------------------------------------------ 3. clock edges across a boundary

@pytest.mark.parametrize("spec", [CLOCK_STEPS, BACKWARDS, ESCAPED * 5], ids=["clock steps", "backwards", "escaped"])
@pytest.mark.parametrize("form", FORMS)
def test_clock_edges_across_a_chunk_boundary(eng, form, spec):
    """Fed row by row, every time event and every escaped-dt record is a chunk's first and last row; each chunk's
    PEKF_EV_TIME_EVENTS flag says what that chunk holds."""
    K = 64
    ev = _events(K, spec)
    planes = _pack(eng, ev, form)
    E = planes.shape[0]
    if form == "f32":
        te = [synth.has_time_events(planes[e:e + 1]) for e in range(E)]
        assert not all(te) and (any(te) or len(spec) == 5 * len(ESCAPED))   # (escaped dts need no time event)
    single = _one_launch(eng, ev, form, K)
    assert single[3].min() > 0
    _equals_one_launch(_chunked(eng, ev, form, [(e, e + 1) for e in range(E)], K), single)
    _equals_one_launch(_chunked(eng, ev, form, _cuttings(E)["2"], K), single)


# ------------------------------------------------------------------ 4. never ready; no record

@pytest.mark.parametrize("form", FORMS)
def test_filters_that_never_got_ready_and_streams_without_records(eng, form):
    K, E, seed = 64, 37, 22
    ev = dict(synth.generate_events(np.arange(K), E, seed=seed))
    dead = np.arange(K) % 5 == 2                       # phase 2 never got ready: NaN init
    ev["init_acc"], ev["init_mag"] = ev["init_acc"].copy(), ev["init_mag"].copy()
    ev["init_acc"][dead] = np.nan
    ev["init_mag"][dead, 1] = np.nan
    ev["types"] = ev["types"].copy()
    mute = np.arange(K) % 7 == 3                       # no gyro sample: no record completes
    ev["types"][:, mute] = np.where(ev["types"][:, mute] == synth.EV_GYRO, synth.EV_ACC, ev["types"][:, mute])
    X0, P0 = _resumed(K, 46)
    single = _one_launch(eng, ev, form, K, X0, P0)
    none = dead | mute
    assert np.all(single[3][none] == 0) and single[3][~none].sum() > K

    def between(s, counts, before, after):
        assert np.all(counts[none] == 0) and np.all(s.total_counts[none] == 0)
        assert np.array_equal(after[0][none], X0[none]) and np.array_equal(after[1][none], P0[none])

    for name in ("1", "3", "random"):
        chunked = _chunked(eng, ev, form, _cuttings(E)[name], K, between, X0=X0, P0=P0)
        _equals_one_launch(chunked, single, name)
        assert np.isnan(chunked[4].traj[:, none]).all() and np.isnan(chunked[4].dt[:, none]).all()
        assert np.array_equal(chunked[0][none], X0[none]) and np.array_equal(chunked[1][none], P0[none])


# ------------------------------------------------------------------ 5. feed of dict chunks

def _ragged_clock(K, E, seed):
    """A generated stream where every third filter pauses for 2^31 ns and more and another third's clock steps
    back: with f32 events those filters need time events and the others get null padding beside them"""
    ev = dict(synth.generate_events(np.arange(K), E, seed=seed))
    t = ev["times"].copy()
    t[10:, 0::3] += (1 << 31) + 5
    t[20:, 1::3] -= 10_000_000
    t[29:, 0::3] += 3 << 31
    ev["times"] = t
    return ev


@pytest.mark.parametrize("form", FORMS)
def test_feed_of_dict_chunks_equals_feed_planes(eng, form):
    K, E, seed = 64, 37, 22
    ev = _ragged_clock(K, E, seed)
    single = _one_launch(eng, ev, form, K)
    planes = _pack(eng, ev, form)
    assert form == "f64" or planes.shape[0] > E
    by_planes = _chunked(eng, ev, form, _cuttings(planes.shape[0])["4"], K)
    _equals_one_launch(by_planes, single)
    f = eng.BatchedEKF(K)
    s = eng.LiveSession(f, ev["init_acc"], ev["init_mag"], ev["t_init"], events=form)
    got = Collected(K, E // 3 + 1)
    edges = [0, 5, 10, 11, 11, 20, 21, 30, E]          # cut at and beside the rows where the clocks step
    for a, b in zip(edges[:-1], edges[1:]):
        chunk = dict(types=ev["types"][a:b], values=ev["values"][a:b], times=ev["times"][a:b])
        counts, tj = s.feed(chunk, trajectory=True)
        got.add(counts, tj)
    X, P = f.get_state()
    _equals_one_launch((X, P, s.refs, s.total_counts, got), single)
    # without a trajectory: the same filter, counts only
    f2 = eng.BatchedEKF(K)
    s2 = eng.LiveSession(f2, ev["init_acc"], ev["init_mag"], ev["t_init"], events=form)
    total = sum(s2.feed(dict(types=ev["types"][a:b], values=ev["values"][a:b], times=ev["times"][a:b]))
                for a, b in zip(edges[:-1], edges[1:]))
    assert np.array_equal(total, single[3]) and np.array_equal(s2.total_counts, single[3])
    assert np.array_equal(f2.get_state()[0], single[0]) and np.array_equal(f2.get_state()[1], single[1])


# ------------------------------------------------------------------ 6. snapshot / restore

@pytest.mark.parametrize("form", FORMS)
def test_snapshot_and_restore_continue_the_session(eng, form):
    K, E, seed = 64, 37, 22
    ev = synth.generate_events(np.arange(K), E, seed=seed)
    single = _one_launch(eng, ev, form, K)
    planes = _pack(eng, ev, form)
    buf = eng.DeviceBuffer(planes.nbytes).upload(planes)
    row = planes[0].nbytes
    f = eng.BatchedEKF(K)
    s = eng.LiveSession(f, ev["init_acc"], ev["init_mag"], ev["t_init"], events=form)
    got = Collected(K, E // 3 + 1)
    got.add(*s.feed_planes(buf, 17, trajectory=True))
    snap = s.snapshot()
    assert snap["state"].dtype == np.uint8 and snap["state"].nbytes == (336 if form == "f64" else 288) * K
    f.set_state(*_resumed(K, 47))                          # the old filters go their own way
    s.feed_planes(buf, 5, offset=17 * row)
    f2 = eng.BatchedEKF(K)
    s2 = eng.LiveSession.restore(f2, snap)
    assert np.array_equal(s2.total_counts, got.pos)
    got.add(*s2.feed_planes(buf, 9, trajectory=True, offset=17 * row))
    got.add(*s2.feed_planes(buf, E - 26, trajectory=True, offset=26 * row))
    X, P = f2.get_state()
    _equals_one_launch((X, P, s2.refs, s2.total_counts, got), single)


# ------------------------------------------------------------------ 7. the oracle chain

@pytest.mark.parametrize("form", FORMS)
def test_chunked_session_follows_the_oracle_chain(eng, form):
    """Every filter of (64, 37, 22), fed in chunks of 3, against ekf_numpy.run_filter on the restatement's records
    (FP64 events: fed the server's own values); the worst distance is printed: 2.7e-14 (f32 events) and 2.8e-14
    (FP64 events) on an MI355X, against the bound of 1e-12."""
    K, E, seed = 64, 37, 22
    ev = synth.generate_events(np.arange(K), E, seed=seed)
    X, _, refs, total, _ = _chunked(eng, ev, form, _cuttings(E)["3"], K)
    worst = 0.0
    for k in range(K):
        Xo, n = _oracle_chain_f64(ev, k, refs, server=form == "f64")
        assert total[k] == n
        if n:
            worst = max(worst, float(np.abs(X[k] - Xo).max()))
    print("chunked session (%s events) vs the oracle chain: %.3e" % (form, worst))
    assert worst < ATOL_F64_CHAIN
