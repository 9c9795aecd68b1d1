"""Per-filter noise: q and r per filter through the fused kernels (engine.BatchedEKF with array q / r:
pekf_run_noise_dev, pekf_run_rec64_noise_dev, pekf_live_resume_noise_dev, pekf_live_join_noise_dev).

The yardstick is the scalar path, whose kernels are not under test and which is pinned to the oracle at these
noise scales (tests/test_gpu_parity.py::test_fused_run_other_noise_scales): a filter whose pair is (q, r) gets
what a scalar BatchedEKF(q, r) gives it, bit for bit, so almost every check needs no tolerance.  The four pairs
are the ones that test runs at, dealt to the columns as b % 4.

k_run: K = 321 filters (one full block, one full wave and one lane: a short last block), W = 24 records of
synth.generate(np.arange(K), W, seed=17, missing=True).  Sessions: 70 phones x 100 rows, the session tests' size
(one wave and a 6-lane tail)."""
import numpy as np
import pytest

from poseestimationkf_amd import synth

from .test_gpu_parity import PREC_GUARD
from .test_live_resume import Collected
from .test_live_traj import _resumed
from .test_long_gaps import with_dts
from .test_phone_session import N_AVG, Fed, _planes_of

pytestmark = pytest.mark.gpu

PAIRS = [(1.0, 0.1), (0.37, 2.5), (4.0, 0.01), (1e-3, 1.0)]
K, W = 321, 24
DEAL = np.arange(K) % 4
KS, ES = 70, 100                      # the sessions
DEAL_S = np.arange(KS) % 4


def _noise(deal):
    pairs = np.array(PAIRS)
    return pairs[deal, 0].copy(), pairs[deal, 1].copy()


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


@pytest.fixture(scope="module")
def rec():
    return synth.generate(np.arange(K), W, seed=17, missing=True)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, cols=slice(None), axis=0):
    """bit for bit, NaNs included, on the columns `cols` of axis `axis`"""
    n = a.shape[axis]
    a, b = np.take(_bits(a), np.arange(n)[cols], axis=axis), np.take(_bits(b), np.arange(n)[cols], axis=axis)
    return a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------ k_run

def _window(eng, rec, kind):
    if kind == "rec64":
        return eng.RecordWindow64.from_arrays(rec.gyro.astype(np.float64), rec.dt_ns, rec.acc.astype(np.float64),
                                              rec.mag.astype(np.float64), rec.acc0, rec.mag0)
    if kind == "dtx":                 # one escaped dt: the window gets its dt side plane
        dt = rec.dt_ns.copy()
        dt[7, 100] = 5e9
        win = eng.IMUWindow.from_records(with_dts(rec, dt))
        assert win.dtx is not None
        return win
    return eng.IMUWindow.from_records(rec)


COUNTS = (np.arange(K) * 7) % (W + 1)
COUNTS[[0, 65]], COUNTS[[1, 320]] = 0, W
assert set(COUNTS) >= {0, 1, W - 1, W}

# case -> (window kind, the launches as (n_steps, step0, want_traj), counts)
CASES = {
    "traj": ("f32", [(W, 0, True)], None),
    "no traj": ("f32", [(W, 0, False)], None),
    "counts, traj": ("f32", [(W, 0, True)], COUNTS),
    "counts": ("f32", [(W, 0, False)], COUNTS),
    "two launches": ("f32", [(10, 0, False), (14, 10, False)], None),
    "two launches, traj": ("f32", [(10, 0, True), (14, 10, True)], None),
    "escaped dt": ("dtx", [(W, 0, False)], None),
    "escaped dt, traj, counts": ("dtx", [(W, 0, True)], COUNTS),
    "rec64": ("rec64", [(W, 0, False)], None),
    "rec64, traj": ("rec64", [(W, 0, True)], None),
    "rec64, counts": ("rec64", [(W, 0, False)], COUNTS),
    "rec64, counts, traj": ("rec64", [(10, 0, True), (14, 10, True)], COUNTS),
}


def _run(eng, rec, case, q, r):
    """-> (X, P, the launches' trajectory rows stacked or None)"""
    kind, launches, counts = CASES[case]
    win = _window(eng, rec, kind)
    f = eng.BatchedEKF(K, q=q, r=r)
    rows = []
    for n, step0, traj in launches:
        c = None if counts is None else np.clip(counts - step0, 0, n)
        out = f.run(win, n_steps=n, step0=step0, want_traj=traj, counts=c)
        if traj:
            assert out.shape == (n, K, 4)
            rows.append(out)
    X, P = f.get_state()
    return X, P, np.concatenate(rows) if rows else None


@pytest.fixture(scope="module")
def scalar(eng, rec):
    """case -> the four scalar runs, one per pair, made once"""
    made = {}

    def get(case):
        if case not in made:
            made[case] = [_run(eng, rec, case, q, r) for q, r in PAIRS]
        return made[case]
    return get


@pytest.mark.parametrize("case", list(CASES))
def test_k_run_equals_the_scalar_launches_column_by_column(eng, rec, scalar, case):
    q, r = _noise(DEAL)
    X, P, tr = _run(eng, rec, case, q, r)
    assert np.isfinite(X).all() and np.isfinite(P).all()
    for p, (Xs, Ps, ts) in enumerate(scalar(case)):
        cols = DEAL == p
        assert _same(X, Xs, cols) and _same(P, Ps, cols), (case, PAIRS[p])
        assert (tr is None) == (ts is None)
        if tr is not None:
            assert _same(tr, ts, cols, axis=1), (case, PAIRS[p])
    # (the pairs do differ: a column run with another pair's noise is another filter)
    assert not _same(scalar(case)[0][0], scalar(case)[1][0])


def test_per_filter_run_against_the_oracle(eng, rec, oracle_c):
    """The per-filter run directly against the C oracle, pair by pair on its columns, to the bounds
    test_fused_run_other_noise_scales holds the scalar kernel to at these pairs."""
    q, r = _noise(DEAL)
    X, P, tr = _run(eng, rec, "traj", q, r)
    for p, (qp, rp) in enumerate(PAIRS):
        cols = DEAL == p
        Xo, Po, to = oracle_c.run(rec, q=qp, r=rp, want_traj=True)
        et = float(np.abs(tr.transpose(1, 0, 2)[cols] - to[cols]).max())
        ep = float(np.abs(P[cols] - Po[cols]).max())
        print("pair %s: trajectory %.3e, P %.3e" % ((qp, rp), et, ep))
        assert et < PREC_GUARD
        assert ep < PREC_GUARD * max(1.0, rp)
    assert np.abs(np.linalg.norm(X, axis=1) - 1.0).max() < 1e-13


def test_a_uniform_plane_is_the_scalar_launch(eng, rec, scalar):
    assert PAIRS[0] == (1.0, 0.1)
    for case in ("traj", "no traj"):
        X, P, tr = _run(eng, rec, case, np.full(K, 1.0), np.full(K, 0.1))
        Xs, Ps, ts = scalar(case)[0]
        assert _same(X, Xs) and _same(P, Ps)
        # ... which is BatchedEKF(K) itself, the default noise
        f = eng.BatchedEKF(K)
        trd = f.run(_window(eng, rec, "f32"), want_traj=ts is not None)
        Xd, Pd = f.get_state()
        assert _same(X, Xd) and _same(P, Pd)
        if ts is not None:
            assert _same(tr, ts) and _same(tr, trd)


def test_lanes_do_not_see_each_other(eng, rec, scalar):
    changed = np.array([0, 63, 64, 255, 256, 320])        # a wave's and a block's first and last lanes, the last lane
    deal = DEAL.copy()
    deal[changed] = (DEAL[changed] + 1) % 4
    for case in ("traj", "no traj"):
        X, P, _ = _run(eng, rec, case, *_noise(DEAL))
        X2, P2, _ = _run(eng, rec, case, *_noise(deal))
        others = np.setdiff1d(np.arange(K), changed)
        assert _same(X, X2, others) and _same(P, P2, others)
        for k in changed:
            Xs, Ps, _ = scalar(case)[deal[k]]
            assert _same(X2, Xs, [k]) and _same(P2, Ps, [k]) and not _same(X2, X, [k])


def test_set_noise_on_the_run_path(eng, rec, scalar):
    """BatchedEKF.set_noise between two launches: P is stored plain between launches, so the second launch runs
    those columns with their new pair -- a scalar filter of the old pair for 10 records, then, from that state, a
    scalar filter of the new pair"""
    win = _window(eng, rec, "f32")
    f = eng.BatchedEKF(K, *_noise(DEAL))
    f.run(win, n_steps=10)
    cols = np.array([2, 64, 320])
    new = (DEAL[cols] + 2) % 4
    f.set_noise(cols, *_noise(new))
    f.run(win, n_steps=14, step0=10)
    X, P = f.get_state()
    others = np.setdiff1d(np.arange(K), cols)
    for p, (Xs, Ps, _) in enumerate(scalar("two launches")):
        assert _same(X, Xs, others[DEAL[others] == p]) and _same(P, Ps, others[DEAL[others] == p])
    for k, pn in zip(cols, new):
        a = eng.BatchedEKF(K, *PAIRS[DEAL[k]])
        a.run(win, n_steps=10)
        b = eng.BatchedEKF(K, *PAIRS[pn])
        b.set_state(*a.get_state())
        b.run(win, n_steps=14, step0=10)
        Xb, Pb = b.get_state()
        assert _same(X, Xb, [k]) and _same(P, Pb, [k])


# ------------------------------------------------------------------ LiveSession

def _ev_rows(ev, a, b):
    return {key: ev[key][a:b] for key in ("types", "values", "values64", "times") if key in ev}


def _by(n, E):
    return [(a, min(a + n, E)) for a in range(0, E, n)]


def _live(eng, ev, form, q, r, cuts, X0, P0):
    f = eng.BatchedEKF(KS, q=q, r=r)
    f.set_state(X0, P0)
    s = eng.LiveSession(f, ev["init_acc"], ev["init_mag"], ev["t_init"], events=form)
    got = Collected(KS, ES // 3 + 2)
    for a, b in cuts:
        got.add(*s.feed(_ev_rows(ev, a, b), trajectory=True))
    X, P = f.get_state()
    return dict(X=X, P=P, refs=s.refs, total=s.total_counts, traj=got.traj, dt=got.dt, times=got.times)


def _sessions_equal(got, want, cols, label):
    for key in ("X", "P", "refs", "total"):
        assert _same(got[key], want[key], cols), "%s: %s" % (label, key)
    for key in ("traj", "dt", "times"):
        assert _same(got[key], want[key], cols, axis=1), "%s: %s" % (label, key)


@pytest.mark.parametrize("form", ["f32", "f64"])
def test_live_session(eng, form):
    ev = synth.generate_events(np.arange(KS), ES, seed=29)
    X0, P0 = _resumed(KS, 31)
    q, r = _noise(DEAL_S)
    one = _live(eng, ev, form, q, r, [(0, ES)], X0, P0)
    threes = _live(eng, ev, form, q, r, _by(3, ES), X0, P0)
    _sessions_equal(threes, one, slice(None), "chunks of 3 against one chunk")
    assert one["total"].min() > 5 and np.isfinite(one["X"]).all()
    for p, (qp, rp) in enumerate(PAIRS):
        want = _live(eng, ev, form, qp, rp, [(0, ES)], X0, P0)
        _sessions_equal(one, want, DEAL_S == p, "pair %s" % ((qp, rp),))
        other = DEAL_S == (p + 1) % 4
        assert not _same(one["X"], want["X"], other)


# ------------------------------------------------------------------ PhoneSession

def _phone(eng, phase2, phase3, q, r, cuts, t_start, X0=None, P0=None, at=None, feds=None):
    """A PhoneSession on BatchedEKF(KS, q, r) fed the row ranges `cuts`; at: {row: f(session, filters) -> None or
    (session, filters) to go on with}, called before the chunk that starts at that row"""
    f = eng.BatchedEKF(KS, q=q, r=r)
    if X0 is not None:
        f.set_state(X0, P0)
    s = eng.PhoneSession(f, n_avg=N_AVG, t_start=t_start)
    rows = phase3["types"].shape[0] // 3 + 2
    fed = Fed(KS, rows)
    feds = dict(feds or {})
    for a, b in cuts:
        if at and a in at:
            s, f = at[a](s, f) or (s, f)
        out = s.feed(_ev_rows(phase2, a, b), _ev_rows(phase3, a, b), trajectory=True)
        fed.add(out)
        for row, extra in feds.items():
            if a >= row:
                extra.add(out)
    X, P = f.get_state()
    assert np.array_equal(s.total_counts >= 0, np.ones(KS, bool))
    return dict(X=X, P=P, refs=s.refs, total=fed.total.copy(), ready=fed.ready.astype(np.int32), traj=fed.got.traj,
                dt=fed.got.dt, times=fed.got.times)


def _phones_equal(got, want, cols, label):
    _sessions_equal(got, want, cols, label)
    assert _same(got["ready"], want["ready"], cols), label


@pytest.fixture(scope="module")
def phones(eng):
    """The 70 x 100 session of tests/test_phone_session.py and the per-filter-noise session over it in chunks of 3"""
    phase2, phase3 = _planes_of(KS, ES, 41)
    X0, P0 = _resumed(KS, 48)
    q, r = _noise(DEAL_S)
    threes = _phone(eng, phase2, phase3, q, r, _by(3, ES), phase2["t_init"], X0, P0)
    return dict(phase2=phase2, phase3=phase3, X0=X0, P0=P0, q=q, r=r, threes=threes)


def test_phone_session(eng, phones):
    w = phones
    phase2, phase3, X0, P0 = w["phase2"], w["phase3"], w["X0"], w["P0"]
    threes = w["threes"]
    one = _phone(eng, phase2, phase3, w["q"], w["r"], [(0, ES)], phase2["t_init"], X0, P0)
    _phones_equal(threes, one, slice(None), "chunks of 3 against one chunk")
    ready = threes["ready"].astype(bool)
    assert 0 < ready.sum() < KS and (threes["total"][ready] > 0).sum() > KS // 2
    # phones join in different chunks
    first3 = np.argmax(phase3["types"] != synth.EV_NONE, axis=0)
    assert len(set(first3[ready & (threes["total"] > 0)] // 3)) > 8
    for p, (qp, rp) in enumerate(PAIRS):
        want = _phone(eng, phase2, phase3, qp, rp, [(0, 40), (40, ES)], phase2["t_init"], X0, P0)
        cols = DEAL_S == p
        assert (want["total"][cols] > 0).sum() > 5
        _phones_equal(threes, want, cols, "pair %s" % ((qp, rp),))
        moved = (DEAL_S == (p + 1) % 4) & (threes["total"] > 0)
        assert not _same(threes["X"], want["X"], moved)


def _padded(ev, rows):
    """the planes with `rows` rows more in which no phone has a message"""
    E = ev["types"].shape[0]
    out = dict(types=np.concatenate([ev["types"], np.full((rows, KS), synth.EV_NONE, np.uint32)]),
               times=np.concatenate([ev["times"], np.repeat(ev["times"][-1:], rows, axis=0)]))
    for key in ("values", "values64"):
        out[key] = np.concatenate([ev[key], np.zeros((rows,) + ev[key].shape[1:], ev[key].dtype)])
    assert out["types"].shape[0] == E + rows
    return out


def test_recycle_with_new_noise(eng, phones):
    w = phones
    R, G2 = 99, ES                      # the recycle's row, a boundary of the chunks of 3; the rows after it
    T = R + G2
    cols = np.array([64, 3])            # unsorted; pairs 0 and 3 ...
    new = np.array([2, 1])              # ... become pairs 2 and 1
    assert all(DEAL_S[cols] != new)
    qn, rn = _noise(new)
    g1 = [_padded(ph, T - ES) for ph in (w["phase2"], w["phase3"])]
    g2 = _planes_of(KS, G2, 43)
    mixed = []
    for a, b in zip(g1, g2):
        m = {key: a[key].copy() for key in a}
        for key in m:
            m[key][R:, cols] = b[key][:, cols]
        mixed.append(m)
    t_new = g2[0]["t_init"][cols]
    X0, P0 = w["X0"], w["P0"]

    def recycle(s, f):
        assert s.total_counts[cols].min() > 0           # both phones had joined and applied records
        assert s.recycle(cols, t_start=t_new, q=qn, r=rn) is None
        assert np.array_equal(f.q[cols], qn) and np.array_equal(f.r[cols], rn)
        plane = f.noise.download((KS, 2), np.float64)
        assert np.array_equal(plane, np.stack([f.q, f.r], axis=1))

    post = Fed(KS, T // 3 + 2)
    A = _phone(eng, mixed[0], mixed[1], w["q"], w["r"], _by(3, T), w["phase2"]["t_init"], X0, P0, at={R: recycle},
               feds={R: post})
    # every other column: the run without the recycle
    B = _phone(eng, g1[0], g1[1], w["q"], w["r"], _by(3, T), w["phase2"]["t_init"], X0, P0)
    others = np.setdiff1d(np.arange(KS), cols)
    _phones_equal(A, B, others, "not recycled")
    _phones_equal(B, dict(w["threes"], traj=B["traj"], dt=B["dt"], times=B["times"]), slice(None), "padding")
    # the recycled columns: a new scalar session at the new pair fed the rows after R, bit for bit
    tD = np.zeros(KS, np.int64)
    tD[cols] = t_new
    for k, pn in zip(cols, new):
        qp, rp = PAIRS[pn]
        postD = Fed(KS, T // 3 + 2)
        D = _phone(eng, _ev_rows(mixed[0], R, T), _ev_rows(mixed[1], R, T), qp, rp, _by(3, G2), tD, feds={0: postD})
        assert D["total"][k] > 2 and D["ready"][k]
        got = dict(A, total=post.total, traj=post.got.traj, dt=post.got.dt, times=post.got.times)
        want = dict(D, total=postD.total, traj=postD.got.traj, dt=postD.got.dt, times=postD.got.times)
        _phones_equal(got, want, [k], "recycled column %d" % k)
        # ... and not with the pair it had
        old = _phone(eng, _ev_rows(mixed[0], R, T), _ev_rows(mixed[1], R, T), *PAIRS[DEAL_S[k]], _by(3, G2), tD)
        assert not _same(A["X"], old["X"], [k])


def test_snapshot_and_restore(eng, phones):
    w = phones
    phase2, phase3, X0, P0 = w["phase2"], w["phase3"], w["X0"], w["P0"]
    cut = 51
    box = {}

    def move(s, f):
        snap = s.snapshot()
        assert np.array_equal(snap["q"], w["q"]) and np.array_equal(snap["r"], w["r"])
        assert snap["q"] is not f.q
        # onto other arrays, or scalars: refused
        for q, r in ((w["q"][::-1].copy(), w["r"][::-1].copy()), (w["q"], np.roll(w["r"], 1)), (1.0, 0.1)):
            with pytest.raises(ValueError, match="batch, q and r"):
                eng.PhoneSession.restore(eng.BatchedEKF(KS, q=q, r=r), snap)
        f2 = eng.BatchedEKF(KS, q=w["q"].copy(), r=w["r"].copy())
        s2 = eng.PhoneSession.restore(f2, snap)
        box["moved"] = s2 is not s and f2 is not f
        return s2, f2

    got = _phone(eng, phase2, phase3, w["q"], w["r"], _by(3, ES), phase2["t_init"], X0, P0, at={cut: move})
    assert box["moved"] and cut in [a for a, _ in _by(3, ES)]
    _phones_equal(got, w["threes"], slice(None), "restored")
