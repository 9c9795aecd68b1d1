"""The two halves of the fused record step that do not involve P, each isolated by a launch that silences the other
and held to exact results (tests/step_families.py, tests/golden/step_families.npz; tests/test_step_halves_cpu.py pins
the conditions and shows that they have teeth):

 - the propagation, rk4_closed / rk4_closed_w with state_norm2's snap (pekf_math.hpp, pekf_step.hpp): records with the
   missing-magnetometer bit are X = RK4(X), P = P-, so a run of them is the gyro chain through the fused kernels' own
   code (OmodMode, denormals flushed, X unnormalised between the loop's records).  P is only asked to be finite.
 - the measurement, wahba_product_ref + wahba_toward_from_product (loop form) and wahba_quat_toward(const Frame &)
   (plain form): with P0 = I, |w| = 2, q = 1 and r = 2^-70 the gain is one to 2^-69 and X is Wahba's flipped quaternion.
   Missing records in front keep P- >= I, so the judged record is the first with a measurement.  k_run<Rec64>'s lazy
   record cannot be isolated so (an FP64 record carries no missing flag: its first record is the eager one);
   tests/test_rec64.py's bit-identity with the 40 B launch covers it.

Bounds, from the reference's own error alone: the last X of a propagation item within 303 Y u of the exact chain on
every fused route, within 8 Y u on the per-call routes; the measurement's X within 303 Y_q of the exact q up to sign,
no item left out, and with the exact sign of q . z wherever |q . z| >= 0.2 (91 % of the items).

Shapes: one batch of all items of a set (295 propagation columns of 1 to 64 rows, 324 / 292 measurement columns: a full
block and a part of one), the set without the items judged apart (the neighbours keep their bits), and the first 65
columns alone.

Measured on MI355X: the worst error of a family as a ratio to its yardstick (every test prints its rows).
Propagation, in Y u (bound 303; 8 on the last row); Y (f32, f64 set) from the fixture:

    route                             ordinary tiny  roots huge  longdt back  offunit sparse chain
    Y                                 1.31     1.28  15.7  2.83  5.38   2.48  1.27    1.27   18.3   (f32)
                                      1.20     1.28  13.8  3.51  6.47   2.54  1.81    0.97   13.4   (f64)
    k_run, also with trajectory       1.53     1.57  0.956 0.729 1.86   0.806 2.37    1.57   0.314
    k_run, per-filter noise           the same bits
    k_run_one x 64                    1.53     1.57  0.968 2.83  2.79   1.61  82      1.57   5.78
    k_update x 64                     the same figures
    noise, one record x 64            1.91     1.76  0.956 0.729 1.86   1.21  1.97    1.74   0.928
    k_gyro_chain, 40 B and FP64 (f32) 1.53     1.57  0.976 1.77  2.05   0.806 1.58    0.784  0.437
    k_gyro_chain, FP64 records (f64)  0.831    1.57  1.13  0.854 0.927  1.18  2.21    1.00   0.671
    k_rk4, k_predict's z (f64)        0.831    0.783 1.27  0.782 1.40   0.788 1.10    1.00   0.745

offunit's 82 is the +-2.8e-14 kinds inside state_norm2's snap (1.4e-14 = 126 u, beside the rsqrt's own error); with the
snap at 1e-13 the restatement puts the -9e-14 kind of these routes at 4.5e-14 = 405 u = 316 Y u (Y = 1.27).  Measurement, in Y_q (bound 303):

    route                        ordinary thin_cur thin_ref flat    upright raw_units near_z  quarter near_opt mag_scale
    Y_q (f32)                    2.67e-15 1.63e-10 7.90e-11 3.32e-5 3.13e-13 4.45e-15 1.20e-8 5.37e-15 2.98e-4
    Y_q (f64)                    2.04e-15 7.78e-5  4.87e-5  8.35e-5 4.32e-10 1.08e-14 2.90e-8 6.24e-15 4.72e-4 2.51e-15
    f32: one-record, k_update    0.333    1.76     4.64     4.0e-11 5.9e-3  0.424     1.3e-7  0.290   4.4e-6
    f32: two rows, counts = 1    0.166    1.32     4.04     1.7e-11 2.8e-3  0.150     4.2e-8  0.155   6.1e-9
    f32: one record, noise       the same figures
    f32: two rows, one missing   the same figures
    f32: three rows, two missing 0.166    1.32     4.04     1.7e-11 2.8e-3  0.125     4.2e-8  0.155   6.1e-9
    f32: the same with noise     the same bits
    f64: one-record (Rec64)      0.218    0.128    0.315    5.3e-12 1.8e-6  0.062     2.1e-8  0.285   5.9e-9   0.221
    f64: two rows, counts = 1    the same figures (a one-record launch over FP64 records runs the loop form)
    f64: one record, noise       the same figures
    f64: k_update                0.334    0.311    0.389    1.9e-11 4.9e-6  0.175     2.2e-8  0.273   3.3e-6   0.774

No family failed on the measurement.  On flat, near_optimum and the f64 thin pairs the reference's own error is large
(303 Y_q is 0.01 to 0.14), so the rule says little there beyond "no wrong rotation": the device is 1e-6 to 1e-11 of Y_q.
"""
from __future__ import annotations

import numpy as np
import pytest

from poseestimationkf_amd import synth

from . import step_families as sf
from . import wahba_families as wf

pytestmark = pytest.mark.gpu

T0 = 2 ** 52        # the handle's clock: 64 steps of up to 2^46 ns either way stay exact in int64 and in float64


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    return engine


@pytest.fixture(scope="module")
def g():
    return sf.golden()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _refs(K):
    """an ordinary reference pair per column (the propagation does not read it; the kernels build its frame)"""
    rng = np.random.default_rng([sf.SEED, 3])
    return wf.pair(rng, rng.uniform(0.3, 1.3, K))


def _eye(K):
    return np.tile(np.eye(4), (K, 1, 1))


# ------------------------------------------------------------------------------------------ propagation
def _prop_batch(form, apart=True, cols=None):
    cat, sl = sf.prop_side_by_side(sf.prop_families(form), apart=apart)
    if cols is not None:
        cat = {k: v[:cols] for k, v in cat.items()}
    return cat, sl


def _prop_records(cat):
    """the batch as 64 rows of 40 B records, every one with the missing-magnetometer bit, its dt in the word or
    escaped to the side plane"""
    K = len(cat["n"])
    dt = np.ascontiguousarray(cat["dt"].T)
    esc = (dt < 0) | (dt > sf.DT_WORD_MAX)
    word = np.where(esc, synth.DT_ESCAPE, np.where(esc, 0, dt)).astype(np.uint32) | np.uint32(synth.MISSING_BIT)
    acc0, mag0 = _refs(K)
    gyro = np.ascontiguousarray(cat["gyro"].transpose(1, 0, 2)).astype(np.float32)
    acc = np.broadcast_to(acc0.astype(np.float32), (sf.CHAIN, K, 3))
    mag = np.broadcast_to(mag0.astype(np.float32), (sf.CHAIN, K, 3))
    return synth.Records(gyro, np.array(acc), np.array(mag), word, acc0, mag0, np.where(esc, dt, 0.0))


def _first_columns(rec, cols):
    """the first cols columns of a batch's records (the reference pairs are drawn for the whole batch)"""
    return synth.Records(rec.gyro[:, :cols], rec.acc[:, :cols], rec.mag[:, :cols], rec.dtw[:, :cols], rec.acc0[:cols],
                         rec.mag0[:cols], rec.dtx[:, :cols])


def _last(traj, n):
    """row n - 1 of each column of a (rows, K, 4) trajectory"""
    return traj[n - 1, np.arange(len(n))]


def _judge_prop(g, form, sl, X, margin, what):
    e = sf.err_state(X[:len(g["p_%s_X" % form])], g["p_%s_X" % form])
    r = {n: e[s].max() / (sf.prop_yard(g, form, s) * sf.U) for n, s in sl.items() if n != "apart"}
    print("%-34s %s" % (what + " (" + form + ")", " ".join("%s %.3g" % kv for kv in r.items())))
    bad = {n: v for n, v in r.items() if not v <= margin}
    assert not bad, (what, form, bad)
    if "apart" in sl:
        a, k = X[sl["apart"]], sf.PROP_APART_FINITE
        assert sf.err_state(a[:k], g["p_apart_X"][:k]).max() <= margin * sf.U, (what, a[:k])
        assert np.isnan(a[k:]).all(), (what, a[k:])


def _run_multi(eng, win, cat, traj, noise=False):
    K = len(cat["n"])
    ekf = eng.BatchedEKF(K, q=np.full(K, 1.0), r=np.full(K, 0.1)) if noise else eng.BatchedEKF(K)
    ekf.set_state(cat["X0"], _eye(K))
    tr = ekf.run(win, n_steps=sf.CHAIN, counts=cat["n"], want_traj=traj)
    X, P = ekf.get_state()
    if traj:    # the trajectory's row of an item's last record is its final X
        ok = np.isfinite(X).all(axis=1)
        assert np.array_equal(_bits(_last(tr, cat["n"])[ok]), _bits(X[ok])) and ok.sum() >= K - 4
    return X, P


def _run_single(eng, win, cat, noise=False):
    """64 launches of one record each (k_run_one; with per-filter noise the multi-record arithmetic for one record)"""
    K = len(cat["n"])
    ekf = eng.BatchedEKF(K, q=np.full(K, 1.0), r=np.full(K, 0.1)) if noise else eng.BatchedEKF(K)
    ekf.set_state(cat["X0"], _eye(K))
    for t in range(int(cat["n"].max())):
        ekf.run(win, n_steps=1, step0=t, counts=np.clip(cat["n"] - t, 0, 1))
    return ekf.get_state()


def test_propagation_through_the_fused_kernels(eng, g):
    """All-missing records over an IMUWindow with its dt side plane, the f32 set with the items judged apart last: one
    multi-record launch with and without trajectory, one-record launches, both again with per-filter noise.  Every
    family within 303 Y u on the last X; P finite; w = 0 and dt = 0 leave exactly representable states where they are
    (to the same bound); NaN, +-Inf and X0 = 0 give NaN in that filter alone -- the launch without them and the first
    65 columns alone give the other filters' bits."""
    cat, sl = _prop_batch("f32")
    win = eng.IMUWindow.from_records(_prop_records(cat))
    n_fam = sl["apart"].start
    out = {}
    for what, fn in (("k_run", lambda: _run_multi(eng, win, cat, False)),
                     ("k_run, trajectory", lambda: _run_multi(eng, win, cat, True)),
                     ("k_run_one x 64", lambda: _run_single(eng, win, cat)),
                     ("k_run noise", lambda: _run_multi(eng, win, cat, False, noise=True)),
                     ("k_run noise, one record x 64", lambda: _run_single(eng, win, cat, noise=True))):
        X, P = out[what] = fn()
        _judge_prop(g, "f32", sl, X, sf.FAST_MARGIN, what)
        assert np.isfinite(P[:n_fam]).all() and np.isfinite(P[sl["apart"]][:sf.PROP_APART_FINITE]).all(), what
    assert np.array_equal(_bits(out["k_run"][0][:n_fam]), _bits(out["k_run, trajectory"][0][:n_fam]))
    assert np.array_equal(_bits(out["k_run"][0][:n_fam]), _bits(out["k_run noise"][0][:n_fam]))
    for cols in (n_fam, 65):
        part, _ = _prop_batch("f32", cols=cols)
        pw = eng.IMUWindow.from_records(_first_columns(_prop_records(cat), cols))
        assert np.array_equal(_bits(_run_multi(eng, pw, part, False)[0]), _bits(out["k_run"][0][:cols])), cols
        assert np.array_equal(_bits(_run_single(eng, pw, part)[0]), _bits(out["k_run_one x 64"][0][:cols])), cols


def test_propagation_through_the_handle(eng, g):
    """FilterHandle.update(missing = 1), record after record (k_update): the X it returns after an item's last record.
    The handle has no counts: a column runs on through its padding (copies of its last record), whose X nothing reads
    and under which P- of the huge items overflows after a few dozen records -- so P is not asked to be finite on this
    route (a skip record's X = z does not read P).  The first 65 columns alone give the same bits."""
    cat, sl = _prop_batch("f32")
    rec = _prop_records(cat)

    def chain(cols):
        h = eng.FilterHandle(rec.acc0[:cols], rec.mag0[:cols], t0_ns=np.full(cols, T0, np.int64))
        h.set_state(cat["X0"][:cols], _eye(cols))
        t, rows = np.full(cols, T0, np.int64), []
        for l in range(sf.CHAIN):
            t = t + cat["dt"][:cols, l].astype(np.int64)
            rows.append(h.update(cat["gyro"][:cols, l], t, rec.acc0[:cols], rec.mag0[:cols], missing=np.ones(cols, np.uint8)))
        h.close()
        return _last(np.stack(rows), cat["n"][:cols])
    X = chain(len(cat["n"]))
    _judge_prop(g, "f32", sl, X, sf.FAST_MARGIN, "k_update x 64")
    assert np.array_equal(_bits(chain(65)), _bits(X[:65]))


def test_propagation_through_gyro_chain(eng, g):
    """IMUWindow.gyro_chain (f32 set) and RecordWindow64.gyro_chain (both sets) on the same items: k_gyro_chain's
    rk4_closed with no snap."""
    cat, sl = _prop_batch("f32")
    win = eng.IMUWindow.from_records(_prop_records(cat))
    _, tr = win.gyro_chain(q0=cat["X0"], want_traj=True)
    full = _last(tr, cat["n"])
    _judge_prop(g, "f32", sl, full, sf.FAST_MARGIN, "k_gyro_chain, 40 B records")
    _, tr = eng.IMUWindow.from_records(_first_columns(_prop_records(cat), 65)).gyro_chain(q0=cat["X0"][:65], want_traj=True)
    assert np.array_equal(_bits(_last(tr, cat["n"][:65])), _bits(full[:65]))
    for form in ("f32", "f64"):
        for cols in (None, 65):
            c64, s64 = _prop_batch(form, apart=False, cols=cols)
            K = len(c64["n"])
            a0, m0 = _refs(K)
            gy = c64["gyro"].transpose(1, 0, 2)
            w64 = eng.RecordWindow64.from_arrays(gy, c64["dt"].T, np.broadcast_to(a0, gy.shape), np.broadcast_to(m0, gy.shape), a0, m0)
            _, tr = w64.gyro_chain(q0=c64["X0"], want_traj=True)
            X = _last(tr, c64["n"])
            if cols is None:
                _judge_prop(g, form, s64, X, sf.FAST_MARGIN, "k_gyro_chain, FP64 records")
                whole = X
            else:
                assert np.array_equal(_bits(X), _bits(whole[:cols]))


def test_propagation_through_the_per_call_operators(eng, g):
    """engine.rk4 chained on the host and engine.predict's z on the f64 set (rk4_literal, the IEEE routes): 8 Y u."""
    cat, sl = _prop_batch("f64", apart=False)
    K = len(cat["n"])
    x, z = cat["X0"].copy(), cat["X0"].copy()
    Q, R = np.tile(np.eye(3), (K, 1, 1)), np.tile(0.1 * np.eye(4), (K, 1, 1))
    for l in range(sf.CHAIN):
        on = (l < cat["n"])[:, None]
        x = np.where(on, eng.rk4(x, cat["dt"][:, l], cat["gyro"][:, l]), x)
        z = np.where(on, eng.predict(cat["gyro"][:, l], cat["dt"][:, l], z, _eye(K), Q, R)[0], z)
    _judge_prop(g, "f64", sl, x, sf.MARGIN, "k_rk4 chained")
    _judge_prop(g, "f64", sl, z, sf.MARGIN, "k_predict's z chained")


# ------------------------------------------------------------------------------------------ measurement
def _meas_batch(form, cols=None):
    cat, sl = sf.meas_side_by_side(sf.meas_families(form))
    ap = sf.meas_apart()
    cat = {k: np.concatenate([cat[k], ap[k]]) for k in cat}
    sl["apart"] = slice(len(cat["acc"]) - len(sf.MEAS_APART), len(cat["acc"]))
    if cols is not None:
        cat = {k: v[:cols] for k, v in cat.items()}
    return cat, sl


def _meas_window(eng, cat, form, rows, lead_missing=True):
    """rows records a column, each the item's with the gain-one gyro sample and dt; lead_missing (40 B records only):
    those before the last carry the missing-magnetometer bit"""
    K = len(cat["acc"])
    shape = (rows, K, 3)
    gyro = np.broadcast_to(np.array(sf.GAIN_GYRO), shape)
    acc, mag = np.broadcast_to(cat["acc"], shape), np.broadcast_to(cat["mag"], shape)
    if form == "f64":
        return eng.RecordWindow64.from_arrays(gyro, np.full((rows, K), sf.GAIN_DT), acc, mag, cat["acc0"], cat["mag0"])
    word = np.full((rows, K), int(sf.GAIN_DT), np.uint32)
    if lead_missing:
        word[:-1] |= np.uint32(synth.MISSING_BIT)
    f32 = lambda a: np.array(a, dtype=np.float32)   # noqa: E731
    return eng.IMUWindow.from_records(synth.Records(f32(gyro), f32(acc), f32(mag), word, cat["acc0"], cat["mag0"]))


def _judge_meas(g, form, cat, sl, X, what):
    n = len(g["m_%s_q" % form])
    n = min(n, len(X))
    e = wf.err_quat(X[:n], g["m_%s_q" % form][:n])
    r = {k: e[s].max() / sf.meas_yard(g, form, s) for k, s in sl.items() if k != "apart" and s.stop <= n}
    print("%-34s %s" % (what + " (" + form + ")", " ".join("%s %.3g" % kv for kv in r.items())))
    bad = {k: v for k, v in r.items() if not v <= sf.FAST_MARGIN}
    assert not bad, (what, form, bad)
    ask = g["m_%s_qz" % form][:n] >= sf.SIGN_QZ
    assert np.array_equal(sf.sign_of(X[:n], g["m_%s_q" % form][:n])[ask], g["m_%s_sign" % form][:n][ask]), what
    assert np.abs(np.linalg.norm(X, axis=1) - 1).max() < 1e-13, what
    if sl["apart"].stop <= len(X):      # rank-1 B: a proper rotation that attains the optimum
        ap = {k: cat[k][sl["apart"]] for k in wf.FIELDS}
        orth, short = wf.optimum_shortfall(wf.quat_rotm(X[sl["apart"]]), ap)
        assert orth.max() < 1e-12 and np.abs(short).max() < 1e-12, (what, orth, short)


def _run_meas(eng, win, cat, rows, counts=None, noise=False):
    K = len(cat["acc"])
    r = sf.R_GAIN_ONE
    ekf = eng.BatchedEKF(K, q=np.full(K, 1.0), r=np.full(K, r)) if noise else eng.BatchedEKF(K, q=1.0, r=r)
    ekf.set_state(cat["X0"], _eye(K))
    ekf.run(win, n_steps=rows, counts=counts)
    return ekf.get_state()[0]


@pytest.mark.parametrize("form", ["f32", "f64"])
def test_measurement_at_gain_one(eng, g, form):
    """The f32 set over IMUWindow and the f64 set over RecordWindow64: a one-record launch; a two-row window with
    counts = 1 (the loop form's eager record); over 40 B records also two and three rows whose leading records are
    missing (the loop form's lazy record, either ping-pong half) and the same with per-filter noise; each within
    303 Y_q of the exact q up to sign, with the exact sign of q . z where |q . z| >= 0.2; the rank-1 items attain the
    optimum.  The first 65 columns alone give the same bits."""
    cat, sl = _meas_batch(form)
    K = len(cat["acc"])
    routes = [("one-record launch", 1, None, False), ("two rows, counts = 1", 2, np.ones(K, np.int32), False),
              ("one record, per-filter noise", 1, None, True)]
    if form == "f32":
        routes += [("two rows, one missing", 2, None, False), ("three rows, two missing", 3, None, False),
                   ("three rows, two missing, noise", 3, None, True)]
    got = {}
    for what, rows, counts, noise in routes:
        got[what] = _run_meas(eng, _meas_window(eng, cat, form, rows, counts is None), cat, rows, counts, noise)
        _judge_meas(g, form, cat, sl, got[what], what)
    part, _ = _meas_batch(form, cols=65)
    for what, rows, counts, noise in routes[:2] + routes[3:5]:
        X = _run_meas(eng, _meas_window(eng, part, form, rows, counts is None), part, rows,
                      None if counts is None else counts[:65], noise)
        assert np.array_equal(_bits(X), _bits(got[what][:65])), what
    if form == "f32":
        assert np.array_equal(_bits(got["three rows, two missing"]), _bits(got["three rows, two missing, noise"]))


@pytest.mark.parametrize("form", ["f32", "f64"])
def test_measurement_through_the_handle(eng, g, form):
    """FilterHandle.update at gain one (k_update, the plain form), both sets (the handle takes float64 samples); the
    first 65 columns alone give the same bits."""
    cat, sl = _meas_batch(form)

    def update(K):
        h = eng.FilterHandle(cat["acc0"][:K], cat["mag0"][:K], q=1.0, r=sf.R_GAIN_ONE, t0_ns=np.zeros(K, np.int64))
        h.set_state(cat["X0"][:K], _eye(K))
        X = h.update(np.tile(sf.GAIN_GYRO, (K, 1)), np.full(K, int(sf.GAIN_DT), np.int64), cat["acc"][:K], cat["mag"][:K])
        h.close()
        return X
    X = update(len(cat["acc"]))
    _judge_meas(g, form, cat, sl, X, "k_update")
    assert np.array_equal(_bits(update(65)), _bits(X[:65]))
