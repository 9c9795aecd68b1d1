"""Wahba's closed form on the device (csrc/pekf_math.hpp make_frame, wahba_rotation, frame_degenerate,
wahba_rank1_rotation; behind k_op<OpWahba>, k_op<OpCorrect>, k_call1, the resident service, dropin/Wahba.py and
k_wahba_stream) against exact optima across pair geometry, weights and scale: the families of tests/wahba_families.py
-- pairs down to 1e-13 rad, weights down to 1e-12 and of either sign, vectors times 2^+-520, optima within 1e-6 of the
identity and 1e-4 of a half turn -- where kat.npz (pairs no thinner than 0.023 rad, unit vectors), edge.npz and the
exactly parallel pairs of test_degenerate_samples.py cannot see an error.  The conditions (the exact R and q of
tests/golden/wahba_families.npz, the error Y of the reference's own float64 statements against them, the family
maximum held to 8 Y on the IEEE routes and 8 (4.2e-15 / 2^-53) Y ~ 303 Y on the FAST one) come from the reference
quantities alone; tests/test_wahba_conditioning_cpu.py pins them and shows that the rule fails the closed form this
file was written against (frame_degenerate at 1e-12 |m|, vectors as given) on under_threshold and scale.

Shapes: 1308 items in one launch per operator (nine families x 32, rank1_by_weight's 16, parallels' 1004: five full
256-item blocks and one of 28), and the first 65 (a full wave and a one-lane tile).

Measured on MI355X: see test_rotation_and_quaternion_against_the_exact_optimum and test_wahba_stream."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from oracle import ekf_numpy as npo
from poseestimationkf_amd._lib import check, lib

from . import wahba_families as wf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = (0, 9, 17, 31)     # of each family, through the n = 1 routes
DROPIN = ("ExtendedKalmanFilter", "Wahba", "UtilityFunctions", "_bootstrap")


@pytest.fixture(scope="module")
def eng():
    from poseestimationkf_amd import engine
    from poseestimationkf_amd._lib import device_count
    assert device_count() > 0, "GPU tests need a HIP device"
    prev = engine.percall_mode()
    yield engine
    engine.percall_mode(prev)


@pytest.fixture(autouse=True)
def _mode_restored(eng):
    prev = eng.percall_mode()
    yield
    eng.percall_mode(prev)


@pytest.fixture(scope="module")
def g():
    return wf.golden()


@pytest.fixture(scope="module")
def batch():
    """The 1308 finite-B items side by side and {group: its rows} (shared, not modified)"""
    return wf.stacked()


@pytest.fixture(scope="module")
def launch(eng, batch):
    """One engine.wahba_rotation and one engine.wahba_quaternion call over all 1308 items (no LinAlgError: every
    status 0)"""
    cat, _ = batch
    args = [cat[k] for k in wf.FIELDS]
    return eng.wahba_rotation(*args), eng.wahba_quaternion(*args)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _wahba_dev(eng, fn, width, ops, n):
    """pekf_wahba_{rotation, quaternion}_dev with a status plane on the first n items -> rows, status"""
    bi = [eng.DeviceBuffer(a.nbytes).upload(a) for a in (np.ascontiguousarray(ops[k][:n], dtype=np.float64) for k in wf.FIELDS)]
    bo = eng.DeviceBuffer(8 * n * width)
    sb = eng.DeviceBuffer(4 * n).upload(np.full(n, -1, np.int32))
    check(fn(n, *[b.ptr for b in bi], bo.ptr, sb.ptr, None))
    check(lib.pekf_device_sync())
    return bo.download((n, width), np.float64), sb.download((n,), np.int32)


def test_rotation_and_quaternion_against_the_exact_optimum(batch, g, launch):
    """Per family: max |R - R_exact| <= 8 Y_R and the sign-insensitive max |q -+ q_e| <= 8 Y_q, Y the worst error of the
    reference's own np.linalg.svd statement on the family; and q carries the reference's sign on every item whose
    exact branch margin and w numerator pin it (262 of 288).
    Measured on MI355X, the device's worst error as a ratio to Y, next to the closed form as it stood on the same box
    (frame_degenerate at 1e-12 |m|, no scaling):
        family           Y_R       Y_q       device (R, q)      as it stood (R, q)
        ordinary         1.61e-15  2.55e-15  0.621    0.348     0.621    0.348
        thin_current     9.80e-5   4.15e-5   1.37     1.67      1.37     1.67
        thin_reference   7.52e-5   3.57e-5   1.53     0.797     1.53     0.797
        both_thin        2.72e-8   1.18e-8   1.3e-4   1.3e-3    1.3e-4   1.3e-3
        under_threshold  3.61e-3   2.27e-3   0.645    2.98      520      491
        filter_weights   9.85e-8   4.23e-8   0.194    0.207     0.194    0.207
        lopsided         4.41e-4   1.87e-4   1.5e-12  4.2e-12   1.5e-12  4.2e-12
        scale            1.65e-15  7.86e-16  0.539    3.67      not finite
        near_optimum     1.75e-15  2.05e-4   0.508    3.16      0.508    3.16
    The device fails where the restatement said it would and nowhere else; away from those two families the present
    form gives the former one's figures (the scaling is by exact powers of two).  k_correct on filter_weights: 0.175
    Y_q.  Exact parallels and zero weights: orthogonal to 1.3e-15, short of the optimum by at most 1.1e-15 sigma_1.
    """
    _, sl = batch
    R, q = launch
    n = 288
    eR, eq = wf.err_rotation(R[:n], g["f64_R"]), wf.err_quat(q[:n], g["f64_q"])
    for name in wf.NAMES:
        YR, Yq = wf.yard(g, "f64", sl[name])
        print("k_wahba %-16s Y_R %.2e Y_q %.2e: R %.3g Y_R, q %.3g Y_q" % (name, YR, Yq, eR[sl[name]].max() / YR, eq[sl[name]].max() / Yq))
    for name in wf.NAMES:
        YR, Yq = wf.yard(g, "f64", sl[name])
        assert wf.MARGIN * YR < wf.INFORMATIVE and wf.MARGIN * Yq < wf.INFORMATIVE
        assert eR[sl[name]].max() <= wf.MARGIN * YR, name
        assert eq[sl[name]].max() <= wf.MARGIN * Yq, name
    ok = wf.sign_qualifies(g, "f64")
    assert ok.sum() >= 0.9 * n and wf.same_sign(q[:n], g["f64_q_ref"])[ok].all()


def test_device_pointer_route_and_status(eng, batch, launch):
    """pekf_wahba_rotation_dev / pekf_wahba_quaternion_dev with a status plane on the same 1308 items and on the first
    65: bit for bit the host route's rows, every status 0 -- B is finite on the scale family too -- and every entry
    finite."""
    cat, sl = batch
    for fn, width, want in ((lib.pekf_wahba_rotation_dev, 9, launch[0]), (lib.pekf_wahba_quaternion_dev, 4, launch[1])):
        for n in (1308, 65):
            got, st = _wahba_dev(eng, fn, width, cat, n)
            assert not st.any(), {k: np.nonzero(st[s])[0] for k, s in sl.items() if st[s].any()}
            assert np.array_equal(_bits(got), _bits(want[:n]).reshape(n, width)) and np.isfinite(got).all()


def test_rank1_groups_take_the_shortest_arc(batch, launch):
    """Exactly parallel pairs (1000 random ones in either pair, test_degenerate_samples' CASES) and exactly zero
    weights: a proper rotation to 1e-12 that attains the optimum to 1e-12 sigma_1, as R and as q -- a parallel pair put
    through Gram-Schmidt would give an e2 of rounding noise and fail the first."""
    cat, sl = batch
    for name in ("parallels", "rank1_by_weight"):
        f = {k: cat[k][sl[name]] for k in wf.FIELDS}
        for Rx in (launch[0][sl[name]], wf.quat_rotm(launch[1][sl[name]])):
            orth, short = wf.optimum_shortfall(Rx, f)
            print("k_wahba %-16s orthogonal to %.2e, short of the optimum by %.2e sigma_1" % (name, orth.max(), np.abs(short).max()))
            assert orth.max() < 1e-12 and np.abs(short).max() < 1e-12, name
        assert np.abs(np.linalg.norm(launch[1][sl[name]], axis=1) - 1.0).max() < 1e-12


def test_overflowing_b_is_the_references_failure(eng):
    """Both pairs times 2^520: status 1 on exactly those items of a 65-item launch, LinAlgError through the engine and
    through both n = 1 routes."""
    cat, _ = wf.stacked()
    ops = {k: np.array(cat[k][:65]) for k in wf.FIELDS}
    over = wf.overflow()
    at = [0, 63, 64]
    for j, i in enumerate(at):
        for k in wf.FIELDS:
            ops[k][i] = over[k][j]
    hit = np.zeros(65, np.int32)
    hit[at] = 1
    for fn, width in ((lib.pekf_wahba_rotation_dev, 9), (lib.pekf_wahba_quaternion_dev, 4)):
        _, st = _wahba_dev(eng, fn, width, ops, 65)
        assert np.array_equal(st, hit)
    with pytest.raises(np.linalg.LinAlgError):
        eng.wahba_quaternion(*[ops[k] for k in wf.FIELDS])
    for mode in (eng.PERCALL_LAUNCH, eng.PERCALL_SERVICE):
        eng.percall_mode(mode)
        with pytest.raises(np.linalg.LinAlgError):
            eng.wahba_rotation(*[over[k][3] for k in wf.FIELDS])


def test_n1_routes_and_dropin_give_the_batched_rows(eng, batch, launch, monkeypatch):
    """Items 0, 9, 17 and 31 of every family and four parallels one at a time, through k_call1 (PERCALL_LAUNCH), the
    resident service (PERCALL_SERVICE) and dropin/Wahba.py's getRotation / getQuarternion: bit for bit the 1308-item
    launch's rows."""
    cat, sl = batch
    rows = [sl[name].start + j for name in wf.NAMES for j in SAMPLE] + [sl["parallels"].start + j for j in (0, 1, 1000, 1003)]
    for mode in (eng.PERCALL_LAUNCH, eng.PERCALL_SERVICE):
        eng.percall_mode(mode)
        for i in rows:
            args = [cat[k][i] for k in wf.FIELDS]
            assert np.array_equal(_bits(eng.wahba_rotation(*args)).reshape(-1), _bits(launch[0][i]).reshape(-1)), (mode, i)
            assert np.array_equal(_bits(eng.wahba_quaternion(*args)).reshape(-1), _bits(launch[1][i])), (mode, i)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "poseestimationkf_amd", "dropin"))
    for m in DROPIN:
        sys.modules.pop(m, None)
    from Wahba import Wahba
    for i in rows:
        w = Wahba(cat["acc0"][i], cat["mag0"][i])
        args = (cat["acc"][i], cat["mag"][i], cat["k_acc"][i], cat["k_mag"][i])
        assert np.array_equal(_bits(w.getRotation(*args)).reshape(-1), _bits(launch[0][i]).reshape(-1)), i
        assert np.array_equal(_bits(w.getQuarternion(*args)), _bits(launch[1][i])), i
    for m in DROPIN:
        sys.modules.pop(m, None)


def test_the_solve_inside_correct(eng, batch, g):
    """engine.correct with K = I and z = q_e: X = z + (Y - z) normalised is the measurement Y flipped towards z.
    Correction takes the weights |acc_z|, 1 - |acc_z| (ExtendedKalmanFilter.py:71), so filter_weights is the family whose
    exact optimum the fixture holds: X within 8 Y_q of q_e there, in z's hemisphere.  On every item X is the
    operator's own quaternion at those weights, normalised (a thin pair's frame is orthogonal only to its rounding
    over theta, and so is q's norm), to 16 u: 3 u of z + (Y - z), 3 u of each of the two norms and divisions, doubled.
    The first 65 and both n = 1 routes give the batched rows bit for bit."""
    cat, sl = batch
    keep = np.ones(288, bool)      # (Correction's own weight |acc_z| = 2^519 overflows B where the current pair is times 2^520)
    keep[sl["scale"]] = [k != "current +520" for k in wf.kinds("scale")]
    rows = np.nonzero(keep)[0]
    n = len(rows)
    eye = np.tile(np.eye(4), (n, 1, 1))
    ops = (cat["mag"][rows], cat["acc"][rows], g["f64_q"][rows], eye, eye, cat["acc0"][rows], cat["mag0"][rows])
    X, _ = eng.correct(*ops)
    ka = np.abs(cat["acc"][rows, 2])
    own = eng.wahba_quaternion(cat["acc0"][rows], cat["mag0"][rows], cat["acc"][rows], cat["mag"][rows], ka, 1.0 - ka)
    own /= np.linalg.norm(own, axis=1, keepdims=True)
    assert np.isfinite(X).all() and wf.err_quat(X, own).max() <= 16 * wf.U
    s = sl["filter_weights"]          # (before scale: the same rows of X)
    Yq = wf.yard(g, "f64", s)[1]
    e = np.abs(X[s] - g["f64_q"][s]).max(axis=1)
    print("k_correct filter_weights   q %.3g Y_q" % (e.max() / Yq))
    assert e.max() <= wf.MARGIN * Yq
    X65, _ = eng.correct(*[a[:65] for a in ops])
    assert np.array_equal(_bits(X65), _bits(X[:65]))
    with pytest.raises(np.linalg.LinAlgError):
        i = sl["scale"].start + wf.kinds("scale").index("current +520")
        eng.correct(cat["mag"][i], cat["acc"][i], g["f64_q"][i], np.eye(4), np.eye(4), cat["acc0"][i], cat["mag0"][i])
    for mode in (eng.PERCALL_LAUNCH, eng.PERCALL_SERVICE):
        eng.percall_mode(mode)
        for i in range(0, n, 16):
            assert np.array_equal(_bits(eng.correct(*[a[i] for a in ops])[0]).reshape(-1), _bits(X[i])), (mode, i)


def test_rotmat_to_quat_on_the_matrix_families(eng, g):
    """RotationMatrix2Quart alone (k_op<OpR2q>, and k_call1 for one item), on turns within 1e-6 of the identity and
    1e-4 of a half turn: within 8 Y of the same formula at 80 digits, Y the float64 reference formula's own error
    (1.6e-4 and 8e-17), and of the reference's sign."""
    for name, M in wf.matrices().items():
        Y = g["mat_%s_err" % name].max()
        q = eng.rotmat_to_quat(M)
        e = wf.err_quat(q, g["mat_%s_q" % name]).max()
        print("k_r2q %-14s Y_q %.2e: q %.3g Y_q" % (name, Y, e / Y))
        assert e <= wf.MARGIN * Y, name
        assert wf.same_sign(q, np.array([npo.rotm_to_quat(m) for m in M])).all()
        assert np.array_equal(_bits(eng.rotmat_to_quat(M[5])), _bits(q[5:6]))


# ------------------------------------------------------------------------------------------ k_wahba_stream (FAST)
def _stream(eng, kind, f):
    """Every item a filter column (its reference pair) with one record (its current pair); one launch per weight pair
    of f, each item's row taken from the launch of its own weights -> q (n, 4)"""
    n = len(f["acc"])
    if kind == "rec64":
        win = eng.RecordWindow64.from_arrays(np.zeros((1, n, 3)), np.ones((1, n)), f["acc"][None], f["mag"][None], f["acc0"], f["mag0"])
    else:
        am = np.concatenate([f["acc"], f["mag"][:, :1]], axis=1)[None].astype(np.float32)
        my = f["mag"][None, :, 1:].astype(np.float32)
        assert np.array_equal(am[0, :, :3].astype(np.float64), f["acc"]) and np.array_equal(my[0].astype(np.float64), f["mag"][:, 1:])
        win = eng.IMUWindow.from_planes(np.zeros((1, n, 4), np.float32), am, my, f["acc0"], f["mag0"])
    w = np.stack([f["k_acc"], f["k_mag"]], axis=1)
    out = np.full((n, 4), np.nan)
    for ka, km in np.unique(w, axis=0):
        rows = (w[:, 0] == ka) & (w[:, 1] == km)
        out[rows] = win.wahba_quaternions(k_acc=ka, k_mag=km)[0][rows]
    return out


@pytest.mark.parametrize("kind", ["rec64", "f32"])
def test_wahba_stream(eng, g, kind):
    """k_wahba_stream<RecordWindow64's record> on the float64 items of every family but scale, and k_wahba_stream<the
    40 B record> on the items rounded to float32: per family the sign-insensitive q error <= 303 Y_q, Y_q over the
    items the route is held to (under_threshold: 5e-13 alone, bound ~0.2), the reference's sign on the qualifying
    items.  Float32 items whose current pair the rounding made exactly parallel (those whose reference pair it made
    parallel have no frame and are not judged), and parallels()' /
    parallels32()'s current-pair items, take the rank-1 route: unit to 1e-10 and short of the optimum by less than
    1e-10 sigma_1 (test_degenerate_samples' bounds for this output).  The first 65 items alone give the same rows.
    Measured on MI355X, the worst q error as a ratio to Y_q (bound 303), FP64 record / 40 B record: ordinary 0.65 /
    1.26, thin_current 0.15 / 3.86, thin_reference 0.30 / 0.71, both_thin 1.5e-3 / 4.7e-4, under_threshold (5e-13, 21
    items, Y_q 8.5e-4) 0.28 / -, filter_weights 0.22 / -, lopsided 8.9e-12 / 9.6e-12, near_optimum 3.37 / 0.49;
    parallels unit to 1.2e-12 and short of the optimum by 1.0e-15 sigma_1.  With frame_degenerate at 1e-12 |m| the
    FP64 record's under_threshold stood at 1.06e3 Y_q (an error of 0.9): the only family that failed."""
    which, names = ("f64", wf.STREAM) if kind == "rec64" else ("f32", wf.F32)
    fam = wf.families() if kind == "rec64" else wf.families32()
    cat, sl = wf.side_by_side(fam, names)
    at = {n: wf.side_by_side(fam)[1][n] for n in names}      # the fixture's rows
    q = _stream(eng, kind, cat)
    rank1 = np.concatenate([g[which + "_rank1"][at[n]] for n in names])
    ref_par = wf.pair_parallel(cat["acc0"], cat["mag0"])     # (no frame: an unspecified q)
    assert rank1[ref_par].all() and np.isfinite(q[~ref_par]).all()
    ok = np.concatenate([wf.sign_qualifies(g, which)[at[n]] for n in names])
    q_ref = np.concatenate([g[which + "_q_ref"][at[n]] for n in names])
    for name in names:
        pick = wf.stream_pick(name) & ~rank1[sl[name]]
        Yq = wf.yard(g, which, at[name], pick)[1]
        e = wf.err_quat(q[sl[name]], g[which + "_q"][at[name]])[pick].max()
        print("k_wahba_stream %-5s %-16s %2d items, Y_q %.2e: q %.3g Y_q (bound %.3g)" % (kind, name, pick.sum(), Yq, e / Yq, wf.FAST_MARGIN))
        assert wf.FAST_MARGIN * Yq < wf.INFORMATIVE and e <= wf.FAST_MARGIN * Yq, name
        held = ok[sl[name]] & pick
        assert wf.same_sign(q[sl[name]], q_ref[sl[name]])[held].all(), name
    # the float32 items with an exactly parallel current pair: the rank-1 route
    cur = rank1 & ~ref_par
    if cur.any():
        short = wf.optimum_shortfall(wf.quat_rotm(q[cur]), {k: cat[k][cur] for k in wf.FIELDS})[1]
        assert np.abs(short).max() < 1e-10 and np.abs(np.linalg.norm(q[cur], axis=1) - 1.0).max() < 1e-10
    # a full wave and one lane more
    first = {k: cat[k][:65] for k in wf.FIELDS}
    assert np.array_equal(_bits(_stream(eng, kind, first)), _bits(q[:65]))
    # exact parallels
    if kind == "rec64":
        p = wf.parallels()
        par = {k: p[k][p["current"]] for k in wf.FIELDS}
    else:
        par = wf.parallels32()
    qp = _stream(eng, kind, par)
    short = wf.optimum_shortfall(wf.quat_rotm(qp), par)[1]
    print("k_wahba_stream %-5s parallels: %d items, |q| - 1 to %.2e, short of the optimum by %.2e sigma_1" % (
        kind, len(qp), np.abs(np.linalg.norm(qp, axis=1) - 1.0).max(), np.abs(short).max()))
    assert np.isfinite(qp).all() and np.abs(np.linalg.norm(qp, axis=1) - 1.0).max() < 1e-10 and np.abs(short).max() < 1e-10
