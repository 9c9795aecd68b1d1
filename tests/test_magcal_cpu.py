"""Phase 1 (the magnetometer calibration) without a GPU: the NumPy restatement (tests/magcal_numpy.py, k_magcal's
order of operations) against the reference's own results (tests/golden/magcal.npz, made by
tests/golden/make_magcal_golden.py), the ABI's argument checks (they return before any launch), and the
session's call sequence with and without a calibration."""
import ctypes
import os

import numpy as np
import pytest

from poseestimationkf_amd import synth, wire  # noqa: F401  (wire binds the real library before any fake is installed)

from . import magcal_numpy as mc
from .conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "magcal.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_shape_and_scale(golden):
    s = golden["samples"]
    assert s.shape == (48, 101, 3) and s.dtype == np.float32
    assert golden["bias"].shape == (48, 3) and golden["fit"].shape == (48, 6) and golden["fit_exact"].shape == (48, 6)
    assert np.abs(golden["bias"]).max() < 45.0          # offsets within +-40 (plus the cloud's own mean)
    assert 0 < golden["e_ref"] < 1e-13 and 0 < golden["w_ref"] < 1e-13
    # the reference's own solve agrees with the exact one to its measured error
    assert mc.fit_error(golden["fit"], golden["fit_exact"]).max() == golden["e_ref"]


def test_restatement_vs_the_reference(golden):
    """bias bit for bit the reference's computeBias; fit within 8 e_ref of the exact rational solution (the
    sequential sums and unpivoted Cholesky, and LAPACK's LU, each carry a different small multiple of n cond
    eps); W symmetric bit for bit and W W - R within 8 w_ref."""
    s = golden["samples"].astype(np.float64)               # (48, 101, 3)
    types = np.full((101, 48), synth.EV_MAG, np.uint32)
    got = mc.calibrate(types, s.transpose(1, 0, 2), n_cal=100)
    assert np.all(got["status"] == 0)
    assert np.array_equal(got["bias"].view(np.uint64), golden["bias"].view(np.uint64))
    e = mc.fit_error(got["fit"], golden["fit_exact"]).max()
    w = mc.root_residual(got["W"], mc.r_of(got["fit"])).max()
    print("restatement: fit error %.3e (e_ref %.3e), root residual %.3e (w_ref %.3e)"
          % (e, golden["e_ref"], w, golden["w_ref"]))
    assert e <= 8 * golden["e_ref"]
    assert np.array_equal(got["W"], got["W"].transpose(0, 2, 1))
    assert w <= 8 * golden["w_ref"]


def test_restatement_message_rule_and_degenerate_phones():
    """n_cal messages: not calibrated (the fit fires on message n_cal + 1); identical samples and a constant z
    (exact by construction: the centred coordinate is 0) give no quadric; +-h on the hyperboloid x^2 + y^2 -
    z^2 = 30^2 fits (1, 1, -1) / 900, which is no ellipsoid."""
    ev = synth.generate_calibration_events(6, 101, seed=5)
    vals = ev["values"].astype(np.float64)
    types = ev["types"].copy()
    types[100, 0] = synth.EV_NONE                              # phone 0: 100 messages only
    types[:, 1] = np.arange(101) % 4                           # phone 1: every message type counts
    vals[:, 2] = [12.5, -3.25, 40.0]                           # phone 2: never moved
    vals[:, 3, 2] = 17.0                                       # phone 3: a flat cloud
    vals[:, 4] = hyperboloid_samples(101)
    got = mc.calibrate(types, vals, n_cal=100)
    assert got["status"].tolist() == [1, 0, 2, 2, 3, 0]
    for k in (0, 2, 3, 4):
        assert np.all(got["bias"][k] == 0) and np.array_equal(got["W"][k], np.eye(3)) and np.isnan(got["fit"][k]).all()
    assert np.isfinite(got["fit"][[1, 5]]).all() and np.isfinite(got["W"]).all()
    h = vals[:100, 4][None]
    assert np.all(mc.bias_of(h) == 0.0)
    fit, spd = mc.cholesky_solve(*mc.normal_equations(h))
    assert spd[0] and np.abs(fit[0] * 900.0 - [1, 1, -1, 0, 0, 0]).max() < 1e-5


def hyperboloid_samples(n):
    """n float32-rounded samples +h_0, -h_0, +h_1, -h_1, ... on x^2 + y^2 - z^2 = 30^2: every pair sums to
    exactly 0, so the mean of an even count is exactly 0."""
    i = np.arange((n + 1) // 2)
    r = 30.0 + 30.0 * ((i * 0.618034) % 1.0)
    phi = 2.399963 * i
    z = np.sqrt(r * r - 900.0) * np.where(i % 3 == 0, -1.0, 1.0)
    h = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32).astype(np.float64)
    return np.stack([h, -h], axis=1).reshape(-1, 3)[:n]


def test_jacobi_rotation_edge_cases():
    """A zero off-diagonal skips its rotation; a tau that overflows gives t -> 0 (no NaN); equal diagonals
    rotate by 45 degrees."""
    R = np.array([np.diag([3.0, 2.0, 1.0]),
                  [[1.0, 1e-300, 0.0], [1e-300, 1e300, 0.0], [0.0, 0.0, 2.0]],
                  [[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 5.0]]])
    W, ok = mc.jacobi_root(R)
    assert ok.all() and np.isfinite(W).all()
    assert np.array_equal(W[0], np.diag(np.sqrt([3.0, 2.0, 1.0])))
    assert np.allclose(W[2] @ W[2], R[2], rtol=0, atol=1e-14)


# ------------------------------------------------------------------ the ABI's argument checks

@pytest.fixture(scope="module")
def lib():
    from poseestimationkf_amd import _lib
    return _lib


P = 4096  # a non-null, 16-byte aligned address; every call below returns before anything reads it


@pytest.mark.parametrize("args,msg", [
    ((-1, 8, P, 100, P, P, P, 0), "negative size"),
    ((8, -1, P, 100, P, P, P, 0), "negative size"),
    ((8, 8, P, 5, P, P, P, 0), "n_cal"),
    ((8, 1 << 30, P, 100, P, P, P, 0), "2^30"),
    ((8, 8, P, 100, P, P, P, 0x8), "unknown flags"),
    ((8, 8, P, 100, P, P, P, 0x2), "unknown flags"),      # PEKF_EV_F32_RECORDS means nothing here
    ((8, 8, None, 100, P, P, P, 0), "null pointer"),
    ((8, 8, P, 100, None, P, P, 0), "null pointer"),
    ((8, 8, P, 100, P, P, None, 0), "null pointer"),
    ((8, 8, P + 8, 100, P, P, P, 0x4), "misaligned"),
])
def test_magcal_arguments_are_checked(lib, args, msg):
    assert lib.lib.pekf_magcal_dev(*args, None) == lib.PEKF_ERR_INVALID
    assert msg in lib.last_error()


@pytest.mark.parametrize("args,msg", [
    ((-1, 8, P, P, P, 0), "negative size"),
    ((8, -1, P, P, P, 0), "negative size"),
    ((8, 1 << 30, P, P, P, 0), "2^30"),
    ((8, 8, P, P, P, 0x10), "unknown flags"),
    ((8, 8, None, P, P, 0), "null pointer"),
    ((8, 8, P, None, P, 0), "null pointer"),
    ((8, 8, P + 4, P, None, 0), "misaligned"),
])
def test_magcal_apply_arguments_are_checked(lib, args, msg):
    assert lib.lib.pekf_magcal_apply_dev(*args, None) == lib.PEKF_ERR_INVALID
    assert msg in lib.last_error()


def test_magcal_empty_batch_is_ok(lib):
    assert lib.lib.pekf_magcal_dev(0, 8, None, 100, None, None, None, 0, None) == lib.PEKF_OK
    assert lib.lib.pekf_magcal_apply_dev(0, 8, None, None, None, 0, None) == lib.PEKF_OK
    assert lib.lib.pekf_magcal_apply_dev(8, 0, None, None, None, 0, None) == lib.PEKF_OK   # no rows: nothing to do


# ------------------------------------------------------------------ the session's call sequence

def _recording_fake(monkeypatch):
    """tests/fake_libpekf.py's host fake with the session's three entry points recorded (they compute nothing)."""
    from . import fake_libpekf

    class Fake(fake_libpekf.FakeLib):
        def _rec(self, name):
            def f(*a):
                self.calls.append(name)
                return 0
            return f

        def __getattr__(self, name):
            if name in ("pekf_frontend_init_ext_dev", "pekf_live_ext_dev", "pekf_magcal_apply_dev",
                        "pekf_wire_events_ext_dev"):
                return self._rec(name)
            raise AttributeError("fake libpekf has no %s" % name)

    from poseestimationkf_amd import _lib, engine, shard
    fake = Fake(1)
    for mod in (_lib, engine, shard):
        monkeypatch.setattr(mod, "lib", fake)
    return fake, engine


def test_session_without_calibration_is_the_same_call_sequence(monkeypatch):
    """calibration=None: phase 2 then the fused phase 3, nothing else -- the launches of the session before
    phase 1 existed; with a calibration, one correction per plane goes before them."""
    fake, engine = _recording_fake(monkeypatch)
    K = 8
    ph2 = synth.generate_events(np.arange(K), 40, seed=1)
    ph3 = synth.generate_events(np.arange(K), 30, seed=2)
    for events in ("f32", "f64"):
        fake.calls.clear()
        out = engine.run_session(ph2, ph3, engine.BatchedEKF(K), events=events)
        assert fake.calls == ["pekf_frontend_init_ext_dev", "pekf_live_ext_dev"]
        assert sorted(out) == ["counts", "ready", "refs"]
    calib = dict(status=np.zeros(K, np.int32), calibrated=np.ones(K, bool), cal=engine.DeviceBuffer(96 * K),
                 status_dev=engine.DeviceBuffer(4 * K))
    fake.calls.clear()
    out = engine.run_session(ph2, ph3, engine.BatchedEKF(K), calibration=calib)
    assert fake.calls == ["pekf_magcal_apply_dev", "pekf_magcal_apply_dev", "pekf_frontend_init_ext_dev",
                          "pekf_live_ext_dev"]
    assert out["calibrated"].all() and sorted(out) == ["calibrated", "counts", "ready", "refs"]
    with pytest.raises(ValueError, match="calibration is of"):
        engine.run_session(ph2, ph3, engine.BatchedEKF(K), calibration=dict(calib, status=np.zeros(3, np.int32)))
    # the wire session: the parse, then the same
    frames = np.full((4, K, 100), ord(" "), np.uint8)
    fake.calls.clear()
    engine.run_wire_session(frames, engine.BatchedEKF(K), frame_rows=False)
    assert fake.calls == ["pekf_wire_events_ext_dev", "pekf_frontend_init_ext_dev", "pekf_live_ext_dev"]
    fake.calls.clear()
    out = engine.run_wire_session(frames, engine.BatchedEKF(K), frame_rows=False, calibration=calib)
    assert fake.calls == ["pekf_wire_events_ext_dev", "pekf_magcal_apply_dev", "pekf_magcal_apply_dev",
                          "pekf_frontend_init_ext_dev", "pekf_live_ext_dev"]
    assert out["calibrated"].all()


def test_generate_calibration_events_layout():
    ev = synth.generate_calibration_events(5, 101, seed=3)
    assert ev["types"].shape == (101, 5) and np.all(ev["types"] == synth.EV_MAG)
    assert ev["values"].shape == (101, 5, 3) and ev["values"].dtype == np.float32
    gaps = np.diff(np.concatenate([ev["t_init"][None], ev["times"]]), axis=0)
    assert gaps.min() >= 9_000_000 and gaps.max() <= 11_000_000
    assert np.abs(ev["hard"]).max() <= 40.0 and np.all(np.linalg.eigvalsh(ev["soft"]) > 0.69)
    again = synth.generate_calibration_events(5, 101, seed=3)
    assert np.array_equal(ev["values"], again["values"]) and np.array_equal(ev["times"], again["times"])
    # the samples are the distorted field: soft^-1 (m - hard) has the field's length to the noise
    u = np.einsum("kij,nkj->nki", np.linalg.inv(ev["soft"]), ev["values"] - ev["hard"][None])
    assert np.abs(np.linalg.norm(u, axis=2) - synth.B_UT).max() < 0.2
    p64 = synth.pack_events64(ev, ev["values"].astype(np.float64))
    assert p64.shape == (101, 5, 4) and ctypes.sizeof(ctypes.c_double) * 4 == p64.strides[1]
