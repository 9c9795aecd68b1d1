"""Per-record trajectories from the fused live launch (pekf_live_traj_dev), the parts a CPU can check: the
entry is declared, bound and exported; its trajectory arguments are refused before any device call; the
engine's row count and record times."""
import re

import numpy as np
import pytest

from .test_capi import HEADER

P = 16  # a non-null, 16-byte aligned "pointer": every case is refused before anything is read or launched


@pytest.fixture(scope="module")
def lib():
    from poseestimationkf_amd import _lib
    return _lib


def _args(traj=P, traj_dt=P, traj_rows=4, batch=8, flags=0):
    return (batch, 8, P, P, P, 0.1, P, P, 1.0, 0.1, P, P, flags, traj, traj_dt, traj_rows, None, None)


def test_entry_is_declared_bound_and_exported(lib):
    text = open(HEADER).read()
    m = re.search(r"^int pekf_live_traj_dev\(([^;]*)\);", text, re.M | re.S)
    assert m, "include/pekf.h does not declare pekf_live_traj_dev"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 18 == len(lib.SIGNATURES["pekf_live_traj_dev"])
    assert [p.split()[-1].lstrip("*") for p in params[-6:]] == ["flags", "traj", "traj_dt", "traj_rows", "dev_error",
                                                                 "stream"]
    ext = re.search(r"^int pekf_live_ext_dev\(([^;]*)\);", text, re.M | re.S).group(1).split(",")
    assert len(ext) == 15 == len(lib.SIGNATURES["pekf_live_ext_dev"])      # the older entry is what it was
    assert hasattr(lib.lib, "pekf_live_traj_dev") and lib.lib.pekf_abi_version() == 1


def test_trajectory_arguments_are_refused_before_any_device_call(lib):
    L = lib.lib
    assert L.pekf_live_traj_dev(*_args(traj_rows=-1)) == lib.PEKF_ERR_INVALID
    assert "traj_rows" in lib.last_error()
    assert L.pekf_live_traj_dev(*_args(traj_rows=1 << 31)) == lib.PEKF_ERR_INVALID
    assert "traj_rows" in lib.last_error()
    assert L.pekf_live_traj_dev(*_args(traj=None)) == lib.PEKF_ERR_INVALID
    assert "traj must be" in lib.last_error()
    assert L.pekf_live_traj_dev(*_args(traj=P + 8)) == lib.PEKF_ERR_INVALID
    assert "traj must be" in lib.last_error()
    assert L.pekf_live_traj_dev(*_args(traj_dt=P + 4)) == lib.PEKF_ERR_INVALID
    assert "traj_dt" in lib.last_error()
    # a null traj_dt is allowed, and traj_rows == 0 looks at neither pointer: the next check refuses these
    assert L.pekf_live_traj_dev(*_args(traj_dt=None, flags=0x8)) == lib.PEKF_ERR_INVALID
    assert "unknown flags" in lib.last_error()
    bad_r = _args(traj=None, traj_dt=None, traj_rows=0)
    assert L.pekf_live_traj_dev(*(bad_r[:9] + (0.0,) + bad_r[10:])) == lib.PEKF_ERR_INVALID
    assert "r must be > 0" in lib.last_error()
    # pekf_live_ext_dev's own checks, in its order
    assert L.pekf_live_traj_dev(*_args(flags=0x5)) == lib.PEKF_ERR_INVALID
    assert "PEKF_EV_F64_EVENTS" in lib.last_error()
    assert L.pekf_live_traj_dev(*_args(batch=-1)) == lib.PEKF_ERR_INVALID
    assert "negative size" in lib.last_error()
    assert L.pekf_live_traj_dev(*_args(batch=0)) == lib.PEKF_OK


def test_trajectory_true_is_a_third_of_the_events():
    from poseestimationkf_amd import engine
    assert engine.trajectory_rows(True, 1500) == 500
    assert engine.trajectory_rows(True, 37) == 12
    assert engine.trajectory_rows(True, 2) == 0
    assert engine.trajectory_rows(False, 1500) == 0 and engine.trajectory_rows(None, 1500) == 0
    assert engine.trajectory_rows(5, 1500) == 5 and engine.trajectory_rows(np.int64(7), 30) == 7
    for bad in (-1, 1 << 31):
        with pytest.raises(ValueError, match="trajectory"):
            engine.trajectory_rows(bad, 1500)


def test_record_times_on_hand_made_arrays():
    from poseestimationkf_amd import engine
    nan = np.nan
    t0 = np.array([1000, 5_000_000_000_000, 7], np.int64)
    dt = np.array([[10.0, 2.0**31 + 0.5, nan],
                   [-4.0, 1.0, nan],          # a clock stepping back
                   [nan, 3.0, nan],           # filter 0 applied two records, filter 2 none
                   [nan, nan, nan]])
    t = engine.record_times_ns(t0, dt)
    assert t.dtype == np.float64 and t.shape == dt.shape
    want = np.array([[1010.0, 5e12 + 2.0**31 + 0.5, nan],
                     [1006.0, 5e12 + 2.0**31 + 1.5, nan],
                     [nan, 5e12 + 2.0**31 + 4.5, nan],
                     [nan, nan, nan]])
    assert np.array_equal(t, want, equal_nan=True)
    assert engine.record_times_ns(t0, np.empty((0, 3))).shape == (0, 3)


def test_without_a_trajectory_the_session_is_the_older_launch(monkeypatch):
    """The default calls pekf_live_ext_dev and nothing new; trajectory=True one pekf_live_traj_dev, after the
    two fills of its buffers."""
    from . import fake_libpekf

    class Fake(fake_libpekf.FakeLib):
        def __getattr__(self, name):
            if name in ("pekf_live_ext_dev", "pekf_live_traj_dev", "pekf_memset"):
                def f(*a):
                    self.calls.append((name, a))
                    return 0
                return f
            raise AttributeError("fake libpekf has no %s" % name)

    from poseestimationkf_amd import _lib, engine, synth
    fake = Fake(1)
    for mod in (_lib, engine):
        monkeypatch.setattr(mod, "lib", fake)
    K, E = 4, 30
    ev = synth.generate_events(np.arange(K), E, seed=3)
    f = engine.BatchedEKF(K)
    fake.calls.clear()
    assert len(f.run_events(ev)) == 2
    assert [c[0] for c in fake.calls] == ["pekf_live_ext_dev"]
    fake.calls.clear()
    out = f.run_events(ev, trajectory=True)
    assert [c[0] for c in fake.calls] == ["pekf_memset", "pekf_memset", "pekf_live_traj_dev"]
    assert fake.calls[0][1][1] == 0xFF and fake.calls[0][1][2] == 32 * 10 * K
    assert fake.calls[1][1][1] == 0xFF and fake.calls[1][1][2] == 8 * 10 * K
    assert fake.calls[2][1][15] == 10
    assert sorted(out[2]) == ["record_dt_ns", "record_times_ns", "trajectory"]
    assert out[2]["trajectory"].shape == (10, K, 4) and out[2]["record_dt_ns"].shape == (10, K)
    fake.calls.clear()
    out = f.run_events(ev, trajectory=3)
    assert fake.calls[2][1][15] == 3 and out[2]["record_times_ns"].shape == (3, K)
