"""The phase-1 fixture stays honest: tests/golden/make_magcal_golden.py is run again -- it imports the
REFERENCE's own MagnetometerCalibration_test.py and calls its computeBias / compute_R unchanged -- into a
scratch directory, and the result is compared with the committed tests/golden/magcal.npz bit for bit.  The
fixture's inputs come from this repo's synth.generate_calibration_events, so a change there would show here.

Runs only where the reference is present (the build container), as tests/test_golden_regen.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import GOLDEN

REF_FILE = "/root/reference/MagnetometerCalibration_test.py"

pytestmark = pytest.mark.skipif(not os.path.isfile(REF_FILE), reason="the reference is not present here")


def test_make_magcal_golden_regenerates_the_committed_fixture(tmp_path):
    env = dict(os.environ, PEKF_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1", MPLBACKEND="Agg")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_magcal_golden.py")], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(os.path.join(GOLDEN, "magcal.npz")) as a, np.load(os.path.join(tmp_path, "magcal.npz")) as b:
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert np.array_equal(a[k].reshape(-1).view(np.uint8), b[k].reshape(-1).view(np.uint8)), k
    assert os.path.getsize(os.path.join(GOLDEN, "magcal.npz")) < 256 * 1024
    assert not os.path.isdir(os.path.join(os.path.dirname(REF_FILE), "__pycache__"))
