"""The step fixture stays honest: tests/golden/make_step_golden.py is run again -- the exact RK4 chains and Wahba optima
by mpmath at 80 digits from tests/step_families.py's items, the reference's float64 statements from
oracle/ekf_numpy.py -- into a scratch directory, and the result is compared with the committed
tests/golden/step_families.npz bit for bit.  The fixture's inputs come from the generator, so a change there would show
here.

Runs only where mpmath is installed, as tests/test_golden_regen_wahba.py does."""
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import GOLDEN

pytest.importorskip("mpmath")


def test_make_step_golden_regenerates_the_committed_fixture(tmp_path):
    env = dict(os.environ, PEKF_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_step_golden.py")], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(os.path.join(GOLDEN, "step_families.npz")) as a, np.load(os.path.join(tmp_path, "step_families.npz")) as b:
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert np.array_equal(a[k].reshape(-1).view(np.uint8), b[k].reshape(-1).view(np.uint8)), k
    assert os.path.getsize(os.path.join(GOLDEN, "step_families.npz")) < 256 * 1024
