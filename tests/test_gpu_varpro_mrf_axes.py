"""The field posterior over the variable projection's dictionary along the b-value axis for the largest layout: K = 3 with a free
T1 (four non-linear rows: the field product's k-step is full) at 16, 33 and 128 b-values -- the NS = 8 kernel, and the NS = 32
kernel that folds one of a lane's four rows per sweep over the dictionary -- at 83 voxels and 33 atoms, against
tests/varpro_mrf_reference.py under the acceptance of tests/test_gpu_varpro_mrf.py; and a zero field as the plain posterior's bytes
there.  The instantiations tests/test_gpu_varpro_mrf.py leaves out."""
from __future__ import annotations

import numpy as np
import pytest
import varpro_mrf_cases as cases
from test_gpu_varpro_mrf import _check_whole, _kw, field_on_device, same_bytes, sentinel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_b", [16, 33, 128])
def test_field_posterior_three_compartments_and_t1_along_the_b_axis(gpu, n_b):
    c, got = _check_whole(gpu, f"axes-{n_b}")
    assert c["nl_atoms"].shape == (4, 33) and c["y"].shape == (83, n_b)
    # and with every precision 0 the same kernel returns the plain posterior's bytes, whatever the field holds
    zero = field_on_device(gpu, c, c["q"], c["n"], np.zeros(len(c["lo"])), 17, 40, sentinel(len(c["lo"]), 83))
    same_bytes(zero, c["plain"], sel=np.arange(17, 57))
    same_bytes(zero, sentinel(len(c["lo"]), 83), sel=np.r_[0:17, 57:83])
    assert _kw(c)["t1_mode"] == 1
