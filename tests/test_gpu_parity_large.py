"""A bounded slice of the large-sample evidence inside the GPU suite: 65 536 voxels of the C3 workload and 16 384 of the C4
workload against the oracle (the full-size runs are profiles/parity_large.py -> profiles/r05_parity_large.json, one stamped set
per round), and 100 fixed-seed cases of each differential fuzzer (tests/fuzz_gpu_vs_oracle*.py -> profiles/r05_fuzz_*.json).  The
thresholds are the recorded rates of those runs with a margin; what the rates mean is argued in DESIGN.md section 3."""
from __future__ import annotations

import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_c3_sample_against_the_oracle(gpu, oracle):
    r = _load("profiles/parity_large.py", "parity_large").c3(1 << 16, verbose=False)
    assert r["success_equal"] == 1.0           # 1 048 576-voxel run: 1.0
    assert r["status_equal"] >= 0.999          # 0.9994
    assert r["nfev_equal"] >= 0.998            # 0.9989
    assert r["within_1e-4"] >= 0.997           # 0.99857; the rest are flat valleys:
    assert r["cost_rel_diff_all_max"] <= 1e-4  # ... their costs agree (1.0e-5 over the large run)
    assert r["median_rel"] < 1e-7
    assert r["pcov_rel_max_where_params_agree_median"] < 1e-6


def test_c4_sample_against_the_oracle(gpu, oracle):
    r = _load("profiles/parity_large.py", "parity_large").c4(1 << 14, verbose=False)
    # 131 072-voxel run: every status, iteration count and support identical
    assert r["status_equal"] == 1.0 and r["iters_equal"] == 1.0 and r["support_equal"] == 1.0
    assert r["coef_err_max"] < 1e-6 and r["rnorm_rel_max"] < 1e-12
    # the sample contains voxels whose passive set passes the block kernel's 128 positions (142 bins): the hand-over to the
    # general kernel is part of what was just compared
    assert r["max_passive_set"] > 128


def test_curvefit_fuzz_100_cases(gpu, oracle):
    r = _load("tests/fuzz_gpu_vs_oracle.py", "fuzz_curvefit").run(100, seed=20260504, verbose=False)
    assert r["failing_cases"] == 0, r
    assert r["voxels"] > 5000
    # 800-case runs: 3-10 status-sign, 4-19 cost, 8-18 parameter-only disagreements in ~84 000 voxels
    assert r["status_sign_disagreements"] <= 0.001 * r["voxels"] + 3, r
    assert r["cost_disagreements"] <= 0.001 * r["voxels"] + 3, r
    assert r["sentinel_disagreements"] == 0, r


def test_curvefit_fuzz_60_cases_at_65_to_128_b_values(gpu, oracle):
    """The same fuzzer with every case drawing 65..128 b-values (blocks of 3, 2 and 1 waves for five and more free parameters):
    the assertions and the margin rule of test_curvefit_fuzz_100_cases."""
    r = _load("tests/fuzz_gpu_vs_oracle.py", "fuzz_curvefit").run(60, seed=20261016, verbose=True, wide_b=True)
    assert r["failing_cases"] == 0, r
    assert r["voxels"] > 3000
    # this seed: 0 status-sign, 3 cost (all in one case: tri_reduced, 79 b-values, 10 % noise, half-infinite bounds, start on a
    # bound), 0 parameter-only and 0 sentinel disagreements in 7 150 voxels -- inside the recorded rates of the 1..64 runs
    assert r["status_sign_disagreements"] <= 0.001 * r["voxels"] + 3, r
    assert r["cost_disagreements"] <= 0.001 * r["voxels"] + 3, r
    assert r["sentinel_disagreements"] == 0, r


def test_nnls_fuzz_100_cases(gpu, oracle):
    r = _load("tests/fuzz_gpu_vs_oracle_nnls.py", "fuzz_nnls").run(100, seed=20260504, verbose=False)
    # 400-case runs: status 4-10, coefficients 0-10 (mu = 0.002 only), rnorm 0 in ~25 000 voxels; cases that fail there are
    # single rank-deficient / cycling voxels, so the bound here is on counts, not on "no failing case"
    assert r["voxels"] > 3000
    assert r["status_disagreements"] <= 0.002 * r["voxels"] + 2, r
    assert r["coefficient_disagreements"] <= 0.002 * r["voxels"] + 2, r
    assert r["rnorm_disagreements"] <= 2, r


def test_nnls_fuzz_wide_40_cases(gpu, oracle):
    """The same fuzzer on the eight-bins-per-lane instantiations (257..512 bins): Gram form with the reference's and with dense
    regularisers, QR form without one."""
    r = _load("tests/fuzz_gpu_vs_oracle_nnls.py", "fuzz_nnls").run(40, seed=20261005, verbose=True, wide=True)
    # 200-case run (profiles/r04_fuzz_nnls_wide.json): status 12 (8 of them in one unregularised max_iter = 20 case, the others
    # single voxels where one side cycles into max_iter = 250 and the other converges -- the iteration counts of 300-512 bin fits
    # sit much closer to the limit than those of 250-bin fits), coefficients 10 (1.6e-6 .. 2.7e-6 of the peak at mu <= 0.02),
    # rnorm 0 in 12 643 voxels
    assert r["voxels"] > 1000
    assert r["status_disagreements"] <= 0.004 * r["voxels"] + 8, r
    # this seed: 13 voxels of ONE case (8 measurements, 300 bins, order 3 at mu = 0.002: the weakly damped class of DESIGN section 3)
    # at 1.4e-6 .. 1.2e-5 of the peak with identical iteration counts and residual norms -- the Gram form's eps * cond(G), which
    # grows with the number of bins and falls with mu (the reference's mu = 0.02 at 32 measurements: < 1e-6 on every fixture and
    # oracle test); so the count is bounded loosely and the SIZE of the largest error by a cap
    assert r["coefficient_disagreements"] <= 0.005 * r["voxels"] + 4, r
    assert r["max_coefficient_error_rel_peak"] < 1e-4, r
    assert r["rnorm_disagreements"] <= 2, r


def test_spectrum_fuzz_100_cases(gpu):
    """Random spectra, bin counts (3..512), heights, rel_height, table sizes and cutoff ranges through the peak / width / cutoff
    kernels against scipy.signal (tests/fuzz_spectrum_vs_scipy.py): no row differs, and the draw reaches the one-lane path and
    the table limits."""
    r = _load("tests/fuzz_spectrum_vs_scipy.py", "fuzz_spectrum").run(100, seed=20261017, verbose=True)
    assert r["failing_cases"] == 0 and r["differing_rows"] == 0, r
    assert r["rows"] > 3000 and r["rows_with_peaks"] > 1500, r
    assert r["one_lane_rows"] > 300 and r["table_overflow_rows"] > 20, r


def test_streamed_host_path_fuzz_40_cases(gpu):
    """Random configurations of the streamed host path against the chunk ring (tests/fuzz_stream_vs_ring.py): bit-identical
    outputs, no watermark time-out, streamed exactly when the batch has two or more granules."""
    r = _load("tests/fuzz_stream_vs_ring.py", "fuzz_stream").run(40, seed=20261004, verbose=True)
    assert r["failing_cases"] == 0, r
    assert r["streamed_cases"] >= 30


def test_streamed_host_path_fuzz_16_cases_at_41_to_128_b_values(gpu):
    """The streamed launch with 41..128 b-values (its blocks of 3, 2 and 1 waves, one block per CU): bit-identical to the ring, no
    watermark time-out, streamed exactly when the batch has two or more granules."""
    r = _load("tests/fuzz_stream_vs_ring.py", "fuzz_stream").run(16, seed=20261016, verbose=True, wide_b=True)
    assert r["failing_cases"] == 0, r
    assert r["streamed_cases"] >= 12


def test_nnls_host_chunkings_fuzz_12_cases(gpu):
    """Random chunkings of the NNLS host path (deferred / per-chunk / overflowing hand-over, float32, peak tables) against the
    single-chunk call, on rows that contain handed-over voxels (tests/fuzz_nnls_host.py)."""
    r = _load("tests/fuzz_nnls_host.py", "fuzz_nnls_host").run(12, seed=20261004, verbose=True)
    assert r["failing_cases"] == 0, r
    assert r["handed_over_voxels"] >= 1
