"""tests/spectrum_reference.py (scipy.signal, written from include/pnx.h) against the reference's own find_spectrum_peaks +
apply_cutoffs as oracle/gen_golden.py recorded them: the g9 / g11 fixtures on NNLS spectra and the constructed rows of the
g14_spectrum_adversarial_* family (flat tops, merged ranges, overlapping / empty ranges, range ends on peaks).  The bars are
those of tests/test_gpu_spectrum.py.  No GPU."""
from __future__ import annotations

import glob
import os

import numpy as np
import pytest
from conftest import GOLDEN, load_golden
from spectrum_reference import spectrum_tables

FIXTURES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "g*_spectrum_*.npz")))
OLD = [f for f in FIXTURES if not f.startswith("g14_")]
G14 = [f for f in FIXTURES if f.startswith("g14_spectrum_adversarial_")]


def flat_topped_rise(x):
    return ((x[:, :-2] < x[:, 1:-1]) & (x[:, 1:-1] == x[:, 2:])).any(axis=1)


def test_the_fixture_families_are_all_here():
    assert len(OLD) == 12 and sum(len(load_golden(f)["n_peaks"]) for f in OLD) == 448
    assert len(G14) == 12 and len(FIXTURES) == 24


@pytest.mark.parametrize("name", FIXTURES)
def test_helper_matches_the_reference(name):
    d = load_golden(name)
    r = spectrum_tables(d["spectrum"], d["bins"], float(d["height"]), bool(d["regularized"]), 0.5, d["d_values"].shape[1], d["cutoffs"])
    np.testing.assert_array_equal(r["n_peaks"], d["n_peaks"])
    np.testing.assert_array_equal(np.isnan(r["d_values"]), np.isnan(d["d_values"]))
    np.testing.assert_array_equal(np.nan_to_num(r["d_values"]), np.nan_to_num(d["d_values"]))  # bins[peak]: exact
    np.testing.assert_allclose(r["f_values"], d["f_values"], rtol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(np.isnan(r["d_cut"]), np.isnan(d["d_cut"]))
    np.testing.assert_allclose(r["d_cut"], d["d_cut"], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(r["f_cut"], d["f_cut"], rtol=1e-12, equal_nan=True)


@pytest.mark.parametrize("name", G14)
def test_adversarial_fixtures_reach_what_they_were_made_for(name):
    """What oracle/gen_golden.py main_g14 promises of every file, read back from the recorded data."""
    d = load_golden(name)
    x, bins, cut, n = d["spectrum"], d["bins"], d["cutoffs"], d["n_peaks"]
    assert x.shape[0] <= 48 and x.shape[1] in (250, 300, 512) and bins.max() <= 0.5
    assert n.max() <= 16 and os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 177 * 1024
    flat = flat_topped_rise(x)
    assert flat.sum() * 3 >= len(x)
    dv = d["d_values"]
    inside = [(dv >= lo) & (dv <= hi) for lo, hi in cut]
    merged = np.array([m.sum(axis=1) for m in inside]).T > 1                  # (rows, ranges)
    assert (merged.any(axis=1) & flat).sum() >= 3                               # several peaks in one range on the one-lane path
    assert (merged.any(axis=1) & ~flat).sum() >= 3                              # ... and on the wave path
    assert any(not m.any() for m in inside)                                    # a range that holds no peak of any row
    assert np.isin(cut.ravel(), dv[np.isfinite(dv)]).any()                      # a range end on a bin value that carries a peak
    overlapping = any(max(a[0], b[0]) <= min(a[1], b[1]) for i, a in enumerate(cut) for b in cut[i + 1:])
    assert overlapping == bool(d["overlapping_cutoffs"])
    if overlapping:  # some peak is counted in two ranges
        assert (np.array([m.any(axis=1) for m in inside]).sum(axis=0) >= 2).any() and (sum(m.astype(int) for m in inside) >= 2).any()


def test_both_cutoff_sets_are_used():
    assert {bool(load_golden(f)["overlapping_cutoffs"]) for f in G14} == {True, False}
