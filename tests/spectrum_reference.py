"""A plain restatement of the spectrum post-processing that include/pnx.h documents for pnx_nnls_spectrum_peaks_f64, row by
row on scipy.signal: what tests/test_spectrum_reference.py pins against the reference-made fixtures and what the GPU tests
(tests/test_gpu_spectrum_paths.py, tests/fuzz_spectrum_vs_scipy.py) compare the device tables with.  Not a conftest."""
from __future__ import annotations

import warnings

import numpy as np
from scipy import signal


def spectrum_tables(spectra, bins, height, regularized, rel_height, max_peaks, cutoffs):
    """dict(n_peaks (n_vox,) int32, d_values, f_values (n_vox, max_peaks), d_cut, f_cut (n_vox, n_cut) or None without cutoffs).

    Per row: peaks = scipy.signal.find_peaks(x, height=height); fractions = peak heights or, regularized, height * fwhm /
    (2 sqrt(2 ln 2)) * sqrt(2 pi) with fwhm = scipy.signal.peak_widths(x, peaks, rel_height); divided by their sum when it is
    > 0; d = bins[peaks].  The first max_peaks of them are reported, NaN padded.  The cutoffs see every peak: per range
    [lo, hi] (both ends inclusive) none -> NaN, one -> kept, several -> log10(prod(d ** (f / sum f))) and sum f; then the
    range fractions are divided by their nansum when it is > 0.

    The library's table limit, stated exactly: a row with more than 64 peaks, or with a flat-topped rise (x[i-1] < x[i] ==
    x[i+1] for an interior i) and more than 16, has all-NaN peak and cutoff rows and its true count in n_peaks."""
    spectra = np.atleast_2d(np.asarray(spectra, np.float64))
    bins = np.asarray(bins, np.float64)
    n_vox = spectra.shape[0]
    cut = None if cutoffs is None else np.asarray(cutoffs, np.float64).reshape(-1, 2)
    n_cut = 0 if cut is None else len(cut)
    n_peaks = np.zeros(n_vox, np.int32)
    d_values = np.full((n_vox, max_peaks), np.nan)
    f_values = np.full((n_vox, max_peaks), np.nan)
    d_cut = np.full((n_vox, n_cut), np.nan) if n_cut else None
    f_cut = np.full((n_vox, n_cut), np.nan) if n_cut else None
    for i, x in enumerate(spectra):
        pk, prop = signal.find_peaks(x, height=height)
        n_peaks[i] = len(pk)
        flat_topped_rise = bool(((x[:-2] < x[1:-1]) & (x[1:-1] == x[2:])).any())
        if len(pk) == 0 or len(pk) > (16 if flat_topped_rise else 64):
            continue
        f = prop["peak_heights"].astype(np.float64)
        if regularized:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # PeakPropertyWarning: a width of 0 (rel_height = 0)
                fwhm = signal.peak_widths(x, pk, rel_height=rel_height)[0]
            f = f * fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0))) * np.sqrt(2.0 * np.pi)
        s = f.sum()
        if s > 0:
            f = f / s
        d = bins[pk]
        k = min(len(pk), max_peaks)
        d_values[i, :k] = d[:k]
        f_values[i, :k] = f[:k]
        for c in range(n_cut):
            sel = (d >= cut[c, 0]) & (d <= cut[c, 1])
            if sel.sum() == 1:
                d_cut[i, c], f_cut[i, c] = d[sel][0], f[sel][0]
            elif sel.sum() > 1:
                fs = f[sel].sum()
                with np.errstate(invalid="ignore", divide="ignore"):  # every width 0: the weights are 0 / 0 and the position NaN
                    d_cut[i, c] = np.log10(np.prod(d[sel] ** (f[sel] / fs)))
                f_cut[i, c] = fs
        if n_cut:
            t = np.nansum(f_cut[i])
            if t > 0:
                f_cut[i] = f_cut[i] / t
    return dict(n_peaks=n_peaks, d_values=d_values, f_values=f_values, d_cut=d_cut, f_cut=f_cut)
