"""Every path of csrc/pnx_spectrum.hip against tests/spectrum_reference.py (scipy.signal, pinned on the reference-made fixtures by
tests/test_spectrum_reference.py): the bin counts on either side of the 64-bin register slots, the one-lane routine of flat-topped
rows with its own fraction / cutoff code under both instantiations, the wave path up to and beyond its 64-peak table, rel_height,
the cutoff semantics, more rows than one sweep of the grid (the second and third row a wave handles), device tensors and the
fused solve.  Rows are constructed; every test asserts that its rows reach the branch it is about, and every row is compared:
n_peaks, the NaN pattern and d_values exact, f_values / d_cut / f_cut within rtol 1e-12 (fuzz_spectrum_vs_scipy.mismatches)."""
from __future__ import annotations

import warnings

import numpy as np
import pytest
from fuzz_spectrum_vs_scipy import TABLES, assert_tables_match, flat_topped_rise
from spectrum_reference import spectrum_tables

pytestmark = pytest.mark.gpu
SLOTS = (64, 128, 192, 256, 320, 384, 448)


def make_bins(n):
    return np.geomspace(0.0008, 0.5, n)  # the reference's d_range: merged positions (log10) stay away from 0


def peaks_call(gpu, X, bins, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "more than 64 peaks": the NaN rows are part of what is compared
        return gpu.spectrum_peaks(X, bins, **kw)


def compare(gpu, X, bins, what="", **kw):
    """Library call on numpy rows against the helper, every row; returns the helper's tables."""
    ref = spectrum_tables(X, bins, kw["height"], kw["regularized"], kw["rel_height"], kw["max_peaks"], kw["cutoffs"])
    assert_tables_match(peaks_call(gpu, X, bins, **kw), ref, what)
    return ref


def all_peaks(X, bins, height):
    """(n_vox, 256) bin indices of every peak of every row, -1 padded (scipy, no table limit)."""
    from scipy import signal

    out = np.full((len(X), 256), -1)
    for i, x in enumerate(X):
        pk = signal.find_peaks(x, height=height)[0]
        out[i, :len(pk)] = pk
    return out


def bumps(rng, n_rows, n, k_max=6, w=(0.6, 12.0)):
    """Sums of Gaussian bumps, exactly zero between them (as NNLS spectra are)."""
    j = np.arange(n)
    X = np.zeros((n_rows, n))
    for x in X:
        for _ in range(int(rng.integers(1, k_max + 1))):
            x += rng.uniform(0.05, 50) * np.exp(-0.5 * ((j - rng.integers(0, n)) / rng.uniform(*w)) ** 2)
    X[X < 1e-3] = 0.0
    return X


def comb(rng, n, positions, plateau_every=0, shoulders=True, floor=0.0):
    """Isolated peaks at `positions` (at least 2 apart; 4 with shoulders or plateaus): random one-decimal or continuous heights,
    lower shoulders of unequal height, every plateau_every-th peak a flat top of two samples."""
    x = np.full(n, float(floor))
    for i, p in enumerate(positions):
        a = float(rng.choice([np.round(rng.uniform(0.5, 40), 1), rng.uniform(0.5, 40)]))
        x[p] = a
        flat = plateau_every and i % plateau_every == 0
        if flat:
            x[p + 1] = a
        if shoulders:
            x[p - 1] = max(x[p - 1], 0.3 * a * rng.random())
            q = p + (2 if flat else 1)
            if q < n:
                x[q] = 0.6 * a * rng.random()
    return x


# ---------------------------------------------------------------------------------------------------------- bin-count axis
def axis_rows(n, rng):
    rows = []

    def put(x):
        rows.append(np.asarray(x, float))

    put(np.zeros(n))
    put(np.full(n, 3.0))
    put(np.linspace(0.5, 9.0, n))
    put(np.linspace(9.0, 0.5, n))
    x = np.zeros(n); x[0], x[-1] = 5.0, 7.0; put(x)                      # maxima at the border are never peaks
    x = np.zeros(n); x[1] = 2.0; put(x)                                   # a peak at bin 1
    x = np.zeros(n); x[n - 2] = 3.0; put(x)                               # a peak at bin n - 2
    x = np.zeros(n); x[1], x[n - 2], x[0], x[-1] = 2.5, 3.5, 1.0, 0.5; put(x)
    x = np.zeros(n); x[n - 2:] = 4.0; put(x)                              # a plateau that runs into the last sample: no peak
    x = np.zeros(n); x[:2] = 4.0; put(x)                                  # ... and one that starts at the first: no rise
    if n >= 5:
        x = np.zeros(n); x[n - 3:] = 4.0; x[1] = 1.0; put(x)              # the same beside a real peak
        x = np.zeros(n); x[1:n - 1] = 2.0; put(x)                          # one plateau over the whole interior: peak at its midpoint
        x = np.zeros(n); x[1:n - 1] = 2.0; x[n // 2] = 2.5; put(x)
    for _ in range(8 if n > 8 else 90):                                   # small integers: ties everywhere
        x = rng.integers(0, 4, n).astype(float)
        if n > 8:
            x *= rng.random(n) < 0.15
        put(x)
    if n >= 16:
        c = n // 2
        x = np.zeros(n); x[[c - 4, c, c + 4]] = 2.0; x[[c - 2, c + 2]] = 0.5; put(x)           # equal peaks, equal valleys
        x = np.zeros(n); x[[c - 6, c - 3, c, c + 3, c + 6]] = (2.0, 1.0, 2.0, 1.0, 2.0)
        x[[c - 5, c - 4, c - 2, c - 1, c + 1, c + 2, c + 4, c + 5]] = 0.5; put(x)             # equal minima: the nearest is the base
        x = np.zeros(n); x[c - 3:c + 4] = (1.0, 2.0, 1.0, 3.0, 1.0, 2.0, 1.0); put(x)          # the sample at the height: h = x[i]
    for B in SLOTS:  # a peak, its bases and its width crossings on either side of each slot boundary
        if B + 6 > n - 1:
            continue
        for c in (B - 2, B - 1, B, B + 1):
            for w in (1, 2, 4, 6):
                x = np.zeros(n)
                for j in range(max(c - w, 0), min(c + w + 1, n)):
                    x[j] = 8.0 * (1 - abs(j - c) / (w + 0.5))
                x += 0.25                                                  # bases are ties: the nearest one counts
                if w == 4:
                    x[c - 2], x[c + 3] = x[c - 2] + 0.0625, 0.125        # unequal flanks, the lower base right
                put(x)
            x = np.zeros(n); x[c] = 3.0; x[max(c - 40, 1)] = 5.0; x[min(c + 40, n - 2)] = 4.0; x[c - 1] = x[c + 1] = 1.0
            put(x)                                                         # the nearest higher samples sit in other slots
        x = np.zeros(n); x[B - 2:B + 2] = 4.0; x[B - 3] = 1.0; put(x)      # a plateau straddling the boundary
        x = np.zeros(n); x[B - 1:B + 1] = 4.0; x[B + 3] = 6.0; put(x)
    fill = bumps(rng, max(100 - len(rows), 12), n, k_max=4, w=(0.6, max(1.0, n / 20))) if n >= 8 else np.zeros((0, n))
    for k, x in enumerate(fill):
        put(np.round(x, 1) if k % 3 == 0 else x)
    return np.array(rows)


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 319, 320, 321, 383, 384, 385,
                               447, 448, 449, 511, 512])
def test_bin_counts_on_either_side_of_the_register_slots(gpu, n):
    rng = np.random.default_rng(1000 + n)
    X, bins = axis_rows(n, rng), make_bins(n)
    cut = [(bins[0], bins[n // 2]), (bins[n // 2], bins[-1]), (bins[1], bins[1]), (bins[n - 2], bins[n - 2]), (0.6, 0.9)]
    flat = flat_topped_rise(X)
    pk = all_peaks(X, bins, 0.1)
    assert 90 <= len(X) <= 200
    assert (pk == 1).any() and (pk == n - 2).any() and not (pk == 0).any() and not (pk == n - 1).any()
    assert flat.sum() >= 2 and ((pk >= 0).any(axis=1) & ~flat).sum() >= 2
    for B in SLOTS:
        if B + 6 <= n - 1:  # wave-path rows with a peak on B - 1, B and B + 1, and a one-lane row with its plateau across B
            assert all((pk[~flat] == b).any() for b in (B - 1, B, B + 1))
            assert (flat & (X[:, B - 1] == X[:, B]) & (X[:, B] > 0)).any()
    for regularized in (False, True):
        compare(gpu, X, bins, f"{n} bins regularized={regularized}", height=0.1, regularized=regularized, rel_height=0.5,
                max_peaks=16, cutoffs=cut)
    compare(gpu, X, bins, f"{n} bins height 2", height=2.0, regularized=True, rel_height=0.5, max_peaks=3, cutoffs=cut)
    # below the bases the scan ends on the base itself: the only place where WHICH of several equal minima is the base shows
    compare(gpu, X, bins, f"{n} bins rel_height 1.5", height=0.1, regularized=True, rel_height=1.5, max_peaks=16, cutoffs=cut)


# ---------------------------------------------------------------------------------------------------- the one-lane path
def one_lane_rows(n, rng):
    """Flat-topped rows with 1..16 peaks and with 17..40 (the NaN rule), peaks 6 bins apart from bin 3 on."""
    rows = []
    for m in list(range(1, 17)) * 2 + list(range(17, 41)):
        start = int(rng.integers(3, n - 6 * m - 2)) if m < 30 else 3
        pos = [start + 6 * k for k in range(m)]
        rows.append(comb(rng, n, pos, plateau_every=int(rng.integers(1, 4)), floor=float(rng.choice([0.0, 0.05]))))
    x = np.zeros(n); x[n - 5:n - 3] = 2.0; rows.append(x)                 # one flat-topped peak beyond every range below
    x = np.zeros(n); x[1:3] = 2.0; x[n - 3:n - 1] = 3.0; rows.append(x)    # flat-topped peaks at bin 1 and bin n - 3
    return np.array(rows)


def eight_ranges(bins):
    n = len(bins)
    return [(bins[0], bins[n // 8]), (bins[n // 8 + 1], bins[n // 4]), (bins[n // 2], bins[n // 2 + 1]), (0.6, 0.9),
            (bins[n // 4], bins[n // 2]), (bins[n // 2], bins[n // 4]), (bins[3 * n // 4], bins[7 * n // 8]), (bins[2], bins[n // 16])]


@pytest.mark.parametrize("n", [250, 400])
@pytest.mark.parametrize("n_cut", [0, 1, 3, 8])
@pytest.mark.parametrize("max_peaks", [0, 4, 16, 64])
def test_one_lane_path_in_full(gpu, n, n_cut, max_peaks):
    rng = np.random.default_rng(77 + n)
    X, bins = one_lane_rows(n, rng), make_bins(n)
    cut = eight_ranges(bins)[:n_cut] or None
    assert flat_topped_rise(X).all()
    pk = all_peaks(X, bins, 0.1)
    cnt = (pk >= 0).sum(axis=1)
    assert ((cnt >= 1) & (cnt <= 16)).sum() >= 30 and ((cnt >= 17) & (cnt <= 40)).sum() >= 20 and (cnt == 16).any() and (cnt == 17).any()
    if n_cut == 8:  # ranges holding one peak, several and none, and a row with peaks whose every range is empty
        small = (cnt >= 1) & (cnt <= 16)
        d = np.where(pk >= 0, bins[np.clip(pk, 0, n - 1)], np.nan)
        per_range = np.array([((d >= lo) & (d <= hi)).sum(axis=1) for lo, hi in cut]).T[small]  # (rows, ranges)
        assert (per_range == 1).any(axis=1).sum() >= 5 and (per_range > 2).any(axis=1).sum() >= 5 and (per_range == 0).any(axis=1).sum() >= 5
        assert (per_range == 0).all(axis=1).any()
    for regularized in (False, True):
        ref = compare(gpu, X, bins, f"{n} bins, {n_cut} ranges, max_peaks {max_peaks}, regularized={regularized}", height=0.1,
                      regularized=regularized, rel_height=0.5, max_peaks=max_peaks, cutoffs=cut)
        np.testing.assert_array_equal(ref["n_peaks"], cnt)


# -------------------------------------------------------------------------------------------------- the wave path's table
@pytest.mark.parametrize("n", [250, 512])
def test_wave_path_up_to_its_table_and_beyond(gpu, n):
    rng = np.random.default_rng(5 + n)
    rows = []
    counts = [17, 18, 24, 31, 32, 33, 47, 48, 49, 62, 63, 64, 64, 65, 66, 70, 100, (n - 2) // 2]
    for m in counts:
        for spacing in (2, 3):
            if 1 + spacing * m > n - 1:
                continue
            start = int(rng.integers(1, n - 1 - spacing * (m - 1)))
            pos = [start + spacing * k for k in range(m)]
            x = comb(rng, n, pos, shoulders=False)
            x[x == 0] = rng.uniform(0.0, 0.09, int((x == 0).sum()))      # unequal valleys below the height: no flat top, real bases
            if spacing == 3 and m % 2:
                x[pos] = np.ceil(x[pos])                                    # equal neighbours among the peaks
            rows.append(x)
    X, bins = np.array(rows), make_bins(n)
    flat = flat_topped_rise(X)
    cnt = (all_peaks(X, bins, 0.1) >= 0).sum(axis=1)
    assert not flat.any()
    assert ((cnt >= 17) & (cnt <= 64)).sum() >= 20 and (cnt == 64).sum() >= 2 and (cnt == 65).any() and (cnt >= 100).sum() >= 2
    assert cnt.max() == (n - 2) // 2
    cut = [(bins[0], bins[-1]), (bins[n // 3], bins[2 * n // 3]), (bins[n // 2], bins[n // 2 + 1])]
    for regularized in (False, True):
        for max_peaks in (64, 16):
            ref = compare(gpu, X, bins, f"{n} bins regularized={regularized} max_peaks={max_peaks}", height=0.1,
                          regularized=regularized, rel_height=0.5, max_peaks=max_peaks, cutoffs=cut)
            np.testing.assert_array_equal(ref["n_peaks"], cnt)
            assert np.isnan(ref["f_cut"][cnt > 64]).all() and np.isfinite(ref["f_cut"][cnt <= 64, 0]).all()


# ------------------------------------------------------------------------------------------------------------- rel_height
@pytest.mark.parametrize("rel_height", [0.0, 0.25, 0.5, 0.75, 1.0, 1.5])
def test_rel_height(gpu, rel_height):
    """At 1.0 the evaluation height of a peak is its higher base (exactly 0 between separated peaks): the crossing lands on a
    sample.  At 0 every width is 0, the fractions sum to 0 and nothing is normalised.  Beyond 1 (SciPy takes any value >= 0, and
    so does the library) the height lies below the bases and the width runs from base to base: with exact zeros between the
    peaks the bases are ties, and the one nearest to the peak counts."""
    for n in (250, 300):
        rng = np.random.default_rng(31 + n)
        B = bumps(rng, 160, n)
        B[1::4] = np.round(B[1::4], 1)                                     # one decimal: samples that equal the evaluation height
        for x in B[2::4]:
            i = int(np.clip(np.argmax(x), 1, n - 4))
            x[i:i + 3] = x[i] + 1.0                                        # flat tops: the same on the one-lane path
        B[3::4] = np.round(B[3::4], 1)
        for x in B[3::8]:
            i = int(np.clip(np.argmax(x), 1, n - 4))
            x[i:i + 2] = x[i] + 0.5
        bins = make_bins(n)
        flat = flat_topped_rise(B)
        cnt = (all_peaks(B, bins, 0.1) >= 0).sum(axis=1)
        assert (flat & (cnt > 0) & (cnt <= 16)).sum() >= 40 and (~flat & (cnt > 1)).sum() >= 20
        cut = [(0.0008, 0.003), (0.003, 0.02), (0.01, 0.5)]
        ref = compare(gpu, B, bins, f"{n} bins rel_height {rel_height}", height=0.1, regularized=True, rel_height=rel_height,
                      max_peaks=16, cutoffs=cut)
        if rel_height == 0.0:
            assert (np.nan_to_num(ref["f_values"]) == 0).all() and (np.nan_to_num(ref["f_cut"]) == 0).all()
        else:
            np.testing.assert_allclose(np.nansum(ref["f_values"][cnt > 0], axis=1), 1.0, rtol=1e-12)


# -------------------------------------------------------------------------------------------------------- cutoff semantics
@pytest.mark.parametrize("n", [250, 400])
def test_cutoff_semantics(gpu, n):
    rng = np.random.default_rng(9 + n)
    bins = make_bins(n)
    a, b, c = n // 4, n // 2, 3 * n // 4
    rows = []
    for k in range(80):
        free = [p for p in range(4, n - 5, 5) if min(abs(p - q) for q in (a, b, c)) >= 5]
        pos = sorted([a, b, c] + [int(p) for p in rng.choice(free, int(rng.integers(0, 10)), replace=False)])
        rows.append(comb(rng, n, pos, plateau_every=(0, 2)[k % 2]))
    X = np.array(rows)
    flat = flat_topped_rise(X)
    pk = all_peaks(X, bins, 0.1)
    assert flat.sum() == 40 and (pk == a).any(axis=1).all() and (pk == b).any(axis=1).all() and (pk == c).any(axis=1).all()
    cnt = (pk >= 0).sum(axis=1)
    assert (cnt[flat] >= 3).sum() >= 20 and (cnt[~flat] >= 3).sum() >= 20 and cnt.max() <= 16
    sets = {
        "overlapping": [(bins[0], bins[b]), (bins[a], bins[c]), (bins[b], bins[-1])],
        "nested": [(bins[0], bins[-1]), (bins[a], bins[c]), (bins[b], bins[b])],
        "inverted": [(bins[c], bins[a]), (bins[a], bins[c]), (0.5, 0.0008)],
        "ends on peaks": [(bins[a], bins[b]), (bins[b], bins[c]), (bins[c], bins[c]), (bins[a], bins[a])],
        "eight": [(bins[0], bins[a]), (bins[a], bins[b]), (bins[b], bins[c]), (bins[c], bins[-1]), (bins[a + 1], bins[b - 1]),
                  (0.6, 0.9), (bins[b], bins[a]), (bins[0], bins[-1])],
        "one range holding every peak": [(0.0, 1.0)],
    }
    for name, cut in sets.items():
        for regularized in (False, True):
            ref = compare(gpu, X, bins, f"{n} bins, {name}, regularized={regularized}", height=0.1, regularized=regularized,
                          rel_height=0.5, max_peaks=8, cutoffs=cut)
            filled = np.isfinite(ref["f_cut"])
            np.testing.assert_allclose(np.nansum(ref["f_cut"], axis=1)[filled.any(axis=1)], 1.0, rtol=1e-12)
            if name == "inverted":
                assert not filled[:, 0].any() and not filled[:, 2].any() and filled[:, 1].all()
            if name == "ends on peaks":
                assert filled.all()  # both ends inclusive: every range holds at least the peak on its end
            if name == "one range holding every peak":
                assert filled.all() and (ref["d_cut"] < 0).sum() == (cnt > 1).sum()  # merged positions are log10 values


# ----------------------------------------------------------------------------------------------- more rows than one sweep
def sweep_rows(n, n_vox, rng):
    """Four kinds in random order: wave path, one-lane path, table overflow (both tables), no peak."""
    kind = rng.integers(0, 4, n_vox)
    X = bumps(rng, n_vox, n, k_max=4)
    for i in np.nonzero(kind == 1)[0]:
        x = X[i]
        p = int(np.clip(np.argmax(x), 1, n - 3))
        x[p:p + 2] = x[p] + 1.0
    for i in np.nonzero(kind == 2)[0]:
        if i % 2:  # more than 64 peaks, no flat top
            m = int(rng.integers(65, (n - 2) // 2))
            X[i] = 0.0
            X[i, 1:1 + 2 * m:2] = rng.uniform(0.5, 9.0, m)
        else:      # more than 16 peaks and a flat top
            m = int(rng.integers(17, 40))
            X[i] = comb(rng, n, [3 + 6 * k for k in range(m)], plateau_every=3)
    none = np.nonzero(kind == 3)[0]
    X[none] = np.minimum(X[none], 0.09)  # below the height
    X[none[::3]] = 0.0
    X[none[1::3]] = np.linspace(1.0, 2.0, n)
    return X, kind


@pytest.mark.parametrize("n", [250, 300])
def test_more_rows_than_one_sweep_of_the_grid(gpu, n):
    """The launch caps the grid at 8 blocks of 4 waves per CU; with 2.5 times as many rows every wave handles a second row and
    half of them a third, reusing its LDS row buffer, the pad samples and the per-lane peak table."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sweep = 32 * cus
    n_vox = int(2.5 * sweep) + 3
    rng = np.random.default_rng(n)
    X, kind = sweep_rows(n, n_vox, rng)
    bins = make_bins(n)
    flat = flat_topped_rise(X)
    assert all((kind == k).sum() >= n_vox // 8 for k in range(4))
    assert (kind[:-sweep] != kind[sweep:]).mean() > 0.5  # a wave's successive rows are of different kinds
    cut = [(0.0008, 0.003), (0.002, 0.02), (0.02, 0.5)]
    kw = dict(height=0.1, regularized=True, rel_height=0.5, max_peaks=8, cutoffs=cut)
    got = peaks_call(gpu, X, bins, **kw)
    ref = spectrum_tables(X, bins, **kw)
    assert_tables_match(got, ref, f"{n_vox} rows of {n} bins")
    over = ref["n_peaks"] > np.where(flat, 16, 64)
    assert (over & flat).sum() >= n_vox // 32 and (over & ~flat).sum() >= n_vox // 32
    assert (flat & ~over & (ref["n_peaks"] > 0)).sum() >= n_vox // 8 and (~flat & ~over & (ref["n_peaks"] > 0)).sum() >= n_vox // 8
    assert (ref["n_peaks"] == 0).sum() >= n_vox // 8
    back = peaks_call(gpu, np.ascontiguousarray(X[::-1]), bins, **kw)
    for k in TABLES:
        np.testing.assert_array_equal(back[k][::-1], got[k], err_msg=k)


# --------------------------------------------------------------------------------------------------------- device tensors
def test_device_tensors_and_two_bin_arrays_back_to_back(gpu):
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    for n, n_vox in ((250, 3000), (300, 20000)):
        X = bumps(rng, 400, n)
        for x in X[::3]:
            p = int(np.clip(np.argmax(x), 1, n - 3))
            x[p:p + 2] = x[p] + 1.0
        X = np.ascontiguousarray(X[rng.integers(0, 400, n_vox)])
        assert flat_topped_rise(X).sum() > n_vox // 5 and (~flat_topped_rise(X)).sum() > n_vox // 5
        bins1, bins2 = make_bins(n), np.geomspace(0.002, 0.3, n)
        cut = [(0.0008, 0.004), (0.004, 0.03), (0.03, 0.5)]
        kw = dict(height=0.1, regularized=True, rel_height=0.5, max_peaks=8, cutoffs=cut)
        host1, host2 = peaks_call(gpu, X, bins1, **kw), peaks_call(gpu, X, bins2, **kw)
        assert not np.array_equal(host1["d_values"], host2["d_values"], equal_nan=True)
        Xd = torch.from_numpy(X).to(dev)
        torch.cuda.synchronize()
        b1, b2 = bins1.copy(), bins2.copy()
        r1 = gpu.spectrum_peaks(Xd, b1, **kw)  # both only enqueue on the current stream: no synchronisation in between
        r2 = gpu.spectrum_peaks(Xd, b2, **kw)
        b1[:] = np.nan                         # the caller's arrays are free again when the call returns
        b2[:] = np.nan
        torch.cuda.synchronize()
        for k in TABLES:
            np.testing.assert_array_equal(r1[k].cpu().numpy(), host1[k], err_msg=f"{k}, first call, {n} bins")
            np.testing.assert_array_equal(r2[k].cpu().numpy(), host2[k], err_msg=f"{k}, second call, {n} bins")
        sub = slice(0, 1500)
        for host, bins in ((host1, bins1), (host2, bins2)):
            ref = spectrum_tables(X[sub], bins, **kw)
            assert_tables_match({k: host[k][sub] for k in TABLES}, ref, f"{n} bins")


# --------------------------------------------------------------------------------------------------------- the fused call
@pytest.mark.parametrize("reg_order", [2, None])
def test_fused_solve_against_the_helper_on_the_solved_spectra(gpu, reg_order):
    """NnlsPlan.solve_peaks against the helper applied to the spectra that a plain solve of the same plan returns: 250 bins with
    the second-order regulariser, and without one (spiky spectra: unregularised fractions are the raw heights)."""
    from pyneapple_amd import synth

    bins, basis, reg = synth.nnls_matrices(32)
    _, y, _ = synth.make_numpy("tri_reduced", 3000 + 7, 32, sigma=0.01, seed=11, scale=1000.0)
    plan = gpu.NnlsPlan(basis, reg if reg_order is not None else None, 0)
    try:
        spectra = plan.solve(y, 250)
        cut = [(0.0008, 0.003), (0.003, 0.02), (0.01, 0.5)]
        kw = dict(height=0.1, regularized=reg_order is not None, rel_height=0.5, max_peaks=8, cutoffs=cut)
        got = plan.solve_peaks(y, bins, max_iter=250, **kw)
    finally:
        plan.close()
    np.testing.assert_array_equal(got["residual"], spectra["residual"])
    np.testing.assert_array_equal(got["status"], spectra["status"])
    ref = spectrum_tables(spectra["coefficients"], bins, **kw)
    assert (ref["n_peaks"] >= 2).mean() > 0.5
    assert_tables_match(got, ref, f"solve_peaks, reg_order {reg_order}")
