#!/usr/bin/env python3
"""Differential fuzzing of the spectrum post-processing kernels (csrc/pnx_spectrum.hip) against scipy.signal
(`python tests/fuzz_spectrum_vs_scipy.py [n_cases] [seed] [--json out.json]` on a GPU box; tests/test_gpu_parity_large.py runs
100 fixed-seed cases of it in the GPU suite).  Random number of bins (3..512, both instantiations) and rows (1, 5, 64, 200),
number and width of the bumps, quantisation (none, one or two decimals: exact ties), forced plateaus (the one-lane path), height,
regularized, rel_height, max_peaks and number of cutoff ranges (overlapping, nested, inverted, ends on bin values).  The
comparison target is tests/spectrum_reference.py on every row; a failing case is any row that differs from it under the bars of
tests/test_gpu_spectrum.py: n_peaks, the NaN pattern and d_values exact, f_values / d_cut / f_cut within rtol 1e-12."""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spectrum_reference import spectrum_tables  # noqa: E402

TABLES = ("n_peaks", "d_values", "f_values", "d_cut", "f_cut")
RTOL = 1e-12


def mismatches(got, ref, rtol=RTOL):
    """Boolean (n_vox,): the rows of `got` (tables of a library call, numpy) that differ from `ref`: n_peaks, the NaN pattern and
    d_values exact; f_values, d_cut and f_cut within rtol of the reference's value."""
    bad = np.asarray(got["n_peaks"]) != ref["n_peaks"]
    for k in TABLES[1:]:
        if ref[k] is None or got[k] is None:
            assert ref[k] is None and got[k] is None, k
            continue
        g, r = np.asarray(got[k]), ref[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        gn, rn = np.isnan(g), np.isnan(r)
        gz, rz = np.where(gn, 0.0, g), np.where(rn, 0.0, r)
        tol = 0.0 if k == "d_values" else rtol * np.abs(rz)
        bad |= ((gn != rn) | ~(np.abs(gz - rz) <= tol)).any(axis=1)
    return bad


def describe(got, ref, rows, what=""):
    """The first differing row, table by table."""
    i = int(rows[0])
    lines = [f"{what}: {len(rows)} of {len(ref['n_peaks'])} rows differ, first {[int(r) for r in rows[:8]]}; row {i}:"]
    for k in TABLES:
        if ref[k] is not None:
            lines.append(f"  {k}: got {np.asarray(got[k])[i]!r}\n  {' ' * len(k)}  ref {ref[k][i]!r}")
    return "\n".join(lines)


def assert_tables_match(got, ref, what="", rtol=RTOL):
    rows = np.nonzero(mismatches(got, ref, rtol))[0]
    assert len(rows) == 0, describe(got, ref, rows, what)


def flat_topped_rise(X):
    """(n_vox,) bool: x[i-1] < x[i] == x[i+1] for an interior i -- the rows the kernel hands to its one-lane routine."""
    X = np.atleast_2d(X)
    return ((X[:, :-2] < X[:, 1:-1]) & (X[:, 1:-1] == X[:, 2:])).any(axis=1)


def random_rows(rng, n_vox, n):
    """Sums of Gaussian bumps with exact zeros between them, in one case of four with single-bin spikes on top (many peaks: the
    table limits), optionally rounded (ties) and with forced plateaus."""
    j = np.arange(n)
    k_max = int(rng.choice([1, 3, 8, 30, 90]))
    w_lo, w_hi = [(0.3, 1.0), (0.6, 12.0), (2.0, 40.0)][int(rng.integers(3))]
    decimals = [None, None, 1, 2][int(rng.integers(4))]
    p_plateau = float(rng.choice([0.0, 0.3, 1.0]))
    spikes = float(rng.choice([0.0, 0.0, 0.0, rng.uniform(0.03, 0.5)]))
    X = np.zeros((n_vox, n))
    for x in X:
        for _ in range(int(rng.integers(0, k_max + 1))):
            x += rng.uniform(0.05, 50) * np.exp(-0.5 * ((j - rng.integers(-2, n + 2)) / rng.uniform(w_lo, w_hi)) ** 2)
        x[x < 1e-3] = 0.0
        if spikes:
            x += (rng.random(n) < spikes) * rng.uniform(0.05, 9.0, n)
        if decimals is not None:
            x[:] = np.round(x, decimals)
        if rng.random() < p_plateau:
            for _ in range(int(rng.integers(1, 4))):
                i, w = int(rng.integers(0, n)), int(rng.integers(2, 6))
                x[i:i + w] = x[i] + float(rng.choice([0.0, 0.5]))
        if rng.random() < 0.1:
            x[0] = x[-1] = x.max() + 1.0  # maxima at the border are never peaks
    return X, f"bumps<={k_max} width {w_lo}-{w_hi} decimals={decimals} plateaus={p_plateau} spikes={spikes:.2f}"


def random_cutoffs(rng, bins, n_cut):
    n = len(bins)
    cut = []
    for _ in range(n_cut):
        kind = int(rng.integers(5))
        a, b = sorted(int(v) for v in rng.integers(0, n, 2))
        if kind == 0:    # ends on bin values (inclusive on both sides)
            cut.append((bins[a], bins[b]))
        elif kind == 1:  # ends between bin values
            cut.append((bins[a] * 0.999, bins[b] * 1.001))
        elif kind == 2:  # inverted: empty unless a == b
            cut.append((bins[b], bins[a]))
        elif kind == 3:  # everything
            cut.append((0.0, 1.0))
        else:            # nothing
            cut.append((0.6, 0.9))
    return np.array(cut, float).reshape(-1, 2)


def run(n_cases=200, seed=0, verbose=True):
    """n_cases random cases from `seed`; returns the summary dict that `--json` writes and the GPU suite asserts on."""
    from pyneapple_amd import _build, api

    say = print if verbose else (lambda *a, **k: None)
    rng = np.random.default_rng(seed)
    bad = rows = rows_bad = one_lane = overflow = with_peaks = 0
    for c in range(n_cases):
        n = int(rng.choice([int(rng.integers(3, 513)), int(rng.integers(3, 9)), int(rng.choice([63, 64, 65, 255, 256, 257, 258, 511, 512]))]))
        n_vox = int(rng.choice([1, 5, 64, 200]))
        bins = np.geomspace(0.0008, 0.5, n)
        X, desc = random_rows(rng, n_vox, n)
        kw = dict(height=float(rng.choice([0.0, 0.1, 0.1, 2.0, 5.0])), regularized=bool(rng.integers(2)),
                  rel_height=float(rng.choice([0.0, 0.25, 0.5, 0.5, 0.75, 1.0, 1.5, float(rng.uniform(0, 1))])),
                  max_peaks=int(rng.choice([0, 1, 4, 8, 16, 64])))
        n_cut = int(rng.choice([0, 1, 3, 8]))
        kw["cutoffs"] = random_cutoffs(rng, bins, n_cut) if n_cut else None
        desc = f"n_bins={n} n_vox={n_vox} {desc} {kw['height']=} {kw['regularized']=} {kw['rel_height']=} {kw['max_peaks']=} n_cut={n_cut}"
        ref = spectrum_tables(X, bins, **kw)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # "more than 64 peaks": those rows are compared like the others
                got = api.spectrum_peaks(X, bins, **kw)
        except Exception as e:
            say(f"[case {c}] GPU raised {e!r}: {desc}")
            bad += 1
            continue
        flat = flat_topped_rise(X)
        rows += n_vox
        one_lane += int(flat.sum())
        overflow += int((ref["n_peaks"] > np.where(flat, 16, 64)).sum())
        with_peaks += int((ref["n_peaks"] > 0).sum())
        diff = np.nonzero(mismatches(got, ref))[0]
        if len(diff):
            bad += 1
            rows_bad += len(diff)
            say(f"[case {c}] FAIL: {desc}\n" + describe(got, ref, diff, f"case {c}"))
    say(f"{n_cases} cases, {rows} rows ({with_peaks} with peaks, {one_lane} on the one-lane path, {overflow} beyond the table): "
        f"{rows_bad} differing rows in {bad} failing cases")
    return {"fuzzer": "spectrum", "n_cases": n_cases, "seed": seed, "rows": rows, "rows_with_peaks": with_peaks,
            "one_lane_rows": one_lane, "table_overflow_rows": overflow,
            "differing_rows": rows_bad, "failing_cases": bad,
            "thresholds": {"n_peaks, NaN pattern, d_values": "exact", "f_values, d_cut, f_cut": f"rtol {RTOL:g}"},
            "source_ids": _build.source_ids()}


def main():
    import json

    out = None
    if "--json" in sys.argv:
        i = sys.argv.index("--json")
        out = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    res = run(n_cases, seed)
    if out:
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 1 if res["failing_cases"] else 0


if __name__ == "__main__":
    sys.exit(main())
