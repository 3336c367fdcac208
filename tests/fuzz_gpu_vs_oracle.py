#!/usr/bin/env python3
"""Differential fuzzing of the HIP curve-fit path against the oracle on unusual inputs (`python tests/fuzz_gpu_vs_oracle.py [n_cases] [seed] [--hostile] [--wide-b] [--json out.json]` on a GPU box;
tests/test_gpu_parity_large.py runs 100 fixed-seed cases of it in the GPU suite).  Every case draws a model, a b-value
set (1..64 values, uniform or clinical or with duplicates), signal scale (1e-6..1e6), noise level, bounds (tight, loose,
half infinite), start values (random inside the box, on a bound, equal to the truth), Jacobian mode, optional
fixed parameters, optional T1 factor, small max_nfev.  Compared: status sign, cost (relative to the signal energy) and
-- where the oracle's own pcov says the parameters are determined -- the parameters at rtol 1e-4.  Prints every
disagreement; exit status 1 if any case shows a status-sign or cost disagreement on more than 2 % of its voxels."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pnx_oracle as oracle  # noqa: E402
from pyneapple_amd import api  # noqa: E402

NAMES = api.MODEL_PARAM_NAMES


def forward(model, b, P, t1_mode=0, tr=0.0, tm=0.0):
    e = lambda D: np.exp(-np.outer(D, b))
    nm = NAMES[model]
    p = {n: P[i][:, None] for i, n in enumerate(nm)}
    if model == "mono":
        s = p["S0"] * e(P[1])
    elif model == "bi_reduced":
        s = p["f1"] * e(P[1]) + (1 - p["f1"]) * e(P[2])
    elif model == "bi_s0":
        s = p["S0"] * (p["f1"] * e(P[1]) + (1 - p["f1"]) * e(P[2]))
    elif model == "bi_full":
        s = p["f1"] * e(P[1]) + p["f2"] * e(P[3])
    elif model == "tri_reduced":
        s = p["f1"] * e(P[1]) + p["f2"] * e(P[3]) + (1 - p["f1"] - p["f2"]) * e(P[4])
    elif model == "tri_s0":
        s = p["S0"] * (p["f1"] * e(P[1]) + p["f2"] * e(P[3]) + (1 - p["f1"] - p["f2"]) * e(P[4]))
    else:
        s = p["f1"] * e(P[1]) + p["f2"] * e(P[3]) + p["f3"] * e(P[5])
    if t1_mode:
        T1 = P[-1][:, None]
        s = s * (1 - np.exp(-tr / T1)) * (np.exp(-tm / T1) if t1_mode == 2 else 1.0)
    return s


def draw_case(rng, wide_b=False):
    model = rng.choice(list(NAMES))
    nm = list(NAMES[model])
    t1_mode = int(rng.choice([0, 0, 0, 1, 2]))
    tr, tm = 3000.0, 25.0
    if t1_mode:
        nm = nm + ["T1"]
    n_all = len(nm)
    hostile = HOSTILE  # also draw ill-posed problems (fewer b-values than parameters, free T1 next to a free amplitude,
    # infinite upper bounds on D, far-away starts): SciPy itself is not reproducible there, only crashes / hangs count
    kind = rng.choice(["lin", "clinical", "dup", "few"] if hostile else ["lin", "clinical", "dup"])
    if wide_b:  # 65..128 b-values (extra draws: the default sequence of cases stays what it was)
        kind = str(rng.choice(["lin", "lin", "dup"]))
    if kind == "lin" and hostile:
        n_b = int(rng.integers(n_all + 1, 65))
        b = np.linspace(0, float(rng.choice([800, 1200, 3000])), n_b)
    elif kind == "lin":
        n_b = int(rng.integers(16, 65))
        b = np.linspace(0, float(rng.choice([800, 1200])), n_b)
        if wide_b:
            b = np.linspace(0, b[-1], int(rng.integers(65, 129)))
    elif kind == "clinical":
        b = np.array([0, 5, 10, 20, 30, 40, 50, 75, 100, 150, 200, 400, 600, 800, 1000, 1500], float)[: int(rng.integers(max(n_all + 1, 6), 17))]
    elif kind == "dup":
        b = np.repeat(np.linspace(0, 1000, int(rng.integers(4, 12) if hostile else rng.integers(12, 20))), 3)
        if wide_b:
            b = np.repeat(np.linspace(0, 1000, int(rng.integers(22, 43))), 3)  # 66 .. 126
    else:
        b = np.sort(rng.uniform(0, 1000, int(rng.integers(1, n_all + 2))))  # fewer b-values than parameters is allowed
    n_b = len(b)
    n_vox = int(rng.choice([1, 37, 64, 130, 300]))
    scale = float(10.0 ** rng.integers(-6, 7)) if model in ("mono", "bi_s0", "bi_full", "tri_s0", "tri_full") else 1.0
    truth = []
    for n in nm:
        if n == "S0":
            truth.append(rng.uniform(0.5, 1.5, n_vox) * scale)
        elif n == "T1":
            truth.append(rng.uniform(800, 1600, n_vox))
        elif n.startswith("f"):
            amp = scale if model in ("bi_full", "tri_full") else 1.0
            truth.append(rng.uniform(0.1, 0.3, n_vox) * amp)
        else:
            k = int(n[1:]) if len(n) > 1 else 3
            truth.append(rng.uniform(*{1: (0.02, 0.1), 2: (0.003, 0.008), 3: (0.0005, 0.0015)}[min(k, 3) if model != "mono" else 3], n_vox))
    if model.startswith("bi") and "D2" in nm:
        truth[nm.index("D2")] = rng.uniform(0.0005, 0.002, n_vox)
    truth = np.array(truth)
    y = forward(model, b, truth, t1_mode, tr, tm)
    sigma = float(rng.choice([0.0, 0.003, 0.02, 0.1]))
    y = y * (1 + sigma * rng.standard_normal(y.shape))
    style = rng.choice(["loose", "tight", "halfinf"])
    lo = np.empty(n_all)
    hi = np.empty(n_all)
    for k in range(n_all):
        t_lo, t_hi = truth[k].min(), truth[k].max()
        if style == "loose" and (hostile or not nm[k].startswith("D")):
            lo[k], hi[k] = t_lo * 0.05, t_hi * 20
        elif style == "loose":
            # a D far above 1 / b_1 makes its Jacobian column vanish: J_aug turns exactly singular and SciPy's step is
            # decided by the rounding garbage of LAPACK's last singular vector (not reproducible by anything else)
            lo[k], hi[k] = t_lo * 0.2, t_hi * 3
        elif style == "tight":
            lo[k], hi[k] = t_lo * 0.9, t_hi * 1.1  # the optimum of noisy voxels sits on the box
        else:
            up_ok = hostile or not nm[k].startswith("D")  # an unbounded D lets a fast compartment run away (flat)
            top = t_hi * (20 if up_ok else 3)
            lo[k], hi[k] = (-np.inf, top) if (rng.random() < 0.5 or not up_ok) else (t_lo * 0.05, np.inf)
    if not hostile:
        # Keep every exponential visible at the first non-zero b-value (exp(-b_1 D_hi) >= 1e-6).  Beyond that the FD
        # column of that D is exactly zero, J_aug is singular and SciPy's trust-region step runs along LAPACK's
        # arbitrary completion of the null singular vector (solve_lsq_trust_region, rank-deficient branch): SciPy
        # itself is then not reproducible -- measured: the oracle freezes that D, SciPy and the kernel kick it back.
        b1 = np.sort(np.unique(b))[1]
        for k in range(n_all):
            if nm[k].startswith("D") and np.isfinite(hi[k]):
                hi[k] = max(min(hi[k], 13.8 / b1), truth[k].max() * 1.1)
    fin_lo = np.where(np.isfinite(lo), lo, truth.min(axis=1) * 0.05)
    fin_hi = np.where(np.isfinite(hi), hi, truth.max(axis=1) * 20)
    p0kind = rng.choice(["inside", "on_lo", "on_hi", "truthmean"])
    if p0kind == "inside" and hostile:
        p0 = fin_lo + rng.uniform(0.1, 0.9, n_all) * (fin_hi - fin_lo)
    elif p0kind == "inside":
        p0 = np.clip(truth.mean(axis=1) * rng.uniform(0.6, 1.6, n_all), fin_lo, fin_hi)
    elif p0kind in ("on_lo", "on_hi"):
        # hostile: every parameter starts on its bound (all Coleman-Li scalings 1e-10: chaotic even SciPy vs the oracle);
        # otherwise one parameter does and the others start near the truth
        on = np.ones(n_all, bool) if hostile else (np.arange(n_all) == rng.integers(n_all))
        edge = lo if p0kind == "on_lo" else hi
        mid = np.clip(truth.mean(axis=1) * rng.uniform(0.8, 1.25, n_all), fin_lo, fin_hi)
        p0 = np.where(on & np.isfinite(edge), edge, mid)
    else:
        p0 = np.clip(truth.mean(axis=1), fin_lo, fin_hi)
    n_fixed = int(rng.choice([0, 0, 1, 2])) if n_all >= 3 else int(rng.choice([0, 1]))
    n_fixed = min(n_fixed, n_all - 1)
    fixed_idx = sorted(rng.choice(n_all, n_fixed, replace=False).tolist())
    if t1_mode and not hostile and (n_all - 1) not in fixed_idx:
        # amplitude x relaxation factor is one identifiable product: keep T1 fixed unless ill-posed cases are wanted
        fixed_idx = sorted(set(fixed_idx[: max(0, min(len(fixed_idx), 1))] + [n_all - 1]))
        n_fixed = len(fixed_idx)
    free = [k for k in range(n_all) if k not in fixed_idx]
    jac = "analytic" if n_fixed else str(rng.choice(["fd", "analytic"]))
    fixed_vals = None
    if n_fixed:
        fixed_vals = truth[fixed_idx] if rng.random() < 0.5 else truth[fixed_idx].mean(axis=1)
    per_voxel = rng.random() < 0.3
    p0f, lof, hif = p0[free], lo[free], hi[free]
    if per_voxel:
        p0f = np.repeat(p0f[:, None], n_vox, 1)
        lof = np.repeat(lof[:, None], n_vox, 1)
        hif = np.repeat(hif[:, None], n_vox, 1)
    max_nfev = int(rng.choice([250, 250, 250, 3, 12]))
    kw = dict(fixed_idx=fixed_idx, fixed_vals=fixed_vals, jac=jac, max_nfev=max_nfev, t1_mode=t1_mode, tr=tr if t1_mode else 0.0,
              tm=tm if t1_mode == 2 else 0.0)
    desc = f"{model} t1={t1_mode} b={kind}:{n_b} n_vox={n_vox} scale={scale:g} sigma={sigma} bounds={style} p0={p0kind} fixed={fixed_idx} jac={jac} pv={per_voxel} max_nfev={max_nfev}"
    return desc, model, b, np.ascontiguousarray(y), p0f, lof, hif, kw


HOSTILE = "--hostile" in sys.argv


def run(n_cases=300, seed=0, verbose=True, n_threads=8, wide_b=False):
    """n_cases random cases from `seed`; returns the summary dict that `--json` writes and the GPU suite asserts on.
    wide_b: every case draws 65..128 b-values."""
    say = print if verbose else (lambda *a, **k: None)
    rng = np.random.default_rng(seed)
    bad_cases = 0
    tot_vox = tot_param_bad = tot_status_bad = tot_cost_bad = tot_sentinel_bad = 0
    for c in range(n_cases):
        desc, model, b, y, p0, lo, hi, kw = draw_case(rng, wide_b)
        try:
            o = oracle.curvefit(model, b, y, p0, lo, hi, n_threads=n_threads, **kw)
        except Exception as e:  # oracle rejects (e.g. m < n is fine, but some combos are invalid): the GPU must reject too
            try:
                api.curvefit(model, b, y, p0, lo, hi, **kw)
                say(f"[case {c}] oracle raised {e!r} but the GPU path did not: {desc}")
                bad_cases += 1
            except Exception:
                pass
            continue
        try:
            r = api.curvefit(model, b, y, p0, lo, hi, **kw)
        except Exception as e:
            say(f"[case {c}] GPU path raised {e!r}: {desc}")
            bad_cases += 1
            continue
        n_vox = y.shape[0]
        ok_r, ok_o = r["status"] > 0, o["status"] > 0
        st_bad = ok_r != ok_o
        energy = 0.5 * np.sum(y * y, axis=1) + 1e-300
        both = ok_r & ok_o
        cost_bad = both & (np.abs(r["cost"] - o["cost"]) > 1e-5 * np.maximum(o["cost"], 0) + 1e-9 * energy)
        sd = np.sqrt(np.abs(np.einsum("vii->vi", o["pcov"])))
        det = both & np.isfinite(sd).all(axis=1) & (sd < 0.2 * np.abs(o["popt"].T) + 1e-300).all(axis=1)
        e = np.abs(r["popt"] - o["popt"]) / np.maximum(np.abs(o["popt"]), 1e-300)
        par_bad = det & (e.max(axis=0) > 1e-4) & ~cost_bad
        fail_same = (~ok_r & ~ok_o)
        sentinel_bad = fail_same & ((r["popt"] != o["popt"]).any(axis=0) | (r["status"] != o["status"]))
        tot_vox += n_vox
        tot_status_bad += int(st_bad.sum()); tot_cost_bad += int(cost_bad.sum()); tot_param_bad += int(par_bad.sum())
        tot_sentinel_bad += int(sentinel_bad.sum())
        n_bad = int(st_bad.sum() + cost_bad.sum() + sentinel_bad.sum())
        if n_bad or par_bad.sum():
            flag = "FAIL" if n_bad > 0.02 * n_vox + (1 if n_vox > 50 else 0) else "note"
            say(f"[case {c}] {flag}: status {int(st_bad.sum())} cost {int(cost_bad.sum())} sentinel {int(sentinel_bad.sum())} "
                f"params {int(par_bad.sum())} of {n_vox}: {desc}")
            if st_bad.any():
                i = int(np.nonzero(st_bad)[0][0]); say(f"      voxel {i}: gpu status {r['status'][i]} nfev {r['nfev'][i]} cost {r['cost'][i]:.6g} | oracle status {o['status'][i]} nfev {o['nfev'][i]} cost {o['cost'][i]:.6g}")
            elif cost_bad.any():
                i = int(np.nonzero(cost_bad)[0][0]); say(f"      voxel {i}: gpu cost {r['cost'][i]:.10g} nfev {r['nfev'][i]} popt {r['popt'][:, i]} | oracle cost {o['cost'][i]:.10g} nfev {o['nfev'][i]} popt {o['popt'][:, i]}")
            if flag == "FAIL":
                bad_cases += 1
    say(f"{n_cases} cases, {tot_vox} voxels: status-sign disagreements {tot_status_bad}, cost disagreements {tot_cost_bad}, "
        f"parameter-only disagreements on determined voxels {tot_param_bad}; failing cases {bad_cases}")
    from pyneapple_amd import _build

    return {"fuzzer": "curvefit", "hostile": HOSTILE, "wide_b": wide_b, "n_cases": n_cases, "seed": seed, "voxels": tot_vox,
            "status_sign_disagreements": tot_status_bad, "cost_disagreements": tot_cost_bad,
            "parameter_only_disagreements_on_determined_voxels": tot_param_bad, "sentinel_disagreements": tot_sentinel_bad,
            "failing_cases": bad_cases,
            "thresholds": {"cost": "1e-5 relative + 1e-9 of the signal energy", "parameters": "rtol 1e-4 where the oracle's pcov "
                           "puts every standard deviation below 20 % of its parameter", "failing case": "status / cost / sentinel "
                           "disagreements on more than 2 % of its voxels"},
            "source_ids": _build.source_ids()}


def main():
    import json

    if HOSTILE:
        sys.argv.remove("--hostile")
    wide_b = "--wide-b" in sys.argv
    if wide_b:
        sys.argv.remove("--wide-b")
    out = None
    if "--json" in sys.argv:
        i = sys.argv.index("--json")
        out = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    res = run(n_cases, seed, wide_b=wide_b)
    if out:
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 1 if res["failing_cases"] else 0


if __name__ == "__main__":
    sys.exit(main())
