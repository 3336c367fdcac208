"""The real drop-in: the reference's own TOML loader resolves `hip_curvefit` / `hip_nnls` / `hip_pixelwise` / `hip_ideal`
through entry points and builds the fitter (io/toml.py:106-148, 202-236, 328-338), with the extra `[Fitting.solver]`
keys forwarded as constructor kwargs.  Modelled on the reference's tests/test_io_plugin_discovery.py:84-148.

Everywhere: tests/golden/g13_toml_plugins.json records what the reference's loader made of the four TOML files below (the
parsed model section, every keyword argument it handed a plugin constructor, the error build_fitter raised), and the test
replays those calls against the entry points of our pyproject.toml.  Where Pyneapple itself is present as well -- importable,
or its source tree named by PYNEAPPLE_SRC (the directory that holds the `pyneapple` package) -- its loader runs too, and
`python tests/test_plugin_dropin.py` re-records the fixture.  Both run in a child process -- the plugin
classes pick their base classes at import time (pyneapple_amd/_compat.py), and this test process has already imported
them without the reference.  The two `sys.modules` stand-ins for loguru / cv2 are SURVEY.md Appendix B's; they live
here, in test code, not in the product."""
from __future__ import annotations

import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pyneapple_src():
    """The directory that holds the `pyneapple` package: $PYNEAPPLE_SRC, else wherever an installed Pyneapple lives; None if neither."""
    src = os.environ.get("PYNEAPPLE_SRC")
    if src:
        return src if os.path.isdir(os.path.join(src, "pyneapple")) else None
    import importlib.util

    spec = importlib.util.find_spec("pyneapple")
    if spec is None or not spec.submodule_search_locations:
        return None
    return os.path.dirname(os.path.abspath(list(spec.submodule_search_locations)[0]))


REF_SRC = _pyneapple_src()

TOMLS = {"tri": """
[Fitting]
fitter = "hip_pixelwise"
[Fitting.model]
type = "triexp"
[Fitting.solver]
type = "hip_curvefit"
max_iter = 250
tol = 1e-8
device = 0
n_gpus = 1
jacobian = "fd"
io_dtype = "float64"
xtol = 1e-9
multi_threading = true
n_pools = 4
[Fitting.solver.p0]
f1 = 0.2
D1 = 0.05
f2 = 0.3
D2 = 0.005
D3 = 0.001
[Fitting.solver.bounds]
f1 = [0.0, 1.0]
D1 = [0.01, 0.5]
f2 = [0.0, 1.0]
D2 = [0.002, 0.01]
D3 = [0.00001, 0.002]
""", "nnls": """
[Fitting]
fitter = "pixelwise"
[Fitting.model]
type = "nnls"
d_range = [0.0008, 0.5]
n_bins = 250
[Fitting.solver]
type = "hip_nnls"
reg_order = 2
mu = 0.02
max_iter = 250
tol = 1e-8
multi_threading = false
device = 0
"""}
TOMLS["ideal"] = TOMLS["tri"].replace('"hip_pixelwise"', '"hip_ideal"')   # a plugin fitter other than the built-in "ideal"
TOMLS["bad"] = TOMLS["tri"].replace("xtol = 1e-9", 'loss = "soft_l1"')     # an unsupported curve_fit argument

PREAMBLE = r'''
import os, sys, types
sys.dont_write_bytecode = True
class _Noop:
    def __getattr__(self, name):
        return lambda *a, **k: None
loguru = types.ModuleType("loguru"); loguru.logger = _Noop(); sys.modules["loguru"] = loguru
cv2 = types.ModuleType("cv2"); cv2.INTER_LINEAR = 1; cv2.INTER_CUBIC = 2; sys.modules["cv2"] = cv2
for name in ("nibabel", "h5py"):
    try:
        __import__(name)
    except Exception:
        sys.modules[name] = types.ModuleType(name)
sys.path.insert(0, REF_SRC); sys.path.insert(0, ROOT)
import numpy as np
try:
    import tomllib
except ModuleNotFoundError:
    import tomli as tomllib
from importlib.metadata import EntryPoint
import pyneapple.io.toml as T
from pyneapple.fitters.base import BaseFitter
from pyneapple.solvers import CurveFitSolver, NNLSSolver

# what `pip install pyneapple-amd` registers: the entry points of OUR pyproject.toml, discovered the reference's way
with open(os.path.join(ROOT, "pyproject.toml"), "rb") as fh:
    eps = tomllib.load(fh)["project"]["entry-points"]
def fake_entry_points(group):
    return [EntryPoint(name=k, value=v, group=group) for k, v in eps.get(group, {}).items()]
T.entry_points = fake_entry_points
T._discover_plugins("pyneapple.solvers", T._SOLVER_REGISTRY)
T._discover_plugins("pyneapple.fitters", T._FITTER_REGISTRY)
assert {"hip_curvefit", "hip_nnls"} <= set(T._SOLVER_REGISTRY) and {"hip_pixelwise", "hip_ideal"} <= set(T._FITTER_REGISTRY)
assert isinstance(T._SOLVER_REGISTRY["hip_curvefit"], EntryPoint)   # lazy: nothing of the plugin imported yet
assert "pyneapple_amd.solvers" not in sys.modules

'''

CHECKS = r'''
cfg = os.path.join(TMP, "tri.toml")
open(cfg, "w").write(TOMLS["tri"])
fitter = T.load_config(cfg).build_fitter()
from pyneapple_amd import _compat, _lib
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.ideal import HipIDEALFitter
from pyneapple_amd.solvers import HipCurveFitSolver, HipNNLSSolver
assert _compat.HAVE_PYNEAPPLE
assert type(fitter) is HipPixelWiseFitter and isinstance(fitter, BaseFitter)
s = fitter.solver
assert type(s) is HipCurveFitSolver and isinstance(s, CurveFitSolver)
assert issubclass(HipNNLSSolver, NNLSSolver)      # fitters/base.py:162-169 picks the R^2 path with isinstance
assert (s.device, s.n_gpus, s.jacobian_mode, s.xtol, s.n_pools, s.multi_threading) == (0, 1, "fd", 1e-9, 4, True)
assert s.max_iter == 250 and s.tol == 1e-8 and s.p0["D3"] == 0.001 and s.bounds["D2"] == (0.002, 0.01)
assert T._SOLVER_REGISTRY["hip_curvefit"] is HipCurveFitSolver   # cached after the first resolve

cfg = os.path.join(TMP, "nnls.toml")
open(cfg, "w").write(TOMLS["nnls"])
f2 = T.load_config(cfg).build_fitter()             # the reference's own PixelWiseFitter around the plugin solver
assert type(f2.solver) is HipNNLSSolver and isinstance(f2.solver, NNLSSolver)
assert (f2.solver.reg_order, f2.solver.mu, f2.solver.device) == (2, 0.02, 0)
np.testing.assert_array_equal(f2.solver.get_regularization_matrix().shape, (250, 250)) if _lib.device_count() else None

# a plugin fitter other than the built-in "ideal" is built as cls(solver=solver) (io/toml.py:236)
cfg = os.path.join(TMP, "ideal.toml")
open(cfg, "w").write(TOMLS["ideal"])
f3 = T.load_config(cfg).build_fitter()
assert type(f3) is HipIDEALFitter and isinstance(f3, BaseFitter) and f3.dim_steps is None

# an unsupported curve_fit argument in [Fitting.solver] is refused at construction, not dropped
bad = os.path.join(TMP, "bad.toml")
open(bad, "w").write(TOMLS["bad"])
try:
    T.load_config(bad).build_fitter()
    raise SystemExit("loss='soft_l1' was accepted")
except ValueError as e:
    assert "loss" in str(e)

# no GPU here: the fit fails loudly through the reference's fitter (no CPU fallback, no oracle)
if _lib.device_count() == 0:
    b = np.linspace(0, 1200, 32)
    img = np.ones((2, 2, 1, 32))
    for f in (fitter, f2):
        try:
            f.fit(b, img)
            raise SystemExit("fit succeeded without a GPU")
        except _lib.PnxError as e:
            assert e.code == -3
assert "oracle" not in " ".join(sys.modules)
print("DROPIN-OK")
'''


# Recorder (run where Pyneapple is present, `python tests/test_plugin_dropin.py`): what the reference's loader makes of each
# TOML file -- the parsed model section and every keyword argument it hands a plugin solver / fitter constructor, or the error
# its build_fitter raises -- stored as data in tests/golden/g13_toml_plugins.json
RECORD = r"""
import json
def enc(v):
    if isinstance(v, dict):
        return {str(k): enc(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [enc(x) for x in v]
    if isinstance(v, np.ndarray):
        return enc(v.tolist())
    if isinstance(v, np.generic):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(type(v))
record = {}
REG = {"solver": T._SOLVER_REGISTRY, "fitter": T._FITTER_REGISTRY}
def recording(role, key):
    cls = T._resolve(REG[role], key)
    def make(*args, **kwargs):
        assert not args
        record[CASE][role] = {"type": key, "class": cls.__name__,
                              "kwargs": {k: enc(v) for k, v in kwargs.items() if k not in ("model", "solver")}}
        return cls(**kwargs)
    return make
for role, reg in REG.items():
    for key in [k for k, v in reg.items() if isinstance(v, EntryPoint)]:
        reg[key] = recording(role, key)
for CASE in ("tri", "nnls", "ideal", "bad"):
    path = os.path.join(TMP, CASE + ".toml")
    open(path, "w").write(TOMLS[CASE])
    c = T.load_config(path)
    record[CASE] = {"fitter_type": c.fitter_type, "model": {"type": c.model_type, "class": T._resolve(T._MODEL_REGISTRY, c.model_type).__name__,
                                                            "kwargs": enc(c.model_kwargs), "fixed_params": enc(c.fixed_params)}}
    try:
        c.build_fitter()
    except Exception as e:
        record[CASE]["error"] = {"type": type(e).__name__, "message": str(e)}
print("RECORD " + json.dumps(record, sort_keys=True))
"""

# Replay (everywhere, no Pyneapple needed): the recorded constructor calls against OUR entry points and classes, with the
# same checks the loader run makes of the plugins it builds
REPLAY = r"""
import json, os, sys
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
import numpy as np
try:
    import tomllib
except ModuleNotFoundError:
    import tomli as tomllib
from importlib.metadata import EntryPoint
with open(os.path.join(ROOT, "pyproject.toml"), "rb") as fh:
    eps = tomllib.load(fh)["project"]["entry-points"]
REG = {role: {k: EntryPoint(name=k, value=v, group=f"pyneapple.{role}s") for k, v in eps[f"pyneapple.{role}s"].items()}
       for role in ("solver", "fitter")}
assert {"hip_curvefit", "hip_nnls"} <= set(REG["solver"]) and {"hip_pixelwise", "hip_ideal"} <= set(REG["fitter"])
assert "pyneapple_amd.solvers" not in sys.modules   # entry points are metadata: nothing of the plugin imported yet
G = json.load(open(GOLDEN))

def build(case):
    rec = G[case]
    from pyneapple_amd import models as M
    kw = dict(rec["model"]["kwargs"])
    if "d_range" in kw:
        kw["d_range"] = tuple(kw["d_range"])
    if rec["model"]["fixed_params"]:
        kw["fixed_params"] = rec["model"]["fixed_params"]
    model = getattr(M, rec["model"]["class"])(**kw)
    skw = dict(rec["solver"]["kwargs"])
    if "bounds" in skw:
        skw["bounds"] = {k: tuple(v) for k, v in skw["bounds"].items()}
    cls = REG["solver"][rec["solver"]["type"]].load()
    assert cls.__name__ == rec["solver"]["class"]
    solver = cls(model=model, **skw)
    fitter = None
    if "fitter" in rec:
        fcls = REG["fitter"][rec["fitter"]["type"]].load()
        assert fcls.__name__ == rec["fitter"]["class"]
        fitter = fcls(solver=solver, **rec["fitter"]["kwargs"])
    return solver, fitter

s, fitter = build("tri")
from pyneapple_amd import _compat, _lib
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.ideal import HipIDEALFitter
from pyneapple_amd.solvers import HipCurveFitSolver, HipNNLSSolver
assert G["tri"]["fitter_type"] == "hip_pixelwise" and "error" not in G["tri"]
assert type(fitter) is HipPixelWiseFitter and issubclass(HipCurveFitSolver, _compat.CurveFitBase)
assert type(s) is HipCurveFitSolver and issubclass(HipNNLSSolver, _compat.NNLSBase)
assert (s.device, s.n_gpus, s.jacobian_mode, s.xtol, s.n_pools, s.multi_threading) == (0, 1, "fd", 1e-9, 4, True)
assert s.max_iter == 250 and s.tol == 1e-8 and s.p0["D3"] == 0.001 and s.bounds["D2"] == (0.002, 0.01)

s2, f2 = build("nnls")                               # the built-in fitter "pixelwise" around the plugin solver
assert f2 is None and G["nnls"]["fitter_type"] == "pixelwise" and "error" not in G["nnls"]
assert type(s2) is HipNNLSSolver and (s2.reg_order, s2.mu, s2.device) == (2, 0.02, 0)
np.testing.assert_array_equal(s2.get_regularization_matrix().shape, (250, 250)) if _lib.device_count() else None

_, f3 = build("ideal")
assert type(f3) is HipIDEALFitter and f3.dim_steps is None and "error" not in G["ideal"]

# the reference's build_fitter raised the plugin's ValueError for loss = "soft_l1"; so does the constructor here
assert G["bad"]["error"]["type"] == "ValueError" and "loss" in G["bad"]["error"]["message"]
try:
    build("bad")
    raise SystemExit("loss='soft_l1' was accepted")
except ValueError as e:
    assert "loss" in str(e)

# no GPU here: the fit fails loudly (no CPU fallback, no oracle)
if _lib.device_count() == 0:
    b = np.linspace(0, 1200, 32)
    img = np.ones((2, 2, 1, 32))
    for f in (fitter, HipPixelWiseFitter(solver=s2)):
        try:
            f.fit(b, img)
            raise SystemExit("fit succeeded without a GPU")
        except _lib.PnxError as e:
            assert e.code == -3
assert "oracle" not in " ".join(sys.modules)
print("REPLAY-OK")
"""

GOLDEN = os.path.join(ROOT, "tests", "golden", "g13_toml_plugins.json")


def _child(body, tmp_path):
    head = (f"REF_SRC = {REF_SRC!r}\nROOT = {ROOT!r}\nTMP = {str(tmp_path)!r}\nTOMLS = {TOMLS!r}\nGOLDEN = {GOLDEN!r}\n")
    env = dict(os.environ, PYNEAPPLE_QUIET="1", PYTHONDONTWRITEBYTECODE="1")
    return subprocess.run([sys.executable, "-c", head + textwrap.dedent(body)], capture_output=True, text=True, env=env, timeout=300)


def test_reference_toml_loader_builds_the_plugins(tmp_path):
    """The reference loader's recorded constructor calls replayed against our entry points (always), and the loader itself
    wherever Pyneapple is present."""
    r = _child(REPLAY, tmp_path)
    assert r.returncode == 0 and "REPLAY-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    if REF_SRC is not None:
        r = _child(PREAMBLE + CHECKS, tmp_path)
        assert r.returncode == 0 and "DROPIN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    # regenerate tests/golden/g13_toml_plugins.json (needs Pyneapple: installed, or PYNEAPPLE_SRC)
    import json
    import tempfile

    assert REF_SRC is not None, "Pyneapple is not installed here and PYNEAPPLE_SRC is not set"
    with tempfile.TemporaryDirectory() as tmp:
        r = _child(PREAMBLE + RECORD, tmp)
    assert r.returncode == 0, r.stderr[-4000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("RECORD ")][0][len("RECORD "):])
    with open(GOLDEN, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", GOLDEN)
