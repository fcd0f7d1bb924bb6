"""sisua_amd.engine is a package of one module per kernel family, and still the one namespace its callers and the host tests reach and
patch: every name, signature and constant recorded in tests/golden/engine_api.json (written from the single-file engine.py the package
replaced; later features add their entries) resolves here unchanged.  No device."""
import ctypes as C
import inspect
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from sisua_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "engine_api.json")) as f:
  API = json.load(f)


def test_fixture_holds_the_whole_single_file_namespace():
  assert len(API["callables"]) >= 77 and len(API["constants"]) >= 31 and len(API["engine_methods"]) >= 72
  assert {"SmxError", "check", "smx_config", "smx_metrics"} <= set(API["imported"])


def test_every_recorded_name_resolves_and_is_no_module():
  names = list(API["callables"]) + list(API["constants"]) + list(API["imported"])
  missing = [n for n in names if not hasattr(engine, n)]
  assert not missing, missing
  shadowed = [n for n in names if isinstance(getattr(engine, n), types.ModuleType)]
  assert not shadowed, shadowed


def test_signatures_and_constants_are_the_recorded_ones():
  got = {n: str(inspect.signature(getattr(engine, n))) for n in API["callables"]}
  assert got == API["callables"]
  assert {n: repr(getattr(engine, n)) for n in API["constants"]} == API["constants"]


def _describe(member):
  if isinstance(member, staticmethod):
    return "staticmethod" + str(inspect.signature(member.__func__))
  if isinstance(member, property):
    return "property"
  if callable(member):
    return str(inspect.signature(member))
  return "constant " + repr(member)


def test_engine_methods_are_the_recorded_ones():
  members = vars(engine.Engine)
  missing = [n for n in API["engine_methods"] if n not in members]
  assert not missing, missing
  assert {n: _describe(members[n]) for n in API["engine_methods"]} == API["engine_methods"]


def test_every_submodule_is_private():
  files = [f for f in os.listdir(os.path.dirname(engine.__file__)) if f.endswith(".py")]
  assert len(files) > 2 and all(f.startswith("_") for f in files), files
  exported = set(API["callables"]) | set(API["constants"]) | set(API["imported"])
  assert not {f[:-3] for f in files} & exported


def test_import_needs_no_device_and_stays_light():
  """In a fresh interpreter.  sisua_amd/__init__.py imports the whole operator surface (scipy.sparse and sisua_amd.data with it), so the child
  stands an empty package in for it: what is then in sys.modules is what the engine package's own imports brought."""
  code = ("import sys, types\npkg = types.ModuleType('sisua_amd')\npkg.__path__ = [%r]\nsys.modules['sisua_amd'] = pkg\n"
          "import sisua_amd.engine\nfrom sisua_amd import _hip\nassert sisua_amd.engine.Engine and sisua_amd.engine.k_prep_apply\n"
          % os.path.join(ROOT, "sisua_amd") +
          "assert _hip._lib is None, 'the library was loaded'\n"
          "heavy = [m for m in ('scipy.sparse', 'sisua_amd.data') if m in sys.modules]\nassert not heavy, heavy\n")
  env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
  run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
  assert run.returncode == 0, run.stderr


@pytest.mark.parametrize("dtype, ctype", [(np.float32, C.c_float), (np.float64, C.c_double), (np.int32, C.c_int32), (np.int64, C.c_int64),
                                          (np.uint8, C.c_uint8), (np.uint16, C.c_uint16)])
def test_ptr_is_typed_by_the_dtype(dtype, ctype):
  a = np.arange(3).astype(dtype)
  p = engine._ptr(a)
  assert type(p) is C.POINTER(ctype)
  assert C.addressof(p.contents) == a.ctypes.data and p[2] == a[2]


def test_ptr_refuses_what_it_has_no_type_for():
  assert engine._ptr(None) is None
  with pytest.raises(TypeError):
    engine._ptr(np.zeros(2, np.float16))


def test_typed_converters_refuse_another_dtype():
  with pytest.raises(TypeError):
    engine._fp(np.zeros(2, np.float64))   # (used to reinterpret the eight-byte words as floats)
  with pytest.raises(TypeError):
    engine._ip(np.zeros(2, np.int64))
  with pytest.raises(TypeError):
    engine._dp(np.zeros(2, np.float32))
  assert engine._fp(None) is None and type(engine._fp(np.zeros(2, np.float32))) is C.POINTER(C.c_float)
