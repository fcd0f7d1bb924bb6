"""CPU-side checks of the drop-in boundary: the library builds, loads, exports every
symbol include/sisua_hip.h declares, and the product fails loudly without a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd import _hip
  return _hip.load()


def test_header_and_binding_agree(lib):
  from sisua_amd import _hip
  hdr = open(os.path.join(ROOT, "include", "sisua_hip.h")).read()
  hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
  declared = set(re.findall(r"\b(smx_[a-z_0-9]+)\s*\(", hdr))
  assert declared == set(_hip.SIGNATURES), declared ^ set(_hip.SIGNATURES)
  for name in declared:
    assert hasattr(lib, name)
  assert lib.smx_abi_version() == _hip.SMX_ABI_VERSION
  # the kernel-level entries of the scVI gene head (tests/test_gpu_scvi_head.py)
  assert {"smx_k_scvi_head_train", "smx_k_scvi_head_fwd", "smx_k_scvi_head_bwd"} <= declared
  # the kernel-level entry of the label heads (tests/test_gpu_label_heads.py)
  assert {"smx_k_label_loss"} <= declared and _hip.SMX_ABI_VERSION >= 19


def test_rows_convention_of_the_header():
  """One entry per operation for a host matrix that is dense or CSR (the rows convention at the top of include/sisua_hip.h): no `_csr`
  twins, and wherever a declaration takes a CSR triple of float32 values -- `indptr, cols, vals`, bare or under one prefix (t_, o_, v_)
  -- the triple follows a `const float*` parameter, the dense form of the same matrix, directly and in that order.  The two device STORES
  filled from CSR, smx_dataset_upload_csr / _csr_dense, are the only entries named after the form and the only ones that take a triple
  alone: they differ from smx_dataset_upload by store, not by input form.  Graph entries (t-SNE, UMAP, Louvain: `indptr, cols` and
  float64 weights of an n x n graph) hold no such matrix; a declaration that names `indptr` without `cols, vals` behind it must be one
  of them, with no `const float*` matrix to pair it with."""
  hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sisua_hip.h")).read(), flags=re.S)
  decls = {name: [p.strip() for p in params.split(",")] for name, params in re.findall(r"\b(smx_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", hdr)}
  stores = {"smx_dataset_upload_csr", "smx_dataset_upload_csr_dense"}
  assert {n for n in decls if n.endswith("_csr") or "_csr_" in n} == stores
  pname = lambda p: re.split(r"[\s*]+", p)[-1]
  ptype = lambda p: " ".join(p[:len(p) - len(pname(p))].replace("*", " * ").split())
  seen = set()
  for name, params in decls.items():
    names = [pname(p) for p in params]
    for i, n in enumerate(names):
      if not n.endswith("indptr"):
        continue
      pre = n[:-len("indptr")]
      assert pre in ("", "t_", "o_", "v_"), (name, n)
      if names[i + 1:i + 3] != [pre + "cols", pre + "vals"]:   # a graph, not a count matrix
        assert pre == "" and names[i + 1] == "cols" and ptype(params[i + 2]) == "const double *", (name, params)
        assert not any(ptype(p) == "const float *" for p in params), (name, params)
        continue
      assert [ptype(p) for p in params[i:i + 3]] == ["const int64_t *", "const int32_t *", "const float *"], (name, params)
      if name in stores:
        continue
      assert i >= 1 and ptype(params[i - 1]) == "const float *" and not pname(params[i - 1]).endswith("vals"), (name, params)
      seen.add(name)
  assert {"smx_predict", "smx_predict_stat", "smx_predict_sample", "smx_predict_stat_cols", "smx_predict_impute", "smx_predict_correlate",
          "smx_marginal_llk", "smx_prep_stats", "smx_gbt_fit"} <= seen


def test_config_struct_layout_matches_header(tmp_path):
  """sizeof / offsetof of every field of smx_config and smx_metrics as gcc lays include/sisua_hip.h out == the ctypes
  mirror in sisua_amd/_hip.py."""
  import ctypes as C
  import subprocess
  from sisua_amd import _hip
  lines = []
  for st in ("smx_config", "smx_metrics"):
    lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
    for name, _ in getattr(_hip, st)._fields_:
      lines.append(f'printf("{st}.{name} %zu\\n", offsetof({st}, {name}));')
  src = tmp_path / "layout.c"
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sisua_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
  for st in ("smx_config", "smx_metrics"):
    cls = getattr(_hip, st)
    assert int(got[st]) == C.sizeof(cls), st
    for name, _ in cls._fields_:
      assert int(got[f"{st}.{name}"]) == getattr(cls, name).offset, (st, name)


def _gcc_layout(tmp_path, structs):
  """sizeof / offsetof of the named structures' fields as gcc lays include/sisua_hip.h out: {'smx_config': size, 'smx_config.field': offset}"""
  import subprocess
  lines = []
  for st, fields in structs.items():
    lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
    lines += [f'printf("{st}.{name} %zu\\n", offsetof({st}, {name}));' for name in fields]
  src = tmp_path / "layout2.c"
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sisua_hip.h"\nint main(void) {\n' + "\n".join(lines) +
                 '\nprintf("abi %d\\n", SMX_ABI_VERSION);\nreturn 0; }\n')
  exe = tmp_path / "layout2"
  subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  return {k: int(v) for k, v in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}


def test_integration_snippet_matches_header(tmp_path):
  """The ctypes stub a maintainer copies from INTEGRATION.md section B is the header's layout: the fenced structure block is
  executed, and sizeof / EVERY field offset / the ABI version are compared with what gcc makes of include/sisua_hip.h (a stale
  stub mis-offsets every later field silently, VERDICT r02 row b).  The block is generated (tools/gen_integration_stub.py);
  the generator's --check mode must agree, and the field NAMES must be exactly the header's, in order."""
  import ctypes as C
  import subprocess
  import sys
  doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
  m = re.search(r"<!-- stub:structs:begin.*?-->\s*```python\n(.*?)```\s*<!-- stub:structs:end -->", doc, flags=re.S)
  assert m, "INTEGRATION.md lost its generated structure block"
  ns = {}
  exec(m.group(1), ns)
  structs = {st: [n for n, _ in ns[st]._fields_] for st in ("smx_config", "smx_metrics")}
  got = _gcc_layout(tmp_path, structs)
  assert ns["SMX_ABI_VERSION"] == got["abi"]
  for st, fields in structs.items():
    assert C.sizeof(ns[st]) == got[st], st
    for name in fields:
      assert getattr(ns[st], name).offset == got[f"{st}.{name}"], (st, name)
  # same fields as the binding the product uses, and no literal version left in the usage example
  from sisua_amd import _hip
  for st in structs:
    assert structs[st] == [n for n, _ in getattr(_hip, st)._fields_], st
  usage = doc[m.end():]
  assert "abi_version=SMX_ABI_VERSION" in usage and not re.search(r"abi_version\s*=\s*\d", usage)
  r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_integration_stub.py"), "--check"], capture_output=True, text=True)
  assert r.returncode == 0, r.stderr + r.stdout


def test_no_cpu_fallback(lib):
  from sisua_amd import _hip
  from sisua_amd.config import ModelConfig
  from sisua_amd.engine import Engine
  if lib.smx_device_count() > 0:
    pytest.skip("a GPU is visible")
  with pytest.raises(_hip.SmxError):
    Engine(ModelConfig(n_genes=8, enc_units=(4,), dec_units=(4,), latent_dim=2))
  assert lib.smx_init(0) != 0
  assert b"no such HIP device" in lib.smx_last_error()


def test_manifest_and_init_match_oracle():
  from oracle import sisua_oracle as so
  from sisua_amd import config
  from tests.util import make_pair
  for kw in (dict(model="vae", n_genes=50, likelihood="zinb", enc_units=(16,), dec_units=(16, 8), latent_dim=5),
             dict(model="scvi", n_genes=33, likelihood="zinbd", enc_units=(8,), dec_units=(8,), latent_dim=3, encl_units=(4,)),
             dict(model="sisua", n_genes=20, likelihood="nb", enc_units=(8,), dec_units=(8,), latent_dim=3,
                  labels=((5, "nb"), (3, "onehot")), batchnorm=False),
             dict(model="dca", n_genes=20, likelihood="nbd", enc_units=(8,), dec_units=(8,), latent_dim=3),
             dict(model="scale", n_genes=20, likelihood="zinb", enc_units=(8,), dec_units=(8,), latent_dim=3, n_components=5),
             dict(model="scale", n_genes=20, likelihood="zinb", enc_units=(8,), dec_units=(8,), latent_dim=3, n_components=4, tie_loc=True, tie_mixtures=True),
             dict(model="scale", n_genes=20, likelihood="zinb", enc_units=(8,), dec_units=(8,), latent_dim=3, n_components=4, covariance="tril"),
             dict(model="scale", n_genes=20, likelihood="zinb", enc_units=(8,), dec_units=(8,), latent_dim=4, n_components=3, latent_mixture=True),
             dict(model="sisua", n_genes=20, likelihood="zinb", enc_units=(8,), dec_units=(8,), latent_dim=3, labels=((5, "mixnb3"),)),
             dict(model="sisua", n_genes=20, likelihood="nb", enc_units=(8,), dec_units=(8,), latent_dim=3, labels=((4, "mixgauss2"), (3, "nb"))),
             dict(model="sisua", n_genes=20, likelihood="nb", enc_units=(8,), dec_units=(8,), latent_dim=3, labels=((4, "mixtril2"), (3, "nb"))),
             dict(model="sisua", n_genes=20, likelihood="nb", enc_units=(8,), dec_units=(8,), latent_dim=3, labels=((4, "mixzinb3"),)),
             dict(model="fvae", n_genes=20, likelihood="zinb", enc_units=(8,), dec_units=(8,), latent_dim=3, disc_units=12, disc_layers=2),
             dict(model="fvae", n_genes=20, likelihood="nb", enc_units=(8,), dec_units=(8,), latent_dim=3, disc_units=12, disc_layers=1,
                  labels=((4, "onehot"),))):
    spec, cfg = make_pair(**kw)
    assert config.manifest(cfg) == so.manifest(spec)
    a, b = config.init_params(cfg), so.init_params(spec)
    assert list(a) == list(b)
    for k in a:
      assert np.array_equal(a[k].astype(np.float64), b[k])
