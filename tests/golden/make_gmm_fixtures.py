"""Makes tests/golden/gmm_fixture.npz: what the reference's ProbabilisticEmbedding (sisua/label_threshold.py) computes on the sets
tests.gmm_ref.FIXTURE_SETS, by EXECUTING the reference's own `_log_norm`, `normalize`, `fit` and `_predict` -- lifted out of their module
with `ast` (the module imports odin, seaborn and matplotlib at its top) and run against numpy, scipy and the installed scikit-learn (1.7.2
when this file was last run), with a stub in place of `self`.  All four could be lifted; nothing is restated here.  The fixture holds inputs
and outputs only, so that no test needs scikit-learn or the reference at run time.  Per set `s` and column `c`:
  {s}_X                      the matrix [N, 2] (tests.gmm_ref.fixture_matrix)
  {s}_c{c}_train             normalize(test_mode=False): float32, the reference takes the log1p in float32
  {s}_c{c}_arg, _sum32       the float32 argument of that log1p and the float32 column sum, as `_log_norm` formed them (read off its calls of
                             np.log1p and np.sum)
and per K in tests.gmm_ref.FIXTURE_K:
  {s}_K{K}_means, _precisions, _weights [K, 2]   of GaussianMixture(n_init=8, max_iter=120, random_state=8), components by increasing mean
  {s}_K{K}_lower_bound [2]                       its lower_bound_
  {s}_K{K}_y_prob, _y_bin [N, 2]                 predict_proba(X) and predict(X) (ci_threshold = -0.68, positive_component = 1)
Run from the repository root:  python -m tests.golden.make_gmm_fixtures <the reference's checkout>"""
import ast
import os
import sys
import warnings

import numpy as np


class RecordingNumpy:
  """numpy, keeping the last argument of log1p and the last result of sum"""

  def __init__(self):
    self.last = {}

  def __getattr__(self, name):
    return getattr(np, name)

  def log1p(self, a):
    self.last["arg"] = np.array(a)
    return np.log1p(a)

  def sum(self, a, *args, **kwargs):
    out = np.sum(a, *args, **kwargs)
    self.last["sum"] = out
    return out


def lift(tree, name, namespace, path, cls=None):
  if cls is not None:   # a method: looked for in its class alone (another class of the module has a `fit` too)
    tree = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls)
  for node in ast.walk(tree):
    if isinstance(node, ast.FunctionDef) and node.name == name:
      node.returns = None
      for a in node.args.args:
        a.annotation = None
      exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
      return namespace[name]
  raise KeyError(name)


def main(reference_root):
  import sklearn
  from scipy import stats
  from sklearn.mixture import GaussianMixture
  from tests import gmm_ref as G
  path = os.path.join(reference_root, "sisua", "label_threshold.py")
  tree = ast.parse(open(path).read())
  rec = RecordingNumpy()
  ns = dict(np=rec, stats=stats, GaussianMixture=GaussianMixture, _DummyGMM=type("_DummyGMM", (), {}))
  lift(tree, "_log_norm", ns, path)
  fns = {n: lift(tree, n, ns, path, "ProbabilisticEmbedding") for n in ("normalize", "fit", "_predict")}

  class Stub:   # what the four functions read from `self`
    def __init__(self, K):
      self.n_components_per_class, self.positive_component = K, 1
      self.remove_zeros, self.log_norm, self.clip_quartile = True, True, 0.0
      self.random_state, self.verbose, self._models = 8, False, []
    n_classes = property(lambda self: len(self._models))
    normalize, fit, _predict = fns["normalize"], fns["fit"], fns["_predict"]

  out = {"sklearn_version": np.array(sklearn.__version__)}
  for s in G.FIXTURE_SETS:
    X = G.fixture_matrix(s)
    out[f"{s}_X"] = X
    for c in range(X.shape[1]):
      out[f"{s}_c{c}_train"] = Stub(2).normalize(X[:, c], test_mode=False)
      out[f"{s}_c{c}_arg"], out[f"{s}_c{c}_sum32"] = rec.last["arg"], np.float32(rec.last["sum"])
    for K in G.FIXTURE_K:
      pbe = Stub(K)
      with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pbe.fit(X)
      srt = lambda get: np.stack([np.asarray(get(gmm)).ravel()[order] for order, gmm in pbe._models], axis=1)
      out[f"{s}_K{K}_means"], out[f"{s}_K{K}_precisions"] = srt(lambda g: g.means_), srt(lambda g: g.precisions_)
      out[f"{s}_K{K}_weights"] = srt(lambda g: g.weights_)
      out[f"{s}_K{K}_lower_bound"] = np.array([gmm.lower_bound_ for _, gmm in pbe._models], np.float64)
      out[f"{s}_K{K}_y_prob"] = pbe._predict(X, threshold=None).astype(np.float64)
      out[f"{s}_K{K}_y_bin"] = pbe._predict(X, threshold=-0.68).astype(np.float32)
      print(s, K, out[f"{s}_K{K}_means"].T, out[f"{s}_K{K}_lower_bound"])
  np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "gmm_fixture.npz"), **out)


if __name__ == "__main__":
  main(sys.argv[1])
