"""CPU checks of tests/scvi_head_ref.py: the reference against float64 autograd of the same chain, the two caps (grid condition, undecided
genes) for every launch tests/test_gpu_scvi_head.py makes, every bound positive and finite where the condition holds, the launchers'
thresholds as the module restates them, and `rel_in=None` leaving likelihood_grad_ref's bounds as they were."""
import os
import re

import numpy as np
import pytest

from tests import likelihood_grad_ref as L
from tests import scvi_head_ref as R
from tests.plane_stat_ref import EPS, logprob_elem_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(c, kind, G):
  Gp = R.round_up(G, 32)
  n_add = R.n_add_train(Gp) if R.train_instance(Gp) else R.n_add_sep(Gp)
  B = c["raw"].shape[0]
  return R.head(kind, c["raw"], c["x"], c["l"].astype(np.float64), c["clip"], np.float32(-1.0 / B), n_add)


def test_thresholds_match_the_launchers():
  """the `Gp <=` ladders of launch_scvi_head_train / _fwd / _bwd and scvi_head_train_supported's limit are the ones scvi_head_ref restates"""
  src = open(os.path.join(ROOT, "sisua_amd", "csrc", "smx_scvi.hip")).read()

  def ladder(name):
    body = src[src.index(f"int {name}("):]
    body = body[:body.index("\n}\n")]
    return [int(v) for v in re.findall(r"a\.Gp <= (\d+)", body)]
  assert ladder("launch_scvi_head_train") == [2048, 4096, 8192, 16384]
  assert ladder("launch_scvi_head_fwd") == [2048, 4096, 8192] and ladder("launch_scvi_head_bwd") == [2048, 4096, 8192]
  assert re.search(r"a\.Gp <= (\d+)", src[src.index("bool scvi_head_train_supported"):]).group(1) == str(R.TRAIN_MAX_GP)
  for top, inst in ((2048, (2, 256)), (4096, (4, 256)), (8192, (8, 256)), (16384, (8, 512)), (20480, (10, 512))):
    assert R.train_instance(top) == inst and R.train_instance(top + 32) != inst
  assert R.train_instance(20512) is None and [R.sep_instance(v) for v in (2048, 2080, 4096, 4128, 8192, 8224)] == [2, 4, 4, 8, 8, 0]
  assert [R.n_add_train(v) for v in (32, 4096, 8192, 16384, 20480)] == [17, 25, 41, 45, 53]
  assert [R.n_add_sep(v) for v in (32, 4096, 8192, 8224, 20480, 20512)] == [17, 25, 41, 33, 41, 45]
  # every width of the GPU file is the smallest or the largest G of an instance
  assert sorted({R.round_up(G, 32) for G in R.WIDTHS} & {2048, 4096, 8192, 16384, 20480}) == [2048, 4096, 8192, 16384, 20480]
  assert {2049, 4097, 8193, 16385, 20481} <= set(R.WIDTHS)


@pytest.mark.parametrize("G", R.WIDTHS)
def test_caps_and_bounds_of_every_gpu_launch(G):
  """at most a tenth of a launch's live elements fail the grid condition, at most 1 % are undecided, no row fails whole, l is never
  undecided; every bound is positive and finite (dl's exactly 0 outside the library clip), every reference finite"""
  for kind in R.KINDS:
    seen = set()
    for c in R.launches(G, kind):
      h = _head(c, kind, G)
      fail, und = R.caps(h)
      print(f"{c['name']}: {int((~h['keep']).sum())} of {h['keep'].size} fail the grid condition, {int(h['und'].sum())} undecided")
      assert fail <= 0.1 and und <= 0.01, (c["name"], fail, und)
      assert h["keep"].any(axis=-1).all() and not h["f"]["l_und"].any(), c["name"]
      assert c["x"].max() <= 65535 and np.array_equal(c["x"], np.floor(c["x"])), c["name"]
      for key in ("draw", "draw_alt", "llk", "dl", "dplanes"):
        assert np.isfinite(h[key]).all(), (c["name"], key)
      keep3 = np.broadcast_to(h["keep"][:, None, :], h["E_draw"].shape)
      assert np.isfinite(h["E_draw"]).all() and (h["E_draw"][keep3] > 0).all(), c["name"]
      assert np.isfinite(h["E_llk"]).all() and (h["E_llk"] > 0).all() and np.isfinite(h["E_s"]).all() and (h["E_s"] > 0).all(), c["name"]
      lin = h["f"]["l_in"]
      assert (h["E_dl"][lin] > 0).all() and np.isfinite(h["E_dl"]).all() and not h["E_dl"][~lin].any() and not h["dl"][~lin].any(), c["name"]
      f = R.forward(c["raw"], c["l"].astype(np.float64), c["clip"], R.n_add_sep(R.round_up(G, 32)))
      for key in ("E_rho", "E_rate", "E_theta"):
        assert np.isfinite(f[key]).all() and (f[key] > 0).all(), (c["name"], key)
      with np.errstate(over="ignore"):
        pl = np.stack([h["f"]["rate"], h["f"]["theta"]], axis=1).astype(np.float32)
      r = R.backward_entry(pl, h["dplanes"][:, :2].astype(np.float32), h["f"]["rho"].astype(np.float32), c["l"], c["clip"], R.n_add_sep(R.round_up(G, 32)))
      assert np.isfinite(pl).all() and np.isfinite(r["E_draw"]).all() and (r["E_draw"][:, 0] > 0).all() and np.isfinite(r["draw"]).all(), c["name"]
      lb = R.library(c["l"].astype(np.float64), R.S_RAW, 0.0, R.library_rows(len(lin))[:, 0], R.library_rows(len(lin))[:, 1], R.KLS, h["dl"], h["E_dl"])
      for key in ("sig", "kl", "dlatl0", "dlatl1"):
        assert np.isfinite(lb[key]).all() and np.isfinite(lb["E_" + key]).all() and (lb["E_" + key] > 0).all(), (c["name"], key)
      seen |= set(c["labels"])
    want = {"moderate", "flat", "dispersion and gate", "library edge l -3", "library edge l 0", "library edge l 11", "library edge l 5.5 clip 6",
            "library edge l 6 clip 6", "library edge l 7 clip 6"}
    if G >= 128:
      want |= {"spike"}
    if G >= 12:
      want |= {f"straddle {k}" for k in ((4, 8, 12, 16, 20) if G >= 512 else (4, 8, 12, 16))}
    assert want <= seen, (G, kind, want - seen)


def test_straddle_and_spike_rows_do_what_they_are_for():
  """the straddle rows put decided genes on both sides of both thresholds and a few undecided ones; the spike gene is at the high clip and
  every other gene of its row at the low one"""
  for G in (2049, 20480):
    h = {c["name"]: (c, _head(c, "nbd", G)) for c in R.launches(G, "nbd")}
    rows = {lab: (hh, i) for c, hh in h.values() for i, lab in enumerate(c["labels"])}
    hh, i = rows["spike"]
    rho = hh["f"]["rho"][i]
    assert (rho >= R.HI).sum() == 1 and (rho < R.LO).sum() == G - 1 and not hh["f"]["inside"][i].any()
    hh, i = rows["straddle 4"]
    rho, und = hh["f"]["rho"][i][1:11], hh["und"][i][1:11]
    assert ((rho > R.LO) & ~und).sum() >= 4 and ((rho < R.LO) & ~und).sum() >= 4 and 1 <= und.sum() <= 4
    for k in (4, 8, 12, 16):
      hh, i = rows[f"straddle {k}"]
      assert hh["f"]["inside"][i][0] and not hh["und"][i][0] and abs(hh["f"]["rho"][i][0] / (R.HI * (1 - 2.0 ** -k)) - 1) < 1e-6


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_against_float64_autograd(kind):
  """the moderate rows: d raw, dl and the likelihood from torch's float64 autograd of the same chain, to 1e-10 of the term sizes"""
  import torch
  for G in (37, 2049):
    for c in R.launches(G, kind):
      rows = [i for i, lab in enumerate(c["labels"]) if lab == "moderate"]
      if not rows:
        continue
      h = _head(c, kind, G)
      gs = float(np.float32(-1.0 / c["raw"].shape[0]))
      raw = torch.tensor(c["raw"][rows].astype(np.float64), requires_grad=True)
      l = torch.tensor(c["l"][rows].astype(np.float64), requires_grad=True)
      x = torch.tensor(c["x"][rows].astype(np.float64))
      rho = torch.softmax(raw[:, 0], dim=-1)
      rate = torch.exp(torch.clamp(l, 0.0, float(np.float32(c["clip"]))))[:, None] * torch.clamp(rho, R.LO, R.HI)
      th = torch.exp(raw[:, 1])
      ell = (torch.lgamma(x + th) - torch.lgamma(th) - th * torch.log1p(rate / (th + EPS)) - x * torch.log1p(th / (rate + EPS)))
      if kind == "zinbd":
        g = raw[:, 2]
        ell = torch.where(x == 0, torch.logaddexp(g, ell), ell) - torch.nn.functional.softplus(g)
      (gs * ell.sum()).backward()
      t = L.count_terms(kind, c["x"][rows], [h["f"]["rate"][rows], h["f"]["theta"][rows], h["f"]["gate"][rows]][:raw.shape[1]], direct=True, exact=True)
      f = h["f"]
      size = [np.abs(f["rho"][rows] * h["dd"][rows] * f["el"][rows]) + np.abs(f["rho"][rows] * h["s"][rows][:, None]),
              abs(gs) * f["theta"][rows] * (t["l1p"] + t["t2"] + t["c"] + t["dg"]), abs(gs) * np.ones_like(t["dg"])]
      got = raw.grad.numpy()
      for p in range(raw.shape[1]):
        assert (np.abs(got[:, p] - h["draw"][rows, p]) <= 1e-10 * (size[p] + np.abs(h["draw"][rows, p]))).all(), (c["name"], p)
      inside = f["l_in"][rows]
      sz = np.abs(h["dd"][rows] * f["rate"][rows]).sum(-1)
      assert (np.abs(l.grad.numpy() - h["dl"][rows]) <= 1e-10 * sz).all() and not l.grad.numpy()[~inside].any(), c["name"]
      assert (np.abs(ell.detach().numpy().sum(-1) - h["llk"][rows]) <= 1e-10 * np.abs(ell.detach().numpy()).sum(-1)).all(), c["name"]


def test_rel_in_none_leaves_the_bounds_as_they_were():
  """grad_elem_bound, logprob_elem_bound and row_sum_bound with rel_in=None (the default) and with (0, 0) give the bits of the call without
  it, on the direct grids of both kinds; a non-zero rel_in only raises a bound"""
  for kind in R.KINDS:
    x, planes, keep = L.grid_elements(kind, direct=True)
    a = L.grad_elem_bound(kind, x, planes, True)
    for b in (L.grad_elem_bound(kind, x, planes, True, rel_in=None), L.grad_elem_bound(kind, x, planes, direct=True, rel_in=(0.0, 0.0)),
              L.grad_elem_bound(kind, x, planes, True, None, False)):
      assert np.array_equal(a, b, equal_nan=True)
    up = L.grad_elem_bound(kind, x, planes, True, rel_in=(3.0, 5.0))
    k3 = np.broadcast_to(keep, a.shape)
    assert (up[k3] >= a[k3]).all() and (up[:2][k3[:2]] > a[:2][k3[:2]]).any()
    p = logprob_elem_bound(kind, x, planes, True)
    assert np.array_equal(p, logprob_elem_bound(kind, x, planes, True, rel_in=None), equal_nan=True)
    assert np.array_equal(p, logprob_elem_bound(kind, x, planes, True, rel_in=(0.0, 0.0)), equal_nan=True)
    r0, r1 = L.row_sum_bound(kind, x, planes, 17, direct=True), L.row_sum_bound(kind, x, planes, 17, direct=True, rel_in=None, exact=False)
    assert np.array_equal(r0[0], r1[0], equal_nan=True) and np.array_equal(r0[1], r1[1], equal_nan=True)
    # float32 planes: `exact` changes nothing
    e = L.grad_elem(kind, x, planes, True, exact=True)
    assert np.array_equal(e, L.grad_elem(kind, x, planes, True), equal_nan=True)
