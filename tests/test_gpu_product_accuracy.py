"""The matrix-product kernels held to the float32 accuracy they claim.  Needs a real MI355X.

Every form reachable through smx_k_gemm -- the LDS-tiled float32-MFMA kernel (tiles 0-5, smx_gemm.hip) and the bf16 x 3 forms
(tile 100 smx_dgemm.h, 101 the 32 x 32-tile weight gradient of smx_headbwd.hip, 102 smx_panel.h, 103 smx_bigk.hip) -- and the two
products of the fused output head (smx_headfused.hip), against float64.  The reference arithmetic, the shapes, the probes' k
positions (with the source lines they come from) and the bound are in tests/product_ref.py; tests/test_product_accuracy_host.py
shows on the CPU that a dropped or mis-paired cross product of the bf16 x 3 arithmetic trips every bound used here.

The contract these tests state ("What the products promise"):
  * domain of the bf16 x 3 forms: an operand is zero or 2^-103 <= |x| < 2^127.  Below 2^-103 the third term of the split
    (as small as ulp_f32(x) = 2^(e - 23)) is a subnormal and what the conversion and the MFMA do with it is not promised: the
    result stays finite and loses at most K 2^-126 max|other operand| per element.  From 3.39e38 (the largest bf16 plus half a
    bf16 ulp, 0x7F7F8000) up, x rounds to a bf16 infinity, the split's remainder is -inf and then NaN: such an operand counts
    as non-finite, and is not tested as a finite one.  The float32-MFMA tiles take every finite float.
  * a NaN or an infinity in A's row i (B's column j) makes row i (column j) of C non-finite and changes no other bit of C.
  * C(2^p A, 2^q B) == 2^(p + q) C(A, B) bit for bit inside the domain (nothing overflowing or leaving the normal range).
"""
import numpy as np
import pytest

from tests import product_ref as pr

pytestmark = pytest.mark.gpu

FAMILIES = [("lds", t) for t in range(6)] + [("dgemm", 100), ("wgrad", 101), ("panel", 102), ("bigk", 103)]
_cache = {}   # float64 references, e_seq32 and e_drop per shape: computed once, shared, never modified


@pytest.fixture(scope="module")
def k_gemm():
  from sisua_amd import engine
  return engine.k_gemm


def _forms(family, first_shape_only=False):
  out, seen = [], set()
  for f in pr.forms():
    if (f[0], f[1]) != family:
      continue
    if first_shape_only and f[1:5] in seen:   # the form's first shape: the small one with a ragged last tile
      continue
    seen.add(f[1:5])
    out.append(f)
  assert out
  return out


def _name(f):
  return "%s tile %d tA=%d tB=%d split %d %s" % (f[0], f[1], f[2], f[3], f[4], f[5])


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: "%s%d" % f)
def test_term_probe(k_gemm, family):
  """known-answer operands (8 non-zero k, every entry three exact bf16 terms): |C - ref64| <= 4 ulp at every element -- the worst
  case of an exact float32 kernel that rounds once per non-zero k; the six-term arithmetic is within 1 ulp, and any dropped or
  mis-paired term moves every element by at least 8"""
  worst = {}
  for f in _forms(family):
    worst[_name(f)] = pr.probe_worst_ulp(k_gemm, f)
    print("%-60s worst %.2f ulp" % (_name(f), worst[_name(f)]))
  bad = {n: w for n, w in worst.items() if not w <= 4.0}
  assert not bad, bad


@pytest.mark.parametrize("scaled", [False, True], ids=["normal", "pow2-scaled"])
@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: "%s%d" % f)
def test_random_operands(k_gemm, family, scaled):
  """N(0, 1) operands (and rows / columns scaled by 2^-20 .. 2^20): relative Frobenius error <= min(2 e_seq32, e_drop / 3)"""
  bad = {}
  for f in _forms(family):
    e, es, ed = pr.random_figures(k_gemm, f, scaled, _cache)
    print("%-60s error %.2e  e_seq32 %.2e  e_drop %.2e  bound %.2e" % (_name(f), e, es, ed, pr.bound(es, ed)))
    if not e <= pr.bound(es, ed):
      bad[_name(f)] = (e, pr.bound(es, ed))
  assert not bad, bad


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: "%s%d" % f)
def test_power_of_two_scaling_is_exact(k_gemm, family):
  """operands of magnitude 2^-3 .. 2^3: C(2^p A, 2^q B) == 2^(p + q) C(A, B) bit for bit; (100, -100) and (-100, 100) put one
  operand's smallest magnitude at 2^-103, the floor of the split's domain"""
  bad = {}
  for f in _forms(family, first_shape_only=True):
    for p, q in pr.SCALINGS:
      n = pr.scaling_mismatches(k_gemm, f, p, q)
      if n:
        bad[(_name(f), p, q)] = n
  assert not bad, bad


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: "%s%d" % f)
def test_subnormal_operands(k_gemm, family):
  """float32 subnormals mixed into N(0, 1) operands: finite, and within the bound plus K 2^-126 max|operand| per element (a
  subnormal may be flushed)"""
  bad = {}
  for f in _forms(family, first_shape_only=True):
    finite, err, allowed = pr.subnormal_figures(k_gemm, f, _cache)
    print("%-60s ||C - ref|| %.3e allowed %.3e" % (_name(f), err, allowed))
    if not (finite and err <= allowed):
      bad[_name(f)] = (finite, err, allowed)
  assert not bad, bad


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: "%s%d" % f)
def test_wide_range_operands(k_gemm, family):
  """|A| up to 2^126 against |B| down at the bottom of the domain: finite and within the bound.  The float32-MFMA tiles take B
  at 2^-126; the bf16 x 3 forms at 2^-103 (their floor) -- at 2^-126 the split's remainders are bf16 subnormals on a grid of
  2^-133, which cannot hold them whatever the hardware does (the emulation itself errs by 5e-4 there), and finite is what holds"""
  bad = {}
  for f in _forms(family, first_shape_only=True):
    floor = -126 if f[0] == "lds" else pr.SPLIT_MIN_EXPONENT
    e, es, ed = pr.wide_range_figures(k_gemm, f, floor, _cache)
    print("%-60s |B| >= 2^%d: error %.2e bound %.2e" % (_name(f), floor, e, pr.bound(es, ed)))
    if not e <= pr.bound(es, ed):
      bad[_name(f)] = (floor, e, pr.bound(es, ed))
    if floor != -126:
      e, _, _ = pr.wide_range_figures(k_gemm, f, -126, _cache)
      print("%-60s |B| >= 2^-126: error %.2e (finite is asserted)" % (_name(f), e))
      if not np.isfinite(e):
        bad[_name(f) + " at 2^-126"] = e
  assert not bad, bad


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: "%s%d" % f)
def test_non_finite_values_stay_in_their_line(k_gemm, family):
  """a NaN, then +inf, in one element of A's row i / B's column j (first tile and last, ragged tile): that row / column of C is
  non-finite throughout, every other element keeps the bits of the clean run (the step's nan_flag relies on it)"""
  bad = {}
  for f in _forms(family, first_shape_only=True):
    for what, line, rest in pr.containment(k_gemm, f):
      if not (line and rest):
        bad[(_name(f), what)] = (line, rest)
  assert not bad, bad


@pytest.mark.parametrize("b_star", pr.HEAD_ROWS)
@pytest.mark.parametrize("lk,k", [("zinb", 3), ("nbd", 2)])
def test_fused_head_products_isolated_from_the_likelihood(lk, k, b_star):
  """smx_k_head_fused at G = 4128.  Launch 1: 128 cells, d zero in every row but b*; launch 2: that cell alone, same grad_scale --
  its db is the cell's dP as the kernel computes it.  dW of launch 1 against the float64 outer product d[b*] (x) db2, and dd of
  launch 2 against the float64 db2 W^T (K = k G): relative Frobenius error <= min(2 e_seq32, e_drop / 3) of that product."""
  from sisua_amd import engine
  h = pr.head_figures(engine.k_head_fused, lk, k, b_star)
  for which in ("dW", "dd"):
    e, es, ed = h[which]
    print("%s b* = %d %s: error %.2e  e_seq32 %.2e  e_drop %.2e  bound %.2e" % (lk, b_star, which, e, es, ed, pr.bound(es, ed)))
  assert h["finite"]
  for which in ("dW", "dd"):
    e, es, ed = h[which]
    assert e <= pr.bound(es, ed), (which, e, es, ed)
