"""The product-accuracy tests are sensitive: on the CPU, with the NumPy emulation of tests/product_ref.py, every dropped or
mis-paired cross product of the bf16 x 3 arithmetic trips the bounds that tests/test_gpu_product_accuracy.py holds the kernels
to -- at every shape and every probe group used there.  (To see it fail: edit product_ref.SIX_TERMS.)"""
import numpy as np
import pytest

from tests import product_ref as pr

PROBE_ALLOWED_ULP = 4.0     # what the GPU test allows
PROBE_MOVED_ULP = 8.0       # what a wrong term list has to move every element by


def test_bf16_rounding_and_split():
  x = np.array([1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415927, 1e-30, 3.3e38, 0.0], np.float32)
  # ties to even: 1 + 2^-8 is halfway between 1 and 1 + 2^-7 -> 1 (even); 1 + 3 2^-8 is halfway between 1 + 2^-7 and 1 + 2^-6 -> 1 + 2^-6
  assert pr.bf16_rne(x)[:4].tolist() == [1.0, 1.0, 1.015625, 1.0078125]
  assert (pr.bf16_rne(x).view(np.uint32) & 0xFFFF == 0).all()
  t0, t1, t2 = pr.split3(x)
  rest = x.astype(np.float64) - t0 - t1 - t2
  assert (np.abs(rest) <= 2.0 ** -24 * np.abs(x)).all()          # three bf16 terms leave less than half a float32 ulp
  assert np.isinf(pr.bf16_rne(np.array([3.4e38], np.float32))[0]) and np.isnan(pr.split3(np.array([3.4e38], np.float32))[2][0])
  assert np.isnan(pr.bf16_rne(np.array([np.nan], np.float32))[0])


def test_six_terms_are_the_kernels():
  """the term list is mfma_bf16x3's, read from the source"""
  import os
  import re
  src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sisua_amd", "csrc", "smx_device.h")).read()
  body = src[src.index("mfma_bf16x3(const Split8& a"):]
  body = body[:body.index("return acc;")]
  assert tuple((int(i), int(j)) for i, j in re.findall(r"bf16\(a\.t(\d), b\.t(\d), acc", body)) == pr.SIX_TERMS


@pytest.mark.parametrize("shape", pr.shapes_used(), ids=lambda s: "x".join(map(str, s)))
def test_term_probe_separates_right_from_wrong(shape):
  """six terms: within 1 ulp of float64 at every element (the GPU test allows 4); any term dropped, or issued twice in
  place of its mirror: every element moves by at least 8 ulp -- for every probe group of every form at this shape"""
  M, N, K = shape
  groups = {tuple(g) for f in pr.forms() if f[5] == shape for g in pr.probe_groups(K, f[6])}
  assert groups
  wrong = [pr.dropped(t) for t in pr.SIX_TERMS] + [pr.mispaired(t) for t in pr.MIRRORED]
  assert len({w for w in wrong}) == 10
  for gi, ks in enumerate(sorted(groups)):
    A, B = pr.term_probe(M, N, K, ks, seed=gi)
    assert (np.count_nonzero(A, axis=1) == pr.PROBE_POSITIONS).all() and (np.count_nonzero(B, axis=0) == pr.PROBE_POSITIONS).all()
    A, B = A[:, list(ks)], B[list(ks), :]                       # (the other k are zero)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    ulp = pr.ulp32(ref)
    assert (ulp == 2.0 ** -20).all()
    assert (np.abs(pr.emulate(A, B) - ref) <= 1.0 * ulp).all()
    for terms in wrong:
      moved = np.abs(pr.emulate(A, B, terms) - ref) / ulp
      assert moved.min() >= PROBE_MOVED_ULP, (ks, terms, moved.min())
      assert moved.min() - 1.0 > PROBE_ALLOWED_ULP     # ... which stays out of reach of the allowance


@pytest.mark.parametrize("scaled", [False, True], ids=["normal", "scaled"])
@pytest.mark.parametrize("shape", pr.shapes_used(), ids=lambda s: "x".join(map(str, s)))
def test_a_dropped_term_is_three_bounds_away(shape, scaled):
  """random operands: the six-term arithmetic sits far inside the bound, and every dropped term (e_drop is the smallest of
  the six) and every mis-paired one at least 3 times over it"""
  M, N, K = shape
  A, B = pr.random_operands(M, N, K, seed=K + M, scaled=scaled)
  ref, e_seq, e_drop = pr.errors(A, B)
  bound = pr.bound(e_seq, e_drop)
  assert bound <= min(2.0 * e_seq, 0.5 * e_drop)
  assert pr.rel_fro(pr.emulate(A, B), ref) <= 0.1 * bound
  assert e_drop >= 3.0 * bound
  for t in pr.SIX_TERMS:
    assert pr.rel_fro(pr.emulate(A, B, pr.dropped(t)), ref) >= 3.0 * bound, t
  for t in pr.MIRRORED:
    assert pr.rel_fro(pr.emulate(A, B, pr.mispaired(t)), ref) >= 3.0 * bound, t


def test_rank_one_and_head_shaped_products_are_sensitive_too():
  """the fused head's two products as the GPU test takes them: a rank-1 weight gradient (K = 1) and a one-row decoder
  gradient over K = k G; operands shaped like the head's (a rectified decoder row, sparse likelihood gradients, 0.08 N(0, 1) weights)"""
  rng = np.random.default_rng(0)
  d = np.maximum(rng.normal(size=(128, 1)), 0).astype(np.float32)
  dP = (rng.normal(size=(1, 3 * 4128)) * (rng.uniform(size=(1, 3 * 4128)) < 0.3) / 128).astype(np.float32)
  W = (rng.normal(size=(3 * 4128, 128)) * 0.08).astype(np.float32)
  for A, B in ((d, dP), (dP, W)):
    ref, e_seq, e_drop = pr.errors(A, B)
    bound = pr.bound(e_seq, e_drop)
    assert pr.rel_fro(pr.emulate(A, B), ref) <= 0.25 * bound     # (the weight gradient is stored as float32: one rounding on top, in the GPU test)
    assert e_drop >= 3.0 * bound


def test_split_commutes_with_powers_of_two_down_to_its_floor():
  """2^p split3(x) == split3(2^p x) while |2^p x| >= 2^-103 (t2 normal), and not below"""
  rng = np.random.default_rng(1)
  x = (rng.choice([-1.0, 1.0], size=4096) * np.exp2(rng.uniform(-3, 3, size=4096))).astype(np.float32)
  base = pr.split3(x)
  for p in (40, -60, -90, 100, -100):
    for t, s in zip(base, pr.split3(np.ldexp(x, p).astype(np.float32))):
      assert np.array_equal(np.ldexp(t.astype(np.float64), p), s.astype(np.float64)), p
  assert int(np.floor(np.log2(np.abs(np.ldexp(x, -100)).min()))) == pr.SPLIT_MIN_EXPONENT
  # one binade lower the smallest remainder is a subnormal, which only a bf16 path that keeps subnormals carries; from 2^-111 down the
  # bf16 subnormal grid (2^-133) cannot hold it at all
  y = np.array([2.0 ** -104 * (1 + 2.0 ** -23)], np.float32)
  assert any(0 < abs(float(t[0])) < 2.0 ** -126 for t in pr.split3(y))
  z = np.array([2.0 ** -111 * (1 + 2.0 ** -23)], np.float32)
  assert sum(float(t[0]) for t in pr.split3(z)) != float(z[0])


def test_positions_cover_what_the_kernels_split_k_by():
  """the probes' k positions: first and last k of a 16-deep step and of a 32-deep stage, both sides of every slice or chunk
  boundary, every wave's share, the ragged end"""
  for name, tile, ta, tb, S, (M, N, K), pos in pr.forms():
    got = {k for g in pr.probe_groups(K, pos) for k in g}
    assert all(len(g) == pr.PROBE_POSITIONS == len(set(g)) and max(g) < K for g in pr.probe_groups(K, pos))
    assert {0, K - 1} <= got
    if name == "lds":
      bk = 32 * {1: 1, 2: 1, 3: 1, 4: 4, 5: 2}.get(tile, 4)
      chunk = -(-(-(-K // S)) // bk) * bk
      assert {k for b in range(chunk, K, chunk) for k in (b - 1, b)} <= got
      assert {k for k in (31, 32, 63, 64, 95, 96, 127) if k < K} <= got          # every wave's 32-deep block of the first tile
    elif name == "dgemm":
      assert {k for q in range(8) for k in (32 * q, 32 * q + 15, 32 * q + 16, 32 * q + 31)} <= got
      assert {k for b in range(256, K, 256) for k in (b - 1, b)} <= got
    elif name in ("wgrad", "panel"):
      assert {k for q in range(8) for k in (16 * q, 16 * q + 15) if k < K} <= got
      assert {k for b in range(128, K, 128) for k in (b - 1, b)} <= got
    else:
      n, chunk = pr.bigk_slices((K + 31) // 32 * 32)
      assert {chunk - 1, chunk, 16 * chunk - 1, 16 * chunk, (n - 1) * chunk - 1, (n - 1) * chunk} <= got
      assert {z for z in range(16)} <= {k // chunk for k in got}                 # every reduce thread's first slice
