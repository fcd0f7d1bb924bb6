"""Reference arithmetic of the matrix-product kernels (NumPy, no GPU).

The bf16 x 3 products of sisua_amd/csrc/smx_device.h split every float32 operand three ways (split3_pair: t0 = bf16(x),
r1 = x - t0, t1 = bf16(r1), t2 = bf16(r1 - t1), round-to-nearest-even) and keep six of the nine cross products
(mfma_bf16x3: SIX_TERMS below, (i, j) = a.t_i * b.t_j).  `emulate` is that arithmetic with the accumulation done in float64, so
that what a kernel adds to it is its own float32 accumulation only; `f32_sequential` is the plain float32 statement of the
product, against which the accuracy bounds are sized; `term_probe` builds known-answer operands on which every cross product
moves every output element the same way.
"""
import numpy as np

SIX_TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))   # the order of mfma_bf16x3 (smallest first)
MIRRORED = ((0, 1), (1, 0), (0, 2), (2, 0))                    # the kept terms whose mirror (j, i) is another kept term


def bf16_rne(x):
  """float32 -> the nearest bfloat16 (ties to even), returned as float32; NaN stays NaN, values beyond the bf16 range give inf."""
  x = np.ascontiguousarray(x, dtype=np.float32)
  u = x.view(np.uint32).astype(np.uint64)
  r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
  out = r.view(np.float32).reshape(x.shape).copy()
  out[np.isnan(x)] = np.nan
  return out


def split3(x):
  """x -> (t0, t1, t2), float32 arrays holding bf16 values with x ~= t0 + t1 + t2 (the roundings of split3_pair, in its order)."""
  x = np.asarray(x, dtype=np.float32)
  t0 = bf16_rne(x)
  r1 = x - t0            # exact in float32
  t1 = bf16_rne(r1)
  t2 = bf16_rne(r1 - t1)
  return t0, t1, t2


def emulate(A, B, terms=SIX_TERMS):
  """sum over the listed (i, j) of split3(A)[i] @ split3(B)[j], every product and sum in float64.  A [M][K], B [K][N]."""
  sa = [t.astype(np.float64) for t in split3(A)]
  sb = [t.astype(np.float64) for t in split3(B)]
  out = np.zeros((A.shape[0], B.shape[1]), np.float64)
  for i, j in terms:
    out += sa[i] @ sb[j]
  return out


def dropped(term):
  """SIX_TERMS without `term`"""
  return tuple(t for t in SIX_TERMS if t != term)


def mispaired(term):
  """SIX_TERMS with `term` issued twice in place of its mirror (a.t2 b.t0 twice and no a.t0 b.t2, ...)"""
  i, j = term
  return tuple(term if t == (j, i) else t for t in SIX_TERMS)


def f32_sequential(A, B):
  """float32 products accumulated in float32 in k order (one rounding per product, one per addition)."""
  A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
  acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
  for k in range(A.shape[1]):
    acc += A[:, k:k + 1] * B[k:k + 1, :]
  return acc


def rel_fro(got, ref):
  ref = np.asarray(ref, np.float64)
  return float(np.linalg.norm(np.asarray(got, np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def ulp32(x):
  """the float32 unit in the last place at |x| (x float64, normal range)"""
  x = np.abs(np.asarray(x, np.float64))
  return np.ldexp(1.0, np.floor(np.log2(np.maximum(x, 2.0 ** -126))).astype(np.int64) - 23)


def errors(A, B, ref=None):
  """(ref64, e_seq32, e_drop): the float64 product, the relative Frobenius error of the sequential float32 product and the
  smallest relative Frobenius error among the six one-term-dropped emulations."""
  if ref is None:
    ref = np.asarray(A, np.float64) @ np.asarray(B, np.float64)
  e_seq = rel_fro(f32_sequential(A, B), ref)
  e_drop = min(rel_fro(emulate(A, B, dropped(t)), ref) for t in SIX_TERMS)
  return ref, e_seq, e_drop


def bound(e_seq32, e_drop):
  """The accuracy bound of a product kernel on random operands (relative Frobenius error against float64).

  2 e_seq32: any blocked order of correctly rounded float32 sums errs less than the sequential one, so a right kernel has
  room.  e_drop / 3: a kernel that loses one of the six cross products sits at e_drop, three times over the bound at every
  shape.  (e_drop is ~2.5e-6 at every K and e_seq32 grows like 1.8e-8 sqrt(K): the first binds up to K ~ 500, the second
  beyond -- with a factor 1/2 instead of 1/3 a dropped term would be only 2 times over the bound there.)"""
  return min(2.0 * e_seq32, e_drop / 3.0)


# ---- known-answer operands ------------------------------------------------------------------------------------------------
PROBE_POSITIONS = 8   # exactly this many non-zero k: every result then lies in [8, 16), where one float32 ulp is 2^-20


def term_probe(M, N, K, ks, seed=0):
  """A [M][K], B [K][N], zero except at the 8 k positions `ks`, where
       A = a0 + a1 2^-10 + a2 2^-19   a0 in {1, 2} (2 at two of a row's positions), a1 in {1, 2, 3}, a2 = +1
       B = b0 + b1 2^-10 + b2 2^-19   b0 in {1.25, 1.5},                            b1 in {-1, -2, -3}, b2 = -1
  and every entry splits into exactly those three bf16 terms (asserted).  Every result is
       sum a0 b0  in [10, 15]  +  low-order terms below 0.1,
  so one float32 ulp is 2^-20 at every element, and every cross product pushes every element the same way:
       t1 t0 / t0 t1   + / - sum a1 b0, a0 |b1|   x 2^-10      (thousands of ulp)
       t2 t0 / t0 t2   + / - sum b0, a0           x 2^-19      (>= 16 ulp)
       t1 t1           - sum a1 |b1|              x 2^-20      (>= 8 ulp)
  A's low terms are positive and B's negative, so a term issued twice in place of its mirror (a.t2 b.t0 for a.t0 b.t2)
  moves the sum by the two terms' DIFFERENCE, which is their magnitudes' sum.  (B's leading term avoids powers of two: below
  one the bf16 grid is twice as fine and b0 - 3 2^-10 would not round back to b0.)"""
  ks = np.asarray(sorted(int(k) for k in ks), np.int64)
  assert len(ks) == PROBE_POSITIONS and len(set(ks.tolist())) == PROBE_POSITIONS and ks[0] >= 0 and ks[-1] < K, (ks, K)
  rng = np.random.default_rng(seed)
  n = PROBE_POSITIONS
  a0 = np.ones((M, n))
  for i in range(M):
    a0[i, rng.choice(n, 2, replace=False)] = 2.0
  a1 = rng.integers(1, 4, size=(M, n)).astype(np.float64)
  b0 = rng.choice([1.25, 1.5], size=(n, N))
  b1 = -rng.integers(1, 4, size=(n, N)).astype(np.float64)
  Ak = a0 + a1 * 2.0 ** -10 + 2.0 ** -19
  Bk = b0 + b1 * 2.0 ** -10 - 2.0 ** -19
  A = np.zeros((M, K), np.float32)
  B = np.zeros((K, N), np.float32)
  A[:, ks] = Ak
  B[ks, :] = Bk
  assert np.array_equal(A[:, ks].astype(np.float64), Ak) and np.array_equal(B[ks, :].astype(np.float64), Bk)   # exact in float32
  for X, parts in ((A[:, ks], (a0, a1 * 2.0 ** -10, np.full((M, n), 2.0 ** -19))),
                   (B[ks, :], (b0, b1 * 2.0 ** -10, np.full((n, N), -2.0 ** -19)))):
    for t, want in zip(split3(X), parts):
      assert np.array_equal(t.astype(np.float64), want), "term_probe: an entry does not split into its three terms"
  return A, B


def probe_groups(K, positions):
  """The k positions a probe has to touch, as groups of exactly PROBE_POSITIONS distinct positions below K (the last group is
  filled up from the first positions)."""
  pos = sorted({int(p) for p in positions if 0 <= int(p) < K})
  spare = [k for k in range(K) if k not in set(pos)]
  while len(pos) < PROBE_POSITIONS:
    pos.append(spare.pop(0))
  pos = sorted(pos)
  groups = [pos[i:i + PROBE_POSITIONS] for i in range(0, len(pos), PROBE_POSITIONS)]
  short = PROBE_POSITIONS - len(groups[-1])
  if short:
    groups[-1] = sorted(groups[-1] + [p for p in pos if p not in groups[-1]][:short])
  return groups


# ---- the forms reachable through smx_k_gemm, their shapes and the k positions their probes touch ---------------------------
# (the constants are the kernels' own; the line that gives each is named beside it)
def _edges(K, period):
  """both sides of every multiple of `period` below K"""
  out = []
  for b in range(period, K, period):
    out += [b - 1, b]
  return out


def lds_tile_positions(K, tile, split_k):
  """smx_gemm.hip, tiles 0-5 (float32 MFMAs of 2 k).
  BK = 32 WK (gemm_body: `BK = 32 * WK`; launch_gemm: tile 1 / 2 / 3 -> WK = 1, tile 4 -> WK = 4, tile 5 -> WK = 2; tile 0
  chooses among 1-4 by shape: both depths are covered), wave wk of a workgroup takes the k rows 32 wk + lh + 2 s of a BK tile
  (`as = As + (wk * 32 + lh) * LDAS`, `as[2 * s * LDAS]`): its share is a 32-deep block, whose first and last k and both lane
  halves (lh = k & 1) are touched; the split-K slices are k_chunk = round_up(ceil(K / split_k), BK) deep (launch_cfg)."""
  pos = [0, 1, K - 1, K - 2] + _edges(min(K, 129), 32)
  for wk in {1: (1,), 2: (1,), 3: (1,), 4: (4,), 5: (2,)}.get(tile, (1, 4)):
    bk = 32 * wk
    chunk = -(-(-(-K // split_k)) // bk) * bk                # round_up(ceil(K / split_k), BK)
    pos += _edges(K, chunk)
    last = (K - 1) // chunk * chunk                          # the ragged last slice: the first k of each of its 32-deep blocks
    pos += [k for k in range(last, K, 32)]
  return pos


def dgemm_positions(K):
  """smx_dgemm.h, tile 100: K padded to 32; wave q takes k = 32 q .. 32 q + 31 of every 256-deep round (`for (int kb = 32 * q; kb < g.K;
  kb += 256)`), as two 16-deep MFMA steps (`16 * t + 8 * hh`)."""
  pos = [0, K - 1]
  for q in range(8):                            # every wave's share: first and last k of its two steps in round 0
    pos += [32 * q, 32 * q + 15, 32 * q + 16, 32 * q + 31]
  pos += _edges(K, 256)                         # both sides of every round boundary
  lastw = (K - 1) // 32 * 32                    # the wave that holds the ragged end
  pos += [lastw, lastw + 7, lastw + 8]
  return pos


def wgrad_positions(K):
  """smx_headbwd.hip wgrad_tile_body, tile 101: K = cells, chunks of 128 (`for (int kc = 0; kc < B; kc += 128)`), wave q takes the 16
  cells kc + 16 q .. + 15 as ONE MFMA step, lane half hh its 8 (`k0 = kc + 16 * q + 8 * hh`)."""
  pos = [0, K - 1]
  for q in range(8):
    pos += [16 * q, 16 * q + 7, 16 * q + 8, 16 * q + 15]
  pos += _edges(K, 128)
  return pos


def panel_positions(K):
  """smx_panel.h panel_body (role 0), tile 102: chunks of 128 cells (`kc += 128`); wave (t, kh) multiplies cells kc + 64 kh + 16 st + 8 hh + s
  (`cbr = 8 * kh + 2 * st + hh`), st = 0..3: 16-deep steps, 64-deep halves that meet through LDS; the panel tile is staged by cell block
  cb = 2 w + hh (8 cells each)."""
  pos = [0, K - 1]
  for kh in range(2):
    for st in range(4):
      pos += [64 * kh + 16 * st, 64 * kh + 16 * st + 7, 64 * kh + 16 * st + 8, 64 * kh + 16 * st + 15]
  pos += _edges(K, 128)
  return pos


def bigk_slices(K, max_slices=256):
  """smx_bigk.hip bigk_slices: (number of slices, k per slice); SMX_BIGK_MAX_SLICES = 256 (smx_model.h)"""
  chunk = max(64, (-(-K // max_slices) + 31) // 32 * 32)
  return -(-K // chunk), chunk


def bigk_positions(K):
  """smx_bigk.hip, tile 103: K padded to 32; slice z takes k_chunk consecutive k (bigk_slices), in 32-deep stages (`n_st = (kend - kbeg + 31) / 32`)
  of two 16-deep steps (`16 * t + 8 * hh`); the reduce launch gives slice z to thread z % 16 of an output's 16 (`for (int z0 = t; z0 < n_slices; z0 += 256)`,
  `z0 + 16 * u`): slices 0..15 are the 16 threads' first, slice 16 the second of thread 0."""
  Kp = (K + 31) // 32 * 32
  n, chunk = bigk_slices(Kp)
  pos = [0, 15, 16, 31, 32, K - 1]
  for z in (1, 2, 15, 16, 17, n // 2, n - 1):   # both sides of these slices' lower boundaries
    pos += [z * chunk - 1, z * chunk]
  for z in range(16):                           # one k in every reduce thread's first slice
    pos.append(z * chunk + (z % 4) * 8 + 3)
  lo = (n - 1) * chunk                          # the last (possibly shorter) slice: first and last k of its stages' steps
  pos += [lo, lo + 15, lo + 16, lo + 31, (K - 1) // 32 * 32, (K - 1) // 16 * 16]
  return pos


# (form, tile, transposes (A stored [K][M], B stored [N][K]), shapes (M, N, K))
LDS_SHAPES = ((37, 128, 200), (130, 128, 515))
LDS_LAYOUTS = ((False, False), (True, False), (False, True))
DGEMM_SHAPES = ((33, 96, 515), (130, 160, 1400))
WGRAD_SHAPES = ((70, 96, 37), (260, 128, 129), (33, 64, 300))
BIGK_SHAPES = ((37, 96, 8224), (128, 128, 4096))


def forms():
  """every (name, tile, trans_a, trans_b, split_k, (M, N, K), positions) the product tests cover"""
  out = []
  for tile in range(6):
    for ta, tb in LDS_LAYOUTS:
      for S in (1, 4):
        for shp in LDS_SHAPES:
          out.append(("lds", tile, ta, tb, S, shp, lds_tile_positions(shp[2], tile, S)))
  for tb in (False, True):
    for shp in DGEMM_SHAPES:
      out.append(("dgemm", 100, False, tb, 1, shp, dgemm_positions(shp[2])))
  for tile, fn in ((101, wgrad_positions), (102, panel_positions)):
    for shp in WGRAD_SHAPES:
      out.append(("wgrad" if tile == 101 else "panel", tile, True, False, 1, shp, fn(shp[2])))
  for tb in (False, True):
    for shp in BIGK_SHAPES:
      out.append(("bigk", 103, False, tb, 1, shp, bigk_positions(shp[2])))
  return out


def shapes_used():
  return sorted({f[5] for f in forms()})


def random_operands(M, N, K, seed, scaled=False):
  """N(0, 1) operands A [M][K], B [K][N]; scaled: A's rows and B's columns times powers of two drawn from 2^-20 .. 2^20"""
  rng = np.random.default_rng(seed)
  A = rng.normal(size=(M, K)).astype(np.float32)
  B = rng.normal(size=(K, N)).astype(np.float32)
  if scaled:
    A = np.ldexp(A, rng.integers(-20, 21, size=(M, 1))).astype(np.float32)
    B = np.ldexp(B, rng.integers(-20, 21, size=(1, N))).astype(np.float32)
  return A, B


# ---- running a form through a k_gemm callable (sisua_amd.engine.k_gemm) -----------------------------------------------------
def run_form(k_gemm, tile, ta, tb, split_k, A, B):
  """C = A B by the form (tile, layouts, split_k): A [M][K] and B [K][N] are handed over in the storage order the form takes"""
  A = np.ascontiguousarray(A.T) if ta else np.ascontiguousarray(A)
  B = np.ascontiguousarray(B.T) if tb else np.ascontiguousarray(B)
  return k_gemm(A, B, ta, tb, split_k=split_k, tile=tile)


def probe_worst_ulp(k_gemm, form):
  """the largest |C - ref64| / ulp_f32(ref64) over every element of every probe group of the form"""
  _, tile, ta, tb, S, (M, N, K), positions = form
  worst = 0.0
  for gi, ks in enumerate(probe_groups(K, positions)):
    A, B = term_probe(M, N, K, ks, seed=gi)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    C = run_form(k_gemm, tile, ta, tb, S, A, B)
    worst = max(worst, float((np.abs(C.astype(np.float64) - ref) / ulp32(ref)).max()))
  return worst


# ---- the fused output head, isolated from the likelihood ------------------------------------------------------------------
HEAD_G = 4128
HEAD_ROWS = (0, 31, 63, 64, 100, 127)   # smx_headfused.hip: wave w owns cells 16 w .. 16 w + 15; waves 0-3 and 4-7 are its two groups


def head_operands(likelihood, k, b_star, seed=0):
  """x [128][G] counts, d [128][128] zero in every row but b_star, W [128][k][G], bias [k][G]"""
  rng = np.random.default_rng(seed)
  B, G = 128, HEAD_G
  x = (rng.poisson(3.0, size=(B, G)) * (rng.uniform(size=(B, G)) < 0.1)).astype(np.float32)
  d = np.zeros((B, 128), np.float32)
  d[b_star] = np.maximum(rng.normal(size=128), 0).astype(np.float32)
  W = (rng.normal(size=(128, k, G)) * 0.08).astype(np.float32)
  bias = (rng.normal(size=(k, G)) * 0.3).astype(np.float32)
  return x, d, W, bias


def head_figures(k_head_fused, likelihood, k, b_star):
  """dict of (error, e_seq32, e_drop) for the weight gradient of launch 1 (all 128 cells, d zero but in row b_star) against
  d[b_star] (x) db2, and for the decoder gradient of launch 2 (that cell alone) against db2 W^T; db2 = launch 2's bias
  gradient = the cell's dP as the kernel computes it."""
  x, d, W, bias = head_operands(likelihood, k, b_star)
  scale = -1.0 / 128
  one = k_head_fused(likelihood, x, d, W, bias, grad_scale=scale)
  two = k_head_fused(likelihood, x[b_star:b_star + 1], d[b_star:b_star + 1], W, bias, grad_scale=scale)
  db2 = two["db"].reshape(1, -1)                                        # [1][k G]
  col = d[b_star].reshape(-1, 1)                                        # [128][1]
  ref_w, es_w, ed_w = errors(col, db2)
  out = {"dW": (rel_fro(one["dW"].reshape(128, -1), ref_w), es_w, ed_w)}
  Wt = np.ascontiguousarray(W.reshape(128, -1).T)                       # [k G][128]
  ref_d, es_d, ed_d = errors(db2, Wt)
  out["dd"] = (rel_fro(two["dd"], ref_d), es_d, ed_d)
  out["finite"] = bool(np.isfinite(one["dW"]).all() and np.isfinite(two["dd"]).all() and np.isfinite(db2).all())
  return out


# ---- properties beyond unit-scale normals ---------------------------------------------------------------------------------
SCALINGS = ((40, -40), (-60, 60), (-90, 0), (100, -100), (-100, 100))
# The split commutes with a power-of-two scaling while every non-zero term of it is a normal bf16 / float32: r1 and r1 - t1 are
# multiples of ulp_f32(x) = 2^(e - 23) (e the exponent of x) and can be as small as that, so t2 stays normal iff e - 23 >= -126:
# |x| >= 2^-103.  Operands in [2^-3, 2^3] times 2^-100 start exactly there ((100, -100) for B, (-100, 100) for A).
SPLIT_MIN_EXPONENT = -103


def unit_range_operands(M, N, K, seed):
  """random signs, magnitudes 2^u with u uniform in [-3, 3]"""
  rng = np.random.default_rng(seed)
  f = lambda *s: (rng.choice([-1.0, 1.0], size=s) * np.exp2(rng.uniform(-3, 3, size=s))).astype(np.float32)
  return f(M, K), f(K, N)


def scaling_mismatches(k_gemm, form, p, q, seed=3):
  """elements of C(2^p A, 2^q B) whose bits differ from 2^(p + q) C(A, B)"""
  _, tile, ta, tb, S, (M, N, K), _ = form
  A, B = unit_range_operands(M, N, K, seed)
  C0 = run_form(k_gemm, tile, ta, tb, S, A, B)
  Cs = run_form(k_gemm, tile, ta, tb, S, np.ldexp(A, p).astype(np.float32), np.ldexp(B, q).astype(np.float32))
  want = np.ldexp(C0.astype(np.float64), p + q).astype(np.float32)
  return int((Cs.view(np.uint32) != want.view(np.uint32)).sum())


def random_figures(k_gemm, form, scaled, cache=None):
  """(error, e_seq32, e_drop) of the form on N(0, 1) operands (scaled: rows / columns times powers of two)"""
  _, tile, ta, tb, S, (M, N, K), _ = form
  key = (M, N, K, scaled)
  if cache is not None and key in cache:
    A, B, ref, es, ed = cache[key]
  else:
    A, B = random_operands(M, N, K, seed=K + M, scaled=scaled)
    ref, es, ed = errors(A, B)
    if cache is not None:
      cache[key] = (A, B, ref, es, ed)
  C = run_form(k_gemm, tile, ta, tb, S, A, B)
  return rel_fro(C, ref) if np.isfinite(C).all() else float("inf"), es, ed


def subnormal_figures(k_gemm, form, cache=None):
  """N(0, 1) operands with one entry in sixteen replaced by a float32 subnormal: (finite, ||C - ref||_F, allowed), allowed =
  bound ||ref||_F + sqrt(M N) K 2^-126 max|operand| (a flushed subnormal costs at most 2^-126 |other| per product)"""
  _, tile, ta, tb, S, (M, N, K), _ = form
  key = (M, N, K, "sub")
  if cache is not None and key in cache:
    A, B, ref, es, ed = cache[key]
  else:
    rng = np.random.default_rng(K * 3 + M)
    A, B = random_operands(M, N, K, seed=K + M + 1)
    for X in (A, B):
      hit = rng.uniform(size=X.shape) < 1.0 / 16
      sub = (rng.choice([-1, 1], size=X.shape) * rng.integers(1, 1 << 23, size=X.shape)).astype(np.float64) * 2.0 ** -149
      X[hit] = sub[hit].astype(np.float32)
    ref, es, ed = errors(A, B)
    if cache is not None:
      cache[key] = (A, B, ref, es, ed)
  C = run_form(k_gemm, tile, ta, tb, S, A, B)
  allowed = bound(es, ed) * np.linalg.norm(ref) + np.sqrt(M * N) * K * 2.0 ** -126 * max(np.abs(A).max(), np.abs(B).max())
  return bool(np.isfinite(C).all()), float(np.linalg.norm(C.astype(np.float64) - ref)), float(allowed)


def wide_range_figures(k_gemm, form, floor=-126, cache=None):
  """A of magnitude up to 2^126 against B of magnitude 2^floor .. 2^(floor + 4): (error, e_seq32, e_drop); error inf when the
  result is not finite"""
  _, tile, ta, tb, S, (M, N, K), _ = form
  key = (M, N, K, "wide", floor)
  if cache is not None and key in cache:
    A, B, ref, es, ed = cache[key]
  else:
    A, B = random_operands(M, N, K, seed=K + M + 2)
    A = np.ldexp(np.clip(A, -4, 4), 124).astype(np.float32)               # |A| <= 2^126
    B = np.ldexp(np.clip(np.where(np.abs(B) < 0.25, np.copysign(0.25, B), B), -4, 4), floor + 2).astype(np.float32)   # 2^floor <= |B| <= 2^(floor + 4)
    assert np.abs(A).max() <= 2.0 ** 126 and np.abs(B).min() >= 2.0 ** floor
    ref, es, ed = errors(A, B)
    if cache is not None:
      cache[key] = (A, B, ref, es, ed)
  C = run_form(k_gemm, tile, ta, tb, S, A, B)
  return rel_fro(C, ref) if np.isfinite(C).all() else float("inf"), es, ed


def containment(k_gemm, form, seed=5):
  """A NaN, then +inf, in one element of A's row i, then of B's column j (i, j in the first tile and in the last, ragged one; a
  valid k): list of (what, line all non-finite, every other element bit-identical to the clean run)"""
  _, tile, ta, tb, S, (M, N, K), _ = form
  A, B = random_operands(M, N, K, seed=seed)
  clean = run_form(k_gemm, tile, ta, tb, S, A, B)
  out = []
  for val in (np.nan, np.inf):
    for i, k in ((1, 3), (M - 1, K - 1)):
      A2 = A.copy(); A2[i, k] = val
      C = run_form(k_gemm, tile, ta, tb, S, A2, B)
      rest = np.delete(C, i, axis=0).view(np.uint32) == np.delete(clean, i, axis=0).view(np.uint32)
      out.append(("A[%d,%d]=%s" % (i, k, val), bool((~np.isfinite(C[i])).all()), bool(rest.all())))
    for j, k in ((2, 0), (N - 1, K - 1)):
      B2 = B.copy(); B2[k, j] = val
      C = run_form(k_gemm, tile, ta, tb, S, A, B2)
      rest = np.delete(C, j, axis=1).view(np.uint32) == np.delete(clean, j, axis=1).view(np.uint32)
      out.append(("B[%d,%d]=%s" % (k, j, val), bool((~np.isfinite(C[:, j])).all()), bool(rest.all())))
  return out
