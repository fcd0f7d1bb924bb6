"""Kernel-level helpers (tests): one launch of the training step by itself, on host arrays, outside any model."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from sisua_amd import _hip, optimizers
from sisua_amd._hip import check
from sisua_amd.engine._args import _f32, _fp, _ip, _ptr


def k_count_llk(likelihood: str, x, planes, direct: bool = False, want_grads: bool = True):
  lib = _hip.require_gpu()
  x = _f32(x)
  B, G = x.shape
  pl = _f32(planes)
  k = pl.shape[0]
  llk = np.empty(B, np.float32)
  grads = np.empty((k, B, G), np.float32) if want_grads else None
  check(lib.smx_k_count_llk(_hip.LIKELIHOODS[likelihood], int(direct), _fp(x), _fp(pl), B, G, _fp(llk), _fp(grads)))
  return llk, grads


def k_head_fused(likelihood: str, x, d, W, bias, grad_scale: float = 1.0, u16: bool = False, reps: int = 0):
  """The fused output head (smx_headfused.hip) over host arrays: x [B][G], d [B][128], W [128][k][G], bias [k][G] ->
  dict(llk [B], dW, db, dd [B][128], sumsq, us)."""
  lib = _hip.require_gpu()
  x, d, W, bias = _f32(x), _f32(d), _f32(W), _f32(bias)
  B, G = x.shape
  k = W.shape[1]
  assert d.shape == (B, 128) and W.shape == (128, k, G) and bias.shape == (k, G)
  llk = np.empty(B, np.float32)
  dW, db, dd = np.empty((128, k, G), np.float32), np.empty((k, G), np.float32), np.empty((B, 128), np.float32)
  sumsq, us = np.zeros(1, np.float32), np.zeros(1, np.float32)
  check(lib.smx_k_head_fused(_hip.LIKELIHOODS[likelihood], int(u16), _fp(x), _fp(d), _fp(W), _fp(bias), B, G, float(grad_scale), int(reps),
                             _fp(llk), _fp(dW), _fp(db), _fp(dd), _fp(sumsq), _fp(us)))
  return dict(llk=llk, dW=dW, db=db, dd=dd, sumsq=float(sumsq[0]), us=float(us[0]))


def k_head_fused_stress(likelihood: str, x, d, W, bias, launches: int, grad_scale: float = 1.0, u16: bool = False):
  """`launches` launches of the fused output head on the same inputs, each compared bit for bit on the device with the first:
  (launches that differed, index of the first differing output word or -1)."""
  lib = _hip.require_gpu()
  x, d, W, bias = _f32(x), _f32(d), _f32(W), _f32(bias)
  B, G = x.shape
  k = W.shape[1]
  assert d.shape == (B, 128) and W.shape == (128, k, G) and bias.shape == (k, G)
  n, first = C.c_int32(0), C.c_int64(-1)
  check(lib.smx_k_head_fused_stress(_hip.LIKELIHOODS[likelihood], int(u16), _fp(x), _fp(d), _fp(W), _fp(bias), B, G, float(grad_scale), int(launches),
                                    C.byref(n), C.byref(first)))
  return int(n.value), int(first.value)


def _flat(params, *lists):
  """Lists of arrays shaped as `params` as the optimiser entries take them: (sizes int32 [n], the flat float32 copy of `params` and of
  every further list, un: a flat array back as the list of arrays in params' shapes)."""
  sizes = np.array([int(np.size(p)) for p in params], dtype=np.int32)
  cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).ravel() for x in xs]))
  cut = np.cumsum(sizes)[:-1]
  shp = [np.shape(p) for p in params]
  un = lambda flat: [a.reshape(sh) for a, sh in zip(np.split(flat, cut), shp)]
  return sizes, [cat(xs) for xs in (params,) + lists], un


def k_adam(params, grads, m, v, step: int, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, clipnorm=100.0):
  """The optimiser launch by itself over lists of arrays (updated copies are returned): (params, m, v, norms)."""
  lib = _hip.require_gpu()
  sizes, (P, G, M, V), un = _flat(params, grads, m, v)
  norms = np.empty(len(sizes), np.float32)
  check(lib.smx_k_adam(len(sizes), _ip(sizes), _fp(P), _fp(G), _fp(M), _fp(V), int(step),
                       float(lr), float(beta1), float(beta2), float(eps), float(clipnorm), _fp(norms)))
  return un(P), un(M), un(V), norms


def k_opt(rule: str, params, grads, m, v, step: int, lr=1e-3, clipnorm=100.0, **hp):
  """The optimiser launch by itself under any rule of Engine.set_optimizer (smx_k_opt); m / v are the rule's slots 2 / 3.  Updated copies
  are returned: (params, m, v, norms)."""
  lib = _hip.require_gpu()
  name, full = optimizers.canonical(rule, **hp)
  hv = optimizers.hp_vector(name, full)
  sizes, (P, G, M, V), un = _flat(params, grads, m, v)
  norms = np.empty(len(sizes), np.float32)
  check(lib.smx_k_opt(optimizers.RULES[name][0], _fp(hv), len(hv), len(sizes), _ip(sizes), _fp(P), _fp(G),
                      _fp(M), _fp(V), int(step), float(lr), float(clipnorm), _fp(norms)))
  return un(P), un(M), un(V), norms


OPT_CARRIERS = {"launch": 0, "sweep": 1, "shard": 2, "body512": 3}   # smx_opt_carrier


def k_opt_carrier(rule: str, params, grads, m, v, step: int, carrier="launch", wgs=0, world=0, use_sq=False, sq=None, lr=1e-3, clipnorm=100.0,
                  grad_scale=1.0, t0=0, tied=(), tied_inv=1.0, hp_raw=None, **hp):
  """Clip + update by one of the launches that carry the optimiser's chunk body (smx_k_opt_carrier): the optimiser launch, the background
  sweep with `wgs` workgroups, the sharded chain of `world` simulated ranks, the 512-thread body.  Lists of arrays as k_opt's.  `use_sq`: the
  norms without the norm pass -- `sq[i]` holds tensor i's sum-of-squares slots, or None for the sweep of its own gradient (what lies behind a
  tensor's slots in the device array is NaN).  `tied`: up to two tensor indices whose sum of squares is multiplied by `tied_inv`.  `hp_raw`: a
  hyper-parameter vector handed to the library as it is, in place of **hp.  Returns dict(params, m, v: the whole padded flat buffers;
  offsets, sizes, pads: where tensor i lies in them; norms; lr_t: the device's step size; guards_ok; unused_ok)."""
  lib = _hip.require_gpu()
  if hp_raw is None:
    name, full = optimizers.canonical(rule, **hp)
    hv = optimizers.hp_vector(name, full)
  else:
    name, hv = rule.lower(), np.ascontiguousarray(hp_raw, dtype=np.float32)
  sizes, (P, G, M, V), _ = _flat(params, grads, m, v)
  pads = (sizes.astype(np.int64) + 63) // 64 * 64
  offsets = np.concatenate([[0], np.cumsum(pads)[:-1]])
  total = int(pads.sum())
  first, count, slots = np.zeros(len(sizes), np.int32), np.zeros(len(sizes), np.int32), [np.full(8, np.nan, np.float32)]
  for i, s in enumerate(sq or []):
    if s is not None:
      first[i], count[i] = sum(len(x) for x in slots), np.size(s)
      slots += [np.asarray(s, np.float32).ravel(), np.full(8, np.nan, np.float32)]
  slots = np.ascontiguousarray(np.concatenate(slots))
  tied = list(tied) + [-1, -1]
  ip = np.array([optimizers.RULES[name][0], len(sizes), OPT_CARRIERS[carrier], wgs, world, int(bool(use_sq)), step, t0, tied[0], tied[1], len(slots)], np.int32)
  fp = np.array([lr, clipnorm, grad_scale, tied_inv], np.float32)
  o = dict(params=np.empty(total, np.float32), m=np.empty(total, np.float32), v=np.empty(total, np.float32), norms=np.empty(len(sizes), np.float32),
           offsets=offsets, sizes=sizes.astype(np.int64), pads=pads)
  lr_t, ok, same = C.c_float(0), C.c_int32(0), C.c_int32(0)
  check(lib.smx_k_opt_carrier(_ip(ip), _fp(fp), _fp(hv), len(hv), _ip(sizes), _fp(P), _fp(G), _fp(M), _fp(V), _ip(first), _ip(count), _fp(slots),
                              _fp(o["params"]), _fp(o["m"]), _fp(o["v"]), _fp(o["norms"]), C.byref(lr_t), C.byref(ok), C.byref(same)))
  o.update(lr_t=np.float32(lr_t.value), guards_ok=bool(ok.value), unused_ok=bool(same.value))
  return o


def k_gemm(A, B, trans_a=False, trans_b=False, split_k=1, tile=0):
  lib = _hip.require_gpu()
  A, B = _f32(A), _f32(B)
  M, K = (A.shape[1], A.shape[0]) if trans_a else A.shape
  N = B.shape[0] if trans_b else B.shape[1]
  Cm = np.empty((M, N), np.float32)
  check(lib.smx_k_gemm(int(trans_a), int(trans_b), _fp(A), _fp(B), M, N, K, int(split_k), int(tile), _fp(Cm)))
  return Cm


def k_row_select(rows, n_genes: Optional[int] = None):
  """smx_k_row_select: the two middle order statistics of the first n_genes entries of every row of `rows` [n, ld] (non-negative or NaN) -> (lo, hi) [n]"""
  lib = _hip.require_gpu()
  r = _f32(rows)
  n, ld = r.shape
  G = ld if n_genes is None else int(n_genes)
  lo, hi = np.empty((n,), np.float32), np.empty((n,), np.float32)
  check(lib.smx_k_row_select(_fp(r), n, G, ld, _fp(lo), _fp(hi)))
  return lo, hi


def k_noise(seed, stream, step, cell_ids, width, p=0.0, sample=0):
  lib = _hip.require_gpu()
  ids = np.ascontiguousarray(cell_ids, dtype=np.int64)
  mult = np.empty((ids.size, width), np.float32)
  nrm = np.empty((ids.size, width), np.float32)
  check(lib.smx_k_noise(int(seed), int(stream), int(step), int(sample), _ptr(ids),
                        ids.size, int(width), float(p), _fp(mult), _fp(nrm)))
  return mult, nrm


def _bn_vec(a, Hp):
  """A per-column vector as the BatchNorm entries take it: [Hp] float32 (a shorter one is padded with zeros), None stays None"""
  if a is None:
    return None
  a = np.asarray(a, np.float32).ravel()
  if a.size < Hp:
    a = np.concatenate([a, np.zeros(Hp - a.size, np.float32)])
  return np.ascontiguousarray(a[:Hp])


def _bn_slabs(x, wide):
  """slabs [S][B][ld] (or [B][ld]) / wide [S][Hp][128] -> (array, S, rows, ld)"""
  x = _f32(x)
  if x.ndim == 2:
    x = x[None]
  if x.ndim != 3 or (wide and x.shape[2] != 128):
    raise ValueError("slabs are [S][B][ld], wide ones [S][Hp][128]")
  return x, x.shape[0], x.shape[1], x.shape[2]


def k_bn_fwd(pre, B, H, Hp, gamma=None, beta=None, bias=None, moving_mean=None, moving_var=None, batchnorm=True, training=True,
             update_moving=True, momentum=0.99, eps=1e-3, leak=0.0, act="relu", drop_p=0.0, mask=None, seed=0, stream=0, step=0,
             rows=None, cell_base=0, wide=False, world=0):
  """The forward BatchNorm launch by itself (smx_k_bn_fwd): `pre` = slabs [S][B][ld], or with `wide` the column-major [S][Hp][128].
  Returns dict(out, xhat [B][Hp]; inv_std, batch_mean, batch_var, moving_mean, moving_var [Hp]; guards_ok).  What the launch does not
  write (batch statistics in evaluation mode, everything of BatchNorm without it) comes back as NaN."""
  lib = _hip.require_gpu()
  pre, S, r, ld = _bn_slabs(pre, wide)
  if (wide and r != Hp) or (not wide and r != B):
    raise ValueError("slab rows do not match B (wide: Hp)")
  g, b, bi, mm, mv = (_bn_vec(v, Hp) for v in (gamma, beta, bias, moving_mean, moving_var))
  m = None if mask is None else _f32(mask)
  rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
  ip = np.array([S, B, H, Hp, Hp if wide else ld, int(wide), int(batchnorm), int(training), int(update_moving), _hip.HIDDEN_ACTIVATIONS[act],
                 0 if m is None else m.shape[1], stream, step, cell_base, world], np.int32)
  fp = np.array([momentum, eps, leak, drop_p], np.float32)
  o = dict(out=np.empty((B, Hp), np.float32), xhat=np.empty((B, Hp), np.float32))
  for k in ("inv_std", "batch_mean", "batch_var", "moving_mean", "moving_var"):
    o[k] = np.empty(Hp, np.float32)
  ok = C.c_int32(0)
  check(lib.smx_k_bn_fwd(_ip(ip), _fp(fp), _fp(pre), _fp(g), _fp(b), _fp(bi), _fp(mm), _fp(mv), _fp(m), _ip(rw), int(seed),
                         _fp(o["out"]), _fp(o["xhat"]), _fp(o["inv_std"]), _fp(o["batch_mean"]), _fp(o["batch_var"]), _fp(o["moving_mean"]),
                         _fp(o["moving_var"]), C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o


def k_bn_bwd(dout, out, xhat, B, H, Hp, inv_std=None, gamma=None, beta=None, batchnorm=True, training=True, leak=0.0, act="relu", drop_p=0.0,
             mask=None, seed=0, stream=0, step=0, rows=None, cell_base=0, wide=False, world=0):
  """The backward BatchNorm launch by itself (smx_k_bn_bwd) on its inputs: the d out slabs (laid out as k_bn_fwd's), the forward's out and
  xhat [B][Hp], inv_std, gamma, beta.  Returns dict(dpre [B][Hp]; dgamma, dbeta [max(world, 1)][Hp]; dbias [Hp]; guards_ok)."""
  lib = _hip.require_gpu()
  dout, S, r, ld = _bn_slabs(dout, wide)
  if (wide and r != Hp) or (not wide and r != B):
    raise ValueError("slab rows do not match B (wide: Hp)")
  out, xhat = _f32(out, (B, Hp)), _f32(xhat, (B, Hp))
  iv, g, b = (_bn_vec(v, Hp) for v in (inv_std, gamma, beta))
  m = None if mask is None else _f32(mask)
  rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
  ip = np.array([S, B, H, Hp, Hp if wide else ld, int(wide), int(batchnorm), int(training), _hip.HIDDEN_ACTIVATIONS[act],
                 0 if m is None else m.shape[1], stream, step, cell_base, world], np.int32)
  fp = np.array([leak, drop_p], np.float32)
  nw = max(int(world), 1)
  o = dict(dpre=np.empty((B, Hp), np.float32), dgamma=np.empty((nw, Hp), np.float32), dbeta=np.empty((nw, Hp), np.float32),
           dbias=np.empty(Hp, np.float32))
  ok = C.c_int32(0)
  check(lib.smx_k_bn_bwd(_ip(ip), _fp(fp), _fp(dout), _fp(out), _fp(xhat), _fp(iv), _fp(g), _fp(b), _fp(m), _ip(rw),
                         int(seed), _fp(o["dpre"]), _fp(o["dgamma"]), _fp(o["dbeta"]), _fp(o["dbias"]), C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o


def _scvi_layout(G, k, Gp, plane_stride, ld):
  """The step's layout of the scVI head's planes unless overridden: Gp = G rounded up to 32, plane_stride = Gp, ld = k Gp"""
  Gp = (int(G) + 31) // 32 * 32 if Gp is None else int(Gp)
  ps = Gp if plane_stride is None else int(plane_stride)
  return Gp, ps, (k - 1) * ps + Gp if ld is None else int(ld)


def k_scvi_head_train(raw, x, hl, Wl, bl, library, G, likelihood="zinbd", rows=None, x_identity=False, eps=None, clip_library=1e3,
                      grad_scale=1.0, kl_weight=0.0, ldl=2, Gp=None, plane_stride=None, ld=None, seed=0, stream=65, step=0, cell_base=0, omit=()):
  """The row-local training launch of the scVI gene head by itself (smx_k_scvi_head_train).  raw [B][ld] in the step's layout (plane c of a
  row at c * plane_stride); x [n_x][Gp] counts, float32 or uint16 (the dtype picks the kernel's load path); hl [B][Kl]; Wl [Kl][2]; bl [2];
  library [n_lib][2]; rows [B] (optional; with x_identity the rows of x are the minibatch's already); eps [B] the injected library noise
  (None: drawn on the device).  Returns every output of the kernel: draw [B][ld]; llk_part, l, sig, eps, kl, dl [B]; latl, dlatl [B][ldl];
  guards_ok.  A word the kernel did not write comes back as NaN.  omit: names of outputs handed to the launcher as NULL (it refuses)."""
  lib = _hip.require_gpu()
  k = 3 if likelihood == "zinbd" else 2
  Gp, ps, ld = _scvi_layout(G, k, Gp, plane_stride, ld)
  raw = _f32(raw)
  B = raw.shape[0]
  raw = _f32(raw.reshape(B, -1), (B, ld))
  u16 = np.asarray(x).dtype == np.uint16
  x = np.ascontiguousarray(x, dtype=np.uint16 if u16 else np.float32)
  if x.ndim != 2 or x.shape[1] < Gp:
    raise ValueError(f"x must be [rows][>= Gp = {Gp}], got {x.shape}")
  hl, Wl = _f32(hl), _f32(Wl)
  if hl.ndim != 2 or hl.shape[0] != B or Wl.shape != (hl.shape[1], 2):
    raise ValueError(f"hl must be [B, Kl] and Wl [Kl, 2], got {hl.shape} and {Wl.shape}")
  bl, library = _f32(bl, (2,)), _f32(library)
  if library.ndim != 2 or library.shape[1] != 2:
    raise ValueError(f"library must be [n, 2], got {library.shape}")
  rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
  ep = None if eps is None else _f32(eps, (B,))
  ip = np.array([B, G, Gp, ps, ld, _hip.LIKELIHOODS[likelihood], int(u16), x.shape[0], x.shape[1], hl.shape[1], hl.shape[1], 2, library.shape[0],
                 int(bool(x_identity)), ldl, stream, step, cell_base], np.int32)
  fp = np.array([clip_library, grad_scale, kl_weight], np.float32)
  o = dict(draw=np.empty((B, ld), np.float32), latl=np.empty((B, ldl), np.float32), dlatl=np.empty((B, ldl), np.float32))
  for name in ("llk_part", "l", "sig", "eps", "kl", "dl"):
    o[name] = np.empty(B, np.float32)
  p = {name: (None if name in omit else _fp(a)) for name, a in o.items()}
  ok = C.c_int32(0)
  check(lib.smx_k_scvi_head_train(_ip(ip), _fp(fp), _fp(raw), x.ctypes.data_as(C.c_void_p), _fp(hl), _fp(Wl), _fp(bl), _fp(library),
                                  _ip(rw), _fp(ep), int(seed), p["draw"], p["llk_part"], p["l"], p["sig"], p["eps"], p["kl"],
                                  p["latl"], p["dlatl"], p["dl"], C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o


def k_scvi_head_fwd(raw, l, G, k=3, clip_library=1e3, Gp=None, plane_stride=None, ld=None, omit=()):
  """The separate forward launch of the scVI gene head (smx_k_scvi_head_fwd): raw [B][ld], l [B] -> dict(planes [B][ld], rho_raw [B][Gp],
  guards_ok)"""
  lib = _hip.require_gpu()
  Gp, ps, ld = _scvi_layout(G, k, Gp, plane_stride, ld)
  raw = _f32(raw)
  B = raw.shape[0]
  raw, l = _f32(raw.reshape(B, -1), (B, ld)), _f32(l, (B,))
  ip, fp = np.array([B, G, Gp, ps, ld, k], np.int32), np.array([clip_library], np.float32)
  o = dict(planes=np.empty((B, ld), np.float32), rho_raw=np.empty((B, Gp), np.float32))
  p = {name: (None if name in omit else _fp(a)) for name, a in o.items()}
  ok = C.c_int32(0)
  check(lib.smx_k_scvi_head_fwd(_ip(ip), _fp(fp), _fp(raw), _fp(l), p["planes"], p["rho_raw"], C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o


def k_scvi_head_bwd(planes, dplanes, rho_raw, l, G, k=3, clip_library=1e3, Gp=None, plane_stride=None, ld=None, omit=()):
  """The separate backward launch of the scVI gene head (smx_k_scvi_head_bwd) on its inputs: planes, dplanes [B][ld], rho_raw [B][Gp],
  l [B] -> dict(draw [B][ld], dl [B], guards_ok)"""
  lib = _hip.require_gpu()
  Gp, ps, ld = _scvi_layout(G, k, Gp, plane_stride, ld)
  planes = _f32(planes)
  B = planes.shape[0]
  planes, dplanes = _f32(planes.reshape(B, -1), (B, ld)), _f32(np.asarray(dplanes).reshape(B, -1), (B, ld))
  rho_raw, l = _f32(rho_raw, (B, Gp)), _f32(l, (B,))
  ip, fp = np.array([B, G, Gp, ps, ld, k], np.int32), np.array([clip_library], np.float32)
  o = dict(draw=np.empty((B, ld), np.float32), dl=np.empty(B, np.float32))
  p = {name: (None if name in omit else _fp(a)) for name, a in o.items()}
  ok = C.c_int32(0)
  check(lib.smx_k_scvi_head_bwd(_ip(ip), _fp(fp), _fp(planes), _fp(dplanes), _fp(rho_raw), _fp(l), p["draw"], p["dl"], C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o


def _label_kind(kind: str):
  """'nb' .. 'normal', 'mixnb3' .. 'mixtril2' -> (smx_label_likelihood, components)"""
  from sisua_amd.config import MIXTURE_HEAD_KINDS
  for base in MIXTURE_HEAD_KINDS:
    if kind.startswith(base) and kind[len(base):].isdigit():
      return _hip.LABEL_LIKELIHOODS[base], int(kind[len(base):])
  return _hip.LABEL_LIKELIHOODS[kind], 1


def k_label_loss(kind: str, raw, Y, P: int, Pp=None, ld=None, rows=None, mask=None, observed=False, grad_scale=1.0, add=False, backward=True,
                 llk_in=None, fill=np.nan):
  """The label heads' launch by itself (smx_k_label_loss).  kind: 'nb', 'nbd', 'zinb', 'zinbd', 'bernoulli', 'normal', 'onehot', 'mixnbC',
  'mixzinbC', 'mixgaussC', 'mixtrilC'.  raw [B][ld] in the step's layout (plane c of a row at c * Pp, Pp = P rounded up to 32 unless given,
  ld = planes * Pp unless given); Y [n_rows][ldy]; rows [B] (None: cell b = row b); mask [n_rows] (None: no cell is labelled).  llk_in [B]:
  the accumulator the launch finds (zeros); fill: what draw [B][ld] holds before the launch, a scalar or an array.  Returns dict(llk [B],
  draw [B][ld], guards_ok)."""
  lib = _hip.require_gpu()
  code, C_ = _label_kind(kind)
  P = int(P)
  Pp = (P + 31) // 32 * 32 if Pp is None else int(Pp)
  raw = _f32(raw)
  if raw.ndim != 2:
    raise ValueError(f"raw must be [B][ld], got {raw.shape}")
  B = raw.shape[0]
  ld = raw.shape[1] if ld is None else int(ld)
  raw, Y = _f32(raw, (B, ld)), _f32(Y)
  if Y.ndim != 2:
    raise ValueError(f"Y must be [n_rows][ldy], got {Y.shape}")
  rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
  mk = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
  if (rw is not None and rw.shape != (B,)) or (mk is not None and mk.shape != (Y.shape[0],)):
    raise ValueError("rows must be [B] and mask [n_rows]")
  llk = np.zeros(B, np.float32) if llk_in is None else _f32(llk_in, (B,)).copy()
  draw = np.ascontiguousarray(np.broadcast_to(np.asarray(fill, np.float32), (B, ld))).copy()
  ip = np.array([code, C_, B, P, Pp, ld, Y.shape[1], Y.shape[0], int(bool(observed)), int(bool(add)), int(bool(backward))], np.int32)
  fp = np.array([grad_scale], np.float32)
  ok = C.c_int32(0)
  check(lib.smx_k_label_loss(_ip(ip), _fp(fp), _fp(raw), _fp(Y), _ip(rw), _ptr(mk, np.uint8), _fp(llk), _fp(draw), C.byref(ok)))
  return dict(llk=llk, draw=draw, guards_ok=bool(ok.value))
