"""160 eager steps of a SISUA (1998 genes zinb, B 128) with one 32-dimensional label head of the given kind, half the cells labelled,
for kernel traces of label_loss_kernel:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/head_kind_profile.py bernoulli      (or nb / normal)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sisua_amd.config import ModelConfig
from sisua_amd.engine import Engine
from tests.util import synth_counts
from tests import head_kinds_ref as ref

kind = sys.argv[1]
P = 32
cfg = ModelConfig(model="sisua", n_genes=1998, likelihood="zinb", enc_units=(128,), dec_units=(128,), latent_dim=32,
                  labels=((P, kind),), alpha=10.0)
x = synth_counts(2048, 1998, sparsity=0.9, seed=0)
y = ref.synth_targets(2048, ((P, kind),))[0] if kind != "nb" else np.random.default_rng(1).poisson(5.0, size=(2048, P)).astype(np.float32)
mask = (np.random.default_rng(2).uniform(size=2048) < 0.5).astype(np.uint8)
e = Engine(cfg, max_batch=128)
e.upload(x, [y], None, mask)
order = np.random.default_rng(3).permutation(2048)[: 128 * 16].astype(np.int32)
for _ in range(10):
  e.train_steps(order, 16, 128, graph=False)
print(kind, e.metrics_history(16)["loss"][-1])
e.close()
