"""The optimiser launch of one rule (Engine.set_optimizer) at C2 -- 60 eager steps, B 128, 1998 genes zinb -- and by itself (smx_k_opt) at
the C5 shard width (the heads' W at 20 000 genes zinb over 8 ranks), for kernel traces:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/opt_rule_profile.py rmsprop '{"momentum": 0.9}'"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sisua_amd.config import ModelConfig  # noqa: E402
from sisua_amd.engine import Engine, k_opt  # noqa: E402
from tests.util import synth_counts  # noqa: E402

rule, hp = sys.argv[1], json.loads(sys.argv[2])
cfg = ModelConfig(model="vae", n_genes=1998, likelihood="zinb", enc_units=(128,), dec_units=(128,), latent_dim=32)
e = Engine(cfg, max_batch=128)
e.set_optimizer(rule, **hp)
e.upload(synth_counts(2048, 1998, seed=1))
order = np.random.default_rng(0).integers(0, 2048, 128 * 60).astype(np.int32)
e.train_steps(order, 60, 128)
e.synchronize()
e.close()
rng = np.random.default_rng(1)
n = 20000 * 3 * 128 // 8   # the heads' W at 20 000 genes zinb, one of eight shards
P, G = [rng.normal(size=n).astype(np.float32)], [rng.normal(size=n).astype(np.float32) * 1e-3]
M, V = [np.zeros(n, np.float32)], [np.full(n, 1e-4, np.float32)]
for _ in range(20):
  k_opt(rule, P, G, M, V, 3, **hp)
print("done", rule, hp)
