"""Makes tests/golden/fit_transcript.npz: what SingleCellModel._fit asks of the engine and the control plane in every case of
tests.fit_fake.CASES, run against the recording stand-in engine (no device).  Per case `c` and transcript entry `k` (tests.fit_fake.transcript)
the file holds `{c}/{k}`: the uploads, the concatenated step orders, every step's batch size, where validation passes and checkpoints fell,
the optimiser / draws / SyncBatchNorm / schedule calls, both histories, the final step, the exception and the warnings.  None of it depends
on how the loop chunked the steps, so two runs write the same arrays.

The file describes the training loop as it was BEFORE the loop was split into sisua_amd/fit_loop.py (written at commit feafbc2) and is what
tests/test_fit_loop_host.py holds the split loop to: it is not to be regenerated from later code.
Run from the repository root:  python -m tests.golden.make_fit_transcript [output path]"""
import os
import sys

import numpy as np


def main(path):
  import sisua_amd.models as M
  from tests import fit_fake as F
  out = {}
  for name in F.CASES:
    t = F.transcript(name, M, lambda cls: setattr(M, "Engine", cls))
    print(name, "steps", t["final_step"][0], str(t["error"]) or "ok")
    out.update({f"{name}/{k}": v for k, v in t.items()})
  np.savez_compressed(path, **out)


if __name__ == "__main__":
  main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "fit_transcript.npz"))
