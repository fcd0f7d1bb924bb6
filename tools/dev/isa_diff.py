#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two builds: which kernels exist in one and not the other, and, for the kernels of
both, whether the instruction text and the kernel metadata (registers, LDS, scratch, arguments, wave size) are identical.  Addresses,
encodings and the padding behind a function are left out.  For moving code between sources: a move that changes no kernel shows nothing.
    python tools/dev/isa_diff.py OLD/sisua_amd/csrc NEW/sisua_amd/csrc     # directories of built objects (*.o), or two objects
Exit status 1 when a kernel present in both differs."""
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isa_lint import LLVM, TARGET  # noqa: E402

_FUNC = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def kernels(path):
  """{kernel symbol: (instruction lines, metadata lines)} of one host object"""
  with open(path, "rb") as f:
    if b".hip_fatbin" not in f.read():   # host code only
      return {}
  with tempfile.TemporaryDirectory() as td:
    fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, path], check=True)
    subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co],
                   check=True, stderr=subprocess.DEVNULL)
    asm = subprocess.run([LLVM + "/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
  code, name = {}, None
  for line in asm.split("\n"):
    m = _FUNC.match(line)
    if m:
      name = m.group(1)
      code[name] = []
    elif name and line.strip():
      code[name].append(line.split("//")[0].strip())
  for c in code.values():   # the padding up to the next function's alignment depends on where the function sits
    while c and c[-1] in ("s_nop 0", "s_code_end", "..."):
      c.pop()
  meta = {}
  for block in re.split(r"\n  - (?=\.agpr_count)", notes.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0]):
    m = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
    if m:
      meta[m.group(1)] = block.strip().split("\n")
  return {k: (code.get(k, []), v) for k, v in meta.items()}


def library(path):
  objs = sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]
  out = {}
  for o in objs:
    for k, v in kernels(o).items():
      out.setdefault(k, []).append(v)   # (a kernel built in two units appears twice)
  return out


def main():
  if len(sys.argv) != 3:
    print(__doc__)
    return 2
  a, b = library(sys.argv[1]), library(sys.argv[2])
  for k in sorted(set(a) - set(b)):
    print("only in old:", k)
  for k in sorted(set(b) - set(a)):
    print("only in new:", k)
  common = sorted(set(a) & set(b))
  differ = [k for k in common if sorted(a[k]) != sorted(b[k])]
  for k in differ:
    print("differs:", k, "(metadata)" if sorted(m for _, m in a[k]) != sorted(m for _, m in b[k]) else "(instructions)")
  print("isa_diff: %d kernels in old, %d in new, %d in both, %d of them differ" % (len(a), len(b), len(common), len(differ)))
  return 1 if differ else 0


if __name__ == "__main__":
  sys.exit(main())
