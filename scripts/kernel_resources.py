#!/usr/bin/env python3
"""Registers, scratch and LDS of every kernel of a built library, from the code object's metadata note - and, with two libraries, what
differs between them.  A change that must not touch the step kernels (a new kernel that reaches the shared out-of-line functions can raise
their register count: DESIGN.md, determinize) is checked with

    python scripts/kernel_resources.py OLD.so NEW.so --match 'k_step|rollout'

which prints every kernel of either library whose (vgpr, agpr, sgpr, scratch bytes, LDS bytes) differ and exits 1 if one matches."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lint_isa_last_vgpr import extract_code_object  # noqa: E402

READELF = os.environ.get("LLVM_READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def resources(path):
    """{kernel name: (vgpr, agpr, sgpr, scratch, lds)}"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(extract_code_object(path))
        f.flush()
        notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        block = "  - .agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        vals = []
        for k in FIELDS:
            m = re.search(re.escape(k) + r":\s+(\d+)", block)
            vals.append(int(m.group(1)) if m else 0)
        out[name.group(1)] = tuple(vals)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--match", default="")
    a = ap.parse_args()
    res = [resources(p) for p in a.libs[:2]]
    if len(res) == 1:
        for k, v in sorted(res[0].items()):
            if re.search(a.match, k):
                print(k, *v)
        return 0
    old, new = res
    bad = 0
    same = sum(1 for k in old if k in new and old[k] == new[k] and re.search(a.match, k))
    for k in sorted(set(old) | set(new)):
        if old.get(k) != new.get(k):
            hit = bool(re.search(a.match, k)) and k in old and k in new
            bad += hit
            print(("DIFFERS " if hit else "other   ") + k, old.get(k), "->", new.get(k))
    print(f"{same} kernels matching {a.match!r} have equal (vgpr, agpr, sgpr, scratch, lds); {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
