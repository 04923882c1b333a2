#!/usr/bin/env python3
"""Kernel table of a libsmfv.so's gfx950 code object, or the diff of two.

    python scripts/codeobj_kernels.py LIB                 # name vgpr sgpr spill bytes
    python scripts/codeobj_kernels.py OLD NEW [NAME..]    # kernels of OLD that differ in NEW

Registers and spills come from the code object's metadata (llvm-readelf
--notes), the code size from its symbol table.  With two libraries the exit
status is 1 if any kernel of OLD (of the given kernel names, e.g. k_rows_ws
k_rows_mh; default: every kernel) is missing from NEW or differs in VGPRs,
SGPRs, spills or code size: the check that a change left the instances it did
not mean to touch exactly as they were.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")


def kernels(lib: str) -> dict[str, tuple[int, int, int, int]]:
    """mangled kernel name -> (vgprs, sgprs, vgpr spills, code bytes)"""
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=tmp, capture_output=True,
                       check=True)
        co = [f for f in os.listdir(tmp) if "gfx950" in f]
        if not co:
            raise SystemExit(f"{lib}: no gfx950 code object")
        co = os.path.join(tmp, co[0])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True,
                               check=True).stdout
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", co], capture_output=True,
                              text=True, check=True).stdout
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
    out = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))  # noqa: E731
        out[name] = (get("vgpr_count"), get("sgpr_count"), get("vgpr_spill_count"), size.get(name, -1))
    return out


def main(argv: list[str]) -> int:
    if len(argv) == 1:
        k = kernels(argv[0])
        for n in sorted(k):
            print(*k[n], n)
        return 0
    # k_rows / k_rows_mh gained a trailing, possibly empty template pack (the
    # epilogue argument): an instance with the empty pack is the old instance,
    # mangled with "JE" after its template arguments and "DpT<n>_" after its
    # parameters
    plain = lambda n: re.sub(r"DpT\d*_$", "", re.sub(r"JE(?=EEv)", "", n))  # noqa: E731
    old, new = ({plain(n): v for n, v in kernels(lib).items()} for lib in argv[:2])
    checked = bad = 0
    for n in sorted(old):
        # _ZN4smfv<len><name>I...: the kernel's own name follows the namespace
        m = re.match(r"_ZN4smfv\d+([A-Za-z_0-9]+?)(?:I|E)", n)
        short = m.group(1) if m else n
        if len(argv) > 2 and short not in argv[2:]:
            continue
        checked += 1
        if new.get(n) != old[n]:
            bad += 1
            print("DIFF", n, old[n], "->", new.get(n))
    print(f"{checked} kernels of {argv[0]} checked, {bad} differ; {len(new) - len(old)} more kernels in {argv[1]}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    raise SystemExit(main(sys.argv[1:]))
