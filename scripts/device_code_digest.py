#!/usr/bin/env python
"""sha256 of the gfx950 machine code of every kernel file, to show that a host-only change moved no device code.

For each ``csrc/kernels/*.hip`` the newest object under ``<root>/build/obj`` (build first, with the same flags
in both trees) gives its ``.hip_fatbin`` section; the ``hipv4-amdgcn-amd-amdhsa--gfx950`` entry is unbundled
from it and the ``.text`` and ``.rodata`` sections of that code object are hashed. Whole code objects are not
compared: they embed a per-compilation symbol suffix, so any edit of the file changes them.

Usage: ``python scripts/device_code_digest.py [--root TREE] [--against OTHER_TREE]`` prints one line per kernel
file (``file  text-sha256  rodata-sha256``); with ``--against`` it exits 1 when any digest differs.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950").split(";")[0]
LLVM = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin"


def _section(obj: Path, name: str, out: Path) -> bytes:
    out.unlink(missing_ok=True)
    subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section={name}={out}", str(obj), os.devnull], check=True)
    return out.read_bytes()


def digests(root: Path) -> dict[str, tuple[str, str]]:
    res = {}
    with tempfile.TemporaryDirectory() as td:
        tmp = Path(td)
        for src in sorted((root / "csrc" / "kernels").glob("*.hip")):
            objs = sorted((root / "build" / "obj").glob(f"{src.stem}-*.o"), key=lambda p: p.stat().st_mtime)
            if not objs:
                raise SystemExit(f"no object for {src.name} under {root / 'build' / 'obj'}: build the tree first")
            (tmp / "fatbin").write_bytes(_section(objs[-1], ".hip_fatbin", tmp / "fatbin.raw"))
            co = tmp / "code.o"
            subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o",
                            f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}", f"--input={tmp / 'fatbin'}",
                            f"--output={co}"], check=True)
            res[src.name] = tuple(hashlib.sha256(_section(co, s, tmp / "sec")).hexdigest() for s in (".text", ".rodata"))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    here = Path(__file__).resolve().parent.parent
    ap.add_argument("--root", type=Path, default=here, help="tree whose build/obj is read (default: this one)")
    ap.add_argument("--against", type=Path, default=None, help="a second built tree to compare with")
    a = ap.parse_args(argv)
    mine = digests(a.root)
    other = digests(a.against) if a.against else None
    bad = 0
    for name, (text, rodata) in mine.items():
        mark = ""
        if other is not None:
            same = other.get(name) == (text, rodata)
            bad += not same
            mark = "  same" if same else f"  DIFFERS from {other.get(name)}"
        print(f"{name:24s} {text} {rodata}{mark}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
