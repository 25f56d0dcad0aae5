#!/usr/bin/env python3
"""sha256 of each source's gfx950 device assembly: makes "no kernel changed" checkable.

    python tools/device_asm_digest.py [-DNAME[=V] ...] [source.hip ...]

Compiles every file of _build.SOURCES (or only the ones named) with the product flags
(_build.FLAGS + SOURCE_FLAGS) plus --cuda-device-only -S and any -D given, drops the lines
holding the compiler's per-unit id symbol (__hip_cuid_<hash>, which follows the source text),
and prints "<sha256>  <file>".  Two trees whose listings are equal build the same kernels.
It only hashes, and it needs hipcc but no GPU.
"""
import concurrent.futures as cf
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tyche_amd import _build  # noqa: E402


def digest(src: str, defines: list) -> str:
    cmd = [_build.HIPCC] + _build.FLAGS + _build.SOURCE_FLAGS.get(src, []) + defines + \
        ["--cuda-device-only", "-S", os.path.join(_build.CSRC, src), "-o", "-"]
    asm = subprocess.run(cmd, check=True, stdout=subprocess.PIPE).stdout
    kept = [line for line in asm.splitlines(keepends=True) if b"__hip_cuid_" not in line]
    return hashlib.sha256(b"".join(kept)).hexdigest()


def main() -> None:
    defines = [a for a in sys.argv[1:] if a.startswith("-D")]
    sources = [a for a in sys.argv[1:] if not a.startswith("-D")] or _build.SOURCES
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        for src, d in zip(sources, ex.map(lambda s: digest(s, defines), sources)):
            print(f"{d}  {src}")


if __name__ == "__main__":
    main()
