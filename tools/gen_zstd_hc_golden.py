#!/usr/bin/env python3
"""Writes tests/golden/zstd_hc_targets.json: the byte totals of the reference's ZSTD_compress
(the vendored 1.1.2 through oracle.ref_zstd_compress, where oracle/_ref is built) at levels 1 and 6
over the first 48 oracle.pagegen pages of distributions 0, 1, 2, 5 at 4096, 16384 and 32768 bytes.
Recorded results only: tests/test_gpu_zstd_hc.py holds ZSTD_HC=1 to half of the gap between the two
levels wherever level 6 saves at least 2 %.

    python tools/gen_zstd_hc_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zstd_hc_cases as C  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    if not O.have_ref():
        sys.exit("oracle/_ref is not built (make -C oracle ref)")
    cells = {}
    for dist in C.RATIO_DISTS:
        for plen in C.RATIO_LENS:
            pages = O.pagegen(C.RATIO_PAGES, plen, dist=dist)
            l1 = sum(len(O.ref_zstd_compress(p.tobytes(), 1)) for p in pages)
            l6 = sum(len(O.ref_zstd_compress(p.tobytes(), 6)) for p in pages)
            cells[f"{dist}/{plen}"] = [l1, l6]
            print(f"dist {dist} L {plen}: level 1 {l1:,} level 6 {l6:,} ({100 * (l1 - l6) / l1:.1f} %)")
    with open(C.TARGETS, "w") as f:
        json.dump({"pages": C.RATIO_PAGES, "levels": [1, 6], "cells": cells}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
