#!/usr/bin/env python3
"""Writes tests/golden/zlib_hc_targets.json: the byte totals of the reference's compress2 (the
vendored zlib 1.2.8 through oracle.ref_zlib_compress, where oracle/_ref is built) at levels 1 and 6
over 48 oracle.pagegen pages (first=1000) of distributions 0, 1, 2, 5 at 4096, 16384 and 32768
bytes.  Recorded results only: the tests hold ZLIB_HC=1 to half of the gap between the two levels
in the cells of distributions 0, 1 and 5, and to the default encoder's size in all of them.

    python tools/gen_zlib_hc_golden.py
    TYCHE_CODEC_LIB=<the parent commit's libtyche_codec.so> python tools/gen_zlib_hc_golden.py --digests
        # on the GPU: tests/golden/zlib_default_digests.json, the length and sha256 (first 32 hex digits) of the
        # default zlib encoder's stream per page of zlib_hc_cases.knob_off_sets, from the library as it stood
        # before ZLIB_HC (test_gpu_zlib_hc.py: the knob-off path keeps these bytes)
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zlib_hc_cases as C  # noqa: E402
from oracle import oracle as O  # noqa: E402


def digests():
    import batch_contract_cases as BC
    import batch_layout as BL
    from tyche_amd import _lib, codec
    assert _lib.load().tyche_device_ready() == 1, _lib.last_error()
    print("library:", _lib.LIB_PATH)
    out = {}
    for group, pages in C.knob_off_sets(O).items():
        lay = BL.build(pages, [codec.compress_bound(len(p), 2) for p in pages], BC.src_shifts(len(pages)),
                       BC.dst_shifts(len(pages)), ("random", 9))
        rv, dst, src = BC.device_compress(codec, lay, 2, max_src_length=65535)
        streams = BL.outputs(dst, rv, lay)
        assert all(int(r) > 0 for r in rv)
        out[group] = {"len": [len(s) for s in streams], "sha": [hashlib.sha256(s).hexdigest()[:32] for s in streams]}
        print(group, len(streams), "streams,", sum(len(s) for s in streams), "bytes")
    with open(os.environ.get("DIGESTS_OUT", C.DEFAULT_DIGESTS), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


def main():
    if "--digests" in sys.argv:
        return digests()
    if not O.have_ref():
        sys.exit("oracle/_ref is not built (make -C oracle ref)")
    cells = {}
    for dist in C.RATIO_DISTS + C.NOGROW_DISTS:
        for plen in C.RATIO_LENS:
            pages = C.ratio_pages(O, dist, plen)
            l1 = sum(len(O.ref_zlib_compress(p.tobytes(), 1)) for p in pages)
            l6 = sum(len(O.ref_zlib_compress(p.tobytes(), 6)) for p in pages)
            cells[f"{dist}/{plen}"] = [l1, l6]
            print(f"dist {dist} L {plen}: level 1 {l1:,} level 6 {l6:,} ({100 * (l1 - l6) / l1:.1f} %)")
    with open(C.TARGETS, "w") as f:
        json.dump({"pages": C.RATIO_PAGES, "first": C.RATIO_FIRST, "levels": [1, 6], "cells": cells}, f, indent=1,
                  sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
