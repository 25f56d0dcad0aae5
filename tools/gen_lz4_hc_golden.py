"""Writes tests/golden/lz4_hc_targets.json: the total bytes of liblz4's LZ4_compress_HC at level 3
(and, for the record, level 9 and LZ4_compress_default) over the ratio test's pages,
oracle.pagegen(256, 16384, dist=d) for every distribution.  tests/test_lz4_hc_emul.py holds the
LZ4_HC=1 encoder to half of the gap between the fast parse and level 3 and reads only this file,
so it needs no liblz4.

    python tools/gen_lz4_hc_golden.py        (needs liblz4.so.1 on the host)
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
import lz4_hc_cases as C  # noqa: E402


def main():
    lz4 = ctypes.CDLL("liblz4.so.1")
    lz4.LZ4_versionString.restype = ctypes.c_char_p
    n, plen = C.RATIO_PAGES, C.RATIO_PLEN
    cap = C.lz4_bound(plen)
    dst = ctypes.create_string_buffer(cap)
    out = {"liblz4": lz4.LZ4_versionString().decode(), "pages": n, "page_len": plen, "level": 3,
           "hc_bytes": {}, "hc_bytes_first64": {}, "hc9_bytes": {}, "fast_bytes": {}}
    for d in range(6):
        pages = C.ratio_pages(O, d)
        h3 = h3_64 = h9 = f = 0
        for i, p in enumerate(pages):
            b = p.tobytes()
            h3 += lz4.LZ4_compress_HC(b, dst, plen, cap, 3)
            if i == 63:
                h3_64 = h3
            h9 += lz4.LZ4_compress_HC(b, dst, plen, cap, 9)
            f += lz4.LZ4_compress_default(b, dst, plen, cap)
        out["hc_bytes_first64"][str(d)] = h3_64
        out["hc_bytes"][str(d)], out["hc9_bytes"][str(d)], out["fast_bytes"][str(d)] = h3, h9, f
    with open(C.TARGETS, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
