#!/usr/bin/env python3
"""Records tests/golden/zstd_dict.npz: what the reference library (zstd 1.1.2 from oracle/_ref)
answers for the shared-dictionary cases of tests/zstd_dict_cases.py, so that the verdict and ratio
tests never depend on that library being present.  Results only: frames the reference made, its
return values, checksums of what it decoded, and its compressed sizes.

    python tools/gen_zstd_dict_golden.py            # needs oracle/_ref/libtyche_ref.so
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zstd_dict_cases as C   # noqa: E402
from oracle import oracle as O   # noqa: E402


def pack(blobs):
    lens = np.array([len(b) for b in blobs], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return np.frombuffer(b"".join(blobs), np.uint8), offs, lens


def main():
    if not O.have_ref():
        sys.exit("oracle/_ref/libtyche_ref.so is not built")
    R = C.Ref(O)
    out = {}
    rt = []
    for D, L, k, dic, page in C.all_cases(O, C.golden_pairs()):
        f = R.compress(dic, page)
        assert R.decompress(dic, f, L) == (L, page), (D, L, k)
        rt.append(f)
    out["rt_data"], out["rt_off"], out["rt_len"] = pack(rt)
    bd = []
    for D, L in C.BOUNDARY:
        dic, page = C.boundary_case(O, D, L)
        f = R.compress(dic, page)
        # the separation the boundary tests rest on
        assert R.decompress(dic, f, L) == (L, page), (D, L)
        assert R.decompress(dic[1:], f, L)[0] < 0, (D, L, "decodes without the dictionary's first byte")
        assert R.decompress_plain(f, L)[0] < 0, (D, L, "decodes without a dictionary")
        bd.append(f)
    out["bd_data"], out["bd_off"], out["bd_len"] = pack(bd)
    dic, frames = C.malformed_cases(O)
    rv, crc = [], []
    for f, cap in frames:
        r, dec = R.decompress(dic, f, cap)
        rv.append(r)
        crc.append(C.crc(dec))
    out["malformed_rv"], out["malformed_crc"] = np.array(rv, np.int32), np.array(crc, np.uint32)
    used, used_plain = [], []
    for L in C.USED_LS:
        dic, page = C.used_case(L)
        used.append(len(R.compress(dic, page)))
        used_plain.append(len(R.compress_plain(page)))
        print(f"dictionary-is-used L={L}: {used[-1]} bytes with the dictionary, {used_plain[-1]} without")
    out["used_ref"], out["used_ref_plain"] = np.array(used, np.int64), np.array(used_plain, np.int64)
    ratio, plain = [], []
    for n, dist in C.RATIO_CELLS:
        dic, pages = C.ratio_inputs(O, n, dist)
        ratio.append(sum(len(R.compress(dic, pages[i].tobytes())) for i in range(len(pages))))
        plain.append(sum(len(R.compress_plain(pages[i].tobytes())) for i in range(len(pages))))
        raw = pages.size
        print(f"{n} B pages, dist {dist}: ratio {raw / plain[-1]:.2f} -> {raw / ratio[-1]:.2f} with the dictionary")
        assert ratio[-1] < plain[-1]
    out["ratio_ref"], out["ratio_ref_plain"] = np.array(ratio, np.int64), np.array(plain, np.int64)
    np.savez_compressed(C.GOLDEN_FILE, **out)
    print(C.GOLDEN_FILE, os.path.getsize(C.GOLDEN_FILE), "bytes;", len(rt), "round-trip frames,", len(bd),
          "boundary frames,", len(rv), "malformed verdicts")


if __name__ == "__main__":
    main()
