#!/usr/bin/env python3
"""Records tests/golden/zlib_dict.npz: what the reference library (zlib 1.2.8 from oracle/_ref,
driven through a ctypes z_stream: deflateInit_, deflateSetDictionary, deflate, inflateInit_,
inflateSetDictionary, inflate) answers for the shared-dictionary cases of tests/zlib_dict_cases.py, so
that the verdict and ratio tests never depend on that library being present.  Results only: streams
the reference made, its return values, checksums of what it decoded, and its compressed sizes.

    python tools/gen_zlib_dict_golden.py            # needs oracle/_ref/libtyche_ref.so
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zlib_dict_cases as C   # noqa: E402
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
    # premises of the contract (include/tyche_codec.h, "zlib with a shared dictionary")
    dic, page = C.dict_of(O, 4096), C.page_of(O, 4096, 4096, "dist0")
    s = R.compress(dic, page)
    assert s[:6] == C.dict_header(dic), "level 1 with a dictionary: 78 3F and the dictionary's adler32"
    assert s[-4:] == C.adler(page).to_bytes(4, "big"), "the trailer covers the page alone"
    assert R.decompress(None, s, 4096) == (C.Z_DATA, b""), "Z_NEED_DICT without a dictionary is Z_DATA_ERROR"
    rnd = C.page_of(O, 4096, 100, "random")
    assert len(R.compress(dic, rnd)) == 115 > C.zlib_bound(100) == 113, "zlib overruns compressBound with a DICTID"
    assert R.compress(dic, b"") == C.dict_header(dic) + bytes([3, 0, 0, 0, 0, 1]), "the empty page behind the dictionary header"
    rt = []
    for D, L, k, dic, page in C.all_cases(O, C.golden_pairs()):
        f = R.compress(dic, page)
        assert R.decompress(dic, f, L) == (L, page), (D, L, k)
        assert C.py_decompress(dic, f, L) == (L, page), (D, L, k)
        assert f[:6] == C.dict_header(dic), (D, L, k)
        rt.append(f)
    out["rt_data"], out["rt_off"], out["rt_len"] = pack(rt)
    rv, crc = [], []
    for name, dic, stream, cap, want in C.crafted_cases():
        r, dec = R.decompress(dic, stream, cap)
        # the cases are what they are meant to be, by the reference and by Python's zlib
        if isinstance(want, bytes):
            assert (r, dec) == (len(want), want), (name, r)
            assert C.py_decompress(dic, stream, cap) == (r, dec), name
        else:
            assert r == want, (name, r, want)
            assert C.py_decompress(dic, stream, cap)[0] == want, name
        rv.append(r)
        crc.append(C.crc(dec))
    out["crafted_rv"], out["crafted_crc"] = np.array(rv, np.int32), np.array(crc, np.uint32)
    dic, streams = C.malformed_cases(O)
    rv, crc = [], []
    for f, cap in streams:
        r, dec = R.decompress(dic, f, cap)
        rv.append(r)
        crc.append(C.crc(dec))
    out["malformed_rv"], out["malformed_crc"] = np.array(rv, np.int32), np.array(crc, np.uint32)
    used, used_plain = [], []
    for L in C.USED_LS:
        dic, page = C.used_case(L)
        used.append(len(R.compress(dic, page)))
        used_plain.append(len(R.compress(b"", page)))
        print(f"dictionary-is-used L={L}: {used[-1]} bytes with the dictionary, {used_plain[-1]} without")
    out["used_ref"], out["used_ref_plain"] = np.array(used, np.int64), np.array(used_plain, np.int64)
    ratio, plain = [], []
    for n, dist in C.RATIO_CELLS:
        dic, pages = C.ratio_inputs(O, n, dist)
        ratio.append(sum(len(R.compress(dic, pages[i].tobytes())) for i in range(len(pages))))
        plain.append(sum(len(R.compress(b"", pages[i].tobytes())) for i in range(len(pages))))
        print(f"{n} B pages, dist {dist}: {plain[-1]} -> {ratio[-1]} bytes with the dictionary ({ratio[-1] / plain[-1]:.4f})")
    out["ratio_ref"], out["ratio_ref_plain"] = np.array(ratio, np.int64), np.array(plain, np.int64)
    np.savez_compressed(C.GOLDEN_FILE, **out)
    print(C.GOLDEN_FILE, os.path.getsize(C.GOLDEN_FILE), "bytes;", len(rt), "round-trip streams,", len(out["crafted_rv"]),
          "crafted verdicts,", len(rv), "malformed verdicts")


if __name__ == "__main__":
    main()
