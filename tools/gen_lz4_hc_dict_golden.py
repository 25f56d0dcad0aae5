"""Writes tests/golden/lz4_hc_dict_targets.json: per distribution, the total bytes of liblz4's two
dictionary modes over the ratio inputs of the LZ4_HC_DICT tests (lz4_hc_dict_cases.ratio_inputs: 48
pages of 4 KiB with one more page's 4 KiB as dictionary) -- F of the fast one (LZ4_loadDict +
LZ4_compress_fast_continue, a fresh stream per page) and H of the HC one at level 3
(LZ4_loadDictHC + LZ4_compress_HC_continue).  tests/test_lz4_hc_dict_emul.py holds the encoder to
half of the gap between them and reads only this file, so it needs no liblz4.

    python tools/gen_lz4_hc_dict_golden.py        (needs liblz4.so.1 on the host)
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
import lz4_dict_cases as DC  # noqa: E402
import lz4_hc_dict_cases as C  # noqa: E402

LEVEL = 3


def load_liblz4():
    lz4 = ctypes.CDLL("liblz4.so.1")
    lz4.LZ4_versionString.restype = ctypes.c_char_p
    lz4.LZ4_createStream.restype = ctypes.c_void_p
    lz4.LZ4_createStreamHC.restype = ctypes.c_void_p
    for fn in (lz4.LZ4_freeStream, lz4.LZ4_freeStreamHC):
        fn.argtypes = [ctypes.c_void_p]
    lz4.LZ4_resetStreamHC_fast.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lz4.LZ4_resetStreamHC_fast.restype = None
    for fn in (lz4.LZ4_loadDict, lz4.LZ4_loadDictHC):
        fn.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    lz4.LZ4_compress_fast_continue.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lz4.LZ4_compress_HC_continue.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    return lz4


def fast_dict(lz4, dic: bytes, page: bytes, dst, cap: int) -> int:
    st = lz4.LZ4_createStream()
    try:
        lz4.LZ4_loadDict(st, dic, len(dic))
        return lz4.LZ4_compress_fast_continue(st, page, dst, len(page), cap, 1)
    finally:
        lz4.LZ4_freeStream(st)


def hc_dict(lz4, dic: bytes, page: bytes, dst, cap: int, level: int = LEVEL) -> int:
    st = lz4.LZ4_createStreamHC()
    try:
        lz4.LZ4_resetStreamHC_fast(st, level)
        lz4.LZ4_loadDictHC(st, dic, len(dic))
        return lz4.LZ4_compress_HC_continue(st, page, dst, len(page), cap)
    finally:
        lz4.LZ4_freeStreamHC(st)


def main():
    lz4 = load_liblz4()
    cap = C.lz4_bound(C.RATIO_PLEN)
    dst = ctypes.create_string_buffer(cap)
    out = {"liblz4": lz4.LZ4_versionString().decode(), "pages": DC.RATIO_PAGES, "page_len": C.RATIO_PLEN,
           "dict_len": C.RATIO_DICT, "level": LEVEL, "F": {}, "H": {}}
    for d in range(6):
        dic, pages = C.ratio_inputs(O, d)
        f = h = 0
        for p in pages:
            b = p.tobytes()
            rf, rh = fast_dict(lz4, dic, b, dst, cap), hc_dict(lz4, dic, b, dst, cap)
            assert rf > 0 and rh > 0
            f += rf
            h += rh
        out["F"][str(d)], out["H"][str(d)] = f, h
    with open(C.TARGETS, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
