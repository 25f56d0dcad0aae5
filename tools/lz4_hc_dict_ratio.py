"""Writes profiles/lz4_hc_dict_ratio.jsonl: what the LZ4_HC_DICT=1 parse (through its host emulator,
tools/lz4_hc_dict_emul.cpp, whose bytes the kernel's equal) gains over the default dictionary
encoder (tools/lz4_dict_emul.cpp) and over plain LZ4_HC=1 (tools/lz4_hc_emul.cpp) -- one line per
page size of 4, 8 and 16 KiB, dictionary of 4 KiB and of the page's size, and distribution 0..5
(lz4_dict_cases.ratio_inputs: 48 pages with one more page of the distribution, cut, as dictionary)
with the three totals, the share of single pages whose stream is longer than the default dictionary
encoder's, and, where liblz4.so.1 loads, the totals F of its fast and H of its HC dictionary mode at
level 3 with the share of the F - H gap the mode closes.  Distributions 3 and 4 are recorded like
the others; tests/test_lz4_hc_dict_emul.py judges 0, 1, 2 and 5 at 4 KiB / 4 KiB.

    python tools/lz4_hc_dict_ratio.py [out.jsonl]
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import oracle as O  # noqa: E402
import lz4_dict_cases as DC  # noqa: E402
import lz4_hc_cases as HC  # noqa: E402
import lz4_hc_dict_cases as C  # noqa: E402
import gen_lz4_hc_dict_golden as G  # noqa: E402


def load_default_dict_emul():
    lib_path, src = os.path.join(ROOT, "tools", "bin", "liblz4dictemul.so"), os.path.join(ROOT, "tools", "lz4_dict_emul.cpp")
    if not os.path.exists(lib_path) or os.path.getmtime(src) > os.path.getmtime(lib_path):
        os.makedirs(os.path.dirname(lib_path), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib_path, src])
    fn = ctypes.CDLL(lib_path).lz4_dict_emul_compress
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    return fn


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lz4_hc_dict_ratio.jsonl")
    emul, plain, default = C.load_emul(), HC.load_emul(), load_default_dict_emul()
    try:
        lz4 = G.load_liblz4()
    except OSError:
        lz4 = None
    with open(path, "w") as f:
        for plen in (4096, 8192, 16384):
            cap = C.lz4_bound(plen)
            dst = ctypes.create_string_buffer(cap)
            for dl in (4096, plen) if plen != 4096 else (4096,):
                for dist in range(6):
                    dic, pages = DC.ratio_inputs(O, plen, dist, dl)
                    bs = [p.tobytes() for p in pages]
                    mode = [emul(dic, b)[0] for b in bs]
                    dflt = [default(dic, len(dic), b, plen, dst, cap) for b in bs]
                    M, Dd, P, n = sum(mode), sum(dflt), sum(plain(b)[0] for b in bs), pages.size
                    rec = {"page_len": plen, "dict_len": dl, "dist": dist, "pages": len(bs), "hc_dict_bytes": M,
                           "default_dict_bytes": Dd, "plain_hc_bytes": P, "hc_dict_ratio": round(n / M, 4),
                           "default_dict_ratio": round(n / Dd, 4), "plain_hc_ratio": round(n / P, 4),
                           "saved_over_default_dict": round(1 - M / Dd, 4), "saved_over_plain_hc": round(1 - M / P, 4),
                           "pages_longer_than_default_dict": round(sum(m > a for m, a in zip(mode, dflt)) / len(bs), 4)}
                    if lz4 is not None:
                        F = sum(G.fast_dict(lz4, dic, b, dst, cap) for b in bs)
                        H = sum(G.hc_dict(lz4, dic, b, dst, cap) for b in bs)
                        rec["liblz4_fast_dict_bytes"], rec["liblz4_hc3_dict_bytes"] = F, H
                        rec["gap_closed"] = round((F - M) / (F - H), 4) if F != H else None
                    f.write(json.dumps(rec) + "\n")
                    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
