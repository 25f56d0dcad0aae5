#!/usr/bin/env python3
"""Records tests/golden/lz4_dict.npz: what the reference library (LZ4 1.7.5 from oracle/_ref)
answers for the shared-dictionary cases of tests/lz4_dict_cases.py, so that the verdict and ratio
tests never depend on that library being present.  Results only: streams the reference made,
its return values, checksums of what it decoded, and its compressed sizes.

    python tools/gen_lz4_dict_golden.py            # needs oracle/_ref/libtyche_ref.so
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lz4_dict_cases as C   # noqa: E402
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
    base = [R.compress(d, p) for d, p in C.base_cases(O)]
    out["base_data"], out["base_off"], out["base_len"] = pack(base)
    rv, crc = [], []
    for name, D, dic, stream, cap in C.crafted(O):
        r, dec = R.decompress(dic, stream, cap)
        rv.append(r)
        crc.append(C.crc(dec))
    out["crafted_rv"], out["crafted_crc"] = np.array(rv, np.int32), np.array(crc, np.uint32)
    dicts = [d for d, _ in C.base_cases(O)]
    rv, crc = [], []
    for name, i, stream, cap in C.malformed(base):
        r, dec = R.decompress(dicts[i], stream, cap)
        rv.append(r)
        crc.append(C.crc(dec))
    out["malformed_rv"], out["malformed_crc"] = np.array(rv, np.int32), np.array(crc, np.uint32)
    rt = [R.compress(dic, page) for D, L, k, dic, page in C.all_cases(O, C.golden_pairs())]
    out["rt_data"], out["rt_off"], out["rt_len"] = pack(rt)
    ratio = []
    for n, dist, dl in C.ratio_cases():
        dic, pages = C.ratio_inputs(O, n, dist, dl)
        ratio.append(sum(len(R.compress(dic, pages[i].tobytes())) for i in range(len(pages))))
    out["ratio_ref"] = np.array(ratio, np.int64)
    with_dict, plain = [], []
    for name, dl in C.sample_cases():
        dic, pages = C.sample_inputs(O, name, dl)
        with_dict.append(sum(len(R.compress(dic, p)) for p in pages))
        plain.append(sum(len(O.ref_lz4_compress(p)) for p in pages))
        print(f"{name} D={dl}: ratio {sum(map(len, pages)) / plain[-1]:.3f} plain, "
              f"{sum(map(len, pages)) / with_dict[-1]:.3f} with the dictionary")
    out["sample_ref"], out["sample_ref_plain"] = np.array(with_dict, np.int64), np.array(plain, np.int64)
    np.savez_compressed(C.GOLDEN_FILE, **out)
    print(C.GOLDEN_FILE, os.path.getsize(C.GOLDEN_FILE), "bytes;", len(out["crafted_rv"]), "crafted,",
          len(out["malformed_rv"]), "malformed,", len(rt), "round-trip streams")


if __name__ == "__main__":
    main()
