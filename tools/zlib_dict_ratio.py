"""Device bytes against the reference's (zlib 1.2.8, level 1) with and without a shared dictionary,
per cell of tests/zlib_dict_cases.RATIO_CELLS: 48 bench pages and the 49th page's first 4 KiB as
dictionary.  One JSON line per cell, the form of profiles/zlib_dict_ratio.jsonl (which the test
test_gpu_zlib_dict.py::test_ratio_against_reference writes when TYCHE_ZLIB_DICT_RATIO_LOG names a file):
q_dict = device / reference bytes with the dictionary, q_plain the same without.  The reference's
bytes come from tests/golden/zlib_dict.npz.

    python tools/zlib_dict_ratio.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zlib_dict_cases as C   # noqa: E402
from oracle import oracle as O   # noqa: E402
from tyche_amd import codec   # noqa: E402

dev = torch.device("cuda:0")
G = C.Golden()
for k, (n, dist) in enumerate(C.RATIO_CELLS):
    dic, host = C.ratio_inputs(O, n, dist)
    d = codec.Dictionary(dic)
    pages = torch.from_numpy(host).to(dev)
    _, clen = codec.compress_pages(pages, C.ZLIB, dictionary=d)
    _, plain = codec.compress_pages(pages, C.ZLIB)
    torch.cuda.synchronize()
    ours, nodict, theirs, theirs_plain = int(clen.sum()), int(plain.sum()), int(G.ratio_ref[k]), int(G.ratio_ref_plain[k])
    print(json.dumps({"page": n, "dist": dist, "dict": C.RATIO_DICT, "device": ours, "reference": theirs,
                      "device_no_dict": nodict, "reference_no_dict": theirs_plain, "q_dict": round(ours / theirs, 4),
                      "q_plain": round(nodict / theirs_plain, 4), "device_gain": round(1 - ours / nodict, 4),
                      "reference_gain": round(1 - theirs / theirs_plain, 4)}), flush=True)
    d.close()
