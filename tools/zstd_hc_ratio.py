"""Writes profiles/zstd_hc_ratio.jsonl: per bench distribution (0, 1, 2, 5) and page length (4096,
16384, 32768), the byte totals of the first 48 oracle.pagegen pages from the default device encoder,
from ZSTD_HC=1, and from the reference's levels 1 and 6 (tests/golden/zstd_hc_targets.json), with
the share of the level-1-to-6 gap that the mode closes.  The cells tests/test_gpu_zstd_hc.py judges.

    python tools/zstd_hc_ratio.py [out.jsonl]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from tyche_amd import _lib, codec  # noqa: E402

ZSTD = _lib.COMPRESSOR_IDS["zstd"]
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "zstd_hc_ratio.jsonl")
with open(os.path.join(ROOT, "tests", "golden", "zstd_hc_targets.json")) as f:
    targets = json.load(f)


def total(host, knob):
    _lib.set_knob("ZSTD_HC", knob)
    try:
        comp, clen = codec.compress_pages(torch.from_numpy(host).to("cuda:0"), compressor_id=ZSTD)
        torch.cuda.synchronize()
        return int(clen.sum())
    finally:
        _lib.clear_knob("ZSTD_HC")


with open(out_path, "w") as f:
    for key, (l1, l6) in sorted(targets["cells"].items(), key=lambda kv: [int(x) for x in kv[0].split("/")]):
        dist, plen = (int(x) for x in key.split("/"))
        host = O.pagegen(targets["pages"], plen, dist=dist)
        d, h = total(host, 0), total(host, 1)
        rec = {"lib": os.path.basename(_lib.LIB_PATH), "dist": dist, "page_len": plen, "pages": targets["pages"],
               "device_default": d, "device_hc": h, "level1": l1, "level6": l6, "share_closed": round((l1 - h) / (l1 - l6), 3)}
        f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)
