#!/usr/bin/env python3
"""Ratio of the high-compression zlib parse against the reference's levels, per cell of
tests/golden/zlib_hc_targets.json.

    python tools/zlib_hc_ratio.py --emul [-DZLH_HASH_LOG=9 ...]   # CPU: the emulator's records, costed with
                                                                 # an exact dynamic-Huffman size
    python tools/zlib_hc_ratio.py --gpu [--out profiles/zlib_hc_ratio.jsonl]
                                                                 # the device's default and ZLIB_HC=1 streams

Per cell it prints one JSON line: the totals, the share of the level-1-to-6 gap closed, and (GPU)
the share of pages whose HC stream is longer than the default's."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zlib_hc_cases as C  # noqa: E402
from oracle import oracle as O  # noqa: E402


def emul_cells(defines):
    tag = "".join("_" + d.replace("ZLH_", "").replace("=", "").lower() for d in defines)
    emul = C.load_emul(defines, C.LIB.replace(".so", tag + ".so")) if defines else C.load_emul()
    t = C.targets()["cells"]
    for key, (l1, l6) in sorted(t.items()):
        dist, plen = (int(x) for x in key.split("/"))
        total = 0
        for p in C.ratio_pages(O, dist, plen):
            page = p.tobytes()
            recs, last = emul(page)
            total += C.stream_size(recs, last, page)
        yield {"cell": key, "level1": l1, "level6": l6, "hc": total, "closed": round((l1 - total) / (l1 - l6), 3),
               "layout": emul.layout}


def gpu_cells():
    import torch
    from tyche_amd import _lib, codec
    t = C.targets()["cells"]
    for key, (l1, l6) in sorted(t.items()):
        dist, plen = (int(x) for x in key.split("/"))
        pages = torch.from_numpy(C.ratio_pages(O, dist, plen)).cuda()
        sizes = {}
        for hc in (0, 1):
            _lib.set_knob("ZLIB_HC", hc)
            try:
                _, n = codec.compress_pages(pages, _lib.ZLIB_COMPRESSOR_ID)
            finally:
                _lib.clear_knob("ZLIB_HC")
            sizes[hc] = n.cpu().numpy().astype("int64")
        d, h = int(sizes[0].sum()), int(sizes[1].sum())
        yield {"cell": key, "level1": l1, "level6": l6, "default": d, "hc": h,
               "closed": round((l1 - h) / (l1 - l6), 3), "fewer_bytes_pct": round(100 * (d - h) / d, 2),
               "pages_longer_pct": round(100 * float((sizes[1] > sizes[0]).mean()), 2)}


def main():
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else None
    rows = gpu_cells() if "--gpu" in args else emul_cells([a[2:] for a in args if a.startswith("-D")])
    lines = []
    for r in rows:
        lines.append(json.dumps(r, sort_keys=True))
        print(lines[-1], flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
