"""Writes profiles/lz4_hc_ratio.jsonl: what the LZ4_HC=1 parse (through its host emulator,
tools/lz4_hc_emul.cpp, whose bytes the kernel's equal) gains over the reference's fast parse --
one line per page size of 4, 8, 16 and 32 KiB and distribution 0..5 (256 pages of oracle.pagegen
each) with both totals, the share of single pages whose HC stream is longer than the reference's
fast stream, and at 16 KiB liblz4's LZ4_compress_HC level 3 total from
tests/golden/lz4_hc_targets.json with the share of the gap the mode closes.  Distributions 3 and 4
are recorded like the others; tests/test_lz4_hc_emul.py judges 0, 1, 2 and 5.

    python tools/lz4_hc_ratio.py [out.jsonl]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
import lz4_hc_cases as C  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lz4_hc_ratio.jsonl")
    emul = C.load_emul()
    with open(path, "w") as f:
        for plen in (4096, 8192, 16384, 32768):
            for dist in range(6):
                pages = C.ratio_pages(O, dist, plen)
                fast = [len(O.lz4_compress(p.tobytes())) for p in pages]
                mode = [emul(p.tobytes())[0] for p in pages]
                F, M, n = sum(fast), sum(mode), pages.size
                rec = {"page_len": plen, "dist": dist, "pages": len(pages), "fast_bytes": F, "hc_mode_bytes": M,
                       "fast_ratio": round(n / F, 4), "hc_mode_ratio": round(n / M, 4), "bytes_saved": round(1 - M / F, 4),
                       "pages_longer_than_fast": round(sum(m > a for m, a in zip(mode, fast)) / len(pages), 4)}
                if plen == C.RATIO_PLEN:
                    H = C.hc3_total(dist)
                    rec["hc3_bytes"], rec["hc3_ratio"] = H, round(n / H, 4)
                    rec["gap_closed"] = round((F - M) / (F - H), 4) if F != H else None
                f.write(json.dumps(rec) + "\n")
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
