"""Times the large-page LZ4 kernels (lz4_encode_large.hip, lz4_decode_large.hip) on dist0 pages,
warm and by HIP events on the launch stream, the way tools/time_codecs.py does:

    SHAPES=8192x131072,1024x1048576,1x4194304 python tools/time_large.py

One JSON line per shape: ratio, compress / decompress ms and GiB/s of uncompressed bytes.  Beside
each, the reference codec on the host gives the yardstick:

    oracle/_ref/cpu_baseline lz4 <pages> <page_len> 16
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tyche_amd import codec  # noqa: E402

GIB = float(1 << 30)
reps = int(os.environ.get("REPS", "3"))
dev = torch.device("cuda:0")


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = float("inf")
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        best = min(best, ev[0].elapsed_time(ev[1]))
    return best


def shape(n, plen):
    pages = codec.pagegen(n, plen, dist=0, device=dev)
    comp, clen = codec.compress_pages(pages)
    torch.cuda.synchronize()
    mx = int(clen.max())
    out, rv = codec.decompress_pages(comp, clen, plen, max_comp_len=mx)
    torch.cuda.synchronize()
    assert bool((rv == plen).all()) and torch.equal(out, pages), (n, plen)
    c_ms = timed(lambda: codec.compress_pages(pages, out=comp, out_len=clen))
    d_ms = timed(lambda: codec.decompress_pages(comp, clen, plen, out=out, rv=rv, max_comp_len=mx))
    nbytes = n * plen
    r = {"codec": "lz4", "page_len": plen, "pages": n, "ratio": round(nbytes / int(clen.to(torch.int64).sum()), 3),
         "compress_ms": round(c_ms, 3), "decompress_ms": round(d_ms, 3),
         "compress_gib_s": round(nbytes / c_ms / 1e-3 / GIB, 3), "decompress_gib_s": round(nbytes / d_ms / 1e-3 / GIB, 3)}
    del pages, comp, clen, out, rv
    torch.cuda.empty_cache()
    return r


if __name__ == "__main__":
    for s in os.environ.get("SHAPES", "8192x131072,1024x1048576,1x4194304").split(","):
        n, plen = s.split("x")
        print(json.dumps(shape(int(n), int(plen))), flush=True)
