"""Times the zlib shared-dictionary kernels beside the plain ones: device-resident batches of
PAGES x PLEN dist-0 pages, dictionaries of 4 KiB and 16 KiB (one more page of the distribution, cut),
HIP events around each call, warm, the median of REPS:

    PAGES=65536 PLEN=16384 python tools/time_zlib_dict.py
    SCALE=1 python tools/time_zlib_dict.py        # also both decoders at 64, 256 and 1,024 pages
    PLAIN_ONLY=1 TYCHE_CODEC_LIB=<an older libtyche_codec.so> python tools/time_zlib_dict.py
                                                  # the plain rows alone, from another build of the library

The reference's dictionary functions on host threads over the same pages: tools/zlib_dict_host.c.
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tyche_amd import codec  # noqa: E402

n = int(os.environ.get("PAGES", "65536"))
plen = int(os.environ.get("PLEN", "16384"))
reps = int(os.environ.get("REPS", "7"))
ZLIB = 2
dev = torch.device("cuda:0")


def row(name, ms, nbytes, **kw):
    med, lo, hi = ms
    print(json.dumps({"what": name, "pages": kw.pop("pages", n), "page_len": plen, "ms_median": round(med, 3),
                      "ms_min": round(lo, 3), "ms_max": round(hi, 3), "GBps": round(nbytes / med / 1e6, 2), **kw}), flush=True)


def timed(fn):
    fn()
    fn()                                   # warm: code object loaded, pools and counters allocated
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


pages = codec.pagegen(n, plen, dist=0, first=0, device=dev)
dict_src = codec.pagegen(1, 32768, dist=0, first=n + 5, device=dev).cpu().numpy().tobytes()
slot = codec.slot_size(plen, ZLIB)
comp = torch.empty((n, slot), dtype=torch.uint8, device=dev)
clen = torch.empty((n,), dtype=torch.int32, device=dev)
out = torch.empty((n, plen), dtype=torch.uint8, device=dev)
rv = torch.empty((n,), dtype=torch.int32, device=dev)
total = n * plen
small = [k for k in (64, 256, 1024) if k <= n] if os.environ.get("SCALE") else []
lib = os.environ.get("TYCHE_CODEC_LIB", "this build")

ms = timed(lambda: codec.compress_pages(pages, ZLIB, out=comp, out_len=clen))
plain_bytes = int(clen.sum())
row("plain encode", ms, total, ratio=round(total / plain_bytes, 4), library=lib)
plain_enc = ms[0]
ms = timed(lambda: codec.decompress_pages(comp, clen, plen, ZLIB, out=out, rv=rv))
assert bool((rv == plen).all()) and torch.equal(out, pages)
row("plain decode", ms, total, library=lib)
plain_dec = ms[0]
for k in small:
    ms = timed(lambda: codec.decompress_pages(comp[:k], clen[:k], plen, ZLIB, out=out[:k], rv=rv[:k]))
    row("plain decode", ms, k * plen, pages=k, library=lib)
if os.environ.get("PLAIN_ONLY"):
    sys.exit(0)

for D in (4096, 16384):
    d = codec.Dictionary(dict_src[:D])
    ms = timed(lambda: codec.compress_pages(pages, ZLIB, out=comp, out_len=clen, dictionary=d))
    dict_bytes = int(clen.sum())
    row(f"dictionary encode D={D}", ms, total, ratio=round(total / dict_bytes, 4), times_plain=round(ms[0] / plain_enc, 2),
        ratio_gain_pct=round(100.0 * (plain_bytes / dict_bytes - 1.0), 2))
    ms = timed(lambda: codec.decompress_pages(comp, clen, plen, ZLIB, out=out, rv=rv, dictionary=d))
    assert bool((rv == plen).all()) and torch.equal(out, pages)
    row(f"dictionary decode D={D}", ms, total, times_plain=round(ms[0] / plain_dec, 2))
    for k in small:
        ms = timed(lambda: codec.decompress_pages(comp[:k], clen[:k], plen, ZLIB, out=out[:k], rv=rv[:k], dictionary=d))
        row(f"dictionary decode D={D}", ms, k * plen, pages=k)
    d.close()
