"""Times the LZ4 shared-dictionary kernels beside the plain ones in one run: device-resident
batches of PAGES x PLEN dist-0 pages, dictionaries of 4 KiB and 16 KiB (one more page of the
distribution, cut), HIP events around each call, warm, the median of REPS:

    PAGES=65536 PLEN=16384 python tools/time_lz4_dict.py
    SCALE=1 python tools/time_lz4_dict.py     # also the dictionary decoder at 64 .. PAGES pages
    HOST=1 PAGES=16384 python tools/time_lz4_dict.py   # instead: the host batch calls (pageable host memory in
                                                        # and out, wall clock), plain and with a process-wide dictionary
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
dev = torch.device("cuda:0")


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


def row(name, ms, nbytes, **kw):
    med, lo, hi = ms
    print(json.dumps({"what": name, "pages": kw.pop("pages", n), "page_len": plen, "ms_median": round(med, 3),
                      "ms_min": round(lo, 3), "ms_max": round(hi, 3), "GBps": round(nbytes / med / 1e6, 2), **kw}), flush=True)




def host_mode():
    """tyche_compress_host / tyche_decompress_host over n pages in ordinary host memory -- the path
    the Buffer entry points take -- without and with a process-wide dictionary."""
    import ctypes
    import time

    import numpy as np

    from tyche_amd import _lib, buffer
    lib = _lib.load()
    host = codec.pagegen(n, plen, dist=0, first=0, device=dev).cpu().numpy()
    dic = codec.pagegen(1, 32768, dist=0, first=n + 5, device=dev).cpu().numpy().tobytes()
    cap = codec.compress_bound(plen)
    comp = np.zeros((n, cap), np.uint8)
    back = np.zeros((n, plen), np.uint8)
    vp, u32 = ctypes.c_void_p * n, ctypes.c_uint32 * n
    p_pages, p_comp, p_back = vp(*[host[i].ctypes.data for i in range(n)]), vp(*[comp[i].ctypes.data for i in range(n)]), \
        vp(*[back[i].ctypes.data for i in range(n)])
    l_page, l_cap, res = u32(*([plen] * n)), u32(*([cap] * n)), (ctypes.c_int32 * n)()

    def wall(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    def both(tag, **kw):
        ms = wall(lambda: _lib.check(lib.tyche_compress_host(1, 1, n, p_pages, l_page, p_comp, l_cap, res), "compress"))
        lens = list(res)
        row(f"host compress, {tag}", ms, total, ratio=round(total / sum(lens), 4), **kw)
        l_comp = u32(*lens)
        enc = ms[0]
        ms = wall(lambda: _lib.check(lib.tyche_decompress_host(1, n, p_comp, l_comp, p_back, l_page, res), "decompress"))
        assert list(res) == [plen] * n and np.array_equal(back, host)
        row(f"host decompress, {tag}", ms, total, **kw)
        return enc, ms[0]

    total = n * plen
    pe, pd = both("no dictionary")
    for D in (4096, 16384):
        d = codec.Lz4Dict(dic[:D])
        buffer.use_dict(d)
        e, dd = both(f"process-wide dictionary D={D}")
        print(json.dumps({"what": f"D={D} against no dictionary", "compress_times": round(e / pe, 2),
                          "decompress_times": round(dd / pd, 2)}), flush=True)
        buffer.use_dict(None)
        d.close()


if os.environ.get("HOST"):
    host_mode()
    sys.exit(0)

pages = codec.pagegen(n, plen, dist=0, first=0, device=dev)
dict_src = codec.pagegen(1, 32768, dist=0, first=n + 5, device=dev).cpu().numpy().tobytes()
slot = codec.slot_size(plen)
comp = torch.empty((n, slot), dtype=torch.uint8, device=dev)
clen = torch.empty((n,), dtype=torch.int32, device=dev)
out = torch.empty((n, plen), dtype=torch.uint8, device=dev)
rv = torch.empty((n,), dtype=torch.int32, device=dev)
total = n * plen

ms = timed(lambda: codec.compress_pages(pages, out=comp, out_len=clen))
plain_bytes = int(clen.sum())
row("plain encode", ms, total, ratio=round(total / plain_bytes, 4))
plain_enc = ms[0]
ms = timed(lambda: codec.decompress_pages(comp, clen, plen, out=out, rv=rv))
assert bool((rv == plen).all()) and torch.equal(out, pages)
row("plain decode", ms, total)
plain_dec = ms[0]

for D in (4096, 16384):
    d = codec.Lz4Dict(dict_src[:D])
    ms = timed(lambda: codec.compress_pages(pages, out=comp, out_len=clen, dictionary=d))
    dict_bytes = int(clen.sum())
    row(f"dictionary encode D={D}", ms, total, ratio=round(total / dict_bytes, 4), times_plain=round(ms[0] / plain_enc, 2),
        ratio_gain_pct=round(100.0 * (plain_bytes / dict_bytes - 1.0), 2))
    ms = timed(lambda: codec.decompress_pages(comp, clen, plen, out=out, rv=rv, dictionary=d))
    assert bool((rv == plen).all()) and torch.equal(out, pages)
    row(f"dictionary decode D={D}", ms, total, times_plain=round(ms[0] / plain_dec, 2))
    if os.environ.get("SCALE") and D == 4096:
        k = 64
        while k <= n:
            ms = timed(lambda: codec.decompress_pages(comp[:k], clen[:k], plen, out=out[:k], rv=rv[:k], dictionary=d))
            row(f"dictionary decode D={D}", ms, k * plen, pages=k)
            k *= 4
    d.close()
