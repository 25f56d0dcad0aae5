"""Times the zstd shared-dictionary kernels beside the plain ones in one run: device-resident batches
of PAGES x PLEN dist-0 pages, dictionaries of 4 KiB and 16 KiB (one more page of the distribution,
cut), HIP events around each call, warm, the median of REPS:

    PAGES=65536 PLEN=16384 python tools/time_zstd_dict.py
    BASELINE=1 ... python tools/time_zstd_dict.py   # the plain zstd rows only: run from a checkout of the
                                                    # parent commit for the baseline the dictionary rows are held against
    REF=1 ... python tools/time_zstd_dict.py        # also the acceptance bar: the reference's ZSTD_compress_usingDict /
                                                    # ZSTD_decompress_usingDict (oracle/_ref, level 1) over the same pages
                                                    # on THREADS (16) host threads, ctypes calls (which release the GIL)
    SCALE=1 ... python tools/time_zstd_dict.py      # also the dictionary decoder at 64 .. PAGES pages (it is one kernel
                                                    # for every batch size) beside the plain decoder at the same counts
    HOST=1 PAGES=16384 python tools/time_zstd_dict.py   # instead: the host batch calls (pageable host memory in and
                                                        # out, wall clock), plain and with a process-wide dictionary
"""
import json
import os
import statistics
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tyche_amd import _lib, codec  # noqa: E402

ZSTD = _lib.ZSTD_COMPRESSOR_ID
n = int(os.environ.get("PAGES", "65536"))
plen = int(os.environ.get("PLEN", "16384"))
reps = int(os.environ.get("REPS", "7"))
dev = torch.device("cuda:0")
total = n * plen


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


def wall(fn):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def row(name, ms, nbytes, **kw):
    med, lo, hi = ms
    print(json.dumps({"what": name, "pages": kw.pop("pages", n), "page_len": plen, "ms_median": round(med, 3),
                      "ms_min": round(lo, 3), "ms_max": round(hi, 3), "GBps": round(nbytes / med / 1e6, 2), **kw}), flush=True)


def host_mode():
    """tyche_compress_host / tyche_decompress_host over n pages in ordinary host memory -- the path the
    Buffer entry points take -- without and with a process-wide zstd dictionary."""
    import ctypes

    import numpy as np
    lib = _lib.load()
    host = codec.pagegen(n, plen, dist=0, first=0, device=dev).cpu().numpy()
    dic = codec.pagegen(1, 32768, dist=0, first=n + 5, device=dev).cpu().numpy().tobytes()
    cap = codec.compress_bound(plen, ZSTD)
    comp = np.zeros((n, cap), np.uint8)
    back = np.zeros((n, plen), np.uint8)
    vp, u32 = ctypes.c_void_p * n, ctypes.c_uint32 * n
    p_pages, p_comp, p_back = vp(*[host[i].ctypes.data for i in range(n)]), vp(*[comp[i].ctypes.data for i in range(n)]), \
        vp(*[back[i].ctypes.data for i in range(n)])
    l_page, l_cap, res = u32(*([plen] * n)), u32(*([cap] * n)), (ctypes.c_int32 * n)()

    def both(tag, **kw):
        ms = wall(lambda: _lib.check(lib.tyche_compress_host(ZSTD, 1, n, p_pages, l_page, p_comp, l_cap, res), "compress"))
        lens = list(res)
        row(f"host compress, {tag}", ms, total, ratio=round(total / sum(lens), 4), **kw)
        l_comp = u32(*lens)
        enc = ms[0]
        ms = wall(lambda: _lib.check(lib.tyche_decompress_host(ZSTD, n, p_comp, l_comp, p_back, l_page, res), "decompress"))
        assert list(res) == [plen] * n and np.array_equal(back, host)
        row(f"host decompress, {tag}", ms, total, **kw)
        return enc, ms[0]

    pe, pd = both("no dictionary")
    for D in (4096, 16384):
        d = codec.Dictionary(dic[:D])
        codec.use_zstd_dict(d)
        e, dd = both(f"process-wide dictionary D={D}")
        print(json.dumps({"what": f"D={D} against no dictionary", "compress_times": round(e / pe, 2),
                          "decompress_times": round(dd / pd, 2)}), flush=True)
        codec.use_zstd_dict(None)
        d.close()


def reference_rows(host, dic, D):
    """The reference on `threads` host threads: every thread its own contexts and a contiguous share
    of the pages; one ctypes call per page, addresses precomputed."""
    import ctypes

    import numpy as np
    threads = int(os.environ.get("THREADS", "16"))
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libtyche_ref.so"))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.ZSTD_createCCtx.restype = vp
    L.ZSTD_createDCtx.restype = vp
    L.ZSTD_compress_usingDict.argtypes = [vp, vp, sz, vp, sz, vp, sz, ctypes.c_int]
    L.ZSTD_compress_usingDict.restype = sz
    L.ZSTD_decompress_usingDict.argtypes = [vp, vp, sz, vp, sz, vp, sz]
    L.ZSTD_decompress_usingDict.restype = sz
    cap = plen + (plen >> 7) + 524
    comp = np.zeros((n, cap), np.uint8)
    back = np.zeros((n, plen), np.uint8)
    dbuf = np.frombuffer(dic[:D], np.uint8).copy()
    src0, comp0, back0, daddr = host.ctypes.data, comp.ctypes.data, back.ctypes.data, dbuf.ctypes.data
    lens = [0] * n
    cuts = [n * t // threads for t in range(threads + 1)]
    ctxs = [(L.ZSTD_createCCtx(), L.ZSTD_createDCtx()) for _ in range(threads)]

    def run(work):
        ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()

    def enc(t):
        c = ctxs[t][0]
        f = L.ZSTD_compress_usingDict
        for i in range(cuts[t], cuts[t + 1]):
            lens[i] = f(c, comp0 + i * cap, cap, src0 + i * plen, plen, daddr, D, 1)

    def dec(t):
        c = ctxs[t][1]
        f = L.ZSTD_decompress_usingDict
        for i in range(cuts[t], cuts[t + 1]):
            f(c, back0 + i * plen, plen, comp0 + i * cap, lens[i], daddr, D)

    ms = wall(lambda: run(enc))
    assert max(lens) <= cap
    row(f"reference ZSTD_compress_usingDict level 1, {threads} host threads, D={D}", ms, total,
        ratio=round(total / sum(lens), 4))
    e = ms[0]
    ms = wall(lambda: run(dec))
    assert np.array_equal(back, host)
    row(f"reference ZSTD_decompress_usingDict, {threads} host threads, D={D}", ms, total)
    return e, ms[0]


if os.environ.get("HOST"):
    host_mode()
    sys.exit(0)

pages = codec.pagegen(n, plen, dist=0, first=0, device=dev)
dict_src = codec.pagegen(1, 32768, dist=0, first=n + 5, device=dev).cpu().numpy().tobytes()
slot = codec.slot_size(plen, ZSTD)
comp = torch.empty((n, slot), dtype=torch.uint8, device=dev)
clen = torch.empty((n,), dtype=torch.int32, device=dev)
out = torch.empty((n, plen), dtype=torch.uint8, device=dev)
rv = torch.empty((n,), dtype=torch.int32, device=dev)
lib_name = os.path.relpath(_lib.LIB_PATH, os.getcwd())

ms = timed(lambda: codec.compress_pages(pages, ZSTD, out=comp, out_len=clen))
plain_bytes = int(clen.sum())
row("plain encode", ms, total, ratio=round(total / plain_bytes, 4), lib=lib_name)
plain_enc = ms[0]
ms = timed(lambda: codec.decompress_pages(comp, clen, plen, ZSTD, out=out, rv=rv))
assert bool((rv == plen).all()) and torch.equal(out, pages)
row("plain decode", ms, total, lib=lib_name)
plain_dec = ms[0]
# the same with the longest stream declared (max_comp_len) instead of the slot width: the decoders size
# their LDS by the declared maximum, and the one-wave kernels' residency follows it
mx = int(clen.max())
ms = timed(lambda: codec.decompress_pages(comp, clen, plen, ZSTD, out=out, rv=rv, max_comp_len=mx))
assert bool((rv == plen).all()) and torch.equal(out, pages)
row("plain decode, longest stream declared", ms, total, max_comp_len=mx, lib=lib_name)
if os.environ.get("SCALE"):
    k = 64
    while k <= n:
        ms = timed(lambda: codec.decompress_pages(comp[:k], clen[:k], plen, ZSTD, out=out[:k], rv=rv[:k]))
        row("plain decode", ms, k * plen, pages=k, lib=lib_name)
        k *= 4
if os.environ.get("BASELINE"):
    sys.exit(0)
# the baseline the dictionary rows are held against: the parent commit's plain rows (BASELINE=1 run of
# its library, "ms" passed in), else this library's own
base_enc = float(os.environ.get("BASE_ENC_MS", plain_enc))
base_dec = float(os.environ.get("BASE_DEC_MS", plain_dec))
host_pages = pages.cpu().numpy() if os.environ.get("REF") else None

for D in (4096, 16384):
    d = codec.Dictionary(dict_src[:D])
    ms = timed(lambda: codec.compress_pages(pages, ZSTD, out=comp, out_len=clen, dictionary=d))
    dict_bytes = int(clen.sum())
    row(f"dictionary encode D={D}", ms, total, ratio=round(total / dict_bytes, 4), times_plain=round(ms[0] / base_enc, 2),
        ratio_gain_pct=round(100.0 * (plain_bytes / dict_bytes - 1.0), 2))
    dict_enc = ms[0]
    ms = timed(lambda: codec.decompress_pages(comp, clen, plen, ZSTD, out=out, rv=rv, dictionary=d))
    assert bool((rv == plen).all()) and torch.equal(out, pages)
    row(f"dictionary decode D={D}", ms, total, times_plain=round(ms[0] / base_dec, 2))
    dict_dec = ms[0]
    mx = int(clen.max())
    ms = timed(lambda: codec.decompress_pages(comp, clen, plen, ZSTD, out=out, rv=rv, dictionary=d, max_comp_len=mx))
    assert bool((rv == plen).all()) and torch.equal(out, pages)
    row(f"dictionary decode D={D}, longest stream declared", ms, total, max_comp_len=mx, times_plain=round(ms[0] / base_dec, 2))
    dict_dec_declared = ms[0]
    if os.environ.get("SCALE") and D == 4096:
        k = 64
        while k <= n:
            ms = timed(lambda: codec.decompress_pages(comp[:k], clen[:k], plen, ZSTD, out=out[:k], rv=rv[:k], dictionary=d))
            row(f"dictionary decode D={D}", ms, k * plen, pages=k)
            k *= 4
    if host_pages is not None:
        re, rd = reference_rows(host_pages, dict_src, D)
        print(json.dumps({"what": f"device against the reference's host run, D={D}", "page_len": plen,
                          "encode_speedup": round(re / dict_enc, 2), "decode_speedup": round(rd / dict_dec, 2),
                          "decode_speedup_longest_stream_declared": round(rd / dict_dec_declared, 2),
                          "device_faster_both_ways": bool(dict_enc < re and dict_dec < rd)}), flush=True)
    d.close()
