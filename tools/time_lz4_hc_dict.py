"""Times the high-compression LZ4 dictionary encoder (LZ4_HC_DICT=1) beside the default dictionary
encoder and plain LZ4_HC=1 in one run: device-resident batches of PAGES dist-0 pages, HIP events
around each call, warm, the median of REPS.  Configurations (page length, dictionary length):
4 KiB / 4 KiB, 16 KiB / 4 KiB, 16 KiB / 16 KiB; the dictionary is one more page of the
distribution, cut.  Per configuration: the default dictionary encoder, plain LZ4_HC=1 without a
dictionary, the new mode, and the dictionary decoder on the default dictionary streams and on the
new ones; then liblz4's HC dictionary mode at level 3 (LZ4_loadDictHC + LZ4_compress_HC_continue,
a stream per thread, the dictionary loaded afresh for every page) on 16 host threads, where
liblz4.so.1 loads.

    PAGES=65536 python tools/time_lz4_hc_dict.py
    TYCHE_LZ4_HC_DICT_PAGES_PER_CU=k ...     # the new encoder's resident pages per CU held to k
"""
import concurrent.futures as cf
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tyche_amd import _lib, codec  # noqa: E402

n = int(os.environ.get("PAGES", "65536"))
reps = int(os.environ.get("REPS", "7"))
dev = torch.device("cuda:0")
CONFIGS = ((4096, 4096), (16384, 4096), (16384, 16384))


def timed(fn):
    fn()
    fn()                                   # warm: code object loaded, pools and counters allocated, seed uploaded
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


def row(name, plen, D, ms, nbytes, **kw):
    med, lo, hi = ms
    print(json.dumps({"what": name, "pages": kw.pop("pages", n), "page_len": plen, "dict_len": D, "ms_median": round(med, 3),
                      "ms_min": round(lo, 3), "ms_max": round(hi, 3), "GBps": round(nbytes / med / 1e6, 2), **kw}), flush=True)


def host_hc_dict(pages, plen, dic):
    try:
        lz4 = ctypes.CDLL("liblz4.so.1")
    except OSError as e:
        print(json.dumps({"what": "liblz4 HC dictionary mode level 3", "skipped": str(e)}), flush=True)
        return
    lz4.LZ4_createStreamHC.restype = ctypes.c_void_p
    lz4.LZ4_freeStreamHC.argtypes = [ctypes.c_void_p]
    lz4.LZ4_resetStreamHC_fast.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lz4.LZ4_resetStreamHC_fast.restype = None
    lz4.LZ4_loadDictHC.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    lz4.LZ4_compress_HC_continue.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    k = min(n, 8192)
    host = pages[:k].cpu().numpy()
    cap = plen + plen // 255 + 16
    threads = 16

    def work(t):
        dst = ctypes.create_string_buffer(cap)
        st = lz4.LZ4_createStreamHC()
        got = 0
        for i in range(t, k, threads):
            lz4.LZ4_resetStreamHC_fast(st, 3)
            lz4.LZ4_loadDictHC(st, dic, len(dic))
            got += lz4.LZ4_compress_HC_continue(st, host[i].ctypes.data, dst, plen, cap)
        lz4.LZ4_freeStreamHC(st)
        return got

    with cf.ThreadPoolExecutor(threads) as ex:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            nbytes = sum(ex.map(work, range(threads)))
            ts.append((time.perf_counter() - t0) * 1e3)
    ms = (statistics.median(ts), min(ts), max(ts))
    row("liblz4 LZ4_loadDictHC + LZ4_compress_HC_continue level 3, 16 host threads", plen, len(dic), ms, k * plen, pages=k,
        ratio=round(k * plen / nbytes, 4), ms_per_64k_pages=round(ms[0] * 65536 / k, 1))


for plen, D in CONFIGS:
    total = n * plen
    pages = codec.pagegen(n, plen, dist=0, first=0, device=dev)
    dic = codec.pagegen(1, 32768, dist=0, first=n + 5, device=dev).cpu().numpy().tobytes()[:D]
    slot = codec.slot_size(plen)
    comp = torch.empty((n, slot), dtype=torch.uint8, device=dev)
    clen = torch.empty((n,), dtype=torch.int32, device=dev)
    out = torch.empty((n, plen), dtype=torch.uint8, device=dev)
    rv = torch.empty((n,), dtype=torch.int32, device=dev)
    d = codec.Lz4Dict(dic)

    def encode(name, dictionary, **kw):
        ms = timed(lambda: codec.compress_pages(pages, out=comp, out_len=clen, dictionary=dictionary))
        nbytes = int(clen.sum())
        row(name, plen, D if dictionary is not None else 0, ms, total, ratio=round(total / nbytes, 4), **kw)
        return ms[0], nbytes

    def decode(name):
        ms = timed(lambda: codec.decompress_pages(comp, clen, plen, out=out, rv=rv, dictionary=d))
        assert bool((rv == plen).all()) and torch.equal(out, pages)
        row(name, plen, D, ms, total)
        return ms[0]

    dict_enc, dict_bytes = encode("default dictionary encode", d)
    dict_dec = decode("dictionary decode of default dictionary streams")
    _lib.set_knob("LZ4_HC", 1)
    hc_enc, hc_bytes = encode("plain LZ4_HC=1 encode, no dictionary", None)
    _lib.clear_knob("LZ4_HC")
    _lib.set_knob("LZ4_HC_DICT", 1)
    new_enc, new_bytes = encode("LZ4_HC_DICT=1 encode", d, pages_per_cu=os.environ.get("TYCHE_LZ4_HC_DICT_PAGES_PER_CU", "all that fit"))
    _lib.clear_knob("LZ4_HC_DICT")
    new_dec = decode("dictionary decode of LZ4_HC_DICT=1 streams")
    print(json.dumps({"what": "LZ4_HC_DICT=1 against the default dictionary encoder and plain LZ4_HC=1", "page_len": plen, "dict_len": D,
                      "encode_times_default_dict": round(new_enc / dict_enc, 2), "encode_times_plain_hc": round(new_enc / hc_enc, 2),
                      "fewer_bytes_pct_default_dict": round(100.0 * (1.0 - new_bytes / dict_bytes), 2),
                      "fewer_bytes_pct_plain_hc": round(100.0 * (1.0 - new_bytes / hc_bytes), 2),
                      "decode_times": round(new_dec / dict_dec, 3)}), flush=True)
    host_hc_dict(pages, plen, dic)
    d.close()
    del pages, comp, clen, out, rv
