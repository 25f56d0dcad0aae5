"""Times the high-compression zlib encoder (ZLIB_HC=1) beside the default encoder in one run:
device-resident batches of PAGES x PLEN dist-0 pages, HIP events around each call, warm, the median
of REPS; then the decoders (the default one, and the one-wave decoder under ZLIB_PAR=0) on the default
streams and on the HC streams.

    PAGES=65536 PLEN=16384 python tools/time_zlib_hc.py
    PARENT_LIB=path/to/libtyche_codec.so ...   # also the default encoder of that library (the parent
                                               # commit's build), in a child process of its own
    REF_CPU=1 ...                              # also the reference's compress2 level 6 on 16 host
                                               # threads over 8,192 pages, where oracle/_ref is built
    ONLY_HC=1 TYCHE_CODEC_LIB=... [TYCHE_ZLIB_HC_PAGES_PER_CU=k] ...   # the HC encoder alone (geometry A/B of variant builds)
"""
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tyche_amd import _lib, codec  # noqa: E402

ZLIB = _lib.COMPRESSOR_IDS["zlib"]
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


def row(name, ms, nbytes, **kw):
    med, lo, hi = ms
    print(json.dumps({"what": name, "lib": os.path.basename(_lib.LIB_PATH), "pages": kw.pop("pages", n), "page_len": plen,
                      "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                      "GBps": round(nbytes / med / 1e6, 2), **kw}), flush=True)


pages = codec.pagegen(n, plen, dist=0, first=0, device=dev)
slot = codec.slot_size(plen, ZLIB)
comp = torch.empty((n, slot), dtype=torch.uint8, device=dev)
clen = torch.empty((n,), dtype=torch.int32, device=dev)
out = torch.empty((n, plen), dtype=torch.uint8, device=dev)
rv = torch.empty((n,), dtype=torch.int32, device=dev)


def encode(name, **kw):
    ms = timed(lambda: codec.compress_pages(pages, compressor_id=ZLIB, out=comp, out_len=clen))
    nbytes = int(clen.sum())
    row(name, ms, total, ratio=round(total / nbytes, 4), **kw)
    return ms[0], nbytes


def decode(name, **kw):
    ms = timed(lambda: codec.decompress_pages(comp, clen, plen, compressor_id=ZLIB, out=out, rv=rv))
    assert bool((rv == plen).all()) and torch.equal(out, pages)
    row(name, ms, total, **kw)
    return ms[0]


def decode_both(what):
    split = decode(f"decode of {what} streams, parallel decoder (default)")
    _lib.set_knob("ZLIB_PAR", 0)
    try:
        one = decode(f"decode of {what} streams, one-wave decoder (ZLIB_PAR=0)")
    finally:
        _lib.clear_knob("ZLIB_PAR")
    return one, split


if os.environ.get("ONLY_HC"):
    _lib.set_knob("ZLIB_HC", 1)
    encode("ZLIB_HC=1 encode", pages_per_cu=os.environ.get("TYCHE_ZLIB_HC_PAGES_PER_CU", "all that fit"))
    sys.exit(0)
plain_enc, plain_bytes = encode("default encode")
if os.environ.get("ONLY_DEFAULT"):
    sys.exit(0)
plain_dec = decode_both("default")
_lib.set_knob("ZLIB_HC", 1)
hc_enc, hc_bytes = encode("ZLIB_HC=1 encode")
_lib.clear_knob("ZLIB_HC")
print(json.dumps({"what": "ZLIB_HC=1 against default", "page_len": plen, "encode_times": round(hc_enc / plain_enc, 2),
                  "fewer_bytes_pct": round(100.0 * (1.0 - hc_bytes / plain_bytes), 2)}), flush=True)
hc_dec = decode_both("ZLIB_HC=1")
print(json.dumps({"what": "decode of HC streams against default streams", "page_len": plen,
                  "one_wave_decoder_times": round(hc_dec[0] / plain_dec[0], 3),
                  "parallel_decoder_times": round(hc_dec[1] / plain_dec[1], 3)}), flush=True)

if os.environ.get("PARENT_LIB"):
    env = dict(os.environ, TYCHE_CODEC_LIB=os.environ["PARENT_LIB"], ONLY_DEFAULT="1")
    env.pop("PARENT_LIB")
    subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, check=True, timeout=300)

if os.environ.get("REF_CPU"):
    import concurrent.futures as cf
    import ctypes
    import time
    ref = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libtyche_ref.so")
    try:
        z = ctypes.CDLL(ref)
    except OSError as e:
        print(json.dumps({"what": "reference compress2 level 6", "skipped": str(e)}), flush=True)
        sys.exit(0)
    z.compress2.restype = ctypes.c_int
    z.compress2.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulong), ctypes.c_void_p, ctypes.c_ulong, ctypes.c_int]
    z.compressBound.restype = ctypes.c_ulong
    z.compressBound.argtypes = [ctypes.c_ulong]
    k = min(n, 8192)
    host = pages[:k].cpu().numpy()
    cap = int(z.compressBound(plen))
    threads = 16

    def work(t):
        dst = ctypes.create_string_buffer(cap)
        total_out = 0
        for i in range(t, k, threads):
            dl = ctypes.c_ulong(cap)
            assert z.compress2(dst, ctypes.byref(dl), host[i].ctypes.data, plen, 6) == 0
            total_out += dl.value
        return total_out

    with cf.ThreadPoolExecutor(threads) as ex:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            nbytes = sum(ex.map(work, range(threads)))
            ts.append((time.perf_counter() - t0) * 1e3)
    ms = (statistics.median(ts), min(ts), max(ts))
    row("reference compress2 level 6, 16 host threads", ms, k * plen, pages=k, ratio=round(k * plen / nbytes, 4),
        ms_scaled_to_the_batch=round(ms[0] * n / k, 1), hc_encode_times_faster=round(ms[0] * n / k / hc_enc, 2))
