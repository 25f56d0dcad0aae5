"""Diagnostic: the LZ4 decoder's page walks against each other and against another build of the
library, on the same compressed pages in one process, every variant in turn within every repetition.

    PARENT_LIB=tyche_amd/libtyche_codec_parent.so PAGES=1048576 PLEN=16384 REPS=7 python tools/time_lz4_order.py

HIP events around the whole decompress call (the ordering pass is inside).  The variants: the
parent library, this tree's stride walk (LZ4_LC_ORDER=0), and the ordered walk over the whole batch
and over the windows in WINDOWS.  The encoders of both libraries are timed too.  Prints one line per
variant: fastest, median and slowest repetition in ms.
"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tyche_amd import _lib, codec  # noqa: E402


def main():
    n = int(os.environ.get("PAGES", str(1 << 20)))
    plen = int(os.environ.get("PLEN", "16384"))
    reps = int(os.environ.get("REPS", "7"))
    windows = [int(w) for w in os.environ.get("WINDOWS", "0,65536,16384,4096").split(",")]
    parent_path = os.environ.get("PARENT_LIB", "")
    dev = torch.device("cuda:0")
    pages = codec.pagegen(n, plen, dist=int(os.environ.get("DIST", "0")), device=dev)
    comp, clen = codec.compress_pages(pages)
    torch.cuda.synchronize()
    mx = int(clen.max())
    out = torch.empty((n, plen), dtype=torch.uint8, device=dev)
    rv = torch.empty((n,), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    dbatch = _lib.Batch(count=n, src=comp.data_ptr(), src_lengths=clen.data_ptr(), src_stride=comp.shape[1],
                        max_src_length=min(mx, comp.shape[1]), dst=out.data_ptr(), dst_stride=plen, dst_capacity=plen,
                        results=rv.data_ptr())
    comp2, clen2 = torch.empty_like(comp), torch.empty_like(clen)
    cbatch = _lib.Batch(count=n, src=pages.data_ptr(), src_stride=plen, src_length=plen, max_src_length=plen,
                        dst=comp2.data_ptr(), dst_stride=comp2.shape[1], dst_capacity=comp2.shape[1], results=clen2.data_ptr())
    branch = _lib.load()
    libs = {"branch": branch}
    if parent_path:
        parent = ctypes.CDLL(os.path.abspath(parent_path))
        for name in ("tyche_decompress_batch", "tyche_compress_batch"):
            getattr(parent, name).restype = ctypes.c_int
        parent.tyche_decompress_batch.argtypes = [ctypes.c_int, ctypes.POINTER(_lib.Batch), ctypes.c_void_p]
        parent.tyche_compress_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(_lib.Batch), ctypes.c_void_p]
        libs["parent"] = parent

    def knobs(order, window):
        _lib.set_knob("LZ4_LC_ORDER", order)
        _lib.set_knob("LZ4_LC_ORDER_WINDOW", window)

    variants = ([("parent", "parent", None)] if parent_path else []) + [("branch stride", "branch", (0, 0))] + \
        [("branch ordered, " + ("whole batch" if w == 0 else f"window {w}"), "branch", (1, w)) for w in windows]

    def decode(lib, kn):
        if kn is not None:
            knobs(*kn)
        r = libs[lib].tyche_decompress_batch(1, ctypes.byref(dbatch), stream)
        assert r == 0, r

    def encode(lib):
        r = libs[lib].tyche_compress_batch(1, 1, ctypes.byref(cbatch), stream)
        assert r == 0, r

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for name, lib, kn in variants:   # every variant restores every page (and is warm afterwards)
        out.fill_(0xAB)
        rv.fill_(0x5A5A5A5A)
        decode(lib, kn)
        torch.cuda.synchronize()
        assert bool((rv == plen).all()) and torch.equal(out, pages), name
    for lib in libs:
        encode(lib)
        torch.cuda.synchronize()
        assert torch.equal(clen2, clen), lib
    times = {name: [] for name, _, _ in variants}
    etimes = {lib: [] for lib in libs}
    for _ in range(reps):
        for name, lib, kn in variants:
            times[name].append(timed(lambda: decode(lib, kn)))
        for lib in libs:
            etimes[lib].append(timed(lambda: encode(lib)))
    print(f"pages {n} x {plen} B, max stream {mx}, {reps} repetitions, ms per call: fastest / median / slowest")
    for name, _, _ in variants:
        t = times[name]
        print(f"  decode  {name:34s} {min(t):8.3f} / {statistics.median(t):8.3f} / {max(t):8.3f}")
    for lib in libs:
        t = etimes[lib]
        print(f"  encode  {lib:34s} {min(t):8.3f} / {statistics.median(t):8.3f} / {max(t):8.3f}")


if __name__ == "__main__":
    main()
