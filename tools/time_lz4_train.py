#!/usr/bin/env python3
"""Times the LZ4 dictionary trainer (tyche_lz4_dict_train_batch) on device-resident dist-0 pages
of 16 KiB: 64, 1,024 and 4,096 pages at D = 4 KiB and 32 KiB.  Per case: one warm call, then 7
timed with device events around the call (which waits for its stream itself); the median is
reported.  Beside it, the host emulator's time for the same call on one core
(tools/lz4_train_emul.cpp, -O2): the only other implementation of this algorithm -- there is no
reference trainer -- and a check that both give the same bytes.

    python tools/time_lz4_train.py [--out profiles/lz4_train_time.log]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tyche_amd import _lib, codec   # noqa: E402

EMUL_SRC = os.path.join(ROOT, "tools", "lz4_train_emul.cpp")
EMUL_LIB = os.path.join(ROOT, "tools", "bin", "liblz4trainemul.so")
PAGE = 16384


def load_emul():
    if not os.path.exists(EMUL_LIB):
        os.makedirs(os.path.dirname(EMUL_LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", EMUL_LIB, EMUL_SRC])
    lib = ctypes.CDLL(EMUL_LIB)
    lib.lz4_train_emul.restype = ctypes.c_int
    lib.lz4_train_emul.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                   ctypes.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pages", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("--dicts", type=int, nargs="*", default=[4096, 32768])
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    emul = load_emul()
    if a.out:
        open(a.out, "w").close()
    for n in a.pages:
        pages = codec.pagegen(n, PAGE, seed=4242, first=200000, dist=0, device=dev)
        torch.cuda.synchronize()
        host = pages.cpu().numpy()
        offs = (np.arange(n, dtype=np.uint64) * PAGE)
        lens = np.full(n, PAGE, np.uint32)
        for D in a.dicts:
            b = _lib.Batch(count=n, src=pages.data_ptr(), src_stride=PAGE, src_length=PAGE)
            stream = torch.cuda.current_stream(dev).cuda_stream
            times, got = [], None
            for rep in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                h = lib.tyche_lz4_dict_train_batch(ctypes.byref(b), D, stream)
                e1.record()
                e1.synchronize()
                assert h, _lib.last_error()
                if rep:
                    times.append(e0.elapsed_time(e1))
                k = lib.tyche_lz4_dict_length(h)
                out = ctypes.create_string_buffer(k)
                lib.tyche_lz4_dict_bytes(h, out, k)
                got = out.raw[:k]
                lib.tyche_lz4_dict_destroy(h)
            eout = np.zeros(D, np.uint8)
            t0 = time.perf_counter()
            r = emul.lz4_train_emul(host.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, D, eout.ctypes.data)
            t_emul = (time.perf_counter() - t0) * 1e3
            same = eout[:max(r, 0)].tobytes() == got
            line = (f"pages {n} x {PAGE} B, D {D}: device median {statistics.median(times):.3f} ms (min {min(times):.3f}, "
                    f"max {max(times):.3f}, {a.reps} runs after 1 warm), emulator on one core {t_emul:.1f} ms, "
                    f"dictionary {len(got)} B, bytes equal: {same}")
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
