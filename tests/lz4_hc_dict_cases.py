"""Inputs and checks shared by the tests of the high-compression LZ4 dictionary encoder
(LZ4_HC_DICT=1; test_lz4_hc_dict_emul.py on the CPU through the emulator
tools/lz4_hc_dict_emul.cpp, test_gpu_lz4_hc_dict.py on the kernel
tyche_amd/csrc/lz4_encode_hc_dict.hip): the emulator's loader, the walker that holds a stream to
the block format, the end rules and the dictionary's reach, a plain Python dictionary decode, the
case lists and the ratio targets.  The mode promises a valid dictionary block, not particular
bytes, so the expected bytes of a GPU test are the emulator's."""
import ctypes
import json
import os
import subprocess

import numpy as np

import lz4_dict_cases as DC
from lz4_hc_cases import FILL, GUARD, lz4_bound
from lz4_large_cases import walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "bin", "liblz4hcdictemul.so")
SRC = os.path.join(ROOT, "tools", "lz4_hc_dict_emul.cpp")
CORES = [os.path.join(ROOT, "tyche_amd", "csrc", f) for f in ("lz4_hc_core.h", "lz4_exact_core.h")]
TARGETS = os.path.join(ROOT, "tests", "golden", "lz4_hc_dict_targets.json")

# the CPU test's matrix: lz4_dict_cases.all_cases restricted to these, and the two limit pairs
DS = (1, 63, 64, 65, 1000, 4096, 32768)
LS = (0, 1, 12, 13, 64, 65, 4095, 16384, 32768)
LIMIT_PAIRS = [(32768, 32768), (64, 65472)]
PAIRS = [(d, l) for d in DS for l in LS if d + l <= DC.WINDOW] + [p for p in LIMIT_PAIRS if p[1] not in LS or p[0] not in DS]
# the GPU test's pairs: the last two put a 16-bit position at 65,535
GPU_PAIRS = [(4096, 4096), (1000, 4095), (65, 13), (63, 4096), (16384, 16384), (32768, 32768), (64, 65472)]
RATIO_PLEN, RATIO_DICT = 4096, 4096


def load_emul():
    """enc(dictionary, page, cap) -> (return value, the bytes it covers); builds the emulator when it
    is missing or older than its sources, and asserts that nothing at or past cap was written."""
    if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in [SRC] + CORES):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.lz4hc_dict_emul_compress.restype = ctypes.c_int
    lib.lz4hc_dict_emul_compress.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    record = os.environ.get("LZ4_HC_DICT_EMUL_RECORD")   # the calls, for the sanitizer replay (tools/lz4_hc_dict_emul.cpp)

    def enc(dic: bytes, page: bytes, cap=None):
        cap = lz4_bound(len(page)) if cap is None else cap
        d = np.frombuffer(dic, np.uint8).copy() if dic else np.zeros(1, np.uint8)
        s = np.frombuffer(page, np.uint8).copy() if page else np.zeros(1, np.uint8)
        dst = np.full(cap + GUARD + 15, FILL, np.uint8)
        shift = (len(page) + cap) % 16                # every destination alignment over a test's calls
        a = (-dst.ctypes.data) % 16 + shift
        r = lib.lz4hc_dict_emul_compress(d.ctypes.data, len(dic), s.ctypes.data, len(page), dst.ctypes.data + a, cap)
        assert bool((dst[:a] == FILL).all()) and bool((dst[a + cap:] == FILL).all()), ("wrote outside the capacity", len(dic), len(page), cap)
        if record:
            with open(record, "ab") as f:
                f.write(np.array([len(dic), len(page), cap, r & 0xFFFFFFFF, shift], np.uint32).tobytes() + dic + page)
        return r, dst[a:a + max(r, 0)].tobytes()
    enc.lib = lib
    return enc


def seen(D: int) -> int:
    """The bytes of a dictionary of D that the encoders see: its last D & ~63."""
    return D & ~63


def check_stream(stream: bytes, dic: bytes, page: bytes):
    """The block's own rules with a dictionary in front: it is no longer than the bound, decodes to
    the page with every offset in 1 .. position + D' (the dictionary bytes the encoder sees), its
    last match starts at or before n - 12, and its last 5 bytes are literals.  Returns how far the
    offsets reach in front of the page (0: not at all)."""
    n, tail = len(page), dic[len(dic) - seen(len(dic)):]
    assert 0 < len(stream) <= lz4_bound(n), (n, len(stream))
    out = bytearray(tail)
    base, reach = len(tail), 0
    seqs = walk(stream)
    assert seqs and seqs[-1][2] is None, "the block does not end in a literal-only sequence"
    for tp, ll, op in seqs:
        lit_end = op if op is not None else len(stream)
        out += stream[lit_end - ll:lit_end]
        if op is None:
            assert lit_end == len(stream)
            assert ll >= min(n, 5) and (len(seqs) == 1 or ll >= 5), ("last literals", n, ll)
            break
        off = stream[op] | (stream[op + 1] << 8)
        assert 1 <= off <= len(out), ("offset", off, len(out) - base, base)
        reach = max(reach, off - (len(out) - base))
        ml, ip = (stream[tp] & 15), op + 2
        if ml == 15:
            while True:
                s = stream[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        ml += 4
        assert len(out) - base <= n - 12, ("a match starts after n - 12", len(out) - base, n)
        for _ in range(ml):
            out.append(out[-off])
        assert len(out) - base <= n - 5, ("a match ends in the last 5 bytes", len(out) - base, n)
    assert bytes(out[base:]) == page, n
    return reach


def py_decode(dic: bytes, stream: bytes, n: int) -> bytes:
    """A plain dictionary decode: the whole dictionary in front of the output."""
    out = bytearray(dic)
    ip = 0
    while ip < len(stream):
        t = stream[ip]
        ip += 1
        ll = t >> 4
        if ll == 15:
            while True:
                s = stream[ip]
                ip += 1
                ll += s
                if s != 255:
                    break
        out += stream[ip:ip + ll]
        ip += ll
        if ip >= len(stream):
            break
        off = stream[ip] | (stream[ip + 1] << 8)
        ip += 2
        ml = t & 15
        if ml == 15:
            while True:
                s = stream[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        assert 1 <= off <= len(out)
        for _ in range(ml + 4):
            out.append(out[-off])
    assert len(out) == len(dic) + n
    return bytes(out[len(dic):])


def restores(ref, dic: bytes, stream: bytes, page: bytes) -> bool:
    """Through the reference's LZ4_decompress_safe_usingDict where it is built, else the plain decode."""
    if ref is not None:
        return ref.decompress(dic, stream, len(page)) == (len(page), page)
    return py_decode(dic, stream, len(page)) == page


def cases(O, pairs=None, kinds=DC.KINDS):
    return DC.all_cases(O, PAIRS if pairs is None else pairs, kinds)


def ratio_inputs(O, dist: int):
    """(dictionary, 48 pages of 4 KiB): lz4_dict_cases.ratio_inputs at n = 4096, one more page's 4 KiB as dictionary."""
    return DC.ratio_inputs(O, RATIO_PLEN, dist, RATIO_DICT)


def targets():
    """liblz4's totals over ratio_inputs, recorded by tools/gen_lz4_hc_dict_golden.py: F of its fast
    dictionary mode, H of its HC dictionary mode at level 3, per distribution."""
    with open(TARGETS) as f:
        t = json.load(f)
    assert t["pages"] == DC.RATIO_PAGES and t["page_len"] == RATIO_PLEN and t["dict_len"] == RATIO_DICT and t["level"] == 3
    return t
