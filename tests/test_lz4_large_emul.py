"""CPU check of the large-page LZ4 kernels' algorithms (tyche_amd/csrc/lz4_large_core.h, the
per-wave code of lz4_decode_large.hip and lz4_encode_large.hip: pages of 65,536 bytes up to 4 MiB)
through their host emulator tools/lz4_large_emul.cpp, against the oracle: decoded bytes and return
values on valid, hand-made and malformed streams, encoder streams that the oracle restores, the
capacity rule, and no byte at or past a capacity written.  The GPU parity tests
(test_gpu_lz4_large.py) run the kernels themselves on the same inputs.

LZ4_LARGE_EMUL_RECORD=<file> records every emulator call of a run for the stand-alone sanitizer
program (tools/lz4_large_emul.cpp with -DLZ4_LARGE_EMUL_MAIN), which replays them."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lz4_large_cases import (FULL_KINDS, KINDS, LENS, MAX_PAGE, crafted_streams, cuts, malformed_sources, page_of,
                             patched_streams)

LIB = os.path.join(ROOT, "tools", "bin", "liblz4largeemul.so")
SRC = os.path.join(ROOT, "tools", "lz4_large_emul.cpp")
CORE = os.path.join(ROOT, "tyche_amd", "csrc", "lz4_large_core.h")
GUARD = 64
RECORD = os.environ.get("LZ4_LARGE_EMUL_RECORD")


class Emul:
    def __init__(self, lib):
        self.lib = lib
        self.calls = 0

    def _call(self, mode, fn, src: bytes, cap: int):
        """(return value, dst[:cap]) of one call with source and destination at varying
        misalignments from a 16-byte line; asserts that nothing at or past cap was written."""
        self.calls += 1
        sa, da = (self.calls * 7) % 16, (self.calls * 5) % 16
        sbuf = np.zeros(len(src) + 32, np.uint8)
        so = (sa - sbuf.ctypes.data) % 16
        sbuf[so:so + len(src)] = np.frombuffer(src, np.uint8)
        dbuf = np.full(cap + GUARD + 32, 0xAB, np.uint8)
        do = (da - dbuf.ctypes.data) % 16
        r = fn(ctypes.c_void_p(sbuf.ctypes.data + so), len(src), ctypes.c_void_p(dbuf.ctypes.data + do), cap)
        assert bool((dbuf[do + cap:] == 0xAB).all()) and bool((dbuf[:do] == 0xAB).all()), \
            ("wrote outside the destination", mode, len(src), cap)
        if RECORD:
            with open(RECORD, "ab") as f:
                f.write(struct.pack("<IIIiII", mode, len(src), cap, r, sa, da) + src)
        return r, dbuf[do:do + cap]

    def dec(self, stream: bytes, cap: int):
        r, d = self._call(0, self.lib.lz4_large_emul_decompress, stream, cap)
        return r, d[:max(r, 0)].tobytes()

    def enc(self, page: bytes, cap: int):
        r, d = self._call(1, self.lib.lz4_large_emul_compress, page, cap)
        return r, d[:max(r, 0)].tobytes()


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in (SRC, CORE)):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    for fn in (lib.lz4_large_emul_decompress, lib.lz4_large_emul_compress):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return Emul(lib)


def check_decode(emul, O, page: bytes):
    stream = O.lz4_compress(page)
    r, got = emul.dec(stream, len(page))
    assert r == len(page), (len(page), r)
    assert got == page, len(page)


def check_encode(emul, O, page: bytes, caps_below=True):
    bound = O.lz4_bound(len(page))
    r, stream = emul.enc(page, bound)
    assert 0 < r <= bound, (len(page), r)
    rv, back = O.lz4_decompress(stream, len(page))
    assert rv == len(page) and back == page, (len(page), rv)
    if O.have_ref():
        rv, back = O.ref_lz4_decompress(stream, len(page))
        assert rv == len(page) and back == page, (len(page), rv)
    r2, again = emul.enc(page, r)                     # the capacity it needs is enough
    assert r2 == r and again == stream, (len(page), r, r2)
    if caps_below:
        for cap in sorted({r - 1, r - 7, r - r // 3, r // 2, 13, 1, 0}):
            if 0 <= cap < r:
                assert emul.enc(page, cap)[0] == 0, (len(page), r, cap)
    return r


@pytest.mark.parametrize("plen", LENS)
@pytest.mark.parametrize("kind", KINDS)
def test_decode(emul, oracle_mod, kind, plen):
    for i in range(2):
        check_decode(emul, oracle_mod, page_of(oracle_mod, kind, plen, i))


@pytest.mark.parametrize("kind", FULL_KINDS)
def test_decode_full_size(emul, oracle_mod, kind):
    check_decode(emul, oracle_mod, page_of(oracle_mod, kind, MAX_PAGE, 0, n=1))


@pytest.mark.parametrize("case", crafted_streams(), ids=lambda c: c[0])
def test_decode_crafted(emul, oracle_mod, case):
    name, stream, size = case
    want = oracle_mod.lz4_decompress(stream, size)
    assert want[0] == size, name                      # (the stream is what it was meant to be)
    assert emul.dec(stream, size) == want, name
    for cap in (size + 1, size + 100):                # room to spare changes nothing
        assert emul.dec(stream, cap) == want, (name, cap)


def test_decode_cut_streams(emul, oracle_mod):
    """Every stream cut at 40 seeded lengths: the oracle's return value, whatever it is."""
    for n, (name, stream, size) in enumerate(malformed_sources(oracle_mod)):
        for c in cuts(stream, n):
            want = oracle_mod.lz4_decompress(stream[:c], size)[0]
            assert emul.dec(stream[:c], size)[0] == want, (name, c, want)


def test_decode_patched_streams(emul, oracle_mod):
    for name, stream, size in patched_streams(oracle_mod):
        for cap in (size, size - 1, size + 1):
            want = oracle_mod.lz4_decompress(stream, cap)[0]
            assert emul.dec(stream, cap)[0] == want, (name, cap, want)


def test_decode_capacities(emul, oracle_mod):
    """Capacity one below and one above the true size, and far below it."""
    for name, stream, size in malformed_sources(oracle_mod):
        for cap in (size - 1, size + 1, size - 11, size - 12, size // 2, 0):
            want = oracle_mod.lz4_decompress(stream, cap)
            got = emul.dec(stream, cap)
            assert got[0] == want[0], (name, cap, want[0], got[0])
            if want[0] > 0:
                assert got[1] == want[1], (name, cap)


@pytest.mark.parametrize("plen", LENS)
@pytest.mark.parametrize("kind", KINDS)
def test_encode(emul, oracle_mod, kind, plen):
    for i in range(2):
        check_encode(emul, oracle_mod, page_of(oracle_mod, kind, plen, i), caps_below=i == 0)


@pytest.mark.parametrize("kind", FULL_KINDS)
def test_encode_full_size(emul, oracle_mod, kind):
    check_encode(emul, oracle_mod, page_of(oracle_mod, kind, MAX_PAGE, 0, n=1), caps_below=False)


def test_encode_small_and_short_tail(emul, oracle_mod):
    """The core has no lower limit of its own (the kernel only gets pages above 65,535 bytes): the
    empty page, pages around the 13-byte minimum, and lengths whose tail past a 64-position block
    is too short for a match."""
    rng = np.random.default_rng(5)
    assert emul.enc(b"", 1) == (1, b"\0") and emul.enc(b"", 0)[0] == 0
    for n in (1, 4, 12, 13, 14, 63, 64, 65, 76, 77, 1000, 65536 + 3, 65536 + 11, 65536 + 12, 65536 + 13):
        for sym in (1, 2, 256):
            check_encode(emul, oracle_mod, rng.integers(0, sym, n, dtype=np.uint8).tobytes(), caps_below=n < 2000)


def test_encode_ratio_against_32k_views(emul, oracle_mod):
    """The CPU stand-in of the GPU ratio test: a 262,144-byte page of each bench distribution takes
    at most 1.005x the bytes of its eight 32 KiB views compressed one by one by the reference parse
    (LZ4 1.7.5, byU16) -- the large page sees 65,535 bytes of history everywhere, a view on average a
    quarter of that, so losing to the views would mean the ring's history is not being used."""
    O = oracle_mod
    for d in range(6):
        page = page_of(O, f"dist{d}", 262144)
        ours = emul.enc(page, O.lz4_bound(len(page)))[0]
        views = sum(len(O.lz4_compress(page[i:i + 32768])) for i in range(0, len(page), 32768))
        print(f"dist{d}: emulator {ours} views {views} ({ours / views:.4f})")
        assert 0 < ours <= 1.005 * views, (d, ours, views)
