"""CPU check of the exact LZ4 encoder's algorithm (tyche_amd/csrc/lz4_exact_core.h, the per-wave
code of lz4_encode_exact.hip, LZ4_EXACT=1) through its host emulator tools/lz4x_emul.cpp, against
the restated LZ4_compress_default of LZ4 1.7.5 (oracle.lz4_compress, lz4.c:697): return value and
bytes on the reference fixtures, every page kind of the GPU tests, 24,000 random small pages and
the limited-output capacities; no byte at or past the capacity is written.  The GPU parity tests
(test_gpu_lz4_exact.py) run the kernel itself on the same inputs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, unpack
from lz4_exact_cases import KINDS, PAGE_LENS, kind_pages, limited_caps, limited_pages, ragged_pages

LIB = os.path.join(ROOT, "tools", "bin", "liblz4xemul.so")
SRC = os.path.join(ROOT, "tools", "lz4x_emul.cpp")
CORE = os.path.join(ROOT, "tyche_amd", "csrc", "lz4_exact_core.h")
GUARD = 64


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in (SRC, CORE)):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.lz4x_emul_compress.restype = ctypes.c_int
    lib.lz4x_emul_sched.restype = ctypes.c_uint32
    lib.lz4x_emul_sched.argtypes = [ctypes.c_uint32]

    def enc(page: bytes, cap: int):
        """(return value, the bytes it covers); asserts that nothing at or past cap was written."""
        src = (ctypes.c_uint8 * max(len(page), 1)).from_buffer_copy(page if page else b"\0")
        dst = np.full(cap + GUARD, 0xAB, np.uint8)
        r = lib.lz4x_emul_compress(src, len(page), dst.ctypes.data_as(ctypes.c_void_p), cap)
        assert bool((dst[cap:] == 0xAB).all()), ("wrote past the capacity", len(page), cap)
        return r, dst[:max(r, 0)].tobytes()
    enc.lib = lib
    return enc


def check(emul, O, page: bytes, cap=None):
    cap = O.lz4_bound(len(page)) if cap is None else cap
    want = O.lz4_compress(page, cap)
    r, got = emul(page, cap)
    assert r == len(want), (len(page), cap, r, len(want))
    assert got == want, (len(page), cap)


def test_schedule_closed_form(emul):
    """lzx::sched(t) is the sum of the steps s_0 = 1, s_j = (63 + j) >> 6 (lz4.c:519-546)."""
    q = 0
    for t in range(70000):
        assert emul.lib.lz4x_emul_sched(t) == q, t
        q += 1 if t == 0 else (63 + t) >> 6
        if q > 1 << 28:
            break


def test_fixtures(emul, oracle_mod):
    O = oracle_mod
    g = load_golden("kat_lorem.npz")
    r, got = emul(g["text"].tobytes(), O.lz4_bound(4096))
    assert r == 2578 and got == g["lz4"].tobytes()
    g = load_golden("lz4_generated.npz")
    seed = int(g["seed"])
    for i, (dist, plen, idx) in enumerate(g["meta"]):
        page = O.pagegen(1, int(plen), seed=seed, first=int(idx), dist=int(dist))[0].tobytes()
        r, got = emul(page, O.lz4_bound(len(page)))
        assert got == unpack(g["comp"], g["comp_off"], g["comp_len"], i), (dist, plen, idx)
    g = load_golden("lz4_sample.npz")
    for k, i in enumerate(g["raw_index"]):
        raw = unpack(g["raw"], g["raw_off"], g["raw_len"], k)
        r, got = emul(raw, O.lz4_bound(len(raw)))
        assert got == unpack(g["comp"], g["comp_off"], g["comp_len"], int(i)), k


@pytest.mark.parametrize("plen", PAGE_LENS)
@pytest.mark.parametrize("kind", KINDS)
def test_page_kinds(emul, oracle_mod, kind, plen):
    pages = kind_pages(oracle_mod, kind, plen)
    for i in range(len(pages)):
        check(emul, oracle_mod, pages[i].tobytes())


@pytest.mark.parametrize("symbols", [2, 4, 256])
def test_random_small_pages(emul, oracle_mod, symbols):
    """8,000 random pages of 1..300 bytes per alphabet, and the empty page; every tenth also at
    a capacity below the bound (limited output)."""
    rng = np.random.default_rng(symbols)
    check(emul, oracle_mod, b"")
    check(emul, oracle_mod, b"", 0)
    for i in range(8000):
        n = int(rng.integers(1, 301))
        page = rng.integers(0, symbols, n, dtype=np.uint8).tobytes()
        check(emul, oracle_mod, page)
        if i % 10 == 0:
            check(emul, oracle_mod, page, int(rng.integers(0, n + 20)))


@pytest.mark.parametrize("symbols", [2, 4, 256])
def test_ragged_small_pages(emul, oracle_mod, symbols):
    for page in ragged_pages(symbols):
        check(emul, oracle_mod, page)


@pytest.mark.parametrize("which", [0, 1], ids=["compressible", "incompressible"])
def test_limited_output(emul, oracle_mod, which):
    page = limited_pages(oracle_mod)[which]
    for cap in limited_caps(oracle_mod, page, 7 + which):
        check(emul, oracle_mod, page, cap)
