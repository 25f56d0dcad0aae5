"""CPU checks of LZ4 with a shared dictionary: the kernels' per-wave code (tyche_amd/csrc/
lz4_dict_core.h -- the decoder of lz4_decode_dict.hip with its verdicts, and the emission of
lz4_encode_dict.hip) through the host emulator tools/lz4_dict_emul.cpp, against the reference
(LZ4 1.7.5's LZ4_decompress_safe_usingDict and LZ4_loadDict + LZ4_compress_fast_continue) where
oracle/_ref is built and against tests/golden/lz4_dict.npz, which was recorded from it; and the
parts of the C API that need no GPU (handle limits, the reach rule's refusal, LZ4_EXACT).
test_gpu_lz4_dict.py runs the kernels themselves on the same cases.

LZ4_DICT_EMUL_RECORD=<file> records every emulator call of a run for the stand-alone sanitizer
program (tools/lz4_dict_emul.cpp with -DLZ4_DICT_EMUL_MAIN), which replays them."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import lz4_dict_cases as C
from conftest import ROOT

LIB = os.path.join(ROOT, "tools", "bin", "liblz4dictemul.so")
SRC = os.path.join(ROOT, "tools", "lz4_dict_emul.cpp")
CORE = os.path.join(ROOT, "tyche_amd", "csrc", "lz4_dict_core.h")
GUARD = 64
RECORD = os.environ.get("LZ4_DICT_EMUL_RECORD")


class Emul:
    def __init__(self, lib):
        self.lib = lib

    def _call(self, mode, fn, dic: bytes, src: bytes, cap: int):
        d = np.frombuffer(dic, np.uint8).copy()
        s = np.frombuffer(src, np.uint8).copy() if src else np.zeros(1, np.uint8)
        dbuf = np.full(GUARD + cap + GUARD, 0xAB, np.uint8)
        r = fn(d.ctypes.data, len(dic), s.ctypes.data, len(src), dbuf.ctypes.data + GUARD, cap)
        assert bool((dbuf[:GUARD] == 0xAB).all()) and bool((dbuf[GUARD + cap:] == 0xAB).all()), \
            ("wrote outside the destination", mode, len(dic), len(src), cap)
        if RECORD:
            with open(RECORD, "ab") as f:
                f.write(struct.pack("<IIIIi", mode, len(dic), len(src), cap, r) + dic + src)
        return r, dbuf[GUARD:GUARD + max(r, 0)].tobytes()

    def dec(self, dic: bytes, stream: bytes, cap: int):
        return self._call(0, self.lib.lz4_dict_emul_decompress, dic, stream, cap)

    def enc(self, dic: bytes, page: bytes, cap: int):
        return self._call(1, self.lib.lz4_dict_emul_compress, dic, page, cap)


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in (SRC, CORE)):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    for fn in (lib.lz4_dict_emul_decompress, lib.lz4_dict_emul_compress):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return Emul(lib)


@pytest.fixture(scope="module")
def golden():
    return C.Golden()


@pytest.fixture(scope="module")
def ref(oracle_mod):
    return C.ref_or_none(oracle_mod)


def test_decode_reference_streams(emul, oracle_mod, golden, ref):
    """Reference-made dictionary streams of every size and page kind decode to the page with
    result L: the golden subset always, the whole matrix where the reference library is built."""
    for D, L, kind, dic, page, stream in golden.rt_cases(oracle_mod):
        assert emul.dec(dic, stream, L) == (L, page), (D, L, kind)
    if ref is None:
        return
    for D, L, kind, dic, page in C.all_cases(oracle_mod):
        stream = ref.compress(dic, page)
        assert emul.dec(dic, stream, L) == (L, page), (D, L, kind)
        for cap in (L + 1, L + 100):                      # room to spare changes nothing
            if cap + D <= C.WINDOW:
                assert emul.dec(dic, stream, cap) == (L, page), (D, L, kind, cap)


def test_encode_roundtrip(emul, oracle_mod, ref):
    """The emission: every stream restores to the page (through the reference where it is built,
    and through the emulated decoder), needs exactly its own size as capacity, and a capacity
    below that gives 0 with nothing written past it."""
    for D, L, kind, dic, page in C.all_cases(oracle_mod):
        bound = C.lz4_bound(L)
        r, stream = emul.enc(dic, page, bound)
        assert 0 < r <= bound, (D, L, kind, r)
        assert emul.dec(dic, stream, L) == (L, page), (D, L, kind)
        if ref is not None:
            assert ref.decompress(dic, stream, L) == (L, page), (D, L, kind)
        assert emul.enc(dic, page, r) == (r, stream), (D, L, kind)
        for cap in sorted({r - 1, r // 2, 0}):
            if 0 <= cap < r:
                assert emul.enc(dic, page, cap)[0] == 0, (D, L, kind, cap)


@pytest.mark.parametrize("L", [64, 4096, 16384])
def test_dictionary_is_used(emul, oracle_mod, L):
    """A page equal to the dictionary's tail is one long match into it."""
    D = 16384
    dic, page = C.dict_of(oracle_mod, D, "tail"), C.page_of(oracle_mod, D, L, "tail")
    r, stream = emul.enc(dic, page, C.lz4_bound(L))
    assert 0 < r <= L // 255 + 32, (L, r)
    assert C.max_reach(stream) > 0, "no offset reaches past the page's start"


def test_crafted_verdicts(emul, oracle_mod, golden, ref):
    cases = C.crafted(oracle_mod)
    assert len(cases) == len(golden.crafted_rv)
    for (name, D, dic, stream, cap), want, crc in zip(cases, golden.crafted_rv, golden.crafted_crc):
        if ref is not None:                               # the golden file is what the reference says
            r, dec = ref.decompress(dic, stream, cap)
            assert (r, C.crc(dec)) == (int(want), int(crc)), name
        r, dec = emul.dec(dic, stream, cap)
        assert r == int(want), (name, r, int(want))
        if want >= 0 and "zero-offset" not in name:
            assert C.crc(dec) == int(crc), name
    names = [c[0] for c in cases]
    rv = dict(zip(names, golden.crafted_rv))
    assert rv["reach-D1000-lead3"] == 19 and rv["reach+1-D1000-lead3"] < 0      # the cases are what they were meant to be
    assert rv["late-match-D64"] < 0 and rv["late-match-ok-D64"] == 13 and rv["lit-overrun-D64"] < 0


def test_empty_input(emul, oracle_mod):
    """The reference reads the byte after an empty input, so its value there is not defined; the
    kernels answer -1, as the plain decoders do."""
    dic = C.dict_of(oracle_mod, 1000, "generic")
    assert emul.dec(dic, b"", 16)[0] == -1 and emul.dec(dic, b"", 0)[0] == -1


def test_malformed_verdicts(emul, oracle_mod, golden, ref):
    """The 10 reference-made dictionary streams (4 KiB pages, D = 1000), each cut at up to 40
    lengths and patched at 40 positions: the reference's value, and its bytes where that is not
    negative."""
    dicts = [d for d, _ in C.base_cases(oracle_mod)]
    if ref is not None:
        assert [ref.compress(d, p) for d, p in C.base_cases(oracle_mod)] == golden.base_streams
    cases = C.malformed(golden.base_streams)
    assert len(cases) == len(golden.malformed_rv)
    accepted = 0
    for (name, i, stream, cap), want, crc in zip(cases, golden.malformed_rv, golden.malformed_crc):
        r, dec = emul.dec(dicts[i], stream, cap)
        assert r == int(want), (name, r, int(want))
        if want > 0 and not C.has_zero_offset(stream):
            assert C.crc(dec) == int(crc), name
            accepted += 1
    assert accepted > 20 and int((golden.malformed_rv < 0).sum()) > 300


# ---------------------------------------------------------------- the C API without a GPU
@pytest.fixture(scope="module")
def lib():
    from tyche_amd import _lib
    return _lib.load()


def test_dict_handle_limits(lib):
    from tyche_amd import _lib
    assert not lib.tyche_lz4_dict_create(b"", 0)
    assert "TYCHE_LZ4_DICT_MAX" in _lib.last_error()
    big = bytes(_lib.LZ4_DICT_MAX + 1)
    assert not lib.tyche_lz4_dict_create(big, len(big))
    assert str(_lib.LZ4_DICT_MAX + 1) in _lib.last_error()
    assert not lib.tyche_lz4_dict_create(None, 5)
    h = lib.tyche_lz4_dict_create(big, _lib.LZ4_DICT_MAX)
    assert h and lib.tyche_lz4_dict_length(h) == _lib.LZ4_DICT_MAX
    lib.tyche_lz4_dict_destroy(h)
    assert lib.tyche_lz4_dict_length(None) == 0
    lib.tyche_lz4_dict_destroy(None)


def test_dict_install_and_remove(lib):
    """The process-wide slot holds a reference of its own: the creator's may go first."""
    h = lib.tyche_lz4_dict_create(b"abcdefgh" * 100, 800)
    assert lib.tyche_lz4_use_dict(h) == 0
    lib.tyche_lz4_dict_destroy(h)
    h2 = lib.tyche_lz4_dict_create(b"12345678" * 10, 80)
    assert lib.tyche_lz4_use_dict(h2) == 0                # replaces (and releases) the first
    assert lib.tyche_lz4_use_dict(None) == 0
    lib.tyche_lz4_dict_destroy(h2)


def test_reach_rule_is_refused_before_any_launch(lib):
    from tyche_amd import _lib
    D = 4096
    h = lib.tyche_lz4_dict_create(bytes(D), D)
    res = (ctypes.c_int32 * 1)()
    dummy = ctypes.addressof(res)                         # never dereferenced: the call is refused first
    b = _lib.Batch(count=1, src=dummy, src_stride=65536, src_length=65536 - D + 1, dst=dummy, dst_stride=70000,
                   dst_capacity=70000, results=dummy)
    assert lib.tyche_lz4_compress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    msg = _lib.last_error()
    assert str(65536 - D + 1) in msg and str(D) in msg and "65536" in msg, msg
    lens = (ctypes.c_uint32 * 1)(100)
    b = _lib.Batch(count=1, src=dummy, src_lengths=ctypes.addressof(lens), max_src_length=0, dst=dummy,
                   dst_capacity=70000, results=dummy)    # an undeclared maximum still means 65535
    assert lib.tyche_lz4_compress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    assert "65535" in _lib.last_error()
    b = _lib.Batch(count=1, src=dummy, src_stride=100, src_length=100, dst=dummy, dst_stride=65536,
                   dst_capacity=65536 - D + 1, results=dummy)
    assert lib.tyche_lz4_decompress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    msg = _lib.last_error()
    assert str(65536 - D + 1) in msg and str(D) in msg, msg
    assert lib.tyche_lz4_compress_batch_dict(None, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    lib.tyche_lz4_dict_destroy(h)


def test_exact_mode_and_dictionary_do_not_combine(lib, knobs):
    from tyche_amd import _lib
    h = lib.tyche_lz4_dict_create(bytes(64), 64)
    res = (ctypes.c_int32 * 1)()
    dummy = ctypes.addressof(res)
    b = _lib.Batch(count=1, src=dummy, src_stride=100, src_length=100, dst=dummy, dst_stride=200, dst_capacity=200,
                   results=dummy)
    knobs(LZ4_EXACT=1)
    assert lib.tyche_lz4_compress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    assert "LZ4_EXACT" in _lib.last_error() and "dictionary" in _lib.last_error()
    # the host entry points with a process-wide dictionary: refused before any device work
    assert lib.tyche_lz4_use_dict(h) == 0
    try:
        page = np.zeros(100, np.uint8)
        out = np.zeros(200, np.uint8)
        srcs = (ctypes.c_void_p * 1)(page.ctypes.data)
        dsts = (ctypes.c_void_p * 1)(out.ctypes.data)
        slen, dcap = (ctypes.c_uint32 * 1)(100), (ctypes.c_uint32 * 1)(200)
        assert lib.tyche_compress_host(1, 1, 1, srcs, slen, dsts, dcap, res) == _lib.E_BAD_ARGS
        assert "LZ4_EXACT" in _lib.last_error()
    finally:
        lib.tyche_lz4_use_dict(None)
        lib.tyche_lz4_dict_destroy(h)


def test_env_dictionary_that_cannot_serve_fails_every_host_call(tmp_path):
    """TYCHE_LZ4_DICT naming a missing, an empty or an oversized file: TYCHE_E_BAD_ARGS with the
    reason from the host entry points, before any device work (a fresh child process each)."""
    import sys
    empty = tmp_path / "empty.dict"
    empty.write_bytes(b"")
    big = tmp_path / "big.dict"
    big.write_bytes(bytes(32769))
    code = ("import ctypes, numpy as np\n"
            "from tyche_amd import _lib\n"
            "lib = _lib.load()\n"
            "page = np.zeros(100, np.uint8); out = np.zeros(200, np.uint8); res = (ctypes.c_int32 * 1)()\n"
            "srcs = (ctypes.c_void_p * 1)(page.ctypes.data); dsts = (ctypes.c_void_p * 1)(out.ctypes.data)\n"
            "slen, dcap = (ctypes.c_uint32 * 1)(100), (ctypes.c_uint32 * 1)(200)\n"
            "for k in range(2):\n"
            "    rc = lib.tyche_compress_host(1, 1, 1, srcs, slen, dsts, dcap, res)\n"
            "    print(rc, _lib.last_error())\n"
            "rc = lib.tyche_decompress_host(1, 1, srcs, slen, dsts, dcap, res)\n"
            "print(rc, _lib.last_error())\n")
    for path, why in ((tmp_path / "missing.dict", "cannot read"), (empty, "is empty"), (big, "longer than")):
        env = dict(os.environ, TYCHE_LZ4_DICT=str(path), PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 3, p.stdout
        for ln in lines:
            assert ln.startswith("190 ") and "TYCHE_LZ4_DICT" in ln and why in ln, ln
