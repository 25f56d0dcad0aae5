"""The parts of the zlib shared-dictionary C API that need no GPU: the argument rules of the two
device-batch calls, the reach rule's refusal before any launch, that every handle is accepted (also one
that zstd refuses), the three independent process-wide slots, TYCHE_ZLIB_DICT files that cannot
serve, the Python surface, and a self-check of the case builders and of tests/golden/zlib_dict.npz
against the reference library (where it is built) and Python's zlib."""
import ctypes
import os
import subprocess
import sys

import pytest

import zlib_dict_cases as C
from conftest import ROOT

ZLIB = C.ZLIB
MAGIC = bytes([0x37, 0xA4, 0x30, 0xEC])


@pytest.fixture(scope="module")
def lib():
    from tyche_amd import _lib
    return _lib.load()


def _dummy_batch(_lib, res, **kw):
    dummy = ctypes.addressof(res)                         # never dereferenced: the calls are refused first
    return _lib.Batch(count=1, src=dummy, dst=dummy, results=dummy, **kw)


def test_null_arguments_and_empty_batches(lib):
    """NULL handle or NULL batch: TYCHE_E_BAD_ARGS; count == 0: TYCHE_E_OK, nothing looked at."""
    from tyche_amd import _lib
    h = lib.tyche_lz4_dict_create(b"abcdefgh" * 16, 128)
    res = (ctypes.c_int32 * 1)()
    b = _dummy_batch(_lib, res, src_stride=100, src_length=100, dst_stride=800, dst_capacity=800)
    empty = _lib.Batch(count=0)
    for call in (lib.tyche_zlib_compress_batch_dict, lib.tyche_zlib_decompress_batch_dict):
        assert call(None, ctypes.byref(b), None) == _lib.E_BAD_ARGS
        assert call(h, None, None) == _lib.E_BAD_ARGS
        assert call(h, ctypes.byref(empty), None) == 0
    lib.tyche_lz4_dict_destroy(h)


def test_reach_rule_is_refused_before_any_launch(lib):
    """declared maximum + D > 65536 (compress) and dst_capacity + D > 65536 (decompress) at D = 32768
    with 32769 against 32768: TYCHE_E_BAD_ARGS with the codec, the rule and both numbers; 32768 + 32768
    is inside the reach (whatever a machine without a GPU answers then, it is not the reach text)."""
    from tyche_amd import _lib
    D = 32768
    h = lib.tyche_lz4_dict_create(bytes(D), D)
    res = (ctypes.c_int32 * 1)()
    b = _dummy_batch(_lib, res, src_stride=65536, src_length=32769, dst_stride=70000, dst_capacity=70000)
    assert lib.tyche_zlib_compress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    msg = _lib.last_error()
    assert "zlib dictionary reach" in msg and "page (32769)" in msg and "(32768 bytes)" in msg and "65536" in msg, msg
    b = _dummy_batch(_lib, res, src_stride=100, src_length=100, dst_stride=65536, dst_capacity=32769)
    assert lib.tyche_zlib_decompress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    msg = _lib.last_error()
    assert "zlib dictionary reach" in msg and "capacity (32769)" in msg and "(32768 bytes)" in msg, msg
    lens = (ctypes.c_uint32 * 1)(100)
    b = _dummy_batch(_lib, res, src_lengths=ctypes.addressof(lens), max_src_length=0, dst_capacity=70000)
    assert lib.tyche_zlib_compress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS   # undeclared: 65535
    assert "65535" in _lib.last_error()
    lib.tyche_lz4_dict_destroy(h)


def test_every_handle_is_accepted(lib):
    """Bytes that begin with zstd's dictionary magic are raw bytes to zlib: the zlib calls get past
    their handle checks with them (an empty batch is TYCHE_E_OK, tyche_zlib_use_dict installs), while
    tyche_zstd_use_dict still refuses the same handle."""
    from tyche_amd import _lib
    blob = MAGIC + bytes(100)
    h = lib.tyche_lz4_dict_create(blob, len(blob))
    empty = _lib.Batch(count=0)
    try:
        assert lib.tyche_zlib_compress_batch_dict(h, ctypes.byref(empty), None) == 0
        assert lib.tyche_zlib_decompress_batch_dict(h, ctypes.byref(empty), None) == 0
        assert lib.tyche_zstd_compress_batch_dict(h, ctypes.byref(empty), None) == _lib.E_BAD_ARGS
        assert lib.tyche_zlib_use_dict(h) == 0, _lib.last_error()
        cur = lib.tyche_zlib_current_dict()
        assert cur and lib.tyche_lz4_dict_length(cur) == len(blob)
        lib.tyche_lz4_dict_destroy(cur)
        assert lib.tyche_zstd_use_dict(h) == _lib.E_BAD_ARGS
        assert "structured dictionaries are not supported" in _lib.last_error()
        assert not lib.tyche_zstd_current_dict()
    finally:
        lib.tyche_zlib_use_dict(None)
        lib.tyche_lz4_dict_destroy(h)
    assert not lib.tyche_zlib_current_dict()


def _bytes_of(lib, h):
    n = lib.tyche_lz4_dict_length(h)
    out = ctypes.create_string_buffer(max(n, 1))
    lib.tyche_lz4_dict_bytes(h, out, n)
    return out.raw[:n]


def test_three_independent_slots(lib):
    """Install in one slot and the other two current_dict calls stay NULL, for each of the three; the
    zlib slot holds a reference of its own, is replaced and removed by tyche_zlib_use_dict alone."""
    slots = {"lz4": (lib.tyche_lz4_use_dict, lib.tyche_lz4_current_dict),
             "zstd": (lib.tyche_zstd_use_dict, lib.tyche_zstd_current_dict),
             "zlib": (lib.tyche_zlib_use_dict, lib.tyche_zlib_current_dict)}
    for use, cur in slots.values():
        assert not cur()
    try:
        for name, (use, cur) in slots.items():
            data = (name + "-dict").encode() * 20
            h = lib.tyche_lz4_dict_create(data, len(data))
            assert use(h) == 0
            lib.tyche_lz4_dict_destroy(h)                  # the creator's reference may go first
            c = cur()
            assert c and _bytes_of(lib, c) == data, name
            lib.tyche_lz4_dict_destroy(c)
            for other, (_, ocur) in slots.items():
                if other != name:
                    assert not ocur(), (name, other)
            assert use(None) == 0
            assert not cur()
        a = lib.tyche_lz4_dict_create(b"a" * 64, 64)
        b = lib.tyche_lz4_dict_create(b"b" * 80, 80)
        assert lib.tyche_zlib_use_dict(a) == 0 and lib.tyche_zlib_use_dict(b) == 0   # replaces (and releases) the first
        assert lib.tyche_lz4_use_dict(a) == 0 and lib.tyche_zstd_use_dict(a) == 0
        assert lib.tyche_lz4_use_dict(None) == 0 and lib.tyche_zstd_use_dict(None) == 0
        c = lib.tyche_zlib_current_dict()
        assert c and _bytes_of(lib, c) == b"b" * 80       # the other slots' installs and removals left it alone
        lib.tyche_lz4_dict_destroy(c)
        lib.tyche_lz4_dict_destroy(a)
        lib.tyche_lz4_dict_destroy(b)
    finally:
        for use, _ in slots.values():
            use(None)


def test_env_dictionary_that_cannot_serve_fails_every_zlib_host_call(tmp_path):
    """TYCHE_ZLIB_DICT naming a missing, an empty or an over-long file: code 190 with the variable's
    name and the reason from the zlib host entry points, every time, before any device work (a fresh
    child process each).  The zstd host calls of that process do not read the variable."""
    empty = tmp_path / "empty.dict"
    empty.write_bytes(b"")
    big = tmp_path / "big.dict"
    big.write_bytes(bytes(32769))
    code = ("import ctypes, numpy as np\n"
            "from tyche_amd import _lib\n"
            "lib = _lib.load()\n"
            "page = np.zeros(100, np.uint8); out = np.zeros(800, np.uint8); res = (ctypes.c_int32 * 1)()\n"
            "srcs = (ctypes.c_void_p * 1)(page.ctypes.data); dsts = (ctypes.c_void_p * 1)(out.ctypes.data)\n"
            "slen, dcap = (ctypes.c_uint32 * 1)(100), (ctypes.c_uint32 * 1)(800)\n"
            "for k in range(2):\n"
            "    rc = lib.tyche_compress_host(2, 1, 1, srcs, slen, dsts, dcap, res)\n"
            "    print(rc, _lib.last_error())\n"
            "rc = lib.tyche_decompress_host(2, 1, srcs, slen, dsts, dcap, res)\n"
            "print(rc, _lib.last_error())\n"
            "print('current', lib.tyche_zlib_current_dict())\n"
            "rc = lib.tyche_compress_host(3, 1, 1, srcs, slen, dsts, dcap, res)\n"
            "print('zstd', rc)\n")
    for path, why in ((tmp_path / "missing.dict", "cannot read"), (empty, "is empty"), (big, "longer than")):
        env = {k: v for k, v in os.environ.items() if not k.startswith(("TYCHE_LZ4_DICT", "TYCHE_ZSTD_DICT"))}
        env.update(TYCHE_ZLIB_DICT=str(path), PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 5, p.stdout
        for ln in lines[:3]:
            assert ln.startswith("190 ") and "TYCHE_ZLIB_DICT" in ln and why in ln, ln
        assert lines[3] == "current None", lines[3]
        assert lines[4].startswith("zstd ") and lines[4] != "zstd 190", lines[4]


def test_python_surface():
    """use_zlib_dict is exported and installs; the private helpers keep raising ValueError for zlib
    with a dictionary (the public functions route that case before they reach them)."""
    import tyche_amd
    from tyche_amd import _lib, codec
    assert tyche_amd.use_zlib_dict is codec.use_zlib_dict
    for name in ("tyche_zlib_compress_batch_dict", "tyche_zlib_decompress_batch_dict", "tyche_zlib_use_dict",
                 "tyche_zlib_current_dict"):
        assert name in _lib.SIGNATURES
    d = codec.Dictionary(b"abcdefgh" * 16)
    res = (ctypes.c_int32 * 1)()
    b = _dummy_batch(_lib, res, src_stride=100, src_length=100, dst_stride=800, dst_capacity=800)
    with pytest.raises(ValueError):
        codec._compress_call(_lib.ZLIB_COMPRESSOR_ID, 1, b, None, d)
    with pytest.raises(ValueError):
        codec._decompress_call(_lib.ZLIB_COMPRESSOR_ID, b, None, d)
    assert not codec._zlib_dict_call(True, _lib.ZLIB_COMPRESSOR_ID, b, None, None)       # no dictionary: not this call
    assert not codec._zlib_dict_call(True, _lib.ZSTD_COMPRESSOR_ID, b, None, d)
    codec.use_zlib_dict(d)
    cur = _lib.load().tyche_zlib_current_dict()
    assert cur
    _lib.load().tyche_lz4_dict_destroy(cur)
    codec.use_zlib_dict(None)
    assert not _lib.load().tyche_zlib_current_dict()
    d.close()


def test_cases_and_golden_file(oracle_mod):
    """The crafted streams are what they are meant to be by Python's zlib and by the recorded
    reference verdicts; every recorded stream restores through Python's zlib with the dictionary, begins
    with 78 3F and the dictionary's adler32, and is refused without the dictionary; six of the eight
    ratio cells gain at least 2 % in the reference.  Where oracle/_ref is built, the reference library
    gives today what was recorded."""
    O = oracle_mod
    G = C.Golden()
    R = C.ref_or_none(O)
    cases = C.crafted_cases()
    assert len(cases) == len(G.crafted_rv) == len(G.crafted_crc)
    for i, (name, dic, stream, cap, want) in enumerate(cases):
        r, dec = C.py_decompress(dic, stream, cap)
        if isinstance(want, bytes):
            assert (r, dec) == (len(want), want), name
            assert int(G.crafted_rv[i]) == len(want) and int(G.crafted_crc[i]) == C.crc(want), name
        else:
            assert r == want == int(G.crafted_rv[i]), (name, r)
        if R is not None:
            rr, rdec = R.decompress(dic, stream, cap)
            assert rr == int(G.crafted_rv[i]) and C.crc(rdec) == int(G.crafted_crc[i]), name
    for D, L, k, dic, page, s in G.rt_cases(O):
        assert s[:6] == C.dict_header(dic), (D, L, k)
        assert C.py_decompress(dic, s, L) == (L, page), (D, L, k)
        assert C.py_decompress(None, s, L)[0] == C.Z_DATA, (D, L, k)
        if R is not None:
            assert R.compress(dic, page) == s, (D, L, k)
    dic, streams = C.malformed_cases(O)
    assert len(G.malformed_rv) == len(streams) == len(G.malformed_crc)
    if R is not None:
        for i, (f, cap) in enumerate(streams):
            r, dec = R.decompress(dic, f, cap)
            assert r == int(G.malformed_rv[i]) and C.crc(dec) == int(G.malformed_crc[i]), i
    assert [int(x) for x in G.used_ref] == [14, 50, 141]
    gains = [1 - int(a) / int(b) for a, b in zip(G.ratio_ref, G.ratio_ref_plain)]
    assert sum(g >= 0.02 for g in gains) == 6, gains
    assert C.stored_stream(b"abc") == bytes.fromhex("7801010300fcff616263") + C.adler(b"abc").to_bytes(4, "big")
