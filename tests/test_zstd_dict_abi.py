"""The parts of the zstd shared-dictionary C API that need no GPU: the handle is the LZ4 one, the
structured-dictionary refusal, the reach rule's refusal before any launch, the process-wide slot
(separate from LZ4's), TYCHE_ZSTD_DICT files that cannot serve, the Python surface's zlib refusal,
and a self-check of tests/golden/zstd_dict.npz against the reference library where it is built."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import zstd_dict_cases as C
from conftest import ROOT

ZSTD = 3


@pytest.fixture(scope="module")
def lib():
    from tyche_amd import _lib
    return _lib.load()


def _dummy_batch(_lib, res, **kw):
    dummy = ctypes.addressof(res)                         # never dereferenced: the calls are refused first
    return _lib.Batch(count=1, src=dummy, dst=dummy, results=dummy, **kw)


def test_handle_is_the_lz4_handle_and_magic_is_refused(lib):
    """A dictionary that begins with ZSTD_DICT_MAGIC is a structured dictionary to the reference:
    TYCHE_E_BAD_ARGS from every zstd dictionary call and from tyche_zstd_use_dict, with the reason;
    the LZ4 calls keep accepting the handle.  Three magic bytes, or the magic anywhere else, are
    raw content."""
    from tyche_amd import _lib
    res = (ctypes.c_int32 * 1)()
    b = _dummy_batch(_lib, res, src_stride=100, src_length=100, dst_stride=800, dst_capacity=800)
    for blob in (C.MAGIC, C.MAGIC + bytes(100)):
        h = lib.tyche_lz4_dict_create(blob, len(blob))
        assert h and lib.tyche_lz4_dict_length(h) == len(blob)
        for call in (lib.tyche_zstd_compress_batch_dict, lib.tyche_zstd_decompress_batch_dict):
            assert call(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS
            assert "structured dictionaries are not supported" in _lib.last_error(), _lib.last_error()
        assert lib.tyche_zstd_use_dict(h) == _lib.E_BAD_ARGS
        assert "structured dictionaries are not supported" in _lib.last_error()
        assert not lib.tyche_zstd_current_dict()
        assert lib.tyche_lz4_use_dict(h) == 0              # raw bytes to LZ4
        assert lib.tyche_lz4_use_dict(None) == 0
        lib.tyche_lz4_dict_destroy(h)
    for blob in (C.MAGIC[:3], b"\x00" + C.MAGIC + bytes(8)):
        h = lib.tyche_lz4_dict_create(blob, len(blob))
        assert lib.tyche_zstd_use_dict(h) == 0, _lib.last_error()
        assert lib.tyche_zstd_use_dict(None) == 0
        lib.tyche_lz4_dict_destroy(h)
    # the handle's own limits are tyche_lz4_dict_create's
    assert not lib.tyche_lz4_dict_create(bytes(C.DICT_MAX + 1), C.DICT_MAX + 1)
    assert lib.tyche_zstd_compress_batch_dict(None, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    assert lib.tyche_zstd_decompress_batch_dict(None, ctypes.byref(b), None) == _lib.E_BAD_ARGS


def test_reach_rule_is_refused_before_any_launch(lib):
    """declared maximum + D > 65536 (compress) and dst_capacity + D > 65536 (decompress):
    TYCHE_E_BAD_ARGS with the rule and both numbers, no device needed."""
    from tyche_amd import _lib
    D = 4096
    h = lib.tyche_lz4_dict_create(bytes(D), D)
    res = (ctypes.c_int32 * 1)()
    b = _dummy_batch(_lib, res, src_stride=65536, src_length=65536 - D + 1, dst_stride=70000, dst_capacity=70000)
    assert lib.tyche_zstd_compress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    msg = _lib.last_error()
    assert "zstd" in msg and str(65536 - D + 1) in msg and str(D) in msg and "65536" in msg, msg
    lens = (ctypes.c_uint32 * 1)(100)
    b = _dummy_batch(_lib, res, src_lengths=ctypes.addressof(lens), max_src_length=0, dst_capacity=70000)
    assert lib.tyche_zstd_compress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS   # undeclared: 65535
    assert "65535" in _lib.last_error()
    b = _dummy_batch(_lib, res, src_stride=100, src_length=100, dst_stride=65536, dst_capacity=65536 - D + 1)
    assert lib.tyche_zstd_decompress_batch_dict(h, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    msg = _lib.last_error()
    assert "zstd" in msg and str(65536 - D + 1) in msg and str(D) in msg, msg
    lib.tyche_lz4_dict_destroy(h)


def _bytes_of(lib, h):
    n = lib.tyche_lz4_dict_length(h)
    out = ctypes.create_string_buffer(max(n, 1))
    lib.tyche_lz4_dict_bytes(h, out, n)
    return out.raw[:n]


def test_install_remove_and_separate_slots(lib):
    """tyche_zstd_use_dict installs, replaces and removes; the slot holds a reference of its own; the
    LZ4 slot and the zstd slot do not see each other."""
    assert not lib.tyche_zstd_current_dict() and not lib.tyche_lz4_current_dict()
    hz = lib.tyche_lz4_dict_create(b"zstd-abc" * 100, 800)
    hl = lib.tyche_lz4_dict_create(b"lz4-1234" * 10, 80)
    try:
        assert lib.tyche_zstd_use_dict(hz) == 0
        assert not lib.tyche_lz4_current_dict()            # installing for zstd leaves LZ4 without one
        assert lib.tyche_lz4_use_dict(hl) == 0
        cur = lib.tyche_zstd_current_dict()
        assert cur and _bytes_of(lib, cur) == b"zstd-abc" * 100   # and LZ4's install left zstd's alone
        lib.tyche_lz4_dict_destroy(cur)
        cur = lib.tyche_lz4_current_dict()
        assert cur and _bytes_of(lib, cur) == b"lz4-1234" * 10
        lib.tyche_lz4_dict_destroy(cur)
        assert lib.tyche_lz4_use_dict(None) == 0
        cur = lib.tyche_zstd_current_dict()
        assert cur and lib.tyche_lz4_dict_length(cur) == 800      # removing LZ4's keeps zstd's
        lib.tyche_lz4_dict_destroy(cur)
        lib.tyche_lz4_dict_destroy(hz)                     # the creator's reference may go first
        hz = None
        cur = lib.tyche_zstd_current_dict()
        assert cur and _bytes_of(lib, cur) == b"zstd-abc" * 100
        lib.tyche_lz4_dict_destroy(cur)
        assert lib.tyche_zstd_use_dict(hl) == 0            # replaces (and releases) the first
        assert lib.tyche_zstd_use_dict(None) == 0
        assert not lib.tyche_zstd_current_dict()
    finally:
        lib.tyche_zstd_use_dict(None)
        lib.tyche_lz4_use_dict(None)
        lib.tyche_lz4_dict_destroy(hl)
        if hz:
            lib.tyche_lz4_dict_destroy(hz)


def test_env_dictionary_that_cannot_serve_fails_every_zstd_host_call(tmp_path):
    """TYCHE_ZSTD_DICT naming a missing, an empty, an oversized or a structured file: TYCHE_E_BAD_ARGS
    with the reason from the zstd host entry points, every time, before any device work (a fresh
    child process each).  The LZ4 host calls of that process do not read the variable: they get past
    their dictionary lookup (whatever a machine without a GPU answers then, it is not 190)."""
    empty = tmp_path / "empty.dict"
    empty.write_bytes(b"")
    big = tmp_path / "big.dict"
    big.write_bytes(bytes(32769))
    structured = tmp_path / "structured.dict"
    structured.write_bytes(C.MAGIC + bytes(252))
    code = ("import ctypes, numpy as np\n"
            "from tyche_amd import _lib\n"
            "lib = _lib.load()\n"
            "page = np.zeros(100, np.uint8); out = np.zeros(800, np.uint8); res = (ctypes.c_int32 * 1)()\n"
            "srcs = (ctypes.c_void_p * 1)(page.ctypes.data); dsts = (ctypes.c_void_p * 1)(out.ctypes.data)\n"
            "slen, dcap = (ctypes.c_uint32 * 1)(100), (ctypes.c_uint32 * 1)(800)\n"
            "for k in range(2):\n"
            "    rc = lib.tyche_compress_host(3, 1, 1, srcs, slen, dsts, dcap, res)\n"
            "    print(rc, _lib.last_error())\n"
            "rc = lib.tyche_decompress_host(3, 1, srcs, slen, dsts, dcap, res)\n"
            "print(rc, _lib.last_error())\n"
            "print('current', lib.tyche_zstd_current_dict())\n"
            "rc = lib.tyche_compress_host(1, 1, 1, srcs, slen, dsts, dcap, res)\n"
            "print('lz4', rc)\n")
    for path, why in ((tmp_path / "missing.dict", "cannot read"), (empty, "is empty"), (big, "longer than"),
                      (structured, "structured")):
        env = dict(os.environ, TYCHE_ZSTD_DICT=str(path), PYTHONPATH=ROOT)
        env.pop("TYCHE_LZ4_DICT", None)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 5, p.stdout
        for ln in lines[:3]:
            assert ln.startswith("190 ") and "TYCHE_ZSTD_DICT" in ln and why in ln, ln
        assert lines[3] == "current None", lines[3]
        assert lines[4].startswith("lz4 ") and lines[4] != "lz4 190", lines[4]


def test_each_env_variable_fails_its_own_codec_only(tmp_path):
    """TYCHE_LZ4_DICT and TYCHE_ZSTD_DICT belong to one slot each: a missing file named in one of
    them makes tyche_compress_host fail for that variable's codec with that variable's text, and
    the same call for the other codec gets past its dictionary stage -- TYCHE_E_DEVICE on a machine
    without a GPU, success on one with it, never TYCHE_E_BAD_ARGS (a fresh child process each)."""
    code = ("import ctypes, sys, numpy as np\n"
            "from tyche_amd import _lib\n"
            "lib = _lib.load()\n"
            "page = np.zeros(100, np.uint8); out = np.zeros(800, np.uint8); res = (ctypes.c_int32 * 1)()\n"
            "srcs = (ctypes.c_void_p * 1)(page.ctypes.data); dsts = (ctypes.c_void_p * 1)(out.ctypes.data)\n"
            "slen, dcap = (ctypes.c_uint32 * 1)(100), (ctypes.c_uint32 * 1)(800)\n"
            "for codec in (int(sys.argv[1]), int(sys.argv[2])):\n"
            "    rc = lib.tyche_compress_host(codec, 1, 1, srcs, slen, dsts, dcap, res)\n"
            "    print(rc, _lib.last_error())\n")
    for var, own, other in (("TYCHE_LZ4_DICT", 1, ZSTD), ("TYCHE_ZSTD_DICT", ZSTD, 1)):
        env = {k: v for k, v in os.environ.items() if not k.startswith(("TYCHE_LZ4_DICT", "TYCHE_ZSTD_DICT"))}
        env.update({var: str(tmp_path / "missing.dict"), "PYTHONPATH": ROOT})
        p = subprocess.run([sys.executable, "-c", code, str(own), str(other)], env=env, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 2, p.stdout
        assert lines[0].startswith("190 ") and (var + ": cannot read") in lines[0], lines[0]
        assert lines[1].split()[0] in ("0", "199"), lines[1]   # (after a success the text is still the first call's)


def test_python_dictionary_still_raises_for_zlib():
    """dictionary= with the zlib codec is a ValueError before anything is launched; Dictionary is the
    codec-neutral name of the handle class and use_zstd_dict is exported."""
    import tyche_amd
    from tyche_amd import _lib, codec
    assert tyche_amd.Dictionary is codec.Lz4Dict and codec.Dictionary is codec.Lz4Dict
    assert tyche_amd.use_zstd_dict is codec.use_zstd_dict
    d = codec.Dictionary(b"abcdefgh" * 16)
    res = (ctypes.c_int32 * 1)()
    b = _dummy_batch(_lib, res, src_stride=100, src_length=100, dst_stride=800, dst_capacity=800)
    with pytest.raises(ValueError):
        codec._compress_call(_lib.ZLIB_COMPRESSOR_ID, 1, b, None, d)
    with pytest.raises(ValueError):
        codec._decompress_call(_lib.ZLIB_COMPRESSOR_ID, b, None, d)
    codec.use_zstd_dict(d)
    cur = _lib.load().tyche_zstd_current_dict()
    assert cur
    _lib.load().tyche_lz4_dict_destroy(cur)
    codec.use_zstd_dict(None)
    assert not _lib.load().tyche_zstd_current_dict()
    magic = codec.Dictionary(C.MAGIC + bytes(60))
    with pytest.raises(_lib.DeviceError) as e:
        codec.use_zstd_dict(magic)
    assert "190" in str(e.value) and "structured" in str(e.value)
    d.close()
    magic.close()


def test_seeded_cases_are_what_they_are_meant_to_be(oracle_mod):
    """The case builders: every pair fits the window, the longest page per dictionary is there, the
    tail page is the dictionary's tail."""
    O = oracle_mod
    assert all(d + l <= C.WINDOW and l <= 65535 for d, l in C.PAIRS)
    assert (1, 65535) in C.PAIRS and (4096, 65536 - 4096) in C.PAIRS and (32768, 32768) in C.PAIRS
    assert C.page_of(O, 4096, 64, "tail") == C.dict_of(O, 4096)[-64:]
    dic, page = C.used_case(4096)
    assert len(dic) == C.USED_D and page == dic[-4096:]
    for D, L in C.BOUNDARY:
        dic, page = C.boundary_case(O, D, L)
        assert len(dic) == D and len(page) == L and page[:64] == dic[:64]


def test_golden_file_against_the_reference(oracle_mod):
    """Where oracle/_ref is built: every recorded frame restores through ZSTD_decompress_usingDict,
    each boundary case really separates (the whole dictionary gives L, the dictionary minus its first
    byte an error, plain ZSTD_decompress an error), and the recorded verdicts and sizes are the
    library's.  Without it the file is only checked for its shape."""
    O = oracle_mod
    G = C.Golden()
    rt = G.rt_cases(O)
    bd = G.boundary_cases(O)
    dic, frames = C.malformed_cases(O)
    assert len(G.malformed_rv) == len(frames) == len(G.malformed_crc)
    assert len(G.ratio_ref) == len(C.RATIO_CELLS) and len(G.used_ref) == len(C.USED_LS)
    assert all(int(a) < int(b) for a, b in zip(G.ratio_ref, G.ratio_ref_plain))   # the issue's table: every cell gains
    R = C.ref_or_none(O)
    if R is None:
        return
    for D, L, k, d, page, f in rt:
        assert R.decompress(d, f, L) == (L, page), (D, L, k)
    for D, L, d, page, f in bd:
        assert R.decompress(d, f, L) == (L, page), (D, L)
        assert R.decompress(d[1:], f, L)[0] < 0, (D, L)
        assert R.decompress_plain(f, L)[0] < 0, (D, L)
    for i, (f, cap) in enumerate(frames):
        r, dec = R.decompress(dic, f, cap)
        assert r == int(G.malformed_rv[i]) and C.crc(dec) == int(G.malformed_crc[i]), i
    for L, want in zip(C.USED_LS, G.used_ref):
        d, page = C.used_case(L)
        assert len(R.compress(d, page)) == int(want)
    assert R.compress_rv(C.MAGIC + bytes(60), bytes(100))[0] < 0   # dictionary_corrupted: why the engine refuses them
