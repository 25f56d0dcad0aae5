"""CPU check of the high-compression LZ4 encoder's algorithm (tyche_amd/csrc/lz4_hc_core.h, the
per-wave code of lz4_encode_hc.hip, LZ4_HC=1) through its host emulator tools/lz4_hc_emul.cpp:
every stream is a valid LZ4 block that obeys the end rules and restores through
LZ4_decompress_safe (oracle.lz4_decompress; the reference's own where it is built); a capacity
below the stream's size gives 0, one at or above it the same bytes, and nothing outside the
capacity is written; and the mode closes at least half of the gap between the fast parse and
liblz4's LZ4_compress_HC level 3 on the bench pages.  The GPU tests (test_gpu_lz4_hc.py) hold the
kernel to the emulator's bytes."""
import ctypes

import numpy as np
import pytest

import lz4_hc_cases as C


@pytest.fixture(scope="module")
def emul():
    return C.load_emul()


def roundtrip(emul, O, page: bytes):
    r, stream = emul(page)
    assert r == len(stream) > 0, (len(page), r)
    C.check_stream(stream, page)
    assert C.restores(O, stream, page), len(page)
    return stream


@pytest.mark.parametrize("plen", C.PAGE_LENS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_page_kinds(emul, oracle_mod, kind, plen):
    pages = C.kind_pages(oracle_mod, kind, plen, n=2 if plen == 65535 else 4)
    for i in range(len(pages)):
        roundtrip(emul, oracle_mod, pages[i].tobytes())


@pytest.mark.parametrize("symbols", [2, 16, 256])
def test_ragged_small_pages(emul, oracle_mod, symbols):
    for page in C.ragged_pages(symbols):
        roundtrip(emul, oracle_mod, page)


def test_small_lengths(emul, oracle_mod):
    """Lengths around LZ4's 13-byte minimum, the 64-position block and one past 16 KiB; the empty
    page is the block 0x00 (result 1; 0 at capacity 0)."""
    for page in C.small_pages():
        stream = roundtrip(emul, oracle_mod, page)
        if len(page) < 13:
            assert len(stream) == len(page) + 1           # one literal-only sequence
    assert emul(b"") == (1, b"\x00")
    assert emul(b"", 0) == (0, b"")
    assert emul(b"", 1) == (1, b"\x00")


def test_a_match_is_found_across_blocks_and_inside_one(emul, oracle_mod):
    """A record repeated 3000 bytes later (the table's candidates) and a 3-byte period (the block's
    own lanes): both compress to a fraction, whichever lane of a block they start in."""
    rng = np.random.default_rng(5)
    for shift in range(0, 64, 7):
        rec = rng.integers(0, 256, 500, dtype=np.uint8).tobytes()
        page = bytes(rng.integers(0, 256, shift, dtype=np.uint8)) + rec + bytes(rng.integers(0, 256, 2500, dtype=np.uint8)) + rec + b"0123456789ab"
        assert len(roundtrip(emul, oracle_mod, page)) < len(page) - 450
        page = bytes(rng.integers(0, 256, shift, dtype=np.uint8)) + b"abc" * 400
        assert len(roundtrip(emul, oracle_mod, page)) < shift + 40


@pytest.mark.parametrize("which", [0, 1], ids=["compressible", "incompressible"])
def test_limited_output(emul, oracle_mod, which):
    page = C.limited_pages(oracle_mod)[which]
    bound = C.lz4_bound(len(page))
    full, stream = emul(page, bound)
    assert full == len(stream) > 0
    for cap in C.limited_caps(full, bound, 7 + which):
        r, got = emul(page, cap)                           # (asserts the guard bytes on either side)
        if cap < full:
            assert r == 0, (cap, full, r)
        else:
            assert r == full and got == stream, (cap, full, r)


def test_limited_output_small_pages(emul):
    """Every capacity from 0 to the bound for pages around the minimum length."""
    for page in C.small_pages():
        if len(page) > 130:
            continue
        full, stream = emul(page)
        for cap in range(C.lz4_bound(len(page)) + 1):
            r, got = emul(page, cap)
            assert (r, got) == ((full, stream) if cap >= full else (0, b"")), (len(page), cap)


def test_out_of_range_arguments(emul):
    buf = (ctypes.c_uint8 * 16)()
    assert emul.lib.lz4hc_emul_compress(buf, 65536, buf, 16) == -2 ** 31
    assert emul.lib.lz4hc_emul_compress(buf, -1, buf, 16) == -2 ** 31


@pytest.mark.parametrize("dist", C.RATIO_DISTS)
def test_ratio_closes_half_of_the_gap_to_hc3(emul, oracle_mod, dist):
    """Totals over oracle.pagegen(256, 16384, dist): F of the reference's fast parse
    (oracle.lz4_compress), H of liblz4's LZ4_compress_HC level 3 (tests/golden/lz4_hc_targets.json),
    M of this mode.  M <= F - (F - H) / 2: level 3 searches 4 candidates per position, so a
    bucketed parse that cannot get halfway there would be a tweak of the default parse, not an HC
    mode.  (Measured, profiles/lz4_hc_ratio.jsonl: the mode closes 0.67-1.00 of the gap.)"""
    O = oracle_mod
    pages = C.ratio_pages(O, dist)
    F = sum(len(O.lz4_compress(p.tobytes())) for p in pages)
    H = C.hc3_total(dist)
    M = 0
    for i, p in enumerate(pages):
        r, stream = emul(p.tobytes())
        if i % 32 == 0:
            assert C.restores(O, stream, p.tobytes())
        M += r
    print(f"dist {dist}: fast {F} hc3 {H} mode {M} bar {C.ratio_bar(F, H):.0f} closes {(F - M) / (F - H):.3f}")
    assert H < F
    assert M <= C.ratio_bar(F, H), (dist, F, H, M)


def test_exact_and_hc_contradict_before_any_launch(knobs):
    """LZ4_EXACT=1 with LZ4_HC=1: TYCHE_E_BAD_ARGS naming both from the device and the host compress
    call, refused before any device work (the pointers are never dereferenced, the output stays
    as it was)."""
    from tyche_amd import _lib
    lib = _lib.load()
    knobs(LZ4_EXACT=1, LZ4_HC=1)
    res = (ctypes.c_int32 * 1)()
    dummy = ctypes.addressof(res)
    b = _lib.Batch(count=1, src=dummy, src_stride=100, src_length=100, dst=dummy, dst_stride=200, dst_capacity=200,
                   results=dummy)
    assert lib.tyche_compress_batch(1, 1, ctypes.byref(b), None) == _lib.E_BAD_ARGS
    assert "LZ4_EXACT" in _lib.last_error() and "LZ4_HC" in _lib.last_error()
    page, out = np.zeros(100, np.uint8), np.zeros(200, np.uint8)
    srcs, dsts = (ctypes.c_void_p * 1)(page.ctypes.data), (ctypes.c_void_p * 1)(out.ctypes.data)
    slen, dcap = (ctypes.c_uint32 * 1)(100), (ctypes.c_uint32 * 1)(200)
    assert lib.tyche_compress_host(1, 1, 1, srcs, slen, dsts, dcap, res) == _lib.E_BAD_ARGS
    assert "LZ4_EXACT" in _lib.last_error() and "LZ4_HC" in _lib.last_error()
    assert not out.any()
