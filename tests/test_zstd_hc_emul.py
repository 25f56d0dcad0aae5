"""CPU check of the high-compression zstd parse (tyche_amd/csrc/zstd_hc_core.h, the per-wave code
of zstd_parse_hc_kernel, ZSTD_HC=1) through its host emulator tools/zstd_hc_emul.cpp: the
sequences and the last literal run of every page rebuild it, with every offset inside what stands
before the match, every match at least 4 bytes and no more sequences than the sequence region
holds; matches are found across blocks, inside one block and at the repeat offset.  The GPU tests
(test_gpu_zstd_hc.py) hold the kernel's frames to the emulator's sequences and the mode to its
ratio."""
import ctypes

import numpy as np
import pytest

import zstd_hc_cases as C


@pytest.fixture(scope="module")
def emul():
    return C.load_emul()


def parsed(emul, page: bytes):
    seqs, last = emul(page)
    C.check_parse(seqs, last, page)
    return seqs, last


@pytest.mark.parametrize("plen", C.PAGE_LENS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_page_kinds(emul, oracle_mod, kind, plen):
    pages = C.kind_pages(oracle_mod, kind, plen, n=1 if plen == 65535 else 2)
    for i in range(len(pages)):
        parsed(emul, pages[i].tobytes())


@pytest.mark.parametrize("symbols", [2, 16, 256])
def test_ragged_small_pages(emul, symbols):
    for page in C.ragged_pages(symbols):
        parsed(emul, page)


def test_small_lengths(emul):
    """Lengths around the 4-byte minimum match, the 62-position block and its two lookahead lanes,
    two blocks, one past 16 KiB and the largest page; below 5 bytes there is nothing to match."""
    for page in C.small_pages():
        seqs, last = parsed(emul, page)
        if len(page) < 5:
            assert seqs == [] and last == len(page)
        if len(page) >= 61:
            assert seqs, len(page)           # 5 symbols: matches everywhere
    assert emul(b"") == ([], 0)


def test_matches_reach_the_end_of_the_page(emul):
    """LZ4's end rules are not zstd's: a match may end with the page's last byte, and the zero bytes
    behind the page are never counted into one."""
    for n in (5, 8, 62, 63, 64, 65, 300, 4096):
        seqs, last = parsed(emul, b"\0" * n)
        assert last == 0 and sum(ll + ml for ll, ml, _ in seqs) == n, (n, seqs, last)
    seqs, last = parsed(emul, b"abcdefgh" * 40)
    assert last == 0


def test_a_match_is_found_across_blocks_and_inside_one(emul):
    """A record repeated 3,000 bytes later (the rings' candidates) and a 3-byte period (the block's
    own lanes), whichever lane of a block they start in."""
    for name, shift, page in C.repeated_record_pages():
        seqs, last = parsed(emul, page)
        matched = sum(ml for _, ml, _ in seqs)
        if name == "record":
            assert any(ml >= 496 and off == 3000 for _, ml, off in seqs), (shift, seqs[-3:])
        else:
            assert matched >= 1200 - 3 - 4 and any(off == 3 for _, _, off in seqs), (shift, seqs)


def test_the_repeat_offset_is_preferred(emul):
    """A page of random bytes whose second half repeats the first at one offset with a byte changed
    every 40 to 90 bytes: random bytes match nowhere else, so every sequence that starts in the second
    half carries that offset, and there is one per stretch between two changed bytes."""
    page, half = C.repeat_offset_page()
    seqs, last = parsed(emul, page)
    pos, tail = 0, []
    for ll, ml, off in seqs:
        if pos + ll >= half:
            tail.append((ll, ml, off))
        pos += ll + ml
    assert len(tail) >= half // 90
    assert all(off == half for _, _, off in tail), [s for s in tail if s[2] != half][:5]


def test_out_of_range_arguments(emul):
    buf = (ctypes.c_uint8 * 16)()
    seqs = (ctypes.c_uint32 * 48)()
    last = ctypes.c_uint32(0)
    assert emul.lib.zstdhc_emul_parse(buf, 65536, seqs, 16, ctypes.byref(last)) == -2 ** 31
    assert emul.lib.zstdhc_emul_parse(buf, -1, seqs, 16, ctypes.byref(last)) == -2 ** 31
