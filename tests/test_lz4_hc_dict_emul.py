"""CPU check of the high-compression LZ4 dictionary encoder's algorithm (LZ4_HC_DICT=1:
tyche_amd/csrc/lz4_hc_core.h's seed_window and encode_window, the per-wave code of
lz4_encode_hc_dict.hip) through its host emulator tools/lz4_hc_dict_emul.cpp: every stream is a
valid LZ4 block whose offsets stay within the dictionary bytes the encoder sees, obeys the end
rules on the page and restores through LZ4_decompress_safe_usingDict (the reference's where it is
built, a plain Python decode otherwise); a dictionary below 64 bytes gives the plain LZ4_HC=1
stream; a capacity below the stream's size gives 0, one at or above it the same bytes, and nothing
outside the capacity is written; and on 4 KiB pages with a 4 KiB dictionary the mode beats both the
default dictionary encoder and plain HC and closes at least half of the gap between liblz4's fast
and HC dictionary modes.  The GPU tests (test_gpu_lz4_hc_dict.py) hold the kernel to the
emulator's bytes.

LZ4_HC_DICT_EMUL_RECORD=<file> records every emulator call of a run for the stand-alone sanitizer
program (tools/lz4_hc_dict_emul.cpp with -DLZ4_HC_DICT_EMUL_MAIN), which replays them."""
import ctypes

import numpy as np
import pytest

import lz4_dict_cases as DC
import lz4_hc_cases as HC
import lz4_hc_dict_cases as C
from test_lz4_dict_emul import emul as dict_emul   # noqa: F401  (fixture: the default dictionary encoder's emulator)


@pytest.fixture(scope="module")
def emul():
    return C.load_emul()


@pytest.fixture(scope="module")
def plain():
    return HC.load_emul()


@pytest.fixture(scope="module")
def ref(oracle_mod):
    return DC.ref_or_none(oracle_mod)


@pytest.fixture(scope="module")
def streams(emul, oracle_mod):
    """(D, L, kind, dictionary, page, result, stream) of the whole matrix, encoded once."""
    out = []
    for D, L, kind, dic, page in C.cases(oracle_mod):
        r, stream = emul(dic, page)
        out.append((D, L, kind, dic, page, r, stream))
    return out


def test_the_matrix_is_the_one_asked_for():
    assert (32768, 32768) in C.PAIRS and (64, 65472) in C.PAIRS and len(set(C.PAIRS)) == len(C.PAIRS)
    assert all(d + l <= 65536 for d, l in C.PAIRS)
    assert {d for d, _ in C.PAIRS} == set(C.DS) and {l for _, l in C.PAIRS} == set(C.LS) | {65472}


def test_block_format_reach_and_restore(streams, ref):
    """Every (D, L, kind): the stream walks as an LZ4 block, every offset is within position + D', the
    last match starts at or before L - 12, the last 5 bytes are literals, and it restores."""
    reached = 0
    for D, L, kind, dic, page, r, stream in streams:
        assert r == len(stream) > 0, (D, L, kind, r)
        reach = C.check_stream(stream, dic, page)
        assert reach <= C.seen(D), (D, L, kind, reach)
        reached += reach > 0
        assert C.restores(ref, dic, stream, page), (D, L, kind)
        if L == 0:
            assert stream == b"\x00"
        elif L < 13:
            assert len(stream) == L + 1                   # one literal-only sequence
    assert reached > len(streams) // 3                    # (the dictionary is used: not a plain encoder in disguise)


def test_the_python_decode_restores_too(streams):
    """The decode that stands in where the reference library is not built, on every seventh case (with
    the library built, the test above has held the same streams to the reference)."""
    for D, L, kind, dic, page, r, stream in streams[::7]:
        assert C.py_decode(dic, stream, len(page)) == page, (D, L, kind)   # (a pagegen kind's page ends at 32 KiB)


def test_a_dictionary_the_encoder_cannot_see_gives_the_plain_stream(streams, plain):
    """D < 64: D' = 0, and the stream is the plain LZ4_HC=1 stream of the page, byte for byte."""
    n = 0
    for D, L, kind, dic, page, r, stream in streams:
        if D < 64:
            assert (r, stream) == plain(page), (D, L, kind)
            n += 1
    assert n >= 2 * 9 * len(DC.KINDS)


def test_random_pages_are_one_literal_run(streams):
    """Kind random: no match exists, so the stream is one literal run.  A match needs two equal 4-byte
    sequences in the window; uniform bytes have one by chance in some of the 16 KiB and larger cases
    (a window of n bytes: about n^2 / 2^33 of them), which is decided here from the input alone: there the stream may hold
    that chance match and is only held to being no longer than the literal run, with no match above
    7 bytes."""
    runs = chance = 0
    for D, L, kind, dic, page, r, stream in streams:
        if kind != "random":
            continue
        run = L
        want = bytes([min(run, 15) << 4]) + (b"\xff" * ((run - 15) // 255) + bytes([(run - 15) % 255]) if run >= 15 else b"") + page
        a = np.frombuffer(dic[len(dic) - C.seen(D):] + page, np.uint8).astype(np.uint32)
        grams = a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24) if len(a) >= 4 else a[:0]
        if len(np.unique(grams)) == len(grams):
            assert stream == want, (D, L)
            runs += 1
        else:
            assert len(stream) <= len(want) and all(ml <= 7 for _, _, ml in DC.walk(stream)), (D, L)
            chance += 1
    assert runs >= 40 and runs > 2 * chance, (runs, chance)       # (the lengths up to 4095: all but certainly runs)


def test_a_run_across_the_seam_finds_its_source(emul, oracle_mod):
    """seam1 .. seam7: the page continues a period that starts in the dictionary's last bytes, so its
    first sequence is a match at the page's first byte with that period as offset."""
    for p in range(1, 8):
        kind = f"seam{p}"
        dic, page = DC.dict_of(oracle_mod, 4096, kind), DC.page_of(oracle_mod, 4096, 4096, kind)
        r, stream = emul(dic, page)
        pos, off, ml = DC.walk(stream)[0]
        assert pos == 0 and ml >= 200 and (off % p == 0 or p % off == 0), (p, pos, off, ml)


@pytest.mark.parametrize("D,L,kind", [(4096, 4096, "dist0"), (4096, 4096, "random"), (1000, 4095, "seam3"), (64, 65, "tail"),
                                      (63, 4095, "dist1"), (32768, 13, "first")])
def test_limited_output(emul, oracle_mod, D, L, kind):
    dic, page = DC.dict_of(oracle_mod, D, kind), DC.page_of(oracle_mod, D, L, kind)
    bound = C.lz4_bound(L)
    full, stream = emul(dic, page, bound)
    assert full == len(stream) > 0
    for cap in HC.limited_caps(full, bound, 7 + D % 5):
        r, got = emul(dic, page, cap)                      # (asserts the guard bytes on either side)
        if cap < full:
            assert r == 0, (cap, full, r)
        else:
            assert r == full and got == stream, (cap, full, r)


def test_empty_page_and_out_of_range_arguments(emul):
    dic = bytes(range(256)) * 4
    assert emul(dic, b"") == (1, b"\x00")
    assert emul(dic, b"", 0) == (0, b"")
    assert emul(dic, b"", 1) == (1, b"\x00")
    buf = (ctypes.c_uint8 * 16)()
    f = emul.lib.lz4hc_dict_emul_compress
    assert f(buf, 4096, buf, 65536 - 4096 + 1, buf, 16) == -2 ** 31
    assert f(buf, 32769, buf, 1, buf, 16) == -2 ** 31
    assert f(buf, 16, buf, -1, buf, 16) == -2 ** 31


@pytest.mark.parametrize("dist", HC.RATIO_DISTS)
def test_ratio(emul, plain, dict_emul, oracle_mod, ref, dist):  # noqa: F811
    """Totals over 48 pages of 4 KiB with one more page's 4 KiB as dictionary: M of this mode is
    strictly below the default dictionary encoder's total and the plain HC encoder's, and
    M <= F - (F - H) / 2 with F of liblz4's fast dictionary mode and H of its HC dictionary mode at
    level 3 (tests/golden/lz4_hc_dict_targets.json): lz4_hc_cases.ratio_bar, the rule the plain mode
    is held to.  (Measured: the mode closes 0.74 / 0.74 / 0.98 / 0.66 of the gap on distributions
    0 / 1 / 2 / 5, profiles/lz4_hc_dict_ratio.jsonl.)"""
    O = oracle_mod
    t = C.targets()
    dic, pages = C.ratio_inputs(O, dist)
    F, H = int(t["F"][str(dist)]), int(t["H"][str(dist)])
    M = Dd = P = 0
    for i, p in enumerate(pages):
        b = p.tobytes()
        r, stream = emul(dic, b)
        if i % 8 == 0:
            C.check_stream(stream, dic, b)
            assert C.restores(ref, dic, stream, b)
        M += r
        rd, _ = dict_emul.enc(dic, b, C.lz4_bound(len(b)))
        assert rd > 0
        Dd += rd
        P += plain(b)[0]
    print(f"dist {dist}: liblz4 fast dict {F} hc dict {H} mode {M} default dict {Dd} plain hc {P} "
          f"bar {HC.ratio_bar(F, H):.0f} closes {(F - M) / (F - H):.3f}")
    assert H < F
    assert M < Dd, (dist, M, Dd)
    assert M < P, (dist, M, P)
    assert M <= HC.ratio_bar(F, H), (dist, F, H, M)
