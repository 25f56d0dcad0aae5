"""The next-page prefetch of the page-loop kernels (TYCHE_NEXT_PAGE, lds_io.h) at its edges.

A page-loop kernel keeps the first W = kVec * kThreads * 16 bytes of its next page in registers and
loads the rest when it installs them.  The looping tests elsewhere use uniform 4 or 16 KiB pages and
never cross that window; here one launch per kernel path stages, at every alignment of the page's
first 16-byte vector (head = src & 15), lengths around 0, one vector, and the window's end: a page
that ends one vector short of it, with it, one byte past it, a vector past it and 1,000 bytes past it,
an empty page, and a page above the launch's declared maximum (INT32_MIN, slot untouched).

16 pages per CU: every one of these kernels stages at least W bytes per resident page in 160 KiB of
LDS, so at most 10 pages per CU are resident -- pages below the CU count are some workgroup's first
page (stage_in), pages from 10 x CUs on are claimed in the loop (fetch / install), and the kinds
cycle with a period coprime to 16, so every kind meets every alignment on both sides.

Encoded pages are restored by the oracle's decoders and, where oracle/_ref is built, by the
reference's own as well (C.restores), as in the other GPU suites: no case is skipped without it.
"""
import functools

import numpy as np
import pytest

import batch_contract_cases as C
import batch_layout as BL
from batch_contract_cases import LZ4, ZLIB, ZSTD, INT32_MIN
from test_gpu_batch_contract import lz4_decode_kernel, tc  # noqa: F401  (tc: the fixture)

pytestmark = pytest.mark.gpu

# path -> (codec, knobs, W).  W from the code: kPrefetchVec (16) x 64 lanes x 16 bytes for the one-wave
# kernels of lz4_encode.hip, lz4_encode_exact.hip, lz4_encode_hc.hip, zlib_deflate.hip and
# zstd_encode.hip; kSplitPrefetch (8) x 128 threads for the two-wave split; split_prefetch<kNW>() x
# kNW x 64 threads for the N-wave split -- 4 x 256 for the default four waves, 6 x 192 for three;
# kPrefetchVec (8) x 64 lanes in lz4_decode.hip.
ENCODE = {
    "lz4_default": (LZ4, dict(), 16384),
    "lz4_one_wave": (LZ4, dict(LZ4_ENC=1), 16384),
    "lz4_waves2": (LZ4, dict(LZ4_ENC_WAVES=2), 16384),
    "lz4_waves3": (LZ4, dict(LZ4_ENC_WAVES=3), 18432),
    "lz4_exact": (LZ4, dict(LZ4_EXACT=1), 16384),
    "lz4_hc": (LZ4, dict(LZ4_HC=1), 16384),
    "zlib": (ZLIB, dict(), 16384),
    # zstd: a launch of this size and page length parses on four waves per page (zstd_parse_split_kernel,
    # which stages without a prefetch); the two kernels with the prefetch are the one-kernel encode and
    # the one-wave parse
    "zstd": (ZSTD, dict(), 16384),
    "zstd_one_kernel": (ZSTD, dict(ZSTD_ENC_SPLIT=0), 16384),
    "zstd_one_wave_parse": (ZSTD, dict(ZSTD_PARSE_WAVES=1), 16384),
}
DECODE_KNOBS = dict(LZ4_SOLO_MAX=0, LZ4_JUMP_MAX=0, LZ4_LANE_MIN=-1)
DECODE_W = 8192
PAGES_PER_CU = 16
KINDS = 11   # coprime to 16
OVER = 10    # the kind above the declared maximum


def staged_length(kind, head, w):
    """The staged length of kind 0..10 for a page whose first vector starts `head` bytes in."""
    return [0, 1, 15, 16, 17, w - 16 - head, w - head, w - head + 1, w + 16, w + 1000, w + 1001][kind]


def page_count():
    import torch
    return PAGES_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count


def check_order(n, kinds, shifts):
    """Every (kind, head) as a first page and as a claimed page; hence an empty and an oversized
    page among the claimed ones, which are some wave's next page.  (The first pages cover the
    11 x 16 pairs on a device of at least 176 CUs -- an MI355X has 256; a smaller one fails here
    rather than run a weaker test.)"""
    ncu = n // PAGES_PER_CU
    first = {(kinds[i], shifts[i]) for i in range(ncu)}
    claimed = {(kinds[i], shifts[i]) for i in range(10 * ncu, n)}
    every = {(k, h) for k in range(KINDS) for h in range(16)}
    assert first == every and claimed == every, (len(first), len(claimed))


@functools.lru_cache(maxsize=None)
def encode_batch(n, w):
    kinds = [i % KINDS for i in range(n)]
    shifts = [i % 16 for i in range(n)]
    check_order(n, kinds, shifts)
    pages = [C.page(staged_length(kinds[i], shifts[i], w), i) for i in range(n)]
    return kinds, shifts, pages


@functools.lru_cache(maxsize=None)
def exact_streams(n, w):
    """The bytes LZ4 1.7.5's LZ4_compress_default gives: from the reference's own sources where
    oracle/_ref is built, else from the oracle's restatement of them (test_oracle.py holds the two
    to the same bytes) -- a checkout without the reference must still run every case."""
    O = C.oracle()
    enc = O.ref_lz4_compress if O.have_ref() else O.lz4_compress
    return [enc(p) for p in encode_batch(n, w)[2]]


@pytest.mark.parametrize("path", list(ENCODE))
def test_encode_across_the_window(tc, knobs, oracle_mod, path):
    codec, kn, w = ENCODE[path]
    n = page_count()
    kinds, shifts, pages = encode_batch(n, w)
    declared = w + 1000
    caps = [tc.compress_bound(len(p), codec) for p in pages]
    lay = BL.build(pages, caps, shifts, C.dst_shifts(n), ("random", 3))
    knobs(**kn)
    rv, out, src = C.device_compress(tc, lay, codec, max_src_length=declared)
    BL.check(out, src, lay)
    got = BL.outputs(out, rv, lay)
    want = exact_streams(n, w) if path == "lz4_exact" else None
    for i, p in enumerate(pages):
        where = (path, i, kinds[i], shifts[i], len(p), int(rv[i]))
        if kinds[i] == OVER:
            a = int(lay.dst_offsets[i])
            assert rv[i] == INT32_MIN and (out[a:a + caps[i]] == lay.fill).all(), where
            continue
        assert rv[i] > 0, where
        assert C.restores(codec, got[i], p), where
        if want is not None:
            assert got[i] == want[i], where


def literal_stream(target, seed):
    """(stream, page): an LZ4 block of exactly `target` bytes over random bytes -- one literal run
    (token, length bytes, literals), behind a first sequence of 4 or 5 literals and a 4-byte match
    where a lone run cannot have that size (its length bytes skip one size in 255)."""
    rng = np.random.default_rng(seed)

    def run_len(k):   # a last sequence of k literals
        return 1 + (0 if k < 15 else (k - 15) // 255 + 1) + k

    for first in (0, 4, 5):
        front = first + 3 if first else 0            # token, literals, offset
        rest = target - front
        k = rest - 1
        while k >= 0 and run_len(k) > rest:
            k -= 1
        if k < 0 or run_len(k) != rest:
            continue
        body = rng.integers(0, 256, first + k, dtype=np.uint8).tobytes()
        ext = b"" if k < 15 else b"\xff" * ((k - 15) // 255) + bytes([(k - 15) % 255])
        run = bytes([min(k, 15) << 4]) + ext + body[first:]
        if not first:
            return run, body
        # the match: offset `first`, 4 bytes
        return bytes([first << 4]) + body[:first] + bytes([first, 0]) + run, body[:first] + body[:4] + body[first:]
    raise AssertionError(target)


@functools.lru_cache(maxsize=None)
def decode_batch(n, w):
    kinds = [i % KINDS for i in range(n)]
    shifts = [i % 16 for i in range(n)]
    check_order(n, kinds, shifts)
    streams, pages = [], []
    for i in range(n):
        t = staged_length(kinds[i], shifts[i], w)
        s, p = (b"", b"") if t == 0 else literal_stream(t, 5000 + i % 176)
        assert len(s) == t
        streams.append(s)
        pages.append(p)
    return kinds, shifts, streams, pages


def test_literal_stream_is_what_the_oracle_decodes(oracle_mod):
    for t in (1, 15, 16, 17, 270, 271, 272, 273, 8192 - 16, 8193, 9192, 9193):
        s, p = literal_stream(t, t)
        r, dec = oracle_mod.lz4_decompress(s, len(p))
        assert len(s) == t and r == len(p) and bytes(dec)[:r] == p, t


def test_decode_across_the_window(tc, knobs, oracle_mod):
    """The wave decoder stages the stream: incompressible pages, whose stream length is chosen."""
    n, w = page_count(), DECODE_W
    kinds, shifts, streams, pages = decode_batch(n, w)
    declared = w + 1000
    out_cap = max(len(p) for p in pages)
    assert lz4_decode_kernel(n, declared, out_cap, DECODE_KNOBS) == "wave"
    caps = [len(p) for p in pages]
    lay = BL.build(streams, caps, shifts, C.dst_shifts(n), ("random", 4))
    knobs(**DECODE_KNOBS)
    rv, out, src = C.device_decode(tc, lay, LZ4, max_src_length=declared, max_capacity=out_cap)
    BL.check(out, src, lay)
    got = BL.outputs(out, rv, lay)
    empty = oracle_mod.lz4_decompress(b"", 0)[0]   # a stream of no bytes: the oracle's verdict
    for i, p in enumerate(pages):
        where = (i, kinds[i], shifts[i], len(streams[i]), int(rv[i]))
        if kinds[i] == OVER:
            a = int(lay.dst_offsets[i])
            assert rv[i] == INT32_MIN and (out[a:a + caps[i]] == lay.fill).all(), where
        elif kinds[i] == 0:
            assert C.verdict_matches(LZ4, int(rv[i]), empty), where
        else:
            assert rv[i] == len(p) and got[i] == p, where
