"""GPU tests of the packed store (pack.hip through tyche_pack_batch and tyche_amd.codec): offsets,
lengths, state and every arena byte against the numpy specification (pack_cases.py) and against the
host emulator (tools/pack_emul.cpp); arenas start as 0xA5 between guard bytes and are compared whole
(the 4 GiB case compares a window), sources are compared by digest.  The tile size T, the pages per
scan workgroup S and the scan's fan-in F come from the code (the emulator exports them)."""
import hashlib

import numpy as np
import pytest
import torch

import pack_cases as P
from test_pack_emul import Emul

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 4096
LZ4, ZLIB, ZSTD = 1, 2, 3


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    assert _lib.load().tyche_device_ready() == 1, _lib.last_error()
    return codec


@pytest.fixture(scope="module")
def emul():
    return Emul()


def dev(a: np.ndarray) -> torch.Tensor:
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host_u64(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def digest(a: np.ndarray) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


class Store:
    """An arena of `capacity` bytes at a chosen misalignment between guard bytes, all 0xA5, and a state."""

    def __init__(self, capacity: int, state=(0, 0), misalign: int = 0):
        self.capacity, self.mis = capacity, misalign
        self.buf = torch.full((GUARD + misalign + capacity + GUARD,), P.FILL, dtype=torch.uint8, device=DEV)
        self.arena = self.buf[GUARD + misalign:GUARD + misalign + capacity]
        self.state = dev(np.asarray(state, np.uint64))

    def append(self, tc, case_or_src, results=None, src_offsets=None, align=16, max_length=0):
        """Appends a Case (its own align and max_length) or (src, results, src_offsets) already on the device."""
        if isinstance(case_or_src, P.Case):
            c = case_or_src
            src, results, src_offsets, align, max_length = dev(c.src), dev(c.results), dev(c.src_offsets), c.align, c.max_length
        else:
            src = case_or_src
        return tc.pack_pages((src, src_offsets), results, self.arena, self.state, align, max_length=max_length)

    def host(self):
        """-> (the arena's bytes, the state) after checking the guards."""
        b = self.buf.cpu().numpy()
        lo = GUARD + self.mis
        assert bool((b[:lo] == P.FILL).all()), "wrote in front of the arena"
        assert bool((b[lo + self.capacity:] == P.FILL).all()), "wrote behind the arena"
        s = host_u64(self.state)
        return b[lo:lo + self.capacity], (int(s[0]), int(s[1]))


def run_case(tc, case: P.Case, misalign=None):
    """One append of a Case into a fresh 0xA5 arena -> (offsets, lengths, state, arena bytes); the source is unchanged."""
    store = Store(case.capacity, case.state, case.skew if misalign is None else misalign)
    d_src = dev(case.src)
    offs, lens, _ = store.append(tc, d_src, dev(case.results), dev(case.src_offsets), case.align, case.max_length)
    torch.cuda.synchronize()
    assert digest(d_src.cpu().numpy()) == digest(case.src), "the source was written"
    arena, state = store.host()
    return host_u64(offs), lens.cpu().numpy().view(np.uint32), state, arena


def check_against(got, want, name):
    assert np.array_equal(got[0], want[0]), (name, "offsets")
    assert np.array_equal(got[1], want[1]), (name, "lengths")
    assert got[2] == want[2], (name, "state", got[2], want[2])
    same = np.array_equal(got[3], want[-1])
    assert same, (name, "arena bytes, first at", int(np.flatnonzero(got[3] != want[-1])[0]))


def check_spec(tc, case, misalign=None):
    want = P.expected(case)
    check_against(run_case(tc, case, misalign), (want[0], want[1], want[2], want[4]), case.name)


# ---------------------------------------------------------------- 1. edges
@pytest.mark.parametrize("align", P.ALIGNS)
def test_edges(tc, emul, align):
    """Lengths 0, 1, 15, 16, 17, T-1, T, T+1, 3T+5, each at every source misalignment; state[1]
    starting at 0, 1 and 13; results 0, -5, INT32_MIN and one above max_length between them; the
    arena itself at a different misalignment per case."""
    cases = [c for c in P.edge_cases(emul.T) if c.align == align]
    assert len(cases) == len(P.STARTS)
    for case in cases:
        check_spec(tc, case)


# ---------------------------------------------------------------- 2. scan levels
def test_scan_levels(tc, emul):
    """Counts 0, 1, S-1, S, S+1, 2S+3 and S*F+1 (the tile-sum scan's second round), pages of 0-3 bytes."""
    cases = P.scan_cases(emul.S, emul.F)
    assert [len(c.results) for c in cases] == P.scan_counts(emul.S, emul.F)
    for case in cases:
        check_spec(tc, case)


# ---------------------------------------------------------------- 3. skew
def test_one_large_stream_between_small_ones(tc):
    """A stream of tyche_compress_bound(LZ4, 4 MiB) bytes between 2,000 streams of 1-300 bytes."""
    rng = np.random.default_rng(77)
    big = tc.compress_bound(4 << 20, LZ4)
    small = rng.integers(1, 301, 2000).astype(np.int32)
    results = np.concatenate([small[:1000], [big], small[1000:]]).astype(np.int32)
    check_spec(tc, P.make_case("skew", results, 16, (0, 0), rng))


# ---------------------------------------------------------------- 4. 64-bit offsets
def test_offsets_beyond_4_gib(tc):
    """state = {2^32 - 100, 2^32 - 100}, an uninitialised arena of 2^32 + 64 KiB, eight pages
    straddling 2^32: the offsets, and the 128 KiB around 2^32 against the specification."""
    start, cap, half = 2 ** 32 - 100, 2 ** 32 + 65536, 65536
    rng = np.random.default_rng(78)
    results = np.asarray([30, 50, 19, 1, 16, 200, 4096 + 3, 17], np.int32)
    case = P.make_case("4gib", results, 16, (start, start), rng, capacity=cap)
    want_offs, want_lens, want_state, stored = P.pack_spec(results, 0, 16, case.state, cap)
    assert stored and int(want_offs[0]) < 2 ** 32 < int(want_offs[-1])
    arena = torch.empty((cap,), dtype=torch.uint8, device=DEV)
    arena[2 ** 32 - half:].fill_(P.FILL)
    state = dev(np.asarray(case.state, np.uint64))
    offs, lens, _ = tc.pack_pages((dev(case.src), dev(case.src_offsets)), dev(results), arena, state, 16)
    torch.cuda.synchronize()
    assert np.array_equal(host_u64(offs), want_offs) and np.array_equal(lens.cpu().numpy().view(np.uint32), want_lens)
    assert tuple(int(x) for x in host_u64(state)) == want_state
    window = np.full(2 * half, P.FILL, np.uint8)
    P.apply_spec(window, case.src, case.src_offsets, want_offs, want_lens, arena_origin=2 ** 32 - half)
    assert np.array_equal(arena[2 ** 32 - half:].cpu().numpy(), window)
    del arena


# ---------------------------------------------------------------- 5. refusal
def test_refusal_is_exact_and_sticky(tc, emul):
    refused, fits, _, _ = P.refusal_cases(emul.T)
    end = fits.capacity
    # capacity end - 1: nothing is written, state[0] stays, state[1] == end
    store = Store(refused.capacity, refused.state, misalign=3)
    store.append(tc, refused)
    # ... and a following one-byte append that would fit is refused as well (no sync in between)
    one = P.make_case("one", np.asarray([1], np.int32), 1, (0, 0), np.random.default_rng(5))
    offs, lens, _ = store.append(tc, one)
    torch.cuda.synchronize()
    arena, state = store.host()
    assert bool((arena == P.FILL).all()) and state == (9, end + 1)
    assert int(host_u64(offs)[0]) == end and int(lens[0]) == 1       # where it would have gone
    assert int(host_u64(offs)[0]) + 1 > state[0]                     # the invariant: not in the arena
    # capacity == end is stored
    check_spec(tc, fits, misalign=3)
    for case in P.refusal_cases(emul.T):
        check_spec(tc, case)


# ---------------------------------------------------------------- 6. chaining and compaction
def test_chained_appends_and_compaction(tc, emul):
    rng = np.random.default_rng(79)
    results, mis, max_length = P.edge_results(emul.T)
    parts = [results[:50], results[50:51], results[51:]]
    whole = P.make_case("whole", results, 16, (0, 0), rng, max_length=max_length, misalign=mis)
    d_src, d_res, d_so = dev(whole.src), dev(whole.results), dev(whole.src_offsets)
    one = Store(whole.capacity)
    o1, l1, _ = one.append(tc, d_src, d_res, d_so, 16, max_length)
    three = Store(whole.capacity)
    got = []
    a = 0
    for part in parts:                      # three appends on one stream, no sync between them
        b = a + len(part)
        got.append(three.append(tc, d_src, d_res[a:b], d_so[a:b], 16, max_length))
        a = b
    torch.cuda.synchronize()
    arena1, state1 = one.host()
    arena3, state3 = three.host()
    assert state1 == state3 and np.array_equal(arena1, arena3)
    assert torch.equal(torch.cat([g[0] for g in got]), o1) and torch.equal(torch.cat([g[1] for g in got]), l1)
    want = P.expected(whole)
    assert np.array_equal(arena1, want[4]) and state1 == want[2]
    # compaction: every other page of that arena into a second arena == packing those pages' slots directly
    keep = torch.arange(0, len(results), 2, device=DEV)
    second, direct = Store(whole.capacity, misalign=7), Store(whole.capacity, misalign=7)
    oc, lc, _ = second.append(tc, one.arena, l1[keep].contiguous(), o1[keep].contiguous(), 16)
    od, ld, _ = direct.append(tc, d_src, d_res[keep].contiguous(), d_so[keep].contiguous(), 16, max_length)
    torch.cuda.synchronize()
    assert torch.equal(oc, od) and torch.equal(lc, ld)
    (arena_c, state_c), (arena_d, state_d) = second.host(), direct.host()
    assert state_c == state_d and np.array_equal(arena_c, arena_d)
    assert state_c[0] < state1[0] and np.array_equal(one.host()[0], arena1)     # smaller; the old arena is unchanged


# ---------------------------------------------------------------- 7. input isolation
def test_bytes_around_the_streams_do_not_show(tc, emul):
    """The slot tails and the gaps between the slots as zeros, 0xFF and random bytes: identical arenas."""
    case = [c for c in P.edge_cases(emul.T) if c.align == 2][1]
    want = P.expected(case)
    rng = np.random.default_rng(80)
    for fill in (np.zeros(len(case.src), np.uint8), np.full(len(case.src), 0xFF, np.uint8),
                 rng.integers(0, 256, len(case.src), dtype=np.uint8)):
        src = np.where(case.stream_mask, case.src, fill).astype(np.uint8)
        other = P.Case(case.name, case.results, case.max_length, case.align, case.state, case.capacity, src,
                       case.src_offsets, case.stream_mask, case.skew)
        check_against(run_case(tc, other), (want[0], want[1], want[2], want[4]), "isolation")


# ---------------------------------------------------------------- 8. end to end
@pytest.mark.parametrize("page_len", [4096, 16384])
@pytest.mark.parametrize("codec_id", [LZ4, ZLIB, ZSTD])
def test_compress_pack_decompress(tc, codec_id, page_len):
    pages = tc.pagegen(1024, page_len, seed=31, dist=0, device=DEV)
    slots, clen = tc.compress_pages(pages, codec_id)
    want_out, want_rv = tc.decompress_pages(slots, clen, page_len, codec_id)
    for align in (1, 16):
        arena = torch.full((int(slots.numel()),), P.FILL, dtype=torch.uint8, device=DEV)
        offs, lens, state = tc.pack_pages(slots, clen, arena, align=align)
        out, rv = tc.decompress_packed(arena, offs, lens, page_len, codec_id)
        torch.cuda.synchronize()
        assert torch.equal(lens, clen) and int(state[0]) == int(state[1]) == int(offs[-1]) + int(lens[-1])
        if align == 1:
            assert int(state[0]) == int(clen.sum())
        assert torch.equal(rv, want_rv) and bool((rv == page_len).all())
        assert torch.equal(out, pages) and torch.equal(out, want_out)


def test_compress_pack_decompress_with_a_dictionary(tc):
    pages = tc.pagegen(1024, 4096, seed=32, dist=0, device=DEV)
    d = tc.Lz4Dict(pages[:8].cpu().numpy().tobytes()[:16384])
    slots, clen = tc.compress_pages(pages, dictionary=d)
    arena = torch.empty((int(slots.numel()),), dtype=torch.uint8, device=DEV)
    offs, lens, _ = tc.pack_pages(slots, clen, arena, align=1)
    out, rv = tc.decompress_packed(arena, offs, lens, 4096, dictionary=d)
    want_out, want_rv = tc.decompress_pages(slots, clen, 4096, dictionary=d)
    torch.cuda.synchronize()
    assert torch.equal(rv, want_rv) and torch.equal(out, pages) and torch.equal(out, want_out)


def test_chunked_compress_into_the_store(tc):
    """compress_pages_packed, 300 rows at a time over 1,000 rows == compress_pages + one pack_pages."""
    pages = tc.pagegen(1000, 16384, seed=33, dist=0, device=DEV)
    slots, clen = tc.compress_pages(pages)
    cap = int(slots.numel())
    a1 = torch.full((cap,), P.FILL, dtype=torch.uint8, device=DEV)
    a2 = torch.full((cap,), P.FILL, dtype=torch.uint8, device=DEV)
    o1, l1, s1 = tc.pack_pages(slots, clen, a1)
    o2, l2, s2 = tc.compress_pages_packed(pages, a2, chunk_pages=300)
    out, rv = tc.decompress_packed(a2, o2, l2, 16384)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and torch.equal(s1, s2) and torch.equal(a1, a2)
    assert torch.equal(out, pages) and bool((rv == 16384).all())


# ---------------------------------------------------------------- 9. the kernel against the emulator
def test_corpus_equals_the_emulator(tc, emul):
    for case in P.corpus(emul.T, emul.S, emul.F):
        want = emul.run(case)
        check_against(run_case(tc, case), (want[0], want[1], want[2], want[4]), case.name)
