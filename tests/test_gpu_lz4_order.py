"""GPU checks of the ordered page walk of the chunked lane-per-page LZ4 decoder
(tyche_amd/csrc/lz4_decode_lc.hip walking the order of page_order.hip): with LZ4_LC_ORDER=1 every
batch gives the results and the bytes it gives under the stride walk (LZ4_LC_ORDER=0), on the
checked layout of batch_layout.py (guard bytes around every output slot, results prefilled with a
sentinel); the device's order array is the host emulator's; and batches with nothing to order keep
the stride walk.  Every test forces the decoder on small batches and caps its grid at two waves
(LZ4_LANE_MIN=0, LZ4_LC_GRID=2: 128 pages per generation), so a few hundred pages are several
generations."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import batch_contract_cases as C
import batch_layout as BL
from batch_contract_cases import INT32_MIN, LZ4
from conftest import load_golden, unpack
from test_page_order_emul import Emul

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = 0x5A5A5A5A   # what device_decode prefills the results with
WINDOWS = [0, 64, 256]
G = 2 * 64              # pages per generation under LZ4_LC_GRID=2


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return codec


@pytest.fixture(scope="module")
def emul():
    return Emul()


@pytest.fixture
def lc(knobs):
    """the decoder under test on every batch size, two waves to a launch; lc(order, window) sets the walk"""
    knobs(LZ4_LC=1, LZ4_LANE_MIN=0, LZ4_LC_GRID=2)

    def walk(order, window=0):
        knobs(LZ4_LC_ORDER=order, LZ4_LC_ORDER_WINDOW=window)
    return walk


def ordered_launches():
    from tyche_amd import _lib
    f = _lib.load().tyche_debug_lz4_lc_ordered_launches
    f.restype = ctypes.c_ulonglong
    f.argtypes = []
    return int(f())


def device_order(lengths, in_cap, window):
    """tyche_debug_lz4_page_order over a batch that has only lengths: the ordering pass alone"""
    from tyche_amd import _lib
    f = _lib.load().tyche_debug_lz4_page_order
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(_lib.Batch), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    d_len = torch.from_numpy(np.ascontiguousarray(lengths, np.int32)).to(DEV)
    out = np.full(len(lengths), 0xFFFFFFFF, np.uint32)
    b = _lib.Batch(count=len(lengths), src_lengths=d_len.data_ptr())
    r = f(ctypes.byref(b), in_cap, window, out.ctypes.data)
    assert r == 0, r
    return out


@functools.lru_cache(maxsize=None)
def mixed_pages(n, plen=4096):
    """n pages of plen bytes of every generator distribution, interleaved, and their oracle streams"""
    O = C.oracle()
    per = (n + 5) // 6
    kinds = [O.pagegen(per, plen, seed=20170303 + d, first=0, dist=d) for d in range(6)]
    pages = [kinds[i % 6][i // 6].tobytes() for i in range(n)]
    return pages, [O.lz4_compress(p) for p in pages]


def decode(tc, lay, **kw):
    rv, out, src = C.device_decode(tc, lay, LZ4, **kw)
    BL.check(out, src, lay)   # no byte outside a slot, the source untouched
    return rv, out


def check_round_trip(tc, lc, pages, streams, window, shift=0):
    lay = BL.build(streams, [len(p) for p in pages], shift, 0, "zero")
    lc(0)
    before = ordered_launches()
    rv0, out0 = decode(tc, lay)
    assert ordered_launches() == before
    lc(1, window)
    rv1, out1 = decode(tc, lay)
    assert ordered_launches() == before + 1, "the ordered walk did not run"
    assert not bool((rv1 == SENTINEL).any()), "a page was skipped"
    assert np.array_equal(rv1, rv0)
    assert np.array_equal(rv1, np.array([len(p) for p in pages], np.int32))
    got = BL.outputs(out1, rv1, lay)
    for i, p in enumerate(pages):
        assert got[i] == p, i
    assert np.array_equal(out1, out0)


@pytest.mark.parametrize("window", WINDOWS)
def test_same_results_with_the_order_on_and_off(tc, lc, window):
    pages, streams = mixed_pages(1000)
    assert len(set(len(s) for s in streams)) > 100, "per-page lengths"
    check_round_trip(tc, lc, pages, streams, window)


@pytest.mark.parametrize("count", [300, 450])
@pytest.mark.parametrize("window", WINDOWS)
def test_partial_last_generation(tc, lc, count, window):
    """300 pages: two full generations and 44 pages of a third (an even, forward one); 450: three and
    66 pages of a fourth, a reversed one -- its pages are on the high lanes of the last wave and the
    low waves' lanes have none.  No page is skipped, none lands in another page's slot."""
    assert 2 * G < 300 < 3 * G < 450 < 4 * G
    pages, streams = mixed_pages(1000)
    check_round_trip(tc, lc, pages[:count], streams[:count], window, shift=3)


def test_rejected_and_malformed_pages(tc, lc, oracle_mod):
    """Pages the decoder answers without decoding (empty stream, empty capacity, a stream above the
    declared maximum, a capacity above the declared maximum) and the malformed fixtures, scattered
    among good pages: the return values of the stride walk, exactly; good pages whole; a page above
    a declared maximum leaves its slot untouched."""
    g = load_golden("lz4_malformed.npz")
    bad = [(unpack(g["comp"], g["comp_off"], g["comp_len"], i), int(g["cap"][i])) for i in range(len(g["cap"]))]
    pages, streams = mixed_pages(1000)
    max_src = max(len(s) for s in streams if len(s) < 4000)
    max_cap = 4096
    bad = [(s, c) for s, c in bad if len(s) <= max_src and c <= max_cap]   # the fixtures within the declared maxima
    assert len(bad) >= 40
    inputs, caps, want = [], [], []
    rng = np.random.default_rng(17)
    nbad = 0
    for i in range(600):
        k = i % 9
        if k == 2 and nbad < len(bad):
            inputs.append(bad[nbad][0])
            caps.append(bad[nbad][1])
            want.append(None)
            nbad += 1
        elif k == 2:
            inputs.append(b"")          # an empty stream
            caps.append(4096)
            want.append(None)
        elif k == 4:
            inputs.append(streams[i])
            caps.append(0 if i % 2 else 4096 + 16 * int(rng.integers(1, 9)))   # no capacity | above the declared maximum
            want.append(None)
        elif k == 7 and len(streams[i]) < 4000:
            inputs.append(streams[i] + bytes(4200 - len(streams[i])))          # a stream above the declared maximum
            caps.append(4096)
            want.append(None)
        else:
            inputs.append(streams[i])
            caps.append(4096)
            want.append(pages[i] if len(streams[i]) <= max_src else None)
    lay = BL.build(inputs, caps, 5, 0, ("random", 4))
    lc(0)
    rv0, out0 = decode(tc, lay, max_src_length=max_src, max_capacity=max_cap)
    assert int((rv0 == INT32_MIN).sum()) > 50 and int((rv0 < 0).sum()) > 100 and int((rv0 == 4096).sum()) > 250
    for i in range(600):   # the stride walk itself against the oracle
        if len(inputs[i]) <= max_src and caps[i] <= max_cap:
            assert rv0[i] == oracle_mod.lz4_decompress(inputs[i], caps[i])[0], i
        else:
            assert rv0[i] == INT32_MIN, i
    for window in WINDOWS:
        lc(1, window)
        before = ordered_launches()
        rv1, out1 = decode(tc, lay, max_src_length=max_src, max_capacity=max_cap)
        assert ordered_launches() == before + 1
        assert np.array_equal(rv1, rv0), np.flatnonzero(rv1 != rv0)[:10]
        got = BL.outputs(out1, rv1, lay)
        for i in range(600):
            a = int(lay.dst_offsets[i])
            if want[i] is not None:
                assert got[i] == want[i], i
            if rv1[i] == INT32_MIN:
                assert bool((out1[a:a + caps[i]] == lay.fill).all()), i


def test_the_stride_walk_is_kept(tc, lc):
    """Nothing to order: a batch with one length for all pages, and a batch of a single generation
    (64 pages; also 255, one short of two generations), take the stride walk whatever the knob says."""
    lc(1, 0)
    pages = tc.pagegen(600, 4096, dist=0, device=DEV)
    comp, clen = tc.compress_pages(pages)
    # one length for all: the same stream in every slot, no src_lengths in the batch
    from tyche_amd import _lib
    n, L = 600, int(clen[0])
    slots = comp[0:1].repeat(n, 1).contiguous()
    out = torch.full((n, 4096), 0xAB, dtype=torch.uint8, device=DEV)
    rv = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    b = _lib.Batch(count=n, src=slots.data_ptr(), src_stride=slots.shape[1], src_length=L, max_src_length=L,
                   dst=out.data_ptr(), dst_stride=4096, dst_capacity=4096, results=rv.data_ptr())
    before = ordered_launches()
    _lib.check(_lib.load().tyche_decompress_batch(LZ4, ctypes.byref(b), 0), "tyche_decompress_batch")
    torch.cuda.synchronize()
    assert ordered_launches() == before
    assert bool((rv == 4096).all()) and bool((out == pages[0:1]).all())
    for count in (64, 2 * G - 1):
        out, rv = tc.decompress_pages(comp[:count], clen[:count], 4096)
        torch.cuda.synchronize()
        assert ordered_launches() == before, count
        assert bool((rv == 4096).all()) and torch.equal(out, pages[:count])
    out, rv = tc.decompress_pages(comp[:2 * G], clen[:2 * G], 4096)   # two generations: ordered
    torch.cuda.synchronize()
    assert ordered_launches() == before + 1
    assert bool((rv == 4096).all()) and torch.equal(out, pages[:2 * G])


@pytest.mark.parametrize("window", WINDOWS + [1000, 5000])
def test_device_order_is_the_emulators(tc, lc, emul, window):
    _, streams = mixed_pages(1000)
    lengths = np.array([len(s) for s in streams], np.uint32)
    in_cap = int(lengths.max())
    got = device_order(lengths, in_cap, window)
    assert np.array_equal(got, emul.order(lengths, in_cap, window))


def test_device_order_across_tiles(tc, lc, emul):
    """more pages than one tile of the ordering pass holds, in windows of several tiles and of a
    count that is no multiple of the tile; lengths at and beyond the bins' ends"""
    rng = np.random.default_rng(23)
    n, in_cap = 3 * emul.TILE + 77, 16464
    lengths = rng.integers(0, in_cap + 300, n).astype(np.uint32)
    lengths[::97] = 0
    for window in (0, emul.TILE + 1, 2 * emul.TILE, 64):
        assert np.array_equal(device_order(lengths, in_cap, window), emul.order(lengths, in_cap, window)), window


def test_offset_layout(tc, lc):
    """the packed store's layout (tyche_pack_batch: src_offsets and src_lengths into one arena) decodes the same"""
    pages = torch.cat([tc.pagegen(100, 4096, dist=d, device=DEV) for d in range(6)])
    pages = pages[torch.randperm(600, generator=torch.Generator().manual_seed(5)).to(DEV)].contiguous()
    arena = torch.empty(600 * 4200, dtype=torch.uint8, device=DEV)
    offsets, lengths, _ = tc.compress_pages_packed(pages, arena)
    res = {}
    for order in (0, 1):
        lc(order, 256)
        before = ordered_launches()
        out = torch.full((600, 4096), 0xAB, dtype=torch.uint8, device=DEV)
        rv = torch.full((600,), SENTINEL, dtype=torch.int32, device=DEV)
        tc.decompress_packed(arena, offsets, lengths, 4096, out=out, rv=rv)
        torch.cuda.synchronize()
        assert ordered_launches() == before + order
        assert bool((rv == 4096).all()) and torch.equal(out, pages)
        res[order] = (out, rv)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
