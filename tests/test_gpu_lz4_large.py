"""GPU tests of LZ4 pages above 65,535 bytes, up to TYCHE_LZ4_MAX_PAGE (4 MiB), at every entry
point: the large-page kernels (tyche_amd/csrc/lz4_encode_large.hip, lz4_decode_large.hip) against
the oracle on the inputs of the CPU emulator tests (test_lz4_large_emul.py checks the same per-wave
code, lz4_large_core.h, without a GPU), page claiming, batches that mix sizes, the limits and their
errors, the host batch and Buffer paths with the restore queue, and the ratio against the
small-page encoder."""
import ctypes

import numpy as np
import pytest
import torch

from lz4_large_cases import (FULL_KINDS, KINDS, LENS, MAX_PAGE, crafted_streams, cuts, kind_pages, malformed_sources,
                             page_of, patched_streams)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILL = 0xAB
GUARD = 64
TOO_LARGE = -2 ** 31
LZ4, ZLIB, ZSTD = 1, 2, 3


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return codec


def _layout(sizes, misalign=True):
    """Offsets of items of the given sizes, item i at alignment i mod 16 from a 16-byte line, each
    followed by GUARD spare bytes; and the total."""
    offs, pos = np.zeros(len(sizes), np.int64), 0
    for i, n in enumerate(sizes):
        pos = (pos + 15) // 16 * 16 + (i % 16 if misalign else 0)
        offs[i] = pos
        pos += n + GUARD
    return offs, pos + 64


def ragged_decompress(tc, streams, caps, max_src=None, max_cap=None):
    """Decodes a list of streams with per-page capacities through the general batch API; sources and
    destinations at every alignment, destinations pre-filled.  Returns (results, outputs), having
    checked that nothing at or past a capacity was written."""
    n = len(streams)
    soffs, stotal = _layout([len(s) for s in streams])
    buf = np.zeros(stotal, np.uint8)
    for i, s in enumerate(streams):
        buf[soffs[i]:soffs[i] + len(s)] = np.frombuffer(s, np.uint8)
    ooffs, ototal = _layout(caps)
    d_out = torch.full((ototal,), FILL, dtype=torch.uint8, device=DEV)
    d_rv = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    tc.decompress_ragged(torch.from_numpy(buf).to(DEV), torch.from_numpy(soffs).to(DEV),
                         torch.tensor([len(s) for s in streams], dtype=torch.int32, device=DEV),
                         torch.tensor(caps, dtype=torch.int32, device=DEV), d_out, torch.from_numpy(ooffs).to(DEV), d_rv,
                         max_src_length=max_src or max(len(s) for s in streams), max_capacity=max_cap or max(caps))
    torch.cuda.synchronize()
    out, rv = d_out.cpu().numpy(), d_rv.cpu().numpy()
    for i in range(n):
        assert bool((out[ooffs[i] + caps[i]:ooffs[i] + caps[i] + GUARD] == FILL).all()), ("wrote past dst_capacity", i)
    return rv, [out[ooffs[i]:ooffs[i] + max(int(rv[i]), 0)].tobytes() for i in range(n)]


def ragged_compress(tc, pages, caps, max_src=None, compressor_id=LZ4):
    """Compresses a list of pages with per-page capacities through the general batch API; same
    layout and guard check.  Returns (results, streams)."""
    n = len(pages)
    soffs, stotal = _layout([len(p) for p in pages])
    buf = np.zeros(stotal, np.uint8)
    for i, p in enumerate(pages):
        buf[soffs[i]:soffs[i] + len(p)] = np.frombuffer(p, np.uint8)
    ooffs, ototal = _layout(caps)
    d_out = torch.full((ototal,), FILL, dtype=torch.uint8, device=DEV)
    d_rv = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    tc.compress_ragged(torch.from_numpy(buf).to(DEV), torch.from_numpy(soffs).to(DEV),
                       torch.tensor([len(p) for p in pages], dtype=torch.int32, device=DEV), d_out,
                       torch.from_numpy(ooffs).to(DEV), torch.tensor(caps, dtype=torch.int32, device=DEV), d_rv,
                       max_src_length=max_src if max_src is not None else max(len(p) for p in pages),
                       compressor_id=compressor_id)
    torch.cuda.synchronize()
    out, rv = d_out.cpu().numpy(), d_rv.cpu().numpy()
    for i in range(n):
        assert bool((out[ooffs[i] + caps[i]:ooffs[i] + caps[i] + GUARD] == FILL).all()), ("wrote past dst_capacity", i)
    return rv, [out[ooffs[i]:ooffs[i] + max(int(rv[i]), 0)].tobytes() for i in range(n)]


def check_stream(O, stream: bytes, page: bytes):
    """The stream is one LZ4 block that restores the page, within the bound."""
    assert 0 < len(stream) <= O.lz4_bound(len(page)), (len(page), len(stream))
    rv, back = O.lz4_decompress(stream, len(page))
    assert rv == len(page) and back == page, (len(page), rv)
    if O.have_ref():
        rv, back = O.ref_lz4_decompress(stream, len(page))
        assert rv == len(page) and back == page, (len(page), rv)


def rows_roundtrip(tc, O, host, sample=None):
    """compress_pages / decompress_pages on a (n, plen) array: every row comes back, and the rows
    in `sample` (all by default) also pass the oracle.  Returns the compressed lengths."""
    pages = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
    comp, clen = tc.compress_pages(pages)
    dec, rv = tc.decompress_pages(comp, clen, host.shape[1])
    torch.cuda.synchronize()
    lh = clen.cpu().numpy()
    assert bool((rv.cpu().numpy() == host.shape[1]).all()), rv.cpu().numpy()
    assert torch.equal(dec, pages)
    ch = comp.cpu().numpy()
    for i in (range(len(host)) if sample is None else sample):
        check_stream(O, ch[i, :lh[i]].tobytes(), host[i].tobytes())
    return lh


def decode_rows(tc, O, host):
    """The oracle's streams of the rows of a (n, plen) array through decompress_pages."""
    n, plen = host.shape
    streams = [O.lz4_compress(host[i].tobytes()) for i in range(n)]
    slot = tc.slot_size(plen)
    buf = np.zeros((n, slot), np.uint8)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = np.frombuffer(s, np.uint8)
    dec, rv = tc.decompress_pages(torch.from_numpy(buf).to(DEV),
                                  torch.tensor([len(s) for s in streams], dtype=torch.int32, device=DEV), plen)
    torch.cuda.synchronize()
    assert bool((rv.cpu().numpy() == plen).all()), rv.cpu().numpy()
    assert bool((dec.cpu().numpy() == host).all())


# ------------------------------------------------------------------ parity with the oracle

@pytest.mark.parametrize("plen", LENS)
@pytest.mark.parametrize("kind", KINDS)
def test_decode(tc, oracle_mod, kind, plen):
    decode_rows(tc, oracle_mod, kind_pages(oracle_mod, kind, plen, 4))


@pytest.mark.parametrize("plen", LENS)
@pytest.mark.parametrize("kind", KINDS)
def test_encode(tc, oracle_mod, kind, plen):
    rows_roundtrip(tc, oracle_mod, kind_pages(oracle_mod, kind, plen, 4))


@pytest.mark.parametrize("kind", FULL_KINDS)
def test_full_size(tc, oracle_mod, kind):
    host = kind_pages(oracle_mod, kind, MAX_PAGE, 2)
    decode_rows(tc, oracle_mod, host)
    rows_roundtrip(tc, oracle_mod, host)


def test_decode_crafted(tc, oracle_mod):
    cases = crafted_streams()
    streams, caps = [], []
    for name, s, size in cases:
        for cap in (size, size + 1, size + 100):
            streams.append(s)
            caps.append(cap)
    rv, outs = ragged_decompress(tc, streams, caps)
    for i, (s, cap) in enumerate(zip(streams, caps)):
        want = oracle_mod.lz4_decompress(s, cap)
        assert want[0] == cases[i // 3][2]
        assert (int(rv[i]), outs[i]) == want, (cases[i // 3][0], cap, int(rv[i]))


def test_decode_malformed(tc, oracle_mod):
    """Cut streams, patched streams and capacities off by one, all in one batch beside valid
    large streams: every result is the oracle's."""
    O = oracle_mod
    streams, caps, names = [], [], []
    for n, (name, s, size) in enumerate(malformed_sources(O)):
        for c in cuts(s, n):
            streams.append(s[:c])
            caps.append(size)
            names.append((name, "cut", c))
        for cap in (size, size - 1, size + 1, size - 11, size - 12, size // 2):
            streams.append(s)
            caps.append(cap)
            names.append((name, "cap", cap))
    for name, s, size in patched_streams(O):
        for cap in (size, size - 1, size + 1):
            streams.append(s)
            caps.append(cap)
            names.append((name, "patched", cap))
    # (every launch sized as the largest of them: the large-page decoder takes the whole batch)
    rv, outs = ragged_decompress(tc, streams, caps, max_src=O.lz4_bound(1 << 20), max_cap=1 << 20)
    for i, (s, cap) in enumerate(zip(streams, caps)):
        want = O.lz4_decompress(s, cap)
        assert int(rv[i]) == want[0], (names[i], int(rv[i]), want[0])
        # (a match of offset 0 copies bytes the reference leaves undefined: its size only)
        if want[0] > 0 and names[i][0] != "offset_zero_mid":
            assert outs[i] == want[1], names[i]


def compress_with_capacities(tc, pages, entries):
    """entries = [(page index, dst_capacity)]: one ragged batch in which every page is stored once
    and may be compressed at several capacities; each output slot is followed by GUARD pre-filled
    bytes, checked here.  Returns (results, streams)."""
    soffs, stotal = _layout([len(p) for p in pages])
    buf = np.zeros(stotal, np.uint8)
    for i, p in enumerate(pages):
        buf[soffs[i]:soffs[i] + len(p)] = np.frombuffer(p, np.uint8)
    caps = [c for _, c in entries]
    ooffs, ototal = _layout(caps)
    d_out = torch.full((ototal,), FILL, dtype=torch.uint8, device=DEV)
    d_rv = torch.full((len(entries),), -7, dtype=torch.int32, device=DEV)
    tc.compress_ragged(torch.from_numpy(buf).to(DEV), torch.from_numpy(soffs[[i for i, _ in entries]]).to(DEV),
                       torch.tensor([len(pages[i]) for i, _ in entries], dtype=torch.int32, device=DEV), d_out,
                       torch.from_numpy(ooffs).to(DEV), torch.tensor(caps, dtype=torch.int32, device=DEV), d_rv,
                       max_src_length=max(len(p) for p in pages))
    torch.cuda.synchronize()
    out, rv = d_out.cpu().numpy(), d_rv.cpu().numpy()
    for k, c in enumerate(caps):
        assert bool((out[ooffs[k] + c:ooffs[k] + c + GUARD] == FILL).all()), ("wrote past dst_capacity", entries[k])
    return rv, [out[ooffs[k]:ooffs[k] + max(int(rv[k]), 0)].tobytes() for k in range(len(entries))]


@pytest.mark.parametrize("plen", LENS)
def test_encode_capacities(tc, oracle_mod, plen):
    """Every kind, 4 pages each, in one ragged batch per step: dst_capacity at the size a page needs
    gives that size and the same bytes; at several values below it the result is 0; nothing at or
    past the capacity is written either way (an incompressible or literal-heavy page reaches the
    HBM-sourced literal copy with the capacity cutting it off)."""
    O = oracle_mod
    pages = [kind_pages(O, kind, plen, 4)[i].tobytes() for kind in KINDS for i in range(4)]
    rv, streams = compress_with_capacities(tc, pages, [(i, O.lz4_bound(plen)) for i in range(len(pages))])
    for i, (p, s) in enumerate(zip(pages, streams)):
        assert int(rv[i]) == len(s) and 0 < len(s) <= O.lz4_bound(plen), (i, int(rv[i]))
        back = O.lz4_decompress(s, plen)
        assert back[0] == plen and back[1] == p, (i, back[0])
    entries = []
    for i, s in enumerate(streams):
        r = len(s)
        entries += [(i, c) for c in sorted({r, r - 1, r - 7, r - r // 3, r // 2, 13, 1, 0}) if c >= 0]
    rv2, streams2 = compress_with_capacities(tc, pages, entries)
    for (i, cap), r, got in zip(entries, rv2, streams2):
        if cap == len(streams[i]):
            assert int(r) == cap and got == streams[i], (i, cap, int(r))
        else:
            assert int(r) == 0, (i, cap, int(r))


# ------------------------------------------------------------------ batches

def test_claiming(tc, oracle_mod):
    """More pages than resident workgroups: 1,200 pages of 66,000 bytes."""
    pages = tc.pagegen(1200, 69632, seed=77, dist=0)[:, :66000].contiguous()
    torch.cuda.synchronize()
    host = pages.cpu().numpy()
    lh = rows_roundtrip(tc, oracle_mod, host, sample=range(0, 1200, 75))
    assert 66000 * 1200 / float(lh.sum()) > 1.5


def test_mixed_ragged_batch(tc, oracle_mod):
    O = oracle_mod
    lens = (0, 100, 16384, 65535, 65536, 200000, 1048576)
    rng = np.random.default_rng(12)
    pages = [page_of(O, "dist0", 1 << 20)[:n] if n != 100 else rng.integers(0, 4, 100, dtype=np.uint8).tobytes()
             for n in lens]
    caps = [O.lz4_bound(n) for n in lens]
    rv, streams = ragged_compress(tc, pages, caps, max_src=max(lens))
    assert int(rv[0]) == 1 and streams[0] == b"\0"
    for p, s in zip(pages[1:], streams[1:]):
        check_stream(O, s, p)
    rv2, outs = ragged_decompress(tc, streams, list(lens), max_src=max(caps), max_cap=max(lens))
    assert [int(r) for r in rv2] == list(lens) and outs == pages
    # the pages of up to 65,535 bytes: the bytes of a batch that holds only them
    rv3, small = ragged_compress(tc, pages[:4], caps[:4], max_src=65535)
    assert small == streams[:4] and [int(r) for r in rv3] == [int(r) for r in rv[:4]]


# ------------------------------------------------------------------ limits

def test_limits(tc, oracle_mod):
    from tyche_amd import _lib
    O = oracle_mod
    pages = [page_of(O, "dist0", 100000)[:n] for n in (70000, 100000, 300)]
    caps = [O.lz4_bound(len(p)) for p in pages]
    with pytest.raises(_lib.DeviceError, match=f"code {_lib.E_BAD_ARGS}") as ei:
        ragged_compress(tc, pages, caps, max_src=MAX_PAGE + 1)
    assert str(MAX_PAGE) in str(ei.value)
    rv, streams = ragged_compress(tc, pages, caps, max_src=MAX_PAGE)      # the limit itself is legal
    for p, s in zip(pages, streams):
        check_stream(O, s, p)
    # a page above a legal declared maximum: INT32_MIN, the others unharmed
    rv, streams = ragged_compress(tc, pages, caps, max_src=80000)
    assert int(rv[1]) == TOO_LARGE
    check_stream(O, streams[0], pages[0])
    check_stream(O, streams[2], pages[2])
    # a host page above the limit
    lib = _lib.load()
    big = np.zeros(MAX_PAGE + 1, np.uint8)
    out = np.zeros(O.lz4_bound(MAX_PAGE + 1), np.uint8)
    res = np.zeros(1, np.int32)
    rc = lib.tyche_compress_host(LZ4, 1, 1, (ctypes.c_void_p * 1)(big.ctypes.data), (ctypes.c_uint32 * 1)(big.size),
                                 (ctypes.c_void_p * 1)(out.ctypes.data), (ctypes.c_uint32 * 1)(out.size),
                                 res.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == _lib.E_BAD_ARGS and str(MAX_PAGE) in _lib.last_error(), (rc, _lib.last_error())
    # a decode capacity above the limit: refused at the launch, as capacities beyond the decoders always were
    with pytest.raises(_lib.DeviceError, match=f"code {_lib.E_DEVICE}") as ei:
        ragged_decompress(tc, [streams[0]], [70000], max_cap=MAX_PAGE + 1)
    assert str(MAX_PAGE) in str(ei.value)
    rv, outs = ragged_decompress(tc, [streams[0]], [70000], max_cap=MAX_PAGE)
    assert int(rv[0]) == 70000 and outs[0] == pages[0]


@pytest.mark.parametrize("codec_id,name", [(ZLIB, "zlib"), (ZSTD, "zstd")])
def test_other_codecs_keep_their_limit(tc, oracle_mod, codec_id, name):
    from tyche_amd import _lib
    page = torch.from_numpy(kind_pages(oracle_mod, "dist0", 65536, 1)).to(DEV)
    with pytest.raises(_lib.DeviceError, match=f"code {_lib.E_BAD_ARGS}") as ei:
        tc.compress_pages(page, compressor_id=codec_id)
    assert f"{name} pages above 65535 bytes" in str(ei.value)
    comp, clen = tc.compress_pages(page[:, :65535].contiguous(), compressor_id=codec_id)   # 65,535 still works
    torch.cuda.synchronize()
    assert int(clen[0]) > 0


def test_exact_mode_stays_byu16(tc, oracle_mod, knobs):
    from tyche_amd import _lib
    host = kind_pages(oracle_mod, "dist0", 65536, 1)
    page = torch.from_numpy(host).to(DEV)
    knobs(LZ4_EXACT=1)
    with pytest.raises(_lib.DeviceError, match=f"code {_lib.E_BAD_ARGS}"):
        tc.compress_pages(page)
    _lib.clear_knob("LZ4_EXACT")
    rows_roundtrip(tc, oracle_mod, host)


# ------------------------------------------------------------------ host batches and Buffers

def _compressed_buffer(B, payload: bytes, data_length: int, id: int):
    buf = B.new_buffer(b"\0" * data_length, id=id)
    mem = B._libc.malloc(len(payload))
    ctypes.memmove(mem, payload, len(payload))
    B.swap_data(buf, mem)
    buf.contents.comp_length = len(payload)
    return buf


@pytest.mark.parametrize("plen", [65536, 300000])
def test_buffer_compress_decompress(tc, oracle_mod, plen):
    from tyche_amd import buffer as B
    page = page_of(oracle_mod, "dist0", plen)
    buf = B.new_buffer(page, id=7)
    rv, comp = B.buffer__compress(buf, LZ4, 1)
    assert rv == 0 and comp is not None, rv
    n = buf.contents.comp_length
    stream = ctypes.string_at(comp, n)
    check_stream(oracle_mod, stream, page)
    # (the stream ends where comp_length says: one byte less no longer decodes to the page)
    assert oracle_mod.lz4_decompress(stream[:-1], plen)[0] != plen
    B.swap_data(buf, comp)
    assert B.buffer__decompress(buf, LZ4) == 0
    assert buf.contents.comp_length == 0 and buf.contents.data_length == plen
    assert B.buffer_bytes(buf) == page
    B.destroy(buf)


def test_buffers_batch_mixed_sizes(tc, oracle_mod):
    from tyche_amd import buffer as B
    O = oracle_mod
    small = O.pagegen(8, 16384, seed=9, dist=0)
    pages = [small[i].tobytes() for i in range(8)] + [page_of(O, "dist1", 100000), page_of(O, "dist2", 500000)]
    bufs = [B.new_buffer(p, id=i) for i, p in enumerate(pages)]
    rc, st, outs = B.buffers_compress(bufs, LZ4)
    assert rc == 0 and st == [0] * len(bufs)
    for b, o, p in zip(bufs, outs, pages):
        check_stream(O, ctypes.string_at(o, b.contents.comp_length), p)
        B.swap_data(b, o)
    rc, st = B.buffers_decompress(bufs, LZ4)
    assert rc == 0 and st == [0] * len(bufs)
    for b, p in zip(bufs, pages):
        assert B.buffer_bytes(b) == p
        B.destroy(b)


def _host_decompress(streams, caps):
    """tyche_decompress_host on lists of streams and capacities: (rc, results, outputs)."""
    from tyche_amd import _lib
    lib = _lib.load()
    n = len(streams)
    sb = [np.frombuffer(s, np.uint8).copy() for s in streams]
    ob = [np.zeros(max(c, 1), np.uint8) for c in caps]
    vp = ctypes.c_void_p * n
    u32 = ctypes.c_uint32 * n
    res = np.full(n, -7, np.int32)
    rc = lib.tyche_decompress_host(LZ4, n, vp(*[a.ctypes.data for a in sb]), u32(*[len(s) for s in streams]),
                                   vp(*[a.ctypes.data for a in ob]), u32(*caps),
                                   res.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return rc, res, [ob[i][:max(int(res[i]), 0)].tobytes() for i in range(n)]


def test_host_batch_classes(tc, oracle_mod):
    """Many small pages beside a large one.  Through the Buffer batch call the classes go to the
    GPU separately and everything is restored.  A raw host batch that holds a large capacity beside
    more than 64 small ones is refused as such batches always were (TYCHE_E_DEVICE, the rule in the
    message; test_host_engine.py pins the refusal) and leaves the next call alone; up to 64 pass."""
    from tyche_amd import _lib, buffer as B
    O = oracle_mod
    small = O.pagegen(100, 16384, seed=10, dist=0)
    pages = [small[i].tobytes() for i in range(100)]
    pages.insert(50, page_of(O, "dist0", 300000))
    streams = [O.lz4_compress(p) for p in pages]
    bufs = [_compressed_buffer(B, s, len(p), i) for i, (s, p) in enumerate(zip(streams, pages))]
    rc, st = B.buffers_decompress(bufs, LZ4)
    assert rc == 0 and st == [0] * len(bufs)
    for b, p in zip(bufs, pages):
        assert B.buffer_bytes(b) == p
        B.destroy(b)
    caps = [len(p) for p in pages]
    rc, res, outs = _host_decompress(streams, caps)
    assert rc == _lib.E_DEVICE, (rc, _lib.last_error())
    assert "call of their own" in _lib.last_error()
    rc, res, outs = _host_decompress(streams[18:83], caps[18:83])       # 64 small pages and the large one
    assert rc == 0 and [int(r) for r in res] == caps[18:83] and outs == pages[18:83]


def test_buffer_decompress_of_a_reference_block(tc, oracle_mod):
    """What a cache written by the reference holds: a byU32 block of a 300,000-byte page."""
    from tyche_amd import buffer as B
    page = page_of(oracle_mod, "dist0", 300000)
    buf = _compressed_buffer(B, oracle_mod.lz4_compress(page), len(page), 3)
    assert B.buffer__decompress(buf, LZ4) == 0
    assert B.buffer_bytes(buf) == page
    B.destroy(buf)


def test_restore_queue_large_page(tc, oracle_mod):
    from tyche_amd import _lib, buffer as B
    lib = _lib.load()
    page = page_of(oracle_mod, "dist3", 300000)
    buf = _compressed_buffer(B, oracle_mod.lz4_compress(page), len(page), 4)
    assert lib.tyche_restore_queue_start(16, 200) == 0
    try:
        st = lib.tyche_buffer_restore(buf, LZ4)
    finally:
        lib.tyche_restore_queue_stop()
    assert st == 0 and B.buffer_bytes(buf) == page
    B.destroy(buf)


# ------------------------------------------------------------------ ratio

def test_ratio_against_small_pages(tc):
    """16 pages of 262,144 bytes per bench distribution: as large pages they compress to at most
    1.005x the bytes the same tensor takes as 32 KiB pages through the small-page encoder (0.5 %:
    the width of the project's ratio pins).  A large page sees 65,535 bytes of history everywhere,
    a 32 KiB page on average a quarter of that."""
    large = small = 0
    for d in range(6):
        pages = tc.pagegen(16, 262144, seed=31 + d, dist=d)
        _, cl = tc.compress_pages(pages)
        _, cs = tc.compress_pages(pages.view(-1, 32768))
        torch.cuda.synchronize()
        assert int(cl.min()) > 0 and int(cs.min()) > 0
        print(f"dist{d}: large {int(cl.sum())} small {int(cs.sum())} ({int(cl.sum()) / int(cs.sum()):.4f})")
        assert int(cl.sum()) <= 1.005 * int(cs.sum()), (d, int(cl.sum()), int(cs.sum()))
        large += int(cl.sum())
        small += int(cs.sum())
    print(f"total: large {large} small {small} ({large / small:.4f})")
    assert large <= 1.005 * small, (large, small)
