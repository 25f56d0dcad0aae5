"""GPU parity for the gfx950 zlib inflate kernel, called through
the C ABI, against the reference's outputs and the restatement oracle.

* streams made by the reference's own compress2 (tests/golden/zlib_streams.npz:
  stored, fixed and dynamic-Huffman blocks, levels 0/1/6/9) decode bit-exactly;
* every malformed / truncated / short-capacity stream of
  tests/golden/zlib_malformed.npz gets the oracle's result exactly and the
  reference's verdict (success and length exactly; failure code up to the
  Z_BUF_ERROR / Z_DATA_ERROR split the oracle tests explain);
* streams from the host zlib (Python's zlib module: a different deflate
  implementation, all strategies) decode exactly -- they exercise long (> 10
  bit) codes, fixed blocks, RLE-only and Huffman-only parses;
* streams at every byte alignment, the Buffer API with its exact-length rule
  (src/buffer.c:257-260), and a 16K-page batch.
"""
import ctypes
import hashlib
import zlib

import numpy as np
import pytest
import torch

from batch_contract_cases import checked_decode
from conftest import load_golden, unpack

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ZLIB = 2


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return codec


def ragged_inflate(tc, streams, caps, shift=0):
    """Inflate byte strings (each placed at a 16-byte boundary + shift) into per-page capacities, on
    the checked layout (batch_layout.py): 64 guard bytes around every output slot and the stream arena
    are compared after the run, so a byte written outside a slot fails whatever test called this."""
    return checked_decode(tc, ZLIB, streams, caps, shift)


def test_inflate_kat(tc):
    g = load_golden("kat_lorem.npz")
    rv, outs = ragged_inflate(tc, [g["zlib"].tobytes()], [4096])
    assert rv[0] == 4096 and outs[0] == g["text"].tobytes()


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 5])
def test_inflate_reference_streams(tc, shift):
    g = load_golden("zlib_streams.npz")
    streams = [unpack(g["comp"], g["comp_off"], g["comp_len"], i) for i in range(len(g["labels"]))]
    caps = [int(x) for x in g["size"]]
    rv, outs = ragged_inflate(tc, streams, caps, shift)
    for i in range(len(streams)):
        assert rv[i] == caps[i], (g["labels"][i], int(g["level"][i]), rv[i])
        assert hashlib.sha256(outs[i]).digest() == g["digest"][i].tobytes(), (g["labels"][i], int(g["level"][i]))


def test_inflate_malformed(tc, oracle_mod):
    g = load_golden("zlib_malformed.npz")
    streams = [unpack(g["comp"], g["comp_off"], g["comp_len"], i) for i in range(len(g["cap"]))]
    caps = [int(c) for c in g["cap"]]
    rv, outs = ragged_inflate(tc, streams, caps)
    for i, s in enumerate(streams):
        orv, oout = oracle_mod.zlib_uncompress(s, caps[i])
        assert rv[i] == orv, (i, rv[i], orv, s[:12])
        want = int(g["rv"][i])
        assert rv[i] == want, (i, rv[i], want)   # the reference's exact code: Z_DATA_ERROR / Z_BUF_ERROR too
        if want >= 0:
            assert hashlib.sha256(outs[i]).digest() == g["digest"][i].tobytes(), i


def _host_streams(oracle_mod):
    """Pages of every pagegen distribution plus skewed-random pages (long codes), encoded by the
    host zlib with every strategy and several levels."""
    rng = np.random.default_rng(7)
    pages = []
    for dist in range(6):
        for plen in (4096, 16384, 32768):
            pages.append(oracle_mod.pagegen(1, plen, seed=11, first=100 * dist + plen // 4096, dist=dist)[0].tobytes())
    for k in range(6):
        # geometric byte distribution: many rare symbols -> 11..15-bit codes
        p = 0.5 ** np.arange(1, 257) + 1e-9
        p /= p.sum()
        pages.append(rng.choice(256, size=16384, p=np.roll(p, 17 * k)).astype(np.uint8).tobytes())
    out = []
    strategies = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]
    for j, page in enumerate(pages):
        for st in strategies:
            for level in (1, 6, 9):
                if st != zlib.Z_DEFAULT_STRATEGY and level != 6:
                    continue
                c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, st)
                out.append((page, c.compress(page) + c.flush()))
    return out


def test_inflate_host_zlib_strategies(tc, oracle_mod):
    pairs = _host_streams(oracle_mod)
    streams = [c for _, c in pairs]
    caps = [len(p) for p, _ in pairs]
    rv, outs = ragged_inflate(tc, streams, caps)
    for i, (page, comp) in enumerate(pairs):
        assert rv[i] == len(page), (i, rv[i])
        assert outs[i] == page, i
        assert oracle_mod.zlib_uncompress(comp, len(page))[0] == len(page)


def test_inflate_flushed_multiblock(tc):
    """Several blocks per stream (Z_FULL_FLUSH inserts empty stored blocks and byte alignment)."""
    rng = np.random.default_rng(3)
    pages, streams = [], []
    for k in range(8):
        page = bytes(rng.integers(0, 8, 12000, dtype=np.uint8)) + bytes(range(256)) * 8
        c = zlib.compressobj(6)
        s = b""
        for j in range(0, len(page), 1000 + 300 * k):
            s += c.compress(page[j:j + 1000 + 300 * k]) + c.flush(zlib.Z_FULL_FLUSH)
        s += c.flush()
        pages.append(page)
        streams.append(s)
    rv, outs = ragged_inflate(tc, streams, [len(p) for p in pages])
    for i in range(len(pages)):
        assert rv[i] == len(pages[i]) and outs[i] == pages[i], i


def test_inflate_buffer_api(tc):
    """buffer__decompress(ZLIB): Z_OK and exactly data_length bytes (src/buffer.c:257-260)."""
    from tyche_amd import buffer as B
    from tyche_amd._lib import E_OK
    g = load_golden("kat_lorem.npz")
    text, comp = g["text"].tobytes(), g["zlib"].tobytes()

    def compressed_buffer(data_length):
        buf = B.new_buffer(b"\0" * data_length, id=9)
        mem = B._libc.malloc(len(comp))
        ctypes.memmove(mem, comp, len(comp))
        B.swap_data(buf, mem)
        buf.contents.comp_length = len(comp)
        return buf

    buf = compressed_buffer(4096)
    assert B.buffer__decompress(buf, ZLIB) == E_OK
    assert buf.contents.comp_length == 0 and buf.contents.comp_hits == 1
    assert B.buffer_bytes(buf) == text
    B.destroy(buf)
    for n in (4095, 4097):          # too small: Z_BUF_ERROR; too large: Z_OK but the wrong length
        buf = compressed_buffer(n)
        assert B.buffer__decompress(buf, ZLIB) == 126
        assert buf.contents.comp_length == len(comp)
        B.destroy(buf)


def test_inflate_large_batch(tc, oracle_mod):
    """16K pages of the bench distribution: fixed-stride slots, all exact; decoding twice is identical."""
    n, plen = 16384, 16384
    host = oracle_mod.pagegen(256, plen, seed=99, first=0, dist=0)
    comps = [zlib.compress(host[i].tobytes(), 1) for i in range(256)]
    slot = (max(len(c) for c in comps) + 127) // 128 * 128
    slots = np.zeros((n, slot), np.uint8)
    clen = np.zeros(n, np.int32)
    for i in range(n):
        c = comps[i % 256]
        slots[i, :len(c)] = np.frombuffer(c, np.uint8)
        clen[i] = len(c)
    d_slots = torch.from_numpy(slots).to(DEV)
    d_clen = torch.from_numpy(clen).to(DEV)
    out, rv = tc.decompress_pages(d_slots, d_clen, plen, compressor_id=ZLIB)
    out2, rv2 = tc.decompress_pages(d_slots, d_clen, plen, compressor_id=ZLIB)
    torch.cuda.synchronize()
    assert bool((rv == plen).all())
    ref = torch.from_numpy(np.stack([host[i % 256] for i in range(n)])).to(DEV)
    assert torch.equal(out, ref) and torch.equal(out2, out) and torch.equal(rv2, rv)


# ----------------------------------------------------------------- deflate (A10)
def _check_zlib_streams(O, comp, clen, host):
    ch, lh = comp.cpu().numpy(), clen.cpu().numpy()
    total = 0
    for i in range(host.shape[0]):
        n = host.shape[1]
        page = host[i].tobytes()
        bound = n + (n >> 12) + (n >> 14) + (n >> 25) + 13      # compressBound (compress.c:74-78)
        assert 0 < lh[i] <= bound, (i, lh[i])
        s = ch[i, :lh[i]].tobytes()
        assert zlib.decompress(s) == page, i                    # host zlib
        r, dec = O.zlib_uncompress(s, n)
        assert r == n and dec == page, (i, r)
        if O.have_ref():
            r2, dec2 = O.ref_zlib_uncompress(s, n)                # the reference's uncompress()
            assert r2 == n and dec2 == page, (i, r2)
        total += int(lh[i])
    return total


# device bytes / reference (zlib 1.2.8 compress2 level 1) bytes per (page size, distribution),
# measured (tools/ratio_probe.py, profiles/r06_ratio_probe.jsonl).  Above 1 only on dist 2 (a
# text-like page the device's one dynamic block per page codes worse than deflate_fast's blocks)
ZLIB_PIN = {(8192, 0): 0.9921, (8192, 1): 0.9632, (8192, 2): 1.2535, (8192, 3): 0.5424, (8192, 4): 1.0000,
            (8192, 5): 0.9652, (16384, 0): 0.9702, (16384, 1): 0.9591, (16384, 2): 1.2939, (16384, 3): 0.4211,
            (16384, 4): 1.0000, (16384, 5): 0.9551, (32768, 0): 1.0160, (32768, 1): 0.9608, (32768, 2): 1.2880,
            (32768, 3): 0.3374, (32768, 4): 0.9998, (32768, 5): 0.9490}


@pytest.mark.parametrize("dist", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("plen", [8192, 16384, 32768])
def test_deflate_roundtrip_reference(tc, oracle_mod, dist, plen):
    """Device-encoded zlib streams inflate with the reference's uncompress(), the oracle, the host
    zlib and the device inflate kernel back to the page."""
    n = 32
    pages = tc.pagegen(n, plen, seed=31337, first=plen + dist * 100, dist=dist, device=DEV)
    comp, clen = tc.compress_pages(pages, compressor_id=ZLIB)
    out, rv = tc.decompress_pages(comp, clen, plen, compressor_id=ZLIB)
    torch.cuda.synchronize()
    assert torch.equal(out, pages) and bool((rv == plen).all())
    host = pages.cpu().numpy()
    total = _check_zlib_streams(oracle_mod, comp, clen, host)
    if dist in (0, 1):
        assert total < 0.6 * n * plen
    if oracle_mod.have_ref():   # ratio pinned within 0.5 % of the measured device/reference bytes
        ref = sum(len(oracle_mod.ref_zlib_compress(host[i].tobytes())) for i in range(n))
        assert total <= (ZLIB_PIN[(plen, dist)] + 0.005) * ref, (total, ref)


@pytest.mark.parametrize("n", [0, 1, 2, 12, 13, 100, 258, 259, 260, 1000, 4095, 40000, 65535])
def test_deflate_sizes(tc, oracle_mod, n):
    """Edge sizes, including long runs split into 258-byte length codes with a 1-2 byte tail
    borrowed from the chunk before (lengths 259/260), and distances above 32768 (turned into literals)."""
    from tyche_amd import _lib
    rng = np.random.default_rng(n + 1)
    if n >= 40000:
        half = rng.integers(0, 256, n // 2, dtype=np.uint8).tobytes()
        data = (half + half + b"\0")[:n]                         # repeats at distance n // 2 > 32768
    else:
        data = (rng.integers(0, 2, n, dtype=np.uint8) * 7).tobytes()
        if n >= 300:
            data = data[:n - 262] + b"\x41" * 262                # a 262-byte run
    src = torch.from_numpy(np.frombuffer(data, np.uint8).copy().reshape(1, n) if n else np.zeros((1, 1), np.uint8))
    src = src.to(DEV)
    slot = tc.slot_size(max(n, 1), ZLIB)
    comp = torch.zeros((1, slot), dtype=torch.uint8, device=DEV)
    clen = torch.zeros(1, dtype=torch.int32, device=DEV)
    b = _lib.Batch(count=1, src=src.data_ptr(), src_stride=max(n, 1), src_length=n, max_src_length=n,
                   dst=comp.data_ptr(), dst_stride=slot, dst_capacity=slot, results=clen.data_ptr())
    _lib.check(_lib.load().tyche_compress_batch(ZLIB, 1, ctypes.byref(b), torch.cuda.current_stream().cuda_stream),
               "compress")
    torch.cuda.synchronize()
    L = int(clen[0])
    s = comp[0, :L].cpu().numpy().tobytes()
    assert zlib.decompress(s) == data
    r, dec = oracle_mod.zlib_uncompress(s, n)
    assert r == n and dec == data
    if oracle_mod.have_ref():
        r2, dec2 = oracle_mod.ref_zlib_uncompress(s, n)
        assert r2 == n and dec2 == data


def test_deflate_incompressible_stored(tc, oracle_mod):
    """Random pages come out as stored blocks within compressBound."""
    rng = np.random.default_rng(12)
    host = rng.integers(0, 256, (8, 32768), dtype=np.uint8)
    comp, clen = tc.compress_pages(torch.from_numpy(host).to(DEV), compressor_id=ZLIB)
    torch.cuda.synchronize()
    _check_zlib_streams(oracle_mod, comp, clen, host)
    assert (clen.cpu().numpy() == 2 + 32768 + 5 + 4).all()


def test_deflate_buffer_api(tc, oracle_mod):
    """buffer__compress(ZLIB) then buffer__decompress(ZLIB) (exact length, buffer.c:190-200, 257-260)."""
    from tyche_amd import buffer as B
    from tyche_amd._lib import E_OK
    g = load_golden("kat_lorem.npz")
    text = g["text"].tobytes()
    buf = B.new_buffer(text, id=5)
    rv, comp = B.buffer__compress(buf, ZLIB, 1)
    assert rv == E_OK and comp
    assert 0 < buf.contents.comp_length <= 4096 + 13
    B.swap_data(buf, comp)
    assert B.buffer__decompress(buf, ZLIB) == E_OK
    assert B.buffer_bytes(buf) == text
    B.destroy(buf)
    pages = oracle_mod.pagegen(24, 8192, seed=8, dist=0)
    bufs = [B.new_buffer(pages[i].tobytes(), id=i) for i in range(24)]
    rc, st, ptrs = B.buffers_compress(bufs, ZLIB, 1)
    assert rc == 0 and st == [0] * 24
    for b, p in zip(bufs, ptrs):
        B.swap_data(b, p)
    rc, st = B.buffers_decompress(bufs, ZLIB)
    assert rc == 0 and st == [0] * 24
    for i, b in enumerate(bufs):
        assert B.buffer_bytes(b) == pages[i].tobytes()
        B.destroy(b)


# ----------------------------------------------------------------- dynamic trees (§8f rank 4)
@pytest.mark.parametrize("plen", [8192, 16384, 32768])
def test_deflate_dynamic_bench_pages(tc, oracle_mod, plen):
    """Bench-distribution pages are coded as one dynamic-Huffman block (BFINAL 1, BTYPE 10 in the
    first stream bits), inflate everywhere, and compress near level 1's ratio (the fixed codes give ~3.1)."""
    n = 48
    pages = tc.pagegen(n, plen, seed=404, dist=0, device=DEV)
    comp, clen = tc.compress_pages(pages, compressor_id=ZLIB)
    out, rv = tc.decompress_pages(comp, clen, plen, compressor_id=ZLIB)
    torch.cuda.synchronize()
    assert torch.equal(out, pages) and bool((rv == plen).all())
    total = _check_zlib_streams(oracle_mod, comp, clen, pages.cpu().numpy())
    ch, lh = comp.cpu().numpy(), clen.cpu().numpy()
    assert sum(ch[i, 2] & 7 == 5 for i in range(n)) >= n - n // 12   # fixed codes only where they are smaller
    # 4-way buckets on a 3-byte hash (lz_parse.h kWays): level 1 gets 4.27 at 16 KiB on these pages
    assert n * plen / total > {8192: 3.7, 16384: 4.0, 32768: 4.2}[plen]


def _literal_heavy_page(rng, plen, draw):
    out = bytearray()
    while len(out) < plen:
        if len(out) > 64 and rng.random() < 0.5:
            p = int(rng.integers(0, len(out) - 8))
            out += out[p:p + int(rng.integers(3, 300))]
        else:
            out += bytes(draw(int(rng.integers(1, 12))))
    return np.frombuffer(bytes(out[:plen]), np.uint8)


@pytest.mark.parametrize("alphabet", ["two", "16", "256", "geo0.97", "skew99", "runs"])
@pytest.mark.parametrize("plen", [1024, 16384, 65535])
def test_deflate_dynamic_alphabets(tc, oracle_mod, alphabet, plen):
    """Skewed and tiny literal alphabets, long matches (258-byte chunks, many length codes), a page of
    runs only (a single distance code: the forced two-code distance tree): every stream inflates
    with the reference, the oracle, host zlib and the device."""
    rng = np.random.default_rng(zlib.crc32(f"{alphabet}:{plen}".encode()))
    if alphabet == "two":
        draw = lambda k: rng.choice(np.array([65, 200], np.uint8), k)
    elif alphabet in ("16", "256"):
        m = int(alphabet)
        draw = lambda k: rng.integers(256 - m, 256, k, dtype=np.uint8)
    elif alphabet == "geo0.97":
        p = 0.97 ** np.arange(256)
        p /= p.sum()
        draw = lambda k: rng.choice(256, k, p=p).astype(np.uint8)
    elif alphabet == "skew99":
        draw = lambda k: np.where(rng.random(k) < 0.99, 7, rng.integers(0, 256, k)).astype(np.uint8)
    if alphabet == "runs":
        host = np.stack([np.repeat(rng.integers(0, 256, plen // 500 + 1, dtype=np.uint8), 500)[:plen]
                         for _ in range(4)])
    else:
        host = np.stack([_literal_heavy_page(rng, plen, draw) for _ in range(4)])
    d = torch.from_numpy(host).to(DEV)
    comp, clen = tc.compress_pages(d, compressor_id=ZLIB)
    out, rv = tc.decompress_pages(comp, clen, plen, compressor_id=ZLIB)
    torch.cuda.synchronize()
    assert bool((rv == plen).all()) and torch.equal(out, d)
    _check_zlib_streams(oracle_mod, comp, clen, host)


@pytest.mark.parametrize("slack", [0, 16, 300, 3000])
def test_deflate_tight_capacity(tc, oracle_mod, slack):
    """Capacity just above the stream size: the parse records no longer fit below the stream, so the
    page is re-coded in one pass with the fixed codes, stored, or reported as not fitting (0)."""
    from tyche_amd import _lib
    plen, n = 16384, 16
    pages = tc.pagegen(n, plen, seed=77, dist=0, device=DEV)
    comp, clen = tc.compress_pages(pages, compressor_id=ZLIB)
    torch.cuda.synchronize()
    cap = int(clen.max()) + slack
    slot = tc.slot_size(plen, ZLIB)
    comp2 = torch.zeros((n, slot), dtype=torch.uint8, device=DEV)
    clen2 = torch.zeros(n, dtype=torch.int32, device=DEV)
    b = _lib.Batch(count=n, src=pages.data_ptr(), src_stride=plen, src_length=plen, max_src_length=plen,
                   dst=comp2.data_ptr(), dst_stride=slot, dst_capacity=cap, results=clen2.data_ptr())
    _lib.check(_lib.load().tyche_compress_batch(ZLIB, 1, ctypes.byref(b), torch.cuda.current_stream().cuda_stream),
               "compress")
    torch.cuda.synchronize()
    ch, lh, host = comp2.cpu().numpy(), clen2.cpu().numpy(), pages.cpu().numpy()
    assert not ch[:, cap:].any()      # nothing at or past the capacity was written (the slot was zeroed)
    for i in range(n):
        assert 0 <= lh[i] <= cap
        if lh[i]:
            s = ch[i, :lh[i]].tobytes()
            assert zlib.decompress(s) == host[i].tobytes()
            if oracle_mod.have_ref():
                r2, dec2 = oracle_mod.ref_zlib_uncompress(s, plen)
                assert r2 == plen and dec2 == host[i].tobytes()


# ----------------------------------------------------------------- lane-parallel inflate
def _bench_streams(tc, oracle_mod, plen, n):
    """Device-encoded and host-zlib level-1 streams of bench pages (one dynamic block each)."""
    pages = oracle_mod.pagegen(n, plen, seed=2024, first=plen, dist=0)
    comp, clen = tc.compress_pages(torch.from_numpy(pages).to(DEV), compressor_id=ZLIB)
    torch.cuda.synchronize()
    ch, lh = comp.cpu().numpy(), clen.cpu().numpy()
    streams = [ch[i, :lh[i]].tobytes() for i in range(n)] + [zlib.compress(pages[i].tobytes(), 1) for i in range(n)]
    return [pages[i % n].tobytes() for i in range(2 * n)], streams


@pytest.mark.parametrize("par,jump,wg", [("0", "512", "1"), ("1", "512", "1"), ("1", "512", "0"), ("1", "0", "1")])
def test_inflate_serial_and_parallel_kernels(tc, oracle_mod, knobs, par, jump, wg):
    """Both inflate kernels (TYCHE_ZLIB_PAR=0: one symbol at a time; 1: lane-parallel symbol
    decode with the serial decoder as its fallback), the parallel one with either match phase
    (TYCHE_ZLIB_JUMP_MAX=0: frontier copies; otherwise pointer jumping for batches below it),
    restore every page of every size exactly."""
    knobs(ZLIB_PAR=par, ZLIB_JUMP_MAX=jump, ZLIB_JUMP_WG=wg)   # WG 1: workgroup per page, 0: one wave
    for plen in (4096, 16384, 32768):
        pages, streams = _bench_streams(tc, oracle_mod, plen, 24)
        rv, outs = ragged_inflate(tc, streams, [plen] * len(streams), shift=plen % 7)
        assert (rv == plen).all() and outs == pages, plen


@pytest.mark.parametrize("jump,wg", [("512", "1"), ("512", "0"), ("0", "1")])
def test_inflate_parallel_corruptions(tc, oracle_mod, knobs, jump, wg):
    """Seeded corruptions of bench streams (byte flips anywhere, flips inside the compressed data,
    truncations, short capacities) through the lane-parallel kernel: the return value of every
    stream and the bytes of every success equal the oracle's -- the parallel path hands every page
    it cannot finish cleanly to the serial decoder, which gives the exact verdict."""
    knobs(ZLIB_JUMP_MAX=jump, ZLIB_JUMP_WG=wg)
    rng = np.random.default_rng(5150)
    pages, streams = _bench_streams(tc, oracle_mod, 16384, 16)
    cases, caps = [], []
    for k in range(1500):
        s = bytearray(streams[k % len(streams)])
        kind = k % 5
        if kind == 0:
            s[int(rng.integers(0, len(s)))] ^= int(rng.integers(1, 256))
        elif kind == 1:
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(2, len(s) - 4))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 2:
            s = s[:int(rng.integers(1, len(s)))]
        elif kind == 3:
            s[int(rng.integers(len(s) // 2, len(s)))] = int(rng.integers(0, 256))
        cases.append(bytes(s))
        caps.append(16384 if kind != 4 else int(rng.integers(1, 16384)))
    rv, outs = ragged_inflate(tc, cases, caps)
    for i, s in enumerate(cases):
        orv, oout = oracle_mod.zlib_uncompress(s, caps[i])
        assert rv[i] == orv, (i, i % 5, rv[i], orv)
        if orv >= 0:
            assert outs[i] == oout[:orv], i
