"""GPU parity of the exact LZ4 encoder (LZ4_EXACT=1, tyche_amd/csrc/lz4_encode_exact.hip): every
result and every stream equals LZ4 1.7.5's LZ4_compress_default, checked against the restatement
oracle.lz4_compress (proven against the reference's own outputs by test_oracle.py) and the golden
streams under tests/golden; nothing at or past a page's dst_capacity is written; with the knob off
or cleared the default encoder's bytes are unchanged.  test_lz4_exact_emul.py checks the same
algorithm (lz4_exact_core.h) on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, unpack
from lz4_exact_cases import KINDS, PAGE_LENS, kind_pages, limited_caps, limited_pages, ragged_pages

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILL = 0xAB


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return codec


def ragged_compress(tc, pages, caps, slot_extra=64):
    """Compresses a list of byte strings with per-page capacities through the general batch API.
    Page i starts at an offset of alignment i mod 16; its output slot (capacity + slot_extra
    bytes) is pre-filled with 0xAB.  Returns (results, slots as numpy arrays)."""
    n = len(pages)
    offs, pos = np.zeros(n, np.int64), 0
    for i, p in enumerate(pages):
        pos = (pos + 15) // 16 * 16 + i % 16
        offs[i] = pos
        pos += len(p)
    buf = np.zeros(pos + 64, np.uint8)
    for i, p in enumerate(pages):
        buf[offs[i]:offs[i] + len(p)] = np.frombuffer(p, np.uint8)
    ooffs, opos = np.zeros(n, np.int64), 0
    for i, c in enumerate(caps):
        ooffs[i] = opos
        opos += c + slot_extra
    d_src = torch.from_numpy(buf).to(DEV)
    d_out = torch.full((opos + 64,), FILL, dtype=torch.uint8, device=DEV)
    d_rv = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    tc.compress_ragged(d_src, torch.from_numpy(offs).to(DEV),
                       torch.tensor([len(p) for p in pages], dtype=torch.int32, device=DEV), d_out,
                       torch.from_numpy(ooffs).to(DEV), torch.tensor(caps, dtype=torch.int32, device=DEV), d_rv,
                       max_src_length=max(len(p) for p in pages))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    return d_rv.cpu().numpy(), [out[ooffs[i]:ooffs[i] + caps[i] + slot_extra] for i in range(n)]


def check_ragged(tc, O, pages, caps):
    rv, slots = ragged_compress(tc, pages, caps)
    for i, (p, c) in enumerate(zip(pages, caps)):
        want = O.lz4_compress(p, c)
        assert rv[i] == len(want), (i, len(p), c, rv[i], len(want))
        assert slots[i][:len(want)].tobytes() == want, (i, len(p), c)
        assert bool((slots[i][c:] == FILL).all()), ("wrote past dst_capacity", i, len(p), c)


def compress_rows(tc, host):
    """compress_pages on a (n, plen) numpy array: (lengths, slots) as numpy arrays."""
    comp, clen = tc.compress_pages(torch.from_numpy(np.ascontiguousarray(host)).to(DEV))
    torch.cuda.synchronize()
    return clen.cpu().numpy(), comp.cpu().numpy()


def check_rows(tc, O, host):
    lh, ch = compress_rows(tc, host)
    for i in range(len(host)):
        want = O.lz4_compress(host[i].tobytes())
        assert lh[i] == len(want), (i, lh[i], len(want))
        assert ch[i, :lh[i]].tobytes() == want, i


def test_fixtures(tc, oracle_mod, knobs):
    """The reference's own outputs: the KAT text -> its 2578 bytes, every reference-generated page
    and every sample page kept raw -> its golden stream."""
    O = oracle_mod
    knobs(LZ4_EXACT=1)
    g = load_golden("kat_lorem.npz")
    lh, ch = compress_rows(tc, g["text"].reshape(1, -1))
    assert lh[0] == 2578 and ch[0, :2578].tobytes() == g["lz4"].tobytes()
    gg, gs = load_golden("lz4_generated.npz"), load_golden("lz4_sample.npz")
    seed = int(gg["seed"])
    pages = [O.pagegen(1, int(plen), seed=seed, first=int(idx), dist=int(dist))[0].tobytes()
             for dist, plen, idx in gg["meta"]]
    want = [unpack(gg["comp"], gg["comp_off"], gg["comp_len"], i) for i in range(len(pages))]
    for k, i in enumerate(gs["raw_index"]):
        pages.append(unpack(gs["raw"], gs["raw_off"], gs["raw_len"], k))
        want.append(unpack(gs["comp"], gs["comp_off"], gs["comp_len"], int(i)))
    rv, slots = ragged_compress(tc, pages, [O.lz4_bound(len(p)) for p in pages])
    for i in range(len(pages)):
        assert rv[i] == len(want[i]), (i, rv[i], len(want[i]))
        assert slots[i][:rv[i]].tobytes() == want[i], i


@pytest.mark.parametrize("plen", PAGE_LENS)
@pytest.mark.parametrize("kind", KINDS)
def test_page_kinds(tc, oracle_mod, knobs, kind, plen):
    """pagegen distributions 0-5, all-zero pages, periods of 1-5 and 7 bytes (overlap matches, the
    immediate match through the ip-2 insert), incompressible pages (thousands of attempts with
    growing steps, abandonment at the page end), long literal runs, and one match long enough for
    more than four 255 length bytes; 8 pages each."""
    knobs(LZ4_EXACT=1)
    check_rows(tc, oracle_mod, kind_pages(oracle_mod, kind, plen))


@pytest.mark.parametrize("symbols", [2, 4, 256])
def test_ragged_small_pages(tc, oracle_mod, knobs, symbols):
    """Every length 1..80 and 127, 128, 129, 255, 256, 4095 in one ragged batch, source offsets of
    every alignment mod 16: the L < 13 path, the mflimit / matchlimit edges, unaligned staging."""
    knobs(LZ4_EXACT=1)
    pages = ragged_pages(symbols)
    check_ragged(tc, oracle_mod, pages, [oracle_mod.lz4_bound(len(p)) for p in pages])


@pytest.mark.parametrize("which", [0, 1], ids=["compressible", "incompressible"])
def test_limited_output(tc, oracle_mod, knobs, which):
    """dst_capacity below LZ4_compressBound: the reference's three conservative checks decide (0
    in a few cases where the stream would have fit), and the slot behind the capacity keeps its
    0xAB fill."""
    knobs(LZ4_EXACT=1)
    page = limited_pages(oracle_mod)[which]
    caps = limited_caps(oracle_mod, page, 7 + which)
    check_ragged(tc, oracle_mod, [page] * len(caps), caps)


def test_more_pages_than_resident_waves(tc, oracle_mod, knobs):
    """4096 x 4 KiB pages of mixed distributions in one launch: every wave takes several pages (a
    table that is not zeroed again, or an error in the prefetched next page, shows here)."""
    O = oracle_mod
    knobs(LZ4_EXACT=1)
    n, plen = 4096, 4096
    host = np.concatenate([O.pagegen(n // 4, plen, seed=515, first=1000 * d, dist=d) for d in (0, 1, 2, 3, 4, 5)])
    host = host[np.random.default_rng(4).permutation(len(host))[:n]]
    lh, ch = compress_rows(tc, host)
    want = np.zeros((n, O.lz4_bound(plen)), np.uint8)
    wl = np.zeros(n, np.int32)
    O.lz4_compress_pages(np.ascontiguousarray(host), want, wl, 0, n)
    assert np.array_equal(lh, wl), np.nonzero(lh != wl)[0][:10]
    mask = np.arange(want.shape[1])[None, :] < wl[:, None]
    assert np.array_equal(ch[:, :want.shape[1]] * mask, want * mask)


def test_host_entry_points(tc, oracle_mod, knobs):
    """buffer__compress and tyche_compress_host with the knob set give the oracle's bytes and length."""
    from tyche_amd import _lib, buffer as B
    O = oracle_mod
    knobs(LZ4_EXACT=1)
    lib = _lib.load()
    page = O.pagegen(1, 8192, seed=3, first=9, dist=0)[0].tobytes()
    want = O.lz4_compress(page)
    buf = B.new_buffer(page, id=7)
    rv, comp = B.buffer__compress(buf, _lib.LZ4_COMPRESSOR_ID, 1)
    assert rv == _lib.E_OK and comp
    assert buf.contents.comp_length == len(want)
    assert ctypes.string_at(comp, len(want)) == want
    B.free_ptr(comp)
    B.destroy(buf)

    n, plen = 64, 16384
    pages = O.pagegen(n, plen, seed=12, first=77, dist=1)
    cap = O.lz4_bound(plen)
    out = np.zeros((n, cap), np.uint8)
    res = np.zeros(n, np.int32)
    vp = ctypes.c_void_p * n
    rc = lib.tyche_compress_host(_lib.LZ4_COMPRESSOR_ID, 1, n, vp(*[pages.ctypes.data + i * plen for i in range(n)]),
                                 (ctypes.c_uint32 * n)(*([plen] * n)), vp(*[out.ctypes.data + i * cap for i in range(n)]),
                                 (ctypes.c_uint32 * n)(*([cap] * n)), res.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == 0, _lib.last_error()
    for i in range(n):
        w = O.lz4_compress(pages[i].tobytes())
        assert res[i] == len(w) and out[i, :res[i]].tobytes() == w, i


def test_knob_off_is_the_default_encoder(tc, oracle_mod):
    """After tyche_clear_knob the same device call gives the bytes it gave before the knob was set;
    the knob at 0 gives them too; and they are not the exact stream on at least one dist-1 page."""
    from tyche_amd import _lib
    host = oracle_mod.pagegen(16, 16384, seed=8, first=3, dist=1)

    def streams():
        lh, ch = compress_rows(tc, host)
        return [ch[i, :lh[i]].tobytes() for i in range(len(host))]
    try:
        before = streams()
        _lib.set_knob("LZ4_EXACT", 1)
        exact = streams()
        _lib.clear_knob("LZ4_EXACT")
        cleared = streams()
        _lib.set_knob("LZ4_EXACT", 0)
        zero = streams()
    finally:
        _lib.clear_knob("LZ4_EXACT")
    assert exact == [oracle_mod.lz4_compress(p.tobytes()) for p in host]
    assert cleared == before
    assert zero == before
    assert any(a != b for a, b in zip(before, exact))


@pytest.mark.parametrize("plen", PAGE_LENS)
def test_exact_streams_decode(tc, oracle_mod, knobs, plen):
    """The exact streams of every page kind go through the device decoder back to the pages."""
    knobs(LZ4_EXACT=1)
    host = np.concatenate([kind_pages(oracle_mod, kind, plen) for kind in KINDS])
    pages = torch.from_numpy(host).to(DEV)
    comp, clen = tc.compress_pages(pages)
    out, rv = tc.decompress_pages(comp, clen, plen, max_comp_len=int(clen.max()))
    torch.cuda.synchronize()
    assert bool((rv == plen).all()), rv
    assert torch.equal(out, pages)
