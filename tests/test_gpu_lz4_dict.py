"""GPU tests of LZ4 with a shared dictionary (lz4_encode_dict.hip, lz4_decode_dict.hip through the
C ABI): round trips over every dictionary and page size, the reference's verdicts on hand-made and
malformed streams, the capacity rule, batches, the reach rule, and the host entry points with a
process-wide dictionary.  Expected values come from tests/golden/lz4_dict.npz (recorded from the
reference, LZ4 1.7.5) and from the reference library itself where oracle/_ref is built; where it
is not, the emulated decoder (tools/lz4_dict_emul.cpp, proven against the reference by
test_lz4_dict_emul.py) restores the device's streams.  That fallback is the kernel's own decode
core compiled for the CPU: the statement that a device stream restores through
LZ4_decompress_safe_usingDict is independent of the code under test only in a run that has the
reference library; without it the independent evidence is the golden file -- the reference's
verdicts, its decoded bytes, its streams for the golden subset of sizes and its compressed sizes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lz4_dict_cases as C
from conftest import ROOT
from test_lz4_dict_emul import emul, golden, ref   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 64
FILL = 0xAB


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return codec


def _layout(sizes):
    """16-byte aligned slots with a guard after each: (offsets, total bytes)."""
    offs, pos = np.zeros(len(sizes), np.int64), 0
    for i, n in enumerate(sizes):
        offs[i] = pos
        pos += (n + 15) // 16 * 16 + GUARD
    return offs, pos + GUARD


def _run(tc, d, srcs, caps, compress, max_src=None, max_cap=None):
    """One ragged dictionary launch over byte strings: (results, outputs up to each result,
    True if no byte at or past any capacity was written)."""
    n = len(srcs)
    lens = [len(s) for s in srcs]
    soffs, stot = _layout(lens)
    buf = np.zeros(stot, np.uint8)
    for i, s in enumerate(srcs):
        buf[soffs[i]:soffs[i] + len(s)] = np.frombuffer(s, np.uint8)
    ooffs, otot = _layout(caps)
    d_src = torch.from_numpy(buf).to(DEV)
    d_out = torch.full((otot,), FILL, dtype=torch.uint8, device=DEV)
    d_rv = torch.full((n,), 12345, dtype=torch.int32, device=DEV)
    args = (d_src, torch.from_numpy(soffs).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV))
    d_caps, d_ooffs = torch.tensor(caps, dtype=torch.int32, device=DEV), torch.from_numpy(ooffs).to(DEV)
    if compress:
        tc.compress_ragged(*args, d_out, d_ooffs, d_caps, d_rv, max(lens + [1]) if max_src is None else max_src,
                           dictionary=d)
    else:
        tc.decompress_ragged(*args, d_caps, d_out, d_ooffs, d_rv, max_src_length=max(lens + [1]),
                             max_capacity=max(caps + [0]) if max_cap is None else max_cap, dictionary=d)
    torch.cuda.synchronize()
    rv, out = d_rv.cpu().numpy(), d_out.cpu().numpy()
    clean = True
    for i in range(n):
        end = ooffs[i + 1] if i + 1 < n else otot
        clean &= bool((out[ooffs[i] + caps[i]:end] == FILL).all())
    return rv, [out[ooffs[i]:ooffs[i] + max(int(rv[i]), 0)].tobytes() for i in range(n)], clean


def _restore(ref, emul, dic, stream, cap):
    return ref.decompress(dic, stream, cap) if ref is not None else emul.dec(dic, stream, cap)


def _groups(cases):
    g = {}
    for c in cases:
        g.setdefault(C.dict_key(c[0], c[2]), []).append(c)
    return g


def test_roundtrip_all_sizes(tc, oracle_mod, golden, ref, emul):
    """Every dictionary length x page length x page kind: the device stream restores through
    LZ4_decompress_safe_usingDict to the page; the device decode of it and of the reference-made
    stream gives the page and result L; guard bytes past every capacity stay untouched."""
    O = oracle_mod
    ref_streams = {(D, L, k): s for D, L, k, _, _, s in golden.rt_cases(O)}
    for (D, _), cases in _groups(C.all_cases(O)).items():
        dic = cases[0][3]
        d = tc.Lz4Dict(dic)
        pages = [c[4] for c in cases]
        lens = [len(p) for p in pages]
        rv, streams, clean = _run(tc, d, pages, [C.lz4_bound(n) for n in lens], True)
        assert clean, D
        for (_, L, k, _, page), r, s in zip(cases, rv, streams):
            assert 0 < r <= C.lz4_bound(L), (D, L, k, r)
            assert _restore(ref, emul, dic, s, L) == (L, page), (D, L, k)
        rv2, outs, clean = _run(tc, d, streams, lens, False)
        assert clean, D
        for (_, L, k, _, page), r, o in zip(cases, rv2, outs):
            assert r == L and o == page, (D, L, k, r)
        theirs = [(c, ref.compress(dic, c[4]) if ref is not None else ref_streams.get((c[0], c[1], c[2]))) for c in cases]
        theirs = [(c, s) for c, s in theirs if s is not None]
        if theirs:
            rv3, outs, clean = _run(tc, d, [s for _, s in theirs], [c[1] for c, _ in theirs], False)
            assert clean, D
            for (c, _), r, o in zip(theirs, rv3, outs):
                assert r == c[1] and o == c[4], (D, c[1], c[2], r)
        d.close()


@pytest.mark.parametrize("L", [64, 4096, 16384])
def test_dictionary_is_used(tc, oracle_mod, L):
    """A page equal to the dictionary's tail is one long match into it (the reference makes 17, 33
    and 74 bytes); without the feature no offset can pass a position."""
    D = 16384
    dic, page = C.dict_of(oracle_mod, D, "tail"), C.page_of(oracle_mod, D, L, "tail")
    d = tc.Lz4Dict(dic)
    rv, streams, _ = _run(tc, d, [page], [C.lz4_bound(L)], True)
    print(f"L {L}: device {rv[0]} bytes")
    assert 0 < rv[0] <= L // 255 + 32, (L, rv[0])
    assert C.max_reach(streams[0]) > 0, "no offset reaches past the page's start"


def test_verdicts(tc, oracle_mod, golden):
    """Hand-made streams (offset == position + D and one more, a dictionary match ending inside the
    last 5 bytes, a literal run past the capacity, capacities off by one) and the 10 reference-made
    dictionary streams cut at up to 40 lengths and patched at 40 positions: every result equals
    the reference's, and the decoded bytes where it is not negative."""
    O = oracle_mod
    cases = C.crafted(O)
    by_d = {}
    for i, c in enumerate(cases):
        by_d.setdefault(c[1], []).append(i)
    for D, idx in by_d.items():
        d = tc.Lz4Dict(cases[idx[0]][2])
        rv, outs, clean = _run(tc, d, [cases[i][3] for i in idx], [cases[i][4] for i in idx], False)
        assert clean, D
        for i, r, o in zip(idx, rv, outs):
            assert r == int(golden.crafted_rv[i]), (cases[i][0], r, int(golden.crafted_rv[i]))
            if r > 0:
                assert C.crc(o) == int(golden.crafted_crc[i]), cases[i][0]
    dicts = [dd for dd, _ in C.base_cases(O)]
    mal = C.malformed(golden.base_streams)
    assert len(mal) == len(golden.malformed_rv)
    for b in range(len(dicts)):
        idx = [j for j, m in enumerate(mal) if m[1] == b]
        d = tc.Lz4Dict(dicts[b])
        rv, outs, clean = _run(tc, d, [mal[j][2] for j in idx], [mal[j][3] for j in idx], False)
        assert clean, b
        for j, r, o in zip(idx, rv, outs):
            assert r == int(golden.malformed_rv[j]), (mal[j][0], r, int(golden.malformed_rv[j]))
            if r > 0 and not C.has_zero_offset(mal[j][2]):
                assert C.crc(o) == int(golden.malformed_crc[j]), mal[j][0]


def test_limited_output(tc, oracle_mod):
    """Capacities at the stream length, one below, LZ4_compressBound and 0: the result is 0 exactly
    when the device's own stream does not fit, and nothing is written at or past the capacity."""
    O = oracle_mod
    cases = [c for c in C.all_cases(O, [(4096, 4095), (65, 65), (1000, 13), (64, 0)]) if c[2] in ("dist0", "random", "tail", "seam3")]
    for (D, _), cs in _groups(cases).items():
        d = tc.Lz4Dict(cs[0][3])
        pages = [c[4] for c in cs]
        full, streams, _ = _run(tc, d, pages, [C.lz4_bound(len(p)) for p in pages], True)
        for caps in ([int(r) for r in full], [int(r) - 1 for r in full], [0] * len(cs)):
            rv, outs, clean = _run(tc, d, pages, caps, True)
            assert clean, (D, caps)
            for r, want, cap, o, s in zip(rv, full, caps, outs, streams):
                assert r == (int(want) if cap >= want else 0), (D, cap, int(want), r)
                if r:
                    assert o == s


@pytest.mark.parametrize("n", [1, 64, 3000, 8192])
def test_batches(tc, oracle_mod, ref, emul, n):
    """1, 64, 3,000 and 8,192 pages of 4 KiB with a 4 KiB dictionary.  The dictionary kernels have no
    batch-size threshold, but a grid: one workgroup per page up to what is resident, and the rest
    claimed from a counter.  The encoder (16.6 KiB of LDS here, 9 workgroups on each of 256 CUs:
    2,304) claims from 3,000 pages on; the decoder (12.2 KiB, 12 per CU: 3,072) only above that, so
    8,192 pages is the case in which every decoder wave decodes several pages one after another --
    the stream and its zero pad staged over the previous page's, the output window reused, the
    dictionary staged once.  Every page's result and bytes are checked in both directions: the
    device's streams through LZ4_decompress_safe_usingDict (the emulated decoder where the reference
    library is not built), the device's decode against the pages."""
    O = oracle_mod
    plen = 4096
    host = O.pagegen(n, plen, first=50, dist=0)
    dic = O.pagegen(1, plen, first=49, dist=0)[0].tobytes()
    d = tc.Lz4Dict(dic)
    pages = torch.from_numpy(host).to(DEV)
    comp, clen = tc.compress_pages(pages, dictionary=d)
    out, rv = tc.decompress_pages(comp, clen, plen, dictionary=d)
    torch.cuda.synchronize()
    ch, lh, oh, rh = comp.cpu().numpy(), clen.cpu().numpy(), out.cpu().numpy(), rv.cpu().numpy()
    assert bool((lh > 0).all()) and bool((lh <= C.lz4_bound(plen)).all())
    bad = np.nonzero((rh != plen) | (oh != host).any(axis=1))[0]
    assert bad.size == 0, (n, bad[:8], rh[bad[:8]])
    for i in range(n):
        assert _restore(ref, emul, dic, ch[i, :lh[i]].tobytes(), plen) == (plen, host[i].tobytes()), (n, i)
    plain, plen_plain = tc.compress_pages(pages)
    torch.cuda.synchronize()
    assert int(lh.sum()) < int(plen_plain.sum())


def test_batch_beyond_the_decoder_grid_16k(tc, oracle_mod):
    """2,000 x 16 KiB pages, D = 4096: the decoder holds 4 workgroups per CU at this size (1,024
    resident), so each wave decodes about two pages; results and bytes of every page."""
    O = oracle_mod
    n, plen = 2000, 16384
    host = O.pagegen(n, plen, first=90, dist=0)
    d = tc.Lz4Dict(O.pagegen(1, plen, first=89, dist=0)[0].tobytes()[:4096])
    pages = torch.from_numpy(host).to(DEV)
    comp, clen = tc.compress_pages(pages, dictionary=d)
    out, rv = tc.decompress_pages(comp, clen, plen, dictionary=d)
    torch.cuda.synchronize()
    oh, rh = out.cpu().numpy(), rv.cpu().numpy()
    bad = np.nonzero((rh != plen) | (oh != host).any(axis=1))[0]
    assert bool((clen > 0).all()) and bad.size == 0, (bad[:8], rh[bad[:8]])


def test_fail_hook_covers_the_dictionary_compress_call(tc, oracle_mod, knobs):
    from tyche_amd import _lib
    d = tc.Lz4Dict(C.dict_of(oracle_mod, 4096, "dist0"))
    page = C.page_of(oracle_mod, 4096, 4095, "dist0")
    knobs(FAIL_COMPRESS_EVERY=1)
    with pytest.raises(_lib.DeviceError) as e:
        _run(tc, d, [page], [C.lz4_bound(len(page))], True)
    assert "199" in str(e.value)


def test_ragged_batch(tc, oracle_mod, ref, emul):
    """Offsets and mixed lengths 0..32768 in one launch."""
    O = oracle_mod
    D = 4096
    lens = [0, 1, 12, 13, 32768, 64, 65, 4095, 16384, 5, 32768, 100, 8192, 0, 777]
    dic = C.dict_of(O, D, "dist0")
    pages = [O.pagegen(1, max(n, 1), first=300 + i, dist=i % 6)[0].tobytes()[:n] for i, n in enumerate(lens)]
    d = tc.Lz4Dict(dic)
    rv, streams, clean = _run(tc, d, pages, [C.lz4_bound(n) for n in lens], True)
    assert clean and bool((rv > 0).all()), rv
    for p, s in zip(pages, streams):
        assert _restore(ref, emul, dic, s, len(p)) == (len(p), p), len(p)
    rv2, outs, clean = _run(tc, d, streams, lens, False)
    assert clean and list(rv2) == lens and outs == pages


def test_limits(tc, oracle_mod, knobs):
    """maximum + D == 65536 works, 65537 is TYCHE_E_BAD_ARGS with both numbers in the message."""
    from tyche_amd import _lib
    O = oracle_mod
    D = 4096
    L = 65536 - D
    dic = C.dict_of(O, D, "dist0")
    d = tc.Lz4Dict(dic)
    page = (O.pagegen(2, 32768, first=5, dist=0).tobytes())[:L]
    rv, streams, clean = _run(tc, d, [page], [C.lz4_bound(L)], True)
    assert clean and rv[0] > 0
    rv2, outs, clean = _run(tc, d, streams, [L], False)
    assert clean and rv2[0] == L and outs[0] == page
    with pytest.raises(_lib.DeviceError) as e:
        _run(tc, d, [page], [C.lz4_bound(L)], True, max_src=L + 1)
    assert "190" in str(e.value) and str(L + 1) in str(e.value) and str(D) in str(e.value)
    with pytest.raises(_lib.DeviceError) as e:
        _run(tc, d, streams, [L], False, max_cap=L + 1)
    assert "190" in str(e.value) and str(L + 1) in str(e.value) and str(D) in str(e.value)
    # a page above the declared maximum: INT32_MIN, as in the plain calls
    rv, _, _ = _run(tc, d, [page[:5000], page[:100]], [6000, 200], True, max_src=4096)
    assert rv[0] == _lib.RESULT_TOO_LARGE and rv[1] > 0
    knobs(LZ4_EXACT=1)
    with pytest.raises(_lib.DeviceError) as e:
        _run(tc, d, [page[:100]], [200], True)
    assert "190" in str(e.value) and "LZ4_EXACT" in str(e.value)


# ---------------------------------------------------------------- host entry points
@pytest.fixture
def process_dict(tc, oracle_mod):
    from tyche_amd import buffer as B
    dic = C.dict_of(oracle_mod, 4096, "dist0")
    d = tc.Lz4Dict(dic)
    B.use_dict(d)
    yield dic
    B.use_dict(None)
    d.close()


def _page(O, n, i=0):
    reps = (n + 32767) // 32768
    return O.pagegen(reps, 32768, first=700 + 10 * i, dist=0).tobytes()[:n]


def test_buffer_entry_points(tc, oracle_mod, ref, emul, process_dict):
    """buffer__compress / buffer__decompress with a process-wide dictionary: the stream is a
    dictionary stream (only LZ4_decompress_safe_usingDict restores it) and the round trip holds."""
    from tyche_amd import buffer as B
    O = oracle_mod
    page = _page(O, 16384)
    b = B.new_buffer(page, id=1)
    rv, comp = B.buffer__compress(b, 1, 1)
    assert rv == 0 and comp
    B.swap_data(b, comp)
    stream = B.buffer_bytes(b)
    assert C.max_reach(stream) > 0
    assert _restore(ref, emul, process_dict, stream, len(page)) == (len(page), page)
    assert O.lz4_decompress(stream, len(page))[0] < 0      # not a plain block
    assert B.buffer__decompress(b, 1) == 0 and B.buffer_bytes(b) == page
    B.destroy(b)


def test_buffers_batch_mixed_reach(tc, oracle_mod, ref, emul):
    """tyche_buffers_compress / _decompress over sizes inside and outside the dictionary's reach:
    the pages outside it (61,441 and 100,000 bytes at D = 4096) get the bytes of a run without a
    dictionary, the others dictionary streams; everything restores."""
    from tyche_amd import buffer as B
    O = oracle_mod
    sizes = [100, 8192, 16384, 61441, 100000]
    pages = [_page(O, n, i) for i, n in enumerate(sizes)]

    def compress_all():
        bufs = [B.new_buffer(p, id=i) for i, p in enumerate(pages)]
        rc, st, ptrs = B.buffers_compress(bufs, 1, 1)
        assert rc == 0 and st == [0] * len(bufs)
        for b, p in zip(bufs, ptrs):
            B.swap_data(b, p)
        return bufs, [B.buffer_bytes(b) for b in bufs]

    bufs0, plain = compress_all()
    for b in bufs0:
        B.destroy(b)
    dic = C.dict_of(O, 4096, "dist0")
    d = tc.Lz4Dict(dic)
    B.use_dict(d)
    try:
        bufs, streams = compress_all()
        assert streams[3] == plain[3] and streams[4] == plain[4]
        for i in range(3):
            assert _restore(ref, emul, dic, streams[i], sizes[i]) == (sizes[i], pages[i]), sizes[i]
        assert C.max_reach(streams[0]) > 0 and C.max_reach(streams[1]) > 0
        rc, st = B.buffers_decompress(bufs, 1)
        assert rc == 0 and st == [0] * len(bufs)
        assert [B.buffer_bytes(b) for b in bufs] == pages
        for b in bufs:
            B.destroy(b)
    finally:
        B.use_dict(None)
        d.close()
    bufs1, again = compress_all()                           # and without it, the bytes of before
    assert again == plain
    for b in bufs1:
        B.destroy(b)


def test_host_batches_and_removal(tc, oracle_mod, ref, emul):
    """tyche_compress_host / tyche_decompress_host with the dictionary; after tyche_lz4_use_dict(NULL)
    a 16 KiB pagegen batch gives byte for byte the streams it gave before it was installed."""
    from tyche_amd import _lib, buffer as B
    O = oracle_mod
    lib = _lib.load()
    n, plen = 96, 16384
    host = O.pagegen(n, plen, first=11, dist=0)

    def compress_host():
        cap = C.lz4_bound(plen)
        out = np.full((n, cap + GUARD), FILL, np.uint8)
        srcs = (ctypes.c_void_p * n)(*[host[i].ctypes.data for i in range(n)])
        dsts = (ctypes.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
        slen, dcap = (ctypes.c_uint32 * n)(*([plen] * n)), (ctypes.c_uint32 * n)(*([cap] * n))
        res = (ctypes.c_int32 * n)()
        _lib.check(lib.tyche_compress_host(1, 1, n, srcs, slen, dsts, dcap, res), "tyche_compress_host")
        assert bool((out[:, cap:] == FILL).all())
        return [out[i, :res[i]].tobytes() for i in range(n)]

    def decompress_host(streams):
        sb = [np.frombuffer(s, np.uint8).copy() for s in streams]
        out = np.full((n, plen + GUARD), FILL, np.uint8)
        srcs = (ctypes.c_void_p * n)(*[s.ctypes.data for s in sb])
        dsts = (ctypes.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
        slen, dcap = (ctypes.c_uint32 * n)(*[len(s) for s in streams]), (ctypes.c_uint32 * n)(*([plen] * n))
        res = (ctypes.c_int32 * n)()
        _lib.check(lib.tyche_decompress_host(1, n, srcs, slen, dsts, dcap, res), "tyche_decompress_host")
        assert bool((out[:, plen:] == FILL).all())
        return list(res), out[:, :plen]

    before = compress_host()
    dic = C.dict_of(O, 4096, "dist0")
    d = tc.Lz4Dict(dic)
    B.use_dict(d)
    try:
        with_dict = compress_host()
        assert sum(map(len, with_dict)) < sum(map(len, before))
        for i in (0, n // 2, n - 1):
            assert _restore(ref, emul, dic, with_dict[i], plen) == (plen, host[i].tobytes()), i
        rv, out = decompress_host(with_dict)
        assert rv == [plen] * n and np.array_equal(out, host)
    finally:
        B.use_dict(None)
        d.close()
    assert compress_host() == before
    rv, out = decompress_host(before)
    assert rv == [plen] * n and np.array_equal(out, host)


def test_restore_queue_with_dictionary(tc, oracle_mod, process_dict):
    from tyche_amd import _lib, buffer as B
    lib = _lib.load()
    page = _page(oracle_mod, 8192, 3)
    b = B.new_buffer(page, id=9)
    rv, comp = B.buffer__compress(b, 1, 1)
    assert rv == 0
    B.swap_data(b, comp)
    assert C.max_reach(B.buffer_bytes(b)) > 0
    assert lib.tyche_restore_queue_start(8, 100) == 0
    try:
        assert lib.tyche_buffer_restore(b, 1) == 0
    finally:
        lib.tyche_restore_queue_stop()
    assert B.buffer_bytes(b) == page
    B.destroy(b)


def test_env_dictionary_in_a_child_process(tmp_path, oracle_mod, ref, emul):
    """TYCHE_LZ4_DICT=<file>: a fresh child process does a Buffer round trip whose stream only the
    dictionary decoder restores."""
    O = oracle_mod
    dic = C.dict_of(O, 4096, "dist0")
    path = tmp_path / "pages.dict"
    path.write_bytes(dic)
    page = _page(O, 16384, 5)
    (tmp_path / "page.bin").write_bytes(page)
    code = ("import sys\n"
            "from tyche_amd import buffer as B\n"
            f"page = open({str(tmp_path / 'page.bin')!r}, 'rb').read()\n"
            "b = B.new_buffer(page, id=1)\n"
            "rv, comp = B.buffer__compress(b, 1, 1)\n"
            "assert rv == 0, rv\n"
            "B.swap_data(b, comp)\n"
            f"open({str(tmp_path / 'stream.bin')!r}, 'wb').write(B.buffer_bytes(b))\n"
            "assert B.buffer__decompress(b, 1) == 0 and B.buffer_bytes(b) == page\n"
            "print('child ok')\n")
    env = dict(os.environ, TYCHE_LZ4_DICT=str(path), PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr
    stream = (tmp_path / "stream.bin").read_bytes()
    assert C.max_reach(stream) > 0 and O.lz4_decompress(stream, len(page))[0] < 0
    assert _restore(ref, emul, dic, stream, len(page)) == (len(page), page)


# device bytes / reference bytes with the same dictionary per (page size, distribution, dictionary
# length), measured (profiles/lz4_dict_ratio.jsonl); the bound is the measurement + 0.5 %
LZ4_DICT_PIN = {(8192, 0, 4096): 1.0099, (8192, 0, 8192): 1.0113, (8192, 1, 4096): 1.0050, (8192, 1, 8192): 1.0119,
                (8192, 2, 4096): 1.0459, (8192, 2, 8192): 1.0477, (8192, 3, 4096): 0.9767, (8192, 3, 8192): 0.9767,
                (8192, 4, 4096): 1.0000, (8192, 4, 8192): 1.0000, (8192, 5, 4096): 0.9930, (8192, 5, 8192): 0.9949,
                (16384, 0, 4096): 1.0217, (16384, 0, 16384): 1.0227, (16384, 1, 4096): 1.0174, (16384, 1, 16384): 1.0196,
                (16384, 2, 4096): 1.0372, (16384, 2, 16384): 1.0421, (16384, 3, 4096): 0.9867, (16384, 3, 16384): 0.9867,
                (16384, 4, 4096): 1.0000, (16384, 4, 16384): 1.0000, (16384, 5, 4096): 0.9975, (16384, 5, 16384): 1.0033,
                (32768, 0, 4096): 1.0173, (32768, 0, 32768): 1.0337, (32768, 1, 4096): 1.0199, (32768, 1, 32768): 1.0341,
                (32768, 2, 4096): 1.0355, (32768, 2, 32768): 1.0446, (32768, 3, 4096): 0.9928, (32768, 3, 32768): 0.9928,
                (32768, 4, 4096): 1.0000, (32768, 4, 32768): 1.0000, (32768, 5, 4096): 1.0022, (32768, 5, 32768): 1.0084}


@pytest.mark.parametrize("case", C.ratio_cases(), ids=lambda c: f"{c[0]}-dist{c[1]}-D{c[2]}")
def test_ratio_against_reference(tc, oracle_mod, golden, case):
    """The inputs of test_encode_roundtrip_oracle with one more page of the distribution as
    dictionary: device bytes within the pinned ratio of the reference's with the same dictionary,
    and on dist 0, 1, 2 and 5 below the device's own bytes without a dictionary."""
    n, dist, dl = case
    dic, host = C.ratio_inputs(oracle_mod, n, dist, dl)
    d = tc.Lz4Dict(dic)
    pages = torch.from_numpy(host).to(DEV)
    comp, clen = tc.compress_pages(pages, dictionary=d)
    out, rv = tc.decompress_pages(comp, clen, n, dictionary=d)
    _, plain = tc.compress_pages(pages)
    torch.cuda.synchronize()
    assert bool((rv == n).all()) and torch.equal(out, pages)
    ours, theirs, nodict = int(clen.sum()), int(golden.ratio_ref[C.ratio_cases().index(case)]), int(plain.sum())
    print(f'{{"page": {n}, "dist": {dist}, "dict": {dl}, "device": {ours}, "reference": {theirs}, '
          f'"device_no_dict": {nodict}, "ratio": {ours / theirs:.4f}}}')
    if dist in (0, 1, 2, 5):
        assert ours < nodict, (ours, nodict)
    assert case in LZ4_DICT_PIN, "no pinned measurement for this case"
    assert ours <= (LZ4_DICT_PIN[case] + 0.005) * theirs, (ours, theirs, ours / theirs)


# the same for the reference's sample_data pages (profiles/lz4_dict_ratio.jsonl, its last lines)
LZ4_DICT_SAMPLE_PIN = {("8k/names/indexes", 4096): 1.0066, ("8k/names/tables", 4096): 1.0048, ("16k/names/indexes", 4096): 1.0103,
                       ("16k/names/tables", 4096): 0.9998, ("32k/names/indexes", 4096): 0.9984, ("32k/names/indexes", 16384): 0.9955,
                       ("32k/names/tables", 4096): 0.9973}


@pytest.mark.parametrize("case", C.sample_cases(), ids=lambda c: f"{c[0].replace('/', '-')}-D{c[1]}")
def test_sample_pages_ratio_against_reference(tc, oracle_mod, golden, ref, emul, case):
    """The reference's sample_data pages, per set: the first page's first bytes as dictionary, the
    remaining 9 pages compressed against it.  Device bytes within the pinned ratio of the
    reference's with the same dictionary, below the device's own without one, and every stream
    restores."""
    name, dl = case
    dic, plist = C.sample_inputs(oracle_mod, name, dl)
    n = len(plist[0])
    host = np.stack([np.frombuffer(p, np.uint8) for p in plist])
    d = tc.Lz4Dict(dic)
    pages = torch.from_numpy(host.copy()).to(DEV)
    comp, clen = tc.compress_pages(pages, dictionary=d)
    out, rv = tc.decompress_pages(comp, clen, n, dictionary=d)
    _, plain = tc.compress_pages(pages)
    torch.cuda.synchronize()
    assert bool((rv == n).all()) and torch.equal(out, pages)
    ch, lh = comp.cpu().numpy(), clen.cpu().numpy()
    for i, p in enumerate(plist):
        assert _restore(ref, emul, dic, ch[i, :lh[i]].tobytes(), n) == (n, p), (name, i)
    k = C.sample_cases().index(case)
    ours, theirs, nodict = int(lh.sum()), int(golden.sample_ref[k]), int(plain.sum())
    print(f'{{"sample": "{name}", "dict": {dl}, "device": {ours}, "reference": {theirs}, "device_no_dict": {nodict}, '
          f'"reference_no_dict": {int(golden.sample_ref_plain[k])}, "ratio": {ours / theirs:.4f}}}')
    assert ours < nodict, (ours, nodict)
    assert case in LZ4_DICT_SAMPLE_PIN, "no pinned measurement for this case"
    assert ours <= (LZ4_DICT_SAMPLE_PIN[case] + 0.005) * theirs, (ours, theirs, ours / theirs)
