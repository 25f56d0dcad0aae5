"""GPU tests of zlib with a shared dictionary (zlib_deflate_dict_kernel, zlib_inflate_dict_kernel,
through the C ABI): round trips over every dictionary and page size, the stored rule, the dictionary
really being used, the reference's verdicts at the reach boundary, on header forms, wrong dictionaries
and the malformed corpus, the batch contract on the checked layout, limited output, the failure hook,
the host entry points with a process-wide dictionary, the knob-off digests and the ratio against the
reference.  Every device result is held to two independent checkers: the reference library (zlib
1.2.8 from oracle/_ref through ctypes, where it is built; tests/golden/zlib_dict.npz has what it
answered otherwise) and Python's own zlib with zdict=."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import batch_contract_cases as BC
import batch_layout as BL
import zlib_dict_cases as C
import zlib_hc_cases as ZHC
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ZLIB = C.ZLIB
GUARD = 64
FILL = 0xAB
SENTINEL = 0x5A5A5A5A
INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return codec


@pytest.fixture(scope="module")
def golden():
    return C.Golden()


@pytest.fixture(scope="module")
def ref(oracle_mod):
    return C.ref_or_none(oracle_mod)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(tc, d, srcs, caps, compress, max_src=None, max_cap=None, whole=False):
    """One ragged zlib launch over byte strings on the checked layout of batch_layout.py (d: the
    dictionary, None: the plain call): sources at every byte shift with random bytes around them,
    destinations at every byte shift with guards on both sides, results preset to a sentinel.
    Returns (results, outputs up to each result -- whole: up to each capacity); guards and the
    source arena are checked."""
    n = len(srcs)
    lay = BL.build(srcs, caps, BC.src_shifts(n), BC.dst_shifts(n), ("random", 9))
    d_src, d_out = _dev(lay.src), _dev(lay.out)
    d_rv = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    lens = [len(s) for s in srcs]
    if compress:
        tc.compress_ragged(d_src, _dev(lay.src_offsets), _dev(lay.src_lengths), d_out, _dev(lay.dst_offsets),
                           _dev(lay.caps), d_rv, max(lens + [1]) if max_src is None else max_src, compressor_id=ZLIB,
                           dictionary=d)
    else:
        tc.decompress_ragged(d_src, _dev(lay.src_offsets), _dev(lay.src_lengths), _dev(lay.caps), d_out,
                             _dev(lay.dst_offsets), d_rv, max_src_length=max(lens + [1]),
                             max_capacity=max(list(caps) + [0]) if max_cap is None else max_cap, compressor_id=ZLIB,
                             dictionary=d)
    torch.cuda.synchronize()
    rv, out = d_rv.cpu().numpy(), d_out.cpu().numpy()
    BL.check(out, d_src.cpu().numpy(), lay)
    if whole:
        return rv, [out[int(o):int(o) + int(c)].tobytes() for o, c in zip(lay.dst_offsets, lay.caps)]
    return rv, BL.outputs(out, rv, lay)


def _restores(ref, dic, stream, page):
    """Both independent checkers restore the stream to the page with the dictionary."""
    assert C.py_decompress(dic, stream, len(page)) == (len(page), page)
    if ref is not None:
        assert ref.decompress(dic, stream, len(page)) == (len(page), page)


def _needs_dictionary(ref, dic, stream, page):
    assert stream[:6] == C.dict_header(dic)
    assert C.py_decompress(None, stream, len(page))[0] == C.Z_DATA
    _restores(ref, dic, stream, page)


# ---------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("D", C.DS)
def test_roundtrip_all_sizes(tc, oracle_mod, golden, ref, D):
    """Every page length x page kind for this dictionary length, one launch each way: the device
    stream is at most tyche_compress_bound, restores to the page through the reference's inflate and
    through Python's zlib with the dictionary, and through the device's dictionary decoder; a stream
    that is not the plain stored one begins 78 3F and the dictionary's adler32.  The device decodes
    the reference-made streams of the same pages (made now, or the golden file's)."""
    O = oracle_mod
    cases = C.all_cases(O, [p for p in C.PAIRS if p[0] == D])
    dic = cases[0][3]
    d = tc.Dictionary(dic)
    pages = [c[4] for c in cases]
    lens = [len(p) for p in pages]
    rv, streams = _run(tc, d, pages, [C.zlib_bound(n) for n in lens], True)
    coded = 0
    for (_, L, k, _, page), r, s in zip(cases, rv, streams):
        assert 0 < r <= C.zlib_bound(L), (D, L, k, r)
        if s[:2] == b"\x78\x01":
            assert s == C.stored_stream(page), (D, L, k)
        else:
            assert s[:6] == C.dict_header(dic), (D, L, k)
            coded += 1
        _restores(ref, dic, s, page)
    assert coded >= len(cases) // 2, (D, coded)
    rv2, outs = _run(tc, d, streams, lens, False)
    for (_, L, k, _, page), r, o in zip(cases, rv2, outs):
        assert r == L and o == page, (D, L, k, r)
    recorded = {(gd, gl, gk): f for gd, gl, gk, _, _, f in golden.rt_cases(O)}
    theirs = [(c, ref.compress(dic, c[4]) if ref is not None else recorded.get((c[0], c[1], c[2]))) for c in cases]
    theirs = [(c, f) for c, f in theirs if f is not None]
    assert theirs or D not in C.GOLDEN_DS
    if theirs:
        rv3, outs = _run(tc, d, [f for _, f in theirs], [c[1] for c, _ in theirs], False)
        for (c, _), r, o in zip(theirs, rv3, outs):
            assert r == c[1] and o == c[4], (D, c[1], c[2], r)
    d.close()


# ---------------------------------------------------------------- 2. the stored rule
def test_stored_rule(tc, oracle_mod, ref):
    """Random pages of 1, 100, 4095, 4096, 8191 and 8192 bytes at a capacity of exactly
    tyche_compress_bound: the result is above 0 and within the bound; the stream begins 78 01 and is
    the plain stored stream, byte for byte what emit_stored writes (built here from its definition) --
    and the plain encoder's own stream for the same page wherever that one is stored too, which is
    every size but 1: the plain encoder codes a single byte in 9 bytes, where this encoder's coded
    form, with its 4 DICTID bytes, is 13 against the stored form's 12.  It decodes through the
    dictionary decoder and through the plain decoder, through Python's zlib with and without a
    dictionary, and through the reference."""
    sizes = (1, 100, 4095, 4096, 8191, 8192)
    dic = C.dict_of(oracle_mod, 4096)
    pages = [C.page_of(oracle_mod, 4096, n, "random") for n in sizes]
    caps = [C.zlib_bound(n) for n in sizes]
    d = tc.Dictionary(dic)
    rv, streams = _run(tc, d, pages, caps, True)
    rvp, plain = _run(tc, None, pages, caps, True)
    for n, page, cap, r, s, ps in zip(sizes, pages, caps, rv, streams, plain):
        assert 0 < r <= cap, (n, r, cap)
        assert s[:2] == b"\x78\x01" and s == C.stored_stream(page), n
        if n > 1:
            assert s == ps, n
        else:
            assert len(ps) == 9 and ps[:2] == b"\x78\x01"
        assert C.py_decompress(dic, s, n) == (n, page) and C.py_decompress(None, s, n) == (n, page)
        if ref is not None:
            assert ref.decompress(dic, s, n) == (n, page) and ref.decompress(None, s, n) == (n, page)
    for dd in (d, None):
        rv2, outs = _run(tc, dd, streams, list(sizes), False)
        assert [int(r) for r in rv2] == list(sizes) and outs == pages
    d.close()


def test_empty_page(tc, oracle_mod, ref):
    """An empty page is the default's empty block behind the dictionary header: the 12 bytes the
    reference writes."""
    dic = C.dict_of(oracle_mod, 4096)
    d = tc.Dictionary(dic)
    rv, streams = _run(tc, d, [b""], [C.zlib_bound(0)], True)
    assert rv[0] == 12 and streams[0] == C.dict_header(dic) + bytes([3, 0, 0, 0, 0, 1])
    assert streams[0] == C.py_compress(dic, b"")
    if ref is not None:
        assert streams[0] == ref.compress(dic, b"")
    rv2, _ = _run(tc, d, streams, [0], False)
    assert rv2[0] == 0
    d.close()


# ---------------------------------------------------------------- 3. the dictionary is used
@pytest.mark.parametrize("L", C.USED_LS)
def test_dictionary_is_used(tc, oracle_mod, golden, ref, L):
    """D = 16384 random bytes, the page its last L bytes: the reference makes 14 / 50 / 141 bytes
    with the dictionary; the device's stream is at most L/16 + 64 bytes, and the plain decoders
    give -3 for it."""
    dic, page = C.used_case(L)
    k = C.USED_LS.index(L)
    d = tc.Dictionary(dic)
    rv, streams = _run(tc, d, [page], [C.zlib_bound(L)], True)
    print(f"L {L}: device {rv[0]} bytes, reference {int(golden.used_ref[k])}")
    assert 0 < rv[0] <= L // 16 + 64, (L, rv[0])
    _needs_dictionary(ref, dic, streams[0], page)
    rvp, _ = _run(tc, None, streams, [L], False)
    assert rvp[0] == C.Z_DATA, rvp
    assert oracle_mod.zlib_uncompress(streams[0], L)[0] == C.Z_DATA
    rv2, outs = _run(tc, d, streams, [L], False)
    assert rv2[0] == L and outs[0] == page
    d.close()


# ---------------------------------------------------------------- 4. verdicts
def test_crafted_verdicts(tc, golden, ref):
    """The crafted fixed-code streams of zlib_dict_cases.crafted_cases: a distance of exactly position
    + D decodes and one more is -3; a plain-header stream may not reach the dictionary; matches that
    begin in the dictionary and overlap their own output or run over the seam; FDICT under every
    valid FLG; truncation inside the DICTID; a wrong dictionary.  Each verdict (and the bytes) is the
    reference's as recorded, the reference's now, and Python's zlib's."""
    cases = C.crafted_cases()
    by_dict = {}
    for i, c in enumerate(cases):
        by_dict.setdefault(c[1], []).append(i)
    for dic, idx in by_dict.items():
        d = tc.Dictionary(dic)
        rv, outs = _run(tc, d, [cases[i][2] for i in idx], [cases[i][3] for i in idx], False)
        for i, r, o in zip(idx, rv, outs):
            name, _, stream, cap, want = cases[i]
            assert int(r) == int(golden.crafted_rv[i]), (name, r)
            assert C.py_decompress(dic, stream, cap)[0] == int(r), name
            if ref is not None:
                assert ref.decompress(dic, stream, cap)[0] == int(r), name
            if int(r) >= 0:
                assert o == want and C.crc(o) == int(golden.crafted_crc[i]), name
        d.close()
    # the plain decoders: -3 for every FDICT stream, as before
    fdict = [c for c in cases if c[2][1:2] and c[2][1] & 0x20 and len(c[2]) > 6]
    rv, _ = _run(tc, None, [c[2] for c in fdict], [c[3] for c in fdict], False)
    assert all(int(r) == C.Z_DATA for r in rv), list(rv)


def test_capacity_above_the_launch_maximum(tc, oracle_mod):
    """INT32_MIN and an untouched destination where a page's capacity is above the launch's."""
    dic = C.dict_of(oracle_mod, 64)
    page = C.page_of(oracle_mod, 64, 4096, "dist0")
    d = tc.Dictionary(dic)
    _, streams = _run(tc, d, [page], [C.zlib_bound(4096)], True)
    rv, outs = _run(tc, d, streams, [4096], False, max_cap=4095, whole=True)
    assert rv[0] == INT32_MIN and outs[0] == bytes([FILL]) * 4096
    rv, outs = _run(tc, d, [page], [C.zlib_bound(4096)], True, max_src=4095, whole=True)
    assert rv[0] == INT32_MIN and outs[0] == bytes([FILL]) * C.zlib_bound(4096)
    d.close()


def test_malformed_streams_with_a_dictionary(tc, oracle_mod, golden, ref):
    """Every stream of tests/golden/zlib_malformed.npz decoded with a 4 KiB dictionary gets the verdict
    the reference gives with that dictionary (and, where that is a length, the bytes)."""
    dic, streams = C.malformed_cases(oracle_mod)
    d = tc.Dictionary(dic)
    rv, outs = _run(tc, d, [f for f, _ in streams], [c for _, c in streams], False)
    for i, (f, cap) in enumerate(streams):
        want, want_crc = int(golden.malformed_rv[i]), int(golden.malformed_crc[i])
        if ref is not None:
            w, dec = ref.decompress(dic, f, cap)
            assert (w, C.crc(dec)) == (want, want_crc), i
        assert int(rv[i]) == want, (i, rv[i], want)
        if want >= 0:
            assert C.crc(outs[i]) == want_crc, i
    d.close()


# ---------------------------------------------------------------- 5. the batch contract
BATCH_PLEN = 2048


@pytest.fixture(scope="module")
def batch_inputs(oracle_mod):
    host = oracle_mod.pagegen(4097, BATCH_PLEN, first=50, dist=0)
    return [host[i].tobytes() for i in range(4097)], oracle_mod.pagegen(1, 4096, first=49, dist=0)[0].tobytes()


@pytest.fixture(scope="module")
def first64_streams(tc, batch_inputs):
    pages, dic = batch_inputs
    d = tc.Dictionary(dic)
    _, streams = _run(tc, d, pages[:64], [C.zlib_bound(BATCH_PLEN)] * 64, True)
    d.close()
    return streams


@pytest.mark.parametrize("n", [1, 64, 4095, 4096, 4097])
def test_batches(tc, batch_inputs, first64_streams, ref, n):
    """1 to 4,097 pages of 2 KiB with a 4 KiB dictionary on the checked layout (every source and
    destination byte shift, random bytes around the sources, guards around every slot, the source arena
    unchanged): every page round-trips, and page i's bytes do not depend on the batch (the first 64
    streams of every count are those of the count-64 run, though the pages sit at other shifts)."""
    all_pages, dic = batch_inputs
    pages = all_pages[:n]
    d = tc.Dictionary(dic)
    rv, streams = _run(tc, d, pages, [C.zlib_bound(BATCH_PLEN)] * n, True)
    assert all(0 < r <= C.zlib_bound(BATCH_PLEN) for r in rv)
    k = min(n, 64)
    assert streams[:k] == first64_streams[:k], n
    rv2, outs = _run(tc, d, streams, [BATCH_PLEN] * n, False)
    bad = [i for i in range(n) if rv2[i] != BATCH_PLEN or outs[i] != pages[i]]
    assert not bad, (n, bad[:8])
    for i in sorted(set(range(min(n, 16))) | set(range(0, n, 257)) | {n - 1}):
        _restores(ref, dic, streams[i], pages[i])
    d.close()


def test_limited_output(tc, oracle_mod, ref):
    """Capacities of the stream size - 1, the size and the size + 1: 0 below the size and the same
    stream from the size on, and nothing is written outside the slot (the checked layout)."""
    O = oracle_mod
    for D, pairs in ((4096, [(4096, 4096), (4096, 65), (4096, 0), (4096, 16384)]), (64, [(64, 64), (64, 1)])):
        cases = C.all_cases(O, pairs)
        dic = cases[0][3]
        d = tc.Dictionary(dic)
        pages = [c[4] for c in cases]
        full, streams = _run(tc, d, pages, [C.zlib_bound(len(p)) for p in pages], True)
        assert all(r > 0 for r in full)
        for delta in (-1, 0, 1):
            caps = [int(r) + delta for r in full]
            rv, outs = _run(tc, d, pages, caps, True)
            if delta < 0:
                assert all(r == 0 for r in rv), (D, list(rv))
            else:
                assert [int(r) for r in rv] == [int(r) for r in full] and outs == streams, (D, delta)
        d.close()


# ---------------------------------------------------------------- 6. the failure hook
def test_fail_hook_covers_the_dictionary_compress_call(tc, oracle_mod, knobs):
    from tyche_amd import _lib
    d = tc.Dictionary(C.dict_of(oracle_mod, 4096))
    page = C.page_of(oracle_mod, 4096, 4096, "dist0")
    knobs(FAIL_COMPRESS_EVERY=1)
    with pytest.raises(_lib.DeviceError) as e:
        _run(tc, d, [page], [C.zlib_bound(len(page))], True)
    assert "199" in str(e.value)
    # counted once per launch: at every second count, exactly every second dictionary launch fails
    knobs(FAIL_COMPRESS_EVERY=2)
    failed = []
    for _ in range(4):
        try:
            _run(tc, d, [page], [C.zlib_bound(len(page))], True)
            failed.append(False)
        except _lib.DeviceError:
            failed.append(True)
    assert failed in ([True, False, True, False], [False, True, False, True]), failed
    d.close()


# ---------------------------------------------------------------- 7. host entry points
def _page(O, n, i=0):
    return C.gen(O, 0, 700 + 10 * i, n)


@pytest.fixture
def process_dict(tc, oracle_mod):
    dic = C.dict_of(oracle_mod, 4096)
    d = tc.Dictionary(dic)
    tc.use_zlib_dict(d)
    yield dic
    tc.use_zlib_dict(None)
    d.close()


def test_buffer_entry_points(tc, oracle_mod, ref, process_dict):
    """buffer__compress / buffer__decompress with a process-wide zlib dictionary: the stream needs the
    dictionary and the round trip holds; zstd through the same entry points is not touched by it."""
    from tyche_amd import buffer as B
    O = oracle_mod
    page = _page(O, 16384)
    b = B.new_buffer(page, id=1)
    rv, comp = B.buffer__compress(b, ZLIB, 1)
    assert rv == 0 and comp
    B.swap_data(b, comp)
    _needs_dictionary(ref, process_dict, B.buffer_bytes(b), page)
    assert B.buffer__decompress(b, ZLIB) == 0 and B.buffer_bytes(b) == page
    B.destroy(b)
    b = B.new_buffer(page, id=2)                              # the zstd slot is empty: a plain frame
    rv, comp = B.buffer__compress(b, 3, 1)
    assert rv == 0
    B.swap_data(b, comp)
    assert O.zstd_decompress(B.buffer_bytes(b), len(page)) == (len(page), page)
    B.destroy(b)


def test_buffers_batch_mixed_reach(tc, oracle_mod, ref):
    """tyche_buffers_compress / _decompress with a 32 KiB dictionary over a 16 KiB page (in reach) and
    a 40,000-byte page (out of reach): the page out of reach gets exactly the bytes it gets with no
    dictionary, the other a dictionary stream; both restore.  After tyche_zlib_use_dict(NULL) the
    streams are those of before the install."""
    from tyche_amd import buffer as B
    O = oracle_mod
    sizes = [16384, 40000]
    pages = [_page(O, n, i) for i, n in enumerate(sizes)]

    def compress_all():
        bufs = [B.new_buffer(p, id=i) for i, p in enumerate(pages)]
        rc, st, ptrs = B.buffers_compress(bufs, ZLIB, 1)
        assert rc == 0 and st == [0] * len(bufs)
        for b, p in zip(bufs, ptrs):
            B.swap_data(b, p)
        return bufs, [B.buffer_bytes(b) for b in bufs]

    bufs0, plain = compress_all()
    for b in bufs0:
        B.destroy(b)
    dic = C.dict_of(O, 32768)
    d = tc.Dictionary(dic)
    tc.use_zlib_dict(d)
    try:
        bufs, streams = compress_all()
        assert streams[1] == plain[1]
        assert streams[0] != plain[0]
        _needs_dictionary(ref, dic, streams[0], pages[0])
        rc, st = B.buffers_decompress(bufs, ZLIB)
        assert rc == 0 and st == [0] * len(bufs)
        assert [B.buffer_bytes(b) for b in bufs] == pages
        for b in bufs:
            B.destroy(b)
    finally:
        tc.use_zlib_dict(None)
        d.close()
    bufs1, again = compress_all()
    assert again == plain
    for b in bufs1:
        B.destroy(b)


def _host_calls(lib, _lib, host, plen):
    n = len(host)

    def compress_host():
        cap = C.zlib_bound(plen)
        out = np.full((n, cap + GUARD), FILL, np.uint8)
        srcs = (ctypes.c_void_p * n)(*[host[i].ctypes.data for i in range(n)])
        dsts = (ctypes.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
        slen, dcap = (ctypes.c_uint32 * n)(*([plen] * n)), (ctypes.c_uint32 * n)(*([cap] * n))
        res = (ctypes.c_int32 * n)(*([12345] * n))
        _lib.check(lib.tyche_compress_host(ZLIB, 1, n, srcs, slen, dsts, dcap, res), "tyche_compress_host")
        assert bool((out[:, cap:] == FILL).all()) and all(0 < r <= cap for r in res)
        return [out[i, :res[i]].tobytes() for i in range(n)]

    def decompress_host(streams):
        sb = [np.frombuffer(s, np.uint8).copy() for s in streams]
        out = np.full((n, plen + GUARD), FILL, np.uint8)
        srcs = (ctypes.c_void_p * n)(*[s.ctypes.data for s in sb])
        dsts = (ctypes.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
        slen, dcap = (ctypes.c_uint32 * n)(*[len(s) for s in streams]), (ctypes.c_uint32 * n)(*([plen] * n))
        res = (ctypes.c_int32 * n)(*([12345] * n))
        _lib.check(lib.tyche_decompress_host(ZLIB, n, srcs, slen, dsts, dcap, res), "tyche_decompress_host")
        assert bool((out[:, plen:] == FILL).all())
        return list(res), out[:, :plen]

    return compress_host, decompress_host


def test_host_batches_removal_and_hc(tc, oracle_mod, ref, knobs):
    """tyche_compress_host / tyche_decompress_host on 300 pages of 4 KiB with the dictionary; with
    ZLIB_HC=1 beside it the pages (all in reach) get the bytes they get with the knob off; after
    tyche_zlib_use_dict(NULL) the batch gives byte for byte the streams it gave before the install."""
    from tyche_amd import _lib
    O = oracle_mod
    lib = _lib.load()
    n, plen = 300, 4096
    host = O.pagegen(n, plen, first=11, dist=0)
    compress_host, decompress_host = _host_calls(lib, _lib, host, plen)
    before = compress_host()
    dic = O.pagegen(1, plen, first=10, dist=0)[0].tobytes()
    d = tc.Dictionary(dic)
    tc.use_zlib_dict(d)
    try:
        with_dict = compress_host()
        assert sum(map(len, with_dict)) < sum(map(len, before))
        for i in (0, n // 2, n - 1):
            _needs_dictionary(ref, dic, with_dict[i], host[i].tobytes())
        rv, out = decompress_host(with_dict)
        assert rv == [plen] * n and np.array_equal(out, host)
        knobs(ZLIB_HC=1)
        assert compress_host() == with_dict
        knobs(ZLIB_HC=0)
    finally:
        tc.use_zlib_dict(None)
        d.close()
    assert compress_host() == before
    rv, out = decompress_host(before)
    assert rv == [plen] * n and np.array_equal(out, host)
    knobs(ZLIB_HC=1)
    assert compress_host() != before                          # without a dictionary the knob is the HC encoder


def test_restore_queue_with_dictionary(tc, oracle_mod, ref, process_dict):
    from tyche_amd import _lib, buffer as B
    lib = _lib.load()
    page = _page(oracle_mod, 8192, 3)
    b = B.new_buffer(page, id=9)
    rv, comp = B.buffer__compress(b, ZLIB, 1)
    assert rv == 0
    B.swap_data(b, comp)
    _needs_dictionary(ref, process_dict, B.buffer_bytes(b), page)
    assert lib.tyche_restore_queue_start(8, 100) == 0
    try:
        assert lib.tyche_buffer_restore(b, ZLIB) == 0
    finally:
        lib.tyche_restore_queue_stop()
    assert B.buffer_bytes(b) == page
    B.destroy(b)


def test_env_dictionary_in_a_child_process(tmp_path, oracle_mod, ref):
    """TYCHE_ZLIB_DICT=<file>: a fresh child process does a Buffer round trip whose stream only a
    decoder with the dictionary restores."""
    O = oracle_mod
    dic = C.dict_of(O, 4096)
    path = tmp_path / "pages.dict"
    path.write_bytes(dic)
    page = _page(O, 16384, 5)
    (tmp_path / "page.bin").write_bytes(page)
    code = ("import sys\n"
            "from tyche_amd import buffer as B\n"
            f"page = open({str(tmp_path / 'page.bin')!r}, 'rb').read()\n"
            "b = B.new_buffer(page, id=1)\n"
            "rv, comp = B.buffer__compress(b, 2, 1)\n"
            "assert rv == 0, rv\n"
            "B.swap_data(b, comp)\n"
            f"open({str(tmp_path / 'stream.bin')!r}, 'wb').write(B.buffer_bytes(b))\n"
            "assert B.buffer__decompress(b, 2) == 0 and B.buffer_bytes(b) == page\n"
            "print('child ok')\n")
    env = dict(os.environ, TYCHE_ZLIB_DICT=str(path), PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr
    _needs_dictionary(ref, dic, (tmp_path / "stream.bin").read_bytes(), page)


# ---------------------------------------------------------------- 8. knob off
def test_no_dictionary_keeps_the_recorded_bytes(tc, oracle_mod):
    """With no zlib dictionary installed (after one was installed and removed), the plain zlib calls
    give the streams recorded in tests/golden/zlib_default_digests.json."""
    from tyche_amd import _lib
    from test_gpu_zlib_hc import compress_list, digest
    d = tc.Dictionary(C.dict_of(oracle_mod, 4096))
    tc.use_zlib_dict(d)
    tc.use_zlib_dict(None)
    d.close()
    assert not _lib.load().tyche_zlib_current_dict()
    with open(ZHC.DEFAULT_DIGESTS) as f:
        gold = json.load(f)
    _lib.clear_knob("ZLIB_HC")
    for group, pages in ZHC.knob_off_sets(oracle_mod).items():
        streams = compress_list(tc, pages, max_src_length=65535)[1]
        assert [len(s) for s in streams] == gold[group]["len"], group
        assert digest(streams) == gold[group]["sha"], group


# ---------------------------------------------------------------- 9. ratio
# device bytes / reference bytes (deflateSetDictionary + deflate, level 1, the same dictionary) per
# (page size, distribution), measured (profiles/zlib_dict_ratio.jsonl); the bound is the measurement
# + 0.5 %
ZLIB_DICT_PIN = {(4096, 0): 0.9926, (16384, 0): 0.9489, (4096, 1): 0.9823, (16384, 1): 0.9470, (4096, 2): 1.0621,
                 (16384, 2): 0.8973, (4096, 5): 0.9713, (16384, 5): 0.9521}


def _ratio_cell(tc, O, n, dist):
    dic, host = C.ratio_inputs(O, n, dist)
    d = tc.Dictionary(dic)
    pages = _dev(host)
    comp, clen = tc.compress_pages(pages, ZLIB, dictionary=d)
    out, rv = tc.decompress_pages(comp, clen, n, ZLIB, dictionary=d)
    _, plain = tc.compress_pages(pages, ZLIB)
    torch.cuda.synchronize()
    assert bool((rv == n).all()) and torch.equal(out, pages)
    d.close()
    return dic, host, int(clen.sum()), int(plain.sum())


def _gain(golden, cell):
    k = C.RATIO_CELLS.index(cell)
    return 1 - int(golden.ratio_ref[k]) / int(golden.ratio_ref_plain[k])


@pytest.mark.parametrize("cell", C.RATIO_CELLS, ids=lambda c: f"{c[0]}-dist{c[1]}")
def test_dictionary_pays(tc, oracle_mod, golden, cell):
    """48 pages and the 49th page's first 4 KiB as dictionary: in every cell where the reference's
    recorded gain is at least 2 % (six of the eight), the device's bytes with the dictionary are below
    its own without.  The other two cells are printed."""
    n, dist = cell
    _, _, ours, nodict = _ratio_cell(tc, oracle_mod, n, dist)
    print(f"{n} B dist {dist}: device {nodict} -> {ours} bytes with the dictionary; reference gain {_gain(golden, cell):.4f}")
    if _gain(golden, cell) >= 0.02:
        assert ours < nodict, (ours, nodict)


@pytest.mark.parametrize("cell", C.RATIO_CELLS, ids=lambda c: f"{c[0]}-dist{c[1]}")
def test_ratio_against_reference(tc, oracle_mod, golden, ref, cell):
    """Device bytes over the reference's level-1 bytes with the same dictionary (q_dict) and without
    (q_plain), printed (and appended to the file TYCHE_ZLIB_DICT_RATIO_LOG names, which is how
    profiles/zlib_dict_ratio.jsonl was taken), q_dict within the pinned measurement + 0.5 %."""
    n, dist = cell
    k = C.RATIO_CELLS.index(cell)
    dic, host, ours, nodict = _ratio_cell(tc, oracle_mod, n, dist)
    theirs, theirs_plain = int(golden.ratio_ref[k]), int(golden.ratio_ref_plain[k])
    if ref is not None:
        assert sum(len(ref.compress(dic, host[i].tobytes())) for i in range(len(host))) == theirs
    line = json.dumps({"page": n, "dist": dist, "dict": C.RATIO_DICT, "device": ours, "reference": theirs,
                       "device_no_dict": nodict, "reference_no_dict": theirs_plain,
                       "q_dict": round(ours / theirs, 4), "q_plain": round(nodict / theirs_plain, 4)})
    print(line)
    if os.environ.get("TYCHE_ZLIB_DICT_RATIO_LOG"):
        with open(os.environ["TYCHE_ZLIB_DICT_RATIO_LOG"], "a") as f:
            f.write(line + "\n")
    assert cell in ZLIB_DICT_PIN, "no pinned measurement for this cell"
    assert ours <= (ZLIB_DICT_PIN[cell] + 0.005) * theirs, (ours, theirs, ours / theirs)


# ---------------------------------------------------------------- 10. Python surface
def test_python_packed_roundtrip(tc, oracle_mod):
    """compress_pages(..., ZLIB, dictionary=d) -> pack_pages -> decompress_packed(..., dictionary=d)
    over 256 pages of 4 KiB; compress_pages_packed gives the same store; without the dictionary the
    store decodes to errors, not bytes."""
    O = oracle_mod
    n, plen = 256, 4096
    host = O.pagegen(n, plen, first=300, dist=1)
    d = tc.Dictionary(O.pagegen(1, plen, first=299, dist=1)[0].tobytes())
    pages = _dev(host)
    comp, clen = tc.compress_pages(pages, ZLIB, dictionary=d)
    arena = torch.zeros(n * tc.slot_size(plen, ZLIB), dtype=torch.uint8, device=DEV)
    offs, lens, state = tc.pack_pages(comp, clen, arena)
    out, rv = tc.decompress_packed(arena, offs, lens, plen, ZLIB, dictionary=d)
    torch.cuda.synchronize()
    assert int(state[0]) == int(state[1]) > 0
    assert bool((rv == plen).all()) and torch.equal(out, pages)
    arena2 = torch.zeros_like(arena)
    offs2, lens2, state2 = tc.compress_pages_packed(pages, arena2, chunk_pages=100, compressor_id=ZLIB, dictionary=d)
    torch.cuda.synchronize()
    assert torch.equal(offs2, offs) and torch.equal(lens2, lens) and torch.equal(arena2, arena)
    _, plain_rv = tc.decompress_packed(arena, offs, lens, plen, ZLIB)
    torch.cuda.synchronize()
    assert bool((plain_rv == C.Z_DATA).all())
    d.close()
