"""GPU tests of zstd with a shared raw-content dictionary (zstd_parse_dict_kernel and the encode passes
behind it, zstd_decode_dict_kernel, through the C ABI): round trips over every dictionary and page
size, the dictionary really being used, the reference's verdicts at the reach boundary and on the
malformed corpus, batches on both sides of the plain codec's split threshold, limited output, the
failure hook, the host entry points with a process-wide dictionary, and the ratio against the
reference.  Expected values come from tests/golden/zstd_dict.npz (recorded from the reference, zstd
1.1.2) and from the reference library itself where oracle/_ref is built.  Where it is not, a device
frame is restored by the device's dictionary decoder only: the independent evidence is then that
this decoder restores the reference-made frames of the golden file, gets its verdicts, and that the
plain restatement (oracle/zstd_oracle.c) refuses the frames that need the dictionary."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import zstd_dict_cases as C
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ZSTD = C.ZSTD
GUARD = 64
FILL = 0xAB
SENTINEL = 12345


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


def _layout(sizes):
    """16-byte aligned slots with a guard after each: (offsets, total bytes)."""
    offs, pos = np.zeros(len(sizes), np.int64), 0
    for i, n in enumerate(sizes):
        offs[i] = pos
        pos += (n + 15) // 16 * 16 + GUARD
    return offs, pos + GUARD


def _run(tc, d, srcs, caps, compress, max_src=None, max_cap=None, whole=False):
    """One ragged zstd launch over byte strings (d: the dictionary, None: the plain call), guard bytes
    after every slot, results preset to a sentinel: (results, outputs up to each result -- whole: up
    to each capacity --, True if no byte at or past any capacity was written)."""
    n = len(srcs)
    lens = [len(s) for s in srcs]
    soffs, stot = _layout(lens)
    buf = np.zeros(stot, np.uint8)
    for i, s in enumerate(srcs):
        buf[soffs[i]:soffs[i] + len(s)] = np.frombuffer(s, np.uint8)
    ooffs, otot = _layout(caps)
    d_src = torch.from_numpy(buf).to(DEV)
    d_out = torch.full((otot,), FILL, dtype=torch.uint8, device=DEV)
    d_rv = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    args = (d_src, torch.from_numpy(soffs).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV))
    d_caps, d_ooffs = torch.tensor(caps, dtype=torch.int32, device=DEV), torch.from_numpy(ooffs).to(DEV)
    if compress:
        tc.compress_ragged(*args, d_out, d_ooffs, d_caps, d_rv, max(lens + [1]) if max_src is None else max_src,
                           compressor_id=ZSTD, dictionary=d)
    else:
        tc.decompress_ragged(*args, d_caps, d_out, d_ooffs, d_rv, max_src_length=max(lens + [1]),
                             max_capacity=max(caps + [0]) if max_cap is None else max_cap, compressor_id=ZSTD,
                             dictionary=d)
    torch.cuda.synchronize()
    rv, out = d_rv.cpu().numpy(), d_out.cpu().numpy()
    clean = True
    for i in range(n):
        end = ooffs[i + 1] if i + 1 < n else otot
        clean &= bool((out[ooffs[i] + caps[i]:end] == FILL).all())
    take = (lambda i: caps[i]) if whole else (lambda i: max(int(rv[i]), 0))
    return rv, [out[ooffs[i]:ooffs[i] + take(i)].tobytes() for i in range(n)], clean


# ---------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("D", C.DS)
def test_roundtrip_all_sizes(tc, oracle_mod, golden, ref, D):
    """Every page length x page kind for this dictionary length: the device frame restores through
    ZSTD_decompress_usingDict to the page (reference library); the device's dictionary decoder gives
    (L, page) for it and for the reference's frame of the same page and dictionary (made now, or the
    golden file's); guard bytes past every capacity stay untouched in both directions."""
    O = oracle_mod
    cases = C.all_cases(O, [p for p in C.PAIRS if p[0] == D])
    dic = cases[0][3]
    d = tc.Dictionary(dic)
    pages = [c[4] for c in cases]
    lens = [len(p) for p in pages]
    rv, frames, clean = _run(tc, d, pages, [C.zstd_bound(n) for n in lens], True)
    assert clean, D
    for (_, L, k, _, page), r, f in zip(cases, rv, frames):
        assert 0 < r <= C.zstd_bound(L), (D, L, k, r)
        if ref is not None:
            assert ref.decompress(dic, f, L) == (L, page), (D, L, k)
    rv2, outs, clean = _run(tc, d, frames, lens, False)
    assert clean, D
    for (_, L, k, _, page), r, o in zip(cases, rv2, outs):
        assert r == L and o == page, (D, L, k, r)
    recorded = {(gd, gl, gk): f for gd, gl, gk, _, _, f in golden.rt_cases(O)}
    theirs = [(c, ref.compress(dic, c[4]) if ref is not None else recorded.get((c[0], c[1], c[2]))) for c in cases]
    theirs = [(c, f) for c, f in theirs if f is not None]
    assert theirs or D not in C.GOLDEN_DS
    if theirs:
        rv3, outs, clean = _run(tc, d, [f for _, f in theirs], [c[1] for c, _ in theirs], False)
        assert clean, D
        for (c, _), r, o in zip(theirs, rv3, outs):
            assert r == c[1] and o == c[4], (D, c[1], c[2], r)
    d.close()


# ---------------------------------------------------------------- 2. the dictionary is used
@pytest.mark.parametrize("L", C.USED_LS)
def test_dictionary_is_used(tc, oracle_mod, golden, ref, L):
    """D = 16384 random bytes, the page its last L bytes: the reference makes 16-19 bytes with the
    dictionary and L + 10 without; the device's frame is at most L/16 + 64 bytes, and neither the
    device's plain decoder nor ZSTD_decompress can restore it."""
    O = oracle_mod
    dic, page = C.used_case(L)
    k = C.USED_LS.index(L)
    assert 16 <= int(golden.used_ref[k]) <= 19 and int(golden.used_ref_plain[k]) == L + (9 if L < 256 else 10)
    d = tc.Dictionary(dic)
    rv, frames, clean = _run(tc, d, [page], [C.zstd_bound(L)], True)
    print(f"L {L}: device {rv[0]} bytes, reference {int(golden.used_ref[k])}")
    assert clean and 0 < rv[0] <= L // 16 + 64, (L, rv[0])
    rvp, _, clean = _run(tc, None, frames, [L], False)
    assert clean and rvp[0] < 0, rvp
    assert O.zstd_decompress(frames[0], L)[0] < 0                    # the restatement of ZSTD_decompress
    if ref is not None:
        assert ref.decompress_plain(frames[0], L)[0] < 0
        assert ref.decompress(dic, frames[0], L) == (L, page)
    rv2, outs, clean = _run(tc, d, frames, [L], False)
    assert clean and rv2[0] == L and outs[0] == page
    d.close()


# ---------------------------------------------------------------- 3. boundary verdicts
def test_boundary_verdicts(tc, oracle_mod, golden, ref):
    """Reference-made frames whose first match reaches dictionary byte 0 (offset == position + D):
    L and the bytes with the whole dictionary; negative with the dictionary minus its first byte;
    negative at a capacity of L - 1; INT32_MIN and an untouched destination where the page's
    capacity is above the launch's maximum."""
    O = oracle_mod
    for D, L, dic, page, frame in golden.boundary_cases(O):
        if ref is not None:
            frame = ref.compress(dic, page)
            assert ref.decompress(dic[1:], frame, L)[0] < 0 and ref.decompress(dic, frame, L) == (L, page)
        d = tc.Dictionary(dic)
        rv, outs, clean = _run(tc, d, [frame, frame], [L, L - 1], False)
        assert clean and rv[0] == L and outs[0] == page, (D, L, rv)
        assert rv[1] < 0 and rv[1] != -2 ** 31, (D, L, rv)
        rv, outs, clean = _run(tc, d, [frame], [L], False, max_cap=L - 1, whole=True)
        assert clean and rv[0] == -2 ** 31 and outs[0] == bytes([FILL]) * L, (D, L, rv)
        d.close()
        if D > 1:
            short = tc.Dictionary(dic[1:])
            rv, _, clean = _run(tc, short, [frame], [L], False)
            assert clean and rv[0] < 0, (D, L, rv)
            short.close()


def test_malformed_frames_with_a_dictionary(tc, oracle_mod, golden, ref):
    """Every frame of tests/golden/zstd_malformed.npz decoded with a 4 KiB dictionary keeps the sign
    ZSTD_decompress_usingDict gives it with that dictionary (and, where that is a size, the size and
    the bytes)."""
    O = oracle_mod
    dic, frames = C.malformed_cases(O)
    d = tc.Dictionary(dic)
    rv, outs, clean = _run(tc, d, [f for f, _ in frames], [c for _, c in frames], False)
    assert clean
    for i, (f, cap) in enumerate(frames):
        want, want_crc = int(golden.malformed_rv[i]), int(golden.malformed_crc[i])
        if ref is not None:
            want, dec = ref.decompress(dic, f, cap)
            want_crc = C.crc(dec)
        assert (rv[i] < 0) == (want < 0), (i, rv[i], want)
        if want >= 0:
            assert rv[i] == want and C.crc(outs[i]) == want_crc, (i, rv[i], want)
    d.close()


# ---------------------------------------------------------------- 4. batches
BATCH_PLEN = 4096


@pytest.fixture(scope="module")
def batch_inputs(oracle_mod):
    host = oracle_mod.pagegen(4097, BATCH_PLEN, first=50, dist=0)
    return host, oracle_mod.pagegen(1, BATCH_PLEN, first=49, dist=0)[0].tobytes()


def _compress_batch(tc, host, d):
    comp, clen = tc.compress_pages(torch.from_numpy(host).to(DEV), ZSTD, dictionary=d)
    torch.cuda.synchronize()
    return comp, clen


@pytest.fixture(scope="module")
def first64_frames(tc, batch_inputs):
    """The frames of the count-64 run, which every other count's first pages are compared with."""
    host, dic = batch_inputs
    d = tc.Dictionary(dic)
    comp, clen = _compress_batch(tc, host[:64], d)
    d.close()
    ch, lh = comp.cpu().numpy(), clen.cpu().numpy()
    return [ch[i, :lh[i]].tobytes() for i in range(64)]


@pytest.mark.parametrize("n", [1, 64, 4095, 4096, 4097])
def test_batches(tc, batch_inputs, first64_frames, ref, n):
    """1, 64, 4,095, 4,096 and 4,097 pages of 4 KiB with a 4 KiB dictionary, on both sides of
    ZSTD_SPLIT_MIN where the plain codec changes kernels: every page round-trips, and page i's result
    and bytes do not depend on the batch size (the first 64 frames of every count, 4,097 included,
    are those of the count-64 run)."""
    host_all, dic = batch_inputs
    host = host_all[:n]
    d = tc.Dictionary(dic)
    comp, clen = _compress_batch(tc, host, d)
    out, rv = tc.decompress_pages(comp, clen, BATCH_PLEN, ZSTD, dictionary=d)
    torch.cuda.synchronize()
    ch, lh, oh, rh = comp.cpu().numpy(), clen.cpu().numpy(), out.cpu().numpy(), rv.cpu().numpy()
    assert bool((lh > 0).all()) and bool((lh <= C.zstd_bound(BATCH_PLEN)).all())
    bad = np.nonzero((rh != BATCH_PLEN) | (oh != host).any(axis=1))[0]
    assert bad.size == 0, (n, bad[:8], rh[bad[:8]])
    if ref is not None:
        for i in sorted(set(range(min(n, 64))) | set(range(0, n, 61)) | {n - 1}):
            assert ref.decompress(dic, ch[i, :lh[i]].tobytes(), BATCH_PLEN) == (BATCH_PLEN, host[i].tobytes()), (n, i)
    k = min(n, 64)
    assert [ch[i, :lh[i]].tobytes() for i in range(k)] == first64_frames[:k], n
    d.close()


# ---------------------------------------------------------------- 5. limited output
def test_limited_output(tc, oracle_mod, ref):
    """Capacities of the frame size, one below and 0: every result is the size (of the same frame,
    which restores to the page) or 0 -- the plain encoder's capacity decisions rest on bounds, so a
    frame that would just fit may be refused --, never a size above the capacity, 0 at a capacity of
    0, and nothing is written at or past the capacity."""
    O = oracle_mod
    for D, pairs in ((4096, [(4096, 4096), (4096, 65), (4096, 0), (4096, 16384)]), (64, [(64, 64), (64, 1)])):
        cases = C.all_cases(O, pairs)
        dic = cases[0][3]
        d = tc.Dictionary(dic)
        pages = [c[4] for c in cases]
        full, frames, _ = _run(tc, d, pages, [C.zstd_bound(len(p)) for p in pages], True)
        assert bool((full > 0).all())
        for caps in ([int(r) for r in full], [int(r) - 1 for r in full], [0] * len(cases)):
            rv, outs, clean = _run(tc, d, pages, caps, True)
            assert clean, (D, caps)
            assert all(r == 0 or (r == w and r <= cap) for r, w, cap in zip(rv, full, caps)), (D, list(rv), list(full), caps)
            kept = [i for i, r in enumerate(rv) if r > 0]
            print(f"D {D} caps {caps[:4]}...: {len(kept)} of {len(caps)} frames fit")
            if kept:
                rv2, back, clean = _run(tc, d, [outs[i] for i in kept], [len(pages[i]) for i in kept], False)
                assert clean
                for i, r, o in zip(kept, rv2, back):
                    assert outs[i] == frames[i], (D, i)
                    assert r == len(pages[i]) and o == pages[i], (D, i, r)
                    if ref is not None:
                        assert ref.decompress(dic, outs[i], len(pages[i])) == (len(pages[i]), pages[i])
        d.close()


# ---------------------------------------------------------------- 6. the failure hook
def test_fail_hook_covers_the_dictionary_compress_call(tc, oracle_mod, knobs):
    from tyche_amd import _lib
    d = tc.Dictionary(C.dict_of(oracle_mod, 4096))
    page = C.page_of(oracle_mod, 4096, 4096, "dist0")
    knobs(FAIL_COMPRESS_EVERY=1)
    with pytest.raises(_lib.DeviceError) as e:
        _run(tc, d, [page], [C.zstd_bound(len(page))], True)
    assert "199" in str(e.value)
    d.close()


# ---------------------------------------------------------------- 7. host entry points
def _page(O, n, i=0):
    return C.gen(O, 0, 700 + 10 * i, n)


def _needs_dictionary(O, ref, dic, frame, page):
    """A dictionary frame: plain ZSTD_decompress refuses it, ZSTD_decompress_usingDict restores it."""
    assert O.zstd_decompress(frame, len(page))[0] < 0
    if ref is not None:
        assert ref.decompress_plain(frame, len(page))[0] < 0
        assert ref.decompress(dic, frame, len(page)) == (len(page), page)


@pytest.fixture
def process_dict(tc, oracle_mod):
    dic = C.dict_of(oracle_mod, 4096)
    d = tc.Dictionary(dic)
    tc.use_zstd_dict(d)
    yield dic
    tc.use_zstd_dict(None)
    d.close()


def test_buffer_entry_points(tc, oracle_mod, ref, process_dict):
    """buffer__compress / buffer__decompress with a process-wide zstd dictionary: the frame needs the
    dictionary and the round trip holds; LZ4 through the same entry points is not touched by it."""
    from tyche_amd import buffer as B
    O = oracle_mod
    page = _page(O, 16384)
    b = B.new_buffer(page, id=1)
    rv, comp = B.buffer__compress(b, ZSTD, 1)
    assert rv == 0 and comp
    B.swap_data(b, comp)
    _needs_dictionary(O, ref, process_dict, B.buffer_bytes(b), page)
    assert B.buffer__decompress(b, ZSTD) == 0 and B.buffer_bytes(b) == page
    B.destroy(b)
    b = B.new_buffer(page, id=2)                              # the LZ4 slot is empty: a plain block
    rv, comp = B.buffer__compress(b, 1, 1)
    assert rv == 0
    B.swap_data(b, comp)
    assert O.lz4_decompress(B.buffer_bytes(b), len(page)) == (len(page), page)
    B.destroy(b)


def test_buffers_batch_mixed_reach(tc, oracle_mod, ref):
    """tyche_buffers_compress / _decompress with a 32 KiB dictionary over a 16 KiB page (in reach) and
    a 40,000-byte page (out of reach): the page out of reach gets exactly the bytes it gets with no
    dictionary, the other a dictionary frame; both restore.  After tyche_zstd_use_dict(NULL) the
    frames are those of before the install."""
    from tyche_amd import buffer as B
    O = oracle_mod
    sizes = [16384, 40000]
    pages = [_page(O, n, i) for i, n in enumerate(sizes)]

    def compress_all():
        bufs = [B.new_buffer(p, id=i) for i, p in enumerate(pages)]
        rc, st, ptrs = B.buffers_compress(bufs, ZSTD, 1)
        assert rc == 0 and st == [0] * len(bufs)
        for b, p in zip(bufs, ptrs):
            B.swap_data(b, p)
        return bufs, [B.buffer_bytes(b) for b in bufs]

    bufs0, plain = compress_all()
    for b in bufs0:
        B.destroy(b)
    dic = C.dict_of(O, 32768)
    d = tc.Dictionary(dic)
    tc.use_zstd_dict(d)
    try:
        bufs, frames = compress_all()
        assert frames[1] == plain[1]
        assert frames[0] != plain[0]
        _needs_dictionary(O, ref, dic, frames[0], pages[0])
        rc, st = B.buffers_decompress(bufs, ZSTD)
        assert rc == 0 and st == [0] * len(bufs)
        assert [B.buffer_bytes(b) for b in bufs] == pages
        for b in bufs:
            B.destroy(b)
    finally:
        tc.use_zstd_dict(None)
        d.close()
    bufs1, again = compress_all()
    assert again == plain
    for b in bufs1:
        B.destroy(b)


def test_host_batches_and_removal(tc, oracle_mod, ref):
    """tyche_compress_host / tyche_decompress_host on 300 pages of 4 KiB with the dictionary; after
    tyche_zstd_use_dict(NULL) the batch gives byte for byte the frames it gave before the install."""
    from tyche_amd import _lib
    O = oracle_mod
    lib = _lib.load()
    n, plen = 300, 4096
    host = O.pagegen(n, plen, first=11, dist=0)

    def compress_host():
        cap = C.zstd_bound(plen)
        out = np.full((n, cap + GUARD), FILL, np.uint8)
        srcs = (ctypes.c_void_p * n)(*[host[i].ctypes.data for i in range(n)])
        dsts = (ctypes.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
        slen, dcap = (ctypes.c_uint32 * n)(*([plen] * n)), (ctypes.c_uint32 * n)(*([cap] * n))
        res = (ctypes.c_int32 * n)(*([SENTINEL] * n))
        _lib.check(lib.tyche_compress_host(ZSTD, 1, n, srcs, slen, dsts, dcap, res), "tyche_compress_host")
        assert bool((out[:, cap:] == FILL).all()) and all(0 < r <= cap for r in res)
        return [out[i, :res[i]].tobytes() for i in range(n)]

    def decompress_host(frames):
        sb = [np.frombuffer(s, np.uint8).copy() for s in frames]
        out = np.full((n, plen + GUARD), FILL, np.uint8)
        srcs = (ctypes.c_void_p * n)(*[s.ctypes.data for s in sb])
        dsts = (ctypes.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
        slen, dcap = (ctypes.c_uint32 * n)(*[len(s) for s in frames]), (ctypes.c_uint32 * n)(*([plen] * n))
        res = (ctypes.c_int32 * n)(*([SENTINEL] * n))
        _lib.check(lib.tyche_decompress_host(ZSTD, n, srcs, slen, dsts, dcap, res), "tyche_decompress_host")
        assert bool((out[:, plen:] == FILL).all())
        return list(res), out[:, :plen]

    before = compress_host()
    dic = O.pagegen(1, plen, first=10, dist=0)[0].tobytes()
    d = tc.Dictionary(dic)
    tc.use_zstd_dict(d)
    try:
        with_dict = compress_host()
        assert sum(map(len, with_dict)) < sum(map(len, before))
        for i in (0, n // 2, n - 1):
            _needs_dictionary(O, ref, dic, with_dict[i], host[i].tobytes())
        rv, out = decompress_host(with_dict)
        assert rv == [plen] * n and np.array_equal(out, host)
    finally:
        tc.use_zstd_dict(None)
        d.close()
    assert compress_host() == before
    rv, out = decompress_host(before)
    assert rv == [plen] * n and np.array_equal(out, host)


def test_restore_queue_with_dictionary(tc, oracle_mod, ref, process_dict):
    from tyche_amd import _lib, buffer as B
    lib = _lib.load()
    page = _page(oracle_mod, 8192, 3)
    b = B.new_buffer(page, id=9)
    rv, comp = B.buffer__compress(b, ZSTD, 1)
    assert rv == 0
    B.swap_data(b, comp)
    _needs_dictionary(oracle_mod, ref, process_dict, B.buffer_bytes(b), page)
    assert lib.tyche_restore_queue_start(8, 100) == 0
    try:
        assert lib.tyche_buffer_restore(b, ZSTD) == 0
    finally:
        lib.tyche_restore_queue_stop()
    assert B.buffer_bytes(b) == page
    B.destroy(b)


def test_env_dictionary_in_a_child_process(tmp_path, oracle_mod, ref):
    """TYCHE_ZSTD_DICT=<file>: a fresh child process does a Buffer round trip whose frame only the
    dictionary decoder restores."""
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
            "rv, comp = B.buffer__compress(b, 3, 1)\n"
            "assert rv == 0, rv\n"
            "B.swap_data(b, comp)\n"
            f"open({str(tmp_path / 'frame.bin')!r}, 'wb').write(B.buffer_bytes(b))\n"
            "assert B.buffer__decompress(b, 3) == 0 and B.buffer_bytes(b) == page\n"
            "print('child ok')\n")
    env = dict(os.environ, TYCHE_ZSTD_DICT=str(path), PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr
    _needs_dictionary(O, ref, dic, (tmp_path / "frame.bin").read_bytes(), page)


# ---------------------------------------------------------------- 8, 9. ratio
# device bytes / reference bytes (ZSTD_compress_usingDict, level 1, the same dictionary) per (page
# size, distribution), measured (profiles/zstd_dict_ratio.jsonl); the bound is the measurement + 0.5 %
# 
ZSTD_DICT_PIN = {(4096, 0): 0.9960, (16384, 0): 1.0082, (4096, 1): 0.9975, (16384, 1): 1.0115, (4096, 2): 1.1885,
                 (16384, 2): 1.0474, (4096, 5): 0.9582, (16384, 5): 0.9778}


def _ratio_cell(tc, O, n, dist):
    dic, host = C.ratio_inputs(O, n, dist)
    d = tc.Dictionary(dic)
    pages = torch.from_numpy(host).to(DEV)
    comp, clen = tc.compress_pages(pages, ZSTD, dictionary=d)
    out, rv = tc.decompress_pages(comp, clen, n, ZSTD, dictionary=d)
    _, plain = tc.compress_pages(pages, ZSTD)
    torch.cuda.synchronize()
    assert bool((rv == n).all()) and torch.equal(out, pages)
    d.close()
    return dic, host, int(clen.sum()), int(plain.sum())


@pytest.mark.parametrize("cell", [c for c in C.RATIO_CELLS if c[1] != 5], ids=lambda c: f"{c[0]}-dist{c[1]}")
def test_dictionary_pays(tc, oracle_mod, cell):
    """dist 0, 1, 2 at 4 and 16 KiB, 48 pages, the 49th page's first 4 KiB as dictionary: the device's
    bytes with the dictionary are strictly below its own without (the reference alone satisfies this
    in every such cell: tests/golden/zstd_dict.npz, checked by test_zstd_dict_abi.py)."""
    n, dist = cell
    _, _, ours, nodict = _ratio_cell(tc, oracle_mod, n, dist)
    print(f"{n} B dist {dist}: device {nodict} -> {ours} bytes with the dictionary")
    assert ours < nodict, (ours, nodict)


@pytest.mark.parametrize("cell", C.RATIO_CELLS, ids=lambda c: f"{c[0]}-dist{c[1]}")
def test_ratio_against_reference(tc, oracle_mod, golden, ref, cell):
    """The same cells plus dist 5: device bytes over the reference's ZSTD_compress_usingDict level 1
    bytes with the same dictionary, printed (and appended to the file TYCHE_ZSTD_DICT_RATIO_LOG names,
    which is how profiles/zstd_dict_ratio.jsonl was taken), within the pinned measurement + 0.5 %."""
    n, dist = cell
    dic, host, ours, nodict = _ratio_cell(tc, oracle_mod, n, dist)
    theirs = int(golden.ratio_ref[C.RATIO_CELLS.index(cell)])
    if ref is not None:
        assert sum(len(ref.compress(dic, host[i].tobytes())) for i in range(len(host))) == theirs
    line = json.dumps({"page": n, "dist": dist, "dict": C.RATIO_DICT, "device": ours, "reference": theirs,
                       "device_no_dict": nodict, "reference_no_dict": int(golden.ratio_ref_plain[C.RATIO_CELLS.index(cell)]),
                       "ratio": round(ours / theirs, 4)})
    print(line)
    if os.environ.get("TYCHE_ZSTD_DICT_RATIO_LOG"):
        with open(os.environ["TYCHE_ZSTD_DICT_RATIO_LOG"], "a") as f:
            f.write(line + "\n")
    assert cell in ZSTD_DICT_PIN, "no pinned measurement for this cell"
    assert ours <= (ZSTD_DICT_PIN[cell] + 0.005) * theirs, (ours, theirs, ours / theirs)


# ---------------------------------------------------------------- 10. Python surface
def test_python_packed_roundtrip(tc, oracle_mod):
    """compress_pages(..., ZSTD, dictionary=d) -> pack_pages -> decompress_packed(..., dictionary=d)
    over 256 pages of 4 KiB; compress_pages_packed gives the same store."""
    O = oracle_mod
    n, plen = 256, 4096
    host = O.pagegen(n, plen, first=300, dist=1)
    d = tc.Dictionary(O.pagegen(1, plen, first=299, dist=1)[0].tobytes())
    pages = torch.from_numpy(host).to(DEV)
    comp, clen = tc.compress_pages(pages, ZSTD, dictionary=d)
    arena = torch.zeros(n * tc.slot_size(plen, ZSTD), dtype=torch.uint8, device=DEV)
    offs, lens, state = tc.pack_pages(comp, clen, arena)
    out, rv = tc.decompress_packed(arena, offs, lens, plen, ZSTD, dictionary=d)
    torch.cuda.synchronize()
    assert int(state[0]) == int(state[1]) > 0
    assert bool((rv == plen).all()) and torch.equal(out, pages)
    arena2 = torch.zeros_like(arena)
    offs2, lens2, state2 = tc.compress_pages_packed(pages, arena2, chunk_pages=100, compressor_id=ZSTD, dictionary=d)
    torch.cuda.synchronize()
    assert torch.equal(offs2, offs) and torch.equal(lens2, lens) and torch.equal(arena2, arena)
    plain_out, plain_rv = tc.decompress_packed(arena, offs, lens, plen, ZSTD)   # without the dictionary: errors, not bytes
    torch.cuda.synchronize()
    assert bool((plain_rv < 0).any())
    d.close()
