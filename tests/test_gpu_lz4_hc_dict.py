"""GPU tests of the high-compression LZ4 dictionary encoder (LZ4_HC_DICT=1,
tyche_amd/csrc/lz4_encode_hc_dict.hip): the kernel's results and bytes equal the host emulator's
(tools/lz4_hc_dict_emul.cpp, the same lz4_hc_core.h; test_lz4_hc_dict_emul.py holds that to the
block format, the dictionary's reach, the limited-output contract and the ratio) through every
compress entry point a dictionary reaches; the batch contract on the checked layout of
batch_layout.py; the streams restore through the dictionary decoders; and with the knob off, or
LZ4_HC alone beside a dictionary, the bytes are the default dictionary encoder's."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import batch_layout as BL
import lz4_dict_cases as DC
import lz4_hc_cases as HC
import lz4_hc_dict_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INT32_MIN = -2 ** 31
LZ4 = 1


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return codec


@pytest.fixture(scope="module")
def emul():
    return C.load_emul()


@pytest.fixture(scope="module")
def plain():
    return HC.load_emul()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def compress_rows(tc, pages, d=None):
    """compress_pages on equally long byte strings: the streams as bytes."""
    host = np.stack([np.frombuffer(p, np.uint8) for p in pages])
    comp, clen = tc.compress_pages(_dev(host), dictionary=d)
    torch.cuda.synchronize()
    lh, ch = clen.cpu().numpy(), comp.cpu().numpy()
    return [ch[i, :max(int(lh[i]), 0)].tobytes() for i in range(len(pages))]


def _groups(cases):
    """One launch per dictionary (lz4_dict_cases.dict_key) and page length."""
    g = {}
    for c in cases:
        g.setdefault((DC.dict_key(c[0], c[2]), len(c[4])), []).append(c)
    return g


@pytest.fixture(scope="module")
def streams_4k(tc, oracle_mod):
    """The device's LZ4_HC_DICT=1 streams of every kind at (4096, 4096): (kind, dictionary, page, stream)."""
    from tyche_amd import _lib
    out = []
    _lib.set_knob("LZ4_HC_DICT", 1)
    try:
        for (key, _), cs in _groups(C.cases(oracle_mod, [(4096, 4096)])).items():
            d = tc.Lz4Dict(cs[0][3])
            got = compress_rows(tc, [c[4] for c in cs], d)
            d.close()
            out += [(c[2], c[3], c[4], s) for c, s in zip(cs, got)]
    finally:
        _lib.clear_knob("LZ4_HC_DICT")
    return out


@pytest.mark.parametrize("pair", C.GPU_PAIRS, ids=lambda p: f"D{p[0]}-L{p[1]}")
def test_kernel_bytes_equal_the_emulator(tc, oracle_mod, emul, knobs, pair):
    """Every page kind, one launch per dictionary.  (32768, 32768) and (64, 65472) put a 16-bit
    position at 65,535 and hold two pages per CU by LDS; (63, 4096) is the dictionary the encoder
    cannot see; (65, 13) the shortest page with a match."""
    knobs(LZ4_HC_DICT=1)
    n = 0
    for (key, _), cs in _groups(C.cases(oracle_mod, [pair])).items():
        d = tc.Lz4Dict(cs[0][3])
        got = compress_rows(tc, [c[4] for c in cs], d)
        d.close()
        for c, s in zip(cs, got):
            r, want = emul(c[3], c[4])
            assert len(s) == r and s == want, (pair, c[2], len(s), r)
            n += 1
    assert n == len(DC.KINDS)


def test_waves_loop(tc, oracle_mod, emul, knobs):
    """300 mixed 4 KiB pages with a 4 KiB dictionary in one launch held to one resident page per CU,
    at every source alignment (a ragged launch): the seed is installed afresh for every page and the
    dictionary image of the page's own shift is used."""
    knobs(LZ4_HC_DICT=1, LZ4_HC_DICT_PAGES_PER_CU=1)
    host = HC.mixed_4k_pages(oracle_mod, 300)
    dic = DC.dict_of(oracle_mod, 4096, "dist0")
    pages = [p.tobytes() for p in host]
    caps = [C.lz4_bound(4096)] * len(pages)
    lay = BL.build(pages, caps, [i % 16 for i in range(len(pages))], [(7 * i) % 16 for i in range(len(pages))], ("random", 9))
    d = tc.Lz4Dict(dic)
    rv, outs, _ = run_layout(tc, lay, d)
    d.close()
    for i, p in enumerate(pages):
        assert (rv[i], outs[i]) == emul(dic, p), i


def run_layout(tc, lay, d, max_src_length=None):
    """A checked layout through compress_ragged with a dictionary: (results, outputs, arena), guards and source verified."""
    d_src, d_out = _dev(lay.src), _dev(lay.out)
    d_rv = torch.full((lay.count,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    if max_src_length is None:
        max_src_length = max([int(x) for x in lay.src_lengths] + [1])
    tc.compress_ragged(d_src, _dev(lay.src_offsets), _dev(lay.src_lengths), d_out, _dev(lay.dst_offsets), _dev(lay.caps),
                       d_rv, max_src_length=max_src_length, dictionary=d)
    torch.cuda.synchronize()
    rv, out = d_rv.cpu().numpy(), d_out.cpu().numpy()
    BL.check(out, d_src.cpu().numpy(), lay)
    return [int(x) for x in rv], BL.outputs(out, rv, lay), out


def test_ragged_batch_contract(tc, oracle_mod, emul, knobs):
    """Lengths 0, 1, 12, 13, 100, 4096, 16384 and 61440 (the reach of a 4 KiB dictionary) at capacities
    of the stream's size, one less, one more and 0, every source and destination alignment, guards
    around every slot, neighbours' bytes poisoned (random gaps): results and bytes are the emulator's,
    nothing outside a slot or in the source changes.  Then a page above a declared maximum of 20000
    gets INT32_MIN and its slot stays as it was."""
    O = oracle_mod
    knobs(LZ4_HC_DICT=1)
    dic = DC.dict_of(O, 4096, "dist1")
    d = tc.Lz4Dict(dic)
    lens = (0, 1, 12, 13, 100, 4096, 16384, 61440)
    base = O.pagegen(2, 32768, seed=31, first=8, dist=1).tobytes()
    pages, caps, want = [], [], []
    for L in lens:
        p = base[:L]
        full, stream = emul(dic, p)
        for cap in (full, full - 1, full + 1, 0):
            pages.append(p)
            caps.append(cap)
            want.append((full, stream) if cap >= full else (0, b""))
    for rnd in range(2):
        n = len(pages)
        ss = [(5 * i + rnd * 7) % 16 for i in range(n)]
        ds = [(3 * i + rnd * 11 + 1) % 16 for i in range(n)]
        assert len(set(ss)) == 16 and len(set(ds)) == 16
        lay = BL.build(pages, caps, ss, ds, ("random", 40 + rnd))
        rv, outs, _ = run_layout(tc, lay, d)
        for i in range(n):
            assert (rv[i], outs[i]) == want[i], (rnd, len(pages[i]), caps[i], rv[i], want[i][0])
    sel = [base[:100], base[:20000], base[:20001], base[:4096]]
    wants = [emul(dic, p) for p in sel]
    bound = C.lz4_bound(20001)
    lay = BL.build(sel, [bound] * 4, [1, 2, 3, 4], [5, 6, 7, 8], "ff")
    rv, outs, out = run_layout(tc, lay, d, max_src_length=20000)
    d.close()
    a = int(lay.dst_offsets[2])
    assert rv[2] == INT32_MIN and bool((out[a:a + bound] == lay.fill).all())
    for i in (0, 1, 3):
        assert (rv[i], outs[i]) == wants[i], i


def test_streams_restore(tc, oracle_mod, streams_4k):
    """The (4096, 4096) streams restore through decompress_pages(dictionary=d) and, where the
    reference library is built, through its LZ4_decompress_safe_usingDict.  With another dictionary
    of the same length the size is still right and the bytes differ on a page whose stream reaches
    the dictionary: the documented caveat of dictionary streams, not a new promise."""
    O = oracle_mod
    ref = DC.ref_or_none(O)
    reached_and_differs = 0
    for kind, dic, page, stream in streams_4k:
        d, wrong = tc.Lz4Dict(dic), tc.Lz4Dict(bytes(b ^ 0x5A for b in dic))
        slots = np.zeros((1, len(stream) + 16), np.uint8)
        slots[0, :len(stream)] = np.frombuffer(stream, np.uint8)
        clen = torch.tensor([len(stream)], dtype=torch.int32, device=DEV)
        out, rv = tc.decompress_pages(_dev(slots), clen, 4096, dictionary=d)
        out2, rv2 = tc.decompress_pages(_dev(slots), clen, 4096, dictionary=wrong)
        torch.cuda.synchronize()
        d.close()
        wrong.close()
        assert int(rv[0]) == 4096 and out.cpu().numpy()[0].tobytes() == page, kind
        if ref is not None:
            assert ref.decompress(dic, stream, 4096) == (4096, page), kind
        assert int(rv2[0]) == 4096, kind
        if DC.max_reach(stream) > 0:
            reached_and_differs += out2.cpu().numpy()[0].tobytes() != page
    assert reached_and_differs >= 1


def test_the_knob(tc, oracle_mod, knobs):
    """48 dist-0 pages of 4 KiB with a 4 KiB dictionary: the total with LZ4_HC_DICT=1 is strictly below
    the total without it and below plain LZ4_HC=1 without a dictionary; after tyche_clear_knob, and
    with the knob at 0, the bytes are those of the first run; LZ4_HC=1 alone beside the dictionary
    still gives the default dictionary encoder's bytes."""
    from tyche_amd import _lib
    dic, host = C.ratio_inputs(oracle_mod, 0)
    pages = [p.tobytes() for p in host]
    d = tc.Lz4Dict(dic)
    try:
        before = compress_rows(tc, pages, d)
        _lib.set_knob("LZ4_HC_DICT", 1)
        both = compress_rows(tc, pages, d)
        _lib.clear_knob("LZ4_HC_DICT")
        cleared = compress_rows(tc, pages, d)
        _lib.set_knob("LZ4_HC_DICT", 0)
        zero = compress_rows(tc, pages, d)
        _lib.clear_knob("LZ4_HC_DICT")
        _lib.set_knob("LZ4_HC", 1)
        hc_beside = compress_rows(tc, pages, d)
        hc_plain = compress_rows(tc, pages)
    finally:
        _lib.clear_knob("LZ4_HC_DICT")
        _lib.clear_knob("LZ4_HC")
        d.close()
    D0, M, P = sum(map(len, before)), sum(map(len, both)), sum(map(len, hc_plain))
    print(f"default dictionary encoder {D0} B, LZ4_HC_DICT=1 {M} B, plain LZ4_HC=1 {P} B")
    assert M < D0 and M < P, (D0, M, P)
    assert cleared == before and zero == before
    assert hc_beside == before


def _compress_host(lib, pages, caps):
    n = len(pages)
    src = [np.frombuffer(p, np.uint8).copy() for p in pages]
    out = [np.full(c + HC.GUARD, HC.FILL, np.uint8) for c in caps]
    vp, u32 = ctypes.c_void_p * n, ctypes.c_uint32 * n
    res = (ctypes.c_int32 * n)()
    rc = lib.tyche_compress_host(LZ4, 1, n, vp(*[s.ctypes.data for s in src]), u32(*[len(p) for p in pages]),
                                 vp(*[o.ctypes.data for o in out]), u32(*caps), res)
    for o, c in zip(out, caps):
        assert bool((o[c:] == HC.FILL).all()), "wrote past a capacity"
    return rc, [o[:max(r, 0)].tobytes() for o, r in zip(out, res)]


def test_host_entry_points(tc, oracle_mod, emul, plain, knobs):
    """A process-wide 4 KiB dictionary and the knob: of a 16 KiB and a 65,000-byte page in one
    tyche_compress_host call the first has the emulator's HC-dictionary bytes, the second, beyond the
    reach, the bytes it has without the knob (with LZ4_HC=1 beside it: the plain HC emulator's);
    buffer__compress -> buffer__decompress and tyche_buffers_compress -> tyche_buffers_decompress
    give the emulator's bytes and the pages back; tyche_lz4_use_dict(NULL) leaves the process plain."""
    from tyche_amd import _lib, buffer as B
    O = oracle_mod
    lib = _lib.load()
    data = O.pagegen(4, 32768, seed=5, first=40, dist=0).tobytes()
    pages = [data[:16384], data[20000:85000]]
    caps = [C.lz4_bound(len(p)) for p in pages]
    dic = O.pagegen(1, 4096, seed=5, first=39, dist=0).tobytes()
    small = [data[i * 777:i * 777 + n] for i, n in enumerate([4096, 8192, 4097, 1000, 65, 13, 1, 12000])]
    rc, no_dict = _compress_host(lib, pages, caps)
    assert rc == 0, _lib.last_error()
    d = tc.Lz4Dict(dic)
    B.use_dict(d)
    try:
        rc, knob_off = _compress_host(lib, pages, caps)
        assert rc == 0, _lib.last_error()
        knobs(LZ4_HC_DICT=1)
        rc, on = _compress_host(lib, pages, caps)
        assert rc == 0, _lib.last_error()
        assert on[0] == emul(dic, pages[0])[1] and on[0] != knob_off[0]
        assert on[1] == knob_off[1] == no_dict[1]
        knobs(LZ4_HC=1)
        rc, with_hc = _compress_host(lib, pages, caps)
        assert rc == 0, _lib.last_error()
        assert with_hc[0] == on[0] and with_hc[1] == plain(pages[1])[1]
        _lib.clear_knob("LZ4_HC")

        buf = B.new_buffer(small[0], id=7)
        rv, comp = B.buffer__compress(buf, LZ4, 1)
        assert rv == _lib.E_OK and comp
        B.swap_data(buf, comp)
        assert B.buffer_bytes(buf) == emul(dic, small[0])[1]
        assert B.buffer__decompress(buf, LZ4) == 0 and B.buffer_bytes(buf) == small[0]
        B.destroy(buf)

        bufs = [B.new_buffer(p, id=i) for i, p in enumerate(small)]
        rc, st, ptrs = B.buffers_compress(bufs, LZ4, 1)
        assert rc == 0 and st == [0] * len(bufs)
        for i, (b, p) in enumerate(zip(bufs, ptrs)):
            assert p, i
            B.swap_data(b, p)
            assert B.buffer_bytes(b) == emul(dic, small[i])[1], len(small[i])
        rc, st = B.buffers_decompress(bufs, LZ4)
        assert rc == 0 and st == [0] * len(bufs)
        assert [B.buffer_bytes(b) for b in bufs] == small
        for b in bufs:
            B.destroy(b)
    finally:
        B.use_dict(None)
        d.close()
    rc, after = _compress_host(lib, pages, caps)             # the knob is still 1: without a dictionary it does nothing
    assert rc == 0 and after == no_dict


def test_environment_in_a_child_process(tmp_path, oracle_mod, emul):
    """TYCHE_LZ4_HC_DICT=1 with TYCHE_LZ4_DICT=<file> in the environment of a fresh process: a Buffer
    round trip whose stream is the emulator's."""
    O = oracle_mod
    dic = DC.dict_of(O, 4096, "dist0")
    (tmp_path / "pages.dict").write_bytes(dic)
    page = O.pagegen(1, 16384, first=705, dist=0).tobytes()
    (tmp_path / "page.bin").write_bytes(page)
    code = ("from tyche_amd import buffer as B\n"
            f"page = open({str(tmp_path / 'page.bin')!r}, 'rb').read()\n"
            "b = B.new_buffer(page, id=1)\n"
            "rv, comp = B.buffer__compress(b, 1, 1)\n"
            "assert rv == 0, rv\n"
            "B.swap_data(b, comp)\n"
            f"open({str(tmp_path / 'stream.bin')!r}, 'wb').write(B.buffer_bytes(b))\n"
            "assert B.buffer__decompress(b, 1) == 0 and B.buffer_bytes(b) == page\n"
            "print('child ok')\n")
    env = dict(os.environ, TYCHE_LZ4_DICT=str(tmp_path / "pages.dict"), TYCHE_LZ4_HC_DICT="1", PYTHONPATH=C.ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr[-2000:]
    assert (tmp_path / "stream.bin").read_bytes() == emul(dic, page)[1]


def test_exact_mode_still_refuses_a_dictionary(tc, oracle_mod, knobs):
    """LZ4_EXACT=1 with a dictionary and LZ4_HC_DICT=1: TYCHE_E_BAD_ARGS naming exact mode and the
    dictionary, from the batch call and from the host entry point; there is no new conflict."""
    from tyche_amd import _lib, buffer as B
    lib = _lib.load()
    knobs(LZ4_EXACT=1, LZ4_HC_DICT=1)
    dic, host = C.ratio_inputs(oracle_mod, 0)
    d = tc.Lz4Dict(dic)
    try:
        with pytest.raises(Exception) as e:
            compress_rows(tc, [host[0].tobytes()], d)
        assert "190" in str(e.value) and "LZ4_EXACT" in str(e.value) and "dictionary" in str(e.value), str(e.value)
        B.use_dict(d)
        rc, streams = _compress_host(lib, [host[0].tobytes()], [C.lz4_bound(4096)])
        assert rc == _lib.E_BAD_ARGS and streams == [b""]
        assert "LZ4_EXACT" in _lib.last_error() and "dictionary" in _lib.last_error()
    finally:
        B.use_dict(None)
        d.close()


def test_other_codecs_ignore_the_knob(tc, oracle_mod, knobs):
    from tyche_amd import _lib
    dic, pages = C.ratio_inputs(oracle_mod, 0)
    host = _dev(np.ascontiguousarray(pages[:8]))
    d = tc.Lz4Dict(dic)

    def run(cid):
        comp, clen = tc.compress_pages(host, compressor_id=cid, dictionary=d)
        torch.cuda.synchronize()
        lh, ch = clen.cpu().numpy(), comp.cpu().numpy()
        return [ch[i, :lh[i]].tobytes() for i in range(8)]
    ids = [_lib.COMPRESSOR_IDS["zlib"], _lib.COMPRESSOR_IDS["zstd"]]
    try:
        before = [run(c) for c in ids]
        knobs(LZ4_HC_DICT=1)
        assert [run(c) for c in ids] == before
    finally:
        d.close()
