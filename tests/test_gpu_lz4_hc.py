"""GPU tests of the high-compression LZ4 encoder (LZ4_HC=1, tyche_amd/csrc/lz4_encode_hc.hip): the
kernel's results and bytes equal the host emulator's (tools/lz4_hc_emul.cpp, the same
lz4_hc_core.h; test_lz4_hc_emul.py holds that to the LZ4 block format, the limited-output
contract and the ratio), through every compress entry point; the batch contract on the checked
layout of batch_layout.py; pages above 65,535 bytes, dictionary pages and the knob-off path keep
the bytes they have without the knob."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import batch_layout as BL
import lz4_hc_cases as C

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


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def compress_rows(tc, host):
    """compress_pages on a (n, plen) numpy array: the streams as bytes."""
    comp, clen = tc.compress_pages(_dev(host))
    torch.cuda.synchronize()
    lh, ch = clen.cpu().numpy(), comp.cpu().numpy()
    return [ch[i, :max(int(lh[i]), 0)].tobytes() for i in range(len(host))]


def run_layout(tc, lay, max_src_length=None):
    """A checked layout through compress_ragged: (results, outputs), guards and source verified."""
    d_src, d_out = _dev(lay.src), _dev(lay.out)
    d_rv = torch.full((lay.count,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    if max_src_length is None:
        max_src_length = max([int(x) for x in lay.src_lengths] + [1])
    tc.compress_ragged(d_src, _dev(lay.src_offsets), _dev(lay.src_lengths), d_out, _dev(lay.dst_offsets), _dev(lay.caps),
                       d_rv, max_src_length=max_src_length)
    torch.cuda.synchronize()
    rv, out = d_rv.cpu().numpy(), d_out.cpu().numpy()
    BL.check(out, d_src.cpu().numpy(), lay)
    return [int(x) for x in rv], BL.outputs(out, rv, lay), out


def test_hc_compresses_better_and_the_knob_goes_away(tc, oracle_mod):
    """64 dist-0 pages of 16 KiB (the first 64 of the ratio test's): with LZ4_HC=1 the total is below
    the knob-off total, and by the ratio test's margin -- M <= F - (F - H) / 2 with F the reference's
    fast parse (oracle.lz4_compress) and H liblz4's LZ4_compress_HC level 3 on these 64 pages
    (tests/golden/lz4_hc_targets.json); every stream restores; after tyche_clear_knob, and with
    the knob at 0, the bytes are those of the first run."""
    from tyche_amd import _lib
    host = oracle_mod.pagegen(64, 16384, dist=0)
    try:
        before = compress_rows(tc, host)
        _lib.set_knob("LZ4_HC", 1)
        hc = compress_rows(tc, host)
        _lib.clear_knob("LZ4_HC")
        cleared = compress_rows(tc, host)
        _lib.set_knob("LZ4_HC", 0)
        zero = compress_rows(tc, host)
    finally:
        _lib.clear_knob("LZ4_HC")
    D, M = sum(map(len, before)), sum(map(len, hc))
    F = sum(len(oracle_mod.lz4_compress(p.tobytes())) for p in host)
    H = C.hc3_total(0, first64=True)
    print(f"knob off {D} B, LZ4_HC=1 {M} B, reference fast {F} B, HC level 3 {H} B, bar {C.ratio_bar(F, H):.0f}")
    assert M < D and M <= C.ratio_bar(F, H), (D, F, H, M)
    for s, p in zip(hc, host):
        assert C.restores(oracle_mod, s, p.tobytes())
    assert cleared == before and zero == before


@pytest.mark.parametrize("plen", [4096, 16384])
def test_kernel_bytes_equal_the_emulator(tc, oracle_mod, emul, knobs, plen):
    """Every page kind, 8 pages each, in one launch."""
    knobs(LZ4_HC=1)
    host = np.concatenate([C.kind_pages(oracle_mod, kind, plen) for kind in C.KINDS])
    got = compress_rows(tc, host)
    for i, p in enumerate(host):
        r, want = emul(p.tobytes())
        assert len(got[i]) == r and got[i] == want, (C.KINDS[i // 8], i % 8, len(got[i]), r)


def test_kernel_bytes_equal_the_emulator_65535(tc, oracle_mod, emul, knobs):
    """One 65,535-byte page per kind (16-bit positions at their limit, one page per CU by LDS)."""
    knobs(LZ4_HC=1)
    host = np.concatenate([C.kind_pages(oracle_mod, kind, 65535, n=1) for kind in C.KINDS])
    got = compress_rows(tc, host)
    for i, p in enumerate(host):
        r, want = emul(p.tobytes())
        assert len(got[i]) == r and got[i] == want, (C.KINDS[i], len(got[i]), r)


def test_waves_claim_pages(tc, oracle_mod, emul, knobs):
    """300 mixed 4 KiB pages in one launch held to one resident page per CU, so that waves loop:
    the table and the ring counters are cleared again, the prefetched next page is the right one."""
    knobs(LZ4_HC=1, LZ4_HC_PAGES_PER_CU=1)
    host = C.mixed_4k_pages(oracle_mod, 300)
    got = compress_rows(tc, host)
    for i, p in enumerate(host):
        r, want = emul(p.tobytes())
        assert len(got[i]) == r and got[i] == want, i


def test_ragged_batch_contract(tc, oracle_mod, emul, knobs):
    """Lengths 0, 1, 12, 13, 100, 4096, 16384 and 65535 at capacities of the stream's size, one
    less and 0, every source and destination alignment, guards around every slot, neighbours'
    bytes poisoned (random gaps): results and bytes are the emulator's, nothing outside a slot or
    in the source changes.  Then a page above a declared maximum of 20000 gets INT32_MIN and its
    slot stays as it was."""
    O = oracle_mod
    knobs(LZ4_HC=1)
    lens = (0, 1, 12, 13, 100, 4096, 16384, 65535)
    base = O.pagegen(2, 32768, seed=31, first=8, dist=1).tobytes()
    pages, caps, want = [], [], []
    for L in lens:
        p = base[:L]
        full, stream = emul(p)
        for cap in (full, full - 1, 0):
            pages.append(p)
            caps.append(cap)
            want.append((full, stream) if cap >= full else (0, b""))
    # two rounds of shifts so that every length meets several alignments, all 16 of each overall
    for rnd in range(2):
        n = len(pages)
        ss = [(5 * i + rnd * 7) % 16 for i in range(n)]
        ds = [(3 * i + rnd * 11 + 1) % 16 for i in range(n)]
        assert rnd or (len(set(ss)) == 16 and len(set(ds)) == 16)
        lay = BL.build(pages, caps, ss, ds, ("random", 40 + rnd))
        rv, outs, _ = run_layout(tc, lay)
        for i in range(n):
            assert (rv[i], outs[i]) == want[i], (rnd, len(pages[i]), caps[i], rv[i], want[i][0])
    # above the declared maximum
    sel = [base[:100], base[:20000], base[:20001], base[:4096]]
    wants = [emul(p) for p in sel]
    bound = C.lz4_bound(20001)
    lay = BL.build(sel, [bound] * 4, [1, 2, 3, 4], [5, 6, 7, 8], "ff")
    rv, outs, out = run_layout(tc, lay, max_src_length=20000)
    a = int(lay.dst_offsets[2])
    assert rv[2] == INT32_MIN and bool((out[a:a + bound] == lay.fill).all())
    for i in (0, 1, 3):
        assert (rv[i], outs[i]) == wants[i], i


def test_mixed_sizes_in_one_launch(tc, oracle_mod, emul, knobs):
    """Pages of 300, 16384, 70000 and 200000 bytes in one ragged launch: the two of up to 65,535
    bytes get the emulator's bytes, the two longer ones the large-page encoder's bytes of a
    knob-off run, and all four restore through decompress_ragged."""
    O = oracle_mod
    sizes = (300, 16384, 70000, 200000)
    data = O.pagegen(8, 32768, seed=77, first=3, dist=0).tobytes()
    pages = [data[i * 1000:i * 1000 + n] for i, n in enumerate(sizes)]
    caps = [tc.compress_bound(n) for n in sizes]
    lay = BL.build(pages, caps, [1, 6, 11, 0], [2, 7, 12, 0], ("random", 3))
    rv0, plain, _ = run_layout(tc, lay)
    knobs(LZ4_HC=1)
    rv, outs, _ = run_layout(tc, lay)
    for i in (0, 1):
        assert (rv[i], outs[i]) == emul(pages[i]), sizes[i]
    assert outs[1] != plain[1] and len(outs[1]) < len(plain[1])
    for i in (2, 3):
        assert rv[i] == rv0[i] > 0 and outs[i] == plain[i], sizes[i]
    back = BL.build(outs, list(sizes), [3, 5, 9, 0], [0, 4, 8, 15], "zero")
    d_src, d_out = _dev(back.src), _dev(back.out)
    d_rv = torch.zeros(4, dtype=torch.int32, device=DEV)
    tc.decompress_ragged(d_src, _dev(back.src_offsets), _dev(back.src_lengths), _dev(back.caps), d_out,
                         _dev(back.dst_offsets), d_rv, max_src_length=max(rv), max_capacity=max(sizes))
    torch.cuda.synchronize()
    res, out = d_rv.cpu().numpy(), d_out.cpu().numpy()
    BL.check(out, d_src.cpu().numpy(), back)
    assert [int(x) for x in res] == list(sizes)
    assert BL.outputs(out, res, back) == pages


def _compress_host(lib, pages, caps):
    n = len(pages)
    src = [np.frombuffer(p, np.uint8).copy() for p in pages]
    out = [np.full(c + C.GUARD, C.FILL, np.uint8) for c in caps]
    vp, u32 = ctypes.c_void_p * n, ctypes.c_uint32 * n
    res = (ctypes.c_int32 * n)()
    rc = lib.tyche_compress_host(LZ4, 1, n, vp(*[s.ctypes.data for s in src]), u32(*[len(p) for p in pages]),
                                 vp(*[o.ctypes.data for o in out]), u32(*caps), res)
    for o, c in zip(out, caps):
        assert bool((o[c:] == C.FILL).all()), "wrote past a capacity"
    return rc, [o[:max(r, 0)].tobytes() for o, r in zip(out, res)]


def test_host_entry_points(tc, oracle_mod, emul, knobs):
    """tyche_compress_host, buffer__compress -> buffer__decompress and tyche_buffers_compress on 8
    pages: the emulator's bytes, and the pages back."""
    from tyche_amd import _lib, buffer as B
    O = oracle_mod
    lib = _lib.load()
    knobs(LZ4_HC=1)
    sizes = [16384, 8192, 4097, 1000, 65, 13, 1, 12000]
    data = O.pagegen(4, 32768, seed=12, first=77, dist=1).tobytes()
    pages = [data[i * 777:i * 777 + n] for i, n in enumerate(sizes)]
    want = [emul(p)[1] for p in pages]

    rc, streams = _compress_host(lib, pages, [C.lz4_bound(n) for n in sizes])
    assert rc == 0, _lib.last_error()
    assert streams == want

    buf = B.new_buffer(pages[0], id=7)
    rv, comp = B.buffer__compress(buf, LZ4, 1)
    assert rv == _lib.E_OK and comp
    B.swap_data(buf, comp)
    assert B.buffer_bytes(buf) == want[0]
    assert B.buffer__decompress(buf, LZ4) == 0 and B.buffer_bytes(buf) == pages[0]
    B.destroy(buf)

    bufs = [B.new_buffer(p, id=i) for i, p in enumerate(pages)]
    rc, st, ptrs = B.buffers_compress(bufs, LZ4, 1)
    assert rc == 0 and st == [0] * len(bufs)
    for i, (b, p) in enumerate(zip(bufs, ptrs)):
        assert p, sizes[i]
        B.swap_data(b, p)
        assert B.buffer_bytes(b) == want[i], sizes[i]
    rc, st = B.buffers_decompress(bufs, LZ4)
    assert rc == 0 and st == [0] * len(bufs)
    assert [B.buffer_bytes(b) for b in bufs] == pages
    for b in bufs:
        B.destroy(b)


def test_exact_and_hc_contradict(tc, oracle_mod, knobs):
    """Both knobs: TYCHE_E_BAD_ARGS naming both, from the device and the host entry point; results
    and destinations are not touched."""
    from tyche_amd import _lib
    lib = _lib.load()
    knobs(LZ4_EXACT=1, LZ4_HC=1)
    host = oracle_mod.pagegen(2, 4096, dist=0)
    with pytest.raises(Exception) as e:
        tc.compress_pages(_dev(host))
    assert "LZ4_EXACT" in str(e.value) and "LZ4_HC" in str(e.value), str(e.value)
    rc, streams = _compress_host(lib, [host[0].tobytes()], [C.lz4_bound(4096)])
    assert rc == _lib.E_BAD_ARGS and streams == [b""]
    assert "LZ4_EXACT" in _lib.last_error() and "LZ4_HC" in _lib.last_error()


def test_a_dictionary_wins_where_it_reaches(tc, oracle_mod, emul, knobs):
    """A process-wide 4 KiB dictionary and the knob: a 16 KiB page has the dictionary encoder's
    bytes (those of a run without the knob), a 65,000-byte page, beyond the dictionary's reach, the
    HC bytes; tyche_lz4_compress_batch_dict ignores the knob."""
    from tyche_amd import _lib, buffer as B
    O = oracle_mod
    lib = _lib.load()
    data = O.pagegen(4, 32768, seed=5, first=40, dist=0).tobytes()
    pages = [data[:16384], data[20000:85000]]
    caps = [C.lz4_bound(len(p)) for p in pages]
    d = tc.Lz4Dict(O.pagegen(1, 4096, seed=5, first=39, dist=0).tobytes())
    B.use_dict(d)
    try:
        rc, with_dict = _compress_host(lib, pages, caps)
        assert rc == 0, _lib.last_error()
        rows = _dev(np.frombuffer(pages[0], np.uint8).reshape(1, -1))
        comp, clen = tc.compress_pages(rows, dictionary=d)
        torch.cuda.synchronize()
        batch_dict = comp.cpu().numpy()[0, :int(clen[0])].tobytes()
        knobs(LZ4_HC=1)
        rc, both = _compress_host(lib, pages, caps)
        assert rc == 0, _lib.last_error()
        comp, clen = tc.compress_pages(rows, dictionary=d)
        torch.cuda.synchronize()
        assert comp.cpu().numpy()[0, :int(clen[0])].tobytes() == batch_dict
    finally:
        B.use_dict(None)
        d.close()
    assert both[0] == with_dict[0] and both[0] != emul(pages[0])[1]
    assert both[1] == emul(pages[1])[1] and both[1] != with_dict[1]


def test_other_codecs_ignore_the_knob(tc, oracle_mod, knobs):
    from tyche_amd import _lib
    host = _dev(oracle_mod.pagegen(8, 8192, dist=0))

    def run(cid):
        comp, clen = tc.compress_pages(host, compressor_id=cid)
        torch.cuda.synchronize()
        lh, ch = clen.cpu().numpy(), comp.cpu().numpy()
        return [ch[i, :lh[i]].tobytes() for i in range(8)]
    ids = [_lib.COMPRESSOR_IDS["zlib"], _lib.COMPRESSOR_IDS["zstd"]]
    before = [run(c) for c in ids]
    knobs(LZ4_HC=1)
    assert [run(c) for c in ids] == before


def test_environment_knob_in_a_child_process(oracle_mod, emul):
    """TYCHE_LZ4_HC=1 in the environment of a fresh process: compress_pages gives the emulator's bytes."""
    host = oracle_mod.pagegen(4, 8192, seed=9, first=2, dist=0)
    code = ("import sys, torch, numpy as np\n"
            "from oracle import oracle as O\n"
            "from tyche_amd import codec\n"
            "host = O.pagegen(4, 8192, seed=9, first=2, dist=0)\n"
            "comp, clen = codec.compress_pages(torch.from_numpy(host).to('cuda:0'))\n"
            "torch.cuda.synchronize()\n"
            "c, l = comp.cpu().numpy(), clen.cpu().numpy()\n"
            "print(' '.join(c[i, :l[i]].tobytes().hex() for i in range(4)))\n")
    env = dict(os.environ, TYCHE_LZ4_HC="1", PYTHONPATH=C.ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [bytes.fromhex(h) for h in p.stdout.split()]
    assert got == [emul(pg.tobytes())[1] for pg in host]
