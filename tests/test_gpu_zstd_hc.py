"""GPU tests of the high-compression zstd encoder (ZSTD_HC=1, zstd_parse_hc_kernel and
launch_zstd_encode_hc in tyche_amd/csrc/zstd_encode.hip): the sequences decoded from the kernel's
frames equal the host emulator's (tools/zstd_hc_emul.cpp, the same zstd_hc_core.h;
test_zstd_hc_emul.py holds that to the parse's own rules) and the frames restore; a page's bytes do
not depend on its batch; the batch contract on the checked layout of batch_layout.py; every
compress entry point; a dictionary wins where it reaches; the knob-off path keeps its bytes; and
the ratio closes half of the gap between the reference's levels 1 and 6."""
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
import zstd_hc_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INT32_MIN = -2 ** 31
ZSTD = 3
GUARD, FILL = 64, 0xAB
# page kinds whose frames must consist of compressed blocks (their sequences are compared)
COMPRESSIBLE = ("zero/", "period", "dist0/", "dist1/", "dist2/", "dist5/", "record/", "repeat_offset")


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
def collect():
    return C.load_collect()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def compress_rows(tc, host):
    """compress_pages on a (n, plen) numpy array: the frames as bytes."""
    comp, clen = tc.compress_pages(_dev(host), compressor_id=ZSTD)
    torch.cuda.synchronize()
    lh, ch = clen.cpu().numpy(), comp.cpu().numpy()
    assert (lh > 0).all(), lh[lh <= 0][:4]
    return [ch[i, :int(lh[i])].tobytes() for i in range(len(host))]


def compress_list(tc, pages, max_src_length=None):
    """Pages of any lengths through compress_ragged at tyche_compress_bound, guards checked."""
    lay = BL.build(pages, [tc.compress_bound(len(p), ZSTD) for p in pages], BC.src_shifts(len(pages)),
                   BC.dst_shifts(len(pages)), ("random", 9))
    rv, out, src = BC.device_compress(tc, lay, ZSTD, max_src_length=max_src_length)
    BL.check(out, src, lay)
    return [int(x) for x in rv], BL.outputs(out, rv, lay)


def restores(O, frame, page):
    r, dec = O.zstd_decompress(frame, len(page))
    ok = r == len(page) and dec[:len(page)] == page
    if ok and O.have_ref():
        r, dec = O.ref_zstd_decompress(frame, len(page))
        ok = r == len(page) and dec[:len(page)] == page
    return ok


# ---------------------------------------------------------------- kernel = emulator
def test_frame_sequences_equal_the_emulator(tc, oracle_mod, emul, collect, knobs):
    """Every page of the CPU cases in one launch of 65,535 declared bytes: the frame restores through
    the oracle's decoder (and the reference's where it is built), is no longer than
    tyche_compress_bound, and the sequences its compressed blocks decode to are the emulator's list.
    A frame with a raw block carries no sequences for it (pass A2 stores a block raw when coding
    would not make it smaller): such a frame is held to the restore alone, and no page of a compressible
    kind (COMPRESSIBLE) may come to one."""
    O = oracle_mod
    cases = C.cpu_case_pages(O)
    pages = [p for _, p in cases]
    plain_rv, plain = compress_list(tc, pages, max_src_length=65535)
    knobs(ZSTD_HC=1)
    rv, frames = compress_list(tc, pages, max_src_length=65535)
    compared = differs = 0
    for (name, page), r, frame, pf in zip(cases, rv, frames, plain):
        assert 0 < r <= tc.compress_bound(len(page), ZSTD), (name, r)
        dr, dec, seqs = collect(frame, len(page))
        assert dr == len(page) and dec == page, (name, dr)
        if O.have_ref():
            assert O.ref_zstd_decompress(frame, len(page)) == (len(page), page), name
        want, last = emul(page)
        if all(t == 2 for t, _ in C.frame_blocks(frame)):
            assert seqs == want, (name, len(seqs), len(want))
            compared += 1
            differs += seqs != collect(pf, len(page))[2]
        else:
            # a raw block: nothing was gained, which no page of a compressible kind may come to
            assert len(frame) >= len(page) and not name.startswith(COMPRESSIBLE), name
    print(f"{len(cases)} pages, {compared} frames of compressed blocks only, {differs} with other sequences than the default parse")


def test_waves_loop_over_pages(tc, oracle_mod, emul, collect, knobs):
    """300 mixed 4 KiB pages in one launch held to one resident page per CU, so that waves loop:
    rings and counters are cleared again, the prefetched next page is the right one."""
    knobs(ZSTD_HC=1, ZSTD_HC_PAGES_PER_CU=1)
    per = 50
    host = np.concatenate([oracle_mod.pagegen(per, 4096, seed=515, first=1000 * d, dist=d) for d in range(6)])
    host = np.ascontiguousarray(host[np.random.default_rng(4).permutation(len(host))])
    frames = compress_rows(tc, host)
    for i in range(len(host)):
        page = host[i].tobytes()
        dr, dec, seqs = collect(frames[i], 4096)
        assert dr == 4096 and dec == page, i
        if all(t == 2 for t, _ in C.frame_blocks(frames[i])):
            assert seqs == emul(page)[0], i


# ---------------------------------------------------------------- batch independence
def test_a_page_has_the_same_bytes_in_any_batch(tc, oracle_mod, knobs):
    """One 4 KiB page alone, in a batch of 65 and in one of 4,097 (above ZSTD_SPLIT_MIN, where the
    default encoder changes kernels)."""
    knobs(ZSTD_HC=1)
    host = oracle_mod.pagegen(4097, 4096, seed=3, first=50, dist=0)
    alone = compress_rows(tc, host[:1])[0]
    assert restores(oracle_mod, alone, host[0].tobytes())
    assert compress_rows(tc, host[:65])[0] == alone
    big = compress_rows(tc, host)
    assert big[0] == alone
    rot = compress_rows(tc, np.roll(host, 1000, axis=0))
    assert rot[1000] == alone and rot[1001] == big[1]
    knobs(ZSTD_SCRATCH_MB=1)                          # the four passes in chunks of 18 pages
    assert compress_rows(tc, host[:65]) == big[:65]


# ---------------------------------------------------------------- the checked layout
def test_batch_contract_on_the_checked_layout(tc, oracle_mod, knobs):
    """Lengths 0, 1, 5, 100, 4096, 16384 and 65535 at capacities of tyche_compress_bound, the
    frame's size and one byte either side of it, every source and destination alignment, three gap
    fills: at the bound the result is the frame's size with the same bytes whatever surrounds the
    page; one byte short gives 0; at the size and one above, the size with the same bytes or 0 (the
    scratch sits in the slot's tail); nothing outside a slot or in the source changes.  Then a page
    above a declared maximum of 20,000 gets INT32_MIN and its slot stays as it was."""
    O = oracle_mod
    lens = (0, 1, 5, 100, 4096, 16384, 65535)
    base = O.pagegen(2, 32768, seed=31, first=8, dist=1).tobytes()
    plain0 = compress_list(tc, [b""])[1][0]
    knobs(ZSTD_HC=1)
    pages = [base[:L] for L in lens]
    bounds = [tc.compress_bound(L, ZSTD) for L in lens]
    rv0, full = compress_list(tc, pages)
    for p, r, f, bd in zip(pages, rv0, full, bounds):
        assert 0 < r <= bd and restores(O, f, p), (len(p), r)
    assert full[0] == plain0                          # src_len == 0: the default encoder's frame
    batch, caps, which = [], [], []
    for i, p in enumerate(pages):
        for cap in (bounds[i], rv0[i], rv0[i] - 1, rv0[i] + 1):
            batch.append(p)
            caps.append(cap)
            which.append(i)
    n = len(batch)
    for rnd, gap in enumerate(("zero", "ff", ("random", 40))):
        ss = [(5 * i + rnd * 7) % 16 for i in range(n)]
        ds = [(3 * i + rnd * 11 + 1) % 16 for i in range(n)]
        assert len(set(ss)) == 16 and len(set(ds)) == 16
        lay = BL.build(batch, caps, ss, ds, gap)
        rv, out, src = BC.device_compress(tc, lay, ZSTD)
        BL.check(out, src, lay)
        outs = BL.outputs(out, rv, lay)
        for j in range(n):
            i, size = which[j], rv0[which[j]]
            if caps[j] == bounds[i]:
                assert int(rv[j]) == size and outs[j] == full[i], (gap, lens[i], caps[j], int(rv[j]))
            elif caps[j] < size:
                assert int(rv[j]) == 0, (gap, lens[i], caps[j], int(rv[j]))
            else:
                assert int(rv[j]) in (0, size) and outs[j] in (b"", full[i]), (gap, lens[i], caps[j], int(rv[j]))
    # above the declared maximum
    sel = [base[:100], base[:20000], base[:20001], base[:4096]]
    bound = tc.compress_bound(20001, ZSTD)
    lay = BL.build(sel, [bound] * 4, [1, 2, 3, 4], [5, 6, 7, 8], "ff")
    rv, out, src = BC.device_compress(tc, lay, ZSTD, max_src_length=20000)
    BL.check(out, src, lay)
    outs = BL.outputs(out, rv, lay)
    a = int(lay.dst_offsets[2])
    assert int(rv[2]) == INT32_MIN and bool((out[a:a + bound] == lay.fill).all())
    for i in (0, 1, 3):
        assert int(rv[i]) > 0 and restores(O, outs[i], sel[i]), i
    with pytest.raises(Exception):                    # a declared maximum above 65,535: TYCHE_E_BAD_ARGS, as without the knob
        BC.device_compress(tc, lay, ZSTD, max_src_length=65536)


# ---------------------------------------------------------------- entry points
ENTRY_SIZES = [16384, 8192, 4097, 1000, 65, 13, 1, 12000]


def _entry_pages(O):
    data = O.pagegen(4, 32768, seed=12, first=77, dist=1).tobytes()
    return [data[i * 777:i * 777 + n] for i, n in enumerate(ENTRY_SIZES)]


CHILD = r"""
import ctypes, sys
import numpy as np
from oracle import oracle as O
from tyche_amd import _lib, buffer as B
lib = _lib.load()
ZSTD = 3
sizes = %r
data = O.pagegen(4, 32768, seed=12, first=77, dist=1).tobytes()
pages = [data[i * 777:i * 777 + n] for i, n in enumerate(sizes)]
n = len(pages)
caps = [int(lib.tyche_compress_bound(ZSTD, len(p))) for p in pages]
src = [np.frombuffer(p, np.uint8).copy() for p in pages]
out = [np.full(c + 64, 0xAB, np.uint8) for c in caps]
vp, u32 = ctypes.c_void_p * n, ctypes.c_uint32 * n
res = (ctypes.c_int32 * n)()
rc = lib.tyche_compress_host(ZSTD, 1, n, vp(*[s.ctypes.data for s in src]), u32(*[len(p) for p in pages]),
                             vp(*[o.ctypes.data for o in out]), u32(*caps), res)
assert rc == 0, _lib.last_error()
for o, c in zip(out, caps):
    assert bool((o[c:] == 0xAB).all()), "wrote past a capacity"
print("host", " ".join(o[:max(r, 0)].tobytes().hex() for o, r in zip(out, res)))
buf = B.new_buffer(pages[0], id=7)
rv, comp = B.buffer__compress(buf, ZSTD, 1)
assert rv == _lib.E_OK and comp
B.swap_data(buf, comp)
print("buffer", B.buffer_bytes(buf).hex())
assert B.buffer__decompress(buf, ZSTD) == 0 and B.buffer_bytes(buf) == pages[0]
B.destroy(buf)
bufs = [B.new_buffer(p, id=i) for i, p in enumerate(pages)]
rc, st, ptrs = B.buffers_compress(bufs, ZSTD, 1)
assert rc == 0 and st == [0] * n
for b, p in zip(bufs, ptrs):
    assert p
    B.swap_data(b, p)
print("buffers", " ".join(B.buffer_bytes(b).hex() for b in bufs))
assert lib.tyche_restore_queue_start(8, 100) == 0
try:
    assert lib.tyche_buffer_restore(bufs[0], ZSTD) == 0
finally:
    lib.tyche_restore_queue_stop()
assert B.buffer_bytes(bufs[0]) == pages[0]
rc, st = B.buffers_decompress(bufs[1:], ZSTD)
assert rc == 0 and st == [0] * (n - 1)
assert [B.buffer_bytes(b) for b in bufs] == pages
for b in bufs:
    B.destroy(b)
print("child ok")
"""


def test_entry_points_with_the_environment_variable(tc, oracle_mod, knobs):
    """TYCHE_ZSTD_HC=1 in the environment of a fresh process: tyche_compress_host, buffer__compress
    and tyche_buffers_compress give the device batch's bytes (taken here under the knob), which are
    not the default encoder's; the pages come back through buffer__decompress,
    tyche_buffers_decompress and the restore queue."""
    pages = _entry_pages(oracle_mod)
    plain = compress_list(tc, pages)[1]
    knobs(ZSTD_HC=1)
    want = compress_list(tc, pages)[1]
    assert want != plain
    env = dict(os.environ, TYCHE_ZSTD_HC="1", PYTHONPATH=C.ROOT)
    p = subprocess.run([sys.executable, "-c", CHILD % (ENTRY_SIZES,)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr[-2000:]
    got = {ln.split()[0]: [bytes.fromhex(h) for h in ln.split()[1:]] for ln in p.stdout.splitlines() if ln and ln != "child ok"}
    assert got["host"] == want
    assert got["buffer"] == [want[0]]
    assert got["buffers"] == want


# ---------------------------------------------------------------- dictionary precedence
def _compress_host(lib, pages, caps):
    n = len(pages)
    src = [np.frombuffer(p, np.uint8).copy() for p in pages]
    out = [np.full(c + GUARD, FILL, np.uint8) for c in caps]
    vp, u32 = ctypes.c_void_p * n, ctypes.c_uint32 * n
    res = (ctypes.c_int32 * n)()
    rc = lib.tyche_compress_host(ZSTD, 1, n, vp(*[s.ctypes.data for s in src]), u32(*[len(p) for p in pages]),
                                 vp(*[o.ctypes.data for o in out]), u32(*caps), res)
    for o, c in zip(out, caps):
        assert bool((o[c:] == FILL).all()), "wrote past a capacity"
    return rc, [o[:max(r, 0)].tobytes() for o, r in zip(out, res)]


def test_a_dictionary_wins_where_it_reaches(tc, oracle_mod, knobs):
    """A process-wide 4 KiB zstd dictionary and the knob: a 16 KiB page has the dictionary encoder's
    bytes (those of a run without the knob), a 65,000-byte page, beyond the dictionary's reach, the
    HC bytes of a run without the dictionary; tyche_zstd_compress_batch_dict ignores the knob."""
    from tyche_amd import _lib
    O = oracle_mod
    lib = _lib.load()
    data = O.pagegen(4, 32768, seed=5, first=40, dist=0).tobytes()
    pages = [data[:16384], data[20000:85000]]
    caps = [tc.compress_bound(len(p), ZSTD) for p in pages]
    rows = _dev(np.frombuffer(pages[0], np.uint8).reshape(1, -1))
    _lib.set_knob("ZSTD_HC", 1)
    try:
        rc, hc = _compress_host(lib, pages, caps)
        assert rc == 0, _lib.last_error()
    finally:
        _lib.clear_knob("ZSTD_HC")
    d = tc.Dictionary(O.pagegen(1, 4096, seed=5, first=39, dist=0).tobytes())
    tc.use_zstd_dict(d)
    try:
        rc, with_dict = _compress_host(lib, pages, caps)
        assert rc == 0, _lib.last_error()
        comp, clen = tc.compress_pages(rows, compressor_id=ZSTD, dictionary=d)
        torch.cuda.synchronize()
        batch_dict = comp.cpu().numpy()[0, :int(clen[0])].tobytes()
        knobs(ZSTD_HC=1)
        rc, both = _compress_host(lib, pages, caps)
        assert rc == 0, _lib.last_error()
        comp, clen = tc.compress_pages(rows, compressor_id=ZSTD, dictionary=d)
        torch.cuda.synchronize()
        assert comp.cpu().numpy()[0, :int(clen[0])].tobytes() == batch_dict
    finally:
        tc.use_zstd_dict(None)
        d.close()
    assert both[0] == with_dict[0] and both[0] != hc[0]
    assert both[1] == hc[1] and both[1] != with_dict[1]
    assert restores(O, both[1], pages[1])


def test_other_codecs_ignore_the_knob(tc, oracle_mod, knobs):
    """LZ4 and zlib keep their bytes under ZSTD_HC=1, zstd keeps its under LZ4_HC=1, and the two
    knobs together give each codec its own mode."""
    host = _dev(oracle_mod.pagegen(8, 8192, dist=0))

    def run(cid):
        comp, clen = tc.compress_pages(host, compressor_id=cid)
        torch.cuda.synchronize()
        lh, ch = clen.cpu().numpy(), comp.cpu().numpy()
        return [ch[i, :lh[i]].tobytes() for i in range(8)]
    before = {c: run(c) for c in (1, 2, 3)}
    knobs(ZSTD_HC=1)
    zhc = run(3)
    assert run(1) == before[1] and run(2) == before[2] and zhc != before[3]
    knobs(LZ4_HC=1)
    lhc = run(1)
    assert lhc != before[1] and run(3) == zhc and run(2) == before[2]
    knobs(ZSTD_HC=0)
    assert run(3) == before[3] and run(1) == lhc


# ---------------------------------------------------------------- knob off
def test_knob_off_keeps_the_default_encoders_bytes(tc, oracle_mod):
    """64 pages per bench distribution at 16 and 32 KiB: the frames taken before the knob was ever
    set in this run, with the knob at 0, and after tyche_clear_knob are the same; with the knob at 1
    in between they are not."""
    from tyche_amd import _lib
    for plen in (16384, 32768):
        host = np.concatenate([oracle_mod.pagegen(64, plen, dist=d) for d in range(6)])
        try:
            _lib.clear_knob("ZSTD_HC")
            before = compress_rows(tc, host)
            _lib.set_knob("ZSTD_HC", 1)
            hc = compress_rows(tc, host)
            _lib.set_knob("ZSTD_HC", 0)
            zero = compress_rows(tc, host)
            _lib.clear_knob("ZSTD_HC")
            cleared = compress_rows(tc, host)
        finally:
            _lib.clear_knob("ZSTD_HC")
        assert zero == before and cleared == before and hc != before, plen


# ---------------------------------------------------------------- ratio
def ratio_cells(tc, O, knob):
    """{(dist, plen): [frame sizes of the first 48 pagegen pages]} for all six distributions."""
    from tyche_amd import _lib
    cells = {}
    try:
        _lib.set_knob("ZSTD_HC", knob)
        for dist in range(6):
            for plen in C.RATIO_LENS:
                cells[dist, plen] = [len(f) for f in compress_rows(tc, O.pagegen(C.RATIO_PAGES, plen, dist=dist))]
    finally:
        _lib.clear_knob("ZSTD_HC")
    return cells


def test_ratio_closes_half_of_the_gap_to_level_6(tc, oracle_mod):
    """Totals over the first 48 oracle.pagegen pages per distribution and page length.  L1 and L6:
    the reference's ZSTD_compress at levels 1 and 6 (tests/golden/zstd_hc_targets.json); D: the
    default device encoder, here, knob off; H: ZSTD_HC=1.  In the nine cells where level 6 saves at
    least 2 %, H <= L1 - (L1 - L6) / 2; in all twelve H <= D; no page of the constant and the random
    distribution (3 and 4) grows."""
    O = oracle_mod
    t = C.targets()["cells"]
    D, H = ratio_cells(tc, O, 0), ratio_cells(tc, O, 1)
    judged, failures = 0, []
    for dist in C.RATIO_DISTS:
        for plen in C.RATIO_LENS:
            l1, l6 = t[f"{dist}/{plen}"]
            d, h = sum(D[dist, plen]), sum(H[dist, plen])
            share = (l1 - h) / (l1 - l6)
            print(json.dumps({"dist": dist, "page_len": plen, "device_default": d, "device_hc": h, "level1": l1,
                              "level6": l6, "share_closed": round(share, 3)}))
            if h > d:
                failures.append(("above the default encoder", dist, plen, d, h))
            if (l1 - l6) * 50 >= l1:
                judged += 1
                if h > C.ratio_bar(l1, l6):
                    failures.append(("less than half of the gap", dist, plen, l1, l6, h, round(share, 3)))
    assert judged == 9
    for dist in (3, 4):
        for plen in C.RATIO_LENS:
            grown = [(i, a, b) for i, (a, b) in enumerate(zip(D[dist, plen], H[dist, plen])) if b > a]
            if grown:
                failures.append(("pages grew", dist, plen, grown[:4]))
    assert not failures, failures
