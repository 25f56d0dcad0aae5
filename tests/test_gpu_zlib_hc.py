"""GPU tests of the high-compression zlib encoder (ZLIB_HC=1, zlib_deflate_hc_kernel in
tyche_amd/csrc/zlib_deflate_hc.hip): the symbols walked out of the kernel's streams equal the host
emulator's records cut by the chunk rule (tools/zlib_hc_emul.cpp, the same zlib_hc_core.h;
test_zlib_hc_emul.py holds that to the parse's own rules) and the streams restore through the
reference's uncompress; a page's bytes do not depend on its batch; the batch contract on the checked
layout of batch_layout.py; every compress entry point; the other codecs and their knobs; the
knob-off path keeps the bytes recorded from the encoder as it stood before this mode; and the ratio
closes half of the gap between the reference's levels 1 and 6."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import batch_contract_cases as BC
import batch_layout as BL
import zlib_hc_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INT32_MIN = -2 ** 31
LZ4, ZLIB, ZSTD = 1, 2, 3
GUARD, FILL = 64, 0xAB


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
def cases(oracle_mod):
    return C.cpu_case_pages(oracle_mod)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def compress_rows(tc, host, cid=ZLIB):
    """compress_pages on a (n, plen) numpy array: the streams as bytes."""
    comp, clen = tc.compress_pages(_dev(host), compressor_id=cid)
    torch.cuda.synchronize()
    lh, ch = clen.cpu().numpy(), comp.cpu().numpy()
    assert (lh > 0).all(), lh[lh <= 0][:4]
    return [ch[i, :int(lh[i])].tobytes() for i in range(len(host))]


def compress_list(tc, pages, max_src_length=None):
    """Pages of any lengths through compress_ragged at tyche_compress_bound, guards checked."""
    lay = BL.build(pages, [tc.compress_bound(len(p), ZLIB) for p in pages], BC.src_shifts(len(pages)),
                   BC.dst_shifts(len(pages)), ("random", 9))
    rv, out, src = BC.device_compress(tc, lay, ZLIB, max_src_length=max_src_length)
    BL.check(out, src, lay)
    return [int(x) for x in rv], BL.outputs(out, rv, lay)


def restores(O, stream, page):
    r, dec = O.zlib_uncompress(stream, len(page))
    ok = r == len(page) and dec[:len(page)] == page
    if ok and O.have_ref():
        ok = O.ref_zlib_uncompress(stream, len(page)) == (len(page), page)
    return ok


def digest(streams):
    return [hashlib.sha256(s).hexdigest()[:32] for s in streams]


# ---------------------------------------------------------------- kernel = emulator
def test_stream_symbols_equal_the_emulator(tc, oracle_mod, emul, cases, knobs):
    """Every page of the CPU cases in one launch of 65,535 declared bytes: the stream restores with
    the exact length through the oracle's and the reference's uncompress, is no longer than
    tyche_compress_bound, begins 78 01, and its literal and (length, distance) symbols are the
    emulator's records cut by the chunk rule, one for one.  A page whose coded stream would not
    beat the stored form is stored (only pages of random bytes come to that): such a stream is held
    to the stored form's size and the restore."""
    O = oracle_mod
    pages = [p for _, p in cases]
    plain = compress_list(tc, pages, max_src_length=65535)[1]
    knobs(ZLIB_HC=1)
    rv, streams = compress_list(tc, pages, max_src_length=65535)
    compared = differs = 0
    for (name, page), r, s, pf in zip(cases, rv, streams, plain):
        assert 0 < r <= tc.compress_bound(len(page), ZLIB), (name, r)
        assert s[:2] == b"\x78\x01", name
        assert restores(O, s, page), name
        syms, dec, kinds = C.walk(s)
        assert dec == page, name
        recs, last = emul(page)
        if kinds == [0] * len(kinds):
            # the stored form: coding would not have made the page smaller, which only random bytes come to
            assert len(s) == 2 + len(page) + 5 + 4 and name.startswith("random/"), name
        else:
            assert syms == C.record_symbols(recs, last, page), (name, len(syms))
            compared += 1
            differs += s != pf
    print(f"{len(cases)} pages, {compared} coded streams compared, {differs} differ from the default encoder's")
    assert compared >= len(cases) // 2 and differs > 10
    # fewer workgroups than pages: waves loop over pages, rings and counters are cleared again
    knobs(ZLIB_HC=1, ZLIB_HC_PAGES_PER_CU=1)
    small = [p for p in pages if len(p) <= 4096]
    many = (small * (600 // len(small) + 1))[:600]
    rv2, again = compress_list(tc, many, max_src_length=4096)
    first = dict(zip(pages, streams))
    assert all(a == first[p] for a, p in zip(again, many))


def test_waves_loop_over_pages(tc, oracle_mod, emul, knobs):
    """300 mixed 4 KiB pages in one launch held to one resident page per CU, so that waves loop:
    the prefetched next page is the right one and stale rings are never seen."""
    knobs(ZLIB_HC=1, ZLIB_HC_PAGES_PER_CU=1)
    host = np.concatenate([oracle_mod.pagegen(50, 4096, seed=515, first=1000 * d, dist=d) for d in range(6)])
    host = np.ascontiguousarray(host[np.random.default_rng(4).permutation(len(host))])
    streams = compress_rows(tc, host)
    for i in range(0, len(host), 3):
        page = host[i].tobytes()
        syms, dec, kinds = C.walk(streams[i])
        assert dec == page, i
        if kinds != [0]:
            recs, last = emul(page)
            assert syms == C.record_symbols(recs, last, page), i


# ---------------------------------------------------------------- batch independence
def test_a_page_has_the_same_bytes_in_any_batch(tc, oracle_mod, knobs):
    """One 4 KiB page alone, in a batch of 65 rows, at another index of a batch of 4,097, and among
    pages of mixed lengths."""
    knobs(ZLIB_HC=1)
    host = oracle_mod.pagegen(4097, 4096, seed=3, first=50, dist=0)
    alone = compress_rows(tc, host[:1])[0]
    assert restores(oracle_mod, alone, host[0].tobytes())
    assert compress_rows(tc, host[:65])[0] == alone
    big = compress_rows(tc, host)
    assert big[0] == alone
    rot = compress_rows(tc, np.roll(host, 1000, axis=0))
    assert rot[1000] == alone and rot[1001] == big[1]
    other = oracle_mod.pagegen(2, 32768, seed=9, dist=1).tobytes()
    mixed = [other[:100], host[0].tobytes(), other[:20000], b"", host[1].tobytes(), other[:3]]
    got = compress_list(tc, mixed)[1]
    assert got[1] == alone and got[4] == big[1]


# ---------------------------------------------------------------- the checked layout
def test_batch_contract_on_the_checked_layout(tc, oracle_mod, knobs):
    """Lengths 0, 1, 5, 100, 4096, 16384 and 65535 at capacities of tyche_compress_bound, the
    stream's size and one byte either side of it, every source and destination alignment, three gap
    fills: at the bound the result is the stream's size with the same bytes whatever surrounds the
    page, and so it is at the size and one above; one byte short gives 0;
    nothing outside a slot or in the source changes.  Then a page above a
    declared maximum of 20,000 gets INT32_MIN and its slot stays as it was."""
    O = oracle_mod
    lens = (0, 1, 5, 100, 4096, 16384, 65535)
    base = O.pagegen(2, 32768, seed=31, first=8, dist=1).tobytes()
    plain0 = compress_list(tc, [b""])[1][0]
    knobs(ZLIB_HC=1)
    pages = [base[:L] for L in lens]
    bounds = [tc.compress_bound(L, ZLIB) for L in lens]
    rv0, full = compress_list(tc, pages)
    for p, r, f, bd in zip(pages, rv0, full, bounds):
        assert 0 < r <= bd and restores(O, f, p), (len(p), r)
    assert full[0] == plain0                          # src_len == 0: the default encoder's stream
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
        rv, out, src = BC.device_compress(tc, lay, ZLIB)
        BL.check(out, src, lay)
        outs = BL.outputs(out, rv, lay)
        for j in range(n):
            i, size = which[j], rv0[which[j]]
            if caps[j] == bounds[i]:
                assert int(rv[j]) == size and outs[j] == full[i], (gap, lens[i], caps[j], int(rv[j]))
            elif caps[j] < size:
                assert int(rv[j]) == 0, (gap, lens[i], caps[j], int(rv[j]))
            else:
                # (the records live in the launch's scratch, not in the slot: a stream that fits is written)
                assert int(rv[j]) == size and outs[j] == full[i], (gap, lens[i], caps[j], int(rv[j]))
    # above the declared maximum
    sel = [base[:100], base[:20000], base[:20001], base[:4096]]
    bound = tc.compress_bound(20001, ZLIB)
    lay = BL.build(sel, [bound] * 4, [1, 2, 3, 4], [5, 6, 7, 8], "ff")
    rv, out, src = BC.device_compress(tc, lay, ZLIB, max_src_length=20000)
    BL.check(out, src, lay)
    outs = BL.outputs(out, rv, lay)
    a = int(lay.dst_offsets[2])
    assert int(rv[2]) == INT32_MIN and bool((out[a:a + bound] == lay.fill).all())
    for i in (0, 1, 3):
        assert int(rv[i]) > 0 and restores(O, outs[i], sel[i]), i
    with pytest.raises(Exception):                    # a declared maximum above 65,535: TYCHE_E_BAD_ARGS, as without the knob
        BC.device_compress(tc, lay, ZLIB, max_src_length=65536)


# ---------------------------------------------------------------- entry points
ENTRY_SIZES = [16384, 8192, 4097, 1000, 65, 13, 1, 12000]


def _entry_pages(O):
    data = O.pagegen(4, 32768, seed=12, first=77, dist=1).tobytes()
    return [data[i * 777:i * 777 + n] for i, n in enumerate(ENTRY_SIZES)]


# One run of every entry point (the device batch and the packed store through the Python helpers,
# the host calls through the C ABI); with a second argument "knob" the mode is switched on by
# tyche_set_knob instead of the environment, and a last round after tyche_clear_knob is printed too.
CHILD = r"""
import ctypes, hashlib, sys
import numpy as np
import torch                        # (first, as in every test process: the library binds to the HIP runtime torch loaded)
from oracle import oracle as O
from tyche_amd import _lib, buffer as B, codec
lib = _lib.load()
ZLIB = 2
sizes = %r
by_knob = %r
data = O.pagegen(4, 32768, seed=12, first=77, dist=1).tobytes()
pages = [data[i * 777:i * 777 + n] for i, n in enumerate(sizes)]
n = len(pages)
big = [p.tobytes() for p in O.pagegen(100, 16384, seed=12, first=90, dist=0)]   # 1.6 MB: two chunks at HOST_CHUNK_MB=1

def host(tag, sel):
    m = len(sel)
    caps = [int(lib.tyche_compress_bound(ZLIB, len(p))) for p in sel]
    src = [np.frombuffer(p, np.uint8).copy() for p in sel]
    out = [np.full(c + 64, 0xAB, np.uint8) for c in caps]
    vp, u32 = ctypes.c_void_p * m, ctypes.c_uint32 * m
    res = (ctypes.c_int32 * m)()
    rc = lib.tyche_compress_host(ZLIB, 1, m, vp(*[s.ctypes.data for s in src]), u32(*[len(p) for p in sel]),
                                 vp(*[o.ctypes.data for o in out]), u32(*caps), res)
    assert rc == 0, _lib.last_error()
    for o, c in zip(out, caps):
        assert bool((o[c:] == 0xAB).all()), "wrote past a capacity"
    print(tag, " ".join(hashlib.sha256(o[:max(r, 0)].tobytes()).hexdigest() for o, r in zip(out, res)))

rows = O.pagegen(8, 4096, seed=2, first=30, dist=5)

def device(prefix):
    dev_rows = torch.from_numpy(rows).cuda()
    comp, clen = codec.compress_pages(dev_rows, compressor_id=ZLIB)             # tyche_compress_batch
    torch.cuda.synchronize()
    ch, lh = comp.cpu().numpy(), clen.cpu().numpy()
    assert (lh > 0).all()
    print(prefix + "batch", " ".join(hashlib.sha256(ch[i, :int(lh[i])].tobytes()).hexdigest() for i in range(len(rows))))
    arena = torch.empty((rows.size + 65536,), dtype=torch.uint8, device=dev_rows.device)
    offs, lens, state = codec.compress_pages_packed(dev_rows, arena, chunk_pages=3, compressor_id=ZLIB)
    torch.cuda.synchronize()
    a, o, l = arena.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
    assert (l > 0).all() and int(state.cpu()[0]) >= int(o[-1]) + int(l[-1])
    print(prefix + "packed", " ".join(hashlib.sha256(a[int(o[i]):int(o[i]) + int(l[i])].tobytes()).hexdigest()
                                       for i in range(len(rows))))

def round_(prefix):
    device(prefix)
    host(prefix + "host", pages)
    host(prefix + "host1", pages[:1])
    host(prefix + "hostbig", big)
    buf = B.new_buffer(pages[0], id=7)
    rv, comp = B.buffer__compress(buf, ZLIB, 1)
    assert rv == _lib.E_OK and comp
    B.swap_data(buf, comp)
    print(prefix + "buffer", hashlib.sha256(B.buffer_bytes(buf)).hexdigest())
    assert B.buffer__decompress(buf, ZLIB) == 0 and B.buffer_bytes(buf) == pages[0]
    B.destroy(buf)
    bufs = [B.new_buffer(p, id=i) for i, p in enumerate(pages)]
    rc, st, ptrs = B.buffers_compress(bufs, ZLIB, 1)
    assert rc == 0 and st == [0] * n
    for b, p in zip(bufs, ptrs):
        assert p
        B.swap_data(b, p)
    print(prefix + "buffers", " ".join(hashlib.sha256(B.buffer_bytes(b)).hexdigest() for b in bufs))
    rc, st = B.buffers_decompress(bufs, ZLIB)
    assert rc == 0 and st == [0] * n
    assert [B.buffer_bytes(b) for b in bufs] == pages
    for b in bufs:
        B.destroy(b)

if by_knob:
    _lib.set_knob("ZLIB_HC", 1)
round_("")
if by_knob:
    _lib.clear_knob("ZLIB_HC")
    round_("off_")
print("child ok")
"""


def _run_child(env_hc, by_knob):
    env = dict(os.environ, PYTHONPATH=C.ROOT, TYCHE_HOST_CHUNK_MB="1")
    env.pop("TYCHE_ZLIB_HC", None)
    if env_hc:
        env["TYCHE_ZLIB_HC"] = "1"
    p = subprocess.run([sys.executable, "-c", CHILD % (ENTRY_SIZES, by_knob)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr[-2000:]
    return {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines() if ln and ln != "child ok"}


def _packed(tc, pages_2d):
    arena = torch.empty((pages_2d.size + 65536,), dtype=torch.uint8, device=DEV)
    offs, lens, state = tc.compress_pages_packed(_dev(pages_2d), arena, chunk_pages=3, compressor_id=ZLIB)
    torch.cuda.synchronize()
    a, o, l = arena.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
    return [a[int(o[i]):int(o[i]) + int(l[i])].tobytes() for i in range(len(pages_2d))]


def test_entry_points_with_the_environment_variable_and_the_knob(tc, oracle_mod, knobs):
    """The HC bytes are taken here from tyche_compress_batch under the knob, and are not the default
    encoder's.  tyche_compress_batch (compress_pages), compress_pages_packed, tyche_compress_host
    (one page and eight: a single chunk; 100 pages of 16 KiB at a host chunk of 1 MiB: more than
    one), buffer__compress followed by buffer__decompress and tyche_buffers_compress give the same
    bytes with TYCHE_ZLIB_HC=1 in the environment of a fresh process and with tyche_set_knob in
    another, and the default's after tyche_clear_knob."""
    O = oracle_mod
    pages = _entry_pages(O)
    plain = compress_list(tc, pages)[1]
    rows = O.pagegen(8, 4096, seed=2, first=30, dist=5)
    plain_rows, plain_packed = compress_rows(tc, rows), _packed(tc, rows)
    assert plain_packed == plain_rows
    knobs(ZLIB_HC=1)
    want = compress_list(tc, pages)[1]
    assert want != plain and all(restores(O, s, p) for s, p in zip(want, pages))
    hc_rows = compress_rows(tc, rows)
    assert _packed(tc, rows) == hc_rows and hc_rows != plain_rows
    from tyche_amd import _lib
    _lib.clear_knob("ZLIB_HC")
    assert _packed(tc, rows) == plain_rows
    sha = lambda streams: [hashlib.sha256(s).hexdigest() for s in streams]
    want, plain = sha(want), sha(plain)
    big = O.pagegen(100, 16384, seed=12, first=90, dist=0)
    plain_big = sha(compress_rows(tc, big))
    knobs(ZLIB_HC=1)
    want_big = sha(compress_rows(tc, big))
    _lib.clear_knob("ZLIB_HC")
    assert want_big != plain_big
    for env_hc, by_knob in ((True, False), (False, True)):
        got = _run_child(env_hc, by_knob)
        assert got["host"] == want and got["host1"] == [want[0]] and got["hostbig"] == want_big, (env_hc, by_knob)
        assert got["buffer"] == [want[0]] and got["buffers"] == want, (env_hc, by_knob)
        assert got["batch"] == sha(hc_rows) and got["packed"] == sha(hc_rows), (env_hc, by_knob)
        if by_knob:
            assert got["off_host"] == plain and got["off_host1"] == [plain[0]] and got["off_hostbig"] == plain_big
            assert got["off_buffer"] == [plain[0]] and got["off_buffers"] == plain
            assert got["off_batch"] == sha(plain_rows) and got["off_packed"] == sha(plain_rows)


# ---------------------------------------------------------------- other codecs
def test_other_codecs_ignore_the_knob(tc, oracle_mod, knobs):
    """LZ4 and zstd keep their bytes under ZLIB_HC=1; zlib keeps its under LZ4_HC=1 and ZSTD_HC=1,
    with its own knob off and on."""
    host = oracle_mod.pagegen(8, 8192, dist=0)
    before = {c: compress_rows(tc, host, c) for c in (LZ4, ZLIB, ZSTD)}
    knobs(ZLIB_HC=1)
    zhc = compress_rows(tc, host, ZLIB)
    assert zhc != before[ZLIB] and compress_rows(tc, host, LZ4) == before[LZ4] and compress_rows(tc, host, ZSTD) == before[ZSTD]
    knobs(LZ4_HC=1, ZSTD_HC=1)
    assert compress_rows(tc, host, ZLIB) == zhc
    assert compress_rows(tc, host, LZ4) != before[LZ4] and compress_rows(tc, host, ZSTD) != before[ZSTD]
    knobs(ZLIB_HC=0)
    assert compress_rows(tc, host, ZLIB) == before[ZLIB]


# ---------------------------------------------------------------- knob off
def test_knob_off_keeps_the_recorded_bytes(tc, oracle_mod):
    """The default encoder's streams on the case set and on 16 bench pages per distribution at
    16 KiB have the lengths and sha256 digests recorded from the library as it stood before this
    mode (tests/golden/zlib_default_digests.json, tools/gen_zlib_hc_golden.py --digests), with the
    knob never set, at 0, and after tyche_clear_knob; with the knob at 1 in between they differ, except on the
    random pages of distribution 4, which both encoders store."""
    from tyche_amd import _lib
    with open(C.DEFAULT_DIGESTS) as f:
        gold = json.load(f)
    for group, pages in C.knob_off_sets(oracle_mod).items():
        try:
            _lib.clear_knob("ZLIB_HC")
            before = compress_list(tc, pages, max_src_length=65535)[1]
            _lib.set_knob("ZLIB_HC", 1)
            hc = compress_list(tc, pages, max_src_length=65535)[1]
            _lib.set_knob("ZLIB_HC", 0)
            zero = compress_list(tc, pages, max_src_length=65535)[1]
            _lib.clear_knob("ZLIB_HC")
            cleared = compress_list(tc, pages, max_src_length=65535)[1]
        finally:
            _lib.clear_knob("ZLIB_HC")
        assert [len(s) for s in before] == gold[group]["len"], group
        assert digest(before) == gold[group]["sha"], group
        assert zero == before and cleared == before, group
        # (random pages are stored by both encoders)
        assert (hc != before) == (group != "bench4/16384"), group


# ---------------------------------------------------------------- ratio
def test_ratio_closes_half_of_the_gap_to_level_6(tc, oracle_mod):
    """Totals over 48 oracle.pagegen pages (first=1000) per distribution and page length.  L1 and
    L6: the reference's compress2 at levels 1 and 6 (tests/golden/zlib_hc_targets.json); D: the
    default device encoder, here, knob off; H: ZLIB_HC=1.  In the nine cells of distributions 0, 1
    and 5, H <= L1 - (L1 - L6) / 2; in all twelve (distribution 2 included) H <= D."""
    from tyche_amd import _lib
    O = oracle_mod
    t = C.targets()["cells"]
    failures = []
    for dist in C.RATIO_DISTS + C.NOGROW_DISTS:
        for plen in C.RATIO_LENS:
            host = C.ratio_pages(O, dist, plen)
            try:
                _lib.clear_knob("ZLIB_HC")
                d = sum(len(s) for s in compress_rows(tc, host))
                _lib.set_knob("ZLIB_HC", 1)
                h = sum(len(s) for s in compress_rows(tc, host))
            finally:
                _lib.clear_knob("ZLIB_HC")
            l1, l6 = t[f"{dist}/{plen}"]
            share = (l1 - h) / (l1 - l6)
            print(json.dumps({"dist": dist, "page_len": plen, "device_default": d, "device_hc": h, "level1": l1,
                              "level6": l6, "share_closed": round(share, 3)}))
            if h > d:
                failures.append(("above the default encoder", dist, plen, d, h))
            if dist in C.RATIO_DISTS and h > C.ratio_bar(l1, l6):
                failures.append(("less than half of the gap", dist, plen, l1, l6, h, round(share, 3)))
    assert not failures, failures
