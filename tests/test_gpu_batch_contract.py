"""The batch contract of include/tyche_codec.h as a tested property of every core (<= 64 KiB)
kernel path, on the checked layout of batch_layout.py:

* nothing outside [dst + dst_offsets[i], + dst_capacities[i]) is written -- 64 guard bytes on either
  side of every slot, slots at every byte alignment (dst_shifts i % 16), sources too ((7 i) % 16);
* src is never written, and no result depends on the bytes around a stream (input isolation: the
  same batch with zero, 0xFF and random gaps);
* compress gives 0 when the output does not fit, and never writes past the capacity it was given;
* a page above the launch's declared maximum gives INT32_MIN and leaves its slot alone;
* the host entry points keep the same promises for host pointers.

Expected values come from the oracle (and the reference decoders when oracle/_ref is built), as
in the codec suites; the corpora are those test_batch_contract_corpus.py vets on the CPU.
"""
import ctypes

import numpy as np
import pytest

import batch_contract_cases as C
import batch_layout as BL
from batch_contract_cases import LZ4, ZLIB, ZSTD, INT32_MIN
from test_gpu_zstd import DECODE_MODES, ENCODE_MODES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return codec


# ------------------------------------------------------------------ kernel paths
WAVE = dict(LZ4_SOLO_MAX=0, LZ4_JUMP_MAX=0)
# name -> (knobs, the kernel launch_lz4_decode must pick, wide batch, declared max_src_length)
LZ4_DECODE = {
    "solo": (dict(), "solo", None, None),
    "solo_lockstep": (dict(LZ4_SOLO_ASYNC=1), "solo", None, None),
    "jump": (dict(LZ4_SOLO_MAX=0), "jump", 32768, None),
    "wave": (WAVE, "wave", 65536, None),
    "lc128": (dict(LZ4_LC=1, LZ4_LANE_MIN=0, LZ4_LC_RING=128), "lc", 65536, None),
    "lc256": (dict(LZ4_LC=1, LZ4_LANE_MIN=0, LZ4_LC_RING=256), "lc", 65536, None),
    "serial": (WAVE, "serial", 65536, 90000),
}
ZSTD_DECODE = dict(default=dict(), **DECODE_MODES)
ZLIB_INFLATE = {f"par{p}_jump{j}_wg{w}": dict(ZLIB_PAR=p, ZLIB_JUMP_MAX=j, ZLIB_JUMP_WG=w)
                for p, j, w in ((0, 512, 1), (1, 512, 1), (1, 512, 0), (1, 0, 1))}
LZ4_ENCODE = {"default": dict(), "one_wave": dict(LZ4_ENC=1), "waves2": dict(LZ4_ENC_WAVES=2),
              "waves3": dict(LZ4_ENC_WAVES=3), "waves4": dict(LZ4_ENC_WAVES=4), "waves8": dict(LZ4_ENC_WAVES=8),
              "split_min0": dict(LZ4_SPLIT_MIN=0)}
ZSTD_ENCODE = dict(default=dict(), **ENCODE_MODES)


def lz4_decode_kernel(count, in_cap, out_cap, kn):
    """launch_lz4_decode's choice (lz4_decode.hip, lz4_decode_lane.hip) restated, so that a test
    named after a kernel fails if its batch would be sent to another one."""
    up16 = lambda x: (x + 15) & ~15
    lane_min = kn.get("LZ4_LANE_MIN", 32768)
    if 0 <= lane_min <= count and in_cap <= 4 << 20 and out_cap <= 4 << 20:
        return "lc"
    stage = up16(in_cap + 16 + 64)                       # the staged stream + kPad
    cells = 2 * ((out_cap + 63) & ~63)
    if count <= kn.get("LZ4_SOLO_MAX", 4096) and out_cap <= 32768 and in_cap < 3 * 8 * 1024:   # solo_layout
        chain = 2 * up16(2 * (in_cap + 1)) + up16(in_cap + 8)
        total = 256 + stage + max(chain, cells + 8 * (in_cap // 3 + 3)) + up16(2 * (((out_cap + 63) & ~63) // 4))
        if total <= 160 * 1024:
            return "solo"
    if count < kn.get("LZ4_JUMP_MAX", 16384) and out_cap <= 32768:
        rows = min(max(out_cap // 512, 24), 64)
        lds = (32 + 4 * 512 + 4 * 3 * 64) + max(cells, up16(in_cap + 4)) + 8 * (out_cap // 17 + 2) + 256 * rows + 8 * 512 + stage
        if lds <= 150 * 1024:
            return "jump"
    if up16(max(out_cap, in_cap + 4) + 16) + stage > 160 * 1024:
        return "large" if up16(out_cap) + stage > 160 * 1024 else "serial"
    return "large" if out_cap > 65536 else "wave"


def test_lz4_decode_kernel_choice_restated():
    """The restatement on launches whose kernel the suites already document."""
    assert lz4_decode_kernel(1, 6000, 16384, {}) == "solo"
    assert lz4_decode_kernel(300, 16500, 16384, {}) == "solo"
    assert lz4_decode_kernel(300, 32900, 32768, {}) == "jump"          # a 32 KiB page does not fit solo's LDS
    assert lz4_decode_kernel(4097, 16500, 16384, {}) == "jump"
    assert lz4_decode_kernel(20000, 16500, 16384, {}) == "wave"
    assert lz4_decode_kernel(65536, 16500, 16384, {}) == "lc"
    assert lz4_decode_kernel(1, 65800, 65535, {}) == "wave"
    assert lz4_decode_kernel(1, 65800, 65537, {}) == "large"
    assert lz4_decode_kernel(1, 90000, 65536, WAVE) == "serial" and lz4_decode_kernel(1, 90000, 16484, WAVE) == "serial"
    assert lz4_decode_kernel(1, 90000, 80000, WAVE) == "large"


# ------------------------------------------------------------------ (a) decode
def _batches(n):
    return [range(a, min(a + C.MAX_BATCH, n)) for a in range(0, n, C.MAX_BATCH)]


def run_decode(tc, codec, cases, want, gap="zero", max_src_length=None, lz4_path=None):
    """Runs the cases in batches of at most MAX_BATCH on the checked layout, every alignment on
    both sides; asserts the guards, the source, rv <= cap and the codec's expected values (LZ4: the
    oracle's exact return, bytes where the stream was not flipped; zlib: exact return and bytes;
    zstd: size and bytes on success, any error on failure).  Returns (results, outputs)."""
    all_rv, all_out = [], []
    for idx in _batches(len(cases)):
        part = [cases[i] for i in idx]
        n = len(part)
        lay = BL.build([c.stream for c in part], [c.cap for c in part], C.src_shifts(n), C.dst_shifts(n), gap)
        if lz4_path is not None:
            kn, kernel = lz4_path
            in_cap = max_src_length or max(max(int(x) for x in lay.src_lengths), 1)
            assert lz4_decode_kernel(n, in_cap, int(lay.caps.max()), kn) == kernel, (n, in_cap, int(lay.caps.max()))
        rv, out, src = C.device_decode(tc, lay, codec, max_src_length=max_src_length)
        BL.check(out, src, lay)
        outs = BL.outputs(out, rv, lay)
        for j, i in enumerate(idx):
            c, (wrv, wout) = cases[i], want[i]
            assert rv[j] <= c.cap, (i, c.kind, rv[j], c.cap)
            assert C.verdict_matches(codec, int(rv[j]), wrv), (i, c.kind, c.cap, len(c.stream), int(rv[j]), wrv)
            if wrv > 0 and (codec != LZ4 or c.exact):
                assert outs[j] == wout, (i, c.kind, c.cap, wrv)
        all_rv += [int(x) for x in rv]
        all_out += outs
    return all_rv, all_out


@pytest.mark.parametrize("path", list(LZ4_DECODE))
def test_lz4_decode_contract(tc, knobs, path):
    """Every LZ4 decode kernel of pages up to 64 KiB: placement, capacities, guards.

    serial: with the wave knobs (no solo, no jump decoder) and a declared max_src_length of 90,000,
    launch_lz4_decode computes for the wave decoder off_in = up16(max(out_cap, 90,004) + 16) = 90,032
    and lds = 90,032 + up16(90,000 + 16 + 64) = 180,112 > 163,840, so it takes the branch for large
    pages; there lds2 = up16(out_cap) + 90,080 is 106,576 for the small batch (out_cap 16,484) and
    155,616 for the wide one (65,536), both <= 163,840: lz4_decode_serial_kernel is launched, not
    the ring decoder.  lz4_decode_kernel() above restates that arithmetic and is asserted per batch."""
    kn, kernel, wide, max_src = LZ4_DECODE[path]
    knobs(**kn)
    for which in ["small"] + ([wide] if wide else []):
        cases, want = C.corpus(LZ4, which), C.expected(LZ4, which)
        run_decode(tc, LZ4, cases, want, max_src_length=max_src, lz4_path=(kn, kernel))


@pytest.fixture(scope="module")
def zstd_extra(tc):
    """Device-encoded frames (the default encoder) of pages of the odd lengths, small and wide, each
    restored by the oracle before it may serve as a valid stream."""
    O = C.oracle()
    out = {}
    for which, sizes in (("small", C.SIZES), (32768, (32768, 32767, 32755))):
        pages = [C.page(plen, k) for k, plen in enumerate(sizes)]
        lay = BL.build(pages, [tc.compress_bound(len(p), ZSTD) for p in pages], 0, 0, "zero")
        rv, arena, src = C.device_compress(tc, lay, ZSTD)
        BL.check(arena, src, lay)
        frames = BL.outputs(arena, rv, lay)
        for p, f in zip(pages, frames):
            r, dec = O.zstd_decompress(f, len(p))
            assert f and r == len(p) and bytes(dec)[:r] == p
        out[which] = tuple((f, len(p)) for p, f in zip(pages, frames))
    return out


@pytest.mark.parametrize("mode", list(ZSTD_DECODE))
def test_zstd_decode_contract(tc, knobs, zstd_extra, mode):
    """The default launch (no knob: the one-launch kernels at these batch sizes) and every entry of
    test_gpu_zstd's DECODE_MODES; the corpus is the golden one plus device-encoded frames."""
    knobs(**ZSTD_DECODE[mode])
    for which in ("small", 32768):
        cases, want = C.corpus(ZSTD, which, zstd_extra[which]), C.expected(ZSTD, which, zstd_extra[which])
        run_decode(tc, ZSTD, cases, want)


@pytest.mark.parametrize("path", list(ZLIB_INFLATE))
def test_zlib_inflate_contract(tc, knobs, path):
    """The serial kernel, and the lane-parallel one with each match phase (workgroup or wave jump
    kernel, frontier copies)."""
    knobs(**ZLIB_INFLATE[path])
    for which in ("small", 32768):
        run_decode(tc, ZLIB, C.corpus(ZLIB, which), C.expected(ZLIB, which))


# ------------------------------------------------------------------ (b) input isolation
ISOLATION = [(LZ4, "default", dict()), (LZ4, "wave", WAVE), (ZSTD, "default", dict()),
             (ZSTD, "seqexec", DECODE_MODES["seqexec"]), (ZLIB, "default", dict()), (ZLIB, "par0", dict(ZLIB_PAR=0))]


@pytest.mark.parametrize("codec,path,kn", ISOLATION, ids=[f"{C.NAMES[c]}-{p}" for c, p, _ in ISOLATION])
def test_input_isolation(tc, knobs, codec, path, kn):
    """The kernels stage whole 16-byte lines, so they see bytes before and after a stream; no verdict
    (a third of the batch is truncated streams) and no output byte may depend on them."""
    knobs(**kn)
    cases, want = C.corpus(codec, "small"), C.expected(codec, "small")
    idx = C.isolation_subset(cases)
    cases, want = [cases[i] for i in idx], [want[i] for i in idx]
    assert sum(c.kind == "trunc" for c in cases) * 4 >= len(cases)
    runs = [run_decode(tc, codec, cases, want, gap=gap) for gap in ("zero", "ff", ("random", 1))]
    for rv, outs in runs[1:]:
        assert rv == runs[0][0]
        for i, c in enumerate(cases):
            if rv[i] > 0 and (codec != LZ4 or c.exact):
                assert outs[i] == runs[0][1][i], (i, c.kind)


# ------------------------------------------------------------------ (c) compress: limited output
def run_compress(tc, codec, pages, caps, gap="zero", max_src_length=None):
    n = len(pages)
    lay = BL.build(pages, caps, C.src_shifts(n), C.dst_shifts(n), gap)
    rv, out, src = C.device_compress(tc, lay, codec, max_src_length=max_src_length)
    BL.check(out, src, lay)
    return [int(x) for x in rv], out, lay


def limited_output(tc, codec, exact):
    """Run 1 at tyche_compress_bound: every page compresses and restores; S_i is its size.  Run 2:
    every page at each of the eight capacities of limited_caps (S_i - 1, S_i, S_i + 1, S_i + 7,
    S_i / 2, 1, 0, bound - 1): 0 <= rv <= cap, whatever is returned restores, guards and source
    intact.  exact (LZ4, whose checks are exact and whose encoder is deterministic): rv == S_i with
    the bytes of run 1 when cap >= S_i, 0 below.

    Twice: all pages in a launch that declares 16,384 bytes, then the pages of up to 1,000 bytes in
    one that declares 1,000 -- the encoders pick their kernel by the declared maximum (LZ4: the
    split kernels from 8,192 or 12,288 bytes, from 0 under LZ4_SPLIT_MIN=0)."""
    for declared in (16384, 1000):
        pages = [p for p in C.compress_pages() if len(p) <= declared]
        bounds = [tc.compress_bound(len(p), codec) for p in pages]
        rv1, out1, lay1 = run_compress(tc, codec, pages, bounds, max_src_length=declared)
        first = BL.outputs(out1, rv1, lay1)
        for i, p in enumerate(pages):
            assert 0 < rv1[i] <= bounds[i], (declared, i, len(p), rv1[i])
            assert C.restores(codec, first[i], p), (declared, i, len(p), rv1[i])
        pages2 = [p for p in pages for _ in range(8)]
        caps2 = [c for i in range(len(pages)) for c in C.limited_caps(rv1[i], bounds[i])]
        assert len(pages2) <= C.MAX_BATCH
        rv2, out2, lay2 = run_compress(tc, codec, pages2, caps2, gap=("random", 2), max_src_length=declared)
        second = BL.outputs(out2, rv2, lay2)
        for j, p in enumerate(pages2):
            i, cap, size = j // 8, caps2[j], rv1[j // 8]
            assert 0 <= rv2[j] <= cap, (declared, i, len(p), cap, size, rv2[j])
            if exact:
                assert rv2[j] == (size if cap >= size else 0), (declared, i, len(p), cap, size, rv2[j])
                assert second[j] == (first[i] if cap >= size else b""), (declared, i, len(p), cap, size)
            if rv2[j] > 0:
                assert C.restores(codec, second[j], p), (declared, i, len(p), cap, size, rv2[j])


@pytest.mark.parametrize("variant", list(LZ4_ENCODE))
def test_lz4_compress_limited_output(tc, knobs, variant):
    """The default encoder, the one-wave kernel, the two-wave and the 3/4/8-wave splits, and the
    three-wave split on every page size: the exact `op + ... > cap` checks and the part join under
    capacities one byte either side of the stream's size."""
    knobs(**LZ4_ENCODE[variant])
    limited_output(tc, LZ4, exact=True)


@pytest.mark.parametrize("mode", list(ZSTD_ENCODE))
def test_zstd_compress_limited_output(tc, knobs, mode):
    """A 0 at or above S_i is allowed (the literal scratch sits at the capacity's tail and the
    blocks fall back); no share of successes is asserted."""
    knobs(**ZSTD_ENCODE[mode])
    limited_output(tc, ZSTD, exact=False)


@pytest.mark.parametrize("path", ["default"])
def test_zlib_compress_limited_output(tc, path):
    """As zstd: the parse records sit below the stream, a tight capacity re-codes or gives 0."""
    limited_output(tc, ZLIB, exact=False)


# ------------------------------------------------------------------ (d) over the declared maximum
def _valid_stream(tc, codec, data):
    if codec != ZSTD:
        return C._encode(codec, data, 1)
    lay = BL.build([data], [tc.compress_bound(len(data), ZSTD)], 0, 0, "zero")
    rv, out, _ = C.device_compress(tc, lay, ZSTD)
    return BL.outputs(out, rv, lay)[0]


@pytest.mark.parametrize("codec", [LZ4, ZLIB, ZSTD], ids=["lz4", "zlib", "zstd"])
def test_page_over_declared_maximum(tc, codec):
    """One page of an ordinary batch above the launch's declared maximum: exactly INT32_MIN, its
    slot and guards untouched, every other page as without it.

    compress: a source length above max_src_length.  decompress: a capacity above dst_capacity; and a
    stream longer than the declared max_src_length, which LZ4 and zstd refuse with INT32_MIN (the
    kernels test src_len > in_cap before staging: lz4_decode.hip, zstd_decode.hip `p.src_len > in_cap`)
    while zlib, whose kernels read the stream from memory through a window and test the capacity
    alone (zlib_inflate.hip `p.dst_cap > out_cap`), gives the oracle's verdict."""
    n, bad, plen = 12, 5, 4096
    pages = [C.page(plen - 100 + k, k % 6) for k in range(n)]   # at least 89 bytes short of plen, compressible or not
    over = C.page(plen + 1, 3)
    # compress
    bound = tc.compress_bound(plen + 1, codec)
    rv0, out0, lay0 = run_compress(tc, codec, pages, [bound] * n, max_src_length=plen)
    src = pages[:bad] + [over] + pages[bad + 1:]
    rv, out, lay = run_compress(tc, codec, src, [bound] * n, max_src_length=plen)
    a = int(lay.dst_offsets[bad])
    assert rv[bad] == INT32_MIN and (out[a:a + bound] == lay.fill).all()
    got, ref = BL.outputs(out, rv, lay), BL.outputs(out0, rv0, lay0)
    for i in range(n):
        if i != bad:
            assert rv[i] == rv0[i] > 0 and got[i] == ref[i] and C.restores(codec, got[i], pages[i]), i
    # decompress: a capacity above the declared one
    streams = [_valid_stream(tc, codec, p) for p in pages]
    caps = [len(p) for p in pages]
    caps[bad] = plen + 904
    lay = BL.build(streams, caps, C.src_shifts(n), C.dst_shifts(n), "ff")
    rv, out, s_after = C.device_decode(tc, lay, codec, max_capacity=plen)
    BL.check(out, s_after, lay)
    a = int(lay.dst_offsets[bad])
    assert rv[bad] == INT32_MIN and (out[a:a + caps[bad]] == lay.fill).all()
    got = BL.outputs(out, rv, lay)
    for i in range(n):
        if i != bad:
            assert rv[i] == len(pages[i]) and got[i] == pages[i], (i, rv[i])
    # decompress: a stream longer than the declared maximum
    declared = max(len(s) for s in streams)
    long_stream = _valid_stream(tc, codec, np.random.default_rng(9).integers(0, 256, plen, dtype=np.uint8).tobytes())
    assert len(long_stream) > declared
    streams2 = streams[:bad] + [long_stream] + streams[bad + 1:]
    caps[bad] = plen
    lay = BL.build(streams2, caps, C.src_shifts(n), C.dst_shifts(n), ("random", 5))
    rv, out, s_after = C.device_decode(tc, lay, codec, max_src_length=declared)
    BL.check(out, s_after, lay)
    got = BL.outputs(out, rv, lay)
    if codec == ZLIB:
        assert rv[bad] == plen and C.restores(ZLIB, long_stream, got[bad])
    else:
        a = int(lay.dst_offsets[bad])
        assert rv[bad] == INT32_MIN and (out[a:a + plen] == lay.fill).all()
    for i in range(n):
        if i != bad:
            assert rv[i] == len(pages[i]) and got[i] == pages[i], (i, rv[i])


# ------------------------------------------------------------------ (e) host entry points
HOST_KNOBS = {"default": dict(), "no_zero_copy": dict(ZERO_COPY_BYTES=0), "staged_out": dict(HOST_DIRECT_OUT=0)}
_vp, _u32, _i32p = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)


def _host_call(fn, head, lay):
    """Calls a host entry point with every pointer inside the layout's two arenas (copies: the
    kernels, the copies and the scatter write into them directly).  Returns (rc, results, out, src)."""
    n = lay.count
    out, src = lay.out.copy(), lay.src.copy()
    res = np.full(n, 0x5A5A5A5A, np.int32)
    sp = (_vp * n)(*[src.ctypes.data + int(o) for o in lay.src_offsets])
    dp = (_vp * n)(*[out.ctypes.data + int(o) for o in lay.dst_offsets])
    assert all(p % 2 == 1 for p in sp) and all(p % 2 == 1 for p in dp)
    rc = fn(*head, n, sp, (_u32 * n)(*[int(x) for x in lay.src_lengths]), dp, (_u32 * n)(*[int(x) for x in lay.caps]),
            res.ctypes.data_as(_i32p))
    return rc, [int(x) for x in res], out, src


def _odd(n, mul):
    return [(2 * (mul * i % 8) + 1) for i in range(n)]


@pytest.mark.parametrize("kn", list(HOST_KNOBS))
@pytest.mark.parametrize("codec", [LZ4, ZLIB, ZSTD], ids=["lz4", "zlib", "zstd"])
def test_host_entry_points(tc, knobs, codec, kn):
    """tyche_compress_host and tyche_decompress_host on 96 pages of up to 16 KiB whose sources and
    destinations all lie in one guarded arena each, at odd addresses, every 5th destination short:
    with the zero-copy path and kernels writing straight into the pinned arena (the defaults), with
    staging copies instead (ZERO_COPY_BYTES=0), and with the output staged through HBM
    (HOST_DIRECT_OUT=0).  Results, bytes and guards as on the device paths."""
    from tyche_amd import _lib
    lib = _lib.load()
    knobs(**HOST_KNOBS[kn])
    n = 96
    sizes = [(16384, 8192, 4097, 1000, 65, 16, 1, 12000)[i % 8] for i in range(n)]
    pages = [C.page(sizes[i], i) for i in range(n)]
    assert lib.tyche_set_device(0) == 0
    try:
        # compress: run 1 at the bound, run 2 with every 5th capacity half the stream's size
        bounds = [tc.compress_bound(len(p), codec) for p in pages]
        lay = BL.build(pages, bounds, _odd(n, 3), _odd(n, 1), ("random", 7))
        rc, rv1, out, src = _host_call(lib.tyche_compress_host, (codec, 1), lay)
        assert rc == 0, _lib.last_error()
        BL.check(out, src, lay)
        first = BL.outputs(out, rv1, lay)
        for i, p in enumerate(pages):
            assert 0 < rv1[i] <= bounds[i] and C.restores(codec, first[i], p), (i, len(p), rv1[i])
        caps = [rv1[i] // 2 if i % 5 == 4 else (rv1[i] if i % 5 == 3 else bounds[i]) for i in range(n)]
        lay = BL.build(pages, caps, _odd(n, 3), _odd(n, 1), "ff")
        rc, rv2, out, src = _host_call(lib.tyche_compress_host, (codec, 1), lay)
        assert rc == 0, _lib.last_error()
        BL.check(out, src, lay)
        second = BL.outputs(out, rv2, lay)
        for i, p in enumerate(pages):
            assert 0 <= rv2[i] <= caps[i], (i, caps[i], rv2[i])
            if codec == LZ4:
                assert rv2[i] == (0 if i % 5 == 4 else rv1[i]) and second[i] == (b"" if i % 5 == 4 else first[i]), i
            elif i % 5 < 3:
                assert rv2[i] > 0, (i, rv2[i])
            if rv2[i] > 0:
                assert C.restores(codec, second[i], p, ref=False), i
        # decompress: valid streams, every 7th truncated, every 5th destination short
        if codec == ZSTD:
            streams = list(first)                         # the frames of run 1, restored by the oracle above
        else:
            streams = [C._encode(codec, p, i) for i, p in enumerate(pages)]
        rng = np.random.default_rng(11 + codec)
        cases = []
        for i, s in enumerate(streams):
            if i % 7 == 3 and len(s) > 1:
                s = s[:int(rng.integers(1, len(s)))]
            cap = sizes[i] if i % 5 != 4 else int(rng.integers(0, sizes[i]))
            cases.append(C.Case(s, cap, "host", True, sizes[i]))
        want = [C.decode_oracle(codec, c) for c in cases]
        assert sum(w[0] >= 0 for w in want) >= n // 2 and sum(w[0] < 0 for w in want) >= n // 5
        lay = BL.build([c.stream for c in cases], [c.cap for c in cases], _odd(n, 5), _odd(n, 7), ("random", 8))
        rc, rv, out, src = _host_call(lib.tyche_decompress_host, (codec,), lay)
        assert rc == 0, _lib.last_error()
        BL.check(out, src, lay)
        outs = BL.outputs(out, rv, lay)
        for i, c in enumerate(cases):
            assert C.verdict_matches(codec, rv[i], want[i][0]), (i, c.cap, len(c.stream), rv[i], want[i][0])
            if want[i][0] > 0:
                assert outs[i] == want[i][1], i
    finally:
        lib.tyche_set_device(_lib.ALL_DEVICES)
