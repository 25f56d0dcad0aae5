"""CPU checks of the host batch path's chunk plan and page-table layout
(tyche_amd/csrc/host_chunk_core.h, run by host_batch.hip) through tools/host_chunk_emul.cpp,
against a Python restatement of the rule:

  up16(x): x rounded up to 16;  chunk_bytes = max(1, HOST_CHUNK_MB) << 20
  tot_in = sum up16(src_len), tot_out = sum up16(dst_cap), est = (tot_in + tot_out) // chunk_bytes
  ramp on: est >= 3 and HOST_RAMP != 0;  quarter = max(chunk_bytes // 4, 1 MiB)
  a chunk's limit is chunk_bytes; with the ramp on and rem = max(rem_in, rem_out) the bytes not yet
  in a chunk: quarter for the first chunk, rem - quarter for a later one when
  quarter < rem <= chunk_bytes + quarter
  a chunk takes its first page whatever its size, then pages while both its input and its output
  bytes stay within the limit;  chunk c uses slot c % 4

For every case: the chunks partition [0, n), every multi-page chunk is within its limit in both
directions, and the five meta arrays are disjoint, inside k * 28 + 64 bytes, with soff and doff the
running up16 sums.  The ramp's stray one-page chunk before the last one ([92, 92, 92, 92, 51, 1, 92]
for the 512-page cycle at 1 MiB) is the rule as it stands and is
pinned here.  tools/host_chunk_emul.cpp with -DHOST_CHUNK_EMUL_MAIN runs a sweep of its own as a
stand-alone program, for sanitizer builds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "tools", "bin", "libhostchunkemul.so")
SRC = os.path.join(ROOT, "tools", "host_chunk_emul.cpp")
CORE = os.path.join(ROOT, "tyche_amd", "csrc", "host_chunk_core.h")
MIB = 1 << 20
CYCLE = (16384, 8192, 16384, 4097, 16384, 1000, 16384, 12000)   # the 512-page size cycle of the host tests


def up16(x):
    return (int(x) + 15) & ~15


def spec_cut(src_len, dst_cap, chunk_mb, ramp_wanted):
    """The rule restated: (chunks as (first, count, in_bytes, out_bytes, max_in, max_out), limits, est, ramp)."""
    n = len(src_len)
    chunk_bytes = max(1, chunk_mb) << 20
    rem_in, rem_out = sum(up16(x) for x in src_len), sum(up16(x) for x in dst_cap)
    est = (rem_in + rem_out) // chunk_bytes
    ramp = est >= 3 and bool(ramp_wanted)
    quarter = max(chunk_bytes // 4, MIB)
    chunks, limits, first = [], [], 0
    while first < n:
        limit = chunk_bytes
        if ramp:
            rem = max(rem_in, rem_out)
            if not chunks:
                limit = quarter
            elif quarter < rem <= chunk_bytes + quarter:
                limit = rem - quarter
        last, ib, ob = first + 1, up16(src_len[first]), up16(dst_cap[first])
        while last < n and ib + up16(src_len[last]) <= limit and ob + up16(dst_cap[last]) <= limit:
            ib += up16(src_len[last])
            ob += up16(dst_cap[last])
            last += 1
        chunks.append((first, last - first, ib, ob, max(int(x) for x in src_len[first:last]),
                       max(int(x) for x in dst_cap[first:last])))
        limits.append(limit)
        rem_in -= ib
        rem_out -= ob
        first = last
    return chunks, limits, est, ramp


class Emul:
    def __init__(self):
        if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in (SRC, CORE)):
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
        self.lib = ctypes.CDLL(LIB)
        vp = ctypes.c_void_p
        self.lib.host_chunk_cut.restype = ctypes.c_size_t
        self.lib.host_chunk_cut.argtypes = [ctypes.c_size_t, vp, vp, ctypes.c_long, ctypes.c_int, vp, vp, vp]
        self.lib.host_chunk_meta.restype = ctypes.c_size_t
        self.lib.host_chunk_meta.argtypes = [vp, ctypes.c_size_t, vp, vp, vp]

    def cut(self, src_len, dst_cap, chunk_mb, ramp_wanted):
        n = len(src_len)
        sl, dc = np.asarray(src_len, np.uint32), np.asarray(dst_cap, np.uint32)
        chunks, limits, info = np.zeros((n, 6), np.uint64), np.zeros(n, np.uint64), np.zeros(4, np.uint64)
        c = self.lib.host_chunk_cut(n, sl.ctypes.data, dc.ctypes.data, chunk_mb, int(ramp_wanted), chunks.ctypes.data,
                                    limits.ctypes.data, info.ctypes.data)
        assert int(info[0]) == max(1, chunk_mb) << 20 and int(info[3]) == 4
        return ([tuple(int(x) for x in row) for row in chunks[:c]], [int(x) for x in limits[:c]], int(info[1]),
                bool(info[2]))

    def meta(self, src_len, dst_cap):
        """The table of one chunk: (buffer, byte offsets of the five arrays, meta bytes); 64 guard bytes either side."""
        k = len(src_len)
        sl, dc = np.asarray(src_len, np.uint32), np.asarray(dst_cap, np.uint32)
        size = k * 28 + 64
        raw = np.full(64 + size + 64 + 8, 0xA5, np.uint8)
        pad = (-raw.ctypes.data) % 8                      # the engine's meta arenas are page-aligned
        buf = raw[pad:pad + 64 + size + 64]
        at = np.zeros(5, np.uint64)
        got = self.lib.host_chunk_meta(buf.ctypes.data + 64, k, sl.ctypes.data, dc.ctypes.data, at.ctypes.data)
        assert got == size
        assert (buf[:64] == 0xA5).all() and (buf[64 + size:] == 0xA5).all(), "wrote outside the meta buffer"
        return buf[64:64 + size], [int(x) for x in at]


@pytest.fixture(scope="module")
def emul():
    return Emul()


def check(emul, src_len, dst_cap, chunk_mb, ramp_wanted):
    """The emulator's cut against the restatement and the properties; returns the page counts."""
    want = spec_cut(src_len, dst_cap, chunk_mb, ramp_wanted)
    got = emul.cut(src_len, dst_cap, chunk_mb, ramp_wanted)
    assert got[2] == want[2] and got[3] == want[3], (got[2:], want[2:])
    assert got[0] == want[0], [c[:2] for c in got[0]]
    assert got[1] == want[1]
    at = 0
    for (first, count, ib, ob, max_in, max_out), limit in zip(*got[:2]):
        assert first == at and count >= 1
        assert count == 1 or (ib <= limit and ob <= limit)
        at += count
    assert at == len(src_len)
    for first, count, ib, ob, _, _ in got[0][:3] + got[0][-2:]:
        check_meta(emul, src_len[first:first + count], dst_cap[first:first + count], ib, ob)
    return [c[1] for c in got[0]]


def check_meta(emul, src_len, dst_cap, in_bytes=None, out_bytes=None):
    k = len(src_len)
    buf, at = emul.meta(src_len, dst_cap)
    spans = sorted(zip(at, (8 * k, 8 * k, 4 * k, 4 * k, 4 * k)))
    assert spans[0][0] == 0 and spans[-1][0] + spans[-1][1] <= k * 28 + 64
    assert all(a + la <= b for (a, la), (b, _) in zip(spans, spans[1:])), spans
    assert all(a % 8 == 0 for a in at[:2]) and all(a % 4 == 0 for a in at[2:])
    soff, doff = buf[at[0]:at[0] + 8 * k].view(np.uint64), buf[at[1]:at[1] + 8 * k].view(np.uint64)
    slen, dcap = buf[at[2]:at[2] + 4 * k].view(np.uint32), buf[at[3]:at[3] + 4 * k].view(np.uint32)
    run_in = np.concatenate(([0], np.cumsum([up16(x) for x in src_len])))
    run_out = np.concatenate(([0], np.cumsum([up16(x) for x in dst_cap])))
    assert np.array_equal(soff, run_in[:-1]) and np.array_equal(doff, run_out[:-1])
    assert np.array_equal(slen, np.asarray(src_len, np.uint32)) and np.array_equal(dcap, np.asarray(dst_cap, np.uint32))
    assert (buf[at[4]:at[4] + 4 * k] == 0xA5).all()       # res is the kernels' to write
    if in_bytes is not None:
        assert int(run_in[-1]) == in_bytes and int(run_out[-1]) == out_bytes


def test_one_page(emul):
    for ramp in (1, 0):
        assert check(emul, [6000], [16384], 32, ramp) == [1]
        assert check(emul, [0], [0], 32, ramp) == [1]


def test_one_page_larger_than_the_chunk_goes_alone(emul):
    big = 3 * MIB
    for ramp in (1, 0):
        assert check(emul, [big], [big], 1, ramp) == [1]
        assert check(emul, [100, big, 100, 100], [100, 100, 100, 100], 1, ramp)[:2] == [1, 1]
        assert check(emul, [100] * 5, [100, 100, big, 100, 100], 1, ramp) == [2, 1, 2]
        assert check(emul, [big] * 4, [big] * 4, 1, ramp) == [1, 1, 1, 1]


def test_zero_length_pages(emul):
    for ramp in (1, 0):
        assert check(emul, [0] * 1000, [0] * 1000, 1, ramp) == [1000]
        assert check(emul, [0, 16384] * 300, [16384, 0] * 300, 1, ramp)
        assert check(emul, [0] * 500, [16384] * 500, 1, ramp)


def test_lengths_that_are_no_multiple_of_16(emul):
    # 1 MiB of up16(4097) = 4112 is 255 pages: 255 x 4112 <= 1 MiB < 256 x 4112; by the raw length 255.9
    assert check(emul, [4097] * 600, [1] * 600, 1, 0) == [255, 255, 90]
    assert check(emul, [1] * 70000, [15] * 70000, 1, 0) == [65536, 4464]
    for ramp in (1, 0):
        check(emul, [1, 15, 17, 4097, 31, 33] * 200, [16, 1, 4097, 17, 65, 1000] * 200, 1, ramp)


def test_input_limit_binds(emul):
    """Incompressible streams: the bound (LZ4's 16384 + 16384 // 255 + 16 = 16464) is above the page."""
    n = 400
    src, dst = [16464] * n, [16384] * n
    per = MIB // 16464                                     # 63: by the output alone it would be 64
    assert per == 63 and MIB // 16384 == 64
    assert check(emul, src, dst, 1, 0) == [63] * 6 + [22]
    check(emul, src, dst, 1, 1)


def test_output_limit_binds(emul):
    n = 400
    src, dst = [6301] * n, [16384] * n                    # streams of size / 2.6
    assert check(emul, src, dst, 1, 0) == [64] * 6 + [16]
    check(emul, src, dst, 1, 1)


def test_ramp_threshold_est_2_and_3(emul):
    """est = (tot_in + tot_out) // chunk_bytes: 2 leaves the ramp off, 3 turns it on."""
    n = 96                                                 # 96 x 16 KiB in, the same out: 3 MiB in all
    src, dst = [16384] * n, [16384] * n
    chunks, _, est, ramp = emul.cut(src, dst, 1, 1)
    assert est == 3 and ramp
    assert check(emul, src, dst, 1, 1)[0] == 64            # quarter == chunk_bytes at 1 MiB
    src[-1] -= 16                                          # 16 bytes short of 3 MiB
    chunks, _, est, ramp = emul.cut(src, dst, 1, 1)
    assert est == 2 and not ramp
    assert check(emul, src, dst, 1, 1) == check(emul, src, dst, 1, 0) == [64, 32]
    # at 4 MiB chunks the ramp's first chunk shows: est 3 needs 12 MiB
    src, dst = [16384] * 384, [16384] * 384
    assert emul.cut(src, dst, 4, 1)[2:] == (3, True) and check(emul, src, dst, 4, 1)[0] == 64
    src[0] -= 1
    assert emul.cut(src, dst, 4, 1)[2:] == (3, True)       # up16 of the length counts, not the length
    src[0] -= 16
    assert emul.cut(src, dst, 4, 1)[2:] == (2, False) and check(emul, src, dst, 4, 1)[0] == 256


def _cycle(n):
    sizes = [CYCLE[i % 8] for i in range(n)]
    return [int(s / 2.6) for s in sizes], sizes


def test_first_chunk_quarter_rule(emul):
    src, dst = _cycle(1536)
    assert check(emul, src, dst, 4, 1)[0] == 92
    assert check(emul, src, dst, 4, 0)[0] == 368


def test_one_mib_chunks_where_the_quarter_is_the_chunk(emul):
    src, dst = _cycle(512)
    assert check(emul, src, dst, 1, 1) == [92, 92, 92, 92, 51, 1, 92]   # the stray page: DESIGN.md section 8, item 4
    assert check(emul, src, dst, 1, 0) == [92, 92, 92, 92, 92, 52]


def test_chunk_mb_below_one_is_one(emul):
    src, dst = _cycle(512)
    for mb in (0, -3):
        assert emul.cut(src, dst, mb, 1) == emul.cut(src, dst, 1, 1)


def test_seeded_random_sweep(emul):
    rng = np.random.default_rng(20240607)
    for _ in range(150):
        n = int(rng.integers(1, 3000))
        top = int(rng.choice([64, 4096, 16384, 65536, MIB]))
        src = rng.integers(0, top + 1, n)
        dst = rng.integers(0, top + 1, n)
        src[rng.random(n) < 0.1] = 0
        dst[rng.random(n) < 0.1] = 0
        mb = int(rng.choice([1, 2, 4, 32]))
        for ramp in (1, 0):
            check(emul, src.tolist(), dst.tolist(), mb, ramp)
