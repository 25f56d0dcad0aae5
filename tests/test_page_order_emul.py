"""CPU checks of the page order of the lane-per-page launches (tyche_amd/csrc/page_order_core.h)
through the host emulator tools/page_order_emul.cpp: the order array is a permutation that sorts
every window by descending length bin and keeps page order inside a bin; the slot map hands every
slot to exactly one (generation, wave, lane), 64 consecutive slots to a wave, mirrored from one
generation to the next; the bin's edge cases; and the balance model on the bench's pages -- with
the ordered walk the slowest wave of a small grid stays close to the mean lane, where the stride
walk leaves it well above.  test_gpu_lz4_order.py holds the device's order array to the emulator's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "tools", "bin", "libpageorderemul.so")
SRC = os.path.join(ROOT, "tools", "page_order_emul.cpp")
CORE = os.path.join(ROOT, "tyche_amd", "csrc", "page_order_core.h")
LC_LIB = os.path.join(ROOT, "tools", "bin", "liblcemul_f1.so")   # (test_lc_emul.py's far16 build, same command)
LC_SRC = os.path.join(ROOT, "tools", "lc_emul.cpp")
LC_CORE = [os.path.join(ROOT, "tyche_amd", "csrc", f) for f in ("lz4_lc_core.h", "byte_funnel.h")]


def _stale(lib, deps):
    return not os.path.exists(lib) or any(os.path.getmtime(f) > os.path.getmtime(lib) for f in deps)


class Emul:
    """The emulator: BINS, TILE, LANES; bin(length, in_cap); order(lengths, in_cap, window);
    slots(grid, count) -> array [generation, wave, lane] of slots, `count` where the lane has none."""

    def __init__(self):
        if _stale(LIB, (SRC, CORE)):
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
        self.lib = ctypes.CDLL(LIB)
        self.lib.page_order_emul_bin.restype = ctypes.c_uint32
        self.lib.page_order_emul_bin.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        self.lib.page_order_emul.restype = ctypes.c_int
        self.lib.page_order_emul.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        self.lib.page_order_emul_generations.restype = ctypes.c_uint64
        self.lib.page_order_emul_generations.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
        self.lib.page_order_emul_slots.restype = None
        self.lib.page_order_emul_slots.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        k = (ctypes.c_uint32 * 3)()
        self.lib.page_order_emul_constants(k)
        self.BINS, self.TILE, self.LANES = (int(x) for x in k)

    def bin(self, length, in_cap):
        return int(self.lib.page_order_emul_bin(int(length), int(in_cap)))

    def bins(self, lengths, in_cap):
        """numpy restatement of the bin: min(length, in_cap) >> the smallest shift leaving fewer than BINS values"""
        shift = 0
        while (in_cap >> shift) >= self.BINS:
            shift += 1
        return np.minimum(lengths.astype(np.int64), in_cap) >> shift

    def order(self, lengths, in_cap, window):
        lengths = np.ascontiguousarray(lengths, np.uint32)
        out = np.full(lengths.size, 0xFFFFFFFF, np.uint32)
        r = self.lib.page_order_emul(lengths.ctypes.data, lengths.size, in_cap, window, out.ctypes.data)
        assert r == 0, r
        return out

    def slots(self, grid, count):
        gens = int(self.lib.page_order_emul_generations(grid, count))
        out = np.zeros((gens, grid, self.LANES), np.uint64)
        self.lib.page_order_emul_slots(grid, count, gens, out.ctypes.data)
        return out


@pytest.fixture(scope="module")
def emul():
    return Emul()


def check_order(emul, order, lengths, in_cap, window):
    """a permutation; inside every window the bins do not increase and equal bins keep page order"""
    n = lengths.size
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)), "not a permutation"
    bins = emul.bins(lengths, in_cap)
    win = n if window == 0 or window > n else window
    for w0 in range(0, n, win):
        o = order[w0:w0 + win].astype(np.int64)
        assert o.min() >= w0 and o.max() < min(w0 + win, n), "a page left its window"
        b = bins[o]
        assert bool((np.diff(b) <= 0).all()), "bins increase inside a window"
        same = np.diff(b) == 0
        assert bool((np.diff(o)[same] > 0).all()), "equal bins out of page order"


COUNTS = [1, 63, 64, 65, 127, 4096, 4097, 10000]
GRIDS = [1, 2, 8]


def windows_for(count):
    return [0, 64, 256, 1000, count + 7]


@pytest.mark.parametrize("count", COUNTS)
def test_order_is_a_windowed_stable_sort(emul, count):
    rng = np.random.default_rng(count)
    in_cap = 4160   # LZ4's bound for 4 KiB pages
    lengths = rng.integers(0, in_cap + 200, count).astype(np.uint32)
    lengths[rng.integers(0, count, max(count // 10, 1))] = 0
    for window in windows_for(count):
        check_order(emul, emul.order(lengths, in_cap, window), lengths, in_cap, window)
    # the restated bin is the emulator's
    for x in lengths[:50]:
        assert emul.bin(x, in_cap) == int(emul.bins(np.array([x]), in_cap)[0])


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("count", COUNTS)
def test_slot_map_is_a_bijection(emul, count, grid):
    s = emul.slots(grid, count)
    G = grid * emul.LANES
    gens = (count + G - 1) // G
    assert s.shape[0] == gens
    taken = s[s < count]
    assert bool((s <= count).all())
    assert np.array_equal(np.sort(taken), np.arange(count, dtype=np.uint64)), "a slot missed or taken twice"
    for k in range(gens):
        full = (k + 1) * G <= count
        gen = s[k].astype(np.int64)
        lo, hi = k * G, min((k + 1) * G, count)
        assert bool(((gen == count) | ((gen >= lo) & (gen < hi))).all()), "a slot outside its generation"
        if not full:
            continue
        # a wave's 64 lanes take 64 consecutive slots
        assert bool((gen.max(axis=1) - gen.min(axis=1) == emul.LANES - 1).all())
        assert bool((gen.min(axis=1) % emul.LANES == lo % emul.LANES).all())
        # the direction over lanes and waves alternates: a position's ranks in two neighbouring full
        # generations mirror each other (rank r, then G - 1 - r)
        if k + 1 < gens and (k + 2) * G <= count:
            nxt = s[k + 1].astype(np.int64)
            assert bool(((gen - lo) + (nxt - lo - G) == G - 1).all())
    # generations after a lane's first missing slot have none for it either (the walk may stop there)
    none = (s == count)
    assert bool((none[:-1] <= none[1:]).all()) if gens > 1 else True


def test_partial_last_generation_holds_the_shortest_pages(emul):
    rng = np.random.default_rng(3)
    in_cap, grid, count = 16464, 2, 300
    lengths = rng.integers(1, in_cap, count).astype(np.uint32)
    order = emul.order(lengths, in_cap, 0)
    s = emul.slots(grid, count)
    last = s[-1][s[-1] < count].astype(np.int64)
    assert last.size == count - 2 * grid * emul.LANES
    bins = emul.bins(lengths, in_cap)
    assert bins[order[last]].max() <= bins[order[: 2 * grid * emul.LANES]].min()


def test_key_edge_cases(emul):
    in_cap = 16464
    assert emul.bin(0, in_cap) == 0 and emul.bin(1, in_cap) == 0
    top = emul.bin(in_cap, in_cap)
    assert 255 <= top < emul.BINS, "a few hundred bins over [0, in_cap]"
    assert emul.bin(in_cap + 1, in_cap) == top and emul.bin(0xFFFFFFFF, in_cap) == top
    for cap in (1, 2, 511, 512, 513, 4160, 65535, 65536, 4 << 20):
        assert emul.bin(cap, cap) < emul.BINS and emul.bin(cap, cap) >= min(cap, 255)
        assert emul.bin(cap + 1, cap) == emul.bin(cap, cap)
    n = 700
    # all equal: nothing to order
    for window in (0, 64, 256):
        assert np.array_equal(emul.order(np.full(n, 1234, np.uint32), in_cap, window), np.arange(n, dtype=np.uint32))
    # all different, one length per bin at most: the order is the descending sort itself
    shift = 6
    assert (in_cap >> shift) < emul.BINS <= (in_cap >> (shift - 1))
    rng = np.random.default_rng(11)
    lengths = (rng.permutation(in_cap >> shift)[:200].astype(np.uint32) << shift) + 5
    assert np.array_equal(emul.order(lengths, in_cap, 0), np.argsort(-lengths.astype(np.int64), kind="stable").astype(np.uint32))
    # the edge lengths side by side: the over-long pages (the decoder rejects them) sort with the longest
    lengths = np.array([0, 1, in_cap, in_cap + 1, 5000, 0, in_cap + 1, 1], np.uint32)
    assert list(emul.order(lengths, in_cap, 0)) == [2, 3, 6, 4, 0, 1, 5, 7]


# ---------------------------------------------------------------- the balance model
def wave_iterations(chunks, pages_of):
    """pages_of[k, w, l] = the page lane l of wave w decodes in generation k (-1: none).  A lane's
    loop iterations are the chunks of its pages; a wave runs until its slowest lane is done."""
    c = np.where(pages_of >= 0, chunks[np.maximum(pages_of, 0)], 0)
    lane_sums = c.sum(axis=0)
    return lane_sums.max(axis=1), float(lane_sums.mean())


def test_balance_model_on_bench_pages(emul, oracle_mod, capsys):
    """4,096 bench pages (16 KiB, dist 0, seed 20170303) compressed by the oracle, their chunks from the
    decoder's emulator at R = 192, on a grid of 8 waves: 8 generations.  With the ordered walk the
    slowest wave exceeds the mean lane sum by at most half of what it does with the stride walk,
    under the whole-batch order and under windows of 4,096 pages."""
    if _stale(LC_LIB, [LC_SRC] + LC_CORE):
        os.makedirs(os.path.dirname(LC_LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-DLC_FAR16=1", "-o", LC_LIB, LC_SRC])
    lc = ctypes.CDLL(LC_LIB)
    lc.lc_emul_chunks.restype = ctypes.c_long
    lc.lc_emul_chunks.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    n, plen, grid = 4096, 16384, 8
    pages = oracle_mod.pagegen(n, plen, seed=20170303, first=0, dist=0)
    streams = [oracle_mod.lz4_compress(pages[i].tobytes()) for i in range(n)]
    lengths = np.array([len(s) for s in streams], np.uint32)
    chunks = np.array([lc.lc_emul_chunks(s, len(s), plen, 192) for s in streams], np.int64)
    assert bool((chunks > 0).all())
    in_cap = plen + plen // 255 + 16
    G = grid * emul.LANES
    gens = n // G
    stride = (np.arange(gens)[:, None, None] * G + np.arange(grid)[None, :, None] * emul.LANES +
              np.arange(emul.LANES)[None, None, :])
    wmax_s, mean = wave_iterations(chunks, stride)
    slots = emul.slots(grid, n).astype(np.int64)
    assert slots.shape == (gens, grid, emul.LANES) and bool((slots < n).all())
    over_s = float(wmax_s.max()) - mean
    with capsys.disabled():
        print(f"\nbalance model: mean lane sum {mean:.1f}; stride walk: slowest wave {wmax_s.max()} "
              f"(+{100 * over_s / mean:.1f} %), mean wave {wmax_s.mean():.1f}")
    for window in (0, 4096):
        order = emul.order(lengths, in_cap, window).astype(np.int64)
        wmax_o, mean_o = wave_iterations(chunks, order[slots])
        assert mean_o == mean
        over_o = float(wmax_o.max()) - mean
        with capsys.disabled():
            print(f"balance model: window {window}: slowest wave {wmax_o.max()} (+{100 * over_o / mean:.1f} %), "
                  f"mean wave {wmax_o.mean():.1f}")
        assert over_o <= 0.5 * over_s, (window, wmax_o.max(), wmax_s.max(), mean)
