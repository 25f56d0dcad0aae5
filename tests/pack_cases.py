"""The packed store's rule restated in numpy, and the case corpus of its tests.

pack_spec / apply_spec are the specification of tyche_pack_batch (include/tyche_codec.h): what the
host emulator (tools/pack_emul.cpp, test_pack_emul.py), tyche_pack_plan and the kernels
(test_gpu_pack.py) are held to.  A Case is one append: the compress results, a source buffer laid
out like a compress batch's slots (every stream at a chosen misalignment, scratch bytes behind it),
and the state it appends to.  The tile size T, the pages per scan workgroup S and the scan's fan-in
F come from the code (the emulator exports pack_core.h's constants)."""
from dataclasses import dataclass

import numpy as np

INT32_MIN = -(2 ** 31)
FILL = 0xA5
ALIGNS = (1, 2, 16, 128, 4096)
STARTS = (0, 1, 13)


def round_up(x: int, align: int) -> int:
    return (x + align - 1) // align * align


def lens_of(results: np.ndarray, max_length: int) -> np.ndarray:
    r = results.astype(np.int64)
    ok = (r > 0) & ((max_length == 0) | (r <= max_length))
    return np.where(ok, r, 0).astype(np.uint32)


def pack_spec(results: np.ndarray, max_length: int, align: int, state, capacity: int):
    """-> (offsets uint64, lengths uint32, (state0, state1) after, stored)."""
    s0, s1 = int(state[0]), int(state[1])
    n = len(results)
    if n == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32), (s0, s1), True
    lens = lens_of(results, max_length)
    rooms = (lens.astype(np.uint64) + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
    base = round_up(s1, align)
    offs = np.uint64(base) + np.concatenate([np.zeros(1, np.uint64), np.cumsum(rooms, dtype=np.uint64)[:-1]])
    end = int(offs[-1]) + int(lens[-1])
    stored = s0 == s1 and end <= capacity
    return offs, lens, ((end, end) if stored else (s0, end)), stored


def apply_spec(arena: np.ndarray, src: np.ndarray, src_offsets: np.ndarray, offsets: np.ndarray, lengths: np.ndarray,
               arena_origin: int = 0) -> None:
    """Copies every stream to its place (a stored batch); arena[0] stands for arena offset arena_origin."""
    for i in np.flatnonzero(lengths):
        o, so, ln = int(offsets[i]) - arena_origin, int(src_offsets[i]), int(lengths[i])
        arena[o:o + ln] = src[so:so + ln]


@dataclass
class Case:
    name: str
    results: np.ndarray        # int32
    max_length: int
    align: int
    state: tuple               # (state0, state1) on entry
    capacity: int
    src: np.ndarray            # uint8
    src_offsets: np.ndarray    # uint64
    stream_mask: np.ndarray    # bool over src: the bytes of the streams that count (len_i > 0)
    skew: int = 0              # emulator only: the arena address's low 7 bits


def build_source(results: np.ndarray, max_length: int, rng, misalign=None):
    """Slots like a compress batch's: page i's stream starts `misalign[i]` (default i % 16) bytes
    past a 16-byte boundary and is followed by 8..40 scratch bytes; a result that does not count
    (negative, or above max_length) still has bytes in its slot.  -> (src, src_offsets, stream_mask)."""
    n = len(results)
    lens = lens_of(results, max_length)
    held = np.where(results.astype(np.int64) > 0, results.astype(np.int64), 0)
    mis = np.arange(n) % 16 if misalign is None else np.asarray(misalign)
    tails = rng.integers(8, 41, n)
    offs = np.zeros(n, np.uint64)
    pos = 16
    for i in range(n):
        pos = round_up(pos, 16) + int(mis[i])
        offs[i] = pos
        pos += int(held[i]) + int(tails[i])
    src = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    mask = np.zeros(len(src), bool)
    for i in np.flatnonzero(lens):
        mask[int(offs[i]):int(offs[i]) + int(lens[i])] = True
    return src, offs, mask


def make_case(name, results, align, state, rng, max_length=0, capacity=None, slack=64, misalign=None, skew=0) -> Case:
    results = np.asarray(results, np.int32)
    src, offs, mask = build_source(results, max_length, rng, misalign)
    if capacity is None:
        end = pack_spec(results, max_length, align, (state[1], state[1]), 1 << 62)[2][1]
        capacity = end + slack
    return Case(name, results, max_length, align, tuple(state), int(capacity), src, offs, mask, skew)


def edge_results(T: int):
    """Lengths 0, 1, 15, 16, 17, T-1, T, T+1, 3T+5, each at every source misalignment 0..15 (144
    pages: 9 and 16 are coprime), with results that mean "no stream" scattered between them: 0, -5,
    INT32_MIN and one above max_length = 3T+5.  -> (results, misalign, max_length)."""
    lengths = [0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5]
    specials = [0, -5, INT32_MIN, 3 * T + 6]
    results, mis = [], []
    for j in range(144):
        results.append(lengths[j % 9])
        mis.append(j % 16)
        if j % 10 == 9:
            results.append(specials[(j // 10) % 4])
            mis.append((j * 7) % 16)
    return np.asarray(results, np.int32), np.asarray(mis), 3 * T + 5


def edge_cases(T: int):
    out = []
    results, mis, max_length = edge_results(T)
    for align in ALIGNS:
        for start in STARTS:
            rng = np.random.default_rng(1000 + align * 16 + start)
            out.append(make_case(f"edges-a{align}-s{start}", results, align, (start, start), rng, max_length=max_length,
                                 misalign=mis, skew=(start * 37 + align) % 128))
    return out


def tiny_results(n: int, seed: int) -> np.ndarray:
    """n pages of 0 to 3 bytes."""
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.int32)


def scan_counts(S: int, F: int):
    """Counts around one scan workgroup's share, and one page past where the one-workgroup scan of
    the tile sums takes a second round (S * F pages fill the first)."""
    return [0, 1, S - 1, S, S + 1, 2 * S + 3, S * F + 1]


def scan_cases(S: int, F: int):
    out = []
    for k, n in enumerate(scan_counts(S, F)):
        rng = np.random.default_rng(2000 + k)
        out.append(make_case(f"scan-n{n}", tiny_results(n, 3000 + k), (1, 4)[k % 2], (5, 5), rng, skew=(11 * k) % 128))
    return out


def refusal_cases(T: int):
    """Capacity end - 1 (refused), == end (stored), an append into a refused state, and a capacity
    the start itself is beyond."""
    rng = np.random.default_rng(4000)
    results = np.asarray([7, T + 3, 0, 40, 300], np.int32)
    end = pack_spec(results, 0, 16, (9, 9), 1 << 62)[2][1]
    return [
        make_case("refused-by-one", results, 16, (9, 9), rng, capacity=end - 1),
        make_case("fits-exactly", results, 16, (9, 9), rng, capacity=end),
        make_case("sticky", np.asarray([1], np.int32), 16, (9, end), rng, capacity=end + 4096),
        make_case("all-empty", np.asarray([0, -1, INT32_MIN], np.int32), 128, (3, 3), rng, capacity=4096),
    ]


def corpus(T: int, S: int, F: int):
    return edge_cases(T) + scan_cases(S, F) + refusal_cases(T)


def expected(case: Case):
    """-> (offsets, lengths, state after, stored, arena of `capacity` bytes) by the specification."""
    offs, lens, state, stored = pack_spec(case.results, case.max_length, case.align, case.state, case.capacity)
    arena = np.full(case.capacity, FILL, np.uint8)
    if stored:
        apply_spec(arena, case.src, case.src_offsets, offs, lens)
    return offs, lens, state, stored, arena
