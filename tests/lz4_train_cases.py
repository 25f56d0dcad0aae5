"""Shared inputs of the LZ4 dictionary-trainer tests (test_lz4_train_emul.py on the CPU,
test_gpu_lz4_train.py on the GPU) and the specification they are held to: `train_spec`, a plain
numpy restatement of the algorithm of DESIGN.md 3.3d.  The host emulator
(tools/lz4_train_emul.cpp, the kernels' own per-page code) must give train_spec's bytes, and the
GPU the emulator's.

The ratio conditions are judged by the reference encoder (LZ4 1.7.5's LZ4_compress_default and
LZ4_loadDict + LZ4_compress_fast_continue from oracle/_ref when it is built); its sizes for
exactly these inputs are also in tests/golden/lz4_train.npz, recorded by
tools/gen_lz4_train_golden.py, so the conditions never depend on that library being present."""
import os

import numpy as np

import lz4_dict_cases as DC
from conftest import GOLDEN

S, KEY, F, STEP = 128, 8, 20, 8
MULT = np.uint64(0x9E3779B185EBCA87)
DICT_MIN, DICT_MAX = 128, 32768
TRAIN_MAX_BYTES = 64 << 20
GOLDEN_FILE = os.path.join(GOLDEN, "lz4_train.npz")


# ---------------------------------------------------------------- the specification
def keys_of(page: bytes) -> np.ndarray:
    """h(q) for q = 0 .. len - 8 (empty below 8 bytes)."""
    a = np.frombuffer(page, np.uint8)
    if len(a) < KEY:
        return np.zeros(0, np.uint64)
    v = np.lib.stride_tricks.sliding_window_view(a, KEY).astype(np.uint64)
    k = np.zeros(len(v), np.uint64)
    for i in range(KEY):
        k |= v[:, i] << np.uint64(8 * i)
    return (k * MULT) >> np.uint64(64 - F)


def train_spec(pages, D: int) -> bytes:
    """The dictionary of `pages` (a list of bytes) at requested length D; b"" when nothing is picked."""
    hs = [keys_of(p) for p in pages]
    df = np.zeros(1 << F, np.int64)
    for h in hs:
        df[np.unique(h)] += 1                       # document frequency: once per page
    w = np.where(df >= 2, df, 0)
    base = np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.int64)
    H = np.concatenate(hs).astype(np.int64) if hs else np.zeros(0, np.int64)
    run = np.zeros(len(H), bool)                    # g(q) = 0 where q > 0 and h(q) == h(q-1)
    for i, h in enumerate(hs):
        if len(h) > 1:
            run[base[i] + 1:base[i + 1]] = h[1:] == h[:-1]
    cand, where = [], []                            # candidates in (page, s) order: argmax's first hit is the tie rule
    for i, p in enumerate(pages):
        for s in range(0, len(p) - S + 1, STEP):
            cand.append(base[i] + s)
            where.append((i, s))
    if not cand:
        return b""
    cand = np.asarray(cand, np.int64)
    nk = S - KEY + 1
    picks = []
    for _ in range(D // S):
        g = np.where(run, 0, w[H])
        c = np.concatenate([[0], np.cumsum(g)])
        score = c[cand + nk] - c[cand]
        b = int(np.argmax(score))
        if score[b] == 0:
            break
        i, s = where[b]
        picks.append(pages[i][s:s + S])
        w[H[cand[b]:cand[b] + nk]] = 0
    return b"".join(reversed(picks))                # the first pick ends the dictionary


# ---------------------------------------------------------------- inputs
_cache = {}


def gen_pages(O, n: int, L: int, dist: int, first: int, seed: int = 4242):
    key = (n, L, dist, first, seed)
    if key not in _cache:
        _cache[key] = [r.tobytes() for r in O.pagegen(n, L, seed=seed, first=first, dist=dist)]
    return _cache[key]


def small_cases(O):
    """(name, pages, D): the edge cases, a few KiB each."""
    rng = np.random.default_rng(20240601)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    d0 = gen_pages(O, 16, 4096, 0, 500)
    out = []
    a = rnd(128)
    out.append(("two-128-equal", [a, a], 128))
    out.append(("two-128-equal-D4096", [a, a], 4096))
    out.append(("two-128-differ", [a, rnd(128)], 128))
    b = d0[0]
    out.append(("tiny-mixed", [b[:7], b[:8], b[:127], b[:129], b[:8], b[1:130], d0[1][:512], b[:7], d0[1][:512]], 512))
    out.append(("three-identical", [d0[2][:1024]] * 3, 1024))
    out.append(("all-zero", [bytes(4096)] * 4, 512))
    out.append(("zero-and-data", [bytes(2048), d0[3][:2048], bytes(2048), d0[3][:2048]], 1024))
    s200 = rnd(200)
    shared = []
    for k, off in enumerate((0, 1, 3, 7, 250, 1001, 1848)):
        p = bytearray(rnd(2048))
        p[off:off + 200] = s200
        shared.append(bytes(p))
    out.append(("shared-200", shared, 512))
    out.append(("random-16", [rnd(4096) for _ in range(16)], 4096))
    lens = (130, 4096, 333, 128, 2049, 4095, 1000, 135, 136, 137, 3001, 8, 127, 2222, 4090, 512)
    out.append(("ragged", [p[:n] for p, n in zip(d0, lens)], 2048))
    out.append(("dist0-4k-floor", d0, 1000 + 128))
    return out


BIG_DS = (128, 4096, 32768)


def big_pages(O, dist: int):
    """64 x 16 KiB of one distribution."""
    return gen_pages(O, 64, 16384, dist, 300 + 100 * dist)


FLOOR_D = 4095 + 128


def pack(pages, misalign: int = 0, gap: int = 0):
    """(buffer, offsets, lengths): the pages one after another from byte `misalign` on, `gap` bytes between them."""
    offs, pos = [], misalign
    for p in pages:
        offs.append(pos)
        pos += len(p) + gap
    buf = np.zeros(pos + 1, np.uint8)
    for o, p in zip(offs, pages):
        buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return buf, np.asarray(offs, np.uint64), np.asarray([len(p) for p in pages], np.uint32)


# ---------------------------------------------------------------- ratio conditions
RATIO_LS = (8192, 16384)
RATIO_DISTS = range(6)
RATIO_D = 4096


def ratio_training_pages(O, L: int, dist: int):
    return gen_pages(O, 64, L, dist, 100000 + 1000 * dist)


def ratio_eval(O, L: int, dist: int):
    """(heuristic dictionary cut to 4,096 bytes, the 48 evaluation pages)."""
    dic, pages = DC.ratio_inputs(O, L, dist, RATIO_D)
    return dic[:RATIO_D], [r.tobytes() for r in pages]


def sample_sets():
    """(set, dictionary length) of the reference's sample_data pages, as lz4_dict_cases.sample_cases."""
    return DC.sample_cases()


def sample_split(O, name: str, dl: int):
    """(first-page prefix, training pages = the set's first 5, evaluation pages = its last 5)."""
    DC.sample_inputs(O, name, dl)                   # fills the cache from tests/golden/lz4_sample.npz
    names = sorted(n for n in DC._cache["sample"] if n.startswith(name + "/"))
    pages = [DC._cache["sample"][n] for n in names]
    assert len(pages) == 10, (name, len(pages))
    return pages[0][:dl], pages[:5], pages[5:]


def judge(O, ref, dictionary, pages) -> int:
    """Total bytes of the reference encoder over `pages`, with `dictionary` (None or b"": without one)."""
    if not dictionary:
        return sum(len(O.ref_lz4_compress(p)) for p in pages)
    return sum(len(ref.compress(dictionary, p)) for p in pages)


def ratio_keys():
    return [(L, d) for L in RATIO_LS for d in RATIO_DISTS]


class Golden:
    """tests/golden/lz4_train.npz: the reference encoder's totals when the file was recorded, and the
    CRC of the trained dictionary they belong to."""

    def __init__(self):
        g = np.load(GOLDEN_FILE, allow_pickle=False)
        self.ratio = {k: tuple(int(x) for x in row) for k, row in zip(ratio_keys(), g["ratio"])}      # plain, heuristic, trained, crc
        self.sample = {k: tuple(int(x) for x in row) for k, row in zip(sample_sets(), g["sample"])}  # prefix, trained, crc
