"""Shared cases of the LZ4 shared-dictionary tests (test_lz4_dict_emul.py on the CPU,
test_gpu_lz4_dict.py on the GPU): dictionaries, pages, hand-made and malformed streams, and the
two sources of expected values -- the reference library (LZ4 1.7.5's LZ4_loadDict +
LZ4_compress_fast_continue and LZ4_decompress_safe_usingDict from oracle/_ref, when it is built)
and tests/golden/lz4_dict.npz, which tools/gen_lz4_dict_golden.py recorded from that library, so
that verdict and ratio checks never depend on it being present."""
import ctypes
import os
import zlib

import numpy as np

from conftest import GOLDEN

DICT_MAX = 32768
WINDOW = 65536
DS = (1, 4, 63, 64, 65, 1000, 4096, 16384, 32768)
LS = (0, 1, 12, 13, 64, 65, 4095, 16384, 32768)
PAIRS = [(d, l) for d in DS for l in LS if d + l <= WINDOW]
KINDS = ("tail",) + tuple(f"seam{p}" for p in range(1, 8)) + ("first", "random") + tuple(f"dist{d}" for d in range(6))
# the subset whose reference-made streams are in the golden file (GOLDEN_DS x GOLDEN_LS x KINDS)
GOLDEN_DS = (1, 63, 65, 4096)
GOLDEN_LS = (13, 65, 4095)
GOLDEN_FILE = os.path.join(GOLDEN, "lz4_dict.npz")

_u8p = ctypes.POINTER(ctypes.c_uint8)


def _p(a: np.ndarray):
    return a.ctypes.data_as(_u8p)


def lz4_bound(n: int) -> int:
    return n + n // 255 + 16


class Ref:
    """The reference's dictionary API through ctypes (oracle.REF_SO)."""

    def __init__(self, O):
        self.lib = ctypes.CDLL(O.REF_SO)
        L = self.lib
        L.LZ4_createStream.restype = ctypes.c_void_p
        L.LZ4_freeStream.argtypes = [ctypes.c_void_p]
        L.LZ4_loadDict.argtypes = [ctypes.c_void_p, _u8p, ctypes.c_int]
        L.LZ4_loadDict.restype = ctypes.c_int
        L.LZ4_compress_fast_continue.argtypes = [ctypes.c_void_p, _u8p, _u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.LZ4_compress_fast_continue.restype = ctypes.c_int
        L.LZ4_decompress_safe_usingDict.argtypes = [_u8p, _u8p, ctypes.c_int, ctypes.c_int, _u8p, ctypes.c_int]
        L.LZ4_decompress_safe_usingDict.restype = ctypes.c_int

    def compress(self, dictionary: bytes, page: bytes) -> bytes:
        d = np.frombuffer(dictionary, np.uint8).copy()
        s = np.frombuffer(page, np.uint8).copy() if page else np.zeros(1, np.uint8)
        cap = lz4_bound(len(page))
        out = np.zeros(cap + 64, np.uint8)
        st = self.lib.LZ4_createStream()
        try:
            self.lib.LZ4_loadDict(st, _p(d), len(dictionary))
            r = self.lib.LZ4_compress_fast_continue(st, _p(s), _p(out), len(page), cap, 1)
        finally:
            self.lib.LZ4_freeStream(st)
        assert r > 0
        return out[:r].tobytes()

    def decompress(self, dictionary: bytes, stream: bytes, cap: int):
        """(LZ4_decompress_safe_usingDict's value, the decoded bytes), the dictionary in a buffer of its own."""
        d = np.frombuffer(dictionary, np.uint8).copy()
        s = np.zeros(len(stream) + 16, np.uint8)
        s[:len(stream)] = np.frombuffer(stream, np.uint8)
        out = np.zeros(max(cap, 1) + 64, np.uint8)
        r = self.lib.LZ4_decompress_safe_usingDict(_p(s), _p(out), len(stream), cap, _p(d), len(dictionary))
        return r, (out[:r].tobytes() if r > 0 else b"")


def ref_or_none(O):
    return Ref(O) if O.have_ref() else None


# ---------------------------------------------------------------- dictionaries and pages
_cache = {}


def _gen(O, dist: int, first: int, n: int = 32768) -> bytes:
    key = (dist, first, n)
    if key not in _cache:
        _cache[key] = O.pagegen(1, n, first=first, dist=dist)[0].tobytes()
    return _cache[key]


def dict_of(O, D: int, kind: str) -> bytes:
    """The dictionary of a case: for the pagegen kinds another page of the same distribution cut
    to D bytes, else a dist-0 page cut to D."""
    if kind.startswith("dist"):
        return _gen(O, int(kind[4:]), 9001)[:D]
    return _gen(O, 0, 9000)[:D]


def dict_key(D: int, kind: str):
    """Cases with equal keys share a dictionary (one handle, one launch)."""
    return (D, kind if kind.startswith("dist") else "generic")


def page_of(O, D: int, L: int, kind: str) -> bytes:
    dic = dict_of(O, D, kind)
    rng = np.random.default_rng(1000003 * D + 31 * L + sum(map(ord, kind)))
    rnd = rng.integers(0, 256, L + 64, dtype=np.uint8).tobytes()
    if kind == "tail":                                   # one long match: the dictionary's tail
        tile = dic[-min(max(L, 1), D):]
        return (tile * (L // len(tile) + 1))[:L]
    if kind.startswith("seam"):                          # starts in the dictionary's last p bytes, runs over the seam
        p = min(int(kind[4:]), D)
        run = min(L, 200 + 13 * p)
        return (bytes(dic[D - p + (i % p)] for i in range(run)) + rnd)[:L]
    if kind == "first":                                  # its only source is the dictionary's first bytes
        return (rnd[:9] + dic[:min(D, 40)] + rnd[9:])[:L]
    if kind == "random":
        return rnd[:L]
    return _gen(O, int(kind[4:]), 7 + D % 5)[:L]


def all_cases(O, pairs=PAIRS, kinds=KINDS):
    """(D, L, kind, dictionary, page) for every pair and kind."""
    return [(D, L, k, dict_of(O, D, k), page_of(O, D, L, k)) for D, L in pairs for k in kinds]


def golden_pairs():
    return [(d, l) for d in GOLDEN_DS for l in GOLDEN_LS]


# ---------------------------------------------------------------- hand-made streams
def _seq(lit: bytes, offset: int, ml: int) -> bytes:
    """One LZ4 sequence: literals, then a match of ml >= 4 bytes at `offset`."""
    out = bytearray()
    ll, mc = len(lit), ml - 4
    out.append((min(ll, 15) << 4) | min(mc, 15))
    if ll >= 15:
        r = ll - 15
        out += b"\xff" * (r // 255) + bytes([r % 255])
    out += lit
    out += bytes([offset & 255, offset >> 8])
    if mc >= 15:
        r = mc - 15
        out += b"\xff" * (r // 255) + bytes([r % 255])
    return bytes(out)


def _last(lit: bytes) -> bytes:
    ll = len(lit)
    out = bytearray([min(ll, 15) << 4])
    if ll >= 15:
        r = ll - 15
        out += b"\xff" * (r // 255) + bytes([r % 255])
    return bytes(out + lit)


def crafted(O):
    """(name, D, dictionary, stream, capacity): the verdict cases made by hand."""
    tail = bytes(range(100, 112))
    out = []
    for D in (1, 64, 1000, 32768):
        dic = dict_of(O, D, "generic")
        for lead in (0, 3):
            lit = bytes(range(1, 1 + lead))
            size = lead + 4 + 12
            ok = _seq(lit, lead + D, 4) + _last(tail)
            out.append((f"reach-D{D}-lead{lead}", D, dic, ok, size))              # offset == position + D: legal
            out.append((f"reach+1-D{D}-lead{lead}", D, dic, _seq(lit, lead + D + 1, 4) + _last(tail), size))
            for cap in (size - 1, size + 1, 0):                                       # capacity off by one either way
                out.append((f"reach-D{D}-lead{lead}-cap{cap}", D, dic, ok, cap))
        if D < 32768:
            out.append((f"reach-long-D{D}", D, dic, _seq(b"", D, 300) + _last(tail), 312))   # across the seam, 300 bytes
        # a dictionary match that ends inside the last 5 bytes of the capacity
        out.append((f"late-match-D{D}", D, dic, _seq(b"", min(D, 9), 8) + _last(tail[:4]), 12))
        out.append((f"late-match-ok-D{D}", D, dic, _seq(b"", min(D, 9), 8) + _last(tail[:5]), 13))
        # a literal run past the capacity
        out.append((f"lit-overrun-D{D}", D, dic, _last(bytes(20)), 16))
        out.append((f"lit-mid-overrun-D{D}", D, dic, _seq(bytes(30), min(D, 5), 6) + _last(tail), 20))
        for p in range(1, 8):                                                        # overlapping copies over the seam
            if p <= D:
                out.append((f"seam-p{p}-D{D}", D, dic, _seq(b"", p, 40) + _seq(b"ab", p + 1, 5) + _last(tail), 59))
        out.append((f"empty-D{D}", D, dic, b"\x00", 0))
        out.append((f"empty-cap1-D{D}", D, dic, b"\x00", 1))
    return out


# ---------------------------------------------------------------- malformed streams
BASE_D = 1000
BASE_L = 4096
BASE_KINDS = ("dist0", "dist1", "dist2", "dist3", "dist4", "dist5", "tail", "seam3", "first", "random")


def base_cases(O):
    """The 10 (dictionary, page) pairs whose reference-made streams are cut and patched."""
    return [(dict_of(O, BASE_D, k), page_of(O, BASE_D, BASE_L, k)) for k in BASE_KINDS]


def cuts(stream: bytes, i: int):
    """40 seeded lengths to cut stream i at (fewer for a stream shorter than that).  Never 0: the
    reference reads the byte after an empty input, so its value there is not defined."""
    rng = np.random.default_rng(77 + i)
    n = len(stream)
    c = {1, 2, n - 1, n - 5, n - 12} | {int(x) for x in rng.integers(1, n, 60)}
    return sorted(x for x in c if 1 <= x < n)[:40]


def patches(stream: bytes, i: int):
    """40 seeded one-byte patches of stream i: (position, new byte)."""
    rng = np.random.default_rng(991 + i)
    pos = rng.integers(0, len(stream), 40)
    val = rng.integers(0, 256, 40)
    return [(int(p), int(v)) for p, v in zip(pos, val)]


def patched(stream: bytes, p: int, v: int) -> bytes:
    b = bytearray(stream)
    b[p] = v if b[p] != v else v ^ 0x55
    return bytes(b)


def malformed(streams):
    """(name, base index, stream, capacity) for every cut and patch of the 10 base streams."""
    out = []
    for i, s in enumerate(streams):
        for c in cuts(s, i):
            out.append((f"cut{i}@{c}", i, s[:c], BASE_L))
        for p, v in patches(s, i):
            out.append((f"patch{i}@{p}={v}", i, patched(s, p, v), BASE_L))
    return out


def walk(stream: bytes):
    """(position, offset, match length) of every match of a stream, as far as it parses."""
    ip, op, n, out = 0, 0, len(stream), []
    while ip < n:
        t = stream[ip]
        ip += 1
        lit = t >> 4
        if lit == 15:
            while ip < n:
                b = stream[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip += lit
        op += lit
        if ip + 2 > n:
            break
        off = stream[ip] | (stream[ip + 1] << 8)
        ip += 2
        ml = t & 15
        if ml == 15:
            while ip < n:
                b = stream[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        out.append((op, off, ml + 4))
        op += ml + 4
    return out


def max_reach(stream: bytes) -> int:
    """How far before the page's first byte the stream's offsets reach (0: not at all)."""
    return max([off - pos for pos, off, _ in walk(stream)] + [0])


def has_zero_offset(stream: bytes) -> bool:
    """Offset 0 copies bytes the reference leaves undefined: only the size is compared then."""
    return any(off == 0 for _, off, _ in walk(stream))


def crc(b: bytes) -> int:
    return zlib.crc32(b) & 0xFFFFFFFF


# ---------------------------------------------------------------- golden file
class Golden:
    """tests/golden/lz4_dict.npz: what the reference library answered when the file was recorded."""

    def __init__(self):
        g = np.load(GOLDEN_FILE, allow_pickle=False)
        self.g = g
        offs, lens = g["base_off"], g["base_len"]
        self.base_streams = [g["base_data"][o:o + n].tobytes() for o, n in zip(offs, lens)]
        self.crafted_rv = g["crafted_rv"]
        self.crafted_crc = g["crafted_crc"]
        self.malformed_rv = g["malformed_rv"]
        self.malformed_crc = g["malformed_crc"]
        offs, lens = g["rt_off"], g["rt_len"]
        self.rt_streams = [g["rt_data"][o:o + n].tobytes() for o, n in zip(offs, lens)]
        self.ratio_ref = g["ratio_ref"]          # reference bytes of the ratio cases, ratio_cases() order
        self.sample_ref = g["sample_ref"]        # sample_cases() order: reference bytes with the dictionary
        self.sample_ref_plain = g["sample_ref_plain"]   # and LZ4_compress_default's without one

    def rt_cases(self, O):
        """(D, L, kind, dictionary, page, reference-made stream) of the golden subset."""
        cs = all_cases(O, golden_pairs())
        assert len(cs) == len(self.rt_streams)
        return [c + (s,) for c, s in zip(cs, self.rt_streams)]


# ---------------------------------------------------------------- ratio cases
RATIO_SIZES = (8192, 16384, 32768)
RATIO_PAGES = 48


def ratio_cases():
    """(page size, distribution, dictionary length): the inputs of test_encode_roundtrip_oracle
    (48 pages of 8 / 16 / 32 KiB, dist 0-5) with one more page of the distribution as dictionary,
    cut to 4 KiB and cut to the page size."""
    return [(n, d, dl) for n in RATIO_SIZES for d in range(6) for dl in (4096, n)]


def ratio_inputs(O, n: int, dist: int, dl: int):
    first = n + dist * 100                       # test_gpu_lz4.py test_encode_roundtrip_oracle's pages
    pages = O.pagegen(RATIO_PAGES, n, seed=4242, first=first, dist=dist)
    dic = O.pagegen(1, n, seed=4242, first=first + RATIO_PAGES, dist=dist)[0].tobytes()[:dl]
    return dic, pages


# ---------------------------------------------------------------- the reference's sample pages
SAMPLE_SETS = [f"{size}/names/{kind}" for size in ("8k", "16k", "32k") for kind in ("indexes", "tables")]


def sample_cases():
    """(set, dictionary length): every set of the reference's sample_data pages with the first 4 KiB
    of its first page as dictionary, and the 32 KiB index pages with 16 KiB of it as well."""
    return [(s, 4096) for s in SAMPLE_SETS] + [("32k/names/indexes", 16384)]


def sample_inputs(O, name: str, dl: int):
    """(dictionary, the set's remaining pages): the pages come out of tests/golden/lz4_sample.npz,
    the reference's own LZ4 encodings of the 60 sample pages, so no reference tree is needed."""
    if "sample" not in _cache:
        g = np.load(os.path.join(GOLDEN, "lz4_sample.npz"), allow_pickle=False)
        pages = {}
        for i, nm in enumerate(g["names"]):
            o, n, size = int(g["comp_off"][i]), int(g["comp_len"][i]), int(g["size"][i])
            r, dec = O.lz4_decompress(g["comp"][o:o + n].tobytes(), size)
            assert r == size
            pages[str(nm)] = dec
        _cache["sample"] = pages
    names = sorted(n for n in _cache["sample"] if n.startswith(name + "/"))
    pages = [_cache["sample"][n] for n in names]
    return pages[0][:dl], pages[1:]
