"""Shared cases of the zstd shared-dictionary tests (test_zstd_dict_abi.py without a GPU,
test_gpu_zstd_dict.py on one): dictionaries, pages, and the two sources of expected values -- the
reference library (zstd 1.1.2's ZSTD_compress_usingDict / ZSTD_decompress_usingDict from
oracle/_ref, when it is built) and tests/golden/zstd_dict.npz, which tools/gen_zstd_dict_golden.py
recorded from that library, so that verdict and ratio checks never depend on it being present."""
import ctypes
import os
import zlib

import numpy as np

from conftest import GOLDEN, load_golden, unpack

ZSTD = 3
DICT_MAX = 32768
WINDOW = 65536
MAGIC = bytes([0x37, 0xA4, 0x30, 0xEC])   # ZSTD_DICT_MAGIC: a structured dictionary to the reference
DS = (1, 7, 8, 9, 63, 64, 65, 4096, 32768)
LS = (0, 1, 63, 64, 65, 4096, 16384, 32768)
KINDS = ("dist0", "tail", "zeros", "random")
# the subset whose reference-made frames are in the golden file (GOLDEN_DS x GOLDEN_LS x KINDS)
GOLDEN_DS = (1, 64, 4096, 32768)
GOLDEN_LS = (1, 65, 4096, 16384)
GOLDEN_FILE = os.path.join(GOLDEN, "zstd_dict.npz")

_u8p = ctypes.POINTER(ctypes.c_uint8)


def _p(a: np.ndarray):
    return a.ctypes.data_as(_u8p)


def zstd_bound(n: int) -> int:
    return n + (n >> 7) + 512 + 12   # ZSTD_compressBound (zstd 1.1.2) = tyche_compress_bound


def page_lengths(D: int):
    """LS that fit the window, and the longest page the dictionary reaches (65536 - D, at most 65535)."""
    top = min(WINDOW - D, 65535)
    return sorted({l for l in LS if l + D <= WINDOW} | {top})


PAIRS = [(d, l) for d in DS for l in page_lengths(d)]


class Ref:
    """The reference's two dictionary functions through ctypes (oracle.REF_SO).  ctypes releases the
    GIL around a call, so one Ref per thread runs them in parallel."""

    def __init__(self, O):
        self.lib = L = ctypes.CDLL(O.REF_SO)
        L.ZSTD_createCCtx.restype = ctypes.c_void_p
        L.ZSTD_createDCtx.restype = ctypes.c_void_p
        L.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
        L.ZSTD_freeDCtx.argtypes = [ctypes.c_void_p]
        L.ZSTD_compress_usingDict.argtypes = [ctypes.c_void_p, _u8p, ctypes.c_size_t, _u8p, ctypes.c_size_t, _u8p,
                                              ctypes.c_size_t, ctypes.c_int]
        L.ZSTD_compress_usingDict.restype = ctypes.c_size_t
        L.ZSTD_decompress_usingDict.argtypes = [ctypes.c_void_p, _u8p, ctypes.c_size_t, _u8p, ctypes.c_size_t, _u8p,
                                                ctypes.c_size_t]
        L.ZSTD_decompress_usingDict.restype = ctypes.c_size_t
        L.ZSTD_compress.argtypes = [_u8p, ctypes.c_size_t, _u8p, ctypes.c_size_t, ctypes.c_int]
        L.ZSTD_compress.restype = ctypes.c_size_t
        L.ZSTD_decompress.argtypes = [_u8p, ctypes.c_size_t, _u8p, ctypes.c_size_t]
        L.ZSTD_decompress.restype = ctypes.c_size_t
        L.ZSTD_isError.argtypes = [ctypes.c_size_t]
        L.ZSTD_isError.restype = ctypes.c_uint
        self.cctx = L.ZSTD_createCCtx()
        self.dctx = L.ZSTD_createDCtx()

    def __del__(self):
        try:
            self.lib.ZSTD_freeCCtx(self.cctx)
            self.lib.ZSTD_freeDCtx(self.dctx)
        except Exception:
            pass

    def compress_rv(self, dictionary: bytes, page: bytes, level: int = 1):
        """(ZSTD_compress_usingDict's value or -1 where ZSTD_isError, the frame)."""
        d = np.frombuffer(dictionary, np.uint8).copy() if dictionary else np.zeros(1, np.uint8)
        s = np.frombuffer(page, np.uint8).copy() if page else np.zeros(1, np.uint8)
        cap = zstd_bound(len(page))
        out = np.zeros(cap + 64, np.uint8)
        r = self.lib.ZSTD_compress_usingDict(self.cctx, _p(out), cap, _p(s), len(page), _p(d), len(dictionary), level)
        if self.lib.ZSTD_isError(r):
            return -1, b""
        return int(r), out[:r].tobytes()

    def compress(self, dictionary: bytes, page: bytes, level: int = 1) -> bytes:
        r, frame = self.compress_rv(dictionary, page, level)
        assert r > 0
        return frame

    def compress_plain(self, page: bytes, level: int = 1) -> bytes:
        s = np.frombuffer(page, np.uint8).copy() if page else np.zeros(1, np.uint8)
        cap = zstd_bound(len(page))
        out = np.zeros(cap + 64, np.uint8)
        r = self.lib.ZSTD_compress(_p(out), cap, _p(s), len(page), level)
        assert not self.lib.ZSTD_isError(r)
        return out[:r].tobytes()

    def decompress(self, dictionary: bytes, frame: bytes, cap: int):
        """(ZSTD_decompress_usingDict's value, or -1 where ZSTD_isError; the decoded bytes), the
        dictionary in a buffer of its own.  An empty dictionary is plain ZSTD_decompress."""
        d = np.frombuffer(dictionary, np.uint8).copy() if dictionary else np.zeros(1, np.uint8)
        s = np.zeros(len(frame) + 16, np.uint8)
        s[:len(frame)] = np.frombuffer(frame, np.uint8)
        out = np.zeros(max(cap, 1) + 64, np.uint8)
        r = self.lib.ZSTD_decompress_usingDict(self.dctx, _p(out), cap, _p(s), len(frame), _p(d), len(dictionary))
        if self.lib.ZSTD_isError(r):
            return -1, b""
        return int(r), out[:r].tobytes()

    def decompress_plain(self, frame: bytes, cap: int):
        s = np.zeros(len(frame) + 16, np.uint8)
        s[:len(frame)] = np.frombuffer(frame, np.uint8)
        out = np.zeros(max(cap, 1) + 64, np.uint8)
        r = self.lib.ZSTD_decompress(_p(out), cap, _p(s), len(frame))
        if self.lib.ZSTD_isError(r):
            return -1, b""
        return int(r), out[:r].tobytes()


def ref_or_none(O):
    return Ref(O) if O.have_ref() else None


# ---------------------------------------------------------------- dictionaries and pages
_cache = {}


def gen(O, dist: int, first: int, n: int) -> bytes:
    """n bytes of bench pages of `dist` (32 KiB pages from page number `first` on)."""
    key = (dist, first, n)
    if key not in _cache:
        reps = max((n + 32767) // 32768, 1)
        _cache[key] = O.pagegen(reps, 32768, first=first, dist=dist).tobytes()[:n]
    return _cache[key]


def dict_of(O, D: int) -> bytes:
    """The dictionary of the round-trip cases: a dist-0 page cut to D bytes."""
    return gen(O, 0, 9000, DICT_MAX)[:D]


def page_of(O, D: int, L: int, kind: str) -> bytes:
    if kind == "dist0":
        return gen(O, 0, 7 + D % 5, L)
    if kind == "tail":                                   # the dictionary's tail, repeated where L > D
        tile = dict_of(O, D)[-min(max(L, 1), D):]
        return (tile * (L // len(tile) + 1))[:L]
    if kind == "zeros":
        return bytes(L)
    assert kind == "random"
    return np.random.default_rng(1000003 * D + 31 * L).integers(0, 256, L, dtype=np.uint8).tobytes()


def all_cases(O, pairs=None, kinds=KINDS):
    """(D, L, kind, dictionary, page) for every pair and kind."""
    return [(D, L, k, dict_of(O, D), page_of(O, D, L, k)) for D, L in (PAIRS if pairs is None else pairs) for k in kinds]


def golden_pairs():
    return [(d, l) for d in GOLDEN_DS for l in GOLDEN_LS]


# ---------------------------------------------------------------- the dictionary is used
USED_D = 16384
USED_LS = (64, 4096, 16384)


def used_case(L: int):
    """D = 16384 random bytes and the page that equals its last L bytes."""
    dic = np.random.default_rng(20170303).integers(0, 256, USED_D, dtype=np.uint8).tobytes()
    return dic, dic[USED_D - L:]


# ---------------------------------------------------------------- boundary frames
BOUNDARY = [(D, L) for L in (65, 4096, 16384) for D in (64, 4096, 32768)]


def boundary_case(O, D: int, L: int):
    """A random dictionary and a page that begins with its first 64 bytes, then a compressible
    (dist-0) page: the reference's first match reaches dictionary byte 0 (offset == position + D),
    so its frame decodes with the whole dictionary and is an error with the dictionary minus its
    first byte (and from plain ZSTD_decompress).  tools/gen_zstd_dict_golden.py asserts that."""
    dic = np.random.default_rng(777 + D).integers(0, 256, D, dtype=np.uint8).tobytes()
    return dic, (dic[:64] + gen(O, 0, 40 + L % 7, L))[:L]


# ---------------------------------------------------------------- malformed frames with a dictionary
MALFORMED_D = 4096


def malformed_cases(O):
    """(dictionary, [(frame, capacity)]): every frame of tests/golden/zstd_malformed.npz, to be decoded
    with a 4 KiB dictionary; the verdict's sign is ZSTD_decompress_usingDict's with that dictionary."""
    g = load_golden("zstd_malformed.npz")
    return dict_of(O, MALFORMED_D), [(unpack(g["comp"], g["comp_off"], g["comp_len"], i), int(g["cap"][i]))
                                     for i in range(len(g["cap"]))]


# ---------------------------------------------------------------- ratio cells
RATIO_PAGES = 48
RATIO_DICT = 4096
RATIO_CELLS = [(n, d) for d in (0, 1, 2, 5) for n in (4096, 16384)]   # (page size, distribution)


def ratio_inputs(O, n: int, dist: int):
    """48 bench pages of n bytes and the 49th page's first 4 KiB as dictionary."""
    first = n + dist * 100
    pages = O.pagegen(RATIO_PAGES, n, seed=4242, first=first, dist=dist)
    dic = O.pagegen(1, n, seed=4242, first=first + RATIO_PAGES, dist=dist)[0].tobytes()[:RATIO_DICT]
    return dic, pages


def crc(b: bytes) -> int:
    return zlib.crc32(b) & 0xFFFFFFFF


# ---------------------------------------------------------------- golden file
class Golden:
    """tests/golden/zstd_dict.npz: what the reference library answered when the file was recorded."""

    def __init__(self):
        g = np.load(GOLDEN_FILE, allow_pickle=False)
        self.rt_frames = [unpack(g["rt_data"], g["rt_off"], g["rt_len"], i) for i in range(len(g["rt_len"]))]
        self.boundary_frames = [unpack(g["bd_data"], g["bd_off"], g["bd_len"], i) for i in range(len(g["bd_len"]))]
        self.malformed_rv = g["malformed_rv"]      # decoded size, or -1 where ZSTD_isError
        self.malformed_crc = g["malformed_crc"]
        self.used_ref = g["used_ref"]              # USED_LS order: reference bytes with the dictionary
        self.used_ref_plain = g["used_ref_plain"]  # and without
        self.ratio_ref = g["ratio_ref"]            # RATIO_CELLS order: reference level-1 bytes with the dictionary
        self.ratio_ref_plain = g["ratio_ref_plain"]

    def rt_cases(self, O):
        """(D, L, kind, dictionary, page, reference-made frame) of the golden subset."""
        cs = all_cases(O, golden_pairs())
        assert len(cs) == len(self.rt_frames)
        return [c + (s,) for c, s in zip(cs, self.rt_frames)]

    def boundary_cases(self, O):
        """(D, L, dictionary, page, reference-made frame)."""
        assert len(self.boundary_frames) == len(BOUNDARY)
        return [(D, L) + boundary_case(O, D, L) + (f,) for (D, L), f in zip(BOUNDARY, self.boundary_frames)]
