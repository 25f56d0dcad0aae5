"""Shared cases of the zlib shared-dictionary tests (test_zlib_dict_abi.py without a GPU,
test_gpu_zlib_dict.py on one): dictionaries, pages, a small deflate bit-writer for crafted
fixed-code streams, and the three sources of expected values -- the reference library (zlib 1.2.8's
deflateSetDictionary / inflateSetDictionary from oracle/_ref through a ctypes z_stream, when it is
built), Python's own zlib (compressobj / decompressobj with zdict=, always there), and
tests/golden/zlib_dict.npz, which tools/gen_zlib_dict_golden.py recorded from the reference, so that
verdict and ratio checks never depend on it being present."""
import ctypes
import os
import shutil
import tempfile
import zlib

import numpy as np

import zstd_dict_cases as ZC
from conftest import GOLDEN, load_golden, unpack

ZLIB = 2
DICT_MAX = 32768
WINDOW = 65536
DS = ZC.DS
LS = ZC.LS
KINDS = ZC.KINDS
PAIRS = ZC.PAIRS
GOLDEN_DS = (1, 64, 4096, 32768)
GOLDEN_LS = (1, 65, 4096, 16384)
GOLDEN_FILE = os.path.join(GOLDEN, "zlib_dict.npz")
Z_DATA, Z_BUF = -3, -5

# dictionaries, pages, the "used" case and the ratio cells are the zstd dictionary tests'
dict_of, page_of, all_cases, gen = ZC.dict_of, ZC.page_of, ZC.all_cases, ZC.gen
USED_D, USED_LS, used_case = ZC.USED_D, ZC.USED_LS, ZC.used_case
RATIO_PAGES, RATIO_DICT, RATIO_CELLS, ratio_inputs = ZC.RATIO_PAGES, ZC.RATIO_DICT, ZC.RATIO_CELLS, ZC.ratio_inputs
crc = ZC.crc


def zlib_bound(n: int) -> int:
    return n + (n >> 12) + (n >> 14) + (n >> 25) + 13   # compressBound (zlib 1.2.8) = tyche_compress_bound


def adler(b: bytes) -> int:
    return zlib.adler32(b) & 0xFFFFFFFF


def dict_header(dic: bytes, flg: int = 0x3F) -> bytes:
    return bytes([0x78, flg]) + adler(dic).to_bytes(4, "big")


def stored_stream(page: bytes) -> bytes:
    """The plain encoder's stored form of a page below 65,536 bytes: 78 01, one final stored block, adler32."""
    n = len(page)
    return b"\x78\x01\x01" + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + page + adler(page).to_bytes(4, "big")


def golden_pairs():
    return [(d, l) for d in GOLDEN_DS for l in GOLDEN_LS]


# ---------------------------------------------------------------- Python's zlib as a checker
def py_compress(dic: bytes, page: bytes, level: int = 1) -> bytes:
    c = zlib.compressobj(level, zdict=dic) if dic else zlib.compressobj(level)
    return c.compress(page) + c.flush()


def py_decompress(dic, stream: bytes, cap: int):
    """uncompress with the dictionary offered when inflate asks for it, as Python's zlib runs it:
    (length, bytes), or (-3, b"") for a data error or a stream that ends early, (-5, b"") for more
    than cap bytes of output.  dic None or empty: no dictionary to offer."""
    d = zlib.decompressobj(zdict=dic) if dic else zlib.decompressobj()
    try:
        out = d.decompress(stream, cap + 1)
    except zlib.error:
        return Z_DATA, b""
    if len(out) > cap:
        return Z_BUF, b""
    if not d.eof:
        return (Z_BUF, b"") if d.unconsumed_tail else (Z_DATA, b"")
    return len(out), out


# ---------------------------------------------------------------- the reference's zlib through ctypes
class _ZStream(ctypes.Structure):
    _fields_ = [("next_in", ctypes.c_void_p), ("avail_in", ctypes.c_uint), ("total_in", ctypes.c_ulong),
                ("next_out", ctypes.c_void_p), ("avail_out", ctypes.c_uint), ("total_out", ctypes.c_ulong),
                ("msg", ctypes.c_char_p), ("state", ctypes.c_void_p), ("zalloc", ctypes.c_void_p),
                ("zfree", ctypes.c_void_p), ("opaque", ctypes.c_void_p), ("data_type", ctypes.c_int),
                ("adler", ctypes.c_ulong), ("reserved", ctypes.c_ulong)]


Z_FINISH, Z_OK, Z_STREAM_END, Z_NEED_DICT = 4, 0, 1, 2


class Ref:
    """deflateInit_ / deflateSetDictionary / deflate and inflateInit_ / inflateSetDictionary / inflate of
    the reference's zlib 1.2.8 (oracle.REF_SO), driven as compress2 and uncompress drive them."""
    VERSION = b"1.2.8"

    def __init__(self, O):
        # The Python process already holds a zlib of its own with global symbols (1.2.11 here), and the
        # reference library's internal calls (deflateInit_ -> deflateInit2_, ...) would bind to that one:
        # a 1.2.8 deflate() would then run on a 1.2.11 state.  So the library is loaded with
        # RTLD_DEEPBIND, its own symbols first -- from a private copy, because a library that is loaded
        # already (oracle.py loads it plainly) keeps the binding it has.
        with tempfile.TemporaryDirectory() as tmp:
            own = shutil.copy(O.REF_SO, os.path.join(tmp, "libtyche_ref_zdict.so"))
            self.lib = L = ctypes.CDLL(own, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        L.zlibVersion.restype = ctypes.c_char_p
        assert L.zlibVersion() == self.VERSION
        sp = ctypes.POINTER(_ZStream)
        L.deflateInit_.argtypes = [sp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.inflateInit_.argtypes = [sp, ctypes.c_char_p, ctypes.c_int]
        for f in (L.deflateSetDictionary, L.inflateSetDictionary):
            f.argtypes = [sp, ctypes.c_void_p, ctypes.c_uint]
        for f in (L.deflate, L.inflate):
            f.argtypes = [sp, ctypes.c_int]
        for f in (L.deflateEnd, L.inflateEnd):
            f.argtypes = [sp]

    def compress(self, dic: bytes, page: bytes, level: int = 1) -> bytes:
        """compress2 at `level` with deflateSetDictionary between init and deflate (dic empty: without)."""
        s = _ZStream()
        assert self.lib.deflateInit_(ctypes.byref(s), level, self.VERSION, ctypes.sizeof(s)) == Z_OK
        d = np.frombuffer(dic, np.uint8).copy() if dic else None
        if d is not None:
            assert self.lib.deflateSetDictionary(ctypes.byref(s), d.ctypes.data, len(dic)) == Z_OK
        src = np.frombuffer(page, np.uint8).copy() if page else np.zeros(1, np.uint8)
        out = np.zeros(zlib_bound(len(page)) + 64, np.uint8)   # (zlib overruns compressBound with a DICTID)
        s.next_in, s.avail_in, s.next_out, s.avail_out = src.ctypes.data, len(page), out.ctypes.data, len(out)
        assert self.lib.deflate(ctypes.byref(s), Z_FINISH) == Z_STREAM_END
        n = int(s.total_out)
        self.lib.deflateEnd(ctypes.byref(s))
        return out[:n].tobytes()

    def decompress(self, dic, stream: bytes, cap: int):
        """uncompress (uncompr.c) with inflateSetDictionary when inflate returns Z_NEED_DICT and a
        dictionary is there to offer: (length, bytes) or (-3 / -5, b"")."""
        s = _ZStream()
        src = np.zeros(len(stream) + 16, np.uint8)
        src[:len(stream)] = np.frombuffer(stream, np.uint8)
        out = np.zeros(max(cap, 1) + 64, np.uint8)
        s.next_in, s.avail_in, s.next_out, s.avail_out = src.ctypes.data, len(stream), out.ctypes.data, cap
        assert self.lib.inflateInit_(ctypes.byref(s), self.VERSION, ctypes.sizeof(s)) == Z_OK
        err = self.lib.inflate(ctypes.byref(s), Z_FINISH)
        if err == Z_NEED_DICT and dic:
            d = np.frombuffer(dic, np.uint8).copy()
            if self.lib.inflateSetDictionary(ctypes.byref(s), d.ctypes.data, len(dic)) != Z_OK:
                self.lib.inflateEnd(ctypes.byref(s))
                return Z_DATA, b""
            err = self.lib.inflate(ctypes.byref(s), Z_FINISH)
        n, left = int(s.total_out), int(s.avail_in)
        self.lib.inflateEnd(ctypes.byref(s))
        if err != Z_STREAM_END:
            if err == Z_NEED_DICT or (err == Z_BUF and left == 0):
                return Z_DATA, b""
            return err, b""
        return n, out[:n].tobytes()


def ref_or_none(O):
    return Ref(O) if O.have_ref() else None


# ---------------------------------------------------------------- a deflate bit-writer (fixed codes)
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_XB = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577]
_DIST_XB = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v: int, n: int):          # n bits of v, least significant first (headers, extra bits)
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c: int, n: int):          # a Huffman code, most significant bit first
        for k in range(n - 1, -1, -1):
            self.bits((c >> k) & 1, 1)

    def litlen(self, s: int):                # RFC 1951 3.2.6
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def match(self, length: int, dist: int):
        i = max(k for k in range(29) if _LEN_BASE[k] <= length and (k == 28 or length < 258))
        self.litlen(257 + i)
        self.bits(length - _LEN_BASE[i], _LEN_XB[i])
        j = max(k for k in range(30) if _DIST_BASE[k] <= dist)
        self.code(j, 5)
        self.bits(dist - _DIST_BASE[j], _DIST_XB[j])

    def done(self) -> bytes:
        if self.n:
            self.out.append(self.acc & 255)
            self.acc, self.n = 0, 0
        return bytes(self.out)


def craft(header: bytes, ops, dic: bytes = b""):
    """A zlib stream of one final fixed-code block: ops are ("lit", bytes) and ("match", length,
    distance).  Returns (stream, the page the ops spell over dic + output -- b"" where a distance
    reaches before the dictionary).  The trailer is the adler32 of that page."""
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    win, legal = bytearray(dic), True
    for op in ops:
        if op[0] == "lit":
            for b in op[1]:
                w.litlen(b)
                win.append(b)
        else:
            _, length, dist = op
            w.match(length, dist)
            if dist > len(win):
                legal = False
            for _ in range(length if legal else 0):
                win.append(win[-dist])
    w.litlen(256)
    page = bytes(win[len(dic):]) if legal else b""
    return header + w.done() + adler(page).to_bytes(4, "big"), page


def _rand(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def crafted_cases():
    """[(name, dictionary offered to the decoder, stream, capacity, want)]: want is the page, or -3.
    Reasoned from inflate.c; tests/golden/zlib_dict.npz has what the reference answered."""
    out = []
    lits = b"hello"

    def add(name, dic, stream, page_or_rv, cap=None):
        cap = (len(page_or_rv) if isinstance(page_or_rv, bytes) else 600) if cap is None else cap
        out.append((name, dic, stream, cap, page_or_rv))

    # a distance of exactly position + D is legal, one more is "invalid distance too far back"
    # (D = 32768 leaves no room for position 5: 32,768 is deflate's largest distance; D = 32763 has it)
    for D, pos in ((1, 0), (1, 5), (64, 0), (64, 5), (4095, 0), (4095, 5), (32768, 0), (32763, 5)):
        dic = _rand(100 + D, D)
        pre = [("lit", lits)] if pos else []
        s, page = craft(dict_header(dic), pre + [("match", 258 if pos == 0 else 10, pos + D)], dic)
        add(f"reach/D{D}/pos{pos}", dic, s, page)
        if pos + D + 1 <= 32768:
            s, _ = craft(dict_header(dic), pre + [("match", 10, pos + D + 1)], dic)
            add(f"too-far/D{D}/pos{pos}", dic, s, Z_DATA)
    dic = _rand(7, 64)
    # no FDICT: inflate never asks for the dictionary, so nothing before the page can be reached
    s, _ = craft(b"\x78\x01", [("match", 10, 1)], dic)
    add("plain-header/reaches-dictionary", dic, s, Z_DATA)
    s, page = craft(b"\x78\x01", [("lit", lits), ("match", 20, 5)])
    add("plain-header/own-output", dic, s, page)
    # matches that begin in the dictionary and overlap their own output, or run over the seam
    for name, dc, ops in (("overlap/D3", b"abc", [("match", 258, 3)]),
                          ("overlap/D1", b"z", [("match", 258, 1), ("match", 70, 1)]),
                          ("seam/D64", dic, [("lit", lits), ("match", 30, 10), ("match", 100, 64 + 35)]),
                          ("seam/long", dic, [("lit", lits), ("match", 258, 40), ("match", 258, 64 + 5 + 258)])):
        s, page = craft(dict_header(dc), ops, dc)
        add(name, dc, s, page)
    # header forms, truncations, the wrong dictionary
    body_ops = [("lit", lits), ("match", 40, 64 + 5), ("lit", b"!")]
    good, page = craft(dict_header(dic), body_ops, dic)
    for flg in (0x20, 0xBB, 0x7D, 0xF9):
        assert (0x7800 | flg) % 31 == 0 and flg & 0x20
        s, _ = craft(dict_header(dic, flg), body_ops, dic)
        add(f"flg/{flg:02X}", dic, s, page)
    for k in (2, 3, 5):
        add(f"truncated/{k}", dic, good[:k], Z_DATA, cap=len(page))
    add("wrong-dictionary/shorter", dic[1:], good, Z_DATA, cap=len(page))
    add("wrong-dictionary/other", _rand(8, 64), good, Z_DATA, cap=len(page))
    add("right-dictionary", dic, good, page)
    add("capacity-one-short", dic, good, Z_BUF, cap=len(page) - 1)
    return out


# ---------------------------------------------------------------- malformed streams with a dictionary
MALFORMED_D = 4096


def malformed_cases(O):
    """(dictionary, [(stream, capacity)]): every stream of tests/golden/zlib_malformed.npz, to be
    decoded with a 4 KiB dictionary."""
    g = load_golden("zlib_malformed.npz")
    return dict_of(O, MALFORMED_D), [(unpack(g["comp"], g["comp_off"], g["comp_len"], i), int(g["cap"][i]))
                                     for i in range(len(g["cap"]))]


# ---------------------------------------------------------------- golden file
class Golden:
    """tests/golden/zlib_dict.npz: what the reference library answered when the file was recorded."""

    def __init__(self):
        g = np.load(GOLDEN_FILE, allow_pickle=False)
        self.rt_streams = [unpack(g["rt_data"], g["rt_off"], g["rt_len"], i) for i in range(len(g["rt_len"]))]
        self.crafted_rv = g["crafted_rv"]          # crafted_cases order: decoded length, -3 or -5
        self.crafted_crc = g["crafted_crc"]
        self.malformed_rv = g["malformed_rv"]
        self.malformed_crc = g["malformed_crc"]
        self.used_ref = g["used_ref"]              # USED_LS order: reference bytes with the dictionary
        self.used_ref_plain = g["used_ref_plain"]
        self.ratio_ref = g["ratio_ref"]            # RATIO_CELLS order: reference level-1 bytes with the dictionary
        self.ratio_ref_plain = g["ratio_ref_plain"]

    def rt_cases(self, O):
        """(D, L, kind, dictionary, page, reference-made stream) of the golden subset."""
        cs = all_cases(O, golden_pairs())
        assert len(cs) == len(self.rt_streams)
        return [c + (s,) for c, s in zip(cs, self.rt_streams)]
