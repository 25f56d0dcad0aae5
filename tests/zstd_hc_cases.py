"""Inputs and checks shared by the high-compression zstd encoder's tests (ZSTD_HC=1;
test_zstd_hc_emul.py on the CPU through the emulator tools/zstd_hc_emul.cpp, test_gpu_zstd_hc.py on
the kernel zstd_parse_hc_kernel of tyche_amd/csrc/zstd_encode.hip): the emulator's loader, the
walker that rebuilds a page from its sequences, the collector of a frame's sequences
(tools/zstd_seq_collect.c around the oracle's decoder), the page lists and the ratio targets.  The
mode promises an ordinary zstd frame, not particular bytes; what ties the kernel to the emulator is
the parse, so a GPU test compares the sequences decoded from the kernel's frame with the
emulator's list."""
import ctypes
import json
import os
import subprocess

import numpy as np

from lz4_exact_cases import KINDS, kind_pages, ragged_pages  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
LIB = os.path.join(BIN, "libzstdhcemul.so")
SRC = os.path.join(ROOT, "tools", "zstd_hc_emul.cpp")
CORES = [os.path.join(ROOT, "tyche_amd", "csrc", f) for f in ("zstd_hc_core.h", "lz4_hc_core.h", "lz4_exact_core.h")]
COLLECT_LIB = os.path.join(BIN, "libzstdseqcollect.so")
COLLECT_SRC = [os.path.join(ROOT, "tools", "zstd_seq_collect.c"), os.path.join(ROOT, "oracle", "zstd_oracle.c")]
TARGETS = os.path.join(ROOT, "tests", "golden", "zstd_hc_targets.json")

PAGE_LENS = (4096, 16384, 65535)
SMALL_LENS = (0, 1, 3, 4, 5, 12, 13, 61, 62, 63, 64, 65, 124, 125, 4096, 16384, 16385, 32768, 65535)
RATIO_DISTS = (0, 1, 2, 5)          # judged against the reference's levels; 3 and 4 must not grow
RATIO_LENS = (4096, 16384, 32768)
RATIO_PAGES = 48


def rec_cap(in_cap):
    """enc_rec_cap of zstd_encode.hip: the sequence region's entries for a launch maximum."""
    return in_cap // 4 + 64


def _stale(lib, sources):
    return not os.path.exists(lib) or any(os.path.getmtime(f) > os.path.getmtime(lib) for f in sources)


def load_emul():
    """parse(page) -> (sequences [(ll, ml, off)], last literal run); builds the emulator when it is
    missing or older than its sources."""
    if _stale(LIB, [SRC] + CORES):
        os.makedirs(BIN, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.zstdhc_emul_parse.restype = ctypes.c_int
    record = os.environ.get("ZSTD_HC_EMUL_RECORD")   # the calls, for the sanitizer replay (tools/zstd_hc_emul.cpp)

    def parse(page: bytes):
        n = len(page)
        src = (ctypes.c_uint8 * max(n, 1)).from_buffer_copy(page if page else b"\0")
        cap = n // 4 + 1
        seqs = np.zeros(3 * cap, np.uint32)
        last = ctypes.c_uint32(0)
        r = lib.zstdhc_emul_parse(src, n, seqs.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(last))
        assert 0 <= r <= cap, (n, r)
        if record:
            d = 2166136261
            for v in seqs[:3 * r].tolist() + [last.value]:
                d = ((d ^ v) * 16777619) & 0xFFFFFFFF
            with open(record, "ab") as f:
                f.write(np.array([n, r, d, 0], np.uint32).tobytes() + page)
        return [tuple(int(x) for x in seqs[3 * i:3 * i + 3]) for i in range(r)], int(last.value)
    parse.lib = lib
    return parse


def load_collect():
    """collect(frame, n) -> (decoder's return value, decoded bytes, sequences [(ll, ml, off)]):
    the oracle's zstd decoder with its sequence trace compiled in."""
    if _stale(COLLECT_LIB, COLLECT_SRC):
        os.makedirs(BIN, exist_ok=True)
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-shared", "-fPIC", "-DZSTD_SEQ_TRACE",
                               "-I" + os.path.join(ROOT, "oracle"), "-o", COLLECT_LIB] + COLLECT_SRC)
    lib = ctypes.CDLL(COLLECT_LIB)
    lib.zstd_seq_collect.restype = ctypes.c_int

    def collect(frame: bytes, n: int):
        src = np.zeros(len(frame) + 16, np.uint8)
        src[:len(frame)] = np.frombuffer(frame, np.uint8)
        out = np.zeros(max(n, 1) + 16, np.uint8)
        cap = n // 3 + 1
        seqs = np.zeros(3 * cap, np.uint32)
        ns = ctypes.c_int(0)
        r = lib.zstd_seq_collect(src.ctypes.data_as(ctypes.c_void_p), len(frame), out.ctypes.data_as(ctypes.c_void_p), n,
                                 seqs.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(ns))
        assert ns.value <= cap
        return r, out[:max(r, 0)].tobytes(), [tuple(int(x) for x in seqs[3 * i:3 * i + 3]) for i in range(ns.value)]
    return collect


def check_parse(seqs, last, page: bytes, in_cap=None):
    """The walker: the sequences and the last literal run rebuild the page (literals are taken from
    the page, matches copied from what stands before them); every offset is 1..position, every
    match at least 4 bytes, the runs tile the page exactly, and the count stays within the sequence
    region of a launch whose maximum is in_cap (default: the page's own length)."""
    n = len(page)
    assert len(seqs) <= n // 4, (n, len(seqs))
    assert len(seqs) <= rec_cap(n if in_cap is None else in_cap)
    out = bytearray()
    for ll, ml, off in seqs:
        out += page[len(out):len(out) + ll]
        assert ml >= 4, ("match length", ml, len(out))
        assert 1 <= off <= len(out), ("offset", off, len(out))
        if off >= ml:
            out += out[len(out) - off:len(out) - off + ml]
        else:
            for _ in range(ml):
                out.append(out[-off])
        assert len(out) <= n, ("a match runs past the page", len(out), n)
    assert len(out) + last == n, ("the runs do not tile the page", len(out), last, n)
    out += page[len(out):]
    assert bytes(out) == page, n


def frame_blocks(frame: bytes):
    """[(type, size)] of a single-segment frame's blocks (0 raw, 1 RLE, 2 compressed)."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    assert fhd & 0x20 and not fhd & 0x04 and not fhd & 0x03, "single segment, no checksum, no dictionary id"
    p = 5 + (1, 2, 4, 8)[fhd >> 6]
    blocks = []
    while True:
        h = frame[p] | (frame[p + 1] << 8) | (frame[p + 2] << 16)
        t, size = (h >> 1) & 3, h >> 3
        blocks.append((t, size))
        p += 3 + (1 if t == 1 else size)
        if h & 1:
            break
    assert p == len(frame)
    return blocks


def small_pages():
    """One page per length of SMALL_LENS: text-like bytes over 5 symbols, so the short ones hold matches."""
    rng = np.random.default_rng(78)
    return [(rng.integers(0, 5, n, dtype=np.uint8) * 50).tobytes() for n in SMALL_LENS]


def repeated_record_pages():
    """A 500-byte record repeated 3,000 bytes later and a 3-byte period, at every 7th start lane."""
    rng = np.random.default_rng(5)
    pages = []
    for shift in range(0, 64, 7):
        rec = rng.integers(0, 256, 500, dtype=np.uint8).tobytes()
        pages.append(("record", shift, bytes(rng.integers(0, 256, shift, dtype=np.uint8)) + rec +
                      bytes(rng.integers(0, 256, 2500, dtype=np.uint8)) + rec + b"0123456789ab"))
        pages.append(("period3", shift, bytes(rng.integers(0, 256, shift, dtype=np.uint8)) + b"abc" * 400))
    return pages


def repeat_offset_page(half=6000, seed=11):
    """The second half repeats the first at one fixed offset, except for one changed byte every 40
    to 90 bytes: every match of the second half is best taken at offset `half`, which after the
    first of them is the repeat offset."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, half, dtype=np.uint8)
    b = a.copy()
    p = 50
    while p < half:
        b[p] ^= 0x55
        p += int(rng.integers(40, 90))
    return np.concatenate([a, b]).tobytes(), half


def cpu_case_pages(O):
    """[(name, page)]: every page of the CPU cases that the GPU test runs through the kernel."""
    out = []
    for plen in PAGE_LENS:
        for kind in KINDS:
            pages = kind_pages(O, kind, plen, n=1 if plen == 65535 else 2)
            out += [(f"{kind}/{plen}/{i}", pages[i].tobytes()) for i in range(len(pages))]
    for symbols in (2, 16, 256):
        out += [(f"ragged{symbols}/{len(p)}", p) for p in ragged_pages(symbols)]
    out += [(f"small/{len(p)}", p) for p in small_pages()]
    out += [(f"{name}/{shift}", p) for name, shift, p in repeated_record_pages()]
    out.append(("repeat_offset", repeat_offset_page()[0]))
    return out


def targets():
    """tests/golden/zstd_hc_targets.json (tools/gen_zstd_hc_golden.py): the reference's level-1 and
    level-6 byte totals over the first RATIO_PAGES pagegen pages, per distribution and page length."""
    with open(TARGETS) as f:
        t = json.load(f)
    assert t["pages"] == RATIO_PAGES and t["levels"] == [1, 6]
    return t


def ratio_bar(l1, l6):
    """The most bytes the mode may take in a cell where level 6 saves at least 2 %: half of the gap."""
    return l1 - (l1 - l6) / 2
