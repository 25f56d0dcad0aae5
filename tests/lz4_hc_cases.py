"""Inputs and checks shared by the high-compression LZ4 encoder's tests (LZ4_HC=1;
test_lz4_hc_emul.py on the CPU through the emulator tools/lz4_hc_emul.cpp, test_gpu_lz4_hc.py on
the kernel tyche_amd/csrc/lz4_encode_hc.hip): the emulator's loader, the stream walker that checks
LZ4's end rules, the page lists and the ratio condition.  The mode promises a valid LZ4 block, not
particular bytes, so the expected bytes of a GPU test are the emulator's and the CPU tests hold the
emulator to the block format, the limited-output contract and the ratio."""
import ctypes
import json
import os
import subprocess

import numpy as np

from lz4_exact_cases import KINDS, kind_pages, limited_pages, ragged_pages  # noqa: F401  (re-exported)
from lz4_large_cases import walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "bin", "liblz4hcemul.so")
SRC = os.path.join(ROOT, "tools", "lz4_hc_emul.cpp")
CORES = [os.path.join(ROOT, "tyche_amd", "csrc", f) for f in ("lz4_hc_core.h", "lz4_exact_core.h")]
TARGETS = os.path.join(ROOT, "tests", "golden", "lz4_hc_targets.json")
GUARD = 64
FILL = 0xAB

PAGE_LENS = (4096, 16384, 65535)
SMALL_LENS = (0, 1, 4, 5, 11, 12, 13, 14, 63, 64, 65, 127, 128, 129, 16385)
RATIO_DISTS = (0, 1, 2, 5)          # judged; 3 (all but constant) and 4 (incompressible) are recorded only
RATIO_PAGES, RATIO_PLEN = 256, 16384


def lz4_bound(n):
    return n + n // 255 + 16


def load_emul():
    """enc(page, cap) -> (return value, the bytes it covers); builds the emulator when it is missing
    or older than its sources, and asserts that nothing at or past cap was written."""
    if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in [SRC] + CORES):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.lz4hc_emul_compress.restype = ctypes.c_int
    record = os.environ.get("LZ4_HC_EMUL_RECORD")   # the calls, for the sanitizer replay (tools/lz4_hc_emul.cpp)

    def enc(page: bytes, cap=None):
        cap = lz4_bound(len(page)) if cap is None else cap
        src = (ctypes.c_uint8 * max(len(page), 1)).from_buffer_copy(page if page else b"\0")
        dst = np.full(cap + GUARD + 15, FILL, np.uint8)
        shift = (len(page) + cap) % 16                # every destination alignment over a test's calls
        a = (-dst.ctypes.data) % 16 + shift
        r = lib.lz4hc_emul_compress(src, len(page), ctypes.c_void_p(dst.ctypes.data + a), cap)
        assert bool((dst[:a] == FILL).all()) and bool((dst[a + cap:] == FILL).all()), ("wrote outside the capacity", len(page), cap)
        if record:
            with open(record, "ab") as f:
                f.write(np.array([len(page), cap, r & 0xFFFFFFFF, shift], np.uint32).tobytes() + page)
        return r, dst[a:a + max(r, 0)].tobytes()
    enc.lib = lib
    return enc


def check_stream(stream: bytes, page: bytes):
    """The block's own rules (lz4.c's MFLIMIT / LASTLITERALS and the format): it is no longer than
    the bound, decodes to the page with every offset in 1..position, its last match starts at or
    before n - 12, and its last 5 bytes are literals."""
    n = len(page)
    assert 0 < len(stream) <= lz4_bound(n), (n, len(stream))
    out = bytearray()
    seqs = walk(stream)
    assert seqs and seqs[-1][2] is None, "the block does not end in a literal-only sequence"
    for tp, ll, op in seqs:
        lit_end = op if op is not None else len(stream)
        out += stream[lit_end - ll:lit_end]
        if op is None:
            assert lit_end == len(stream)
            assert ll >= min(n, 5) and (len(seqs) == 1 or ll >= 5), ("last literals", n, ll)
            break
        off = stream[op] | (stream[op + 1] << 8)
        assert 1 <= off <= len(out), ("offset", off, len(out))
        ml, ip = (stream[tp] & 15), op + 2
        if ml == 15:
            while True:
                s = stream[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        ml += 4
        assert len(out) <= n - 12, ("a match starts after n - 12", len(out), n)
        for _ in range(ml):
            out.append(out[-off])
        assert len(out) <= n - 5, ("a match ends in the last 5 bytes", len(out), n)
    assert bytes(out) == page, n


def restores(O, stream: bytes, page: bytes) -> bool:
    """Through the oracle's LZ4_decompress_safe and, where it is built, the reference's."""
    r, dec = O.lz4_decompress(stream, len(page))
    ok = r == len(page) and bytes(dec)[:len(page)] == page
    if ok and O.have_ref():
        r, dec = O.ref_lz4_decompress(stream, len(page))
        ok = r == len(page) and bytes(dec)[:len(page)] == page
    return ok


def small_pages():
    """One page per length of SMALL_LENS: text-like bytes over 5 symbols, so the short ones hold matches."""
    rng = np.random.default_rng(77)
    return [(rng.integers(0, 5, n, dtype=np.uint8) * 50).tobytes() for n in SMALL_LENS]


def limited_caps(full, bound, seed):
    """The capacities of the limited-output tests for a page whose HC stream takes `full` bytes."""
    caps = [full - 1, full, full + 1, 0, 1, 2, 12, 13, bound - 1, bound]
    return caps + [int(c) for c in np.random.default_rng(seed).integers(0, full + 16, 32)]


def ratio_pages(O, dist, plen=RATIO_PLEN, n=RATIO_PAGES):
    return O.pagegen(n, plen, dist=dist)


def hc3_total(dist, first64=False):
    """Total bytes of liblz4's LZ4_compress_HC level 3 over ratio_pages(dist), or over its first
    64 pages, recorded by tools/gen_lz4_hc_golden.py."""
    with open(TARGETS) as f:
        t = json.load(f)
    assert t["pages"] == RATIO_PAGES and t["page_len"] == RATIO_PLEN and t["level"] == 3
    return int(t["hc_bytes_first64" if first64 else "hc_bytes"][str(dist)])


def ratio_bar(F, H):
    """The most bytes the mode may take: it closes at least half of the gap between the fast
    parse's total F and HC level 3's total H."""
    return F - (F - H) / 2


def mixed_4k_pages(O, n=300):
    """n 4 KiB pages of all six distributions, shuffled: more than a launch's resident waves."""
    per = (n + 5) // 6
    host = np.concatenate([O.pagegen(per, 4096, seed=515, first=1000 * d, dist=d) for d in range(6)])
    return np.ascontiguousarray(host[np.random.default_rng(4).permutation(len(host))[:n]])
