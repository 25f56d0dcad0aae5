"""Inputs and checks shared by the high-compression zlib encoder's tests (ZLIB_HC=1;
test_zlib_hc_emul.py on the CPU through the emulator tools/zlib_hc_emul.cpp, test_gpu_zlib_hc.py on
the kernel zlib_deflate_hc_kernel of tyche_amd/csrc/zlib_deflate_hc.hip): the emulator's loader, the
page makers, a deflate symbol walker, the chunk rule that cuts a record into symbols, an exact
dynamic-Huffman size of a record list, and the ratio targets.  The mode promises an ordinary zlib
stream from a stated parse; what ties the kernel to the emulator is the parse, so a GPU test
compares the symbols walked out of the kernel's stream with the emulator's records."""
import ctypes
import heapq
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
LIB = os.path.join(BIN, "libzlibhcemul.so")
SRC = os.path.join(ROOT, "tools", "zlib_hc_emul.cpp")
CORES = [os.path.join(ROOT, "tyche_amd", "csrc", f) for f in ("zlib_hc_core.h", "lz4_hc_core.h", "lz4_exact_core.h")]
TARGETS = os.path.join(ROOT, "tests", "golden", "zlib_hc_targets.json")
DEFAULT_DIGESTS = os.path.join(ROOT, "tests", "golden", "zlib_default_digests.json")

RATIO_DISTS = (0, 1, 5)             # the nine judged cells
NOGROW_DISTS = (2,)                 # recorded too: HC must not be larger than the default there
RATIO_LENS = (4096, 16384, 32768)
RATIO_PAGES = 48
RATIO_FIRST = 1000
MAX_DIST = 32768


def ratio_pages(O, dist, plen):
    return O.pagegen(RATIO_PAGES, plen, first=RATIO_FIRST, dist=dist)


def _stale(lib, sources):
    return not os.path.exists(lib) or any(os.path.getmtime(f) > os.path.getmtime(lib) for f in sources)


def load_emul(defines=(), lib_path=LIB):
    """parse(page) -> (records [(ls, ll, ml, dist)], last literal run); builds the emulator when it
    is missing or older than its sources.  parse.trace(page) -> the blocks' gains; parse.layout:
    the constants of zlib_hc_core.h the library was built with."""
    if _stale(lib_path, [SRC] + CORES):
        os.makedirs(BIN, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", lib_path, SRC] + ["-D" + d for d in defines])
    lib = ctypes.CDLL(lib_path)
    lib.zlibhc_emul_parse.restype = ctypes.c_int
    lib.zlibhc_emul_trace.restype = ctypes.c_int
    record = os.environ.get("ZLIB_HC_EMUL_RECORD")   # the calls, for the sanitizer replay (tools/zlib_hc_emul.cpp)

    def parse(page: bytes):
        n = len(page)
        src = (ctypes.c_uint8 * max(n, 1)).from_buffer_copy(page if page else b"\0")
        cap = n // 3 + 1
        recs = np.zeros(4 * cap, np.uint32)
        last = ctypes.c_uint32(0)
        r = lib.zlibhc_emul_parse(src, n, recs.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(last))
        assert 0 <= r <= cap, (n, r)
        if record:
            d = 2166136261
            for v in recs[:4 * r].tolist() + [last.value]:
                d = ((d ^ v) * 16777619) & 0xFFFFFFFF
            with open(record, "ab") as f:
                f.write(np.array([n, r, d, 0], np.uint32).tobytes() + page)
        return [tuple(t) for t in recs[:4 * r].reshape(r, 4).tolist()], int(last.value)

    def trace(page: bytes):
        n = len(page)
        src = (ctypes.c_uint8 * max(n, 1)).from_buffer_copy(page if page else b"\0")
        cap = n // 62 + 3
        out = np.zeros(196 * cap, np.uint32)
        r = lib.zlibhc_emul_trace(src, n, out.ctypes.data_as(ctypes.c_void_p), cap)
        assert 0 <= r <= cap, (n, r)
        return out[:196 * r].reshape(r, 196)

    lay = (ctypes.c_uint32 * 11)()
    lib.zlibhc_emul_layout(lay)
    parse.layout = dict(zip(("ways", "hash_log", "probe", "len_w", "far3", "far4", "lazy1", "lazy2", "gain_base",
                             "stride", "back_max"), [int(v) for v in lay]))
    parse.trace = trace
    parse.lib = lib
    return parse


# ---- the chunk rule (n_chunks / chunk_len of zlib_deflate_core.h) and the symbols of a record list

def chunks(ml):
    """The lengths a match of ml bytes is coded as: 258-byte chunks, a 1- or 2-byte tail borrowing
    from the chunk before it."""
    if ml == 0:
        return []
    n = (ml + 257) // 258
    last = ml - 258 * (n - 1)
    if last >= 3:
        return [258] * (n - 1) + [last]
    return [258] * (n - 2) + [258 - (3 - last), 3]


def record_symbols(recs, last, page: bytes):
    """The symbols of a stream coded from the records: ints for literal bytes, (length, distance)
    for match chunks."""
    out = []
    end = 0
    for ls, ll, ml, d in recs:
        out.extend(page[ls:ls + ll])
        out.extend((c, d) for c in chunks(ml))
        end = ls + ll + ml
    out.extend(page[end:end + last])
    return out


def check_records(recs, last, page: bytes):
    """The records tile the page in order, every match is a true match of at least 3 bytes at a
    distance of 1..min(position, 32768)."""
    n = len(page)
    a = np.frombuffer(page, np.uint8)
    end = 0
    for ls, ll, ml, d in recs:
        assert ls == end, ("a record does not start where the last one ended", ls, end)
        p = ls + ll
        assert ml >= 3, ("match length", ml, p)
        assert 1 <= d <= min(p, MAX_DIST), ("distance", d, p)
        assert p + ml <= n, ("a match runs past the page", p, ml, n)
        assert np.array_equal(a[p:p + ml], a[p - d:p - d + ml]), ("not a match", p, ml, d)
        end = p + ml
    assert end + last == n, ("the records do not tile the page", end, last, n)
    assert len(recs) <= n // 3


# ---- deflate symbol walker (RFC 1950 / 1951)

_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _decode_table(lengths):
    """(table over maxbits reversed bits -> (symbol, length), maxbits) of a canonical code."""
    maxb = max(lengths) if len(lengths) else 0
    assert maxb > 0, "an empty code"
    count = [0] * (maxb + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt = [0] * (maxb + 2)
    code = 0
    for b in range(1, maxb + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = [None] * (1 << maxb)
    for s, l in enumerate(lengths):
        if l:
            c = nxt[l]
            nxt[l] += 1
            r = int(format(c, "0%db" % l)[::-1], 2)
            for k in range(r, 1 << maxb, 1 << l):
                table[k] = (s, l)
    return table, maxb


class _Bits:
    def __init__(self, data, pos):
        self.d, self.p, self.acc, self.n = data, pos, 0, 0

    def need(self, k):
        while self.n < k:
            self.acc |= (self.d[self.p] if self.p < len(self.d) else 0) << self.n
            self.p += 1
            self.n += 8

    def get(self, k):
        if k == 0:
            return 0
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def sym(self, tab):
        table, maxb = tab
        self.need(maxb)
        e = table[self.acc & ((1 << maxb) - 1)]
        assert e is not None, "a code the tree does not hold"
        self.acc >>= e[1]
        self.n -= e[1]
        return e[0]

    def align(self):
        drop = self.n & 7
        self.acc >>= drop
        self.n -= drop
        # whole bytes still buffered go back
        self.p -= self.n // 8
        self.acc, self.n = 0, 0


_FIXED = None


def walk(stream: bytes):
    """(symbols, decoded bytes, block types) of a zlib stream: ints for literals, (length,
    distance) for matches; the bytes of stored blocks appear as literals.  Checks the header, the
    stream's end and the adler32."""
    global _FIXED
    assert len(stream) >= 6 and stream[0] == 0x78 and (stream[0] * 256 + stream[1]) % 31 == 0 and not stream[1] & 0x20
    b = _Bits(stream, 2)
    out = bytearray()
    syms = []
    kinds = []
    while True:
        final = b.get(1)
        bt = b.get(2)
        kinds.append(bt)
        if bt == 0:
            b.align()
            n = stream[b.p] | (stream[b.p + 1] << 8)
            assert n ^ 0xFFFF == stream[b.p + 2] | (stream[b.p + 3] << 8)
            blk = stream[b.p + 4:b.p + 4 + n]
            assert len(blk) == n
            out += blk
            syms.extend(blk)
            b.p += 4 + n
        else:
            assert bt in (1, 2)
            if bt == 1:
                if _FIXED is None:
                    _FIXED = (_decode_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _decode_table([5] * 30))
                lt, dt = _FIXED
            else:
                hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_CL_ORDER[i]] = b.get(3)
                ct = _decode_table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = b.sym(ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.get(2))
                    elif s == 17:
                        lens += [0] * (3 + b.get(3))
                    else:
                        lens += [0] * (11 + b.get(7))
                assert len(lens) == hlit + hdist
                lt, dt = _decode_table(lens[:hlit]), _decode_table(lens[hlit:])
            while True:
                s = b.sym(lt)
                if s < 256:
                    out.append(s)
                    syms.append(s)
                elif s == 256:
                    break
                else:
                    assert s <= 285
                    ln = _LBASE[s - 257] + b.get(_LEXT[s - 257])
                    ds = b.sym(dt)
                    assert ds < 30
                    d = _DBASE[ds] + b.get(_DEXT[ds])
                    assert d <= len(out), ("distance before the page", d, len(out))
                    syms.append((ln, d))
                    if d >= ln:
                        out += out[len(out) - d:len(out) - d + ln]
                    else:
                        for _ in range(ln):
                            out.append(out[-d])
        if final:
            break
    b.align()
    assert b.p + 4 == len(stream), ("bytes behind the stream's end", b.p, len(stream))
    a, s2 = 1, 0
    arr = np.frombuffer(bytes(out), np.uint8).astype(np.uint64)
    for i in range(0, len(arr), 4096):      # adler32 in exact integer steps
        c = arr[i:i + 4096]
        n = len(c)
        s2 = (s2 + n * a + int((c * np.arange(n, 0, -1, dtype=np.uint64)).sum())) % 65521
        a = (a + int(c.sum())) % 65521
    assert int.from_bytes(stream[-4:], "big") == (s2 << 16 | a), "adler32"
    return syms, bytes(out), kinds


# ---- exact size of the dynamic-Huffman stream of a record list (an estimate of the device's
# stream: optimal length-limited codes, where the device's construction may differ by a few bits)

def limited_lengths(freqs, maxbits):
    """Optimal code lengths of at most maxbits (package-merge) for the used symbols of freqs."""
    used = [(int(f), i) for i, f in enumerate(freqs) if f > 0]
    lens = [0] * len(freqs)
    if len(used) == 1:
        lens[used[0][1]] = 1
        return lens
    if not used:
        return lens
    # plain Huffman first
    heap = [(f, i, None, None) for f, i in used]
    heapq.heapify(heap)
    uid = len(freqs)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], uid, a, b))
        uid += 1
    stack = [(heap[0], 0)]
    deepest = 0
    while stack:
        node, depth = stack.pop()
        if node[2] is None:
            lens[node[1]] = depth
            deepest = max(deepest, depth)
        else:
            stack.append((node[2], depth + 1))
            stack.append((node[3], depth + 1))
    if deepest <= maxbits:
        return lens
    n = len(used)
    idx = {s: j for j, (_, s) in enumerate(sorted(used))}
    leaves = []
    for f, s in sorted(used):
        v = np.zeros(n, np.int32)
        v[idx[s]] = 1
        leaves.append((f, v))
    cur = list(leaves)
    for _ in range(maxbits - 1):
        pk = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda t: t[0])
    tot = sum(v for _, v in cur[:2 * n - 2])
    for s, j in idx.items():
        lens[s] = int(tot[j])
    return lens


def _len_sym(ln):
    for s in range(28, -1, -1):
        if ln >= _LBASE[s]:
            return s
    raise AssertionError(ln)


_LEN_SYM = [0] * 259
for _l in range(3, 259):
    _LEN_SYM[_l] = _len_sym(_l)


def _dist_sym(d):
    d -= 1
    if d < 4:
        return d
    h = d.bit_length() - 1
    return 2 * h + ((d >> (h - 1)) & 1)


def _tree_bits(lens):
    """(counts of the 19 code-length symbols, their extra bits) of a code-length sequence
    (trees.c scan_tree)."""
    cnt = [0] * 19
    extra = 0
    n = len(lens)
    prevlen, nextlen, count = -1, lens[0], 0
    max_count, min_count = (138, 3) if nextlen == 0 else (7, 4)
    for i in range(n):
        curlen = nextlen
        nextlen = lens[i + 1] if i + 1 < n else 0xFFFF
        count += 1
        if count < max_count and curlen == nextlen:
            continue
        if count < min_count:
            cnt[curlen] += count
        elif curlen != 0:
            if curlen != prevlen:
                cnt[curlen] += 1
            cnt[16] += 1
            extra += 2
        elif count <= 10:
            cnt[17] += 1
            extra += 3
        else:
            cnt[18] += 1
            extra += 7
        count, prevlen = 0, curlen
        max_count, min_count = (138, 3) if nextlen == 0 else (6, 3) if curlen == nextlen else (7, 4)
    return cnt, extra


def stream_size(recs, last, page: bytes):
    """The bytes of the zlib stream that codes the records in one block: dynamic or fixed codes,
    whichever is smaller, or the stored form when that is not larger."""
    n = len(page)
    a = np.frombuffer(page, np.uint8)
    lit = np.zeros(n, bool)
    ll_h = [0] * 286
    d_h = [0] * 30
    extra = 0
    end = 0
    for ls, ll, ml, d in recs:
        lit[ls:ls + ll] = True
        ds = _dist_sym(d)
        for c in chunks(ml):
            s = _LEN_SYM[c]
            ll_h[257 + s] += 1
            d_h[ds] += 1
            extra += _LEXT[s] + _DEXT[ds]
        end = ls + ll + ml
    lit[end:] = True
    ll_h[:256] = np.bincount(a[lit], minlength=256).tolist()
    ll_h[256] = 1
    lll = limited_lengths(ll_h, 15)
    if sum(1 for x in lll if x) < 2:
        lll[0] = lll[256] = 1
    dl = limited_lengths(d_h, 15)
    if sum(1 for x in dl if x) < 2:
        u = max([i for i, x in enumerate(dl) if x], default=-1)
        dl = [0] * 30
        dl[0] = 1
        dl[u if u > 0 else 1] = 1
    data = sum(f * l for f, l in zip(ll_h, lll)) + sum(f * l for f, l in zip(d_h, dl)) + extra
    nlit = max(257, max(i for i, x in enumerate(lll) if x) + 1)
    ndist = max(1, max(i for i, x in enumerate(dl) if x) + 1)
    c1, x1 = _tree_bits(lll[:nlit])
    c2, x2 = _tree_bits(dl[:ndist])
    clc = [p + q for p, q in zip(c1, c2)]
    cll = limited_lengths(clc, 7)
    if sum(1 for x in cll if x) < 2:
        u = max([i for i, x in enumerate(cll) if x], default=-1)
        cll = [0] * 19
        cll[0] = 1
        cll[u if u > 0 else 1] = 1
    ncl = 19
    while ncl > 4 and cll[_CL_ORDER[ncl - 1]] == 0:
        ncl -= 1
    dyn = 3 + 14 + 3 * ncl + sum(f * l for f, l in zip(clc, cll)) + x1 + x2 + data
    fixed = 3 + sum(f * (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) for s, f in enumerate(ll_h)) + \
        5 * sum(d_h) + extra
    size = 2 + (min(dyn, fixed) + 7) // 8 + 4
    stored = 2 + n + 5 * max(1, (n + 65534) // 65535) + 4
    return min(size, stored)


# ---- pages

SMALL_LENS = (0, 1, 2, 3, 4, 61, 62, 63, 64, 65, 66, 123, 124, 125, 126)
EXACT_LENS = (257, 258, 259, 260, 516, 517)
NEAR3, FAR3 = 100, 5000             # a 3-byte repeat the cost rule takes, and one it refuses


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def exact_match_page(m, seed=3):
    """13 random bytes, a random record of m bytes, 300 random bytes, the record again, and an end
    that differs: one match of exactly m bytes at distance m + 300."""
    rng = np.random.default_rng(seed + m)
    rec = _rand(rng, m)
    tail = bytes([rec[0] ^ 0xFF]) + _rand(rng, 9)      # (differs where the record would go on)
    return _rand(rng, 13) + rec + _rand(rng, 300) + rec + tail


def distance_page(dist, seed=17):
    """40 random non-zero bytes repeated at exactly `dist` bytes, zero bytes between them (one
    bucket's worth of positions: the first copy stays in its rings) and random bytes behind."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 256, 40, dtype=np.uint8).tobytes()
    return _rand(rng, 7) + a + b"\0" * (dist - 40) + a + _rand(rng, 20)


def three_byte_page(dist, seed=23):
    """Bytes over four values (compressible, so the stream is coded, not stored) with the triple
    (250, 251, 252) at two places `dist` apart and nowhere else, a byte that occurs only once before
    and behind each: a repeat of exactly 3 bytes."""
    rng = np.random.default_rng(seed)
    p = bytearray((rng.integers(0, 4, 300 + dist + 300, dtype=np.uint8) * 50).tobytes())
    for at, (pre, post) in ((300, (201, 202)), (300 + dist, (203, 204))):
        p[at - 1:at + 4] = bytes([pre, 250, 251, 252, post])
    return bytes(p)


CROWDED_RUN, CROWDED_KEPT, CROWDED_GAP = 200, 10, 1000


def crowded_page():
    """A run of 200 equal bytes -- every position of a block in one bucket, far more than a ring's
    16 ways, in the parsed block and in the positions the run's match skips -- then a 20-byte tail,
    1,000 random bytes, and the run's last 10 bytes with the tail again.  The repeat of 30 bytes
    starts 10 bytes before the run's end: a candidate that is there only if each store kept the
    latest 16 positions of the bucket.  Returns (page, position of the repeat, its distance)."""
    rng = np.random.default_rng(29)
    tail = rng.integers(1, 200, 20, dtype=np.uint8).tobytes()
    head = _rand(rng, 5)
    page = head + b"\xEE" * CROWDED_RUN + tail + bytes(rng.integers(0, 200, CROWDED_GAP, dtype=np.uint8)) + \
        b"\xEE" * CROWDED_KEPT + tail + b"\xFF" + _rand(rng, 8)
    pos = len(head) + CROWDED_RUN + len(tail) + CROWDED_GAP
    return page, pos, pos - (len(head) + CROWDED_RUN - CROWDED_KEPT)


def cpu_case_pages(O):
    """[(name, page)]: every page the emulator and the kernel are compared on."""
    rng = np.random.default_rng(78)
    out = [(f"small/{n}", (rng.integers(0, 5, n, dtype=np.uint8) * 50).tobytes()) for n in SMALL_LENS]
    out.append(("bench0/65535", O.pagegen(1, 65535, first=RATIO_FIRST, dist=0)[0].tobytes()))
    for shift in (0, 5, 61):
        pre = _rand(rng, shift)
        out.append((f"run/{shift}", pre + b"\x55" * 700))
        for period in (2, 3, 5):
            out.append((f"period{period}/{shift}", pre + bytes(range(65, 65 + period)) * (700 // period)))
    out += [(f"exact/{m}", exact_match_page(m)) for m in EXACT_LENS]
    out += [(f"distance/{d}", distance_page(d)) for d in (32768, 32769)]
    out += [(f"three/{d}", three_byte_page(d)) for d in (NEAR3, FAR3)]
    out.append(("crowded", crowded_page()[0]))
    out += [(f"random/{n}", _rand(rng, n)) for n in (100, 4096)]
    for dist in (0, 1, 2, 5):
        pages = O.pagegen(2, 4096, first=RATIO_FIRST, dist=dist)
        out += [(f"bench{dist}/4096/{i}", pages[i].tobytes()) for i in range(2)]
    return out


def knob_off_sets(O):
    """{group: pages} the default encoder's stream digests are recorded on
    (tests/golden/zlib_default_digests.json): the case set and 16 bench pages per distribution."""
    sets = {"cases": [p for _, p in cpu_case_pages(O)]}
    for dist in range(6):
        sets[f"bench{dist}/16384"] = [p.tobytes() for p in O.pagegen(16, 16384, dist=dist)]
    return sets


def targets():
    """tests/golden/zlib_hc_targets.json (tools/gen_zlib_hc_golden.py): the reference's compress2
    byte totals at levels 1 and 6 over RATIO_PAGES pagegen pages, per distribution and page length."""
    with open(TARGETS) as f:
        t = json.load(f)
    assert t["pages"] == RATIO_PAGES and t["first"] == RATIO_FIRST and t["levels"] == [1, 6]
    return t


def ratio_bar(l1, l6):
    """The most bytes the mode may take in a judged cell: half of the gap between the two levels."""
    return l1 - (l1 - l6) / 2
