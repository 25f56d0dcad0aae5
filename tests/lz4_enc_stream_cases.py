"""Inputs of the LZ4 encoder's stream-digest test (test_gpu_lz4_enc_streams.py) and of the generator
of its fixture (tools/gen_lz4_enc_streams_golden.py -> tests/golden/lz4_enc_streams.npz): pages of
the benchmark's generator, a batch with per-page lengths, pages crafted around the joints of the
four-wave split encoder (tyche_amd/csrc/lz4_encode.hip: part 0 takes 19/64 of a page, three equal
parts the rest; every later part's first match is emitted by wave 0 as the joint sequence), and
capacity cases.  Pure numpy; run_all() is the one place that touches the device, so the test and
the generator compress exactly the same batches.

The fixture holds what the encoder gave when it was recorded: the sha256 and the length of every
stream.  It says nothing about whether a stream is a good one; the test decodes every stream
through the oracle for that, and checks the crafted properties (literal and match lengths of the
joint sequences) on the streams themselves."""
import hashlib
import os

import numpy as np

import batch_layout as BL

LZ4 = 1
INT32_MIN = -(2 ** 31)
PLEN = 16384
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_enc_streams.npz")
BENCH_SEED = 20170303


def bounds(L, nw=4, p0=19):
    """Part boundaries of the split encoder's default (launch_lz4_encode: four waves, part 0 19/64)."""
    h = (L * p0 // 64) & ~63
    return [0] + [(h + ((L - h) * (w - 1)) // (nw - 1)) & ~63 for w in range(1, nw)] + [L]


B = bounds(PLEN)
assert B == [0, 4864, 8704, 12544, 16384]


# ------------------------------------------------------------------ reading a stream
def sequences(stream):
    """[(literal start, literal count, match position, match length, offset)] of an LZ4 block; the
    last item is the closing literal run (match length 0)."""
    s, i, pos, out = stream, 0, 0, []
    while i < len(s):
        tok = s[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                x = s[i]
                i += 1
                lit += x
                if x != 255:
                    break
        i += lit
        if i >= len(s):
            out.append((pos, lit, pos + lit, 0, 0))
            break
        off = s[i] | (s[i + 1] << 8)
        i += 2
        ml = (tok & 15) + 4
        if (tok & 15) == 15:
            while True:
                x = s[i]
                i += 1
                ml += x
                if x != 255:
                    break
        out.append((pos, lit, pos + lit, ml, off))
        pos += lit + ml
    return out


def joint_of(stream, b):
    """The sequence that crosses or starts at part boundary b: the first whose match ends past b
    (a part's matches end by its boundary; the next part's first match starts at most 4 before it)."""
    for q in sequences(stream):
        if q[3] and q[2] + q[3] > b:
            return q
    return None


# ------------------------------------------------------------------ crafted pages
def _slots(page):
    """the 2^10-slot hash of every position's four bytes (lz_parse.h hash4)"""
    p = page.astype(np.uint64)
    v = p[:-3] | (p[1:-2] << 8) | (p[2:-1] << 16) | (p[3:] << 24)
    return ((v * 2654435761) & 0xFFFFFFFF) >> 22


def _survives(page, src, pos):
    """position pos finds src in the table: no position between src and pos's block shares its slot"""
    h = _slots(page)
    blk = pos & ~63
    # (positions of src's own block that share its slot are excluded on both sides: which lane of a
    # block wins a slot is not specified)
    return src < blk and h[src] == h[pos] and int((h[src & ~63:blk] == h[src]).sum()) == 1


def _differ(page, a, b, rng):
    while page[a] == page[b]:
        page[a] = rng.integers(0, 256)


def crafted(w, lit, mlen, back=0, eq=None, e1=None, seed=0):
    """A page of random bytes with two planted matches around part boundary b = B[w]:
    M1 [b-40, e1) in part w-1 (e1 = b - 10 unless given), copied from 128 bytes before it, and M2,
    part w's first match, found at p2 = e1 + lit + back with `eq` (default: back) equal bytes before
    it, mlen bytes long from p2 - back, copied from a multiple of 64 bytes before it.  The bytes
    around the copies differ, so the joint sequence has `lit` literals, a catch-up of `back` bytes
    and a match of mlen bytes.  Seeds are tried until both sources survive in the 2^10-slot table."""
    b = B[w]
    e1 = b - 10 if e1 is None else e1
    eq = back if eq is None else eq
    p2 = e1 + lit + back
    assert p2 >= b and (back == 0 or p2 == b), "the backward extension lies in the previous part"
    m2 = mlen - back                                    # bytes from p2 on
    dist = (m2 + 4 + 180 + 63) // 64 * 64 if p2 - 170 < b + 64 else (m2 + 4 + 63) // 64 * 64 + 64
    for attempt in range(200):
        rng = np.random.default_rng([seed, w, lit, mlen, back, attempt])
        page = rng.integers(0, 256, PLEN, dtype=np.uint8)
        s1, p1 = b - 168, b - 40
        page[p1:e1] = page[s1:s1 + (e1 - p1)]
        _differ(page, s1 - 1, p1 - 1, rng)
        s2 = p2 - dist
        # the source takes the destination's bytes (the destination may overlap M1's tail)
        page[s2 - eq:s2 + m2] = page[p2 - eq:p2 + m2]
        _differ(page, s2 - eq - 1, p2 - eq - 1, rng)
        _differ(page, s2 + m2, p2 + m2, rng)
        if page[e1] == page[s1 + (e1 - p1)]:
            continue
        if _survives(page, s1, p1) and _survives(page, s2, p2):
            return page
    raise AssertionError("no seed found")


def joint_cases():
    """[(name, page, checks)]: checks is a list of (boundary, literals or None, match length or None)
    the joint sequence at that boundary must show."""
    rng = np.random.default_rng(7)
    cases = []
    base = np.frombuffer(bytes(range(256)) * 64, np.uint8)
    text = (np.arange(PLEN) * 37 % 101 % 64 + 32).astype(np.uint8)     # compressible, short matches
    for w in (2, 3):
        p = np.tile(np.frombuffer(b"the quick brown fox jumps over the lazy dog, ", np.uint8), PLEN // 40)[:PLEN].copy()
        p[::97] = rng.integers(0, 256, len(p[::97]), dtype=np.uint8)
        p[B[w - 1]:B[w]] = rng.integers(0, 256, B[w] - B[w - 1], dtype=np.uint8)
        cases.append((f"random_part{w - 1}", p, []))
    cases.append(("random_page", rng.integers(0, 256, PLEN, dtype=np.uint8), []))
    cases.append(("zero_page", np.zeros(PLEN, np.uint8), []))
    cases.append(("period7", np.tile(np.frombuffer(b"abcdefg", np.uint8), PLEN // 7 + 1)[:PLEN].copy(), []))
    cases.append(("ramp", base.copy(), []))
    cases.append(("text", text, []))
    for i, lit in enumerate((14, 15, 269, 270, 271)):
        w = 1 + i % 3
        cases.append((f"lit{lit}_part{w}", crafted(w, lit, 12), [(B[w], lit, 12)]))
    for i, ml in enumerate((18, 19, 273, 274)):
        w = 1 + (i + 1) % 3
        cases.append((f"mlen{ml}_part{w}", crafted(w, 20, ml), [(B[w], 20, ml)]))
    for back in range(5):
        w = 1 + back % 3
        cases.append((f"back{back}_part{w}", crafted(w, 10 - back, 16 + back, back=back), [(B[w], 10 - back, 16 + back)]))
    # four equal bytes before both positions, but M1 ends two bytes before the boundary: the catch-up is 2
    cases.append(("back_capped", crafted(2, 0, 18, back=2, eq=4, e1=B[2] - 2), [(B[2], 0, 18)]))
    return cases


# ------------------------------------------------------------------ the batches
def bench_groups(O):
    """{name: (n, plen) uint8 array}: 64 pages of each generator distribution at 8 and 16 KiB"""
    return {f"bench_{plen}_d{d}": O.pagegen(64, plen, seed=BENCH_SEED, first=0, dist=d)
            for plen in (8192, 16384) for d in range(6)}


RAGGED_LENGTHS = (8192, 12352, 16384, 65535)
RAGGED_TOO_LONG = 65600      # above the declared maximum (65,535): INT32_MIN, the kRagged claim path


def ragged_pages(O):
    """two pages of every length (distributions 0..5 in turn and one of random bytes), the too-long
    page in the middle of the batch"""
    big = [O.pagegen(1, 65536, seed=BENCH_SEED + 1, first=3 * d, dist=d)[0] for d in range(6)]
    rng = np.random.default_rng(11)
    pages = []
    for k, n in enumerate(RAGGED_LENGTHS * 2):
        pages.append(big[k % 6][:n].tobytes())
        if k == 3:
            pages.append(big[1][:65536].tobytes() + bytes(RAGGED_TOO_LONG - 65536))
    pages.append(rng.integers(0, 256, 12352, dtype=np.uint8).tobytes())
    return pages


CAP_CASES = ("lit270_part1", "zero_page", "random_part1")


def lz4_bound(n):
    return n + n // 255 + 16


def _sha(b):
    return np.frombuffer(hashlib.sha256(b).digest(), np.uint8)


def device_ragged(tc, pages, caps, max_src_length):
    """compress_ragged over a checked layout (64 guard bytes around every slot); (results, streams)"""
    import batch_contract_cases as C
    lay = BL.build(pages, caps, 0, C.dst_shifts(len(pages)), "zero")
    rv, out, src = C.device_compress(tc, lay, LZ4, max_src_length=max_src_length)
    BL.check(out, src, lay)   # no byte outside a slot, the guards after dst_cap included
    return rv, BL.outputs(out, rv, lay)


def run_all(tc, O, dev):
    """Compresses every batch with the default encoder.  Returns {group: (pages, results, streams)}
    with pages as byte strings, results as ints and streams as byte strings (empty where the result
    is not positive)."""
    import torch
    res = {}

    def uniform(name, arr):
        comp, clen = tc.compress_pages(torch.from_numpy(np.ascontiguousarray(arr)).to(dev))
        torch.cuda.synchronize()
        comp, clen = comp.cpu().numpy(), clen.cpu().numpy()
        res[name] = ([p.tobytes() for p in arr], [int(x) for x in clen],
                     [comp[i, :max(int(clen[i]), 0)].tobytes() for i in range(len(arr))])

    for name, arr in bench_groups(O).items():
        uniform(name, arr)
    jc = joint_cases()
    uniform("joint", np.stack([p for _, p, _ in jc]))
    pages = ragged_pages(O)
    rv, streams = device_ragged(tc, pages, [lz4_bound(len(p)) for p in pages], 65535)
    res["ragged"] = (pages, [int(x) for x in rv], streams)
    # capacity: the stream's own length, then one byte less
    names = [n for n, _, _ in jc]
    cp, caps = [], []
    for n in CAP_CASES:
        i = names.index(n)
        for d in (0, 1):
            cp.append(jc[i][1].tobytes())
            caps.append(res["joint"][1][i] - d)
    rv, streams = device_ragged(tc, cp, caps, PLEN)
    res["cap"] = (cp, [int(x) for x in rv], streams)
    return res


def digests(res):
    """{group_sha: (n, 32) uint8, group_len: (n,) int32} of run_all's result"""
    out = {}
    for name, (_, rv, streams) in res.items():
        out[name + "_sha"] = np.stack([_sha(s) for s in streams])
        out[name + "_len"] = np.array(rv, np.int64).astype(np.int32)
    return out
