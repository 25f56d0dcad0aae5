"""Inputs shared by the large-page LZ4 tests (test_lz4_large_emul.py on the CPU through the
emulator, test_gpu_lz4_large.py on the kernels): the page lengths, hand-made streams that put a
ring wrap under every kind of copy, and malformed streams.  Expected results always come from the
oracle (oracle.lz4_compress switches to byU32 at 65,547 bytes as LZ4 1.7.5 does; lz4_decompress is
LZ4_decompress_safe restated)."""
import numpy as np

from lz4_exact_cases import KINDS, kind_pages

MAX_PAGE = 4 << 20                                    # TYCHE_LZ4_MAX_PAGE
LENS = (65536, 65547, 70001, 131072, 196613, 1048579)
FULL_KINDS = ("zero", "random", "dist0")              # the kinds also run at MAX_PAGE
RING = 128 << 10                                      # the kernels' LDS ring: copies that cross a multiple wrap


def page_of(O, kind, plen, i=0, n=2):
    """Page i of kind_pages(O, kind, plen, n) as bytes."""
    return kind_pages(O, kind, plen, n)[i].tobytes()


def _length_bytes(n):
    """The bytes after a token for a length field of n >= 15."""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def sequence(lits: bytes, off: int, mlen: int) -> bytes:
    """One LZ4 sequence: literals, then a match of mlen >= 4 bytes at offset off."""
    ll, mc = len(lits), mlen - 4
    out = bytes([(min(ll, 15) << 4) | min(mc, 15)])
    if ll >= 15:
        out += _length_bytes(ll)
    out += lits + bytes([off & 255, off >> 8])
    if mc >= 15:
        out += _length_bytes(mc)
    return out


def last_literals(lits: bytes) -> bytes:
    ll = len(lits)
    return bytes([min(ll, 15) << 4]) + (_length_bytes(ll) if ll >= 15 else b"") + lits


def crafted_streams():
    """[(name, stream, decoded size)]: valid blocks no encoder of ours would emit."""
    rng = np.random.default_rng(4711)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    tail = last_literals(rnd(12))
    out = [("lit70000_off65535", sequence(rnd(70000), 65535, 1000) + tail, 70000 + 1000 + 12),
           ("off1_len300000", sequence(b"x", 1, 300000) + tail, 1 + 300000 + 12),
           # the match starts 72 bytes before the ring wraps, its source 65,535 bytes back
           ("off65535_across_wrap", sequence(rnd(RING - 72), 65535, 500) + tail, RING - 72 + 500 + 12),
           # two sequences: the second literal run and match both cross the wrap
           ("lits_across_wrap", sequence(rnd(RING - 5000), 4000, 4900) + sequence(rnd(300), 65000, 70000) + tail,
            RING - 5000 + 4900 + 300 + 70000 + 12)]
    for per in range(2, 8):
        out.append((f"period{per}", sequence(rnd(per), per, 200000 + per) + tail, per + 200000 + per + 12))
    return out


def walk(stream: bytes):
    """[(token position, literal length, offset position)] of a valid block's sequences (the
    last, literal-only one has offset position None)."""
    seqs, ip, n = [], 0, len(stream)
    while ip < n:
        tp = ip
        token = stream[ip]
        ip += 1
        ll = token >> 4
        if ll == 15:
            while True:
                s = stream[ip]
                ip += 1
                ll += s
                if s != 255:
                    break
        ip += ll
        if ip >= n:
            seqs.append((tp, ll, None))
            break
        seqs.append((tp, ll, ip))
        ip += 2
        if token & 15 == 15:
            while stream[ip] == 255:
                ip += 1
            ip += 1
    return seqs


def malformed_sources(O):
    """About 20 (name, valid stream, decoded size) to damage: the oracle's streams of pages of
    several kinds and lengths, and the crafted ones."""
    out = []
    for kind, plen in (("dist0", 65536), ("dist1", 65547), ("dist3", 70001), ("dist5", 131072), ("zero", 70001),
                       ("zero", 196613), ("period1", 131072), ("period3", 65547), ("period7", 196613),
                       ("random", 65536), ("random", 70001), ("literal_runs", 131072), ("literal_runs", 196613),
                       ("long_match", 70001), ("dist2", 196613), ("dist4", 65547)):
        page = page_of(O, kind, plen)
        out.append((f"{kind}_{plen}", O.lz4_compress(page), plen))
    out += crafted_streams()[:4]
    return out


def cuts(stream: bytes, seed: int, n=40):
    """n seeded lengths at which to cut a stream (always some near both ends)."""
    rng = np.random.default_rng(seed)
    c = {1, 2, 3, len(stream) - 1, len(stream) - 2, len(stream) - 8, len(stream) - 16}
    while len(c) < n:
        c.add(int(rng.integers(1, len(stream))))
    return sorted(x for x in c if 0 < x < len(stream))


def patched_streams(O):
    """[(name, stream, capacity)]: an offset that reaches before the page start, and runs of length
    bytes made longer (a literal run, a match)."""
    out = []
    page = page_of(O, "dist0", 70001)
    s = O.lz4_compress(page)
    seqs = walk(s)
    tp, ll, offp = seqs[0]
    assert offp is not None
    out.append(("offset_before_start", s[:offp] + b"\xff\xff" + s[offp + 2:], 70001))
    tp, ll, offp = seqs[len(seqs) // 2]
    out.append(("offset_zero_mid", s[:offp] + b"\x00\x00" + s[offp + 2:], 70001))
    z = O.lz4_compress(bytes(196613))                 # token, one literal, offset 1, a long run of 255s
    i = z.index(b"\xff\xff\xff")
    out.append(("match_length_longer", z[:i] + b"\xff" * 10 + z[i:], 196613))
    out.append(("match_length_shorter", z[:i] + z[i + 10:], 196613))
    r = O.lz4_compress(page_of(O, "random", 70001))   # one literal run: its length bytes start at 1
    out.append(("literal_length_longer", r[:1] + b"\xff" * 3 + r[1:], 70001))
    out.append(("literal_length_shorter", r[:1] + r[3:], 70001))
    return out
