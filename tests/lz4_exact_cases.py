"""Inputs shared by the exact LZ4 encoder's tests (test_lz4_exact_emul.py on the CPU,
test_gpu_lz4_exact.py on the GPU): the page kinds, the ragged small pages and the limited-output
capacities.  Expected bytes always come from oracle.lz4_compress (LZ4_compress_default restated)."""
import numpy as np

PAGE_LENS = (4096, 16384, 65535)
KINDS = ["dist0", "dist1", "dist2", "dist3", "dist4", "dist5", "zero", "period1", "period2", "period3", "period4",
         "period5", "period7", "random", "literal_runs", "long_match"]
LONG_MATCH = 15 + 4 * 255 + 300   # a match-length field of more than four 255 bytes


def literal_run_pages(n, plen, seed):
    """Pages mixing random stretches (long literal runs) with repeated records (matches), in
    several proportions (the generator of test_gpu_lz4.py's long-literal-run test)."""
    rng = np.random.default_rng(seed)
    pages = np.zeros((n, plen), np.uint8)
    for i in range(n):
        pos = 0
        rec = rng.integers(0, 256, 24, dtype=np.uint8)
        while pos < plen:
            kind = rng.integers(0, 4)
            m = int(rng.integers(1, [3000, 400, 60, 900][kind]))
            m = min(m, plen - pos)
            if kind in (0, 1):
                pages[i, pos:pos + m] = rng.integers(0, 256, m, dtype=np.uint8)
            else:
                pages[i, pos:pos + m] = np.resize(rec, m)
            pos += m
    return pages


def kind_pages(O, kind, plen, n=8):
    """(n, plen) uint8 pages of one kind."""
    rng = np.random.default_rng(plen * 31 + KINDS.index(kind))
    if kind.startswith("dist"):
        gen = (plen + 4095) // 4096 * 4096
        return np.ascontiguousarray(O.pagegen(n, gen, seed=606 + plen, first=plen, dist=int(kind[4:]))[:, :plen])
    if kind == "zero":
        return np.zeros((n, plen), np.uint8)
    if kind.startswith("period"):
        per = int(kind[6:])
        return np.stack([np.resize(rng.integers(0, 256, per, dtype=np.uint8), plen) for _ in range(n)])
    if kind == "random":
        return rng.integers(0, 256, (n, plen), dtype=np.uint8)
    if kind == "literal_runs":
        return literal_run_pages(n, plen, plen + 7)
    assert kind == "long_match"
    pages = rng.integers(0, 256, (n, plen), dtype=np.uint8)
    for i in range(n):
        m = LONG_MATCH + 1 + 37 * i          # one match longer than LONG_MATCH bytes
        a = 100 + 11 * i                     # source of the copy
        d = a + m + 40 + i                   # its destination: behind the source, no overlap
        pages[i, d:d + m] = pages[i, a:a + m]
    return pages


RAGGED_LENS = list(range(1, 81)) + [127, 128, 129, 255, 256, 4095]


def ragged_pages(symbols, seed=1):
    """One page per length of RAGGED_LENS over an alphabet of `symbols` byte values."""
    rng = np.random.default_rng(seed * 1000 + symbols)
    alphabet = rng.choice(256, symbols, replace=False).astype(np.uint8)
    return [alphabet[rng.integers(0, symbols, n)].tobytes() for n in RAGGED_LENS]


def limited_pages(O):
    """(compressible, incompressible) 16 KiB pages of the limited-output tests."""
    comp = O.pagegen(1, 16384, seed=4242, first=5, dist=0)[0].tobytes()
    rnd = np.random.default_rng(99).integers(0, 256, 16384, dtype=np.uint8).tobytes()
    return comp, rnd


def limited_caps(O, page, seed):
    """The capacities of the limited-output tests for one page."""
    full = len(O.lz4_compress(page))
    bound = O.lz4_bound(len(page))
    caps = [1, 2, 12, 13, full - 1, full, full + 1, bound - 1, bound]
    caps += [int(c) for c in np.random.default_rng(seed).integers(0, full + 16, 32)]
    return caps
