"""Inputs of the batch-contract tests (test_gpu_batch_contract.py on the kernels,
test_batch_contract_corpus.py on the CPU): decode corpora per codec with the oracle's verdicts, the
pages of the limited-output compress tests, and the two helpers that run a checked layout
(batch_layout.py) on the device.  The corpora need no GPU; expected values always come from the
oracle, never from the kernels."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import batch_layout as BL
from conftest import load_golden, unpack

LZ4, ZLIB, ZSTD = 1, 2, 3
NAMES = {LZ4: "lz4", ZLIB: "zlib", ZSTD: "zstd"}
INT32_MIN = -(2 ** 31)

SIZES = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 16384)   # around the kernels' granules
SMALL_CAP = 16484     # capacities of a "small" batch: the sizes above + 13, and the golden malformed sets' largest
MAX_BATCH = 400

# kind: golden | malformed | valid | flip | store | trunc.  exact: the stream's bytes were not
# flipped, so an LZ4 success has defined bytes (an offset-0 match leaves them undefined).
# page: the decoded size the stream was made for (or None when it is unknown).  trunc: the stream
# is a proper prefix of a valid one (kind trunc, and those of the golden malformed sets that are)
Case = namedtuple("Case", "stream cap kind exact page trunc", defaults=(False,))


def oracle():
    import os
    from oracle import oracle as O
    if not os.path.exists(O.ORACLE_SO):
        O.build(ref=False)
    return O


def src_shifts(n):
    return [(7 * i) % 16 for i in range(n)]


def dst_shifts(n):
    return [i % 16 for i in range(n)]


@functools.lru_cache(maxsize=None)
def _base_pages():
    O = oracle()
    return [O.pagegen(1, 65536, seed=606, first=10 * d, dist=d)[0] for d in range(6)]


def page(plen, k):
    """A page of plen bytes: pagegen distribution k % 6 (k % 12 >= 6: seeded random bytes)."""
    if k % 12 >= 6:
        return np.random.default_rng(1000 + k).integers(0, 256, plen, dtype=np.uint8).tobytes()
    return _base_pages()[k % 6][:plen].tobytes()


def six_caps(plen, rng, limit):
    """The capacities a page of plen bytes is decoded into: exact, one short, one and 13 over,
    a seeded short value and 0 (those the launch's limit allows)."""
    caps = [plen, plen - 1, plen + 1, plen + 13, int(rng.integers(0, plen)) if plen else 0, 0]
    return [c for c in caps if 0 <= c <= limit]


def _encode(codec, data, k):
    """A valid stream of `data` from a CPU encoder (LZ4: the oracle's LZ4 1.7.5 restatement; zlib:
    Python's zlib, level and strategy chosen by k).  zstd has no CPU encoder here."""
    if codec == LZ4:
        return oracle().lz4_compress(data)
    assert codec == ZLIB
    level, strategy = [(1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                       (6, zlib.Z_FILTERED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE), (6, zlib.Z_FIXED),
                       (0, zlib.Z_DEFAULT_STRATEGY)][k % 8]
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


def _streams(g):
    comp, off, ln = g["comp"], g["comp_off"], g["comp_len"]   # (an .npz member is read anew on every access)
    return [unpack(comp, off, ln, i) for i in range(len(ln))]


@functools.lru_cache(maxsize=None)
def _golden_all(codec):
    name = NAMES[codec]
    valid = [(load_golden("kat_lorem.npz")[name].tobytes(), 4096)]
    if codec == LZ4:
        g = load_golden("lz4_generated.npz")
        valid += list(zip(_streams(g), [int(m[1]) for m in g["meta"]]))
        g = load_golden("lz4_sample.npz")
        valid += list(zip(_streams(g), [int(x) for x in g["size"]]))
    else:
        g = load_golden(f"{name}_streams.npz")
        valid += list(zip(_streams(g), [int(x) for x in g["size"]]))
    g = load_golden(f"{name}_malformed.npz")
    defined = [bool(x) for x in g["defined"]] if codec == LZ4 else [True] * len(g["cap"])
    whole = [v[0] for v in valid]
    bad = [Case(s, int(c), "malformed", d, None, any(len(s) < len(v) and v.startswith(s) for v in whole))
           for s, c, d in zip(_streams(g), g["cap"], defined)]
    return valid, bad


def _golden(codec, lo, hi):
    """(valid streams with their sizes, malformed cases) of tests/golden whose capacity is in (lo, hi]."""
    valid, bad = _golden_all(codec)
    return [v for v in valid if lo < v[1] <= hi], [c for c in bad if lo < c.cap <= hi]


def corruptions(bases, rng, n_flip, n_store, n_trunc, limit):
    """Seeded damage to valid (stream, page length) pairs: bit flips, byte stores, truncations.
    One case in seven gets a seeded short capacity."""
    out = []
    for kind, n in (("flip", n_flip), ("store", n_store), ("trunc", n_trunc)):
        for _ in range(n):
            s, plen = bases[int(rng.integers(len(bases)))]
            b = bytearray(s)
            if kind == "flip":
                for _ in range(int(rng.integers(1, 4))):
                    b[int(rng.integers(len(b)))] ^= 1 << int(rng.integers(8))
            elif kind == "store":
                i = int(rng.integers(len(b)))
                w = int(rng.choice([1, 3]))
                b[i:i + w] = rng.integers(0, 256, len(b[i:i + w]), dtype=np.uint8).tobytes()
            else:
                cut = int(rng.integers(1, len(b))) if len(b) > 1 else 0
                if rng.random() < 0.25:                      # near the end: the last sequence / checksum
                    cut = max(len(b) - int(rng.integers(1, 9)), 0)
                b = b[:cut]
            cap = plen if rng.random() < 6 / 7 or plen == 0 else int(rng.integers(0, plen))
            out.append(Case(bytes(b), min(cap, limit), kind, kind == "trunc", plen, kind == "trunc"))
    return out


def _valid_cases(streams, rng, limit):
    return [Case(s, c, "valid", True, plen) for s, plen in streams for c in six_caps(plen, rng, limit)]


@functools.lru_cache(maxsize=None)
def corpus(codec, which, extra=()):
    """The decode corpus of one codec.  which: "small" (capacities up to SMALL_CAP), 32768 or 65536
    (a "wide" batch: the golden streams above SMALL_CAP that fit, pages at the limit, their
    corruptions; 65536 holds a 65,535-byte page in a 65,536-byte capacity).  extra: more valid
    (stream, page length) pairs -- the device-encoded zstd frames, which need a GPU to make -- that
    get the six capacities each.  A tuple of Cases, any length: run it in batches of MAX_BATCH."""
    rng = np.random.default_rng(20170303 + 10 * codec + (0 if which == "small" else which))
    if which == "small":
        valid, bad = _golden(codec, -1, SMALL_CAP)
        cases = [Case(s, plen, "golden", True, plen) for s, plen in valid] + bad
        if codec == LZ4:      # one CPU encoder: every size as a pagegen page and as random bytes
            own = [(_encode(codec, page(plen, k + 6 * j), 0), plen) for j in range(2) for k, plen in enumerate(SIZES)]
        elif codec == ZLIB:   # every size at five of the level / strategy pairs
            own = [(_encode(codec, page(plen, k + j), k + j), plen) for j in range(5) for k, plen in enumerate(SIZES)]
        else:                 # no CPU encoder: two golden frames of every size the fixtures hold
            own = [v for size in sorted({v[1] for v in valid}) for v in [w for w in valid if w[1] == size][:2]]
        own += list(extra)
        cases += _valid_cases(own, rng, SMALL_CAP)
        # bases to damage: valid streams of at least 2 KiB of page, golden and own
        bases = [v for v in valid if v[1] >= 2048][::2] + [v for v in own if v[1] >= 4095]
        if codec != ZSTD:
            bases += [(_encode(codec, page(plen, k), k), plen) for k, plen in ((1, 8192), (2, 5000), (7, 3000), (4, 12000))]
        # about 200: mostly truncations, which with those of the golden set are a quarter of the corpus
        cases += corruptions(bases, rng, *((30, 20, 150) if codec == LZ4 else (20, 10, 170)), SMALL_CAP)
    else:
        limit = int(which)
        valid, _ = _golden(codec, SMALL_CAP, limit)
        cases = [Case(s, plen, "golden", True, plen) for s, plen in valid]
        top = min(limit, 65535)                               # the largest page: 65,535 bytes (byU16)
        own = valid[:3] if codec == ZSTD else [(_encode(codec, page(plen, k), k), plen)
                                               for k, plen in enumerate((top, top - 1, limit - 13, top, limit - 13), 5)]
        own += list(extra)
        cases += _valid_cases(own, rng, limit)
        cases += corruptions(valid[::3] + own, rng, 10, 6, 24, limit)
    return tuple(cases)


def decode_oracle(codec, case):
    O = oracle()
    f = {LZ4: O.lz4_decompress, ZLIB: O.zlib_uncompress, ZSTD: O.zstd_decompress}[codec]
    rv, out = f(case.stream, case.cap)
    return int(rv), bytes(out)[:max(int(rv), 0)]


@functools.lru_cache(maxsize=None)
def expected(codec, which, extra=()):
    """The oracle's (result, bytes) for every case of corpus(codec, which, extra), computed once."""
    return tuple(decode_oracle(codec, c) for c in corpus(codec, which, extra))


def isolation_subset(cases):
    """Indices of the cases the input-isolation test runs, MAX_BATCH at most: 120 truncations (30 %),
    every golden stream, and an even sample of the rest (valid streams at their six capacities,
    flips, stores, the malformed set)."""
    tr = [i for i, c in enumerate(cases) if c.kind == "trunc"][:120]
    gold = [i for i, c in enumerate(cases) if c.kind == "golden"]
    rest = [i for i, c in enumerate(cases) if c.kind not in ("trunc", "golden")]
    keep = MAX_BATCH - len(tr) - len(gold)
    pick = [rest[j * len(rest) // keep] for j in range(keep)] if len(rest) > keep else rest
    return sorted(tr + gold + pick)


def verdict_matches(codec, got, want):
    """LZ4 and zlib: the oracle's exact value.  zstd: its size on success, any negative value on
    failure (src/buffer.c:264-266 only tests ZSTD_isError)."""
    if codec == ZSTD and want < 0:
        return got < 0 and got != INT32_MIN
    return got == want


# ------------------------------------------------------------------ compress pages
@functools.lru_cache(maxsize=None)
def compress_pages():
    """The pages of the limited-output tests: pagegen distributions 0..5 at 4096 and 16384 bytes,
    random pages, all-zero pages, and pages of 0, 1, 13 and 64 bytes."""
    O = oracle()
    pages = []
    for plen in (4096, 16384):
        for d in range(6):
            pages.append(O.pagegen(1, plen, seed=99, first=plen + d, dist=d)[0].tobytes())
        pages.append(np.random.default_rng(plen).integers(0, 256, plen, dtype=np.uint8).tobytes())
        pages.append(bytes(plen))
    pages.append(np.random.default_rng(3).integers(0, 256, 1000, dtype=np.uint8).tobytes())
    pages.append(bytes(777))
    rng = np.random.default_rng(4)
    for n in (0, 1, 13, 64):
        pages.append((rng.integers(0, 3, n, dtype=np.uint8) * 40).tobytes())
    return tuple(pages)


def limited_caps(size, bound):
    """The capacities of the second run for a page whose stream took `size` bytes."""
    return [max(size - 1, 0), size, size + 1, size + 7, size // 2, 1, 0, bound - 1]


def restores(codec, stream, want, ref=True):
    """The stream decodes to the page through the oracle (and the reference decoder when built;
    zlib also through Python's)."""
    O = oracle()
    n = len(want)
    name = {LZ4: "lz4_decompress", ZLIB: "zlib_uncompress", ZSTD: "zstd_decompress"}[codec]
    r, dec = getattr(O, name)(stream, n)
    ok = r == n and bytes(dec)[:n] == want
    if ok and codec == ZLIB:
        ok = zlib.decompress(stream) == want
    if ok and ref and O.have_ref():
        r2, dec2 = getattr(O, "ref_" + name)(stream, n)
        ok = r2 == n and bytes(dec2)[:n] == want
    return ok


# ------------------------------------------------------------------ the device side
def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def device_decode(tc, lay, codec_id, max_src_length=None, max_capacity=None):
    """Runs a layout through tyche_decompress_batch; returns (results, output arena, source arena)
    as the device left them.  The declared maxima default to the batch's own."""
    import torch
    d_src, d_out = _to_dev(lay.src), _to_dev(lay.out)
    d_rv = torch.full((lay.count,), 0x5A5A5A5A, dtype=torch.int32, device=d_src.device)
    if max_src_length is None:
        max_src_length = max([int(x) for x in lay.src_lengths] + [1])
    if max_capacity is None:
        max_capacity = max([int(x) for x in lay.caps] + [0])
    tc.decompress_ragged(d_src, _to_dev(lay.src_offsets), _to_dev(lay.src_lengths), _to_dev(lay.caps), d_out,
                         _to_dev(lay.dst_offsets), d_rv, max_src_length=max_src_length, max_capacity=max_capacity,
                         compressor_id=codec_id)
    torch.cuda.synchronize()
    return d_rv.cpu().numpy(), d_out.cpu().numpy(), d_src.cpu().numpy()


def device_compress(tc, lay, codec_id, max_src_length=None):
    """Runs a layout through tyche_compress_batch (compress_ragged); same returns."""
    import torch
    d_src, d_out = _to_dev(lay.src), _to_dev(lay.out)
    d_rv = torch.full((lay.count,), 0x5A5A5A5A, dtype=torch.int32, device=d_src.device)
    if max_src_length is None:
        max_src_length = max([int(x) for x in lay.src_lengths] + [1])
    tc.compress_ragged(d_src, _to_dev(lay.src_offsets), _to_dev(lay.src_lengths), d_out, _to_dev(lay.dst_offsets),
                       _to_dev(lay.caps), d_rv, max_src_length=max_src_length, compressor_id=codec_id)
    torch.cuda.synchronize()
    return d_rv.cpu().numpy(), d_out.cpu().numpy(), d_src.cpu().numpy()


def checked_decode(tc, codec_id, streams, caps, shift=0):
    """What the suites' ragged_decode / ragged_inflate helpers do: streams at a 16-byte boundary +
    shift, 16-byte-aligned output slots, guards and source checked.  Returns (results, outputs)."""
    lay = BL.build(streams, caps, shift, 0, "zero")
    rv, out, src = device_decode(tc, lay, codec_id)
    BL.check(out, src, lay)
    return rv, BL.outputs(out, rv, lay)
