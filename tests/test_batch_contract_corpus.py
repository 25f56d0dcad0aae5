"""The decode corpora of the batch-contract tests (batch_contract_cases.py) exercise what they are
meant to: judged by the oracle alone, each holds enough successes, failures, short outputs,
capacity failures and truncations that test_gpu_batch_contract.py cannot pass on a corpus that
decides nothing.  No GPU: the device-encoded zstd frames the GPU test adds are not part of this
(the golden zstd frames are)."""
import pytest

import batch_contract_cases as C
import batch_layout as BL

CODECS = [C.LZ4, C.ZLIB, C.ZSTD]
IDS = [C.NAMES[c] for c in CODECS]


def _stats(codec, cases, want):
    n = len(cases)
    ok = [i for i in range(n) if want[i][0] >= 0]
    short = [i for i in ok if want[i][0] < cases[i].cap]
    # a capacity failure: a valid stream that fails only because its page does not fit
    capfail = [i for i in range(n) if cases[i].kind == "valid" and cases[i].page is not None
               and cases[i].cap < cases[i].page and want[i][0] < 0]
    trunc = [i for i in range(n) if cases[i].trunc]
    return dict(n=n, ok=len(ok), fail=n - len(ok), short=len(short), capfail=len(capfail), trunc=len(trunc))


RUNS = [(c, w) for c in CODECS for w in (None, 32768, 65536) if w != 65536 or c == C.LZ4]


@pytest.mark.parametrize("codec,wide", RUNS, ids=[f"{C.NAMES[c]}-small" + (f"+{w}" if w else "") for c, w in RUNS])
def test_decode_corpus_decides_something(codec, wide):
    """The corpus of (a) as each kernel path runs it: the small batches alone, or with a wide one
    (65,536: the LZ4 wave, lane-chunked and serial decoders only)."""
    cases, want = [], []
    for which in ["small"] + ([wide] if wide else []):
        cases += C.corpus(codec, which)
        want += C.expected(codec, which)
    s = _stats(codec, cases, want)
    print(C.NAMES[codec], s)
    assert s["ok"] >= 0.30 * s["n"], s
    assert s["fail"] >= 0.30 * s["n"], s
    assert s["short"] >= 1 and s["capfail"] >= 1, s
    assert s["trunc"] >= 0.25 * s["n"], s
    assert sum(c.kind in ("flip", "store", "trunc") for c in C.corpus(codec, "small")) == 200
    for c in cases:
        assert 0 <= c.cap <= 65536 and len(c.stream) < 90000


@pytest.mark.parametrize("codec", CODECS, ids=IDS)
def test_isolation_corpus_decides_something(codec):
    """The batch of (b): the small corpus cut down so that truncations are a quarter of it."""
    cases, want = C.corpus(codec, "small"), C.expected(codec, "small")
    idx = C.isolation_subset(cases)
    assert len(idx) <= C.MAX_BATCH and idx == sorted(set(idx))
    s = _stats(codec, [cases[i] for i in idx], [want[i] for i in idx])
    print(C.NAMES[codec], s)
    assert s["ok"] >= 0.30 * s["n"], s
    assert s["fail"] >= 0.30 * s["n"], s
    assert s["short"] >= 1 and s["capfail"] >= 1, s
    assert s["trunc"] >= 0.25 * s["n"], s


@pytest.mark.parametrize("codec", CODECS, ids=IDS)
def test_corpus_is_reproducible_and_lays_out(codec):
    """Seeded: the same cases every time; and a batch of them fits the checked layout."""
    C.corpus.cache_clear()
    a = C.corpus(codec, "small")
    C.corpus.cache_clear()
    assert C.corpus(codec, "small") == a
    part = a[:C.MAX_BATCH]
    lay = BL.build([c.stream for c in part], [c.cap for c in part], C.src_shifts(len(part)), C.dst_shifts(len(part)),
                   ("random", 1))
    BL.check(lay.out.copy(), lay.src.copy(), lay)
    assert {int(x) % 16 for x in lay.dst_offsets} == set(range(16))
    assert {int(x) % 16 for x in lay.src_offsets} == set(range(16))


def test_compress_pages_cover_the_issue():
    pages = C.compress_pages()
    lens = sorted({len(p) for p in pages})
    assert lens == [0, 1, 13, 64, 777, 1000, 4096, 16384]
    assert sum(1 for p in pages if len(p) == 16384) == 8 and 8 * len(pages) <= C.MAX_BATCH
    assert any(p == bytes(len(p)) and len(p) == 16384 for p in pages)
    assert C.limited_caps(100, 120) == [99, 100, 101, 107, 50, 1, 0, 119]
