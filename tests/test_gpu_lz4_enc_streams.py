"""The default LZ4 encoder's streams, byte for byte: every batch of lz4_enc_stream_cases.py is
compressed again and the sha256 and length of every stream compared with
tests/golden/lz4_enc_streams.npz (tools/gen_lz4_enc_streams_golden.py recorded it from the encoder
as it stood before its control code was reshaped), and every stream is decoded by the oracle.
The batches are compressed once for the module."""
import numpy as np
import pytest
import torch

import lz4_enc_stream_cases as S
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def run(oracle_mod):
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return S.run_all(codec, oracle_mod, DEV)


@pytest.fixture(scope="module")
def golden():
    return load_golden("lz4_enc_streams.npz")


def check_digests(run, golden, group):
    got = S.digests({group: run[group]})
    want_len, want_sha = golden[group + "_len"], golden[group + "_sha"]
    assert np.array_equal(got[group + "_len"], want_len), np.flatnonzero(got[group + "_len"] != want_len)[:10]
    bad = np.flatnonzero((got[group + "_sha"] != want_sha).any(axis=1))
    assert bad.size == 0, f"{group}: streams {bad[:10]} differ from the recorded ones"


def check_decodes(run, O, group):
    pages, rv, streams = run[group]
    for i, (p, r, s) in enumerate(zip(pages, rv, streams)):
        if r <= 0:
            continue
        assert r == len(s)
        n, dec = O.lz4_decompress(s, len(p))
        assert n == len(p) and bytes(dec)[:n] == p, (group, i)


@pytest.mark.parametrize("plen", [8192, 16384])
@pytest.mark.parametrize("dist", range(6))
def test_bench_like_pages(run, golden, oracle_mod, plen, dist):
    group = f"bench_{plen}_d{dist}"
    assert min(run[group][1]) > 0
    check_digests(run, golden, group)
    check_decodes(run, oracle_mod, group)


def test_ragged_batch(run, golden, oracle_mod):
    pages, rv, _ = run["ragged"]
    long = [i for i, p in enumerate(pages) if len(p) > 65535]
    assert len(long) == 1 and rv[long[0]] == S.INT32_MIN, "the page above the declared maximum"
    assert sorted(set(len(p) for p in pages)) == sorted(S.RAGGED_LENGTHS + (S.RAGGED_TOO_LONG,))
    assert all(r > 0 for i, r in enumerate(rv) if i != long[0])
    check_digests(run, golden, "ragged")
    check_decodes(run, oracle_mod, "ragged")


def test_joint_cases(run, golden, oracle_mod):
    assert min(run["joint"][1]) > 0
    check_digests(run, golden, "joint")
    check_decodes(run, oracle_mod, "joint")


def test_joint_cases_are_what_they_claim(run):
    """the crafted pages' joint sequences have the literal and match lengths they were built for;
    the pages without a match in a part carry one literal run across it"""
    _, _, streams = run["joint"]
    cases = S.joint_cases()
    for (name, _, checks), s in zip(cases, streams):
        for b, lit, ml in checks:
            q = S.joint_of(s, b)
            assert q is not None and q[1] == lit and q[3] == ml, (name, q, lit, ml)
    by = {c[0]: s for c, s in zip(cases, streams)}
    assert len(S.sequences(by["random_page"])) == 1
    for w in (1, 2):
        runs = [q for q in S.sequences(by[f"random_part{w}"]) if q[0] <= S.B[w] + 64 and q[2] >= S.B[w + 1] - 64]
        assert runs, f"no literal run spans part {w}"
    for name in ("zero_page", "period7"):   # matches run up to every boundary and go on from it
        for b in S.B[1:4]:
            q = S.joint_of(by[name], b)
            assert q is not None and q[1] == 0 and q[2] == b, (name, b, q)


def test_capacity(run, golden):
    """dst_cap = the stream's length: the length; one byte less: 0 (run_all checked the 64 guard
    bytes after every dst_cap)"""
    pages, rv, streams = run["cap"]
    assert len(pages) == 2 * len(S.CAP_CASES)
    names = [c[0] for c in S.joint_cases()]
    for k, name in enumerate(S.CAP_CASES):
        i = names.index(name)
        assert rv[2 * k] == run["joint"][1][i] and streams[2 * k] == run["joint"][2][i], name
        assert rv[2 * k + 1] == 0, name
    check_digests(run, golden, "cap")
