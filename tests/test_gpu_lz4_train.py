"""GPU tests of the LZ4 dictionary trainer (lz4_dict_train.hip through the C ABI): the device's
dictionary is, byte for byte, the host emulator's (tools/lz4_train_emul.cpp, which
test_lz4_train_emul.py holds to the numpy specification) for every batch layout; a trained handle
is an ordinary dictionary handle; the device encoder's totals with the trained dictionary are
pinned beside the heuristic dictionary's; and TYCHE_LZ4_DICT_AUTO trains and installs once, in a
child process, with every Buffer restoring bit-exactly."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lz4_dict_cases as DC
import lz4_train_cases as T
from conftest import ROOT
from test_lz4_train_emul import load_emul

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def tc():
    from tyche_amd import _lib, codec
    lib = _lib.load()
    assert lib.tyche_device_ready() == 1, _lib.last_error()
    return codec


@pytest.fixture(scope="module")
def emul():
    return load_emul()


@pytest.fixture(scope="module")
def ref(oracle_mod):
    return DC.ref_or_none(oracle_mod)


def _handle_bytes(lib, h) -> bytes:
    n = lib.tyche_lz4_dict_length(h)
    out = ctypes.create_string_buffer(max(n, 1))
    assert lib.tyche_lz4_dict_bytes(h, out, n) == n
    return out.raw[:n]


def _finish(h) -> bytes:
    """A training call's dictionary; b"" for the one refusal that is a result (nothing shared)."""
    from tyche_amd import _lib
    lib = _lib.load()
    if not h:
        assert "share no content" in _lib.last_error(), _lib.last_error()
        return b""
    try:
        return _handle_bytes(lib, h)
    finally:
        lib.tyche_lz4_dict_destroy(h)


def train_offsets(pages, D: int, misalign: int = 0, gap: int = 0, declare_max: bool = True) -> bytes:
    """tyche_lz4_dict_train_batch over src_offsets / src_lengths."""
    from tyche_amd import _lib
    buf, offs, lens = T.pack(pages, misalign, gap)
    d_buf = torch.from_numpy(buf).to(DEV)
    d_offs = torch.from_numpy(offs.astype(np.int64)).to(DEV)
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    b = _lib.Batch(count=len(pages), src=d_buf.data_ptr(), src_offsets=d_offs.data_ptr(), src_lengths=d_lens.data_ptr(),
                   max_src_length=int(lens.max()) if declare_max else 0)
    h = _lib.load().tyche_lz4_dict_train_batch(ctypes.byref(b), D, torch.cuda.current_stream(DEV).cuda_stream)
    return _finish(h)


def train_stride(pages, D: int, pad: int = 0, misalign: int = 0) -> bytes:
    """The same over src_stride / src_length: equal pages, `pad` bytes between the rows."""
    from tyche_amd import _lib
    L = len(pages[0])
    assert all(len(p) == L for p in pages)
    host = np.zeros(misalign + len(pages) * (L + pad) + 1, np.uint8)
    for i, p in enumerate(pages):
        host[misalign + i * (L + pad):misalign + i * (L + pad) + L] = np.frombuffer(p, np.uint8)
    d = torch.from_numpy(host).to(DEV)
    b = _lib.Batch(count=len(pages), src=d.data_ptr() + misalign, src_stride=L + pad, src_length=L)
    h = _lib.load().tyche_lz4_dict_train_batch(ctypes.byref(b), D, torch.cuda.current_stream(DEV).cuda_stream)
    return _finish(h)


# ---------------------------------------------------------------- byte identity with the emulator
def test_small_cases(tc, emul, oracle_mod):
    for name, pages, D in T.small_cases(oracle_mod):
        want = emul(pages, D)
        assert train_offsets(pages, D) == want, name
    name, pages, D = [c for c in T.small_cases(oracle_mod) if c[0] == "ragged"][0]
    assert train_offsets(pages, D, declare_max=False) == emul(pages, D)      # an undeclared maximum means 65535


@pytest.mark.parametrize("dist", [0, 2, 4])
def test_big_cases(tc, emul, oracle_mod, dist):
    """64 x 16 KiB at D = 128, 4,096 and 32,768 (1, 32 and 256 rounds)."""
    pages = T.big_pages(oracle_mod, dist)
    for D in T.BIG_DS:
        got = train_stride(pages, D)
        assert got == emul(pages, D), (dist, D, len(got))


def test_layouts_and_misalignment(tc, emul, oracle_mod):
    """A stride with room between the rows, offsets with gaps, and the source base off by 1 and by
    15 bytes: the bytes depend on the pages alone."""
    pages = T.gen_pages(oracle_mod, 16, 4096, 0, 500)
    want = emul(pages, 2048)
    assert len(want) == 2048
    assert train_stride(pages, 2048) == want
    assert train_stride(pages, 2048, pad=24) == want
    assert train_offsets(pages, 2048, gap=5) == want
    for mis in (1, 15):
        assert train_stride(pages, 2048, pad=3, misalign=mis) == want, mis
        assert train_offsets(pages, 2048, misalign=mis) == want, mis
    name, ragged, D = [c for c in T.small_cases(oracle_mod) if c[0] == "ragged"][0]
    for mis in (1, 15):
        assert train_offsets(ragged, D, misalign=mis, gap=1) == emul(ragged, D), mis


def test_more_pages_than_workgroups(tc, emul, oracle_mod):
    """1,024 x 8 KiB of dist 0: pages are claimed from the counter, and most are passed over in
    most rounds."""
    pages = T.gen_pages(oracle_mod, 1024, 8192, 0, 70000)
    got = train_stride(pages, 4096)
    assert got == emul(pages, 4096) and len(got) == 4096


def test_two_runs_and_every_entry_point_agree(tc, emul, oracle_mod):
    from tyche_amd import _lib
    lib = _lib.load()
    pages = T.gen_pages(oracle_mod, 64, 8192, 1, 4000)
    want = emul(pages, 4096)
    assert train_stride(pages, 4096) == want and train_stride(pages, 4096) == want
    keep, srcs, lens = _host(pages)
    assert _finish(lib.tyche_lz4_dict_train_host(len(pages), srcs, lens, 4096)) == want
    d = tc.Lz4Dict.train(pages, 4096)
    assert d.data == want and len(d) == len(want)
    d.close()
    rows = torch.from_numpy(np.stack([np.frombuffer(p, np.uint8) for p in pages])).to(DEV)
    d = tc.Lz4Dict.train(rows, 4096)
    assert d.data == want
    d.close()
    name, differ, D = [c for c in T.small_cases(oracle_mod) if c[0] == "two-128-differ"][0]
    assert emul(differ, D) == b""
    with pytest.raises(ValueError, match="share no content"):
        tc.Lz4Dict.train(differ, D)
    name, ragged, D = [c for c in T.small_cases(oracle_mod) if c[0] == "ragged"][0]
    keep, srcs, lens = _host(ragged)
    assert _finish(lib.tyche_lz4_dict_train_host(len(ragged), srcs, lens, D)) == emul(ragged, D)


def _host(pages):
    """(the buffers, kept alive by the caller; their addresses; their lengths) for the host calls."""
    keep = [ctypes.create_string_buffer(p, max(len(p), 1)) for p in pages]
    srcs = (ctypes.c_void_p * len(pages))(*[ctypes.addressof(k) for k in keep])
    lens = (ctypes.c_uint32 * len(pages))(*[len(p) for p in pages])
    return keep, srcs, lens


def test_device_rules(tc, oracle_mod):
    """The two refusals only the device can decide: a page above the declared maximum, and
    src_lengths that add up to more than TYCHE_LZ4_TRAIN_MAX_BYTES."""
    from tyche_amd import _lib
    lib = _lib.load()
    pages = T.gen_pages(oracle_mod, 16, 4096, 0, 500)
    buf, offs, lens = T.pack(pages)
    d_buf = torch.from_numpy(buf).to(DEV)
    d_offs = torch.from_numpy(offs.astype(np.int64)).to(DEV)
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    b = _lib.Batch(count=16, src=d_buf.data_ptr(), src_offsets=d_offs.data_ptr(), src_lengths=d_lens.data_ptr(),
                   max_src_length=4095)
    assert not lib.tyche_lz4_dict_train_batch(ctypes.byref(b), 1024, None)
    assert "declared maximum" in _lib.last_error() and "4095" in _lib.last_error()
    # 1,100 "pages" of 65,535 bytes, all at offset 0 of one buffer: 72 MB of samples in 64 KiB of memory
    n = 1100
    one = torch.zeros(65536, dtype=torch.uint8, device=DEV)
    zoffs = torch.zeros(n, dtype=torch.int64, device=DEV)
    zlens = torch.full((n,), 65535, dtype=torch.int32, device=DEV)
    b = _lib.Batch(count=n, src=one.data_ptr(), src_offsets=zoffs.data_ptr(), src_lengths=zlens.data_ptr(), max_src_length=65535)
    assert not lib.tyche_lz4_dict_train_batch(ctypes.byref(b), 1024, None)
    assert "TYCHE_LZ4_TRAIN_MAX_BYTES" in _lib.last_error() and str(n * 65535) in _lib.last_error()


# ---------------------------------------------------------------- use
def test_trained_handle_is_a_dictionary_handle(tc, oracle_mod, ref):
    """Pages compressed with the trained handle decode with it on the device, and with the
    reference's LZ4_decompress_safe_usingDict where that is built; some offset reaches into it."""
    O = oracle_mod
    L = 8192
    d = tc.Lz4Dict.train(T.ratio_training_pages(O, L, 0), 4096)
    assert len(d) == 4096
    _, evalp = T.ratio_eval(O, L, 0)
    pages = torch.from_numpy(np.stack([np.frombuffer(p, np.uint8) for p in evalp])).to(DEV)
    comp, clen = tc.compress_pages(pages, dictionary=d)
    out, rv = tc.decompress_pages(comp, clen, L, dictionary=d)
    torch.cuda.synchronize()
    assert bool((rv == L).all()) and torch.equal(out, pages)
    ch, lh = comp.cpu().numpy(), clen.cpu().numpy()
    streams = [ch[i, :lh[i]].tobytes() for i in range(len(evalp))]
    assert max(DC.max_reach(s) for s in streams) > 0
    if ref is not None:
        dic = d.data
        for s, p in zip(streams, evalp):
            assert ref.decompress(dic, s, L) == (L, p)
    d.close()


# device encoder, total bytes of the 48 evaluation pages with the trained 4 KiB dictionary, measured
# (profiles/lz4_train_ratio.jsonl); the bound is the measurement + 0.5 %
LZ4_TRAIN_PIN = {(8192, 0): 115486, (8192, 1): 116403, (8192, 2): 82466, (8192, 3): 2016, (8192, 4): 394848, (8192, 5): 176563,
                 (16384, 0): 232171, (16384, 1): 234114, (16384, 2): 160127, (16384, 3): 3552, (16384, 4): 789600,
                 (16384, 5): 349805}


@pytest.mark.parametrize("L,dist", T.ratio_keys(), ids=lambda v: str(v))
def test_device_encoder_ratio(tc, oracle_mod, L, dist):
    """The inputs of the CPU ratio conditions through the device encoder: the trained dictionary
    (trained on the device) beside the heuristic one, the capability the engine already had."""
    O = oracle_mod
    heur, evalp = T.ratio_eval(O, L, dist)
    pages = torch.from_numpy(np.stack([np.frombuffer(p, np.uint8) for p in evalp])).to(DEV)
    trained = tc.Lz4Dict.train(T.ratio_training_pages(O, L, dist), T.RATIO_D)
    totals = {}
    for name, d in (("trained", trained), ("heuristic", tc.Lz4Dict(heur))):
        comp, clen = tc.compress_pages(pages, dictionary=d)
        out, rv = tc.decompress_pages(comp, clen, L, dictionary=d)
        torch.cuda.synchronize()
        assert bool((rv == L).all()) and torch.equal(out, pages), name
        totals[name] = int(clen.sum())
        d.close()
    _, plain = tc.compress_pages(pages)
    torch.cuda.synchronize()
    print(json.dumps({"page": L, "dist": dist, "dict": T.RATIO_D, "device_trained": totals["trained"],
                      "device_heuristic": totals["heuristic"], "device_no_dict": int(plain.sum()),
                      "ratio": round(totals["trained"] / totals["heuristic"], 4)}))
    assert (L, dist) in LZ4_TRAIN_PIN, "no pinned measurement for this case"
    assert totals["trained"] <= LZ4_TRAIN_PIN[(L, dist)] * 1.005, (totals, LZ4_TRAIN_PIN[(L, dist)])


# ---------------------------------------------------------------- TYCHE_LZ4_DICT_AUTO
_AUTO_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from oracle import oracle as O
from tyche_amd import _lib, buffer as B
lib = _lib.load()
pages = [r.tobytes() for r in O.pagegen(96, 8192, seed=4242, first=31000, dist=0)]
bufs, streams = [], []
for k in range(3):
    assert (lib.tyche_lz4_current_dict() is None) == (k < 2), k      # installed by the call that completed the sample
    batch = [B.new_buffer(p, id=32 * k + i) for i, p in enumerate(pages[32 * k:32 * k + 32])]
    rc, st, ptrs = B.buffers_compress(batch, 1, 1)
    assert rc == 0 and st == [0] * 32, (rc, st, _lib.last_error())
    for b, p in zip(batch, ptrs):
        B.swap_data(b, p)
    bufs += batch
    streams += [B.buffer_bytes(b) for b in batch]
cur = lib.tyche_lz4_current_dict()
assert cur
n = lib.tyche_lz4_dict_length(cur)
out = ctypes.create_string_buffer(n)
lib.tyche_lz4_dict_bytes(cur, out, n)
keep = [ctypes.create_string_buffer(p, len(p)) for p in pages[:64]]
srcs = (ctypes.c_void_p * 64)(*[ctypes.addressof(x) for x in keep])
lens = (ctypes.c_uint32 * 64)(*[8192] * 64)
h = lib.tyche_lz4_dict_train_host(64, srcs, lens, 4096)
assert h, _lib.last_error()
m = lib.tyche_lz4_dict_length(h)
mine = ctypes.create_string_buffer(m)
lib.tyche_lz4_dict_bytes(h, mine, m)
assert out.raw[:n] == mine.raw[:m] and n == 4096, (n, m)
rc, st = B.buffers_decompress(bufs, 1)
assert rc == 0 and st == [0] * 96, (rc, st)
assert [B.buffer_bytes(b) for b in bufs] == pages                     # the 64 pre-install ones included
open(sys.argv[2], "wb").write(b"".join(len(s).to_bytes(4, "little") + s for s in streams))
print("child ok")
"""

_PLAIN_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from oracle import oracle as O
from tyche_amd import _lib, buffer as B
pages = [r.tobytes() for r in O.pagegen(96, 8192, seed=4242, first=31000, dist=0)]
streams = []
for k in range(3):
    batch = [B.new_buffer(p, id=32 * k + i) for i, p in enumerate(pages[32 * k:32 * k + 32])]
    rc, st, ptrs = B.buffers_compress(batch, 1, 1)
    assert rc == 0 and st == [0] * 32
    for b, p in zip(batch, ptrs):
        B.swap_data(b, p)
    streams += [B.buffer_bytes(b) for b in batch]
open(sys.argv[2], "wb").write(b"".join(len(s).to_bytes(4, "little") + s for s in streams))
print("child ok")
"""


def _read_streams(path):
    raw, out, at = open(path, "rb").read(), [], 0
    while at < len(raw):
        n = int.from_bytes(raw[at:at + 4], "little")
        out.append(raw[at + 4:at + 4 + n])
        at += 4 + n
    return out


def test_auto_mode_in_a_child_process(tmp_path):
    """TYCHE_LZ4_DICT_AUTO=4096 with 64 sample pages, three tyche_buffers_compress batches of 32 x
    8 KiB dist-0 Buffers: the first two are the plain encoder's streams; then the process-wide
    dictionary is what tyche_lz4_dict_train_host makes of those 64 pages; the third batch is smaller
    than its plain encoding; all 96 Buffers restore bit-exactly."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("TYCHE_LZ4_DICT", "TYCHE_LZ4_DICT_AUTO", "TYCHE_LZ4_DICT_AUTO_PAGES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", _PLAIN_CHILD, ROOT, str(tmp_path / "plain.bin")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr
    env.update(TYCHE_LZ4_DICT_AUTO="4096", TYCHE_LZ4_DICT_AUTO_PAGES="64")
    p = subprocess.run([sys.executable, "-c", _AUTO_CHILD, ROOT, str(tmp_path / "auto.bin")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr
    plain, auto = _read_streams(tmp_path / "plain.bin"), _read_streams(tmp_path / "auto.bin")
    assert len(plain) == len(auto) == 96
    assert auto[:64] == plain[:64]
    a, b = sum(map(len, auto[64:])), sum(map(len, plain[64:]))
    print(f"third batch: {a} bytes with the trained dictionary, {b} plain")
    assert a < b
    assert max(DC.max_reach(s) for s in auto[64:]) > 0
