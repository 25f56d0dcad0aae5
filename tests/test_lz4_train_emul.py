"""CPU checks of the LZ4 dictionary trainer: the kernels' per-page and per-segment code
(tyche_amd/csrc/lz4_train_core.h) through the host emulator tools/lz4_train_emul.cpp against the
numpy restatement of the algorithm (lz4_train_cases.train_spec), byte for byte; the ratio
conditions the trained dictionary has to meet, judged by the reference encoder (oracle/_ref when
built, else its sizes in tests/golden/lz4_train.npz); and the parts of the C API that need no GPU
(every refusal with its message, the TYCHE_LZ4_DICT_AUTO environment rules).
test_gpu_lz4_train.py holds the kernels to the emulator's bytes.

LZ4_TRAIN_EMUL_RECORD=<file> records every emulator call of a run for the stand-alone sanitizer
program (tools/lz4_train_emul.cpp with -DLZ4_TRAIN_EMUL_MAIN), which replays them."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import lz4_dict_cases as DC
import lz4_train_cases as T
from conftest import ROOT

LIB = os.path.join(ROOT, "tools", "bin", "liblz4trainemul.so")
SRC = os.path.join(ROOT, "tools", "lz4_train_emul.cpp")
CORE = os.path.join(ROOT, "tyche_amd", "csrc", "lz4_train_core.h")
RECORD = os.environ.get("LZ4_TRAIN_EMUL_RECORD")
GUARD = 64


def load_emul():
    """The emulator as train(pages, D, misalign=0) -> bytes; built with g++ when missing or stale."""
    if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in (SRC, CORE)):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.lz4_train_emul.restype = ctypes.c_int
    lib.lz4_train_emul.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                   ctypes.c_void_p]

    def train(pages, D: int, misalign: int = 0) -> bytes:
        buf, offs, lens = T.pack(pages, misalign)
        out = np.full(GUARD + D + GUARD, 0xAB, np.uint8)
        r = lib.lz4_train_emul(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(pages), D, out.ctypes.data + GUARD)
        assert bool((out[:GUARD] == 0xAB).all()) and bool((out[GUARD + D:] == 0xAB).all()), "wrote outside the output"
        assert r >= 0 and r % T.S == 0 and r <= D, (r, D)
        dic = out[GUARD:GUARD + r].tobytes()
        if RECORD:
            with open(RECORD, "ab") as f:
                f.write(struct.pack("<IIi", len(pages), D, r) + lens.tobytes() + b"".join(pages) + dic)
        return dic
    return train


@pytest.fixture(scope="module")
def emul():
    return load_emul()


@pytest.fixture(scope="module")
def ref(oracle_mod):
    return DC.ref_or_none(oracle_mod)


@pytest.fixture(scope="module")
def golden():
    return T.Golden()


# ---------------------------------------------------------------- the emulator is the specification
def test_small_cases_equal_the_specification(emul, oracle_mod):
    """Pages of exactly 128 bytes; of 7, 8, 127 and 129 bytes (no key, one key, no candidate, one
    candidate); identical pages (the tie goes to page 0); all-zero pages (the run rule); one string
    at different misalignments; random pages; ragged lengths; the floor rule."""
    seen = {}
    for name, pages, D in T.small_cases(oracle_mod):
        want = T.train_spec(pages, D)
        for mis in (0, 1, 15):
            assert emul(pages, D, mis) == want, (name, mis)
        seen[name] = want
    a = T.small_cases(oracle_mod)[0][1][0]
    assert seen["two-128-equal"] == a and seen["two-128-equal-D4096"] == a     # one candidate, taken once
    assert seen["two-128-differ"] == b""                                       # nothing shared: no dictionary
    three = dict((n, p) for n, p, _ in T.small_cases(oracle_mod))["three-identical"]
    assert seen["three-identical"][-T.S:] in three[0] and len(seen["three-identical"]) <= 1024
    assert len(seen["all-zero"]) == T.S                                        # a run scores once, then nothing is left
    assert len(seen["dist0-4k-floor"]) == (1000 + 128) // T.S * T.S


@pytest.mark.parametrize("dist", range(6))
def test_big_cases_equal_the_specification(emul, oracle_mod, dist):
    """64 x 16 KiB of every distribution at D = 128, 4,096 and 32,768, and D = 4,095 + 128 (floor)."""
    pages = T.big_pages(oracle_mod, dist)
    for D in T.BIG_DS + ((T.FLOOR_D,) if dist == 0 else ()):
        want = T.train_spec(pages, D)
        assert emul(pages, D) == want, (dist, D)
        assert len(want) <= D // T.S * T.S


def test_random_pages_share_only_chance(emul, oracle_mod):
    """16 random pages: whatever the 2^20-slot table's chance collisions make of them is the
    specification's too, and the reference encoder gains nothing from it (ratio conditions, dist 4)."""
    pages = [p for n, p, _ in T.small_cases(oracle_mod) if n == "random-16"][0]
    assert emul(pages, 4096) == T.train_spec(pages, 4096)


# ---------------------------------------------------------------- ratio conditions
def _totals(O, ref, golden_row, trained, heur, evalp):
    """(plain, heuristic, trained) totals of the reference encoder: from oracle/_ref when it is built
    (and then equal to the golden file's), else the golden file's, which belong to the dictionary
    whose CRC it records."""
    if ref is not None:
        got = (T.judge(O, ref, None, evalp), T.judge(O, ref, heur, evalp), T.judge(O, ref, trained, evalp))
        assert got == tuple(golden_row[:3]), "tests/golden/lz4_train.npz is stale: run tools/gen_lz4_train_golden.py"
        return got
    assert DC.crc(trained) == golden_row[3], "the trained dictionary is not the one tests/golden/lz4_train.npz was recorded for"
    return tuple(golden_row[:3])


@pytest.mark.parametrize("L", T.RATIO_LS)
@pytest.mark.parametrize("dist", T.RATIO_DISTS)
def test_ratio_conditions(emul, oracle_mod, ref, golden, L, dist):
    """A 4 KiB dictionary trained on 64 pages, the 48 pages of lz4_dict_cases.ratio_inputs compressed
    by the reference encoder: at least 4 % below the heuristic dictionary (another page's first
    4 KiB) on dist 0 and 1, at most 1.01 x on dist 2 and 5, equal to no dictionary on dist 3 and 4."""
    O = oracle_mod
    trained = emul(T.ratio_training_pages(O, L, dist), T.RATIO_D)
    heur, evalp = T.ratio_eval(O, L, dist)
    plain, h, t = _totals(O, ref, golden.ratio[(L, dist)], trained, heur, evalp)
    print(f"dist {dist}, {L} B: plain {plain}, heuristic {h}, trained {t} ({t / h:.4f})")
    if dist in (0, 1):
        assert t <= 0.96 * h, (plain, h, t)
    elif dist in (2, 5):
        assert t <= 1.01 * h, (plain, h, t)
    else:
        assert t == plain, (plain, h, t)


@pytest.mark.parametrize("name,dl", T.sample_sets())
def test_sample_data_conditions(emul, oracle_mod, ref, golden, name, dl):
    """The reference's sample_data pages: trained on a set's first 5, its last 5 compressed by the
    reference encoder -- at most 1.04 x what the first page's prefix gives as dictionary."""
    O = oracle_mod
    prefix, train, evalp = T.sample_split(O, name, dl)
    trained = emul(train, dl)
    row = golden.sample[(name, dl)]
    if ref is not None:
        p, t = T.judge(O, ref, prefix, evalp), T.judge(O, ref, trained, evalp)
        assert (p, t) == tuple(row[:2]), "tests/golden/lz4_train.npz is stale: run tools/gen_lz4_train_golden.py"
    else:
        assert DC.crc(trained) == row[2]
        p, t = row[:2]
    print(f"{name} D={dl}: prefix {p}, trained {t} ({t / p:.4f})")
    assert t <= 1.04 * p, (p, t)


# ---------------------------------------------------------------- the C API without a GPU
@pytest.fixture(scope="module")
def lib():
    from tyche_amd import _lib
    return _lib.load()


def _host_args(pages):
    keep = [ctypes.create_string_buffer(p, max(len(p), 1)) for p in pages]
    srcs = (ctypes.c_void_p * max(len(pages), 1))(*[ctypes.addressof(k) for k in keep])
    lens = (ctypes.c_uint32 * max(len(pages), 1))(*[len(p) for p in pages])
    return keep, srcs, lens


def test_training_refusals_name_the_rule_and_the_numbers(lib):
    """Every NULL of tyche_lz4_dict_train_batch / _host that is decided before any device work."""
    from tyche_amd import _lib
    res = (ctypes.c_int32 * 1)()
    dummy = ctypes.addressof(res)                         # never dereferenced: the calls are refused first
    ok = _lib.Batch(count=4, src=dummy, src_stride=4096, src_length=4096)
    for bad in (0, 127, 32769, 1 << 20):
        assert not lib.tyche_lz4_dict_train_batch(ctypes.byref(ok), bad, None)
        msg = _lib.last_error()
        assert "dict_len" in msg and str(bad) in msg and "128" in msg and "32768" in msg, msg
    b = _lib.Batch(count=0, src=dummy, src_stride=4096, src_length=4096)
    assert not lib.tyche_lz4_dict_train_batch(ctypes.byref(b), 4096, None)
    assert "count is 0" in _lib.last_error()
    b = _lib.Batch(count=4, src=dummy, src_stride=65536, src_length=65536)
    assert not lib.tyche_lz4_dict_train_batch(ctypes.byref(b), 4096, None)
    assert "65536" in _lib.last_error() and "65535" in _lib.last_error()
    lens = (ctypes.c_uint32 * 4)(100, 100, 100, 100)
    b = _lib.Batch(count=4, src=dummy, src_stride=70000, src_lengths=ctypes.addressof(lens), max_src_length=70000)
    assert not lib.tyche_lz4_dict_train_batch(ctypes.byref(b), 4096, None)
    assert "70000" in _lib.last_error() and "65535" in _lib.last_error()
    n = T.TRAIN_MAX_BYTES // 16384 + 1
    b = _lib.Batch(count=n, src=dummy, src_stride=16384, src_length=16384)
    assert not lib.tyche_lz4_dict_train_batch(ctypes.byref(b), 4096, None)
    msg = _lib.last_error()
    assert "TYCHE_LZ4_TRAIN_MAX_BYTES" in msg and str(n * 16384) in msg and str(T.TRAIN_MAX_BYTES) in msg, msg
    b = _lib.Batch(count=_lib.LZ4_TRAIN_MAX_PAGES + 1, src=dummy, src_stride=8, src_length=8)
    assert not lib.tyche_lz4_dict_train_batch(ctypes.byref(b), 4096, None)
    assert "TYCHE_LZ4_TRAIN_MAX_PAGES" in _lib.last_error() and str(_lib.LZ4_TRAIN_MAX_PAGES + 1) in _lib.last_error()
    assert not lib.tyche_lz4_dict_train_batch(None, 4096, None)
    # the host form: the same rules, the page rule per page
    keep, srcs, lens = _host_args([bytes(200), bytes(300)])
    for bad in (127, 32769):
        assert not lib.tyche_lz4_dict_train_host(2, srcs, lens, bad)
        assert "dict_len" in _lib.last_error() and str(bad) in _lib.last_error()
    assert not lib.tyche_lz4_dict_train_host(0, srcs, lens, 4096)
    assert "count is 0" in _lib.last_error()
    keep, srcs, lens = _host_args([bytes(200), bytes(65536)])
    assert not lib.tyche_lz4_dict_train_host(2, srcs, lens, 4096)
    msg = _lib.last_error()
    assert "page 1" in msg and "65536" in msg and "65535" in msg, msg
    big = bytes(65535)
    m = T.TRAIN_MAX_BYTES // 65535 + 1
    keep = ctypes.create_string_buffer(big, len(big))
    srcs = (ctypes.c_void_p * m)(*[ctypes.addressof(keep)] * m)
    lens = (ctypes.c_uint32 * m)(*[65535] * m)
    assert not lib.tyche_lz4_dict_train_host(m, srcs, lens, 4096)
    msg = _lib.last_error()
    assert "TYCHE_LZ4_TRAIN_MAX_BYTES" in msg and str(m * 65535) in msg, msg


def test_dict_bytes_and_current_dict(lib):
    from tyche_amd import _lib
    data = bytes(range(256)) * 3 + b"xyz"
    h = lib.tyche_lz4_dict_create(data, len(data))
    out = ctypes.create_string_buffer(1000)
    assert lib.tyche_lz4_dict_bytes(h, out, 1000) == len(data) and out.raw[:len(data)] == data
    out = ctypes.create_string_buffer(b"\xAA" * 20, 20)
    assert lib.tyche_lz4_dict_bytes(h, out, 10) == len(data) and out.raw == data[:10] + b"\xAA" * 10
    assert lib.tyche_lz4_dict_bytes(h, None, 0) == len(data) and lib.tyche_lz4_dict_bytes(None, out, 10) == 0
    assert not lib.tyche_lz4_current_dict()
    assert lib.tyche_lz4_use_dict(h) == 0
    cur = lib.tyche_lz4_current_dict()
    try:
        assert cur == h
    finally:
        lib.tyche_lz4_dict_destroy(cur)
        lib.tyche_lz4_use_dict(None)
        lib.tyche_lz4_dict_destroy(h)
    assert not lib.tyche_lz4_current_dict()


_CHILD = ("import ctypes, numpy as np\n"
          "from tyche_amd import _lib\n"
          "lib = _lib.load()\n"
          "page = np.zeros(100, np.uint8); out = np.zeros(200, np.uint8); res = (ctypes.c_int32 * 1)()\n"
          "srcs = (ctypes.c_void_p * 1)(page.ctypes.data); dsts = (ctypes.c_void_p * 1)(out.ctypes.data)\n"
          "slen, dcap = (ctypes.c_uint32 * 1)(100), (ctypes.c_uint32 * 1)(200)\n")


def _child(code: str, **env):
    e = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("TYCHE_LZ4_DICT", "TYCHE_LZ4_DICT_AUTO", "TYCHE_LZ4_DICT_AUTO_PAGES", "TYCHE_LZ4_EXACT"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", _CHILD + code], env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout.strip().splitlines()


def test_env_auto_rules(tmp_path):
    """TYCHE_LZ4_DICT_AUTO malformed, out of range, or set beside TYCHE_LZ4_DICT: every LZ4 host call
    is TYCHE_E_BAD_ARGS with the reason, before any device work; LZ4_EXACT=1 beside it is the
    does-not-combine error (a fresh child process each)."""
    calls = ("for k in range(2):\n"
             "    print(lib.tyche_compress_host(1, 1, 1, srcs, slen, dsts, dcap, res), _lib.last_error())\n"
             "print(lib.tyche_decompress_host(1, 1, srcs, slen, dsts, dcap, res), _lib.last_error())\n")
    dic = tmp_path / "some.dict"
    dic.write_bytes(bytes(1000))
    for env, why in ((dict(TYCHE_LZ4_DICT_AUTO="abc"), "abc"), (dict(TYCHE_LZ4_DICT_AUTO="4096x"), "4096x"),
                     (dict(TYCHE_LZ4_DICT_AUTO="127"), "127"), (dict(TYCHE_LZ4_DICT_AUTO="32769"), "32769"),
                     (dict(TYCHE_LZ4_DICT_AUTO="4096", TYCHE_LZ4_DICT_AUTO_PAGES="0"), "TYCHE_LZ4_DICT_AUTO_PAGES"),
                     (dict(TYCHE_LZ4_DICT_AUTO="4096", TYCHE_LZ4_DICT=str(dic)), "both")):
        lines = _child(calls, **env)
        assert len(lines) == 3, lines
        for ln in lines:
            assert ln.startswith("190 ") and "TYCHE_LZ4_DICT_AUTO" in ln and why in ln, (env, ln)
    lines = _child("print(lib.tyche_compress_host(1, 1, 1, srcs, slen, dsts, dcap, res), _lib.last_error())\n",
                   TYCHE_LZ4_DICT_AUTO="4096", TYCHE_LZ4_EXACT="1")
    assert lines[0].startswith("190 ") and "LZ4_EXACT" in lines[0], lines
    # a tyche_lz4_use_dict call ends auto mode and wins, whatever was collected
    lines = _child("h = lib.tyche_lz4_dict_create(bytes(64), 64)\n"
                   "print(lib.tyche_lz4_use_dict(h), lib.tyche_lz4_current_dict() == h)\n",
                   TYCHE_LZ4_DICT_AUTO="4096")
    assert lines == ["0 True"], lines


def test_no_device_is_an_error_not_a_cpu_trainer(lib):
    """Without a usable device the trainer returns NULL and says why; with one, this is
    test_gpu_lz4_train.py's ground."""
    from tyche_amd import _lib
    if lib.tyche_device_ready() == 1:
        return
    keep, srcs, lens = _host_args([bytes(range(256)) * 4] * 4)
    assert not lib.tyche_lz4_dict_train_host(4, srcs, lens, 1024)
    assert "device" in _lib.last_error().lower(), _lib.last_error()
