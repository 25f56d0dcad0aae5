"""CPU checks of the packed store: the kernels' rule and copy geometry (tyche_amd/csrc/pack_core.h)
through the host emulator tools/pack_emul.cpp against the numpy restatement (pack_cases.pack_spec /
apply_spec) on every corpus case -- offsets, lengths, state and every arena byte; tyche_pack_plan
(the same rule on host arrays, no GPU) against it; and every TYCHE_E_BAD_ARGS refusal of
tyche_pack_batch with its message.  test_gpu_pack.py holds the kernels to the emulator's bytes.

PACK_EMUL_RECORD=<file> records every emulator call of a run for the stand-alone sanitizer program
(tools/pack_emul.cpp with -DPACK_EMUL_MAIN), which replays them."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import pack_cases as P
from conftest import ROOT

LIB = os.path.join(ROOT, "tools", "bin", "libpackemul.so")
SRC = os.path.join(ROOT, "tools", "pack_emul.cpp")
CORE = os.path.join(ROOT, "tyche_amd", "csrc", "pack_core.h")
RECORD = os.environ.get("PACK_EMUL_RECORD")
GUARD = 256


class Emul:
    """The emulator: constants T, S, F, PROBES and run(case) -> (offsets, lengths, state, stored, arena)."""

    def __init__(self):
        if not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in (SRC, CORE)):
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
        self.lib = ctypes.CDLL(LIB)
        self.lib.pack_emul.restype = ctypes.c_int
        self.lib.pack_emul.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        k = (ctypes.c_uint32 * 4)()
        self.lib.pack_emul_constants(k)
        self.T, self.S, self.F, self.PROBES = (int(x) for x in k)

    def run(self, case: P.Case):
        n = len(case.results)
        src = case.src.copy()
        arena = np.full(GUARD + case.capacity + GUARD, P.FILL, np.uint8)
        state = np.asarray(case.state, np.uint64)
        offs, lens = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
        r = self.lib.pack_emul(src.ctypes.data, case.src_offsets.ctypes.data, 0, case.results.ctypes.data, n, case.max_length,
                               arena.ctypes.data + GUARD, case.capacity, case.align, case.skew, state.ctypes.data,
                               offs.ctypes.data, lens.ctypes.data)
        assert r in (0, 1), r
        assert bool((arena[:GUARD] == P.FILL).all()) and bool((arena[GUARD + case.capacity:] == P.FILL).all()), "wrote outside the arena"
        assert np.array_equal(src, case.src), "wrote to the source"
        body = arena[GUARD:GUARD + case.capacity]
        if RECORD:
            streams = b"".join(case.src[int(o):int(o) + int(ln)].tobytes()
                               for o, ln in zip(case.src_offsets, P.lens_of(case.results, case.max_length)))
            with open(RECORD, "ab") as f:
                f.write(struct.pack("<IIIIQQQQQi", n, case.max_length, case.align, case.skew, case.capacity, case.state[0],
                                    case.state[1], int(state[0]), int(state[1]), r))
                f.write(case.results.tobytes() + streams + offs[:n].tobytes() + lens[:n].tobytes() + body.tobytes())
        return offs[:n], lens[:n], (int(state[0]), int(state[1])), bool(r), body


@pytest.fixture(scope="module")
def emul():
    return Emul()


def check_case(emul, case):
    want = P.expected(case)
    got = emul.run(case)
    assert np.array_equal(got[0], want[0]), (case.name, "offsets")
    assert np.array_equal(got[1], want[1]), (case.name, "lengths")
    assert got[2] == want[2] and got[3] == want[3], (case.name, got[2:4], want[2:4])
    assert np.array_equal(got[4], want[4]), (case.name, "arena bytes", int(np.flatnonzero(got[4] != want[4])[0]))


# ---------------------------------------------------------------- the emulator against the specification
def test_constants(emul):
    assert emul.T % 128 == 0 and emul.PROBES == 64 and emul.S >= 64 and emul.F >= 2


def test_edge_cases_equal_the_specification(emul):
    """Every length around a line and a tile at every source misalignment, every align and start."""
    cases = P.edge_cases(emul.T)
    assert len(cases) == len(P.ALIGNS) * len(P.STARTS)
    for case in cases:
        check_case(emul, case)


def test_scan_cases_equal_the_specification(emul):
    for case in P.scan_cases(emul.S, emul.F):
        check_case(emul, case)


def test_refusal_cases_equal_the_specification(emul):
    cases = P.refusal_cases(emul.T)
    for case in cases:
        check_case(emul, case)
    assert [P.expected(c)[3] for c in cases] == [False, True, False, True]


@pytest.mark.parametrize("skew", [0, 1, 15, 16, 127])
def test_arena_address_does_not_show(emul, skew):
    """Where the tiles fall (the arena address's low bits) changes nothing."""
    case = P.edge_cases(emul.T)[4]
    case.skew = skew
    check_case(emul, case)


def test_compaction_is_the_same_call(emul):
    """Every other page of a packed arena, with its offsets as src_offsets and its lengths as
    results, into a second arena == packing those pages' slots directly."""
    case = P.edge_cases(emul.T)[6]
    offs, lens, state, stored, arena = emul.run(case)
    assert stored
    keep = np.arange(0, len(lens), 2)
    second = P.Case("compact", lens[keep].astype(np.int32), 0, 16, (0, 0), state[1], arena, offs[keep].copy(),
                    np.zeros(len(arena), bool), 5)
    direct = P.Case("direct", case.results[keep].copy(), case.max_length, 16, (0, 0), state[1], case.src,
                    case.src_offsets[keep].copy(), case.stream_mask, 5)
    a, b = emul.run(second), emul.run(direct)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    check_case(emul, second)


# ---------------------------------------------------------------- tyche_pack_plan
def plan(lib, results, max_length, align, capacity, state):
    n = len(results)
    st = np.asarray(state, np.uint64)
    offs, lens = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    end = lib.tyche_pack_plan(n, results.ctypes.data, max_length, align, capacity, st.ctypes.data, offs.ctypes.data,
                              lens.ctypes.data)
    return end, offs[:n], lens[:n], (int(st[0]), int(st[1]))


def test_pack_plan_equals_the_specification(emul):
    from tyche_amd import _lib
    lib = _lib.load()
    for case in P.corpus(emul.T, emul.S, emul.F):
        want = P.pack_spec(case.results, case.max_length, case.align, case.state, case.capacity)
        end, offs, lens, state = plan(lib, case.results, case.max_length, case.align, case.capacity, case.state)
        assert np.array_equal(offs, want[0]) and np.array_equal(lens, want[1]), case.name
        assert state == want[2] and end == want[2][1], (case.name, state, want[2])
    # sizing an arena: no output arrays, capacity 0 -- the state's second word is the size needed
    r = np.asarray([5, 0, 17], np.int32)
    st = np.zeros(2, np.uint64)
    assert lib.tyche_pack_plan(3, r.ctypes.data, 0, 16, 0, st.ctypes.data, None, None) == 33 and list(st) == [0, 33]


def test_pack_plan_offsets_beyond_32_bits():
    from tyche_amd import _lib
    r = np.full(8, 100, np.int32)
    start = 2 ** 32 - 100
    end, offs, lens, state = plan(_lib.load(), r, 0, 1, 2 ** 33, (start, start))
    assert list(offs) == [start + 100 * i for i in range(8)] and end == start + 800 and state == (end, end)


# ---------------------------------------------------------------- refusals, decided before any device call
def test_bad_args_and_messages():
    from tyche_amd import _lib
    lib = _lib.load()
    one = ctypes.c_uint64(0)
    ptr = ctypes.addressof(one)

    def call(**kw):
        f = dict(count=1, src=ptr, results=ptr, arena=ptr, arena_capacity=8, align=16, state=ptr, offsets=ptr, lengths=ptr)
        f.update(kw)
        return lib.tyche_pack_batch(ctypes.byref(_lib.Pack(**f)), None)

    for align in (0, 3, 24, 8192):
        assert call(align=align) == _lib.E_BAD_ARGS
        msg = _lib.last_error()
        assert "power of two" in msg and "4096" in msg and f"got {align}" in msg, msg
        assert call(align=align, count=0) == _lib.E_BAD_ARGS          # also for an empty batch
    for field in ("src", "results", "arena", "state", "offsets", "lengths"):
        assert call(**{field: None}) == _lib.E_BAD_ARGS, field
        msg = _lib.last_error()
        assert "NULL" in msg and field in msg and "1 pages" in msg, msg
    assert call(count=_lib.PACK_MAX_PAGES + 1) == _lib.E_BAD_ARGS
    msg = _lib.last_error()
    assert "TYCHE_PACK_MAX_PAGES" in msg and str(_lib.PACK_MAX_PAGES) in msg and str(_lib.PACK_MAX_PAGES + 1) in msg, msg
    assert _lib.PACK_MAX_PAGES >= 2 ** 24
    assert lib.tyche_pack_batch(None, None) == _lib.E_BAD_ARGS
    # an empty batch needs nothing and touches nothing
    assert call(count=0, src=None, results=None, arena=None, state=None, offsets=None, lengths=None) == _lib.E_OK
    # the plan refuses the same arguments
    st = np.zeros(2, np.uint64)
    assert lib.tyche_pack_plan(1, ptr, 0, 3, 0, st.ctypes.data, None, None) == 2 ** 64 - 1
    assert "power of two" in _lib.last_error()
    assert lib.tyche_pack_plan(1, None, 0, 16, 0, st.ctypes.data, None, None) == 2 ** 64 - 1
    assert "NULL" in _lib.last_error()


def test_pack_without_a_device_is_a_device_error():
    """No GPU here: a well-formed call reports TYCHE_E_DEVICE; nothing packs on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from tyche_amd import _lib
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(buf)
    pk = _lib.Pack(count=1, src=p, results=p, arena=p + 32, arena_capacity=8, align=16, state=p + 16, offsets=p + 48, lengths=p + 56)
    assert _lib.load().tyche_pack_batch(ctypes.byref(pk), None) == _lib.E_DEVICE
    assert _lib.last_error()
