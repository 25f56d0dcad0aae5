"""The checked layout (tests/batch_layout.py) against a fake numpy "kernel" with planted faults:
every fault is reported with the page and the offset it was planted at, a clean run passes, and
the arenas are laid out as the GPU suites rely on.  No GPU."""
import numpy as np
import pytest

import batch_layout as BL

LENS = [0, 1, 15, 16, 17, 63, 64, 65, 300, 0, 4097, 33]
CAPS = [0, 1, 15, 16, 17, 0, 64, 65, 299, 7, 4096, 48]
N = len(LENS)
SRC_SHIFTS = [(7 * i) % 16 for i in range(N)]
DST_SHIFTS = [i % 16 for i in range(N)]
GAPS = ["zero", "ff", ("random", 1)]


def _inputs():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENS]


def _layout(gap="zero", **kw):
    return BL.build(_inputs(), CAPS, SRC_SHIFTS, DST_SHIFTS, gap, **kw)


def fake_kernel(lay, results=None):
    """Copies min(len, cap) input bytes into each slot, like a codec that respects the contract."""
    out, src = lay.out.copy(), lay.src.copy()
    rv = np.zeros(lay.count, np.int32)
    for i in range(lay.count):
        k = min(int(lay.src_lengths[i]), int(lay.caps[i]))
        out[lay.dst_offsets[i]:lay.dst_offsets[i] + k] = src[lay.src_offsets[i]:lay.src_offsets[i] + k]
        rv[i] = k
    return out, src, rv


@pytest.mark.parametrize("gap", GAPS, ids=["zero", "ff", "random"])
def test_layout_placement_and_fill(gap):
    lay = _layout(gap)
    inputs = _inputs()
    assert lay.src_offsets.dtype == np.int64 and lay.dst_offsets.dtype == np.int64
    assert lay.src_lengths.dtype == np.int32 and lay.caps.dtype == np.int32
    assert list(lay.src_lengths) == LENS and list(lay.caps) == CAPS
    owned = np.zeros(lay.src.size, bool)
    for i in range(N):
        a = int(lay.src_offsets[i])
        assert a % 16 == SRC_SHIFTS[i] and int(lay.dst_offsets[i]) % 16 == DST_SHIFTS[i]
        assert lay.src[a:a + LENS[i]].tobytes() == inputs[i]
        assert not owned[a:a + LENS[i]].any()
        owned[a:a + LENS[i]] = True
        nxt = int(lay.src_offsets[i + 1]) if i + 1 < N else lay.src.size
        assert nxt - (a + LENS[i]) >= BL.SRC_GAP                     # at least 64 bytes after every item
    want = BL._gap_bytes(gap, lay.src.size)
    assert np.array_equal(lay.src[~owned], want[~owned])             # heads of first lines, gaps, the tail
    if gap != "zero":
        assert lay.src[~owned].any()
    assert (lay.out == 0xAB).all()
    ends = lay.dst_offsets + lay.caps
    assert lay.dst_offsets[0] >= lay.guard and lay.out.size - ends[-1] >= lay.guard
    assert (lay.dst_offsets[1:] - ends[:-1] >= 2 * lay.guard).all()  # guards are not shared


@pytest.mark.parametrize("gap", GAPS, ids=["zero", "ff", "random"])
def test_clean_run_passes(gap):
    lay = _layout(gap)
    out, src, rv = fake_kernel(lay)
    BL.check(out, src, lay)
    got = BL.outputs(out, rv, lay)
    inputs = _inputs()
    assert got == [inputs[i][:min(LENS[i], CAPS[i])] for i in range(N)]
    rv[3] = -5                                                        # an error result yields no bytes
    assert BL.outputs(out, rv, lay)[3] == b""


def test_unspecified_tail_inside_the_slot_is_not_checked():
    """[rv, cap) belongs to the page: a kernel may leave anything there."""
    lay = _layout()
    out, src, rv = fake_kernel(lay)
    i = 9                                                            # a 0-byte input with a 7-byte capacity
    out[lay.dst_offsets[i]:lay.dst_offsets[i] + CAPS[i]] = 0x5A
    BL.check(out, src, lay)
    assert BL.outputs(out, rv, lay)[i] == b""


def _fault(page, pos, width=1, value=0x11, **kw):
    lay = _layout(**kw)
    out, src, _ = fake_kernel(lay)
    a = int(lay.dst_offsets[page])
    at = {"cap": a + CAPS[page], "start-1": a - 1, "last_guard": a + CAPS[page] + lay.guard - 1,
          "first_guard": a - lay.guard, "straddle": a + CAPS[page] - 5}[pos]
    out[at:at + width] = value
    with pytest.raises(BL.LayoutViolation) as e:
        BL.check(out, src, lay)
    return e.value


@pytest.mark.parametrize("page", range(N))
def test_one_byte_at_cap(page):
    """Zero capacities (pages 0 and 5) included: the byte at start + cap is the first guard byte."""
    v = _fault(page, "cap")
    assert (v.kind, v.page, v.distance, v.value, v.count) == ("after", page, 0, 0x11, 1), str(v)
    assert f"page {page}:" in str(v) and "byte 0 past the end" in str(v) and "0x11" in str(v)


@pytest.mark.parametrize("page", range(N))
def test_one_byte_before_start(page):
    v = _fault(page, "start-1")
    assert (v.kind, v.page, v.distance, v.value, v.count) == ("before", page, 1, 0x11, 1), str(v)
    assert f"page {page}:" in str(v) and "byte 1 before the start" in str(v)


@pytest.mark.parametrize("page", [2, 3, 8, 10])
def test_16_byte_store_straddling_cap(page):
    """A 16-byte store that starts 5 bytes inside the slot: 11 bytes land outside it."""
    v = _fault(page, "straddle", width=16, value=0xEE)
    assert (v.kind, v.page, v.distance, v.value, v.count) == ("after", page, 0, 0xEE, 11), str(v)


@pytest.mark.parametrize("page", [0, 4, N - 1])
@pytest.mark.parametrize("guard", [64, 1, 37])
def test_last_and_first_guard_byte(page, guard):
    v = _fault(page, "last_guard", guard=guard)
    assert (v.kind, v.page, v.distance, v.count) == ("after", page, guard - 1, 1), str(v)
    v = _fault(page, "first_guard", guard=guard)
    assert (v.kind, v.page, v.distance, v.count) == ("before", page, guard, 1), str(v)


def test_other_fill_values():
    """A stray byte equal to the fill cannot be seen; the same fault under another fill is caught."""
    for fill, caught in ((0xAB, False), (0x00, True)):
        lay = _layout(fill=fill)
        out, src, _ = fake_kernel(lay)
        out[lay.dst_offsets[4] + CAPS[4]] = 0xAB
        if caught:
            with pytest.raises(BL.LayoutViolation):
                BL.check(out, src, lay)
        else:
            BL.check(out, src, lay)


@pytest.mark.parametrize("where", ["item", "gap", "tail"])
def test_write_into_source_arena(where):
    lay = _layout(("random", 3))
    out, src, _ = fake_kernel(lay)
    i = 8
    at = {"item": int(lay.src_offsets[i]) + 10, "gap": int(lay.src_offsets[i]) + LENS[i] + 3,
          "tail": lay.src.size - 1}[where]
    src[at] ^= 0x40
    with pytest.raises(BL.LayoutViolation) as e:
        BL.check(out, src, lay)
    v = e.value
    assert (v.kind, v.distance, v.count) == ("source", at, 1), str(v)
    assert v.page == (N - 1 if where == "tail" else i)
    assert (lay.src == BL.build(_inputs(), CAPS, SRC_SHIFTS, DST_SHIFTS, ("random", 3)).src).all()   # check() kept its copy


def test_all_zero_capacities_and_empty_inputs():
    lay = BL.build([b""] * 5, [0] * 5, 0, [0, 1, 2, 3, 15], "ff")
    out, src, rv = fake_kernel(lay)
    BL.check(out, src, lay)
    assert BL.outputs(out, rv, lay) == [b""] * 5
    out[lay.dst_offsets[2]] = 0
    with pytest.raises(BL.LayoutViolation) as e:
        BL.check(out, src, lay)
    assert (e.value.kind, e.value.page, e.value.distance) == ("after", 2, 0)


def test_bad_arguments():
    with pytest.raises(ValueError):
        BL.build([b"a"], [1], 16, 0, "zero")
    with pytest.raises(ValueError):
        BL.build([b"a"], [1], 0, 0, "ones")
    with pytest.raises(ValueError):
        BL.build([b"a"], [1, 2], 0, 0, "zero")
