"""The checked batch layout: arenas for a ragged batch whose every byte outside the pages is known,
so a test can assert the batch contract of include/tyche_codec.h after a run --

* page i reads src_lengths[i] bytes at src + src_offsets[i] and nothing it reads outside them
  changes its result (the bytes around every item are chosen by the caller: gap_fill);
* page i writes at most dst_capacities[i] bytes at dst + dst_offsets[i] (every other output byte
  is pre-filled and compared afterwards);
* src is never written.

Pure numpy: build() lays a batch out, the caller runs any "kernel" over the arenas (the GPU
suites copy them to the device and back), check() compares.  Bytes in [result, capacity) of a slot
are unspecified (the zstd kernels keep their literal buffer there) and are never looked at.
"""
import hashlib
from dataclasses import dataclass

import numpy as np

SRC_GAP = 64            # bytes after every source item that belong to no item (at least)


class LayoutViolation(AssertionError):
    """A byte outside every output slot changed, or the source arena did.

    kind     -- "after" (at or past a slot's end), "before" (ahead of its start) or "source"
    page     -- the page whose guard was hit (source: the item at or before the byte, or -1)
    distance -- after: offset from the slot's end (0 = the byte at `capacity`); before: bytes ahead
                of the start (1 = the byte at start - 1); source: offset in the source arena
    value    -- the byte found there
    """

    def __init__(self, kind, page, distance, value, count, extra=""):
        self.kind, self.page, self.distance, self.value, self.count = kind, int(page), int(distance), int(value), int(count)
        if kind == "source":
            msg = f"source arena written: byte {distance} (item {page}) is now 0x{value:02x}; {count} bytes differ"
        elif kind == "after":
            msg = (f"page {page}: byte {distance} past the end of its slot (capacity{extra}) is 0x{value:02x};"
                   f" {count} bytes outside the slots changed")
        else:
            msg = (f"page {page}: byte {distance} before the start of its slot{extra} is 0x{value:02x};"
                   f" {count} bytes outside the slots changed")
        super().__init__(msg)


@dataclass
class Layout:
    src: np.ndarray          # uint8 source arena (check() compares against it: hand the kernel a copy)
    src_offsets: np.ndarray  # int64
    src_lengths: np.ndarray  # int32
    out: np.ndarray          # uint8 output arena, all `fill`
    dst_offsets: np.ndarray  # int64
    caps: np.ndarray         # int32
    guard: int
    fill: int
    src_digest: bytes        # sha256 of the source arena

    @property
    def count(self):
        return len(self.caps)


def _gap_bytes(gap_fill, n):
    if gap_fill == "zero":
        return np.zeros(n, np.uint8)
    if gap_fill == "ff":
        return np.full(n, 0xFF, np.uint8)
    if isinstance(gap_fill, tuple) and len(gap_fill) == 2 and gap_fill[0] == "random":
        return np.random.default_rng(gap_fill[1]).integers(0, 256, n, dtype=np.uint8)
    raise ValueError(f"gap_fill {gap_fill!r}: 'zero', 'ff' or ('random', seed)")


def _shifts(shifts, n):
    s = [int(shifts)] * n if np.isscalar(shifts) else [int(x) for x in shifts]
    if len(s) != n or any(not 0 <= x <= 15 for x in s):
        raise ValueError("shifts: one value in 0..15 per item")
    return s


def build(inputs, caps, src_shifts, dst_shifts, gap_fill, guard=64, fill=0xAB) -> Layout:
    """Lays out a batch.  inputs: byte strings; caps: output capacities; *_shifts: one value (or one
    per item) in 0..15 added to the item's 16-byte boundary.  Every source byte that belongs to no
    item -- the head of an item's first 16-byte line, at least SRC_GAP bytes after it, the arena's
    tail -- comes from gap_fill.  Every output slot has `guard` bytes of `fill` of its own on either
    side (neighbours do not share them), and the arena holds `fill` everywhere."""
    n = len(inputs)
    if len(caps) != n:
        raise ValueError("one capacity per input")
    if guard < 1:
        raise ValueError("guard must be at least one byte")
    ss, ds = _shifts(src_shifts, n), _shifts(dst_shifts, n)
    src_offsets, pos = np.zeros(n, np.int64), 0
    for i, s in enumerate(inputs):
        src_offsets[i] = (pos + 15) // 16 * 16 + ss[i]
        pos = int(src_offsets[i]) + len(s) + SRC_GAP
    src = _gap_bytes(gap_fill, (pos + 15) // 16 * 16 + SRC_GAP)
    for i, s in enumerate(inputs):
        src[src_offsets[i]:src_offsets[i] + len(s)] = np.frombuffer(bytes(s), np.uint8)
    dst_offsets, pos = np.zeros(n, np.int64), 0
    for i, c in enumerate(caps):
        if c < 0:
            raise ValueError("capacities are not negative")
        dst_offsets[i] = (pos + guard + 15) // 16 * 16 + ds[i]
        pos = int(dst_offsets[i]) + int(c) + guard
    out = np.full((pos + 15) // 16 * 16 + 16, fill, np.uint8)
    return Layout(src=src, src_offsets=src_offsets, src_lengths=np.array([len(s) for s in inputs], np.int32),
                  out=out, dst_offsets=dst_offsets, caps=np.array([int(c) for c in caps], np.int32),
                  guard=guard, fill=fill, src_digest=hashlib.sha256(src).digest())


def check(out_after, src_after, layout: Layout) -> None:
    """Asserts that every byte outside all [start_i, start_i + cap_i) of out_after still is `fill`,
    and that src_after is the source arena build() made.  Raises LayoutViolation naming the page,
    the distance from its slot's end (or start) and the value of the first such byte."""
    out_after = np.ascontiguousarray(out_after, np.uint8).reshape(-1)
    src_after = np.ascontiguousarray(src_after, np.uint8).reshape(-1)
    assert out_after.shape == layout.out.shape, (out_after.shape, layout.out.shape)
    assert src_after.shape == layout.src.shape, (src_after.shape, layout.src.shape)
    starts = layout.dst_offsets
    ends = starts + layout.caps.astype(np.int64)
    # the bytes outside the slots: [end of slot i-1, start of slot i), the arena's head and tail included
    gap_a = np.concatenate([[0], ends])
    gap_n = np.concatenate([starts, [out_after.size]]) - gap_a
    assert (gap_n >= layout.guard).all()
    outside = np.repeat(gap_a - (np.cumsum(gap_n) - gap_n), gap_n) + np.arange(int(gap_n.sum()))
    bad = outside[out_after[outside] != layout.fill]
    if bad.size:
        x = int(bad[0])
        i = int(np.searchsorted(starts, x, side="right")) - 1   # the last slot that starts at or before x
        nxt = i + 1
        if i < 0 or (nxt < layout.count and int(starts[nxt]) - x <= layout.guard):
            raise LayoutViolation("before", nxt, int(starts[nxt]) - x, out_after[x], bad.size,
                                  f" at {int(starts[nxt])}")
        raise LayoutViolation("after", i, x - int(ends[i]), out_after[x], bad.size, f" {int(layout.caps[i])}")
    if hashlib.sha256(src_after).digest() != layout.src_digest:
        diff = np.nonzero(src_after != layout.src)[0]
        assert diff.size, "the layout's own source arena was changed: hand the kernel a copy"
        x = int(diff[0])
        i = int(np.searchsorted(layout.src_offsets, x, side="right")) - 1
        raise LayoutViolation("source", i, x, src_after[x], diff.size)


def outputs(out_after, results, layout: Layout):
    """out[start_i : start_i + max(rv_i, 0)] per page, as bytes.  Bytes in [rv_i, cap_i) are
    unspecified and never returned."""
    out_after = np.asarray(out_after, np.uint8).reshape(-1)
    res = []
    for i in range(layout.count):
        a = int(layout.dst_offsets[i])
        res.append(out_after[a:a + max(int(results[i]), 0)].tobytes())
    return res
