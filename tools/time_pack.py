"""Times the packed store (pack.hip) on one MI355X, LZ4 on pagegen dist 0 pages of 16 KiB, warm and
by HIP events on the launch stream:

    python tools/time_pack.py [--pages 65536,1048576] [--reps 7] [--pack-only]

Per shape, one JSON line with
  (a) pack_ms        tyche_pack_batch at align 16 into a fresh state (the state's reset is in the window)
  (b) copy_ms        a device-to-device copy of the same `used` bytes, same session: the yardstick of (a)
  (c) decode_*_ms    LZ4 decode from the slots, and from the arena packed at align 1, 16 and 128
  (d) encode_ms      the encode that filled the slots, for scale
Every figure is the median of --reps runs, the variants of a group taken in turn inside each
repetition, with the spread (min .. max) beside it.  --pack-only stops after (a) and (b): for A/B
libraries (TYCHE_CODEC_LIB=<a build with -DTYCHE_PACK_TILE=...>), whose line carries the library's name.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tyche_amd import _lib, codec  # noqa: E402

dev = torch.device("cuda:0")
PLEN = 16384


def rounds(variants: dict, reps: int) -> dict:
    """name -> fn; every repetition runs each once, in turn; -> name -> (median, min, max) ms."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in variants}
    for k, fn in variants.items():      # warm: code objects, scratch leases, counters
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in variants.items():
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def put(r: dict, name: str, t) -> None:
    r[name + "_ms"] = round(t[0], 3)
    r[name + "_spread_ms"] = [round(t[1], 3), round(t[2], 3)]


def shape(n: int, reps: int, pack_only: bool) -> dict:
    pages = codec.pagegen(n, PLEN, dist=0, device=dev)
    slots, clen = codec.compress_pages(pages)
    torch.cuda.synchronize()
    total = int(clen.to(torch.int64).sum())
    r = {"lib": os.path.basename(_lib.LIB_PATH), "pages": n, "page_len": PLEN, "slot": int(slots.shape[1]),
         "stream_bytes": total, "ratio": round(n * PLEN / total, 3)}
    offsets = torch.empty((n,), dtype=torch.int64, device=dev)
    lengths = torch.empty((n,), dtype=torch.int32, device=dev)
    state = codec.new_pack_state(dev)
    arena = torch.empty((total + 128 * n,), dtype=torch.uint8, device=dev)   # room for align 128

    def pack(align):
        state.zero_()
        codec.pack_pages(slots, clen, arena, state, align, offsets, lengths)

    pack(16)
    torch.cuda.synchronize()
    used = int(state[0])
    assert used == int(state[1]) and used <= arena.numel()
    flat, other = slots.reshape(-1), torch.empty((used,), dtype=torch.uint8, device=dev)
    t = rounds({"pack": lambda: pack(16), "copy": lambda: other.copy_(flat[:used])}, reps)
    r["used_bytes_align16"] = used
    put(r, "pack", t["pack"])
    put(r, "copy", t["copy"])
    r["pack_over_copy"] = round(t["pack"][0] / t["copy"][0], 3)
    r["pack_gb_s"] = round(used / t["pack"][0] / 1e6, 1)     # arena bytes written per second
    r["copy_gb_s"] = round(used / t["copy"][0] / 1e6, 1)
    del other
    if pack_only:
        return r
    out = torch.empty((n, PLEN), dtype=torch.uint8, device=dev)
    rv = torch.empty((n,), dtype=torch.int32, device=dev)
    mx = int(clen.max())
    stores = {}
    for align in (1, 16, 128):
        a = torch.empty((total + align * n,), dtype=torch.uint8, device=dev)
        o, ln, st = codec.pack_pages(slots, clen, a, align=align)
        codec.decompress_packed(a, o, ln, PLEN, out=out, rv=rv, max_comp_len=mx)
        torch.cuda.synchronize()
        assert int(st[0]) == int(st[1]) and bool((rv == PLEN).all()) and torch.equal(out, pages), align
        stores[align] = (a, o, ln)
    variants = {"decode_slots": lambda: codec.decompress_pages(slots, clen, PLEN, out=out, rv=rv, max_comp_len=mx)}
    for align, (a, o, ln) in stores.items():
        variants[f"decode_align{align}"] = (lambda a=a, o=o, ln=ln: codec.decompress_packed(a, o, ln, PLEN, out=out, rv=rv,
                                                                                            max_comp_len=mx))
    variants["encode"] = lambda: codec.compress_pages(pages, out=slots, out_len=clen)
    for k, v in rounds(variants, reps).items():
        put(r, k, v)
    return r


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", default="65536,1048576")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pack-only", action="store_true")
    args = ap.parse_args()
    assert _lib.load().tyche_device_ready() == 1, _lib.last_error()
    for n in args.pages.split(","):
        print(json.dumps(shape(int(n), args.reps, args.pack_only)), flush=True)
        torch.cuda.empty_cache()
