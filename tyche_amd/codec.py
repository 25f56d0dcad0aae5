"""Device-resident batch codec on torch tensors (thin layer over the C ABI).

torch is only the plumbing here: it owns the HBM buffers and the stream; every
byte of codec work is done by the gfx950 kernels in libtyche_codec.so, reached
through ``tyche_compress_batch`` / ``tyche_decompress_batch``.

Layout in HBM: pages are rows of a (n, page_len) uint8
tensor; compressed pages are rows of a (n, slot) uint8 tensor whose slot is
``compress_bound(page_len)`` rounded up to 128 bytes, plus an int32 length per
row.  Only ``comp_len`` bytes of a slot are read or written by the kernels.

Page sizes: LZ4 rows may be up to ``TYCHE_LZ4_MAX_PAGE`` (4 MiB) long, in both
directions; rows above 65,535 bytes take the large-page kernels and still
become one standard LZ4 block each.  zlib and zstd compress rows of up to
65,535 bytes, and so does LZ4 under ``LZ4_EXACT=1``; beyond a limit the call
raises ``DeviceError`` (``TYCHE_E_BAD_ARGS``, the limit in the message).

High-compression modes: with ``TYCHE_LZ4_HC=1`` in the environment, or
``_lib.set_knob("LZ4_HC", 1)``, ``compress_pages`` / ``compress_ragged`` give
rows of up to 65,535 bytes to the high-compression encoder: the same LZ4 blocks
from a better parse, 11-20 % fewer bytes on the 16 KiB bench pages at about 23x
the default encoder's time, restored by ``decompress_pages`` as any other block
(a little faster: fewer sequences).  Longer rows and ``dictionary=`` calls are
as without the knob; ``LZ4_EXACT=1`` beside it raises ``DeviceError``
(``TYCHE_E_BAD_ARGS``).  ``dictionary=`` calls have a knob of their own:
with ``TYCHE_LZ4_HC_DICT=1`` or ``_lib.set_knob("LZ4_HC_DICT", 1)`` the LZ4
rows a dictionary reaches take the same parse over dictionary and row --
ordinary dictionary blocks, 3-14 % fewer bytes than the dictionary alone on
4 KiB bench pages, restored by ``decompress_pages(..., dictionary=d)``.
zstd has the same kind of mode: with ``TYCHE_ZSTD_HC=1`` or
``_lib.set_knob("ZSTD_HC", 1)`` every zstd compress call takes the
high-compression parse -- ordinary zstd frames, 3-6 % fewer bytes on the bench
pages (up to 9 % on pages of fixed-size items) at 4-11x the default encoder's
time, restored by ``decompress_pages`` in the same time as any other frame.
``dictionary=`` calls are as without the knob, and the two knobs are
independent.
zlib too: with ``TYCHE_ZLIB_HC=1`` or ``_lib.set_knob("ZLIB_HC", 1)`` every zlib
compress call takes the high-compression parse -- ordinary zlib streams, 6-10 %
fewer bytes on the bench pages (a quarter on pages of index-like items) at
3-6x the default encoder's time, restored by ``decompress_pages`` in the time
any other stream takes.  The three knobs are independent.

Packed store: ``pack_pages`` appends the streams of ``compress_pages`` to a 1-D
arena at their compressed size (``tyche_pack_batch``) and returns offsets and
lengths, ``decompress_packed`` decodes from them, ``compress_pages_packed`` does
compress + append a chunk of rows at a time.  A store's state is two int64 words
on the device, ``{used, wanted}``; the device decides whether an append fits.

Shared dictionary (all three codecs): ``dictionary=Dictionary(bytes)`` makes the
dictionary and each row one window.  LZ4: the blocks are what
``LZ4_decompress_safe_usingDict`` restores.  zstd: the bytes are a raw-content
dictionary, the frames what ``ZSTD_decompress_usingDict`` restores (bytes that
begin with zstd's dictionary magic 37 A4 30 EC are refused: structured
dictionaries are not supported).  Either way the same dictionary is needed to
decode, and row length (capacity, when decoding) plus dictionary may not exceed
65,536 bytes.  zlib: the bytes are a preset dictionary, the streams what
``inflateSetDictionary`` + ``inflate`` restore (header 78 3F and the dictionary's
adler32; a row that does not compress is the plain stored stream), so a wrong
dictionary is an error (-3), never wrong bytes.  ``Dictionary`` is the
codec-neutral name of ``Lz4Dict``: one handle serves all three codecs.
``Lz4Dict.train(pages, length)`` makes one from sample pages on the GPU;
``Lz4Dict.data`` returns a dictionary's bytes.  ``use_zstd_dict(d)`` installs
one for the host entry points' zstd calls (``None`` removes it),
``use_zlib_dict(d)`` one for their zlib calls; the three slots are independent.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import LZ4_COMPRESSOR_ID, ZLIB_COMPRESSOR_ID, ZSTD_COMPRESSOR_ID

SLOT_ALIGN = 128


def compress_bound(n: int, compressor_id: int = LZ4_COMPRESSOR_ID) -> int:
    return int(_lib.load().tyche_compress_bound(compressor_id, n))


def slot_size(page_len: int, compressor_id: int = LZ4_COMPRESSOR_ID) -> int:
    b = compress_bound(page_len, compressor_id)
    return (b + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN


def _stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


def _check_pages(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (the codec runs only on the GPU)")
    if t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous 2-D uint8 tensor")


class Lz4Dict:
    """A shared dictionary (tyche_lz4_dict_create): 1..LZ4_DICT_MAX bytes, copied, immutable, for the
    LZ4, zstd and zlib calls alike (``Dictionary`` is the same class).  The engine uploads it to a
    device the first time a launch there uses it."""

    def __init__(self, data: bytes):
        data = bytes(data)
        self._lib = _lib.load()
        self.handle = self._lib.tyche_lz4_dict_create(data, len(data))
        if not self.handle:
            raise ValueError(_lib.last_error())
        self.length = len(data)

    @classmethod
    def _from_handle(cls, handle) -> "Lz4Dict":
        d = cls.__new__(cls)
        d._lib = _lib.load()
        d.handle = handle
        d.length = int(d._lib.tyche_lz4_dict_length(handle))
        return d

    @classmethod
    def train(cls, pages, length: int) -> "Lz4Dict":
        """Trains a dictionary of at most ``length`` bytes (128..LZ4_DICT_MAX) on the GPU
        (tyche_lz4_dict_train_batch / _host): ``pages`` is an (n, page_len) uint8 device tensor, page_len
        up to 65,535, or a list of ``bytes``.  Blocks until the dictionary is made; raises ValueError with
        the engine's reason when it refuses (too few or too many samples, no device, pages that share
        nothing)."""
        lib = _lib.load()
        if isinstance(pages, torch.Tensor):
            _check_pages(pages, "pages")
            n, page_len = pages.shape
            b = _lib.Batch(count=n, src=_ptr(pages), src_stride=page_len, src_length=page_len, max_src_length=page_len)
            handle = lib.tyche_lz4_dict_train_batch(ctypes.byref(b), int(length), _stream_handle(pages.device))
        else:
            pages = [bytes(p) for p in pages]
            n = len(pages)
            keep = [ctypes.create_string_buffer(p, max(len(p), 1)) for p in pages]
            srcs = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(k) for k in keep])
            lens = (ctypes.c_uint32 * max(n, 1))(*[len(p) for p in pages])
            handle = lib.tyche_lz4_dict_train_host(n, srcs, lens, int(length))
        if not handle:
            raise ValueError(_lib.last_error())
        return cls._from_handle(handle)

    @property
    def data(self) -> bytes:
        """The dictionary's bytes."""
        out = ctypes.create_string_buffer(max(self.length, 1))
        n = self._lib.tyche_lz4_dict_bytes(self.handle, out, self.length)
        return out.raw[:n]

    def __len__(self) -> int:
        return self.length

    def close(self) -> None:
        """Drops this reference; a process-wide installation or a launch in flight keeps its own."""
        if self.handle:
            self._lib.tyche_lz4_dict_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


Dictionary = Lz4Dict   # the codec-neutral name


def use_zstd_dict(dictionary: Lz4Dict | None) -> None:
    """Installs ``dictionary`` as the process-wide zstd dictionary of the host entry points
    (tyche_zstd_use_dict); ``None`` removes it.  The LZ4 slot is not touched."""
    _lib.check(_lib.load().tyche_zstd_use_dict(dictionary.handle if dictionary is not None else None),
               "tyche_zstd_use_dict")


def use_zlib_dict(dictionary: Lz4Dict | None) -> None:
    """Installs ``dictionary`` as the process-wide zlib dictionary of the host entry points
    (tyche_zlib_use_dict); ``None`` removes it.  The LZ4 and zstd slots are not touched."""
    _lib.check(_lib.load().tyche_zlib_use_dict(dictionary.handle if dictionary is not None else None),
               "tyche_zlib_use_dict")


def _zlib_dict_call(compress: bool, compressor_id: int, b, stream: int, dictionary) -> bool:
    """zlib and a dictionary: the tyche_zlib_*_batch_dict call; False when the call is not that."""
    if dictionary is None or compressor_id != ZLIB_COMPRESSOR_ID:
        return False
    name = "tyche_zlib_compress_batch_dict" if compress else "tyche_zlib_decompress_batch_dict"
    _lib.check(getattr(_lib.load(), name)(dictionary.handle, ctypes.byref(b), stream), name)
    return True


def _compress_call(compressor_id: int, level: int, b, stream: int, dictionary) -> None:
    if dictionary is None:
        _lib.check(_lib.load().tyche_compress_batch(compressor_id, level, ctypes.byref(b), stream), "tyche_compress_batch")
        return
    if compressor_id == ZSTD_COMPRESSOR_ID:
        _lib.check(_lib.load().tyche_zstd_compress_batch_dict(dictionary.handle, ctypes.byref(b), stream),
                   "tyche_zstd_compress_batch_dict")
        return
    if compressor_id != LZ4_COMPRESSOR_ID:
        raise ValueError("dictionary= is an LZ4 and zstd feature")
    _lib.check(_lib.load().tyche_lz4_compress_batch_dict(dictionary.handle, ctypes.byref(b), stream),
               "tyche_lz4_compress_batch_dict")


def _decompress_call(compressor_id: int, b, stream: int, dictionary) -> None:
    if dictionary is None:
        _lib.check(_lib.load().tyche_decompress_batch(compressor_id, ctypes.byref(b), stream), "tyche_decompress_batch")
        return
    if compressor_id == ZSTD_COMPRESSOR_ID:
        _lib.check(_lib.load().tyche_zstd_decompress_batch_dict(dictionary.handle, ctypes.byref(b), stream),
                   "tyche_zstd_decompress_batch_dict")
        return
    if compressor_id != LZ4_COMPRESSOR_ID:
        raise ValueError("dictionary= is an LZ4 and zstd feature")
    _lib.check(_lib.load().tyche_lz4_decompress_batch_dict(dictionary.handle, ctypes.byref(b), stream),
               "tyche_lz4_decompress_batch_dict")


def compress_pages(pages: torch.Tensor, compressor_id: int = LZ4_COMPRESSOR_ID, level: int = 1,
                   out: torch.Tensor | None = None, out_len: torch.Tensor | None = None,
                   dictionary: Lz4Dict | None = None):
    """Compress every row of ``pages``; returns (slots, comp_len).

    comp_len[i] is LZ4_compress_default's return for row i (compressed bytes,
    0 on failure).  Asynchronous on the current stream.  LZ4 rows may be up to
    4 MiB long (module docstring).
    """
    _check_pages(pages, "pages")
    n, page_len = pages.shape
    slot = slot_size(page_len, compressor_id)
    if out is None:
        out = torch.empty((n, slot), dtype=torch.uint8, device=pages.device)
    if out_len is None:
        out_len = torch.empty((n,), dtype=torch.int32, device=pages.device)
    _check_pages(out, "out")
    b = _lib.Batch(count=n, src=_ptr(pages), src_stride=page_len, src_length=page_len, max_src_length=page_len,
                   dst=_ptr(out), dst_stride=out.shape[1], dst_capacity=out.shape[1], results=_ptr(out_len))
    if not _zlib_dict_call(True, compressor_id, b, _stream_handle(pages.device), dictionary):
        _compress_call(compressor_id, level, b, _stream_handle(pages.device), dictionary)
    return out, out_len


def decompress_pages(slots: torch.Tensor, comp_len: torch.Tensor, page_len: int,
                     compressor_id: int = LZ4_COMPRESSOR_ID, out: torch.Tensor | None = None,
                     rv: torch.Tensor | None = None, max_comp_len: int = 0, dictionary: Lz4Dict | None = None):
    """Decompress row i of ``slots`` (comp_len[i] bytes) into a page_len row.

    rv[i] is LZ4_decompress_safe's return (decoded size, or -(consumed)-1).
    ``max_comp_len`` (optional) bounds comp_len for LDS sizing; 0 = slot width.
    LZ4: page_len up to 4 MiB, whoever wrote the blocks.
    """
    _check_pages(slots, "slots")
    if comp_len.dtype != torch.int32 or not comp_len.is_cuda:
        raise ValueError("comp_len must be a device int32 tensor")
    n = slots.shape[0]
    if out is None:
        out = torch.empty((n, page_len), dtype=torch.uint8, device=slots.device)
    if rv is None:
        rv = torch.empty((n,), dtype=torch.int32, device=slots.device)
    _check_pages(out, "out")
    cap = max_comp_len if max_comp_len > 0 else slots.shape[1]
    b = _lib.Batch(count=n, src=_ptr(slots), src_lengths=_ptr(comp_len), src_stride=slots.shape[1],
                   max_src_length=min(cap, slots.shape[1]), dst=_ptr(out), dst_stride=out.shape[1],
                   dst_capacity=page_len, results=_ptr(rv))
    if not _zlib_dict_call(False, compressor_id, b, _stream_handle(slots.device), dictionary):
        _decompress_call(compressor_id, b, _stream_handle(slots.device), dictionary)
    return out, rv


def decompress_ragged(stream: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, capacities: torch.Tensor,
                      out: torch.Tensor, out_offsets: torch.Tensor, rv: torch.Tensor, max_src_length: int,
                      max_capacity: int, compressor_id: int = LZ4_COMPRESSOR_ID, dictionary: Lz4Dict | None = None):
    """General form: page i = stream[offsets[i] : offsets[i]+lengths[i]] -> out[out_offsets[i] : +capacities[i]]."""
    b = _lib.Batch(count=offsets.numel(), src=_ptr(stream), src_offsets=_ptr(offsets), src_lengths=_ptr(lengths),
                   max_src_length=max_src_length, dst=_ptr(out), dst_offsets=_ptr(out_offsets),
                   dst_capacities=_ptr(capacities), dst_capacity=max_capacity, results=_ptr(rv))
    if not _zlib_dict_call(False, compressor_id, b, _stream_handle(stream.device), dictionary):
        _decompress_call(compressor_id, b, _stream_handle(stream.device), dictionary)
    return out, rv


def compress_ragged(src: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, out: torch.Tensor,
                    out_offsets: torch.Tensor, capacities: torch.Tensor, results: torch.Tensor, max_src_length: int,
                    compressor_id: int = LZ4_COMPRESSOR_ID, level: int = 1, dictionary: Lz4Dict | None = None):
    """General form of compress_pages.  ``max_src_length`` declares the longest page (0: at most
    65,535 bytes); a longer page gets INT32_MIN.  With LZ4 it may be up to 4 MiB, and in a batch
    that mixes sizes the pages of up to 65,535 bytes get the bytes they would get on their own."""
    b = _lib.Batch(count=offsets.numel(), src=_ptr(src), src_offsets=_ptr(offsets), src_lengths=_ptr(lengths),
                   max_src_length=max_src_length, dst=_ptr(out), dst_offsets=_ptr(out_offsets),
                   dst_capacities=_ptr(capacities), results=_ptr(results))
    if not _zlib_dict_call(True, compressor_id, b, _stream_handle(src.device), dictionary):
        _compress_call(compressor_id, level, b, _stream_handle(src.device), dictionary)
    return out, results


def new_pack_state(device) -> torch.Tensor:
    """A fresh packed store's state: {used, wanted} = {0, 0} (two 64-bit words on the device)."""
    return torch.zeros((2,), dtype=torch.int64, device=device)


def _check_vec(t: torch.Tensor, name: str, dtype, n: int) -> None:
    if not t.is_cuda or t.dtype != dtype or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous device tensor of {n} {dtype} values")


def pack_pages(slots, comp_len: torch.Tensor, arena: torch.Tensor, state: torch.Tensor | None = None, align: int = 16,
               offsets: torch.Tensor | None = None, lengths: torch.Tensor | None = None, max_length: int = 0):
    """Appends the streams of a compress batch to ``arena`` at their compressed size
    (tyche_pack_batch); returns (offsets, lengths, state).

    ``slots`` is the (n, slot) tensor of ``compress_pages`` with ``comp_len`` its results; or, to
    compact a store after evictions, ``(old_arena, offsets)`` with ``comp_len`` the surviving pages'
    lengths.  ``arena`` is a 1-D uint8 device tensor that does not overlap the source.  ``state``
    (two int64 words: used, wanted) is appended to; without one a fresh store is started.  Page i
    went to ``arena[offsets[i] : offsets[i] + lengths[i]]`` iff ``offsets[i] + lengths[i] <= state[0]``
    afterwards; an append that does not fit stores nothing, and every later one into that state is
    refused too, with ``state[1]`` the arena size that would have held everything.  Offsets are int64,
    lengths int32 (the bits of the C API's unsigned values).  Asynchronous on the current stream;
    the decision is made on the device, so appends chain without a host sync.
    """
    if isinstance(slots, (tuple, list)):
        src, src_offsets = slots
        if not src.is_cuda or src.dtype != torch.uint8 or not src.is_contiguous():
            raise ValueError("the source arena must be a contiguous uint8 device tensor")
        n = src_offsets.numel()
        _check_vec(src_offsets, "the source offsets", torch.int64, n)
        stride = 0
    else:
        _check_pages(slots, "slots")
        src, src_offsets, n, stride = slots, None, slots.shape[0], slots.shape[1]
    if not arena.is_cuda or arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise ValueError("arena must be a contiguous 1-D uint8 device tensor")
    _check_vec(comp_len, "comp_len", torch.int32, n)
    if state is None:
        state = new_pack_state(arena.device)
    _check_vec(state, "state", torch.int64, 2)
    if offsets is None:
        offsets = torch.empty((n,), dtype=torch.int64, device=arena.device)
    if lengths is None:
        lengths = torch.empty((n,), dtype=torch.int32, device=arena.device)
    _check_vec(offsets, "offsets", torch.int64, n)
    _check_vec(lengths, "lengths", torch.int32, n)
    p = _lib.Pack(count=n, src=_ptr(src), src_offsets=_ptr(src_offsets) if src_offsets is not None else None,
                  src_stride=stride, results=_ptr(comp_len), max_length=max_length, arena=_ptr(arena),
                  arena_capacity=arena.numel(), align=align, state=_ptr(state), offsets=_ptr(offsets), lengths=_ptr(lengths))
    _lib.check(_lib.load().tyche_pack_batch(ctypes.byref(p), _stream_handle(arena.device)), "tyche_pack_batch")
    return offsets, lengths, state


def decompress_packed(arena: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, page_len: int,
                      compressor_id: int = LZ4_COMPRESSOR_ID, out: torch.Tensor | None = None,
                      rv: torch.Tensor | None = None, max_comp_len: int = 0, dictionary: Lz4Dict | None = None):
    """Decompress page i from ``arena[offsets[i] : offsets[i] + lengths[i]]`` (what ``pack_pages``
    returned) into a page_len row; returns (out, rv) as ``decompress_pages`` does.  One batch with
    src_offsets / src_lengths; ``max_comp_len`` (optional) bounds the lengths for LDS sizing."""
    n = offsets.numel()
    _check_vec(offsets, "offsets", torch.int64, n)
    _check_vec(lengths, "lengths", torch.int32, n)
    if out is None:
        out = torch.empty((n, page_len), dtype=torch.uint8, device=arena.device)
    if rv is None:
        rv = torch.empty((n,), dtype=torch.int32, device=arena.device)
    _check_pages(out, "out")
    b = _lib.Batch(count=n, src=_ptr(arena), src_offsets=_ptr(offsets), src_lengths=_ptr(lengths),
                   max_src_length=max_comp_len, dst=_ptr(out), dst_stride=out.shape[1], dst_capacity=page_len,
                   results=_ptr(rv))
    if not _zlib_dict_call(False, compressor_id, b, _stream_handle(arena.device), dictionary):
        _decompress_call(compressor_id, b, _stream_handle(arena.device), dictionary)
    return out, rv


def compress_pages_packed(pages: torch.Tensor, arena: torch.Tensor, state: torch.Tensor | None = None,
                          chunk_pages: int = 65536, compressor_id: int = LZ4_COMPRESSOR_ID, level: int = 1,
                          align: int = 16, dictionary: Lz4Dict | None = None):
    """``compress_pages`` + ``pack_pages``, ``chunk_pages`` rows at a time through one reused slot
    tensor: beside the arena, a million 16 KiB pages need one chunk's slots (about 1 GiB at the
    default) instead of 17 GB.  Returns (offsets, lengths, state) for all rows, as one ``pack_pages``
    over all of them would.  No host sync inside: every chunk's compress and append are enqueued on
    the current stream, which orders the reuse of the slots."""
    _check_pages(pages, "pages")
    n, page_len = pages.shape
    chunk = max(1, min(int(chunk_pages), max(n, 1)))
    dev = pages.device
    slots = torch.empty((chunk, slot_size(page_len, compressor_id)), dtype=torch.uint8, device=dev)
    clen = torch.empty((chunk,), dtype=torch.int32, device=dev)
    offsets = torch.empty((n,), dtype=torch.int64, device=dev)
    lengths = torch.empty((n,), dtype=torch.int32, device=dev)
    if state is None:
        state = new_pack_state(dev)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        compress_pages(pages[a:b], compressor_id, level, out=slots[:b - a], out_len=clen[:b - a], dictionary=dictionary)
        pack_pages(slots[:b - a], clen[:b - a], arena, state, align, offsets[a:b], lengths[a:b])
    return offsets, lengths, state


def pagegen(n: int, page_len: int, seed: int = 20170303, first: int = 0, dist: int = 0,
            device: torch.device | str = "cuda", out: torch.Tensor | None = None) -> torch.Tensor:
    """Synthetic database pages straight into HBM (tyche_amd/csrc/pagegen.h)."""
    dev = torch.device(device)
    if out is None:
        out = torch.empty((n, page_len), dtype=torch.uint8, device=dev)
    rc = _lib.load().tyche_pagegen(_ptr(out), out.shape[1], page_len, seed, first, n, dist, _stream_handle(dev))
    _lib.check(rc, "tyche_pagegen")
    return out
