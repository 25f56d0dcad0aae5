"""bench.py --dump-outputs: the files it writes for given outputs (no GPU: the tensors here are host
tensors, the function only indexes, masks and saves them)."""
import os

import numpy as np
import pytest
import torch

import bench


@pytest.fixture(scope="module")
def outputs():
    """A small stand-in for a step's outputs: n slots with garbage past each stream's end."""
    g = torch.Generator().manual_seed(5)
    n, plen, slot = 3001, 1024, 1040
    out = torch.randint(0, 256, (n, plen), dtype=torch.uint8, generator=g)
    comp = torch.randint(1, 256, (n, slot), dtype=torch.uint8, generator=g)
    clen = torch.randint(1, slot + 1, (n,), dtype=torch.int32, generator=g)
    rv = torch.full((n,), plen, dtype=torch.int32)
    return out, rv, comp, clen


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_files(outputs, tmp_path):
    out, rv, comp, clen = outputs
    written = bench.dump_outputs(str(tmp_path / "a"), 20170303, out, rv, comp, clen)
    got = _load(tmp_path / "a")
    assert sorted(got) == ["clen", "comp_sample", "out_sample", "rv"] == sorted(written)
    assert all(a.dtype == np.float32 for a in got.values())
    assert {k: list(a.shape) for k, a in got.items()} == written
    k = bench.DUMP_SAMPLE_PAGES
    idx = np.sort(np.random.default_rng(20170303).choice(out.shape[0], size=k, replace=False))
    assert np.array_equal(got["rv"], rv.numpy()) and np.array_equal(got["clen"], clen.numpy())
    assert np.array_equal(got["out_sample"], out.numpy()[idx])
    lens = clen.numpy()[idx]
    keep = np.arange(comp.shape[1])[None, :] < lens[:, None]
    assert np.array_equal(got["comp_sample"], comp.numpy()[idx] * keep)   # nothing past a stream's end
    assert (got["comp_sample"][~keep] == 0).all() and (got["comp_sample"][keep] > 0).all()


def test_dump_outputs_repeatable_and_decode_only(outputs, tmp_path):
    out, rv, comp, clen = outputs
    bench.dump_outputs(str(tmp_path / "a"), 7, out, rv, comp, clen)
    comp2 = comp.clone()
    comp2[torch.arange(comp.shape[1])[None, :] >= clen[:, None]] = 0      # other garbage in the slots' tails
    bench.dump_outputs(str(tmp_path / "b"), 7, out, rv, comp2, clen)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    written = bench.dump_outputs(str(tmp_path / "c"), 7, out, rv)         # --config C4: decode only
    c = _load(tmp_path / "c")
    assert sorted(c) == ["out_sample", "rv"] == sorted(written)
    assert np.array_equal(c["out_sample"], a["out_sample"])


def test_dump_outputs_stays_under_64_mb(outputs, tmp_path):
    """The caps by arithmetic, and the page sample shrinking for wide pages."""
    assert 2 * 4 * bench.DUMP_MAX_RESULTS + bench.DUMP_SAMPLE_BYTES <= 64_000_000
    out, rv, comp, clen = outputs
    wide = out[:600].reshape(6, -1)                                        # 6 pages of 100 KiB
    old = bench.DUMP_SAMPLE_BYTES
    bench.DUMP_SAMPLE_BYTES = 4 * wide.shape[1] * 4                       # room for four of them
    try:
        written = bench.dump_outputs(str(tmp_path / "w"), 1, wide, rv[:6])
    finally:
        bench.DUMP_SAMPLE_BYTES = old
    assert written["out_sample"] == [4, wide.shape[1]]
