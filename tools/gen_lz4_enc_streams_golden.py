"""Writes tests/golden/lz4_enc_streams.npz: the sha256 and the length of every stream the default
LZ4 encoder gives for the batches of tests/lz4_enc_stream_cases.py (benchmark-like pages, a ragged
batch, pages crafted around the split encoder's joints, capacity cases).
tests/test_gpu_lz4_enc_streams.py compresses the same batches and compares: run this with the
encoder whose bytes are the reference (the commit before a change that must keep them), on a GPU.

    python tools/gen_lz4_enc_streams_golden.py [--check] [--out FILE]
    (--check: compare with the fixture, write nothing; --out: write FILE instead of the fixture)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from oracle import oracle as O  # noqa: E402
from tyche_amd import codec  # noqa: E402
import lz4_enc_stream_cases as S  # noqa: E402


def main():
    if not os.path.exists(O.ORACLE_SO):
        O.build(ref=False)
    res = S.run_all(codec, O, torch.device("cuda:0"))
    d = S.digests(res)
    for (name, _, checks), s in zip(S.joint_cases(), res["joint"][2]):
        q = S.sequences(s)
        print(f"joint {name}: {len(s)} bytes, {len(q)} sequences", [(S.joint_of(s, b), lit, ml) for b, lit, ml in checks])
    for g, (_, rv, _) in res.items():
        print(f"{g}: {len(rv)} streams, {sum(max(r, 0) for r in rv)} bytes, results {min(rv)}..{max(rv)}")
    if "--check" in sys.argv:
        g = np.load(S.GOLDEN, allow_pickle=False)
        same = sorted(g.files) == sorted(d) and all(np.array_equal(g[k], d[k]) for k in d)
        print("same as the fixture" if same else "DIFFERS from the fixture")
        sys.exit(0 if same else 1)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else S.GOLDEN
    np.savez_compressed(out, **d)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
