#!/usr/bin/env python3
"""Records tests/golden/lz4_train.npz: the reference encoder's totals (LZ4 1.7.5 from oracle/_ref)
for the ratio conditions of tests/lz4_train_cases.py -- without a dictionary, with the heuristic
dictionary and with the trained one -- and the CRC of the trained dictionary (the specification's,
lz4_train_cases.train_spec) those totals belong to, so that the conditions never depend on that
library being present.  Results only: sizes and checksums.

    python tools/gen_lz4_train_golden.py            # needs oracle/_ref/libtyche_ref.so
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lz4_dict_cases as DC   # noqa: E402
import lz4_train_cases as T   # noqa: E402
from oracle import oracle as O   # noqa: E402


def main():
    if not O.have_ref():
        sys.exit("oracle/_ref/libtyche_ref.so is not built")
    R = DC.Ref(O)
    ratio = []
    for L, dist in T.ratio_keys():
        trained = T.train_spec(T.ratio_training_pages(O, L, dist), T.RATIO_D)
        heur, pages = T.ratio_eval(O, L, dist)
        row = (T.judge(O, R, None, pages), T.judge(O, R, heur, pages), T.judge(O, R, trained, pages), DC.crc(trained))
        ratio.append(row)
        print(f"dist {dist}, {L} B: plain {row[0]}, heuristic {row[1]}, trained {row[2]} ({row[2] / row[1]:.4f})")
    sample = []
    for name, dl in T.sample_sets():
        prefix, train, evalp = T.sample_split(O, name, dl)
        trained = T.train_spec(train, dl)
        row = (T.judge(O, R, prefix, evalp), T.judge(O, R, trained, evalp), DC.crc(trained))
        sample.append(row)
        print(f"{name} D={dl}: first-page prefix {row[0]}, trained {row[1]} ({row[1] / row[0]:.4f})")
    np.savez_compressed(T.GOLDEN_FILE, ratio=np.array(ratio, np.int64), sample=np.array(sample, np.int64))
    print(T.GOLDEN_FILE, os.path.getsize(T.GOLDEN_FILE), "bytes")


if __name__ == "__main__":
    main()
