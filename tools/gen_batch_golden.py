"""Record tests/golden/batch/frame_ids.json: the genuine reference's snippet bounds and equally-sampled frame ids (CPU).

    python tools/gen_batch_golden.py

Imports misc/utils.py's own `get_uniform_ids_from_k_snippets` (:311-317) through oracle.ref_import's path handling and calls
it on a list of (length, k) pairs; the bounds are the function's own expression (:313) evaluated beside it.  Stores DATA only:
{"cases": [{"n_total", "n_frames", "bounds", "ids"}, ...]}.  tests/test_batch_cpu.py holds tests/batch_reference.py and
care_amd.clipstore.snippet_bounds to this file.

dataloader.py and misc/utils_corpora.py do not import in this image (h5py, nltk and a downloader are absent), so `_padding` and
the concept labels are pinned by hand-worked cases in the test instead.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "batch", "frame_ids.json")
CASES = [(60, 28), (60, 8), (60, 60), (60, 1), (64, 64), (64, 1), (8, 3), (1, 1), (32, 8), (100, 28), (7, 5), (3, 8), (1, 4)]


def main():
    from oracle import ref_import

    if not ref_import.reference_available():
        raise RuntimeError("reference tree not found at {}".format(ref_import.REFERENCE_ROOT))
    ref_import._stub_modules()
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from misc.utils import get_uniform_ids_from_k_snippets

    cases = []
    for length, k in CASES:
        ids = [int(i) for i in get_uniform_ids_from_k_snippets(length, k)]
        bounds = [int(i) for i in np.linspace(0, length, k + 1)]   # misc/utils.py:313
        cases.append({"n_total": length, "n_frames": k, "bounds": bounds, "ids": ids})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump({"source": "misc/utils.py:311-317 get_uniform_ids_from_k_snippets", "cases": cases}, fh, indent=1)
        fh.write("\n")
    print("{}: {} cases".format(OUT, len(cases)))


if __name__ == "__main__":
    main()
