#!/usr/bin/env python3
"""G18: the submission table from the REFERENCE's utils/utils.py, run on the CPU (build container only).

tests/golden/G18_submission_lut.npz: for CITYSCAPES and ADE20K and every experiment each defines, ``<DATASET>_<experiment>`` =
remap_mask(arange(num_classes), reverse_mapping(CLASS_INFO[experiment][0])) as the reference's save_output computes it
(managers/BaseManager.py:694-696), uint8 [num_classes]; num_classes = the number of network ids, the ignore id included (it is the
last one and maps to 255).  An experiment on which the reference's own code raises under this numpy (CITYSCAPES experiment 0: its
class id -1 does not fit the uint8 table) is left out and reported.  The reference is imported at run time through
tools/ref_shim.py; none of its text is here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()
ref_shim.quiet()
from utils.utils import remap_mask, reverse_mapping  # noqa: E402  (the reference's)
from utils import DATASETS_INFO  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "G18_submission_lut.npz")


def main():
    tables = {}
    for dataset in ("CITYSCAPES", "ADE20K"):
        for experiment, info in enumerate(DATASETS_INFO[dataset].CLASS_INFO):
            num_classes = len(info[1])
            try:
                got = remap_mask(np.arange(num_classes), reverse_mapping(info[0]))
            except OverflowError as e:
                print(f"{dataset}_{experiment}: left out, the reference raises: {e}")
                continue
            assert got.dtype == np.uint8 and got.shape == (num_classes,)
            tables[f"{dataset}_{experiment}"] = got
            print(f"{dataset}_{experiment}: {num_classes} ids, starts {got[:6].tolist()}, ends {got[-2:].tolist()}")
    np.savez_compressed(OUT, **tables)
    print(f"{os.path.basename(OUT)}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
