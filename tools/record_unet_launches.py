#!/usr/bin/env python
"""Record tests/golden/unet_launches.npz: the profiled launch sequence (label, depth, algorithmic flops and bytes per launch) and
launch_count() of one U-Net evaluation per case of tests/test_gpu_unet_launches.py.  Needs the MI355X; the milliseconds are not stored.

    SF_LIB_PATH=/path/to/libsyncfusion_amd.so python tools/record_unet_launches.py [output.npz]

The library is taken through SF_LIB_PATH (default: the in-tree build).  The committed table is FROZEN at the parent of the change that rebuilt
the item path around one plan per item (item_plan): it was recorded from that parent's library, so that test_gpu_unet_launches.py proves the
rebuilt item path issues every launch as the old one did.  Regenerate it only with a change that means to move a launch, and say so in that
change.  The set of labels every case reaches is printed, to be read before the file is committed.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch

    import test_gpu_unet_launches as T
    from syncfusion_amd import _lib

    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    nets = T.Nets(torch.device("cuda:0"))
    results = {}
    for case in T.cases():
        results[T.case_id(case)] = r = T.run_case(nets, case)
        print(f"{T.case_id(case)}: {len(r[0])} launches, launch_count {r[4]}: {' '.join(sorted(set(r[0])))}", flush=True)
    arrays = T.pack(results)
    np.savez_compressed(out, **arrays)
    print(f"{out}: {os.path.getsize(out)} bytes, {len(arrays['cases'])} cases, {len(arrays['label'])} launches, "
          f"{len(arrays['strings'])} distinct labels, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
