#!/usr/bin/env python
"""Record tests/golden/conv1d_dispatch.npz: what the three host-only dispatch queries (sf_op_conv1d_variant, sf_op_conv1d_bwd_variant,
sf_op_conv1d_train_images) answer at every point of the grid of tests/test_conv_gemm_plan_cpu.py.  Nothing is launched: no GPU needed.

    SF_LIB_PATH=/path/to/libsyncfusion_amd.so python tools/record_conv1d_dispatch.py [output.npz]

The library is taken through SF_LIB_PATH (default: the in-tree build).  The committed table is FROZEN at the parent of the change that rebuilt
the dispatcher around one plan per launch (ConvGemmPlan): it was recorded from that parent's library, so that test_conv_gemm_plan_cpu.py
proves the rebuilt dispatcher decides every grid point as the old one did.  Regenerate it only with a change that means to move a threshold
or a tile rule, and say so in that change.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import test_conv_gemm_plan_cpu as T
    from syncfusion_amd import _lib

    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    arrays = T.pack(T.record(_lib.load(), _lib.DTYPES))
    np.savez_compressed(out, **arrays)
    print(f"{out}: {os.path.getsize(out)} bytes, {len(arrays['strings'])} distinct strings, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
