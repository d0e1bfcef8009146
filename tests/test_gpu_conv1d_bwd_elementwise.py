"""The training backward of the op-level 1-D convolution (sf_op_conv1d_bwd_cl_x, groups = 0), element by element against fp64 on the MI355X,
on every weight-gradient / data-gradient launch path.

test_gpu_train.py gates this backward by a whole-tensor rel-L2 of 2e-5 on shapes that reach few of its paths and never asks which kernel
ran.  Every case here makes ONE call, first asserts that sf_op_conv1d_bwd_variant names the launch plan its row is written for (data-gradient
kernel, weight-gradient kernel and staging, row splits, reducer, column-sum kernel, bias slices -- a literal in the table), then holds every
element of dx, dw and db to one of the two gates of conv1d_bwd_ref.py.  Outputs are NaN-filled before the call, the workspace is filled with
0xFF bytes and is exactly sf_op_conv1d_bwd_workspace_bytes long.  SF_WGRAD_TARGET (a tuning hook that moves the split count) must be unset.

EXACT_CASES (exact gate: non-zero integer operands, device == fp64 reference bit for bit) -- the paths no reference met before:
  * the thin kernel in its three widths, both reducers, the scalar reducer with C % 4 != 0 and with S >= 64, row splits whose trailing slices
    own no rows (they must still write zeros), the bias gradient on the reducer's tail blocks and on its own reduction, every column-sum kernel;
  * both family fallbacks (128-wide -> 64-wide tiles, wide shapes -> the thin kernel) and N % 4 != 0;
  * whole-rows staging of the LDS-staged kernels (halo rows, column tiles straddling taps) at 3, 5, 7 and 9 taps (nr = 40: the edge of the
    LDS window), single-tap staging with a ragged last Q tile, ragged N tiles;
  * clip edges: L = 1, L < taps, clip boundaries inside a 32-row chunk, on a thin, a 64-wide and a 128-wide shape;
  * dx / dw / db left out in turn, on a shape with row splits and on one without;
  * one shape for every (weight-gradient kernel / staging, reducer, column-sum kernel) the dispatcher can reach and for every data-gradient
    label (test_conv1d_bwd_elementwise_cpu.py pins both sets by a sweep of the query).
ROUNDING_CASES (rounding gate: real operands, |dev - ref| <= gamma A with gamma derived in conv1d_bwd_ref.py): the table's shapes of at most
2200 rows, the data gradient alone on the longer shapes whose label nothing shorter reaches (its bound does not grow with the rows), and
dy scaled by 1e-9 and 1e6 on one shape per split kernel.  In the fp32x mode both tables reach every wgrad_x3<TW>/{tap, rows}, data-gradient
labels with "<x3" and without.
"""
import ctypes as C
import os
import time

import pytest
import torch

import conv1d_bwd_ref as R
import numerics as nx
from conv1d_bwd_ref import Case, case_id

pytestmark = pytest.mark.gpu

#        mode, B, L, C, N, taps, outputs asked for (x = dx, w = dw, b = db), expected label[, dy scale]
EXACT_CASES = [
    Case("fp32", 2, 8200, 8, 8, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=64 scalar | db vec4 Sb=8"),   # thin<1,1>, scalar reducer at S = 64, db on the reducer's tail; 7 trailing slices without rows
    Case("fp32", 2, 9000, 6, 8, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=70 scalar | db vec4 Sb=8"),   # C % 4 != 0: scalar reducer at S = 70; 7 trailing slices without rows
    Case("fp32", 2, 300, 6, 8, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 scalar | db vec4 Sb=1"),   # scalar reducer at S = 2
    Case("fp32", 3, 3000, 16, 16, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,2> S=35 vec | db vec4 Sb=8"),   # thin<1,2>, vec reducer; 3 trailing slices without rows
    Case("fp32", 2, 4100, 40, 32, 1, "xwb", "dgrad conv_gemm<f32,64x64> | wgrad_thin<1,2> S=32 vec | db vec4 Sb=16"),   # thin<1,2> at taps = 1; 3 trailing slices without rows
    Case("fp32", 2, 8200, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # thin<1,3>; 7 trailing slices without rows
    Case("fp32", 2, 8200, 33, 17, 3, "wb", "dgrad refused | wgrad_thin<1,3> S=64 scalar | db generic Sb=17"),   # ragged thin tiles, generic column sums; the entry refuses this data gradient: dx = NULL; 7 trailing slices without rows
    Case("fp32", 2, 2050, 96, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_thin<1,3> S=16 vec | db vec4 Sb=16"),   # wide shape falling back to the thin family; 1 trailing slice without rows
    Case("fp32", 2, 1030, 160, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_thin<1,3> S=8 vec | db vec4 Sb=16"),   # wide shape falling back to the thin family
    Case("fp32", 2, 520, 64, 66, 3, "wb", "dgrad refused | wgrad_thin<1,3> S=4 vec | db generic Sb=4"),   # N % 4 != 0: thin family; the entry refuses this data gradient: dx = NULL
    Case("fp32", 5, 333, 32, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/rows S=6 vec | db vec4 Sb=6"),   # 64-wide tiles, whole-rows staging, clip edges inside chunks
    Case("fp32", 2, 600, 32, 64, 9, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<1>/rows S=4 vec | db vec4 Sb=4"),   # whole-rows staging with nr = 40, the edge of the LDS window
    Case("fp32", 2, 1100, 64, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=8 vec | db vec4 Sb=8"),   # single-tap staging at taps = 1
    Case("fp32", 2, 600, 96, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=4 vec | db vec4 Sb=4"),   # single-tap staging, ragged last Q tile (cwid = 32)
    Case("fp32", 4, 2100, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=32 vec | db vec4 Sb=32"),   # C % 64 == 0: single-tap staging, S = 32; 2 trailing slices without rows
    Case("fp32", 2, 600, 128, 68, 3, "wb", "dgrad refused | wgrad_lds<1>/tap S=4 vec | db generic Sb=4"),   # ragged N tile; the entry refuses this data gradient: dx = NULL
    Case("fp32", 2, 1030, 192, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<1>/tap S=8 vec | db vec4 Sb=16"),   # 128-wide tiles falling back to 64-wide
    Case("fp32", 7, 77, 64, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles, whole-rows staging
    Case("fp32", 2, 600, 96, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=4 vec | db vec4 Sb=9"),   # 128-wide tiles, whole-rows staging, column tiles straddling taps
    Case("fp32", 2, 600, 32, 128, 5, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=4 vec | db vec4 Sb=9"),   # 128-wide tiles at 5 taps
    Case("fp32", 2, 300, 32, 128, 9, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles at 9 taps
    Case("fp32", 2, 300, 64, 128, 7, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles at 7 taps
    Case("fp32", 2, 1100, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/tap S=8 vec | db vec4 Sb=17"),   # 128-wide tiles, single-tap staging
    Case("fp32", 3, 700, 256, 256, 3, "xwb", "dgrad conv_gemm_fast<f32,32x32> | wgrad_lds<2>/tap S=8 vec | db vec4 Sb=32"),   # 128-wide tiles, single-tap staging, 2 x 6 tiles
    Case("fp32", 2, 600, 160, 128, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<2>/tap S=4 vec | db vec4 Sb=9"),   # 128-wide tiles at taps = 1, ragged last Q tile
    Case("fp32", 2, 520, 128, 132, 3, "wb", "dgrad refused | wgrad_lds<2>/tap S=4 vec | db generic Sb=8"),   # ragged N tile at 128-wide tiles; the entry refuses this data gradient: dx = NULL
    Case("fp32", 40, 1, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # L = 1: dw of the outer taps is exactly 0
    Case("fp32", 40, 1, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=1 direct | db vec4 Sb=1"),   # L = 1: dw of the outer taps is exactly 0
    Case("fp32", 40, 1, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/tap S=1 direct | db vec4 Sb=1"),   # L = 1: dw of the outer taps is exactly 0
    Case("fp32", 30, 17, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32", 30, 17, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32", 30, 17, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/tap S=1 direct | db vec4 Sb=3"),   # clip boundaries inside a 32-row chunk
    Case("fp32", 3, 31, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32", 3, 31, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32", 3, 31, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32", 1, 33, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32", 1, 33, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32", 1, 33, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/tap S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32", 64, 2, 32, 64, 9, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<1>/rows S=1 direct | db vec4 Sb=1"),   # L < taps
    Case("fp32", 5, 333, 32, 64, 3, "xw", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/rows S=6 vec | db vec4 Sb=6"),   # db = NULL (S > 1)
    Case("fp32", 5, 333, 32, 64, 3, "xb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/rows S=6 vec | db vec4 Sb=6"),   # dw = NULL: db from the standalone slice reduction (S > 1)
    Case("fp32", 5, 333, 32, 64, 3, "wb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/rows S=6 vec | db vec4 Sb=6"),   # dx = NULL (S > 1)
    Case("fp32", 3, 31, 64, 64, 3, "xw", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=1 direct | db vec4 Sb=1"),   # db = NULL (S = 1)
    Case("fp32", 3, 31, 64, 64, 3, "xb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=1 direct | db vec4 Sb=1"),   # dw = NULL: db from the standalone slice reduction (S = 1)
    Case("fp32", 3, 31, 64, 64, 3, "wb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=1 direct | db vec4 Sb=1"),   # dx = NULL (S = 1)
    Case("fp32x", 2, 8200, 8, 8, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=64 scalar | db vec4 Sb=8"),   # thin<1,1>, scalar reducer at S = 64, db on the reducer's tail; 7 trailing slices without rows
    Case("fp32x", 2, 9000, 6, 8, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=70 scalar | db vec4 Sb=8"),   # C % 4 != 0: scalar reducer at S = 70; 7 trailing slices without rows
    Case("fp32x", 2, 300, 6, 8, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 scalar | db vec4 Sb=1"),   # scalar reducer at S = 2
    Case("fp32x", 3, 3000, 16, 16, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,2> S=35 vec | db vec4 Sb=8"),   # thin<1,2>, vec reducer; 3 trailing slices without rows
    Case("fp32x", 2, 4100, 40, 32, 1, "xwb", "dgrad conv_gemm<f32,64x64> | wgrad_thin<1,2> S=32 vec | db vec4 Sb=16"),   # thin<1,2> at taps = 1; 3 trailing slices without rows
    Case("fp32x", 2, 8200, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # thin<1,3>; 7 trailing slices without rows
    Case("fp32x", 2, 8200, 33, 17, 3, "wb", "dgrad refused | wgrad_thin<1,3> S=64 scalar | db generic Sb=17"),   # ragged thin tiles, generic column sums; the entry refuses this data gradient: dx = NULL; 7 trailing slices without rows
    Case("fp32x", 2, 2050, 96, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_thin<1,3> S=16 vec | db vec4 Sb=16"),   # wide shape falling back to the thin family; 1 trailing slice without rows
    Case("fp32x", 2, 1030, 160, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_thin<1,3> S=8 vec | db vec4 Sb=16"),   # wide shape falling back to the thin family
    Case("fp32x", 2, 520, 64, 66, 3, "wb", "dgrad refused | wgrad_thin<1,3> S=4 vec | db generic Sb=4"),   # N % 4 != 0: thin family; the entry refuses this data gradient: dx = NULL
    Case("fp32x", 5, 333, 32, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/rows S=6 vec | db vec4 Sb=6"),   # 64-wide tiles, whole-rows staging, clip edges inside chunks
    Case("fp32x", 2, 600, 32, 64, 9, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<1>/rows S=4 vec | db vec4 Sb=4"),   # whole-rows staging with nr = 40, the edge of the LDS window
    Case("fp32x", 2, 1100, 64, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=8 vec | db vec4 Sb=8"),   # single-tap staging at taps = 1
    Case("fp32x", 2, 600, 96, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=4 vec | db vec4 Sb=4"),   # single-tap staging, ragged last Q tile (cwid = 32)
    Case("fp32x", 4, 2100, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=32 vec | db vec4 Sb=32"),   # C % 64 == 0: single-tap staging, S = 32; 2 trailing slices without rows
    Case("fp32x", 2, 600, 128, 68, 3, "wb", "dgrad refused | wgrad_x3<1>/tap S=4 vec | db generic Sb=4"),   # ragged N tile; the entry refuses this data gradient: dx = NULL
    Case("fp32x", 2, 1030, 192, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<1>/tap S=8 vec | db vec4 Sb=16"),   # 128-wide tiles falling back to 64-wide
    Case("fp32x", 7, 77, 64, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles, whole-rows staging
    Case("fp32x", 2, 600, 96, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=4 vec | db vec4 Sb=9"),   # 128-wide tiles, whole-rows staging, column tiles straddling taps
    Case("fp32x", 2, 600, 32, 128, 5, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=4 vec | db vec4 Sb=9"),   # 128-wide tiles at 5 taps
    Case("fp32x", 2, 300, 32, 128, 9, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles at 9 taps
    Case("fp32x", 2, 300, 64, 128, 7, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles at 7 taps
    Case("fp32x", 2, 1100, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=8 vec | db vec4 Sb=17"),   # 128-wide tiles, single-tap staging
    Case("fp32x", 3, 700, 256, 256, 3, "xwb", "dgrad conv_gemm_fast<x3,32x32> | wgrad_x3<2>/tap S=8 vec | db vec4 Sb=32"),   # 128-wide tiles, single-tap staging, 2 x 6 tiles
    Case("fp32x", 2, 600, 160, 128, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<2>/tap S=4 vec | db vec4 Sb=9"),   # 128-wide tiles at taps = 1, ragged last Q tile
    Case("fp32x", 2, 520, 128, 132, 3, "wb", "dgrad refused | wgrad_x3<2>/tap S=4 vec | db generic Sb=8"),   # ragged N tile at 128-wide tiles; the entry refuses this data gradient: dx = NULL
    Case("fp32x", 40, 1, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # L = 1: dw of the outer taps is exactly 0
    Case("fp32x", 40, 1, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=1 direct | db vec4 Sb=1"),   # L = 1: dw of the outer taps is exactly 0
    Case("fp32x", 40, 1, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=1 direct | db vec4 Sb=1"),   # L = 1: dw of the outer taps is exactly 0
    Case("fp32x", 30, 17, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32x", 30, 17, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32x", 30, 17, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=1 direct | db vec4 Sb=3"),   # clip boundaries inside a 32-row chunk
    Case("fp32x", 3, 31, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32x", 3, 31, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32x", 3, 31, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32x", 1, 33, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32x", 1, 33, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32x", 1, 33, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32x", 64, 2, 32, 64, 9, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<1>/rows S=1 direct | db vec4 Sb=1"),   # L < taps
    Case("fp32x", 5, 333, 32, 64, 3, "xw", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/rows S=6 vec | db vec4 Sb=6"),   # db = NULL (S > 1)
    Case("fp32x", 5, 333, 32, 64, 3, "xb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/rows S=6 vec | db vec4 Sb=6"),   # dw = NULL: db from the standalone slice reduction (S > 1)
    Case("fp32x", 5, 333, 32, 64, 3, "wb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/rows S=6 vec | db vec4 Sb=6"),   # dx = NULL (S > 1)
    Case("fp32x", 3, 31, 64, 64, 3, "xw", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=1 direct | db vec4 Sb=1"),   # db = NULL (S = 1)
    Case("fp32x", 3, 31, 64, 64, 3, "xb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=1 direct | db vec4 Sb=1"),   # dw = NULL: db from the standalone slice reduction (S = 1)
    Case("fp32x", 3, 31, 64, 64, 3, "wb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=1 direct | db vec4 Sb=1"),   # dx = NULL (S = 1)
    Case("fp32", 1, 33, 32, 68, 3, "xwb", "dgrad conv_direct | wgrad_lds<1>/rows S=1 direct | db generic Sb=1"),   # reaches wgrad_lds<1>/rows direct | db generic
    Case("fp32", 2, 8200, 32, 68, 3, "xwb", "dgrad conv_direct | wgrad_lds<1>/rows S=64 scalar | db generic Sb=68"),   # reaches wgrad_lds<1>/rows scalar | db generic; 7 trailing slices without rows
    Case("fp32", 2, 8200, 32, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/rows S=64 scalar | db vec4 Sb=64"),   # reaches wgrad_lds<1>/rows scalar | db vec4; 7 trailing slices without rows
    Case("fp32", 2, 300, 32, 68, 3, "xwb", "dgrad conv_direct | wgrad_lds<1>/rows S=2 vec | db generic Sb=2"),   # reaches wgrad_lds<1>/rows vec | db generic
    Case("fp32", 1, 33, 64, 68, 1, "wb", "dgrad refused | wgrad_lds<1>/tap S=1 direct | db generic Sb=1"),   # reaches wgrad_lds<1>/tap direct | db generic
    Case("fp32", 2, 8200, 64, 68, 1, "wb", "dgrad refused | wgrad_lds<1>/tap S=64 scalar | db generic Sb=68"),   # reaches wgrad_lds<1>/tap scalar | db generic; 7 trailing slices without rows
    Case("fp32", 2, 8200, 64, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=64 scalar | db vec4 Sb=64"),   # reaches wgrad_lds<1>/tap scalar | db vec4; 7 trailing slices without rows
    Case("fp32", 1, 33, 32, 132, 5, "wb", "dgrad refused | wgrad_lds<2>/rows S=1 direct | db generic Sb=1"),   # reaches wgrad_lds<2>/rows direct | db generic
    Case("fp32", 1, 33, 32, 128, 5, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=1 direct | db vec4 Sb=1"),   # reaches wgrad_lds<2>/rows direct | db vec4
    Case("fp32", 2, 8200, 32, 132, 5, "wb", "dgrad refused | wgrad_lds<2>/rows S=64 scalar | db generic Sb=132"),   # reaches wgrad_lds<2>/rows scalar | db generic; 7 trailing slices without rows
    Case("fp32", 2, 8200, 32, 128, 5, "xwb", "dgrad conv_gemm_sk<f32,32x32> | wgrad_lds<2>/rows S=64 scalar | db vec4 Sb=128"),   # reaches wgrad_lds<2>/rows scalar | db vec4; 7 trailing slices without rows
    Case("fp32", 2, 300, 32, 132, 5, "wb", "dgrad refused | wgrad_lds<2>/rows S=2 vec | db generic Sb=4"),   # reaches wgrad_lds<2>/rows vec | db generic
    Case("fp32", 1, 33, 128, 132, 1, "wb", "dgrad refused | wgrad_lds<2>/tap S=1 direct | db generic Sb=1"),   # reaches wgrad_lds<2>/tap direct | db generic
    Case("fp32", 2, 8200, 128, 132, 1, "wb", "dgrad refused | wgrad_lds<2>/tap S=64 scalar | db generic Sb=132"),   # reaches wgrad_lds<2>/tap scalar | db generic; 7 trailing slices without rows
    Case("fp32", 2, 8200, 128, 128, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<2>/tap S=64 scalar | db vec4 Sb=128"),   # reaches wgrad_lds<2>/tap scalar | db vec4; 7 trailing slices without rows
    Case("fp32", 1, 33, 1, 6, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=1 direct | db generic Sb=1"),   # reaches wgrad_thin<1,1> direct | db generic
    Case("fp32", 1, 33, 1, 1, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=1 direct | db vec1 Sb=1"),   # reaches wgrad_thin<1,1> direct | db vec1
    Case("fp32", 1, 33, 1, 8, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=1 direct | db vec4 Sb=1"),   # reaches wgrad_thin<1,1> direct | db vec4
    Case("fp32", 2, 300, 1, 6, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 scalar | db generic Sb=1"),   # reaches wgrad_thin<1,1> scalar | db generic
    Case("fp32", 2, 300, 1, 1, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 scalar | db vec1 Sb=1"),   # reaches wgrad_thin<1,1> scalar | db vec1
    Case("fp32", 2, 300, 8, 6, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 vec | db generic Sb=1"),   # reaches wgrad_thin<1,1> vec | db generic
    Case("fp32", 2, 300, 8, 1, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 vec | db vec1 Sb=1"),   # reaches wgrad_thin<1,1> vec | db vec1
    Case("fp32", 2, 300, 8, 8, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 vec | db vec4 Sb=1"),   # reaches wgrad_thin<1,1> vec | db vec4
    Case("fp32", 1, 33, 33, 6, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=1 direct | db generic Sb=1"),   # reaches wgrad_thin<1,2> direct | db generic
    Case("fp32", 1, 33, 33, 1, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=1 direct | db vec1 Sb=1"),   # reaches wgrad_thin<1,2> direct | db vec1
    Case("fp32", 1, 33, 33, 8, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=1 direct | db vec4 Sb=1"),   # reaches wgrad_thin<1,2> direct | db vec4
    Case("fp32", 2, 300, 33, 6, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=2 scalar | db generic Sb=1"),   # reaches wgrad_thin<1,2> scalar | db generic
    Case("fp32", 2, 300, 33, 1, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=2 scalar | db vec1 Sb=1"),   # reaches wgrad_thin<1,2> scalar | db vec1
    Case("fp32", 2, 300, 33, 8, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=2 scalar | db vec4 Sb=1"),   # reaches wgrad_thin<1,2> scalar | db vec4
    Case("fp32", 2, 300, 8, 6, 5, "xwb", "dgrad conv_direct | wgrad_thin<1,2> S=2 vec | db generic Sb=1"),   # reaches wgrad_thin<1,2> vec | db generic
    Case("fp32", 2, 300, 8, 1, 5, "xwb", "dgrad conv_direct | wgrad_thin<1,2> S=2 vec | db vec1 Sb=1"),   # reaches wgrad_thin<1,2> vec | db vec1
    Case("fp32", 1, 33, 66, 6, 1, "wb", "dgrad refused | wgrad_thin<1,3> S=1 direct | db generic Sb=1"),   # reaches wgrad_thin<1,3> direct | db generic
    Case("fp32", 1, 33, 66, 1, 1, "wb", "dgrad refused | wgrad_thin<1,3> S=1 direct | db vec1 Sb=1"),   # reaches wgrad_thin<1,3> direct | db vec1
    Case("fp32", 2, 300, 66, 1, 1, "wb", "dgrad refused | wgrad_thin<1,3> S=2 scalar | db vec1 Sb=1"),   # reaches wgrad_thin<1,3> scalar | db vec1
    Case("fp32", 2, 300, 68, 1, 1, "wb", "dgrad refused | wgrad_thin<1,3> S=2 vec | db vec1 Sb=1"),   # reaches wgrad_thin<1,3> vec | db vec1
    Case("fp32x", 1, 33, 1, 6, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=1 direct | db generic Sb=1"),   # reaches wgrad_thin<1,1> direct | db generic
    Case("fp32x", 1, 33, 1, 1, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=1 direct | db vec1 Sb=1"),   # reaches wgrad_thin<1,1> direct | db vec1
    Case("fp32x", 1, 33, 1, 8, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=1 direct | db vec4 Sb=1"),   # reaches wgrad_thin<1,1> direct | db vec4
    Case("fp32x", 2, 300, 1, 6, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 scalar | db generic Sb=1"),   # reaches wgrad_thin<1,1> scalar | db generic
    Case("fp32x", 2, 300, 1, 1, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 scalar | db vec1 Sb=1"),   # reaches wgrad_thin<1,1> scalar | db vec1
    Case("fp32x", 2, 300, 8, 6, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 vec | db generic Sb=1"),   # reaches wgrad_thin<1,1> vec | db generic
    Case("fp32x", 2, 300, 8, 1, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 vec | db vec1 Sb=1"),   # reaches wgrad_thin<1,1> vec | db vec1
    Case("fp32x", 2, 300, 8, 8, 1, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 vec | db vec4 Sb=1"),   # reaches wgrad_thin<1,1> vec | db vec4
    Case("fp32x", 1, 33, 33, 6, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=1 direct | db generic Sb=1"),   # reaches wgrad_thin<1,2> direct | db generic
    Case("fp32x", 1, 33, 33, 1, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=1 direct | db vec1 Sb=1"),   # reaches wgrad_thin<1,2> direct | db vec1
    Case("fp32x", 1, 33, 33, 8, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=1 direct | db vec4 Sb=1"),   # reaches wgrad_thin<1,2> direct | db vec4
    Case("fp32x", 2, 300, 33, 6, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=2 scalar | db generic Sb=1"),   # reaches wgrad_thin<1,2> scalar | db generic
    Case("fp32x", 2, 300, 33, 1, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=2 scalar | db vec1 Sb=1"),   # reaches wgrad_thin<1,2> scalar | db vec1
    Case("fp32x", 2, 300, 33, 8, 1, "wb", "dgrad refused | wgrad_thin<1,2> S=2 scalar | db vec4 Sb=1"),   # reaches wgrad_thin<1,2> scalar | db vec4
    Case("fp32x", 2, 300, 8, 6, 5, "xwb", "dgrad conv_direct | wgrad_thin<1,2> S=2 vec | db generic Sb=1"),   # reaches wgrad_thin<1,2> vec | db generic
    Case("fp32x", 2, 300, 8, 1, 5, "xwb", "dgrad conv_direct | wgrad_thin<1,2> S=2 vec | db vec1 Sb=1"),   # reaches wgrad_thin<1,2> vec | db vec1
    Case("fp32x", 1, 33, 66, 6, 1, "wb", "dgrad refused | wgrad_thin<1,3> S=1 direct | db generic Sb=1"),   # reaches wgrad_thin<1,3> direct | db generic
    Case("fp32x", 1, 33, 66, 1, 1, "wb", "dgrad refused | wgrad_thin<1,3> S=1 direct | db vec1 Sb=1"),   # reaches wgrad_thin<1,3> direct | db vec1
    Case("fp32x", 2, 300, 66, 1, 1, "wb", "dgrad refused | wgrad_thin<1,3> S=2 scalar | db vec1 Sb=1"),   # reaches wgrad_thin<1,3> scalar | db vec1
    Case("fp32x", 2, 300, 68, 1, 1, "wb", "dgrad refused | wgrad_thin<1,3> S=2 vec | db vec1 Sb=1"),   # reaches wgrad_thin<1,3> vec | db vec1
    Case("fp32x", 1, 33, 32, 68, 3, "xwb", "dgrad conv_direct | wgrad_x3<1>/rows S=1 direct | db generic Sb=1"),   # reaches wgrad_x3<1>/rows direct | db generic
    Case("fp32x", 2, 8200, 32, 68, 3, "xwb", "dgrad conv_direct | wgrad_x3<1>/rows S=64 scalar | db generic Sb=68"),   # reaches wgrad_x3<1>/rows scalar | db generic; 7 trailing slices without rows
    Case("fp32x", 2, 8200, 32, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/rows S=64 scalar | db vec4 Sb=64"),   # reaches wgrad_x3<1>/rows scalar | db vec4; 7 trailing slices without rows
    Case("fp32x", 2, 300, 32, 68, 3, "xwb", "dgrad conv_direct | wgrad_x3<1>/rows S=2 vec | db generic Sb=2"),   # reaches wgrad_x3<1>/rows vec | db generic
    Case("fp32x", 1, 33, 64, 68, 1, "wb", "dgrad refused | wgrad_x3<1>/tap S=1 direct | db generic Sb=1"),   # reaches wgrad_x3<1>/tap direct | db generic
    Case("fp32x", 2, 8200, 64, 68, 1, "wb", "dgrad refused | wgrad_x3<1>/tap S=64 scalar | db generic Sb=68"),   # reaches wgrad_x3<1>/tap scalar | db generic; 7 trailing slices without rows
    Case("fp32x", 2, 8200, 64, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=64 scalar | db vec4 Sb=64"),   # reaches wgrad_x3<1>/tap scalar | db vec4; 7 trailing slices without rows
    Case("fp32x", 1, 33, 32, 132, 5, "wb", "dgrad refused | wgrad_x3<2>/rows S=1 direct | db generic Sb=1"),   # reaches wgrad_x3<2>/rows direct | db generic
    Case("fp32x", 1, 33, 32, 128, 5, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=1 direct | db vec4 Sb=1"),   # reaches wgrad_x3<2>/rows direct | db vec4
    Case("fp32x", 2, 8200, 32, 132, 5, "wb", "dgrad refused | wgrad_x3<2>/rows S=64 scalar | db generic Sb=132"),   # reaches wgrad_x3<2>/rows scalar | db generic; 7 trailing slices without rows
    Case("fp32x", 2, 8200, 32, 128, 5, "xwb", "dgrad conv_gemm_mt<x3> | wgrad_x3<2>/rows S=64 scalar | db vec4 Sb=128"),   # reaches wgrad_x3<2>/rows scalar | db vec4; 7 trailing slices without rows
    Case("fp32x", 2, 300, 32, 132, 5, "wb", "dgrad refused | wgrad_x3<2>/rows S=2 vec | db generic Sb=4"),   # reaches wgrad_x3<2>/rows vec | db generic
    Case("fp32x", 1, 33, 128, 132, 1, "wb", "dgrad refused | wgrad_x3<2>/tap S=1 direct | db generic Sb=1"),   # reaches wgrad_x3<2>/tap direct | db generic
    Case("fp32x", 2, 8200, 128, 132, 1, "wb", "dgrad refused | wgrad_x3<2>/tap S=64 scalar | db generic Sb=132"),   # reaches wgrad_x3<2>/tap scalar | db generic; 7 trailing slices without rows
    Case("fp32x", 2, 8200, 128, 128, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<2>/tap S=64 scalar | db vec4 Sb=128"),   # reaches wgrad_x3<2>/tap scalar | db vec4; 7 trailing slices without rows
    Case("fp32", 2, 8200, 512, 32, 1, "xwb", "dgrad conv_gemm<f32,128x128> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # data gradient through conv_gemm<f32,128x128>; 7 trailing slices without rows
    Case("fp32", 2, 8200, 132, 32, 1, "xwb", "dgrad conv_gemm<f32,128x64> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # data gradient through conv_gemm<f32,128x64>; 7 trailing slices without rows
    Case("fp32", 2, 8200, 96, 256, 1, "xwb", "dgrad conv_gemm_mt<f32> | wgrad_lds<1>/tap S=64 scalar | db vec4 Sb=256"),   # data gradient through conv_gemm_mt<f32>; 7 trailing slices without rows
    Case("fp32", 2, 8200, 512, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,128x128> | wgrad_lds<1>/tap S=64 scalar | db vec4 Sb=64"),   # data gradient through conv_gemm_v2<f32,128x128>; 7 trailing slices without rows
    Case("fp32x", 2, 8200, 512, 32, 1, "xwb", "dgrad conv_gemm<f32,128x128> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # data gradient through conv_gemm<f32,128x128>; 7 trailing slices without rows
    Case("fp32x", 2, 8200, 132, 32, 1, "xwb", "dgrad conv_gemm<f32,128x64> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # data gradient through conv_gemm<f32,128x64>; 7 trailing slices without rows
    Case("fp32x", 1, 33, 1, 32, 9, "xwb", "dgrad conv_gemm_sk<f32,32x32> | wgrad_thin<1,1> S=1 direct | db vec4 Sb=1"),   # data gradient through conv_gemm_sk<f32,32x32>
    Case("fp32x", 2, 8200, 512, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,128x128> | wgrad_x3<1>/tap S=64 scalar | db vec4 Sb=64"),   # data gradient through conv_gemm_v2<f32,128x128>; 7 trailing slices without rows
]

ROUNDING_CASES = [
    Case("fp32", 2, 300, 6, 8, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 scalar | db vec4 Sb=1"),   # scalar reducer at S = 2
    Case("fp32", 2, 1030, 160, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_thin<1,3> S=8 vec | db vec4 Sb=16"),   # wide shape falling back to the thin family
    Case("fp32", 2, 520, 64, 66, 3, "wb", "dgrad refused | wgrad_thin<1,3> S=4 vec | db generic Sb=4"),   # N % 4 != 0: thin family; the entry refuses this data gradient: dx = NULL
    Case("fp32", 5, 333, 32, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/rows S=6 vec | db vec4 Sb=6"),   # 64-wide tiles, whole-rows staging, clip edges inside chunks
    Case("fp32", 2, 600, 32, 64, 9, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<1>/rows S=4 vec | db vec4 Sb=4"),   # whole-rows staging with nr = 40, the edge of the LDS window
    Case("fp32", 2, 1100, 64, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=8 vec | db vec4 Sb=8"),   # single-tap staging at taps = 1
    Case("fp32", 2, 600, 96, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=4 vec | db vec4 Sb=4"),   # single-tap staging, ragged last Q tile (cwid = 32)
    Case("fp32", 2, 600, 128, 68, 3, "wb", "dgrad refused | wgrad_lds<1>/tap S=4 vec | db generic Sb=4"),   # ragged N tile; the entry refuses this data gradient: dx = NULL
    Case("fp32", 2, 1030, 192, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<1>/tap S=8 vec | db vec4 Sb=16"),   # 128-wide tiles falling back to 64-wide
    Case("fp32", 7, 77, 64, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles, whole-rows staging
    Case("fp32", 2, 600, 96, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=4 vec | db vec4 Sb=9"),   # 128-wide tiles, whole-rows staging, column tiles straddling taps
    Case("fp32", 2, 600, 32, 128, 5, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=4 vec | db vec4 Sb=9"),   # 128-wide tiles at 5 taps
    Case("fp32", 2, 300, 32, 128, 9, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles at 9 taps
    Case("fp32", 2, 300, 64, 128, 7, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles at 7 taps
    Case("fp32", 2, 1100, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/tap S=8 vec | db vec4 Sb=17"),   # 128-wide tiles, single-tap staging
    Case("fp32", 3, 700, 256, 256, 3, "xwb", "dgrad conv_gemm_fast<f32,32x32> | wgrad_lds<2>/tap S=8 vec | db vec4 Sb=32"),   # 128-wide tiles, single-tap staging, 2 x 6 tiles
    Case("fp32", 2, 600, 160, 128, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<2>/tap S=4 vec | db vec4 Sb=9"),   # 128-wide tiles at taps = 1, ragged last Q tile
    Case("fp32", 2, 520, 128, 132, 3, "wb", "dgrad refused | wgrad_lds<2>/tap S=4 vec | db generic Sb=8"),   # ragged N tile at 128-wide tiles; the entry refuses this data gradient: dx = NULL
    Case("fp32", 3, 31, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32", 3, 31, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32", 3, 31, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32", 1, 33, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32", 1, 33, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_lds<1>/tap S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32", 1, 33, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<f32,32x32> | wgrad_lds<2>/tap S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32x", 2, 300, 6, 8, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,1> S=2 scalar | db vec4 Sb=1"),   # scalar reducer at S = 2
    Case("fp32x", 2, 1030, 160, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_thin<1,3> S=8 vec | db vec4 Sb=16"),   # wide shape falling back to the thin family
    Case("fp32x", 2, 520, 64, 66, 3, "wb", "dgrad refused | wgrad_thin<1,3> S=4 vec | db generic Sb=4"),   # N % 4 != 0: thin family; the entry refuses this data gradient: dx = NULL
    Case("fp32x", 5, 333, 32, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/rows S=6 vec | db vec4 Sb=6"),   # 64-wide tiles, whole-rows staging, clip edges inside chunks
    Case("fp32x", 2, 600, 32, 64, 9, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<1>/rows S=4 vec | db vec4 Sb=4"),   # whole-rows staging with nr = 40, the edge of the LDS window
    Case("fp32x", 2, 1100, 64, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=8 vec | db vec4 Sb=8"),   # single-tap staging at taps = 1
    Case("fp32x", 2, 600, 96, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=4 vec | db vec4 Sb=4"),   # single-tap staging, ragged last Q tile (cwid = 32)
    Case("fp32x", 2, 600, 128, 68, 3, "wb", "dgrad refused | wgrad_x3<1>/tap S=4 vec | db generic Sb=4"),   # ragged N tile; the entry refuses this data gradient: dx = NULL
    Case("fp32x", 2, 1030, 192, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<1>/tap S=8 vec | db vec4 Sb=16"),   # 128-wide tiles falling back to 64-wide
    Case("fp32x", 7, 77, 64, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles, whole-rows staging
    Case("fp32x", 2, 600, 96, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=4 vec | db vec4 Sb=9"),   # 128-wide tiles, whole-rows staging, column tiles straddling taps
    Case("fp32x", 2, 600, 32, 128, 5, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=4 vec | db vec4 Sb=9"),   # 128-wide tiles at 5 taps
    Case("fp32x", 2, 300, 32, 128, 9, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles at 9 taps
    Case("fp32x", 2, 300, 64, 128, 7, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=2 vec | db vec4 Sb=4"),   # 128-wide tiles at 7 taps
    Case("fp32x", 2, 1100, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=8 vec | db vec4 Sb=17"),   # 128-wide tiles, single-tap staging
    Case("fp32x", 3, 700, 256, 256, 3, "xwb", "dgrad conv_gemm_fast<x3,32x32> | wgrad_x3<2>/tap S=8 vec | db vec4 Sb=32"),   # 128-wide tiles, single-tap staging, 2 x 6 tiles
    Case("fp32x", 2, 600, 160, 128, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<2>/tap S=4 vec | db vec4 Sb=9"),   # 128-wide tiles at taps = 1, ragged last Q tile
    Case("fp32x", 2, 520, 128, 132, 3, "wb", "dgrad refused | wgrad_x3<2>/tap S=4 vec | db generic Sb=8"),   # ragged N tile at 128-wide tiles; the entry refuses this data gradient: dx = NULL
    Case("fp32x", 3, 31, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32x", 3, 31, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32x", 3, 31, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=1 direct | db vec4 Sb=1"),   # clip boundaries inside a 32-row chunk
    Case("fp32x", 1, 33, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32x", 1, 33, 64, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32x", 1, 33, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=1 direct | db vec4 Sb=1"),   # one clip, a ragged second chunk
    Case("fp32", 2, 600, 16, 16, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,2> S=4 vec | db vec4 Sb=1"),   # thin<1,2> with row splits
    Case("fp32", 2, 600, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=4 vec | db vec4 Sb=2"),   # thin<1,3> with row splits
    Case("fp32x", 2, 600, 16, 16, 3, "xwb", "dgrad conv_direct | wgrad_thin<1,2> S=4 vec | db vec4 Sb=1"),   # thin<1,2> with row splits
    Case("fp32x", 2, 600, 32, 32, 3, "xwb", "dgrad conv_gemm<f32,128x32> | wgrad_thin<1,3> S=4 vec | db vec4 Sb=2"),   # thin<1,3> with row splits
    Case("fp32", 2, 4100, 40, 32, 1, "x", "dgrad conv_gemm<f32,64x64> | wgrad_thin<1,2> S=32 vec | db vec4 Sb=16"),   # data gradient alone through conv_gemm<f32,64x64> (its bound does not grow with the rows); 3 trailing slices without rows
    Case("fp32x", 2, 4100, 40, 32, 1, "x", "dgrad conv_gemm<f32,64x64> | wgrad_thin<1,2> S=32 vec | db vec4 Sb=16"),   # data gradient alone through conv_gemm<f32,64x64> (its bound does not grow with the rows); 3 trailing slices without rows
    Case("fp32", 2, 8200, 32, 128, 5, "x", "dgrad conv_gemm_sk<f32,32x32> | wgrad_lds<2>/rows S=64 scalar | db vec4 Sb=128"),   # data gradient alone through conv_gemm_sk<f32,32x32> (its bound does not grow with the rows); 7 trailing slices without rows
    Case("fp32x", 2, 8200, 32, 128, 5, "x", "dgrad conv_gemm_mt<x3> | wgrad_x3<2>/rows S=64 scalar | db vec4 Sb=128"),   # data gradient alone through conv_gemm_mt<x3> (its bound does not grow with the rows); 7 trailing slices without rows
    Case("fp32", 2, 8200, 512, 32, 1, "x", "dgrad conv_gemm<f32,128x128> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # data gradient alone through conv_gemm<f32,128x128> (its bound does not grow with the rows); 7 trailing slices without rows
    Case("fp32", 2, 8200, 132, 32, 1, "x", "dgrad conv_gemm<f32,128x64> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # data gradient alone through conv_gemm<f32,128x64> (its bound does not grow with the rows); 7 trailing slices without rows
    Case("fp32", 2, 8200, 96, 256, 1, "x", "dgrad conv_gemm_mt<f32> | wgrad_lds<1>/tap S=64 scalar | db vec4 Sb=256"),   # data gradient alone through conv_gemm_mt<f32> (its bound does not grow with the rows); 7 trailing slices without rows
    Case("fp32", 2, 8200, 512, 64, 1, "x", "dgrad conv_gemm_v2<f32,128x128> | wgrad_lds<1>/tap S=64 scalar | db vec4 Sb=64"),   # data gradient alone through conv_gemm_v2<f32,128x128> (its bound does not grow with the rows); 7 trailing slices without rows
    Case("fp32x", 2, 8200, 512, 32, 1, "x", "dgrad conv_gemm<f32,128x128> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # data gradient alone through conv_gemm<f32,128x128> (its bound does not grow with the rows); 7 trailing slices without rows
    Case("fp32x", 2, 8200, 132, 32, 1, "x", "dgrad conv_gemm<f32,128x64> | wgrad_thin<1,3> S=64 scalar | db vec4 Sb=32"),   # data gradient alone through conv_gemm<f32,128x64> (its bound does not grow with the rows); 7 trailing slices without rows
    Case("fp32x", 1, 33, 1, 32, 9, "x", "dgrad conv_gemm_sk<f32,32x32> | wgrad_thin<1,1> S=1 direct | db vec4 Sb=1"),   # data gradient alone through conv_gemm_sk<f32,32x32> (its bound does not grow with the rows)
    Case("fp32x", 2, 8200, 512, 64, 1, "x", "dgrad conv_gemm_v2<f32,128x128> | wgrad_x3<1>/tap S=64 scalar | db vec4 Sb=64"),   # data gradient alone through conv_gemm_v2<f32,128x128> (its bound does not grow with the rows); 7 trailing slices without rows
    Case("fp32x", 5, 333, 32, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/rows S=6 vec | db vec4 Sb=6", 1e-09),   # dy x 1e-09
    Case("fp32x", 5, 333, 32, 64, 3, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/rows S=6 vec | db vec4 Sb=6", 1e+06),   # dy x 1e+06
    Case("fp32x", 2, 1100, 64, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=8 vec | db vec4 Sb=8", 1e-09),   # dy x 1e-09
    Case("fp32x", 2, 1100, 64, 64, 1, "xwb", "dgrad conv_gemm_v2<f32,64x64> | wgrad_x3<1>/tap S=8 vec | db vec4 Sb=8", 1e+06),   # dy x 1e+06
    Case("fp32x", 7, 77, 64, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=2 vec | db vec4 Sb=4", 1e-09),   # dy x 1e-09
    Case("fp32x", 7, 77, 64, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/rows S=2 vec | db vec4 Sb=4", 1e+06),   # dy x 1e+06
    Case("fp32x", 2, 1100, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=8 vec | db vec4 Sb=17", 1e-09),   # dy x 1e-09
    Case("fp32x", 2, 1100, 128, 128, 3, "xwb", "dgrad conv_gemm_wp<x3,32x32> | wgrad_x3<2>/tap S=8 vec | db vec4 Sb=17", 1e+06),   # dy x 1e+06
]


def variant(lib, _l, c: Case) -> str:
    """The launch plan sf_op_conv1d_bwd_cl_x makes for this case (query only)."""
    buf = C.create_string_buffer(160)
    _l.check(lib.sf_op_conv1d_bwd_variant(_l.DTYPES[c.mode], c.B, c.L, c.C, c.N, c.taps, c.pad, buf, 160), "sf_op_conv1d_bwd_variant")
    return buf.value.decode()


_spent = {"seconds": 0.0, "cases": 0, "worst": {}}


@pytest.fixture(scope="module", autouse=True)
def _total():
    assert "SF_WGRAD_TARGET" not in os.environ, "SF_WGRAD_TARGET moves the split count: the labels of the tables are written for the default"
    yield
    worst = ", ".join(f"{k} {r:.3f}" for k, r in sorted(_spent["worst"].items()))
    print(f"\nconv1d backward element-wise gates: {_spent['cases']} cases in {_spent['seconds']:.1f} s; worst rounding-gate err/bound: {worst}")


def _run(cuda, c: Case, ops):
    """One call of the entry on NaN-filled outputs and a poisoned workspace of exactly the advertised size -> ({which: tensor}, label)."""
    from syncfusion_amd import _lib as _l

    lib = _l.load()
    x, w, dy = (t.to(cuda) for t in ops)
    out = {}
    if "x" in c.outs:
        out["dx"] = nx.nan_like((c.B, c.L, c.C), torch.float32, cuda)
    if "w" in c.outs:
        out["dw"] = nx.nan_like((c.N, c.C, c.taps), torch.float32, cuda)
    if "b" in c.outs:
        out["db"] = nx.nan_like((c.N,), torch.float32, cuda)
    n = int(lib.sf_op_conv1d_bwd_workspace_bytes(c.B, c.L, c.C, c.N, c.taps, 0))
    assert n > 0
    ws = nx.poisoned_workspace(n, cuda)
    assert ws.numel() == n
    label = variant(lib, _l, c)
    assert label == c.expected_label, f"{case_id(c)}: the dispatcher plans {label!r}, the row is written for {c.expected_label!r}"
    ptr = lambda k: out[k].data_ptr() if k in out else None   # noqa: E731
    _l.check(lib.sf_op_conv1d_bwd_cl_x(_l.DTYPES[c.mode], x.data_ptr(), None, None, w.data_ptr(), None, None, 0, 0.0, dy.data_ptr(), c.B, c.L, c.C, c.N,
                                       c.taps, c.pad, ptr("dx"), ptr("dw"), ptr("db"), None, ws.data_ptr(), n, _l.stream_ptr(cuda)), "sf_op_conv1d_bwd_cl_x")
    return out, label


@pytest.mark.parametrize("case", EXACT_CASES, ids=case_id)
def test_conv1d_bwd_exact(cuda, case):
    t0 = time.time()
    ops = R.exact_operands(case)
    out, label = _run(cuda, case, ops)
    refs = R.references(case, ops)                                             # on the CPU while the launches run
    torch.cuda.synchronize()
    for which, (ref, A) in refs.items():
        R.exact_gate(out[which].cpu(), ref, A, which, case_id(case), label)
    dt = time.time() - t0
    _spent["seconds"] += dt
    _spent["cases"] += 1
    print(f"{label}: {', '.join(refs)} bit-equal to fp64, {dt:.2f} s")


@pytest.mark.parametrize("case", ROUNDING_CASES, ids=case_id)
def test_conv1d_bwd_rounding(cuda, case):
    t0 = time.time()
    ops = R.operands(case)
    out, label = _run(cuda, case, ops)
    refs = R.references(case, ops)
    gam = R.gammas(case, R.parse(label))
    torch.cuda.synchronize()
    said = []
    for which, (ref, A) in refs.items():
        r = R.rounding_gate(out[which].cpu(), ref, A, gam[which], which, case_id(case), label)
        key = f"{case.mode} {which}"
        _spent["worst"][key] = max(_spent["worst"].get(key, 0.0), r)
        said.append(f"{which} err/bound {r:.3f} (rel-L2 {R.rel_l2(out[which].cpu(), ref):.2e})")
    dt = time.time() - t0
    _spent["seconds"] += dt
    _spent["cases"] += 1
    print(f"{label}: {', '.join(said)}, {dt:.2f} s")
