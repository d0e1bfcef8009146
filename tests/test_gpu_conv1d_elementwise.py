"""Every 1-D convolution kernel family of the op-level entry (sf_op_conv1d_cl, groups = 0), element by element against fp64 on the MI355X.

test_gpu_ops.py gates these kernels by whole-tensor rel-L2 (2e-2 bf16, 4e-3 fp16): a 32x32 tile that is wrong in a 10^6-element output passes.
Here every element of every case is held to the bound of conv1d_ref.py, |dev - ref| <= u_T |ref| + gamma A, with the output buffer NaN-filled
and the workspace poisoned beforehand, and each case first asks sf_op_conv1d_variant which kernel the dispatcher takes and asserts that it is
the one its row names -- a test of a family proves nothing if the shape quietly went elsewhere.

CASES has, for every label the dispatcher can return at op level (test_conv1d_elementwise_cpu.py pins that set by a sweep), the smallest
aligned shape that reaches it (B = 1, rows and columns multiples of 32) and a ragged one (B >= 2, L odd so that clip boundaries fall inside
tiles, M no multiple of 32, taps = 3 with a residual, and a partial column tile wherever the family takes one: conv_gemm_rs needs N % 32 == 0),
then the geometries the families share: test_conv_direct's shapes without GroupNorm, clips shorter than the halo, L = 1, x4 upsampling with
N < 32, the strided k = 5 / k = 9 Encoder1d shapes, x2 upsampling, and the large ragged outputs in which the CPU test plants its faults.
The labels conv_gemm_mt<f32> and conv_gemm_mt<x3> each stand for more than one tile instantiation (128x128 and 128x64; the split form also
256x128 from 512 tiles of 256x128 on): each of them has a row of its own.
"""
import ctypes as C
import time

import pytest
import torch

import conv1d_ref as R
import numerics as nx
from conv1d_ref import Case

pytestmark = pytest.mark.gpu

TD = {"fp32": torch.float32, "fp32x": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}

#        dtype, B, L, C, N, taps, stride, pad, up, residual, expected_label
CASES = [
    Case("bf16", 1, 65536, 32, 96, 1, 1, 0, 1, False, "conv_gemm<bf16,128x128>"),   # smallest aligned (0.8 GFLOP in fp64)
    Case("bf16", 5, 6553, 32, 136, 3, 1, 1, 1, True, "conv_gemm<bf16,128x128>"),   # ragged (1.7 GFLOP in fp64)
    Case("bf16", 1, 32, 32, 32, 1, 1, 0, 1, False, "conv_gemm<bf16,128x32>"),   # smallest aligned
    Case("bf16", 5, 25, 32, 24, 3, 1, 1, 1, True, "conv_gemm<bf16,128x32>"),   # ragged
    Case("bf16", 1, 32768, 32, 96, 1, 1, 0, 1, False, "conv_gemm<bf16,128x64>"),   # smallest aligned
    Case("bf16", 3, 5461, 32, 136, 3, 1, 1, 1, True, "conv_gemm<bf16,128x64>"),   # ragged (0.9 GFLOP in fp64)
    Case("bf16", 1, 32, 32, 64, 1, 1, 0, 1, False, "conv_gemm<bf16,64x64>"),   # smallest aligned
    Case("bf16", 5, 25, 32, 40, 3, 1, 1, 1, True, "conv_gemm<bf16,64x64>"),   # ragged
    Case("bf16", 1, 5632, 256, 96, 1, 1, 0, 1, False, "conv_gemm_fast<bf16,32x32>"),   # smallest aligned (0.6 GFLOP in fp64)
    Case("bf16", 3, 2731, 128, 40, 3, 1, 1, 1, True, "conv_gemm_fast<bf16,32x32>"),   # ragged (0.5 GFLOP in fp64)
    Case("bf16", 1, 10240, 256, 96, 1, 1, 0, 1, False, "conv_gemm_mt<bf16,128x128>"),   # smallest aligned (1.0 GFLOP in fp64)
    Case("bf16", 3, 3413, 128, 72, 3, 1, 1, 1, True, "conv_gemm_mt<bf16,128x128>"),   # ragged (1.1 GFLOP in fp64)
    Case("bf16", 1, 5632, 256, 192, 1, 1, 0, 1, False, "conv_gemm_mt<bf16,128x192,2wg>"),   # smallest aligned (1.1 GFLOP in fp64)
    Case("bf16", 3, 1877, 128, 136, 3, 1, 1, 1, True, "conv_gemm_mt<bf16,128x192,2wg>"),   # ragged (1.2 GFLOP in fp64)
    Case("bf16", 1, 10240, 256, 128, 1, 1, 0, 1, False, "conv_gemm_mt<bf16,128x64,2wg>"),   # smallest aligned (1.3 GFLOP in fp64)
    Case("bf16", 3, 1365, 128, 320, 3, 1, 1, 1, True, "conv_gemm_mt<bf16,128x64,2wg>"),   # ragged (2.0 GFLOP in fp64)
    Case("bf16", 1, 45056, 256, 96, 1, 1, 0, 1, False, "conv_gemm_mt<bf16,192x128>"),   # smallest aligned (4.4 GFLOP in fp64)
    Case("bf16", 3, 10923, 128, 72, 3, 1, 1, 1, True, "conv_gemm_mt<bf16,192x128>"),   # ragged (3.6 GFLOP in fp64)
    Case("bf16", 1, 16384, 256, 320, 1, 1, 0, 1, False, "conv_gemm_mt<bf16,256x128>"),   # smallest aligned (5.4 GFLOP in fp64)
    Case("bf16", 3, 5461, 128, 264, 3, 1, 1, 1, True, "conv_gemm_mt<bf16,256x128>"),   # ragged (6.6 GFLOP in fp64)
    Case("bf16", 1, 32, 256, 32, 1, 1, 0, 1, False, "conv_gemm_rs<bf16,32x32>"),   # smallest aligned
    Case("bf16", 5, 25, 128, 32, 3, 1, 1, 1, True, "conv_gemm_rs<bf16,32x32>"),   # ragged
    Case("bf16", 1, 32, 96, 32, 3, 1, 1, 1, False, "conv_gemm_sk<bf16,32x32>"),   # smallest aligned
    Case("bf16", 5, 25, 96, 24, 3, 1, 1, 1, True, "conv_gemm_sk<bf16,32x32>"),   # ragged
    Case("bf16", 1, 32, 64, 32, 1, 1, 0, 1, False, "conv_gemm_v2<bf16,64x64>"),   # smallest aligned
    Case("bf16", 5, 25, 64, 24, 3, 1, 1, 1, True, "conv_gemm_v2<bf16,64x64>"),   # ragged
    Case("bf16", 1, 32, 1024, 32, 3, 1, 1, 1, False, "conv_gemm_wp<bf16,32x32>"),   # smallest aligned
    Case("bf16", 5, 25, 128, 24, 3, 1, 1, 1, True, "conv_gemm_wp<bf16,32x32>"),   # ragged
    Case("fp16", 1, 65536, 32, 96, 1, 1, 0, 1, False, "conv_gemm<f16,128x128>"),   # smallest aligned (0.8 GFLOP in fp64)
    Case("fp16", 5, 6553, 32, 136, 3, 1, 1, 1, True, "conv_gemm<f16,128x128>"),   # ragged (1.7 GFLOP in fp64)
    Case("fp16", 1, 32, 32, 32, 1, 1, 0, 1, False, "conv_gemm<f16,128x32>"),   # smallest aligned
    Case("fp16", 5, 25, 32, 24, 3, 1, 1, 1, True, "conv_gemm<f16,128x32>"),   # ragged
    Case("fp16", 1, 32768, 32, 96, 1, 1, 0, 1, False, "conv_gemm<f16,128x64>"),   # smallest aligned
    Case("fp16", 3, 5461, 32, 136, 3, 1, 1, 1, True, "conv_gemm<f16,128x64>"),   # ragged (0.9 GFLOP in fp64)
    Case("fp16", 1, 32, 32, 64, 1, 1, 0, 1, False, "conv_gemm<f16,64x64>"),   # smallest aligned
    Case("fp16", 5, 25, 32, 40, 3, 1, 1, 1, True, "conv_gemm<f16,64x64>"),   # ragged
    Case("fp16", 1, 5632, 256, 96, 1, 1, 0, 1, False, "conv_gemm_fast<f16,32x32>"),   # smallest aligned (0.6 GFLOP in fp64)
    Case("fp16", 3, 2731, 128, 40, 3, 1, 1, 1, True, "conv_gemm_fast<f16,32x32>"),   # ragged (0.5 GFLOP in fp64)
    Case("fp16", 1, 10240, 256, 96, 1, 1, 0, 1, False, "conv_gemm_mt<f16,128x128>"),   # smallest aligned (1.0 GFLOP in fp64)
    Case("fp16", 3, 3413, 128, 72, 3, 1, 1, 1, True, "conv_gemm_mt<f16,128x128>"),   # ragged (1.1 GFLOP in fp64)
    Case("fp16", 1, 5632, 256, 192, 1, 1, 0, 1, False, "conv_gemm_mt<f16,128x192,2wg>"),   # smallest aligned (1.1 GFLOP in fp64)
    Case("fp16", 3, 1877, 128, 136, 3, 1, 1, 1, True, "conv_gemm_mt<f16,128x192,2wg>"),   # ragged (1.2 GFLOP in fp64)
    Case("fp16", 1, 10240, 256, 128, 1, 1, 0, 1, False, "conv_gemm_mt<f16,128x64,2wg>"),   # smallest aligned (1.3 GFLOP in fp64)
    Case("fp16", 3, 1365, 128, 320, 3, 1, 1, 1, True, "conv_gemm_mt<f16,128x64,2wg>"),   # ragged (2.0 GFLOP in fp64)
    Case("fp16", 1, 45056, 256, 96, 1, 1, 0, 1, False, "conv_gemm_mt<f16,192x128>"),   # smallest aligned (4.4 GFLOP in fp64)
    Case("fp16", 3, 10923, 128, 72, 3, 1, 1, 1, True, "conv_gemm_mt<f16,192x128>"),   # ragged (3.6 GFLOP in fp64)
    Case("fp16", 1, 16384, 256, 320, 1, 1, 0, 1, False, "conv_gemm_mt<f16,256x128>"),   # smallest aligned (5.4 GFLOP in fp64)
    Case("fp16", 3, 5461, 128, 264, 3, 1, 1, 1, True, "conv_gemm_mt<f16,256x128>"),   # ragged (6.6 GFLOP in fp64)
    Case("fp16", 1, 32, 256, 32, 1, 1, 0, 1, False, "conv_gemm_rs<f16,32x32>"),   # smallest aligned
    Case("fp16", 5, 25, 128, 32, 3, 1, 1, 1, True, "conv_gemm_rs<f16,32x32>"),   # ragged
    Case("fp16", 1, 32, 96, 32, 3, 1, 1, 1, False, "conv_gemm_sk<f16,32x32>"),   # smallest aligned
    Case("fp16", 5, 25, 96, 24, 3, 1, 1, 1, True, "conv_gemm_sk<f16,32x32>"),   # ragged
    Case("fp16", 1, 32, 64, 32, 1, 1, 0, 1, False, "conv_gemm_v2<f16,64x64>"),   # smallest aligned
    Case("fp16", 5, 25, 64, 24, 3, 1, 1, 1, True, "conv_gemm_v2<f16,64x64>"),   # ragged
    Case("fp16", 1, 32, 1024, 32, 3, 1, 1, 1, False, "conv_gemm_wp<f16,32x32>"),   # smallest aligned
    Case("fp16", 5, 25, 128, 24, 3, 1, 1, 1, True, "conv_gemm_wp<f16,32x32>"),   # ragged
    Case("fp32", 1, 65536, 32, 96, 1, 1, 0, 1, False, "conv_gemm<f32,128x128>"),   # smallest aligned (0.8 GFLOP in fp64)
    Case("fp32", 5, 6553, 32, 136, 3, 1, 1, 1, True, "conv_gemm<f32,128x128>"),   # ragged (1.7 GFLOP in fp64)
    Case("fp32", 1, 32, 32, 32, 1, 1, 0, 1, False, "conv_gemm<f32,128x32>"),   # smallest aligned
    Case("fp32", 5, 25, 32, 24, 3, 1, 1, 1, True, "conv_gemm<f32,128x32>"),   # ragged
    Case("fp32", 1, 32768, 32, 96, 1, 1, 0, 1, False, "conv_gemm<f32,128x64>"),   # smallest aligned
    Case("fp32", 3, 5461, 32, 136, 3, 1, 1, 1, True, "conv_gemm<f32,128x64>"),   # ragged (0.9 GFLOP in fp64)
    Case("fp32", 1, 32, 32, 64, 1, 1, 0, 1, False, "conv_gemm<f32,64x64>"),   # smallest aligned
    Case("fp32", 5, 25, 32, 40, 3, 1, 1, 1, True, "conv_gemm<f32,64x64>"),   # ragged
    Case("fp32", 1, 5632, 256, 96, 1, 1, 0, 1, False, "conv_gemm_fast<f32,32x32>"),   # smallest aligned (0.6 GFLOP in fp64)
    Case("fp32", 3, 2731, 128, 40, 3, 1, 1, 1, True, "conv_gemm_fast<f32,32x32>"),   # ragged (0.5 GFLOP in fp64)
    Case("fp32", 1, 32768, 256, 32, 1, 1, 0, 1, False, "conv_gemm_mt<f32>"),   # smallest aligned (1.1 GFLOP in fp64)
    Case("fp32", 5, 6553, 96, 24, 3, 1, 1, 1, True, "conv_gemm_mt<f32>"),   # ragged (0.9 GFLOP in fp64)
    Case("fp32", 1, 32, 96, 32, 3, 1, 1, 1, False, "conv_gemm_sk<f32,32x32>"),   # smallest aligned
    Case("fp32", 5, 25, 96, 24, 3, 1, 1, 1, True, "conv_gemm_sk<f32,32x32>"),   # ragged
    Case("fp32", 1, 20480, 64, 192, 1, 1, 0, 1, False, "conv_gemm_v2<f32,128x128>"),   # smallest aligned (1.0 GFLOP in fp64)
    Case("fp32", 3, 6827, 64, 136, 3, 1, 1, 1, True, "conv_gemm_v2<f32,128x128>"),   # ragged (2.1 GFLOP in fp64)
    Case("fp32", 1, 32, 64, 32, 1, 1, 0, 1, False, "conv_gemm_v2<f32,64x64>"),   # smallest aligned
    Case("fp32", 5, 25, 64, 24, 3, 1, 1, 1, True, "conv_gemm_v2<f32,64x64>"),   # ragged
    Case("fp32", 1, 32, 256, 32, 1, 1, 0, 1, False, "conv_gemm_wp<f32,32x32>"),   # smallest aligned
    Case("fp32", 5, 25, 128, 24, 3, 1, 1, 1, True, "conv_gemm_wp<f32,32x32>"),   # ragged
    Case("fp32x", 1, 65536, 32, 96, 1, 1, 0, 1, False, "conv_gemm<f32,128x128>"),   # smallest aligned (0.8 GFLOP in fp64)
    Case("fp32x", 5, 6553, 32, 136, 3, 1, 1, 1, True, "conv_gemm<f32,128x128>"),   # ragged (1.7 GFLOP in fp64)
    Case("fp32x", 1, 32, 32, 32, 1, 1, 0, 1, False, "conv_gemm<f32,128x32>"),   # smallest aligned
    Case("fp32x", 5, 25, 32, 24, 3, 1, 1, 1, True, "conv_gemm<f32,128x32>"),   # ragged
    Case("fp32x", 1, 32768, 32, 96, 1, 1, 0, 1, False, "conv_gemm<f32,128x64>"),   # smallest aligned
    Case("fp32x", 3, 5461, 32, 136, 3, 1, 1, 1, True, "conv_gemm<f32,128x64>"),   # ragged (0.9 GFLOP in fp64)
    Case("fp32x", 1, 32, 32, 64, 1, 1, 0, 1, False, "conv_gemm<f32,64x64>"),   # smallest aligned
    Case("fp32x", 5, 25, 32, 40, 3, 1, 1, 1, True, "conv_gemm<f32,64x64>"),   # ragged
    Case("fp32x", 1, 5632, 256, 96, 1, 1, 0, 1, False, "conv_gemm_fast<x3,32x32>"),   # smallest aligned (0.6 GFLOP in fp64)
    Case("fp32x", 3, 2731, 128, 40, 3, 1, 1, 1, True, "conv_gemm_fast<x3,32x32>"),   # ragged (0.5 GFLOP in fp64)
    Case("fp32x", 1, 16384, 256, 32, 1, 1, 0, 1, False, "conv_gemm_mt<x3>"),   # smallest aligned (0.5 GFLOP in fp64)
    Case("fp32x", 3, 5461, 96, 24, 3, 1, 1, 1, True, "conv_gemm_mt<x3>"),   # ragged
    Case("fp32x", 1, 32, 256, 32, 1, 1, 0, 1, False, "conv_gemm_rs<x3,32x32>"),   # smallest aligned
    Case("fp32x", 5, 25, 128, 32, 3, 1, 1, 1, True, "conv_gemm_rs<x3,32x32>"),   # ragged
    Case("fp32x", 1, 32, 96, 32, 3, 1, 1, 1, False, "conv_gemm_sk<f32,32x32>"),   # smallest aligned
    Case("fp32x", 5, 25, 96, 24, 3, 1, 1, 1, True, "conv_gemm_sk<f32,32x32>"),   # ragged
    Case("fp32x", 1, 20480, 64, 192, 1, 1, 0, 1, False, "conv_gemm_v2<f32,128x128>"),   # smallest aligned (1.0 GFLOP in fp64)
    Case("fp32x", 3, 6827, 64, 136, 3, 1, 1, 1, True, "conv_gemm_v2<f32,128x128>"),   # ragged (2.1 GFLOP in fp64)
    Case("fp32x", 1, 32, 64, 32, 1, 1, 0, 1, False, "conv_gemm_v2<f32,64x64>"),   # smallest aligned
    Case("fp32x", 5, 25, 64, 24, 3, 1, 1, 1, True, "conv_gemm_v2<f32,64x64>"),   # ragged
    Case("fp32x", 1, 32, 512, 32, 3, 1, 1, 1, False, "conv_gemm_wp<x3,32x32>"),   # smallest aligned
    Case("fp32x", 5, 25, 128, 24, 3, 1, 1, 1, True, "conv_gemm_wp<x3,32x32>"),   # ragged
    Case("fp32", 2, 2816, 8, 8, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("fp32", 2, 704, 1, 8, 1, 1, 0, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp32", 2, 704, 8, 1, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("fp32", 2, 1024, 2, 8, 9, 4, 4, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp32", 3, 500, 16, 32, 9, 4, 4, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp32", 2, 640, 2, 2, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("fp32", 2, 640, 1, 2, 3, 1, 1, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp32", 5, 3, 64, 64, 3, 1, 1, 1, True, "conv_gemm_v2<f32,64x64>"),   # clips shorter than the halo
    Case("fp32", 4, 1, 64, 64, 3, 1, 1, 1, True, "conv_gemm_v2<f32,64x64>"),   # L = 1
    Case("fp32", 67, 1, 256, 64, 3, 1, 1, 1, True, "conv_gemm_wp<f32,32x32>"),   # L = 1, short-activation family
    Case("fp32", 2, 88, 64, 8, 3, 1, 1, 4, False, "conv_gemm_v2<f32,64x64>"),   # x4 upsample, N < 32
    Case("fp32", 2, 352, 32, 64, 5, 2, 2, 1, False, "conv_gemm<f32,64x64>"),   # Encoder1d strided k = 5
    Case("fp32", 2, 89, 64, 96, 3, 1, 1, 2, True, "conv_gemm_v2<f32,64x64>"),   # x2 upsample, ragged
    Case("fp32", 3, 1367, 128, 128, 3, 1, 1, 2, True, "conv_gemm_fast<f32,32x32>"),   # x2 upsample on a long activation (1.6 GFLOP in fp64)
    Case("fp32", 3, 8194, 32, 64, 5, 2, 2, 1, True, "conv_gemm<f32,64x64>"),   # strided k = 5, padding right of the last position (0.5 GFLOP in fp64)
    Case("fp32", 2, 357, 256, 64, 3, 2, 1, 1, True, "conv_gemm_wp<f32,32x32>"),   # strided k = 3 on a short-activation family, odd L
    Case("fp32x", 2, 2816, 8, 8, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("fp32x", 2, 704, 1, 8, 1, 1, 0, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp32x", 2, 704, 8, 1, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("fp32x", 2, 1024, 2, 8, 9, 4, 4, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp32x", 3, 500, 16, 32, 9, 4, 4, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp32x", 2, 640, 2, 2, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("fp32x", 2, 640, 1, 2, 3, 1, 1, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp32x", 5, 3, 64, 64, 3, 1, 1, 1, True, "conv_gemm_v2<f32,64x64>"),   # clips shorter than the halo
    Case("fp32x", 4, 1, 64, 64, 3, 1, 1, 1, True, "conv_gemm_v2<f32,64x64>"),   # L = 1
    Case("fp32x", 67, 1, 256, 64, 3, 1, 1, 1, True, "conv_gemm_rs<x3,32x32>"),   # L = 1, short-activation family
    Case("fp32x", 2, 88, 64, 8, 3, 1, 1, 4, False, "conv_gemm_v2<f32,64x64>"),   # x4 upsample, N < 32
    Case("fp32x", 2, 352, 32, 64, 5, 2, 2, 1, False, "conv_gemm<f32,64x64>"),   # Encoder1d strided k = 5
    Case("fp32x", 2, 89, 64, 96, 3, 1, 1, 2, True, "conv_gemm_v2<f32,64x64>"),   # x2 upsample, ragged
    Case("fp32x", 3, 1367, 128, 128, 3, 1, 1, 2, True, "conv_gemm_mt<x3>"),   # x2 upsample on a long activation (1.6 GFLOP in fp64)
    Case("fp32x", 3, 8194, 32, 64, 5, 2, 2, 1, True, "conv_gemm<f32,64x64>"),   # strided k = 5, padding right of the last position (0.5 GFLOP in fp64)
    Case("fp32x", 2, 357, 256, 64, 3, 2, 1, 1, True, "conv_gemm_rs<x3,32x32>"),   # strided k = 3 on a short-activation family, odd L
    Case("bf16", 2, 2816, 8, 8, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("bf16", 2, 704, 1, 8, 1, 1, 0, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("bf16", 2, 704, 8, 1, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("bf16", 2, 1024, 2, 8, 9, 4, 4, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("bf16", 3, 500, 16, 32, 9, 4, 4, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("bf16", 2, 640, 2, 2, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("bf16", 2, 640, 1, 2, 3, 1, 1, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("bf16", 5, 3, 64, 64, 3, 1, 1, 1, True, "conv_gemm_v2<bf16,64x64>"),   # clips shorter than the halo
    Case("bf16", 4, 1, 64, 64, 3, 1, 1, 1, True, "conv_gemm_v2<bf16,64x64>"),   # L = 1
    Case("bf16", 67, 1, 256, 64, 3, 1, 1, 1, True, "conv_gemm_rs<bf16,32x32>"),   # L = 1, short-activation family
    Case("bf16", 2, 88, 64, 8, 3, 1, 1, 4, False, "conv_gemm_v2<bf16,64x64>"),   # x4 upsample, N < 32
    Case("bf16", 2, 352, 32, 64, 5, 2, 2, 1, False, "conv_gemm<bf16,64x64>"),   # Encoder1d strided k = 5
    Case("bf16", 2, 89, 64, 96, 3, 1, 1, 2, True, "conv_gemm_v2<bf16,64x64>"),   # x2 upsample, ragged
    Case("bf16", 3, 1367, 128, 128, 3, 1, 1, 2, True, "conv_gemm_fast<bf16,32x32>"),   # x2 upsample on a long activation (1.6 GFLOP in fp64)
    Case("bf16", 3, 8194, 32, 64, 5, 2, 2, 1, True, "conv_gemm<bf16,64x64>"),   # strided k = 5, padding right of the last position (0.5 GFLOP in fp64)
    Case("bf16", 2, 357, 256, 64, 3, 2, 1, 1, True, "conv_gemm_rs<bf16,32x32>"),   # strided k = 3 on a short-activation family, odd L
    Case("fp16", 2, 2816, 8, 8, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("fp16", 2, 704, 1, 8, 1, 1, 0, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp16", 2, 704, 8, 1, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("fp16", 2, 1024, 2, 8, 9, 4, 4, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp16", 3, 500, 16, 32, 9, 4, 4, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp16", 2, 640, 2, 2, 3, 1, 1, 1, True, "conv_direct"),   # test_conv_direct geometry
    Case("fp16", 2, 640, 1, 2, 3, 1, 1, 1, False, "conv_direct"),   # test_conv_direct geometry
    Case("fp16", 5, 3, 64, 64, 3, 1, 1, 1, True, "conv_gemm_v2<f16,64x64>"),   # clips shorter than the halo
    Case("fp16", 4, 1, 64, 64, 3, 1, 1, 1, True, "conv_gemm_v2<f16,64x64>"),   # L = 1
    Case("fp16", 67, 1, 256, 64, 3, 1, 1, 1, True, "conv_gemm_rs<f16,32x32>"),   # L = 1, short-activation family
    Case("fp16", 2, 88, 64, 8, 3, 1, 1, 4, False, "conv_gemm_v2<f16,64x64>"),   # x4 upsample, N < 32
    Case("fp16", 2, 352, 32, 64, 5, 2, 2, 1, False, "conv_gemm<f16,64x64>"),   # Encoder1d strided k = 5
    Case("fp16", 2, 89, 64, 96, 3, 1, 1, 2, True, "conv_gemm_v2<f16,64x64>"),   # x2 upsample, ragged
    Case("fp16", 3, 1367, 128, 128, 3, 1, 1, 2, True, "conv_gemm_fast<f16,32x32>"),   # x2 upsample on a long activation (1.6 GFLOP in fp64)
    Case("fp16", 3, 8194, 32, 64, 5, 2, 2, 1, True, "conv_gemm<f16,64x64>"),   # strided k = 5, padding right of the last position (0.5 GFLOP in fp64)
    Case("fp16", 2, 357, 256, 64, 3, 2, 1, 1, True, "conv_gemm_rs<f16,32x32>"),   # strided k = 3 on a short-activation family, odd L
    Case("bf16", 1, 5120, 512, 192, 1, 1, 0, 1, False, "conv_gemm_mt<bf16,128x64,2wg>"),   # macro tiles: the wide_small rule (192 columns, K >= 512, <= 176 tiles) (2.0 GFLOP in fp64)
    Case("bf16", 1, 896, 256, 1536, 1, 1, 0, 1, False, "conv_gemm_mt<bf16,128x192,2wg>"),   # macro tiles: the wide rule on 1536 columns (K <= 1024) (1.4 GFLOP in fp64)
    Case("bf16", 3, 5851, 64, 192, 3, 1, 1, 2, True, "conv_gemm_v2<bf16,64x64>"),   # x2 upsample, 6.7e6 outputs, two rows in the last tile (5.2 GFLOP in fp64)
    Case("fp16", 1, 5120, 512, 192, 1, 1, 0, 1, False, "conv_gemm_mt<f16,128x64,2wg>"),   # macro tiles: the wide_small rule (192 columns, K >= 512, <= 176 tiles) (2.0 GFLOP in fp64)
    Case("fp16", 1, 896, 256, 1536, 1, 1, 0, 1, False, "conv_gemm_mt<f16,128x192,2wg>"),   # macro tiles: the wide rule on 1536 columns (K <= 1024) (1.4 GFLOP in fp64)
    Case("fp16", 3, 5851, 64, 192, 3, 1, 1, 2, True, "conv_gemm_v2<f16,64x64>"),   # x2 upsample, 6.7e6 outputs, two rows in the last tile (5.2 GFLOP in fp64)
    Case("bf16", 2, 10945, 32, 320, 3, 1, 1, 1, True, "conv_gemm<bf16,128x128>"),   # partial column tile 256-319, two rows in the last tile (2.7 GFLOP in fp64)
    Case("fp16", 2, 40001, 32, 320, 3, 1, 1, 1, True, "conv_gemm<f16,128x128>"),   # partial column tile 256-319, two rows in the last tile, 2.6e7 outputs (9.8 GFLOP in fp64)
    Case("fp32", 2, 1025, 32, 320, 3, 1, 1, 1, True, "conv_gemm<f32,64x64>"),   # partial column tile 256-319, two rows in the last tile
    Case("fp32x", 2, 1025, 32, 320, 3, 1, 1, 1, True, "conv_gemm<f32,64x64>"),   # partial column tile 256-319, two rows in the last tile
    Case("fp32", 1, 32768, 256, 64, 1, 1, 0, 1, False, "conv_gemm_mt<f32>"),   # fp32 macro tiles, the 128x64 variant (2.1 GFLOP in fp64)
    Case("fp32x", 3, 5451, 128, 256, 3, 1, 1, 1, True, "conv_gemm_mt<x3>"),   # split macro tiles, the 128x128 variant, one row in the last tile (6.4 GFLOP in fp64)
    Case("fp32x", 2, 8193, 256, 1024, 1, 1, 0, 1, True, "conv_gemm_mt<x3>"),   # split macro tiles, the 256x128 variant (520 tiles), ragged rows (17.2 GFLOP in fp64)
]


def case_id(c: Case) -> str:
    return f"{c.dtype}-B{c.B}-L{c.L}-C{c.C}-N{c.N}-k{c.taps}-s{c.stride}-u{c.up}{'-res' if c.residual else ''}"


def variant(lib, _l, c: Case) -> str:
    """The label of the launch sf_op_conv1d_cl makes for this case (query only)."""
    buf = C.create_string_buffer(96)
    _l.check(lib.sf_op_conv1d_variant(_l.DTYPES[c.dtype], c.B, c.L, c.C, c.N, c.taps, c.stride, c.pad, c.up, 0, buf, 96), "sf_op_conv1d_variant")
    return buf.value.decode()


_spent = {"seconds": 0.0, "cases": 0, "worst": {}}


@pytest.fixture(scope="module", autouse=True)
def _total():
    yield
    worst = ", ".join(f"{d} {r:.3f}" for d, r in sorted(_spent["worst"].items()))
    print(f"\nconv1d element-wise gate: {_spent['cases']} cases in {_spent['seconds']:.1f} s; worst err/bound per dtype: {worst}")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conv1d_elementwise(cuda, case):
    from syncfusion_amd import _lib as _l

    lib = _l.load()
    t0 = time.time()
    ops = R.operands(case)
    x, w, _, bias, res = ops
    td = TD[case.dtype]
    xd, wd, bd = x.to(td).to(cuda), w.to(cuda), bias.to(cuda)
    rd = res.to(td).to(cuda) if case.residual else None
    out = nx.nan_like((case.B, case.Lout, case.N), td, cuda)                   # an unwritten element fails the gate
    ws = nx.poisoned_workspace(16 * case.N * case.K + (1 << 20), cuda)         # up to four images of the weight
    label = variant(lib, _l, case)
    _l.check(lib.sf_op_conv1d_cl(_l.DTYPES[case.dtype], xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, None, 0, 0.0,
                                 rd.data_ptr() if case.residual else None, case.B, case.L, case.C, case.N, case.taps, case.stride, case.pad, case.up,
                                 out.data_ptr(), ws.data_ptr(), ws.numel(), _l.stream_ptr(cuda)), "sf_op_conv1d_cl")
    assert label == case.expected_label, f"{case_id(case)}: the dispatcher takes {label}, the row is written for {case.expected_label}"
    ref, A = R.case_ref(case, ops)                                             # on the CPU while the launch runs
    torch.cuda.synchronize()
    r, rel = R.gate(out.cpu(), ref, A, case.K, case.dtype, label, case_id(case), quiet=True)
    dt = time.time() - t0
    _spent["seconds"] += dt
    _spent["cases"] += 1
    _spent["worst"][case.dtype] = max(_spent["worst"].get(case.dtype, 0.0), r)
    print(f"{label}: err/bound {r:.3f}, rel-L2 {rel:.3e}, {out.numel()} elements, {dt:.2f} s")
