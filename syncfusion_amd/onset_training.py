"""Differentiable VideoOnsetNet forward on the HIP kernels: the training path of ``main.module_onset.Model`` (main/module_onset.py:22-66).

``onset_train_forward(net, frames)`` runs ``main/onset_net.py:57-63`` -- the R(2+1)D-18 trunk with its temporal strides removed, spatial mean
pooling and the 512-128-1 head -- in train mode: every BatchNorm3d normalises with the statistics of the batch and updates its running
statistics (momentum, unbiased variance, ``num_batches_tracked``), as ``nn.BatchNorm3d`` does in ``.train()``.

The activations stay in the kernels' own layout from the first convolution to the pooling: channels-last rows ``((n*T + t)*H + h)*W + w``
whose channel counts are padded to the inference engine's row lengths (``ld``; zeros in the padding).  Each step is a
``torch.autograd.Function`` whose forward and backward call the C ABI (include/syncfusion_amd.h):

* ``_VConv``    -- Conv3d without bias (``sf_op_vconv_fwd`` / ``sf_op_vconv_bwd``); saves its input and weight;
* ``_BNTrain``  -- BatchNorm3d (+ residual) (+ ReLU) (``sf_op_bn_train_fwd`` / ``sf_op_bn_train_bwd``); saves its input, its output (the ReLU
  mask) and the batch mean / 1/std;
* ``_Pool``     -- AdaptiveAvgPool3d((None, 1, 1)) (``sf_op_video_pool`` / ``sf_op_video_pool_bwd``).

The fc head (0.01 % of the FLOPs), the pooled transpose and the loss run on ATen.  fp32 throughout (plain ``v_mfma_f32_32x32x2_f32``
products): the reference trains the onset net in fp32.  No atomics: a second backward gives the same bits.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

Tensor = torch.Tensor

_STAGES = ("layer1", "layer2", "layer3", "layer4")


def row_ld(c: int) -> int:
    """Row length of a channels-last activation of ``c`` channels: the inference engine's padding (onset_engine.cpp make_conv)."""
    return (c + 3) // 4 * 4 if c < 32 else (c + 63) // 64 * 64


_ws_keep: dict = {}


def _workspace(nbytes: int, device: torch.device) -> Tensor:
    """One growing scratch buffer per device; every op runs on the current stream, so consecutive ops may share it."""
    ws = _ws_keep.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_keep[device] = ws
    return ws


def _stream(t: Tensor) -> int:
    return _lib.stream_ptr(t.device)


def _bump(*tensors: Optional[Tensor]) -> None:
    """A kernel wrote these buffers through a raw pointer: advance their version counters so that whoever keys on ``_version`` (the
    inference engine's staleness check) sees the change."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


class Geometry(tuple):
    """(N, T, Hi, Wi, cin, cin_ld, cout, cout_ld, kt, kh, kw, sh, sw, pt, ph, pw) of one convolution."""

    @property
    def out_hw(self) -> Tuple[int, int]:
        N, T, Hi, Wi, _, _, _, _, _kt, kh, kw, sh, sw, _pt, ph, pw = self
        return (Hi + 2 * ph - kh) // sh + 1, (Wi + 2 * pw - kw) // sw + 1

    def desc(self) -> _lib.VConvDesc:
        return _lib.VConvDesc(*self)


def conv_geometry(conv: nn.Conv3d, N: int, T: int, H: int, W: int, cin_ld: Optional[int] = None, cout_ld: Optional[int] = None) -> Geometry:
    kt, kh, kw = conv.kernel_size
    st, sh, sw = conv.stride
    pt, ph, pw = conv.padding
    if st != 1 or conv.bias is not None or conv.groups != 1 or tuple(conv.dilation) != (1, 1, 1):
        raise ValueError("onset training: Conv3d with temporal stride 1, no bias, no groups or dilation expected")
    cin, cout = conv.in_channels, conv.out_channels
    return Geometry((N, T, H, W, cin, cin_ld or row_ld(cin), cout, cout_ld or row_ld(cout), kt, kh, kw, sh, sw, pt, ph, pw))


class _VConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, geo: Geometry) -> Tensor:
        lib = _lib.load()
        N, T = geo[0], geo[1]
        Ho, Wo = geo.out_hw
        d = geo.desc()
        y = torch.empty(N * T * Ho * Wo, geo[7], dtype=torch.float32, device=x.device)
        n = lib.sf_op_vconv_workspace_bytes(C.byref(d))
        if n < 0:
            raise _lib.SyncFusionAmdError(f"sf_op_vconv_workspace_bytes: {lib.sf_last_error().decode()}")
        ws = _workspace(n, x.device)
        wc = w.detach().contiguous()
        _lib.check(lib.sf_op_vconv_fwd(C.byref(d), x.data_ptr(), wc.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x)),
                   "sf_op_vconv_fwd")
        ctx.save_for_backward(x, wc)
        ctx.geo = geo
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        geo = ctx.geo
        d = geo.desc()
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        if dx is None and dw is None:
            return None, None, None
        ws = _workspace(lib.sf_op_vconv_workspace_bytes(C.byref(d)), x.device)
        _lib.check(lib.sf_op_vconv_bwd(C.byref(d), x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr() if dx is not None else None,
                                       dw.data_ptr() if dw is not None else None, ws.data_ptr(), ws.numel(), _stream(x)), "sf_op_vconv_bwd")
        return dx, dw, None


def vconv(x: Tensor, w: Tensor, geo: Geometry) -> Tensor:
    """Conv3d (no bias) on channels-last rows: x (N*T*Hi*Wi, cin_ld) -> (N*T*Ho*Wo, cout_ld)."""
    return _VConv.apply(x, w, geo)


class _BNTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, gamma: Tensor, beta: Tensor, res: Optional[Tensor], bn: nn.BatchNorm3d, relu: bool) -> Tensor:
        lib = _lib.load()
        rows, ld = x.shape
        Cc = bn.num_features
        y = torch.empty_like(x)
        mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        ws = _workspace(lib.sf_op_bn_train_workspace_bytes(rows, Cc), x.device)
        track = bn.track_running_stats and bn.running_mean is not None
        if track and bn.momentum is None:
            raise NotImplementedError("onset training: BatchNorm3d(momentum=None) (cumulative averaging) is not supported")
        rm, rv, nbt = (bn.running_mean, bn.running_var, bn.num_batches_tracked) if track else (None, None, None)
        _lib.check(lib.sf_op_bn_train_fwd(x.data_ptr(), res.data_ptr() if res is not None else None, rows, Cc, ld, gamma.data_ptr(), beta.data_ptr(),
                                          float(bn.eps), float(bn.momentum or 0.0), rm.data_ptr() if track else None,
                                          rv.data_ptr() if track else None, nbt.data_ptr() if track else None, int(relu), y.data_ptr(),
                                          mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x)), "sf_op_bn_train_fwd")
        _bump(rm, rv, nbt)
        ctx.save_for_backward(x, y if relu else None, gamma, mean, invstd)
        ctx.has_res = res is not None
        ctx.Cc = Cc
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        lib = _lib.load()
        x, y, gamma, mean, invstd = ctx.saved_tensors
        rows, ld = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dres = torch.empty_like(x) if ctx.has_res and ctx.needs_input_grad[3] else None
        dgamma = torch.empty_like(gamma) if ctx.needs_input_grad[1] else None
        dbeta = torch.empty_like(gamma) if ctx.needs_input_grad[2] else None
        ws = _workspace(lib.sf_op_bn_train_workspace_bytes(rows, ctx.Cc), x.device)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        _lib.check(lib.sf_op_bn_train_bwd(x.data_ptr(), ptr(y), dy.data_ptr(), rows, ctx.Cc, ld, gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                          ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), ws.data_ptr(), ws.numel(), _stream(x)), "sf_op_bn_train_bwd")
        return dx, dgamma, dbeta, dres, None, None


def batch_norm_train(x: Tensor, bn: nn.BatchNorm3d, res: Optional[Tensor] = None, relu: bool = False) -> Tensor:
    """BatchNorm3d in train mode (+ res) (+ ReLU) on channels-last rows (rows, ld); updates ``bn``'s running statistics."""
    return _BNTrain.apply(x, bn.weight, bn.bias, res, bn, relu)


class _Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, NT: int, HW: int, Cc: int) -> Tensor:
        out = torch.empty(NT, Cc, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().sf_op_video_pool(x.data_ptr(), NT, HW, Cc, x.shape[1], out.data_ptr(), _stream(x)), "sf_op_video_pool")
        ctx.meta = (NT, HW, Cc, x.shape[1])
        return out

    @staticmethod
    def backward(ctx, dp: Tensor):
        NT, HW, Cc, ld = ctx.meta
        dp = dp.contiguous()
        dx = torch.empty(NT * HW, ld, dtype=torch.float32, device=dp.device)
        _lib.check(_lib.load().sf_op_video_pool_bwd(dp.data_ptr(), NT, HW, Cc, ld, dx.data_ptr(), _stream(dp)), "sf_op_video_pool_bwd")
        return dx, None, None, None


def frames_to_rows(x: Tensor, ld: int = 4) -> Tensor:
    """(N, C, T, H, W) fp32 -> channels-last rows (N*T*H*W, ld), zeros in the padding.  Frames take no gradient (none is needed)."""
    N, Cc, T, H, W = x.shape
    xs = _lib.f32c(x)
    out = torch.empty(N * T * H * W, ld, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().sf_op_video_to_cl(xs.data_ptr(), N, Cc, T, H, W, ld, out.data_ptr(), _stream(x)), "sf_op_video_to_cl")
    return out


class _Act:
    """A channels-last activation and its geometry."""

    def __init__(self, rows: Tensor, N: int, T: int, H: int, W: int):
        self.rows, self.N, self.T, self.H, self.W = rows, N, T, H, W


def _conv(conv: nn.Conv3d, a: _Act) -> _Act:
    geo = conv_geometry(conv, a.N, a.T, a.H, a.W, cin_ld=a.rows.shape[1])
    Ho, Wo = geo.out_hw
    return _Act(vconv(a.rows, conv.weight, geo), a.N, a.T, Ho, Wo)


def _bn(bn: nn.BatchNorm3d, a: _Act, res: Optional[_Act] = None, relu: bool = True) -> _Act:
    return _Act(batch_norm_train(a.rows, bn, res.rows if res is not None else None, relu), a.N, a.T, a.H, a.W)


def _basic_block(blk: nn.Module, a: _Act) -> _Act:
    # main/resnet.py:100-114: relu(bn(conv2(relu(bn(conv1(x))))) + shortcut(x)), each conv a (1,k,k) -> BN -> ReLU -> (3,1,1) pair
    c1, c2 = blk.conv1, blk.conv2
    out = _bn(c1[0][1], _conv(c1[0][0], a))
    out = _bn(c1[1], _conv(c1[0][3], out))
    out = _bn(c2[0][1], _conv(c2[0][0], out))
    out = _conv(c2[0][3], out)
    res = a
    if blk.downsample is not None:
        res = _bn(blk.downsample[1], _conv(blk.downsample[0], a), relu=False)
    return _bn(c2[1], out, res=res, relu=True)


def onset_train_forward(net: nn.Module, x: Tensor) -> Tensor:
    """VideoOnsetNet.forward in train mode with an autograd graph onto every parameter: (N, 3, T, H, W) -> (N, T) logits."""
    N, _, T, H, W = x.shape
    trunk = net.net.model
    a = _Act(frames_to_rows(x), N, T, H, W)
    st = trunk.stem   # main/resnet.py:181-192
    a = _bn(st[1], _conv(st[0], a))
    a = _bn(st[4], _conv(st[3], a))
    for name in _STAGES:
        for blk in getattr(trunk, name):
            a = _basic_block(blk, a)
    feats = _Pool.apply(a.rows, N * T, a.H * a.W, 512)      # AdaptiveAvgPool3d((None, 1, 1)): (N*T, 512)
    # main/resnet.py:244-249 squeezes (N, 512, T, 1, 1) and re-adds the batch axis when N == 1: (N, 512, T) either way;
    # main/onset_net.py:59-62 transposes to (N, T, 512) and applies the head
    h = feats.view(N, T, 512)
    h = F.relu(F.linear(h, net.fc[0].weight, net.fc[0].bias))
    return F.linear(h, net.fc[2].weight, net.fc[2].bias).squeeze(-1)
