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
* ``_BNSyncTrain`` -- the same BatchNorm with statistics shared by the ranks of a process group (``sf_op_bn_sync_*``): every direction is
  cut where the per-channel numbers are small and one ``all_gather`` of ``2 C`` floats runs there (37 + 37 small collectives per step).  It is
  selected per module: an ``nn.SyncBatchNorm`` (``torch.nn.SyncBatchNorm.convert_sync_batchnorm``) with an initialised process group of more
  than one rank; everything else runs ``_BNTrain``, as ``torch.nn.SyncBatchNorm`` itself falls back to plain batch norm;
* ``_Pool``     -- AdaptiveAvgPool3d((None, 1, 1)) (``sf_op_video_pool`` / ``sf_op_video_pool_bwd``).

The fc head (0.01 % of the FLOPs) and the pooled transpose run on ATen; so does the loss, unless ``module_onset.Model(loss="hip")`` puts
loss and step metrics on the device (syncfusion_amd/onset_loss.py) -- then ``GraphedOnsetTrainStep`` below replays the whole step from one
HIP graph.  fp32 throughout (plain ``v_mfma_f32_32x32x2_f32``
products): the reference trains the onset net in fp32.  No atomics: a second backward gives the same bits.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist
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


# ---- cross-rank BatchNorm -----------------------------------------------------------------------------------------------------------------
class SyncGroup:
    """One process group's share of a synchronised forward: the clip counts of its ranks (gathered ONCE per forward, not once per layer) and
    the collectives of the 37 BatchNorms.  ``group=None`` with no initialised process group is a world of one whose "gather" is a reshape
    (the forced split-phase path of the tests and of tools/onset_train_step_bench.py)."""

    def __init__(self, group, clips: int, device: torch.device):
        self.group, self.device = group, device
        self.live = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.live else 1
        self.rank = dist.get_rank(group) if self.live else 0
        # device tensors go straight into the collective on nccl (RCCL); gloo carries host tensors (as training.allreduce_gradients)
        self.nccl = self.live and dist.get_backend(group) == "nccl"
        self.stage_host = self.live and not self.nccl and device.type == "cuda"
        self.collectives = 0
        self.clips = self._gather_clips(int(clips))
        empty = [r for r, n in enumerate(self.clips) if n < 1]
        if empty:     # every rank sees the same table, so every rank raises: nobody is left waiting in a collective
            raise ValueError(f"onset training (synchronised BatchNorm): rank(s) {empty} of {self.world} hold no clips (clip counts per rank "
                             f"{self.clips}; this is rank {self.rank}): every rank needs at least one clip per step")
        self._counts: Dict[int, Tensor] = {}

    def _gather_clips(self, clips: int) -> List[int]:
        if not self.live:
            return [clips]
        mine = torch.tensor([clips], dtype=torch.int64, device="cpu" if self.stage_host or self.device.type != "cuda" else self.device)
        out = torch.empty(self.world, dtype=torch.int64, device=mine.device)
        dist.all_gather(list(out.split(1)), mine, group=self.group)
        self.collectives += 1
        return [int(v) for v in out.cpu().tolist()]

    def row_counts(self, rows_per_clip: int) -> Tensor:
        """(world,) int64 on the device: every rank's row count of a layer = its clip count times the layer's T*H*W (exact integers)."""
        t = self._counts.get(rows_per_clip)
        if t is None:
            t = torch.tensor([n * rows_per_clip for n in self.clips], dtype=torch.int64).to(self.device)
            self._counts[rows_per_clip] = t
        return t

    def total_rows(self, rows_per_clip: int) -> int:
        return sum(self.clips) * rows_per_clip

    def all_gather(self, local: Tensor) -> Tensor:
        """(C, 2) of this rank -> (world, C, 2) in rank order, on ``local``'s device."""
        if not self.live:
            return local.unsqueeze(0)
        self.collectives += 1
        if self.nccl:
            out = torch.empty((self.world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
            dist.all_gather_into_tensor(out, local, group=self.group)
            return out
        host = local.cpu() if self.stage_host else local
        out = torch.empty((self.world,) + tuple(host.shape), dtype=host.dtype, device=host.device)
        dist.all_gather(list(out.unbind(0)), host, group=self.group)
        return out.to(local.device)


def _no_capture(x: Tensor) -> None:
    if x.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("onset training: a step with synchronised BatchNorm cannot be captured into a HIP graph (its collectives run "
                           "between the kernels); capture is supported on the single-rank path only")


class _BNSyncTrain(torch.autograd.Function):
    """_BNTrain with the statistics of all ranks: stats kernel -> all_gather(2 C floats) -> merge + apply kernels; backward: sums kernel ->
    all_gather(2 C floats) -> apply kernel.  dgamma / dbeta are the LOCAL sums (the gradient all-reduce averages them), as in
    torch.nn.SyncBatchNorm."""

    @staticmethod
    def forward(ctx, x: Tensor, gamma: Tensor, beta: Tensor, res: Optional[Tensor], bn: nn.Module, relu: bool, sg: SyncGroup) -> Tensor:
        lib = _lib.load()
        _no_capture(x)
        rows, ld = x.shape
        Cc = bn.num_features
        mine = sg.clips[sg.rank]
        if rows % mine:
            raise ValueError(f"synchronised BatchNorm: {rows} rows do not divide into this rank's {mine} clips")
        rpc = rows // mine
        if sg.total_rows(rpc) < 2:
            raise ValueError("synchronised BatchNorm: more than one value per channel is needed over all ranks (as nn.BatchNorm3d in train mode)")
        track = bn.track_running_stats and bn.running_mean is not None
        if track and bn.momentum is None:
            raise NotImplementedError("onset training: BatchNorm3d(momentum=None) (cumulative averaging) is not supported")
        rm, rv, nbt = (bn.running_mean, bn.running_var, bn.num_batches_tracked) if track else (None, None, None)
        counts = sg.row_counts(rpc)
        y = torch.empty_like(x)
        mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        local = torch.empty(Cc, 2, dtype=torch.float32, device=x.device)
        ws = _workspace(lib.sf_op_bn_sync_workspace_bytes(rows, Cc), x.device)
        _lib.check(lib.sf_op_bn_sync_stats(x.data_ptr(), rows, Cc, ld, local.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x)), "sf_op_bn_sync_stats")
        table = sg.all_gather(local)
        _lib.check(lib.sf_op_bn_sync_fwd_apply(x.data_ptr(), res.data_ptr() if res is not None else None, rows, Cc, ld, table.data_ptr(), counts.data_ptr(),
                                               sg.world, gamma.data_ptr(), beta.data_ptr(), float(bn.eps), float(bn.momentum or 0.0),
                                               rm.data_ptr() if track else None, rv.data_ptr() if track else None, nbt.data_ptr() if track else None,
                                               int(relu), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x)),
                   "sf_op_bn_sync_fwd_apply")
        _bump(rm, rv, nbt)
        ctx.save_for_backward(x, y if relu else None, gamma, mean, invstd, counts)
        ctx.has_res = res is not None
        ctx.Cc, ctx.sg = Cc, sg
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        lib = _lib.load()
        x, y, gamma, mean, invstd, counts = ctx.saved_tensors
        sg: SyncGroup = ctx.sg
        _no_capture(x)
        rows, ld = x.shape
        dy = dy.contiguous()
        need_dx = ctx.needs_input_grad[0]
        need_dres = ctx.has_res and ctx.needs_input_grad[3]
        dgamma = torch.empty_like(gamma) if ctx.needs_input_grad[1] else None
        dbeta = torch.empty_like(gamma) if ctx.needs_input_grad[2] else None
        local = torch.empty(ctx.Cc, 2, dtype=torch.float32, device=x.device)
        ws = _workspace(lib.sf_op_bn_sync_workspace_bytes(rows, ctx.Cc), x.device)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        # the sums and the gather run on every rank whatever this rank needs: the collective count must not depend on it
        _lib.check(lib.sf_op_bn_sync_bwd_sums(x.data_ptr(), ptr(y), dy.data_ptr(), rows, ctx.Cc, ld, mean.data_ptr(), invstd.data_ptr(), local.data_ptr(),
                                              ptr(dgamma), ptr(dbeta), ws.data_ptr(), ws.numel(), _stream(x)), "sf_op_bn_sync_bwd_sums")
        table = sg.all_gather(local)
        dx = torch.empty_like(x) if need_dx else None
        dres = torch.empty_like(x) if need_dres else None
        if dx is not None or dres is not None:
            _lib.check(lib.sf_op_bn_sync_bwd_apply(x.data_ptr(), ptr(y), dy.data_ptr(), rows, ctx.Cc, ld, table.data_ptr(), counts.data_ptr(), sg.world,
                                                   gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ptr(dx), ptr(dres), ws.data_ptr(), ws.numel(),
                                                   _stream(x)), "sf_op_bn_sync_bwd_apply")
        return dx, dgamma, dbeta, dres, None, None, None


def batch_norm_train_sync(x: Tensor, bn: nn.Module, sg: SyncGroup, res: Optional[Tensor] = None, relu: bool = False) -> Tensor:
    """``batch_norm_train`` with the batch statistics of every rank of ``sg``; updates ``bn``'s running statistics (the same bits on every rank)."""
    return _BNSyncTrain.apply(x, bn.weight, bn.bias, res, bn, relu, sg)


class _SyncState:
    """Which BatchNorms of one forward run synchronised, and over which group (one SyncGroup, hence one clip-count gather, per group)."""

    def __init__(self, clips: int, device: torch.device, force: bool = False):
        self.clips, self.device, self.force = clips, device, force
        self._groups: Dict[object, SyncGroup] = {}

    def group_for(self, bn: nn.Module) -> Optional[SyncGroup]:
        """torch.nn.SyncBatchNorm's own rule: an nn.SyncBatchNorm module, an initialised process group (the module's, else the default one) and
        more than one rank.  Everything else -- a converted net without a process group or in a world of one included -- takes the plain path."""
        live = dist.is_available() and dist.is_initialized()
        group = None
        if not self.force:
            if not isinstance(bn, nn.SyncBatchNorm) or not live:
                return None
            group = bn.process_group
            if dist.get_world_size(group) < 2:
                return None
        elif live and isinstance(bn, nn.SyncBatchNorm):
            group = bn.process_group
        sg = self._groups.get(group)
        if sg is None:
            sg = self._groups[group] = SyncGroup(group, self.clips, self.device)
        return sg


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

    def __init__(self, rows: Tensor, N: int, T: int, H: int, W: int, sync: Optional[_SyncState] = None):
        self.rows, self.N, self.T, self.H, self.W, self.sync = rows, N, T, H, W, sync


def _conv(conv: nn.Conv3d, a: _Act) -> _Act:
    geo = conv_geometry(conv, a.N, a.T, a.H, a.W, cin_ld=a.rows.shape[1])
    Ho, Wo = geo.out_hw
    return _Act(vconv(a.rows, conv.weight, geo), a.N, a.T, Ho, Wo, a.sync)


def _bn(bn: nn.BatchNorm3d, a: _Act, res: Optional[_Act] = None, relu: bool = True) -> _Act:
    r = res.rows if res is not None else None
    sg = a.sync.group_for(bn) if a.sync is not None else None
    rows = batch_norm_train(a.rows, bn, r, relu) if sg is None else batch_norm_train_sync(a.rows, bn, sg, r, relu)
    return _Act(rows, a.N, a.T, a.H, a.W, a.sync)


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


def onset_train_forward(net: nn.Module, x: Tensor, _force_sync: bool = False) -> Tensor:
    """VideoOnsetNet.forward in train mode with an autograd graph onto every parameter: (N, 3, T, H, W) -> (N, T) logits.

    A net converted by ``torch.nn.SyncBatchNorm.convert_sync_batchnorm`` normalises with the statistics of every rank's clips when a process
    group of more than one rank is initialised (ranks may hold different clip counts, none zero); average the gradients afterwards
    (``syncfusion_amd.allreduce_gradients``).  ``_force_sync`` (tests, tools) sends every BatchNorm through the split-phase kernels whatever
    the module type and the world size."""
    N, _, T, H, W = x.shape
    trunk = net.net.model
    # without a process group (and unforced) no module can take the synchronised path: the step is today's, with nothing added per layer
    sync = _SyncState(N, x.device, _force_sync) if _force_sync or (dist.is_available() and dist.is_initialized()) else None
    if N == 0:
        # a rank whose shard is empty still joins the clip-count gather, so that EVERY rank of the group raises instead of waiting for it
        if sync is not None:
            sync.group_for(trunk.stem[1])
        raise ValueError("onset training: empty batch (0 clips)")
    a = _Act(frames_to_rows(x), N, T, H, W, sync)
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


# ---- the whole step from one graph ---------------------------------------------------------------------------------------------------------
class GraphedOnsetTrainStep:
    """``module_onset.Model.training_step`` + ``loss.backward()`` captured ONCE in a HIP graph and replayed per step (static batch shape): the
    onset counterpart of ``training.GraphedTrainStep``, with the same rules.

    The model must carry the device loss (``Model(..., loss="hip")``): ``BCLoss.evaluate`` reads the logits back on every step, which a
    capture cannot hold.  ``batch`` is ``{"frames": (N, 3, T, H, W), "label": (N, T)}``; both are copied into static buffers.

        gs = GraphedOnsetTrainStep(model, example_batch, optimizer=opt)   # build it BEFORE the first eager backward on these parameters
        for batch in loader:
            loss = gs.step(batch)                                         # copy-in, replay; gs.metrics = [AP, Acc, OnsNumAcc] of the step

    ``loss`` and ``metrics`` are static device tensors that every replay overwrites (read them after the step, outside a timed loop).
    Gradients land in the ``.grad`` tensors the capture allocated: do NOT ``zero_grad(set_to_none=True)`` afterwards.  With ``optimizer=`` a
    ``syncfusion_amd.optim.AdamW`` its step (clipping included when ``max_grad_norm`` is set) is captured behind the backward pass, and
    ``gs.step(batch)`` is the WHOLE training step; any other optimizer is stepped by the caller after ``gs.step()``.

    Constructing the object does not train the model: the warm-up passes update the BatchNorm running statistics and ``num_batches_tracked``
    (and one warm-up ``optimizer.step()`` moves parameters, moments and step counters); all of them are put back before the capture.  Every
    ``step()`` advances the version counters of what the graph writes -- the running buffers, and the parameters when the optimizer is
    captured -- so ``net.eval()`` rebuilds the inference engine as it does after an eager step.

    Refused: more than one rank (the gradient all-reduce and the BatchNorm collectives run between the kernels) and a net with
    ``nn.SyncBatchNorm`` modules while a process group is initialised."""

    def __init__(self, model, batch, warmup: int = 2, optimizer=None):
        from .onset_loss import DeviceBCLoss
        from .optim import AdamW

        if not isinstance(getattr(model, "loss", None), DeviceBCLoss):
            raise ValueError('GraphedOnsetTrainStep: the model must be built with loss="hip" (syncfusion_amd.onset_loss.DeviceBCLoss): '
                             f"{type(getattr(model, 'loss', None)).__name__}.evaluate reads the logits back on the host, which a capture cannot hold")
        if optimizer is not None and not isinstance(optimizer, AdamW):
            raise TypeError(f"GraphedOnsetTrainStep: only syncfusion_amd.optim.AdamW can be captured with the step, got {type(optimizer).__name__} "
                            "(step any other optimizer after gs.step(), with optimizer=None)")
        if dist.is_available() and dist.is_initialized():
            if dist.get_world_size() > 1:
                raise RuntimeError("GraphedOnsetTrainStep: capture is supported on the single-rank path only (the gradient all-reduce and the "
                                   "collectives of a synchronised BatchNorm run between the kernels)")
            if any(isinstance(m, nn.SyncBatchNorm) for m in model.modules()):
                raise RuntimeError("GraphedOnsetTrainStep: the net holds nn.SyncBatchNorm modules and a process group is initialised: a step with "
                                   "synchronised BatchNorm cannot be captured into a HIP graph")
        if not model.model.training:
            raise RuntimeError("GraphedOnsetTrainStep: the onset net is in eval mode; call .train() first")
        self.model, self.optimizer = model, optimizer
        self.batch = {"frames": batch["frames"].clone(), "label": batch["label"].clone()}
        params = [p for p in model.parameters() if p.requires_grad]
        buffers = [b for b in model.buffers() if b is not None]
        keep = [b.detach().clone() for b in buffers]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):     # warm-up on a side stream: allocator pools, lazy kernel loads, the growing workspace, .grad allocation
            for _ in range(max(1, warmup)):
                for p in params:
                    p.grad = None
                self._fwd_bwd()
            if optimizer is not None:
                self._warm_optimizer()
            with torch.no_grad():
                for b, k in zip(buffers, keep):
                    b.copy_(k)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for p in params:
            p.grad = None
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = self._fwd_bwd()
            if optimizer is not None:
                optimizer.step()
        self.metrics = model.loss.last_metrics
        if optimizer is not None:
            optimizer.sync_device_state()   # the table of the gradients the capture allocated: uploaded now, the captured kernels hold its address
        self._written = buffers + ([p for group in optimizer.param_groups for p in group["params"]] if optimizer is not None else [])

    def _warm_optimizer(self) -> None:
        from .training import GraphedTrainStep

        GraphedTrainStep._warm_optimizer(self)   # one real step on the warm-up's gradients, then parameters, moments and counters put back

    def _fwd_bwd(self) -> Tensor:
        loss = self.model.training_step(self.batch, 0)
        loss.backward()
        return loss

    def step(self, batch=None) -> Tensor:
        """Copy ``batch`` (same shapes as the example) into the static buffers and replay.  Returns the static loss tensor."""
        if batch is not None:
            self.batch["frames"].copy_(batch["frames"])
            self.batch["label"].copy_(batch["label"])
        if self.optimizer is not None:
            self.optimizer.sync_device_state()
        self.graph.replay()
        _bump(*self._written)
        return self.loss
