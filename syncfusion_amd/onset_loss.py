"""The end of the onset net's training step on the device: ``main.module_onset.BCLoss`` (main/module_onset.py:268-354) without the host.

``BCLoss.forward`` is a handful of ATen launches; ``BCLoss.evaluate`` -- called on EVERY training / validation / test step
(main/module_onset.py:50-55) -- copies logits and labels to the host three times, removes consecutive onsets in a Python double loop over
every (clip, frame) and sorts in numpy for the average precision.  The host therefore waits for the end of every step, and the step cannot
be captured into a HIP graph.  Here the same numbers come from ``syncfusion_amd/csrc/onset_loss.hip``:

* ``balanced_bce(logits, target)``  -- the class-balanced BCE-with-logits loss as a ``torch.autograd.Function`` over ``sf_op_onset_bce_fwd`` /
  ``sf_op_onset_bce_bwd`` (``pos_weight`` is computed on the device and never read back; the upstream gradient is read from the device);
* ``step_metrics(logits, target)``  -- ``[AP, Acc, OnsNumAcc]`` as a (3,) float64 device tensor (``sf_op_onset_metrics``);
* ``DeviceBCLoss``                  -- the reference's surface (``threshold``, ``forward``, ``evaluate``) on the two; ``evaluate`` returns
  0-d device tensors.

No call reads from the device or synchronises, workspaces come from torch's allocator, and nothing that changes per step is a kernel
argument: all of it runs inside a stream capture (``onset_training.GraphedOnsetTrainStep``).  Opt-in: ``module_onset.Model(..., loss="hip")``.

Where the reference is undefined the device path is defined: a batch that holds one class only has an empty balanced subset, for which
``BCLoss.evaluate`` raises (``average_precision``) -- here AP and Acc are NaN and OnsNumAcc is computed as usual.  A batch without positive
labels gives a non-finite loss and gradient, as the reference does.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib

Tensor = torch.Tensor

METRIC_NAMES = ("AP", "Acc", "OnsNumAcc")


def _flat_inputs(logits: Tensor, target: Tensor, where: str):
    _lib.require_gpu_tensor(logits, where)
    if logits.dtype != torch.float32:
        raise TypeError(f"{where}: fp32 logits expected (the onset net trains in fp32), got {logits.dtype}")
    if target.device != logits.device or target.numel() != logits.numel():
        raise ValueError(f"{where}: logits {tuple(logits.shape)} on {logits.device} and target {tuple(target.shape)} on {target.device} do not match")
    if logits.numel() < 1:
        raise ValueError(f"{where}: empty batch")
    return logits.detach().contiguous().view(-1), target.detach().contiguous().view(-1).float()


def _workspace(n: int, device: torch.device) -> Tensor:
    need = int(_lib.load().sf_op_onset_loss_workspace_bytes(n))
    if need < 0:
        raise ValueError(f"onset loss: {n} elements are out of range")
    return torch.empty(need, dtype=torch.uint8, device=device)


class _BalancedBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor) -> Tensor:
        z, t = _flat_inputs(logits, target, "balanced_bce")
        lib = _lib.load()
        n = z.numel()
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        stats = torch.empty(2, dtype=torch.float32, device=z.device)     # (sum t, pos_weight)
        ws = _workspace(n, z.device)
        with torch.cuda.device(z.device):
            _lib.check(lib.sf_op_onset_bce_fwd(z.data_ptr(), t.data_ptr(), n, loss.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                               _lib.stream_ptr(z.device)), "sf_op_onset_bce_fwd")
        ctx.save_for_backward(z, t, stats)
        ctx.shape = logits.shape
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        z, t, stats = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        dz = torch.empty_like(z)
        with torch.cuda.device(z.device):
            _lib.check(_lib.load().sf_op_onset_bce_bwd(z.data_ptr(), t.data_ptr(), stats.data_ptr(), g.data_ptr(), z.numel(), dz.data_ptr(),
                                                       _lib.stream_ptr(z.device)), "sf_op_onset_bce_bwd")
        return dz.view(ctx.shape), None


def balanced_bce(logits: Tensor, target: Tensor) -> Tensor:
    """``BCEWithLogitsLoss(pos_weight=(n - sum t) / sum t)(logits.view(-1), target.view(-1).float())`` (main/module_onset.py:274-286): a 0-d
    fp32 device tensor with an autograd graph onto ``logits``.  Labels of another dtype are cast with ``.float()`` on the device."""
    return _BalancedBCE.apply(logits, target)


def step_metrics(logits: Tensor, target: Tensor, threshold: float = 0.75) -> Tensor:
    """``[AP, Acc, OnsNumAcc]`` of ``BCLoss.evaluate`` (main/module_onset.py:288-354) for (N, T) logits and 0 / 1 labels: a (3,) float64
    tensor on the logits' device.  A batch with one class only: AP = Acc = NaN."""
    if logits.dim() != 2:
        raise ValueError(f"step_metrics: (N, T) logits expected, got {tuple(logits.shape)}")
    z, t = _flat_inputs(logits, target, "step_metrics")
    N, T = logits.shape
    out = torch.empty(3, dtype=torch.float64, device=z.device)
    ws = _workspace(N * T, z.device)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().sf_op_onset_metrics(z.data_ptr(), t.data_ptr(), N, T, float(threshold), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   _lib.stream_ptr(z.device)), "sf_op_onset_metrics")
    return out


class DeviceBCLoss(nn.Module):
    """``BCLoss`` on the HIP kernels.  ``forward`` returns the loss, ``evaluate`` the metrics as 0-d float64 device tensors (views of
    ``last_metrics``, the (3,) tensor of the latest call: what a captured step keeps as its static metrics)."""

    def __init__(self):
        super().__init__()
        self.threshold = 0.75
        self.last_metrics: Optional[Tensor] = None

    def forward(self, pred: Tensor, target: Tensor) -> Tensor:
        return balanced_bce(pred, target)

    def evaluate(self, pred: Tensor, target: Tensor) -> Dict[str, Tensor]:
        m = step_metrics(pred, target, self.threshold)
        self.last_metrics = m
        return {name: m[i] for i, name in enumerate(METRIC_NAMES)}
