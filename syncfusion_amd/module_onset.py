"""Boundary object of the onset net's training: mirror of ``main.module_onset.Model`` (main/module_onset.py:22-130, 268-354).

Same constructor arguments and attribute (``model``: checkpoint keys ``model.net.model.*`` / ``model.fc.*``), the same AdamW set-up, the
same ``common_step`` / ``training_step`` / ``validation_step`` / ``test_step`` returning the loss, and the same ``BCLoss`` (class-balanced
``BCEWithLogitsLoss``) with its ``evaluate`` metrics (AP, Acc, OnsNumAcc).  ``pytorch_lightning`` is the base class when it imports,
otherwise the ``torch.nn.Module`` fallback of ``syncfusion_amd/module.py`` (``log`` is a no-op).

The test stage (:99-129, 142-229: ``log_annotations`` per batch, ``concat_annotations`` at the end of the epoch) is
``syncfusion_amd/onset_test.py``: ``Model(..., annotations_dir=DIR)`` makes ``test_step`` feed an ``OnsetTestStage`` with the logits
``common_step`` computed (no second forward) whenever the batch carries ``video_name`` / ``start_frame`` / ``end_frame`` / ``frame_rate``,
and ``on_test_epoch_end()`` finish it: ``DIR/media/annotations/{target,pred}/{video}.times.csv`` and ``test_results``.  With the default
(``None``) ``test_step`` returns the loss and writes nothing, as before.  ``log_labels`` (wandb plots) is not mirrored;
``syncfusion_amd.onsets_to_track`` is the in-memory, one-clip form of the logits -> onset times hand-off.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from .module import _Base, check_optimizer_choice, make_adamw
from .onset_net import VideoOnsetNet

Tensor = torch.Tensor


def average_precision(target: np.ndarray, score: np.ndarray) -> float:
    """``sklearn.metrics.average_precision_score`` for binary labels: sum over the distinct score thresholds (descending) of
    (recall step) * precision, ties resolved as one threshold."""
    target = np.asarray(target).reshape(-1).astype(np.float64)
    score = np.asarray(score).reshape(-1).astype(np.float64)
    order = np.argsort(-score, kind="mergesort")
    score, target = score[order], target[order]
    last = np.r_[np.nonzero(np.diff(score))[0], score.size - 1]   # last index of every distinct score
    tps = np.cumsum(target)[last]
    fps = (last + 1) - tps
    if tps.size == 0 or tps[-1] == 0:
        return float("nan")   # (sklearn warns and returns nan-equivalent: no positive sample)
    precision = tps / (tps + fps)
    recall = tps / tps[-1]
    recall_prev = np.r_[0.0, recall[:-1]]
    return float(np.sum((recall - recall_prev) * precision))


class BCLoss(nn.Module):
    """main/module_onset.py:268-354.  ``forward``: ``BCEWithLogitsLoss(pos_weight = (n - sum t) / sum t)`` over the flattened logits; as in
    the reference, a batch without positive labels gives ``pos_weight = inf`` and the loss is inf / nan."""

    def __init__(self):
        super().__init__()
        self.threshold = 0.75

    def forward(self, pred: Tensor, target: Tensor) -> Tensor:
        pred = pred.contiguous().view(-1)
        target = target.contiguous().view(-1)
        pos_weight = (target.shape[0] - target.sum()) / target.sum()
        criterion = nn.BCEWithLogitsLoss(pos_weight=pos_weight).to(pred.device)
        return criterion(pred, target.float())

    def evaluate(self, pred: Tensor, target: Tensor) -> Dict[str, float]:
        ons_num_acc = self.onset_num_acc(pred, target)
        pred = torch.sigmoid(pred.detach().contiguous().view(-1)).cpu().numpy()
        target = target.detach().contiguous().view(-1).cpu().numpy()
        pos_index = np.nonzero(target == 1)[0]
        neg_index = np.nonzero(target == 0)[0]
        balance_num = min(pos_index.shape[0], neg_index.shape[0])   # the first balance_num positives and negatives
        index = np.concatenate((pos_index[:balance_num], neg_index[:balance_num]), axis=0)
        pred, target = pred[index], target[index]
        return {"AP": average_precision(target, pred), "Acc": self.binary_acc(pred, target), "OnsNumAcc": ons_num_acc}

    def binary_acc(self, pred: np.ndarray, target: np.ndarray) -> float:
        pred = np.where(pred > self.threshold, 1.0, 0.0)
        return np.sum(pred == target) / target.shape[0]

    def onset_num_acc(self, pred: Tensor, target: Tensor) -> float:
        p = torch.sigmoid(pred.detach()).cpu().numpy()
        t = target.detach().cpu().numpy().astype(int)
        p = (p > self.threshold).astype(int)
        for i in range(p.shape[0]):              # remove consecutive onsets (the later frame of a pair, left to right)
            for j in range(p.shape[-1] - 1):
                if p[i][j] == 1 and p[i][j + 1] == 1:
                    p[i][j + 1] = 0
        return np.sum(np.sum(p, axis=-1) == np.sum(t, axis=-1)) / len(p)


LOSSES = ("torch", "hip")


def check_loss_choice(loss: str) -> str:
    """The ``loss`` init-arg of ``Model``: ``"torch"`` (default: ``BCLoss``, ATen loss and host-side metrics, Python floats) or ``"hip"``
    (``syncfusion_amd.onset_loss.DeviceBCLoss``: loss, gradient and metrics in the HIP library, metrics as device tensors, no host read)."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
    return loss


class Model(_Base):
    """Drop-in for ``main.module_onset.Model`` (cfg/model/model-onset.yaml ``class_path``)."""

    def __init__(self, lr: float, lr_beta1: float, lr_beta2: float, lr_eps: float, lr_weight_decay: float, onset_model: VideoOnsetNet,
                 optimizer: str = "torch", loss: str = "torch", annotations_dir: Optional[str] = None):
        super().__init__()
        self.annotations_dir = annotations_dir
        self.test_stage = None              # syncfusion_amd.onset_test.OnsetTestStage, created by the first annotated test batch
        self.test_results: Optional[dict] = None
        self.optimizer = check_optimizer_choice(optimizer)
        self.loss_choice = check_loss_choice(loss)
        self.lr = lr
        self.lr_beta1 = lr_beta1
        self.lr_beta2 = lr_beta2
        self.lr_eps = lr_eps
        self.lr_weight_decay = lr_weight_decay
        self.model: VideoOnsetNet = onset_model
        if self.loss_choice == "hip":
            from .onset_loss import DeviceBCLoss

            self.loss = DeviceBCLoss()
        else:
            self.loss = BCLoss()

    def configure_optimizers(self) -> torch.optim.Optimizer:
        # the single-kernel multi-tensor AdamW on the GPU; optimizer="hip": syncfusion_amd.optim.AdamW (module.py, make_adamw)
        return make_adamw(list(self.model.parameters()), self.optimizer, lr=self.lr, betas=(self.lr_beta1, self.lr_beta2), eps=self.lr_eps,
                          weight_decay=self.lr_weight_decay)

    def common_step(self, batch, batch_idx, mode: str = "train"):
        frames, labels = batch["frames"], batch["label"]
        pred = self.model(frames)
        loss = self.loss(pred, labels)
        metrics = self.loss.evaluate(pred, labels)
        return loss, metrics

    def log_metrics(self, metrics: Dict[str, object], mode: str = "val") -> None:
        for key, value in metrics.items():
            self.log(f"metrics/{mode}/{key}", value, on_step=False, on_epoch=True, prog_bar=True, logger=True, sync_dist=True)

    def _step(self, batch, batch_idx, mode: str) -> Tensor:
        loss, metrics = self.common_step(batch, batch_idx, mode=mode)
        self.log(f"loss/{mode}", loss, on_step=False, on_epoch=True, prog_bar=True, logger=True, sync_dist=True)
        self.log_metrics(metrics, mode=mode)
        return loss

    def training_step(self, batch, batch_idx) -> Tensor:
        return self._step(batch, batch_idx, "train")

    def validation_step(self, batch, batch_idx) -> Tensor:
        return self._step(batch, batch_idx, "val")

    def test_step(self, batch, batch_idx) -> Tensor:
        if self.annotations_dir is None or "video_name" not in batch:
            return self._step(batch, batch_idx, "test")
        from .onset_test import OnsetTestStage, batch_chunks

        frames, labels = batch["frames"], batch["label"]
        pred = self.model(frames)                      # the one forward of the batch: loss, metrics and annotations read these logits
        loss = self.loss(pred, labels)
        self.log("loss/test", loss, on_step=False, on_epoch=True, prog_bar=True, logger=True, sync_dist=True)
        self.log_metrics(self.loss.evaluate(pred, labels), mode="test")
        if self.test_stage is None:
            self.test_stage = OnsetTestStage(self, self.annotations_dir)
        self.test_stage.step_logits(pred.detach(), labels, batch_chunks(batch))
        return loss

    def on_test_epoch_end(self) -> None:
        """``concat_annotations`` (main/module_onset.py:127-128, 185-229): the merged files under ``annotations_dir`` and ``test_results``."""
        if self.test_stage is not None:
            self.test_results = self.test_stage.finish()
