"""The onset net's TEST stage: what ``main.module_onset.Model`` does between ``trainer.test`` and the predicted-onset shard
(main/module_onset.py:99-129 ``test_step`` / ``on_test_epoch_end``, :142-183 ``log_annotations``, :185-229 ``concat_annotations``), and the
packing of the resulting files into the ``times.pred.csv`` members ``syncfusion_amd.shards`` reads.

The reference runs the net up to three times per test batch (``common_step``, ``log_annotations``, every tenth batch ``log_labels``),
copies logits and labels to the host for the metrics and again for the thresholding, writes one csv per chunk and per kind, and at the end
of the epoch reads them all back (``np.loadtxt``), merges them per video in ``natsorted`` order, and deletes them.  Here a batch is ONE
eval forward and one ``sf_op_onset_test_step`` (csrc/onset_test.hip): the thresholded frames of every clip are compacted into epoch tables
on the device and the loss / metric sums of the epoch accumulate there; ``OnsetTestStage.step`` never synchronises, ``finish`` makes the
one device-to-host copy of the stage and writes the merged files directly.  The new device code is small; what this module adds is the
closed workflow.

* ``annotation_rows(logits, labels)``    the thresholded frame indices of one batch (device tensors: the HIP entry; CPU tensors: numpy);
* ``OnsetTestStage``                      ``step`` per batch, ``finish`` -> epoch figures, per-video onset times and the merged csv files;
* ``test_onset_model``                    frame directory -> ``chunk_table`` -> frames -> stage -> ``finish`` (``script/test_onset_model.sh``);
* ``pack_onset_preds``                    a shard plus a directory of ``<video>.times.csv`` -> a shard whose samples carry ``times.pred.csv``.

File contents.  The time of onset frame ``idx`` of a chunk is ``(idx + start_frame) / frame_rate`` in float64, written ``"%.4f\\n"``; a
video's chunks follow each other as ``natsorted`` orders the reference's per-chunk names ``{video}.{start}-{end}.times.csv`` (by start
frame, numerically: ``video_chunks.natural_sorted``); a video without onsets gives an empty file.  Going through the per-chunk files (write
``%.4f``, parse, write ``%.4f``) changes no byte, so they are not written.  The reference's "remove consecutive onsets" loop (:170-172)
compares index VALUES with 1 and never removes anything; it is not "fixed" here.  The reference recovers the video name as the text before
the first ``.`` of a file name, so a name with a dot would be merged under another name: such a name raises ``ValueError``.
``log_labels`` (wandb plots) is not mirrored.

Epoch figures.  ``loss/test`` and ``metrics/test/*`` are ``sums[k] / sums[4]`` of the device accumulator, the mean over batches weighted by
batch size: what Lightning's ``self.log(..., on_step=False, on_epoch=True)`` reduces to.  Lightning accumulates in fp32, this stage in
fp64.  UNPINNED: pytorch_lightning is not installed where this was written, so the statement about its reduction rests on its
documentation, not on a run.  A batch that holds one class only makes AP and Acc NaN for the epoch (``onset_loss.py``); the reference
raises there.
"""
from __future__ import annotations

import collections
import io
import math
import os
import tarfile
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .shards import _split_key
from .video_chunks import chunk_frames_u8, chunk_table, iter_clips, natural_sorted

Tensor = torch.Tensor

LOGIT_THRESHOLD = 0.5      # main/module_onset.py:162, on the raw logit
METRIC_THRESHOLD = 0.75    # BCLoss.threshold, on the sigmoid
FIGURES = ("loss/test", "metrics/test/AP", "metrics/test/Acc", "metrics/test/OnsNumAcc")


def _check_batch(logits: Tensor, labels: Tensor, where: str) -> Tuple[int, int]:
    if logits.dim() != 2 or tuple(labels.shape) != tuple(logits.shape) or labels.device != logits.device:
        raise ValueError(f"{where}: (N, T) logits and labels of the same shape on one device expected, got {tuple(logits.shape)} on "
                         f"{logits.device} and {tuple(labels.shape)} on {labels.device}")
    N, T = int(logits.shape[0]), int(logits.shape[1])
    if N < 1 or T < 1:
        raise ValueError(f"{where}: empty batch")
    return N, T


def _host_rows(mask: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(N, T) bool -> (count (N,), frames (N, T) with the set indices first, ascending, then -1), int32."""
    N, T = mask.shape
    frames = np.full((N, T), -1, dtype=np.int32)
    count = mask.sum(axis=1).astype(np.int32)
    for n in range(N):
        frames[n, :count[n]] = np.nonzero(mask[n])[0]
    return count, frames


def _device_step(logits: Tensor, labels: Tensor, threshold: float, clip0: int, capacity: int, tables: Sequence[Tensor], sums: Tensor) -> None:
    """One ``sf_op_onset_test_step`` on the current stream: rows [clip0, clip0 + N) of the tables, ``sums`` += this batch."""
    N, T = int(logits.shape[0]), int(logits.shape[1])
    lib = _lib.load()
    need = int(lib.sf_op_onset_test_workspace_bytes(N, T))
    if need < 0:
        raise ValueError(f"onset test step: a batch of {N} x {T} logits is out of range (at most 2^24)")
    z = logits.detach().to(torch.float32).contiguous()
    t = labels.detach().to(torch.float32).contiguous()
    ws = torch.empty(need, dtype=torch.uint8, device=z.device)
    pc, pf, tc, tf = tables
    with torch.cuda.device(z.device):
        _lib.check(lib.sf_op_onset_test_step(z.data_ptr(), t.data_ptr(), N, T, float(threshold), METRIC_THRESHOLD, int(clip0), int(capacity),
                                             pc.data_ptr(), pf.data_ptr(), tc.data_ptr(), tf.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _lib.stream_ptr(z.device)), "sf_op_onset_test_step")


def _new_tables(capacity: int, T: int, device) -> List[Tensor]:
    return [torch.empty(capacity, dtype=torch.int32, device=device), torch.empty((capacity, T), dtype=torch.int32, device=device),
            torch.empty(capacity, dtype=torch.int32, device=device), torch.empty((capacity, T), dtype=torch.int32, device=device)]


@torch.no_grad()
def annotation_rows(logits: Tensor, labels: Tensor, threshold: float = LOGIT_THRESHOLD) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(pred_count (N,), pred_frames (N, T), target_count (N,), target_frames (N, T))``, int32 on the inputs' device, for one batch of
    (N, T) raw logits and labels: row n of ``pred_frames`` starts with the frames whose logit exceeds ``threshold`` (ascending; NaN is no
    onset), of ``target_frames`` with the frames whose label is non-zero, and ends in -1.  Device tensors run ``sf_op_onset_test_step``
    (clip0 = 0, capacity = N); CPU tensors take numpy."""
    N, T = _check_batch(logits, labels, "annotation_rows")
    if not logits.is_cuda:
        z = logits.detach().to(torch.float32).numpy()
        with np.errstate(invalid="ignore"):
            pc, pf = _host_rows(z > np.float32(threshold))
        tc, tf = _host_rows(labels.detach().numpy() != 0)
        return torch.from_numpy(pc), torch.from_numpy(pf), torch.from_numpy(tc), torch.from_numpy(tf)
    tables = _new_tables(N, T, logits.device)
    sums = torch.zeros(5, dtype=torch.float64, device=logits.device)
    _device_step(logits, labels, threshold, 0, N, tables, sums)
    return tuple(tables)


def _chunk_meta(chunk) -> Tuple[str, int, int, object]:
    name = str(chunk["video_name"])
    rate = chunk["frame_rate"]
    if isinstance(rate, torch.Tensor):
        rate = rate.item()
    if "." in name:
        raise ValueError(f"video_name {name!r} contains '.': the reference takes the text before the first dot of a file name as the video "
                         "name (main/module_onset.py:195) and would merge this video's chunks under another name")
    return name, int(chunk["start_frame"]), int(chunk["end_frame"]), rate


def batch_chunks(batch: dict) -> List[dict]:
    """The per-clip records of a collated test batch (``video_name``: N names; ``start_frame`` / ``end_frame`` / ``frame_rate``: N-element
    tensors or sequences, as the reference's DataLoader stacks them) in the form ``video_chunks.chunk_table`` gives them."""
    def column(key):
        v = batch[key]
        return v.tolist() if isinstance(v, torch.Tensor) else list(v)

    cols = [column(k) for k in ("video_name", "start_frame", "end_frame", "frame_rate")]
    return [dict(video_name=n, start_frame=s, end_frame=e, frame_rate=r) for n, s, e, r in zip(*cols)]


def merge_video_times(metas: Sequence[Tuple[str, int, int, object]], frames: Sequence[np.ndarray]) -> Dict[str, List[float]]:
    """Per video, the onset times of its chunks in the order of ``concat_annotations``: chunk i has the onset frame indices ``frames[i]``
    and ``metas[i] = (video_name, start_frame, end_frame, frame_rate)``.  Times are the 4-decimal values the files hold.  Two chunks of one
    name (the same video and frame range) are one file in the reference: the later one wins."""
    per_video: Dict[str, Dict[str, List[float]]] = {}
    for (name, start, end, rate), idx in zip(metas, frames):
        times = (np.asarray(idx, dtype=np.int64) + start) / rate             # float64, :175-176
        per_video.setdefault(name, {})[f"{name}.{start}-{end}.times.csv"] = [float("%.4f" % v) for v in np.atleast_1d(times)]
    return {name: [v for f in natural_sorted(list(files)) for v in files[f]] for name, files in per_video.items()}


def write_times(path: str, times: Sequence[float]) -> None:
    with open(path, "w") as f:
        f.write("".join("%.4f\n" % v for v in times))


class OnsetTestStage:
    """The test epoch of an onset model.  ``model``: an ``OnsetModel`` (its ``.model`` is the net) or a bare ``VideoOnsetNet``; it is put
    into eval mode.  ``out_dir``: where ``finish`` writes ``media/annotations/{target,pred}/{video_name}.times.csv`` (None: no files).
    ``capacity``: the first size of the epoch tables in clips (they grow by doubling; pass the clip count of the epoch to allocate once).

    On a GPU the tables ``(capacity,)`` / ``(capacity, T)`` and the five fp64 sums live on the device; ``step`` queues work on the current
    stream and returns, ``finish`` reads them once.  With CPU logits (``step_logits`` only: the net has no CPU path) the same figures come
    from ``BCLoss`` and numpy."""

    def __init__(self, model, out_dir: Optional[str] = None, capacity: Optional[int] = None):
        from .onset_net import VideoOnsetNet

        self.net = model if isinstance(model, VideoOnsetNet) else model.model
        self.out_dir = out_dir
        if capacity is not None and capacity < 1:
            raise ValueError(f"capacity must be >= 1, got {capacity}")
        self._first_capacity = int(capacity) if capacity else 256
        self.reset()

    def reset(self) -> None:
        self.capacity = 0
        self.clips = 0
        self.T: Optional[int] = None
        self._tables: Optional[List[Tensor]] = None
        self._sums: Optional[Tensor] = None
        self._metas: List[Tuple[str, int, int, object]] = []
        self._host: Optional[List[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]] = None
        self._host_sums = np.zeros(5, dtype=np.float64)

    # ---- per batch ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, frames: Tensor, labels: Tensor, chunks: Sequence[dict]) -> Tensor:
        """One test batch: (N, 3, T, H, W) frames and (N, T) labels on the GPU, ``chunks`` the N dicts of ``video_chunks.chunk_table``
        (``video_name``, ``start_frame``, ``end_frame``, ``frame_rate``).  One eval forward, one device step, no host synchronisation.
        Returns the logits."""
        self.net.eval()
        logits = self.net(frames)
        self.step_logits(logits, labels.to(logits.device), chunks)
        return logits

    @torch.no_grad()
    def step_logits(self, logits: Tensor, labels: Tensor, chunks: Sequence[dict]) -> None:
        """``step`` for logits that exist already (``OnsetModel.test_step`` has them from ``common_step``)."""
        N, T = _check_batch(logits, labels, "OnsetTestStage.step")
        if len(chunks) != N:
            raise ValueError(f"OnsetTestStage.step: {N} clips but {len(chunks)} chunk records")
        metas = [_chunk_meta(c) for c in chunks]
        if self.T is None:
            self.T = T
        elif T != self.T:
            raise ValueError(f"OnsetTestStage.step: clips of {T} frames after clips of {self.T}: one stage takes one clip length "
                             "(the reference's DataLoader stacks clips of one length)")
        if logits.is_cuda:
            if self._host is not None:
                raise ValueError("OnsetTestStage.step: device logits after CPU logits in one epoch")
            self._reserve(self.clips + N, logits.device)
            _device_step(logits, labels, LOGIT_THRESHOLD, self.clips, self.capacity, self._tables, self._sums)
        else:
            if self._tables is not None:
                raise ValueError("OnsetTestStage.step: CPU logits after device logits in one epoch")
            self._host_step(logits, labels, N)
        self._metas += metas
        self.clips += N

    def _reserve(self, need: int, device) -> None:
        if self._tables is None:
            self.capacity = max(self._first_capacity, need)
            self._tables = _new_tables(self.capacity, self.T, device)
            self._sums = torch.zeros(5, dtype=torch.float64, device=device)
            return
        if need <= self.capacity:
            return
        cap = self.capacity
        while cap < need:
            cap *= 2
        grown = _new_tables(cap, self.T, device)
        for new, old in zip(grown, self._tables):          # device-to-device on the current stream, behind the steps that wrote the rows
            new[: self.clips].copy_(old[: self.clips])
        self._tables, self.capacity = grown, cap

    def _host_step(self, logits: Tensor, labels: Tensor, N: int) -> None:
        from .module_onset import BCLoss

        if self._host is None:
            self._host = []
        rows = annotation_rows(logits, labels)
        self._host.append(tuple(r.numpy() for r in rows))
        crit = BCLoss()
        m = crit.evaluate(logits, labels)
        self._host_sums += N * np.array([float(crit(logits.detach(), labels)), m["AP"], m["Acc"], m["OnsNumAcc"], 1.0], dtype=np.float64)

    # ---- end of the epoch -----------------------------------------------------------------------------------------------------------------
    def _read(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        n = self.clips
        if self._tables is not None:
            pc, pf, tc, tf = self._tables
            packed = torch.cat([self._sums.view(torch.int32), pc[:n], tc[:n], pf[:n].reshape(-1), tf[:n].reshape(-1)]).cpu()   # THE copy
            a = packed.numpy()
            sums = a[:10].copy().view(np.float64)
            rest = a[10:]
            return sums, rest[:n], rest[2 * n: 2 * n + n * self.T].reshape(n, self.T), rest[n: 2 * n], rest[2 * n + n * self.T:].reshape(n, self.T)
        if self._host:
            pc, pf, tc, tf = (np.concatenate([h[k] for h in self._host]) for k in range(4))
            return self._host_sums, pc, pf, tc, tf
        z = np.zeros((0, 1), dtype=np.int32)
        return self._host_sums, z[:, 0], z, z[:, 0], z

    def finish(self) -> dict:
        """Ends the epoch: one device-to-host copy (tables and sums in one buffer), then the epoch figures
        ``{"loss/test", "metrics/test/AP", "metrics/test/Acc", "metrics/test/OnsNumAcc"}`` (means over batches weighted by batch size,
        accumulated in fp64; NaN without a batch), ``"videos": {name: {"target": [...], "pred": [...]}}`` with the times the files hold,
        and -- with ``out_dir`` -- the files themselves.  The stage is empty afterwards."""
        sums, pc, pf, tc, tf = self._read()
        out: dict = {k: (float(sums[i] / sums[4]) if sums[4] > 0 else math.nan) for i, k in enumerate(FIGURES)}
        pred = merge_video_times(self._metas, [pf[i, : pc[i]] for i in range(self.clips)])
        target = merge_video_times(self._metas, [tf[i, : tc[i]] for i in range(self.clips)])
        out["videos"] = {name: {"target": target[name], "pred": pred[name]} for name in pred}
        if self.out_dir is not None:
            for kind in ("target", "pred"):
                d = os.path.join(self.out_dir, "media", "annotations", kind)
                os.makedirs(d, exist_ok=True)
                for name, v in out["videos"].items():
                    write_times(os.path.join(d, f"{name}.times.csv"), v[kind])
        self.reset()
        return out


# ---- the stage over a frame directory ---------------------------------------------------------------------------------------------------
def _read_samples(samples_or_split_file: Union[str, Sequence[str]]) -> List[str]:
    if isinstance(samples_or_split_file, (str, os.PathLike)):
        with open(samples_or_split_file, "r") as f:                      # main/dataset_onset.py:53-54
            return [s for s in f.read().splitlines() if s.strip()]
    return list(samples_or_split_file)


def _prefetched_clips(chunks: Sequence[dict], batch_size: int, device, frame_file_suffix: str, frames_transforms,
                      num_workers: int) -> Iterator[Tuple[Tensor, Tensor, List[dict]]]:
    """``iter_clips`` (no shuffle) with the frames of the next batches decoded by ``num_workers`` threads while the device works on this
    one; the device side of a batch is the one ``iter_clips`` runs, so both give the same clips."""
    from .input_pipeline import frames_to_clip

    parts = [list(chunks[i: i + batch_size]) for i in range(0, len(chunks), batch_size)]
    ahead = 1 + -(-num_workers // max(1, batch_size))
    with ThreadPoolExecutor(max_workers=num_workers) as pool:
        def submit(part):
            return part, [pool.submit(chunk_frames_u8, c, frame_file_suffix, False) for c in part]

        it = iter(parts)
        pending = collections.deque(submit(p) for _, p in zip(range(ahead), it))
        while pending:
            part, futures = pending.popleft()
            nxt = next(it, None)
            if nxt is not None:
                pending.append(submit(nxt))
            frames = [f.result() for f in futures]
            if frames_transforms is None:
                clips = torch.stack([frames_to_clip(u8.pin_memory().to(device, non_blocking=True)[None], (112, 112))[0] for u8 in frames])
            else:
                if any(f.shape != frames[0].shape for f in frames):
                    raise ValueError("chunks of one batch differ in frame count or frame size")
                clips = frames_transforms(torch.stack(frames).pin_memory().to(device, non_blocking=True), generator=None)
            yield clips, torch.stack([c["labels"] for c in part]).to(device), part


@torch.no_grad()
def test_onset_model(model, root_dir: str, samples_or_split_file: Union[str, Sequence[str]], out_dir: Optional[str], batch_size: int = 16,
                     frames_transforms=None, frame_file_suffix: str = ".jpg", num_workers: int = 0, device="cuda") -> dict:
    """``script/test_onset_model.sh`` for a frame directory (layout: ``video_chunks``): the chunk table of the listed samples (a sequence
    of names or a split file with one name per line), their frames in table order in batches of ``batch_size`` through
    ``OnsetTestStage``, and ``finish()``: the epoch figures, the per-video times and, under ``out_dir``, the merged annotation files.
    ``frames_transforms``: the test chain of the data YAML (``frame_transforms.Compose``; None: the default evaluation chain).
    ``num_workers > 0``: that many threads decode the frames of the next batches (PIL releases the GIL while it decodes; with 0 the stage
    waits for one host thread's JPEG decoding)."""
    device = torch.device(device)
    _lib.require_gpu_tensor(torch.empty(0, device=device), "test_onset_model")
    chunks = chunk_table(root_dir, _read_samples(samples_or_split_file))
    model.to(device)
    stage = OnsetTestStage(model, out_dir, capacity=max(1, len(chunks)))
    if num_workers > 0:
        batches = _prefetched_clips(chunks, batch_size, device, frame_file_suffix, frames_transforms, num_workers)
    else:
        batches = iter_clips(chunks, batch_size, device, frame_file_suffix, frames_transforms)
    for frames, labels, part in batches:
        stage.step(frames, labels, part)
    return stage.finish()


test_onset_model.__test__ = False      # (a library function, not a pytest case, wherever it is imported)


# ---- predicted onsets into a shard ------------------------------------------------------------------------------------------------------
def pack_onset_preds(shard_in: str, pred_dir: str, shard_out: str, skip_empty: bool = False) -> Tuple[List[str], List[str]]:
    """Copy the tar shard ``shard_in`` to ``shard_out`` and add, behind the members of every sample, ``<key>.times.pred.csv`` with the
    bytes of ``pred_dir/<basename(key)>.times.csv`` (the ``pred`` directory ``OnsetTestStage.finish`` writes); the key is WebDataset's
    (``shards._split_key``: the path up to the first dot of the base name).  A ``times.pred.csv`` the sample already carries is replaced.
    Returns ``(missing, empty)``: the keys without a prediction file -- copied as they are; ``slice_chunks`` then falls back to the
    annotated onsets, as the reference's ``_get_slices`` does -- and the keys whose file holds no onset -- packed all the same;
    ``slice_chunks`` asserts on those, as the reference does.  ``skip_empty=True`` leaves both kinds out of ``shard_out``."""
    missing: List[str] = []
    empty: List[str] = []
    with tarfile.open(shard_in, "r:*") as tin, tarfile.open(shard_out, "w") as tout:
        def flush(key: str, members: List[Tuple[tarfile.TarInfo, bytes]]) -> None:
            path = os.path.join(pred_dir, f"{os.path.basename(key)}.times.csv")
            data: Optional[bytes] = None
            if os.path.exists(path):
                with open(path, "rb") as f:
                    data = f.read()
                if not data.strip():
                    empty.append(key)
            else:
                missing.append(key)
            if not members or (skip_empty and (data is None or not data.strip())):
                return
            for info, payload in members:
                tout.addfile(info, io.BytesIO(payload))
            if data is not None:
                info = tarfile.TarInfo(f"{key}.times.pred.csv")
                info.size = len(data)
                info.mtime = members[-1][0].mtime
                tout.addfile(info, io.BytesIO(data))

        cur_key: Optional[str] = None
        group: List[Tuple[tarfile.TarInfo, bytes]] = []
        for m in tin:
            if not m.isfile():
                continue
            key, ext = _split_key(m.name)
            if cur_key is not None and key != cur_key:
                flush(cur_key, group)
                group = []
            cur_key = key
            if ext != "times.pred.csv":
                group.append((m, tin.extractfile(m).read()))
        if cur_key is not None:
            flush(cur_key, group)
    return missing, empty
