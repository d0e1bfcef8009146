"""Frame-directory side of the onset path: what ``main/dataset_onset.py`` builds for ``VideoOnsetNet`` --
the per-video chunk table (:62-116) and the frames of one chunk (:121-165) -- with the per-pixel work (ToTensor -> antialiased
Resize -> Normalize -> (C, T, H, W)) in the HIP library (``frames_to_clip`` / ``sf_frames_preprocess``).

Layout the reference reads (Greatest Hits as it preprocesses it):
    <root>/<sample>/<sample>.metadata.json      {"processed": {"video_frame_rate": f, "video_duration": d}}
    <root>/<sample>/<sample>.times.csv          ``time,label`` lines (no header)
    <root>/<sample>/frames/*.jpg                one image per frame, naturally sorted
Image decoding is host I/O through PIL by default (as in the reference); everything after the uint8 pixels runs on the device.  With
``frame_decoder("hip")`` the host only reads the files and the JPEG decoding itself is one device call per batch (``syncfusion_amd.jpeg``).
"""
from __future__ import annotations

import contextlib
import glob
import json
import os
import re
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import torch

from .input_pipeline import frame_labels, frames_to_clip

Tensor = torch.Tensor


def natural_sorted(items: Sequence[str]) -> List[str]:
    """natsort's default order for file names: digit runs compare as numbers (1, 2, 10 instead of 1, 10, 2)."""
    def key(s: str):
        return [(0, int(t), "") if t.isdigit() else (1, 0, t) for t in re.split(r"(\d+)", s) if t != ""]

    return sorted(items, key=key)


def chunk_table(root_dir: str, samples: Sequence[str], chunk_length_in_seconds: float = 2.0, annotations_file_suffix: str = ".times.csv",
                metadata_file_suffix: str = ".metadata.json") -> List[dict]:
    """main/dataset_onset.py:62-116: whole chunks of ``chunk_length_in_seconds`` per video with their frame ranges and 0/1 labels."""
    out: List[dict] = []
    for sample in samples:
        with open(os.path.join(root_dir, sample, f"{sample}{metadata_file_suffix}"), "r") as f:
            meta = json.load(f)
        frame_rate = meta["processed"]["video_frame_rate"]
        duration = meta["processed"]["video_duration"]
        num_chunks = int(duration / chunk_length_in_seconds)
        times: List[float] = []
        with open(os.path.join(root_dir, sample, f"{sample}{annotations_file_suffix}"), "r") as f:
            for line in f.read().splitlines():
                if line.strip():
                    times.append(float(line.split(",")[0]))
        for i in range(num_chunks):
            t0 = i * chunk_length_in_seconds
            t1 = t0 + chunk_length_in_seconds
            out.append(dict(video_name=sample, frames_path=os.path.join(root_dir, sample, "frames"), start_time=t0, end_time=t1,
                            start_frame=int(t0 * frame_rate), end_frame=int(t1 * frame_rate), frame_rate=frame_rate,
                            labels=frame_labels(times, t0, chunk_length_in_seconds, frame_rate)))
    return out


def read_frames_u8(paths: Sequence[str], pin: bool = True) -> Tensor:
    """Decode images (PIL, ``convert('RGB')`` as main/dataset_onset.py:155) into one ``(T, H, W, 3)`` uint8 tensor (pinned for the upload)."""
    from PIL import Image
    import numpy as np

    arrs = [np.asarray(Image.open(p).convert("RGB")) for p in paths]
    if not arrs:
        raise ValueError("no frames")
    if any(a.shape != arrs[0].shape for a in arrs):
        raise ValueError("frames of one chunk differ in size")
    t = torch.from_numpy(np.stack(arrs))
    return t.pin_memory() if pin and torch.cuda.is_available() else t


DECODERS = ("pil", "hip")


_decoder = "pil"


def _check_decoder(decoder: str) -> None:
    if decoder not in DECODERS:
        raise ValueError(f"decoder {decoder!r}: one of {DECODERS}")


def current_frame_decoder() -> str:
    return _decoder


def set_frame_decoder(decoder: str) -> str:
    """Which decoder ``chunk_clip`` and ``iter_clips`` (and through it ``onset_test.test_onset_model`` with ``num_workers=0``) use:
    ``"pil"`` (the default: host decoding, as before) or ``"hip"`` (``read_frames_device`` / ``batch_frames_device``).  Returns the
    previous setting.  The entry points keep their arguments; the clips are the same bytes either way.

    The setting is one module-level value: it is NOT thread-local, a ``frame_decoder`` block in one thread changes ``chunk_clip`` in
    every other.  Code that wants the choice per call uses ``read_frames_device`` / ``batch_frames_device`` or ``run_onset_test``,
    which take it as an argument.  ``onset_test.test_onset_model`` with ``num_workers > 0`` decodes on its worker threads through
    ``chunk_frames_u8`` (always Pillow); under ``"hip"`` that function warns, and ``run_onset_test`` is the route whose threads only
    read files."""
    global _decoder
    _check_decoder(decoder)
    previous, _decoder = _decoder, decoder
    return previous


@contextlib.contextmanager
def frame_decoder(decoder: str):
    """``with frame_decoder("hip"): ...``: ``set_frame_decoder`` for the block.  ``iter_clips`` takes the setting when it is called, so
    its batches may be consumed after the block."""
    previous = set_frame_decoder(decoder)
    try:
        yield
    finally:
        set_frame_decoder(previous)


def read_frames_device(paths: Sequence[str], device, decoder: str = "hip") -> Tensor:
    """The frames of ``paths`` as one ``(T, H, W, 3)`` uint8 tensor ON ``device``: ``decoder="hip"`` reads the files and decodes them in
    one device call (``jpeg.decode_jpeg_batch``; files the kernels do not cover go through Pillow); ``"pil"`` is ``read_frames_u8`` and
    the upload.  Both give the same bytes."""
    _check_decoder(decoder)
    if not paths:
        raise ValueError("no frames")
    if decoder == "pil":
        return read_frames_u8(paths).to(device, non_blocking=True)
    from .jpeg import decode_jpeg_batch, read_files

    return decode_jpeg_batch(read_files(paths), device)


def chunk_frame_paths(chunk: dict, frame_file_suffix: str = ".jpg") -> List[str]:
    """The frame files of one chunk in natural order (main/dataset_onset.py:121-134)."""
    return natural_sorted(glob.glob(f"{chunk['frames_path']}/*{frame_file_suffix}"))[chunk["start_frame"]: chunk["end_frame"]]


def chunk_frames_u8(chunk: dict, frame_file_suffix: str = ".jpg", pin: bool = True) -> Tensor:
    """The decoded frames of one chunk, ``(T, H, W, 3)`` uint8 on the host (main/dataset_onset.py:121-134).  Always Pillow: host frames
    are what it returns.  Called while ``set_frame_decoder("hip")`` is in force it says so once (a ``RuntimeWarning``): that is
    ``test_onset_model(num_workers > 0)`` decoding on its worker threads -- ``run_onset_test(decoder="hip")`` keeps them to file reads."""
    if _decoder == "hip":
        import warnings

        warnings.warn('chunk_frames_u8 decodes with Pillow on the host although frame_decoder("hip") is set (test_onset_model with '
                      'num_workers > 0 takes this route); use run_onset_test(..., decoder="hip") for reader threads + device decoding',
                      RuntimeWarning, stacklevel=2)
    return read_frames_u8(chunk_frame_paths(chunk, frame_file_suffix), pin)


def chunk_clip(chunk: dict, device, frame_file_suffix: str = ".jpg", size: Tuple[int, int] = (112, 112), frames_transforms=None,
               generator: Optional[torch.Generator] = None) -> Tensor:
    """Frames of one chunk -> ``(3, T, 112, 112)`` float32 on ``device``: main/dataset_onset.py:121-165 (``__getitem__`` +
    ``read_image_and_apply_transforms``) with the transform chain in one HIP pass.  ``frames_transforms``: a
    ``frame_transforms.Compose`` (the dataset's ``frames_transforms`` argument) instead of the default evaluation chain.
    The frames come from the decoder ``set_frame_decoder`` / ``frame_decoder`` selected; the clip is the same."""
    u8 = read_frames_device(chunk_frame_paths(chunk, frame_file_suffix), device, _decoder)
    if frames_transforms is not None:
        return frames_transforms(u8[None], generator=generator)[0]
    return frames_to_clip(u8[None], size)[0]


def batch_frames_device(paths_per_chunk: Sequence[Sequence[str]], device, blobs: Optional[Sequence[Sequence[bytes]]] = None) -> Tensor:
    """The frames of a batch of chunks, ``(N, T, H, W, 3)`` uint8 on ``device``, decoded by ONE ``decode_jpeg_batch`` call.  ``blobs``:
    the file contents when somebody (a reader thread) has them already."""
    from .jpeg import decode_jpeg_batch, read_files

    if blobs is None:
        blobs = [read_files(p) for p in paths_per_chunk]
    T = len(blobs[0])
    if T == 0:
        raise ValueError("no frames")
    if any(len(b) != T for b in blobs):
        raise ValueError("chunks of one batch differ in frame count or frame size")
    flat = decode_jpeg_batch([x for b in blobs for x in b], device)
    return flat.view(len(blobs), T, *flat.shape[1:])


def clips_from_u8(u8: Tensor, frames_transforms, generator: Optional[torch.Generator]) -> Tensor:
    """``(N, T, H, W, 3)`` uint8 on the device -> the clips of the batch, as ``iter_clips`` makes them from host-decoded frames."""
    if frames_transforms is not None:
        return frames_transforms(u8, generator=generator)
    return frames_to_clip(u8, (112, 112))


def iter_clips(chunks: Sequence[dict], batch_size: int, device, frame_file_suffix: str = ".jpg", frames_transforms=None, shuffle: bool = False,
               drop_last: bool = False, generator: Optional[torch.Generator] = None) -> Iterator[Tuple[Tensor, Tensor, List[dict]]]:
    """Batches ``(frames (N, 3, T, 112, 112), labels (N, T), chunk dicts)`` as the reference's DataLoader stacks them.
    ``shuffle`` / ``drop_last`` are what ``train_dataloader`` sets (main/datamodule_onset.py:104-112); the permutation is drawn from
    ``generator`` before the first batch.  With ``frames_transforms`` the frames of a whole batch are decoded, uploaded once and
    transformed in one launch sequence, the random parameters of its clips drawn from ``generator`` in batch order.
    Under ``frame_decoder("hip")`` the files of a whole batch are read on the host and decoded in ONE device call
    (``batch_frames_device``)."""
    return _iter_clips(chunks, batch_size, device, frame_file_suffix, frames_transforms, shuffle, drop_last, generator, _decoder)


def _iter_clips(chunks, batch_size, device, frame_file_suffix, frames_transforms, shuffle, drop_last, generator, decoder):
    idx = torch.randperm(len(chunks), generator=generator).tolist() if shuffle else list(range(len(chunks)))
    for i in range(0, len(idx), batch_size):
        part = [chunks[j] for j in idx[i: i + batch_size]]
        if drop_last and len(part) < batch_size:
            break
        if decoder == "hip":
            clips = clips_from_u8(batch_frames_device([chunk_frame_paths(c, frame_file_suffix) for c in part], device), frames_transforms, generator)
        elif frames_transforms is None:
            clips = torch.stack([frames_to_clip(read_frames_device(chunk_frame_paths(c, frame_file_suffix), device, "pil")[None], (112, 112))[0]
                                 for c in part])
        else:
            frames = [chunk_frames_u8(c, frame_file_suffix, pin=False) for c in part]
            if any(f.shape != frames[0].shape for f in frames):
                raise ValueError("chunks of one batch differ in frame count or frame size")
            u8 = torch.stack(frames)
            if torch.cuda.is_available():
                u8 = u8.pin_memory()
            clips = frames_transforms(u8.to(device, non_blocking=True), generator=generator)
        yield clips, torch.stack([c["labels"] for c in part]).to(device), part


def prefetched_clips(chunks: Sequence[dict], batch_size: int, device, frame_file_suffix: str = ".jpg", frames_transforms=None,
                     num_workers: int = 4) -> Iterator[Tuple[Tensor, Tensor, List[dict]]]:
    """``iter_clips`` (no shuffle) with the device decoder and ``num_workers`` threads that ONLY READ the files of the next batches
    while the device works on this one; a batch is decoded by one ``decode_jpeg_batch`` call, so the clips are ``iter_clips``'."""
    import collections
    from concurrent.futures import ThreadPoolExecutor

    from .jpeg import read_files

    parts = [list(chunks[i: i + batch_size]) for i in range(0, len(chunks), batch_size)]
    ahead = 1 + -(-num_workers // max(1, batch_size))
    with ThreadPoolExecutor(max_workers=max(1, num_workers)) as pool:
        def submit(part):
            return part, [pool.submit(read_files, chunk_frame_paths(c, frame_file_suffix)) for c in part]

        it = iter(parts)
        pending = collections.deque(submit(p) for _, p in zip(range(ahead), it))
        while pending:
            part, futures = pending.popleft()
            nxt = next(it, None)
            if nxt is not None:
                pending.append(submit(nxt))
            u8 = batch_frames_device(None, device, blobs=[f.result() for f in futures])
            yield clips_from_u8(u8, frames_transforms, None), torch.stack([c["labels"] for c in part]).to(device), part


@torch.no_grad()
def run_onset_test(model, root_dir: str, samples_or_split_file, out_dir: Optional[str], batch_size: int = 16, frames_transforms=None,
                   frame_file_suffix: str = ".jpg", num_workers: int = 0, device="cuda", decoder: str = "pil") -> dict:
    """``onset_test.test_onset_model`` with the decoder as an argument (that function's own arguments are left as they are).
    ``decoder="pil"`` IS ``test_onset_model``.  ``decoder="hip"``: the same chunk table, batches and ``OnsetTestStage``, with the JPEG
    files decoded on the device, one call per batch; with ``num_workers > 0`` that many threads read the files of the next batches and
    do nothing else.  The result is the same dict (and the same files under ``out_dir``)."""
    from . import onset_test

    _check_decoder(decoder)
    if decoder == "pil":
        return onset_test.test_onset_model(model, root_dir, samples_or_split_file, out_dir, batch_size=batch_size, frames_transforms=frames_transforms,
                                           frame_file_suffix=frame_file_suffix, num_workers=num_workers, device=device)
    device = torch.device(device)
    chunks = chunk_table(root_dir, onset_test._read_samples(samples_or_split_file))
    model.to(device)
    stage = onset_test.OnsetTestStage(model, out_dir, capacity=max(1, len(chunks)))
    if num_workers > 0:
        batches = prefetched_clips(chunks, batch_size, device, frame_file_suffix, frames_transforms, num_workers)
    else:
        batches = _iter_clips(chunks, batch_size, device, frame_file_suffix, frames_transforms, False, False, None, "hip")
    for frames, labels, part in batches:
        stage.step(frames, labels, part)
    return stage.finish()
