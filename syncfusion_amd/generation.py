"""Device side of the reference's denoising driver, ``main.generation.generate_dataset``.

Reference loop body (main/generation.py:49-103): ``noise = randn(B,1,length)`` ->
``onsets_encoder(y, with_info=True)`` -> CLAP embedding -> ``model.model.sample(...)`` -> per clip:
zero everything before the first onset (``cut_prefix``), crop to ``cut_length``, resample, save.
``generate_batch`` is that body up to (not including) the CPU resample/save, with the same keyword
names; the DataLoader / WebDataset / torchaudio.save plumbing around it is out of scope (SURVEY.md
section 2 rows 5 and 8f-2).  ``generate_dataset`` takes what the reference passes it -- an UN-batched dataset of
``(x, y, z, text, filename)`` chunks (``exp/evaluate_gh_gen.yaml:21,31-40``: ``create_sfx_dataset(...)`` + ``batch_size``) -- and
batches it itself with ``batch_size`` / ``num_workers`` + ``collate_fn`` as main/generation.py:37-38 does; an iterable of
already-collated batches is passed through.  Output files are 32-bit IEEE-float wav (RIFF format tag 3) written with the
standard library: what ``torchaudio.save`` of a float32 tensor (:104-122) produces -- samples are stored bit-exactly, nothing is
clamped or quantised.
"""
from __future__ import annotations

import math
import struct
from pathlib import Path
from typing import Iterable, List, Optional, Sequence, Union

import torch

from . import _lib
from .input_pipeline import collate_fn
from .onset_glue import cut_prefix_crop
from .resample import resample

Tensor = torch.Tensor


@torch.no_grad()
def generate_batch(model, y: Tensor, z: Optional[Tensor] = None, text: Optional[Sequence[str]] = None, *,
                   num_steps: int = 150, length: int = 2 ** 18, embedding_scale: float = 7.5, cut_prefix: bool = False,
                   cond_text: bool = False, cut_length: Optional[int] = None, noise: Optional[Tensor] = None,
                   generator: Optional[torch.Generator] = None, solver: Optional[str] = None, schedule=None,
                   guidance_rescale: Optional[float] = None, guidance_interval=None) -> Tensor:
    """One batch of main/generation.py:69-89,100 on the device of ``model``.  Returns ``(B, 1, cut_length)``.
    ``solver`` / ``schedule`` (additions): ``VSampler``'s solver name and schedule module for this call; ``None`` keeps the sampler's own.
    ``embedding_scale`` may also be a ``(B,)``, ``(T,)`` or ``(T, B)`` array of scales, and ``guidance_rescale`` / ``guidance_interval``
    are ``VSampler``'s (additions; DESIGN.md, "Guidance schedules"); ``None`` keeps the sampler's own."""
    device = model.device
    _lib.require_gpu_tensor(torch.empty(0, device=device), "generate_batch")
    B = y.shape[0]
    if noise is None:
        noise = torch.randn((B, 1, length), device=device, generator=generator)   # the ONLY RNG on the path (:69)
    y = y.to(device)
    _, y_latent = model.onsets_encoder(y, with_info=True)                        # :71
    if cond_text:
        z_latent = model.clap_encode_text(list(text))                             # :73
    else:
        z_latent = model.clap_encode_audio(z.to(device))                          # :75
    gen = model.model.sample(x_noisy=noise.to(device), num_steps=num_steps, channels=y_latent["xs"][2:-1],
                             embedding=z_latent.to(device), embedding_scale=embedding_scale,
                             **_solver_kwargs(solver, schedule, guidance_rescale, guidance_interval))   # :77-83
    if cut_prefix:
        # one device pass for the batch (:86-89, :100); IndexError on a track without onsets, as the reference's [0] does
        return cut_prefix_crop(gen, y[:, :1], cut_length or length)
    return gen[:, :, : (cut_length or length)]                                     # :91,100


def _solver_kwargs(solver, schedule, guidance_rescale=None, guidance_interval=None) -> dict:
    """Only what the caller chose reaches ``sample()``: with none of them, the call is what it was."""
    kw = {}
    if guidance_rescale is not None:
        kw["guidance_rescale"] = guidance_rescale
    if guidance_interval is not None:
        kw["guidance_interval"] = guidance_interval
    if solver is not None:
        kw["solver"] = solver
    if schedule is not None:
        kw["schedule"] = schedule
    return kw


@torch.no_grad()
def vary_batch(model, audio: Tensor, y: Tensor, z: Optional[Tensor] = None, text: Optional[Sequence[str]] = None, *, strength: float = 0.5,
               num_steps: int = 50, embedding_scale: float = 7.5, cond_text: bool = False, seed: int = 0, solver: str = "ab2",
               guidance_rescale: Optional[float] = None, guidance_interval=None) -> Tensor:
    """Variations of an existing clip ``audio`` ``(B, 1, L)`` under the onset track ``y`` and the CLAP conditioning: the clip is noised to
    the level ``strength`` in (0, 1],

        x_noisy = cos(strength * pi / 2) * audio + sin(strength * pi / 2) * philox_normal(audio.shape, seed, 0),

    and sampled from there on ``LinearSchedule(strength, 0)`` with ``solver``.  Small ``strength`` stays close to the clip, 1 forgets
    it.  The noise is the device's counter-based generator: a pure function of ``seed``.  ``embedding_scale`` (a float or an array of
    scales), ``guidance_rescale`` and ``guidance_interval`` are ``generate_batch``'s."""
    from .diffusion import LinearSchedule, philox_normal

    if not 0.0 < float(strength) <= 1.0:
        raise ValueError(f"strength must lie in (0, 1], got {strength}")
    device = model.device
    _lib.require_gpu_tensor(torch.empty(0, device=device), "vary_batch")
    if audio.dim() != 3:
        raise ValueError(f"audio must be (B, 1, L), got shape {tuple(audio.shape)}")
    angle = float(strength) * math.pi / 2
    x_noisy = math.cos(angle) * audio.to(device).to(torch.float32) + math.sin(angle) * philox_normal(tuple(audio.shape), seed, 0, device)
    _, y_latent = model.onsets_encoder(y.to(device), with_info=True)
    z_latent = _embed(model, z, text, cond_text, device)
    return model.model.sample(x_noisy=x_noisy, num_steps=num_steps, channels=y_latent["xs"][2:-1], embedding=z_latent,
                              embedding_scale=embedding_scale,
                              **_solver_kwargs(solver, LinearSchedule(float(strength), 0.0), guidance_rescale, guidance_interval))


def regions_to_keep_mask(regions, B: int, L: int) -> Tensor:
    """``regions`` -> the bool keep mask ``(B, 1, L)`` (CPU) of ``inpaint_batch``: True = keep the source, False = regenerate.
    ``regions`` is a list of ``(start, end)`` sample ranges (end exclusive) to regenerate in every clip, or a list of ``B`` such lists, one
    per clip.  Ranges may be empty, touch or overlap; each must satisfy ``0 <= start <= end <= L``.  No ranges: everything is kept."""
    regions = list(regions)
    per_clip = len(regions) > 0 and all(isinstance(r, (list, tuple)) and (len(r) == 0 or isinstance(r[0], (list, tuple))) for r in regions)
    if per_clip:
        if len(regions) != B:
            raise ValueError(f"per-clip regions: expected {B} lists, got {len(regions)}")
        clips = [list(r) for r in regions]
    else:
        clips = [regions] * B
    keep = torch.ones((B, 1, L), dtype=torch.bool)
    for b, rs in enumerate(clips):
        for r in rs:
            if not isinstance(r, (list, tuple)) or len(r) != 2:
                raise ValueError(f"a region is a (start, end) pair, got {r!r}")
            start, end = int(r[0]), int(r[1])
            if not 0 <= start <= end <= L:
                raise ValueError(f"region ({start}, {end}) is not inside [0, {L}] with start <= end")
            keep[b, :, start:end] = False
    return keep


def _embed(model, z, text, cond_text: bool, device) -> Tensor:
    if cond_text:
        return model.clap_encode_text(list(text)).to(device)
    return model.clap_encode_audio(z.to(device)).to(device)


def _draw_seed(seed: Optional[int]) -> int:
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)


@torch.no_grad()
def inpaint_batch(model, audio: Tensor, y: Tensor, z: Optional[Tensor] = None, text: Optional[Sequence[str]] = None, *,
                  regions=None, keep_mask: Optional[Tensor] = None, num_steps: int = 150, num_resamples: int = 4,
                  embedding_scale: float = 7.5, cond_text: bool = False, seed: Optional[int] = None, noise: Optional[Tensor] = None,
                  generator: Optional[torch.Generator] = None) -> Tensor:
    """``generate_batch`` with a source: regenerates parts of ``audio`` ``(B, 1, L)`` under the same onset track ``y`` and CLAP
    conditioning and keeps the rest bit for bit.  Exactly one of ``regions`` (``(start, end)`` sample ranges to REGENERATE, for the
    batch or per clip: ``regions_to_keep_mask``) and ``keep_mask`` (bool, True = keep, ``audio``'s shape or broadcastable to it).

    ``num_resamples=4`` is an UNVALIDATED default (no listening test was possible): RePaint (Lugmayr et al., CVPR 2022, section 4.2 and
    table 3) finds that re-noising and denoising again at one level is what makes the regenerated part agree with the kept one, with
    most of the gain in the first few resamples; each costs a full U-Net evaluation, so a call costs ``num_resamples`` x ``sample()``.
    ``seed`` keys the device noise of the kept region (``None``: drawn from torch's CPU generator); ``noise`` / ``generator``: the
    start noise, as in ``generate_batch``."""
    if (regions is None) == (keep_mask is None):
        raise ValueError("exactly one of `regions` and `keep_mask` must be given")
    device = model.device
    _lib.require_gpu_tensor(torch.empty(0, device=device), "inpaint_batch")
    if audio.dim() != 3:
        raise ValueError(f"audio must be (B, 1, L), got shape {tuple(audio.shape)}")
    B, _, L = audio.shape
    if keep_mask is None:
        keep_mask = regions_to_keep_mask(regions, B, L)
    if noise is None:
        noise = torch.randn(tuple(audio.shape), device=device, generator=generator)
    y = y.to(device)
    _, y_latent = model.onsets_encoder(y, with_info=True)
    z_latent = _embed(model, z, text, cond_text, device)
    return model.model.inpaint(audio.to(device), keep_mask.to(device), num_steps, num_resamples, x_noisy=noise.to(device),
                               seed=_draw_seed(seed), channels=y_latent["xs"][2:-1], embedding=z_latent, embedding_scale=embedding_scale)


def long_windows(total: int, length: int, overlap: int) -> List[tuple]:
    """Windows of ``length`` samples that cover ``total`` with at least ``overlap`` samples shared between neighbours (pure host
    function): starts 0, hop, 2 hop, ... with hop = length - overlap while start + length < total, then a last window at
    total - length.  Returns ``[(start, kept_prefix)]``, kept_prefix = end of the previous window - start (0 for the first)."""
    total, length, overlap = int(total), int(length), int(overlap)
    if not 0 < overlap < length <= total:
        raise ValueError(f"need 0 < overlap < length <= total, got overlap={overlap}, length={length}, total={total}")
    hop = length - overlap
    starts, start = [], 0
    while start + length < total:
        starts.append(start)
        start += hop
    starts.append(total - length)
    out, prev_end = [], None
    for st in starts:
        out.append((st, 0 if prev_end is None else prev_end - st))
        prev_end = st + length
    return out


@torch.no_grad()
def generate_long(model, y: Tensor, z: Optional[Tensor] = None, text: Optional[Sequence[str]] = None, *, length: int = 2 ** 18,
                  overlap: int = 2 ** 14, num_steps: int = 150, num_resamples: int = 4, embedding_scale: float = 7.5,
                  cond_text: bool = False, seed: Optional[int] = None, generator: Optional[torch.Generator] = None) -> Tensor:
    """A track longer than one window: ``y`` is ``(B, 1, total)`` and so is the result.  The CLAP embedding is computed once.  Window 0
    (``long_windows``) comes from ``sample()``; window w > 0 from ``inpaint()`` with its first kept_prefix samples held to the previous
    window's tail (mask True there), its own slice of ``y`` through the onset encoder and the noise seed ``seed + w``.  Joins are
    sample-exact: no cross-fade.

    UNVALIDATED defaults (no listening test was possible).  ``overlap=2**14`` (0.34 s at 48 kHz): the kept prefix is what tells the
    new window which sound is ringing, so it should span the decay of a typical Foley hit; it costs 1/16 of every window's new
    samples.  ``num_resamples=4``: see ``inpaint_batch``.  ``seed=None``: drawn from torch's CPU generator."""
    device = model.device
    _lib.require_gpu_tensor(torch.empty(0, device=device), "generate_long")
    if y.dim() != 3:
        raise ValueError(f"y must be (B, channels, total), got shape {tuple(y.shape)}")
    B, total = y.shape[0], y.shape[2]
    windows = long_windows(total, length, overlap)
    seed = _draw_seed(seed)
    y = y.to(device)
    z_latent = _embed(model, z, text, cond_text, device)
    out = torch.empty((B, 1, total), dtype=torch.float32, device=device)
    for w, (start, kept) in enumerate(windows):
        _, y_latent = model.onsets_encoder(y[:, :, start:start + length].contiguous(), with_info=True)
        noise = torch.randn((B, 1, length), device=device, generator=generator)
        cond = dict(channels=y_latent["xs"][2:-1], embedding=z_latent, embedding_scale=embedding_scale)
        if w == 0:
            win = model.model.sample(x_noisy=noise, num_steps=num_steps, **cond)
        else:
            source = torch.zeros((B, 1, length), dtype=torch.float32, device=device)
            source[:, :, :kept] = out[:, :, start:start + kept]
            mask = torch.zeros((B, 1, length), dtype=torch.bool, device=device)
            mask[:, :, :kept] = True
            win = model.model.inpaint(source, mask, num_steps, num_resamples, x_noisy=noise, seed=seed + w, **cond)
        out[:, :, start:start + length] = win
    return out


def save_wav(path: Union[str, Path], audio: Tensor, sample_rate: int) -> None:
    """(channels, n) float tensor -> 32-bit IEEE-float wav, the file ``torchaudio.save(path, float32 tensor, rate)`` writes
    (main/generation.py:104-122): RIFF/WAVE, ``fmt `` with format tag 3 (WAVE_FORMAT_IEEE_FLOAT), the ``fact`` chunk non-PCM
    formats carry, interleaved little-endian float32 frames.  Samples keep their bits: no clamp, no rounding."""
    a = audio.detach().to(torch.float32).cpu()
    if a.dim() != 2:
        raise ValueError(f"save_wav expects (channels, samples), got shape {tuple(a.shape)}")
    ch, n = int(a.shape[0]), int(a.shape[1])
    data = a.t().contiguous().numpy().astype("<f4", copy=False).tobytes()
    rate = int(sample_rate)
    fmt = struct.pack("<HHIIHH", 3, ch, rate, rate * ch * 4, ch * 4, 32)
    body = (b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<II", 4, n) +
            b"data" + struct.pack("<I", len(data)) + data)
    with open(str(path), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def save_wav_pcm16(path: Union[str, Path], audio: Tensor, sample_rate: int) -> None:
    """(channels, n) float tensor -> 16-bit PCM wav (format tag 1), the file ``torchaudio.save(..., bits_per_sample=16)`` writes for a float
    tensor: samples are scaled by 32768, rounded to nearest and clamped to [-32768, 32767].  ``load_wav`` reads it back."""
    a = audio.detach().to(torch.float32).cpu()
    if a.dim() != 2:
        raise ValueError(f"save_wav_pcm16 expects (channels, samples), got shape {tuple(a.shape)}")
    ch = int(a.shape[0])
    data = torch.clamp(torch.round(a.t().contiguous() * 32768.0), -32768.0, 32767.0).to(torch.int16).numpy().astype("<i2", copy=False).tobytes()
    rate = int(sample_rate)
    fmt = struct.pack("<HHIIHH", 1, ch, rate, rate * ch * 2, ch * 2, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with open(str(path), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def load_wav(path: Union[str, Path]):
    """Reader for the files ``save_wav`` writes (and 16-bit PCM wav): -> ((channels, n) float32 tensor, sample_rate).
    The standard library's ``wave`` module rejects format tag 3."""
    raw = Path(path).read_bytes()
    if raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", raw[pos + 8:pos + 24])
        elif cid == b"data":
            data = raw[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f"{path}: missing fmt / data chunk")
    tag, ch, rate, _, _, bits = fmt
    import numpy as np

    if tag == 3 and bits == 32:
        a = torch.from_numpy(np.frombuffer(data, dtype="<f4").astype(np.float32))
    elif tag == 1 and bits == 16:
        a = torch.from_numpy(np.frombuffer(data, dtype="<i2").astype(np.float32) / 32768.0)
    else:
        raise ValueError(f"{path}: unsupported wav encoding (format tag {tag}, {bits} bits)")
    return a.reshape(-1, ch).t().contiguous(), int(rate)


def _is_collated(elem) -> bool:
    """A collated batch carries (B, C, T) waveforms and a sequence of filenames; a dataset element (C, T) and one filename."""
    x = elem[0]
    return isinstance(x, torch.Tensor) and x.dim() == 3 and not isinstance(elem[4], (str, bytes))


def iter_batches(dataset: Iterable, batch_size: int, num_workers: int = 0) -> Iterable:
    """What ``DataLoader(dataset, batch_size=batch_size, num_workers=num_workers, collate_fn=collate_fn)`` yields
    (main/generation.py:37-38).  torch ``Dataset`` / ``IterableDataset`` objects go through that very DataLoader; any other
    iterable of un-collated ``(x, y, z, text, filename)`` chunks is grouped here in order (last batch short, as the
    DataLoader's ``drop_last=False``); an iterable whose elements already are collated batches is passed through."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if isinstance(dataset, (torch.utils.data.Dataset, torch.utils.data.IterableDataset)):
        yield from torch.utils.data.DataLoader(dataset, batch_size=batch_size, num_workers=num_workers, collate_fn=collate_fn)
        return
    it = iter(dataset)
    try:
        first = next(it)
    except StopIteration:
        return
    if _is_collated(first):
        yield first
        yield from it
        return
    buf = [first]
    for elem in it:
        if len(buf) == batch_size:
            yield collate_fn(buf)
            buf = []
        buf.append(elem)
    if buf:
        yield collate_fn(buf)


@torch.no_grad()
def generate_dataset(experiment_path: Union[str, Path], model, dataset: Iterable, device: str = "cuda",
                     model_path: Optional[str] = None, batch_size: int = 16, num_workers: int = 4, sample_rate: int = 48000,
                     num_steps: int = 150, length: int = 2 ** 18, embedding_scale: float = 7.5, cut_prefix: bool = False,
                     cond_text: bool = False, one_chunk_per_track: bool = False, cut_length: Optional[int] = None,
                     downsample_rate: Optional[int] = None, save_cond: bool = False, solver: Optional[str] = None,
                     schedule=None, guidance_rescale: Optional[float] = None, guidance_interval=None) -> List[Path]:
    """Same signature as main/generation.py:12-30.  ``dataset``: the reference's un-batched chunk dataset (batched here with
    ``batch_size`` / ``num_workers`` + ``collate_fn``, :37-38) or an iterable of already-collated batches (``iter_batches``)."""
    experiment_path = Path(experiment_path)
    experiment_path.mkdir(exist_ok=True, parents=True)
    if model_path:                                                                  # :40-44
        checkpoint = torch.load(model_path, map_location=device)
        model.load_state_dict(checkpoint["state_dict"])     # upstream or local key layout (syncfusion_amd/keymap.py)
    model.to(device)
    written: List[Path] = []
    chunk_id = 0
    for batch in iter_batches(dataset, batch_size, num_workers):
        x, y, z, text, filenames = batch
        B = x.shape[0]
        if not one_chunk_per_track:
            last = experiment_path / f"{chunk_id + B - 1}.wav"
            if last.exists():                                                       # crude resume, :52-59
                chunk_id += B
                continue
        gen = generate_batch(model, y, z, text, num_steps=num_steps, length=length, embedding_scale=embedding_scale,
                             cut_prefix=cut_prefix, cond_text=cond_text, cut_length=cut_length, solver=solver, schedule=schedule,
                             guidance_rescale=guidance_rescale, guidance_interval=guidance_interval)
        out_sr = sample_rate
        cond = z.to(gen.device).to(torch.float32) if (save_cond and not cond_text) else None   # :93-96: the conditioning audio itself
        if downsample_rate:                                                       # :90-98, on the device instead of the CPU
            gen = resample(gen, orig_freq=sample_rate, new_freq=downsample_rate)
            if cond is not None:
                cond = resample(cond, orig_freq=sample_rate, new_freq=downsample_rate)
            out_sr = downsample_rate
        for i in range(B):
            stem = f"{chunk_id}" if not one_chunk_per_track else str(filenames[i]).split('/')[-1]
            # file set of :104-122: `{stem}.wav`; with save_cond `{stem}_{text}.wav` (text conditioning, replaces the plain name)
            # or `{stem}.wav` + `{stem}_cond.wav` (audio conditioning)
            name = f"{stem}_{text[i]}.wav" if (save_cond and cond_text) else f"{stem}.wav"
            save_wav(experiment_path / name, gen[i], out_sr)
            written.append(experiment_path / name)
            if cond is not None:
                save_wav(experiment_path / f"{stem}_cond.wav", cond[i], out_sr)
                written.append(experiment_path / f"{stem}_cond.wav")
            chunk_id += 1
    return written


@torch.no_grad()
def prepare_gt_for_fad(experiment_path: Union[str, Path], dataset: Iterable, batch_size: int = 16, num_workers: int = 4,
                       sample_rate: int = 48000, one_chunk_per_track: bool = False, downsample_rate: Optional[int] = None) -> List[Path]:
    """Same signature as main/dataset_diffusion.py:146-197: the ground-truth directory ``evaluate_fad`` takes as ``gt_path``.  The waveform
    chunks of ``dataset`` (batched as ``generate_dataset`` batches them, ``iter_batches``) are written under the names ``generate_dataset``
    gives the generated ones: ``{chunk_id}.wav`` with the same crude resume (a batch whose LAST file exists is skipped and counted), or,
    with ``one_chunk_per_track``, ``{basename(filename)}.wav`` -- there the reference's "Skipping" only prints and the batch is written
    again; so it is here.  ``downsample_rate``: the chunks go through this package's ``resample`` on the device (the reference resamples
    clip by clip with torchaudio on the CPU) and the files carry that rate.  Files are written by ``save_wav``."""
    experiment_path = Path(experiment_path)
    experiment_path.mkdir(exist_ok=True, parents=True)
    written: List[Path] = []
    chunk_id = 0
    for batch in iter_batches(dataset, batch_size, num_workers):
        waveforms, _, _, _, filenames = batch
        B = waveforms.shape[0]
        if not one_chunk_per_track:
            last = experiment_path / f"{chunk_id + B - 1}.wav"
            if last.exists():                                                       # :166-173
                print(f"Skipping path: {last}")
                chunk_id += B
                continue
            print(f"{chunk_id=}")
        else:
            last = experiment_path / f"{str(filenames[-1]).split('/')[-1]}.wav"
            if last.exists():                                                       # :175-179: prints, and goes on to write
                print(f"Skipping path: {last}")
            print(f"{filenames[0] = }")
        out_sr = sample_rate
        if downsample_rate:                                                         # :186-189, one device call for the batch
            if not waveforms.is_cuda:
                waveforms = waveforms.to("cuda")                                    # the resampler is a HIP kernel: no CPU path
            waveforms = resample(waveforms, orig_freq=sample_rate, new_freq=downsample_rate)
            out_sr = downsample_rate
        for i in range(B):
            if not one_chunk_per_track:
                path = experiment_path / f"{chunk_id}.wav"
                chunk_id += 1
            else:
                path = experiment_path / f"{str(filenames[i]).split('/')[-1]}.wav"
            save_wav(path, waveforms[i], out_sr)
            written.append(path)
    return written
