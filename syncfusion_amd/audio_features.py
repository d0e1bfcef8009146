"""Log-mel spectrogram, spectral-flux onset envelope and onset detection on the device (``syncfusion_amd/csrc/audio_features.hip``).

Replaces ``librosa.onset.onset_detect(y=wav, sr=22050, units='samples', delta=0.3)`` of the reference's evaluation
(script/evaluate_onset.py:30) and the ``torchaudio.transforms.MelSpectrogram`` + ``power_to_db`` pair ``SampleLogger`` draws for every
validation sample (main/module_diffusion.py:120-152).  Neither ``librosa`` nor ``torchaudio`` is needed: the filterbank is built here in
fp64, the window and twiddle tables in the library, and everything per sample runs in three HIP kernels.

Pinning status: UNPINNED.  The arithmetic lives in ``librosa`` (``onset.onset_detect``, ``onset.onset_strength``, ``util.peak_pick``,
``filters.mel``, ``power_to_db``), absent from the reference tree and from this image (pip has no index): restated from the published
algorithm, anchored on the reference's call site (script/evaluate_onset.py:30) and, for the framing, padding and window, on
``torch.stft`` in fp64 (tests/test_audio_features_cpu.py).  Every parameter of the pipeline is therefore an explicit argument; whoever
pins it against librosa later should change defaults, not code.

The pipeline, as restated:

* frames: ``center=True``; frame ``t`` covers samples ``[t*hop - n_fft/2, t*hop + n_fft/2)`` of the clip padded with zeros (``constant``)
  or mirrored without repeating the edge (``reflect``); ``T = 1 + L // hop``; periodic Hann window of ``n_fft`` points;
* ``P = filterbank @ |rfft(frame)|**2``; ``dB = 10*log10(max(amin, P))``, floored at ``max(dB over the clip) - top_db``;
* envelope: ``d[t] = mean_m max(0, dB[m, t] - dB[m, t - lag])`` for ``t >= lag``, preceded by ``lag + n_fft // (2*hop)`` zero frames and cut
  to ``T`` frames;
* peaks: ``x = (e - min e) / (max(e - min e) + FLT_MIN)``; frame ``n`` is an onset when ``x[n]`` is the maximum of
  ``x[max(0, n-pre_max) : min(T, n+post_max)]``, ``x[n] >= mean(x[max(0, n-pre_avg) : min(T, n+post_avg)]) + delta`` and
  ``n - previous onset > wait``; an all-zero envelope has no onsets.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib

Tensor = torch.Tensor
PAD_MODES = {"constant": 0, "reflect": 1}


# ---- mel filterbank (host, fp64) --------------------------------------------------------------------------------------------------------------
_F_SP = 200.0 / 3.0                    # slaney: linear below 1 kHz, 200/3 Hz per mel ...
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP     # ... = 15 mel at 1 kHz
_LOGSTEP = np.log(6.4) / 27.0          # ... and logarithmic above, 27 mels per factor 6.4


def hz_to_mel(f, mel_scale: str = "slaney") -> np.ndarray:
    f = np.asarray(f, dtype=np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    if mel_scale != "slaney":
        raise ValueError(f"mel_scale {mel_scale!r}: 'slaney' or 'htk'")
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m, mel_scale: str = "slaney") -> np.ndarray:
    m = np.asarray(m, dtype=np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    if mel_scale != "slaney":
        raise ValueError(f"mel_scale {mel_scale!r}: 'slaney' or 'htk'")
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (np.maximum(m, _MIN_LOG_MEL) - _MIN_LOG_MEL)), _F_SP * m)


def mel_frequencies(n: int, fmin: float, fmax: float, mel_scale: str = "slaney") -> np.ndarray:
    """``n`` frequencies (Hz) equally spaced on the mel scale from ``fmin`` to ``fmax``."""
    return mel_to_hz(np.linspace(float(hz_to_mel(fmin, mel_scale)), float(hz_to_mel(fmax, mel_scale)), n), mel_scale)


def mel_filterbank(sr: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None, mel_scale: str = "slaney",
                   norm: Optional[str] = "slaney") -> np.ndarray:
    """``(n_mels, n_fft//2 + 1)`` fp64 triangular filters: filter ``m`` rises from ``f[m]`` to 1 at ``f[m+1]`` and falls to 0 at ``f[m+2]``,
    ``f = mel_frequencies(n_mels + 2, fmin, fmax)``, sampled at the DFT bin frequencies; ``norm="slaney"`` scales row ``m`` by
    ``2 / (f[m+2] - f[m])`` (unit area per filter)."""
    if norm not in (None, "slaney"):
        raise ValueError(f"norm {norm!r}: None or 'slaney'")
    if n_mels < 1 or n_fft < 2:
        raise ValueError("n_mels >= 1 and n_fft >= 2 expected")
    fmax = float(sr) / 2.0 if fmax is None else float(fmax)
    bins = np.linspace(0.0, float(sr) / 2.0, n_fft // 2 + 1)
    f = mel_frequencies(n_mels + 2, fmin, fmax, mel_scale)
    fdiff = np.diff(f)
    ramps = f[:, None] - bins[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    fb = np.maximum(0.0, np.minimum(lower, upper))
    if norm == "slaney":
        fb = fb * (2.0 / (f[2:] - f[:-2]))[:, None]
    return fb


def compact_filterbank(fb: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Dense ``(n_mels, bins)`` -> ``(first_bin int32, bin_count int32, packed fp32 weights)``: the contiguous non-zero range of every row.
    A row without a non-zero weight (a filter narrower than the bin spacing) gets count 0, which the library refuses."""
    fb = np.asarray(fb, dtype=np.float64)
    first, count, packed = [], [], []
    for row in fb:
        nz = np.nonzero(row)[0]
        if nz.size == 0:
            first.append(0)
            count.append(0)
            continue
        first.append(int(nz[0]))
        count.append(int(nz[-1] - nz[0] + 1))
        packed.append(row[nz[0]:nz[-1] + 1])
    w = np.concatenate(packed) if packed else np.zeros(0)
    return np.asarray(first, dtype=np.int32), np.asarray(count, dtype=np.int32), np.ascontiguousarray(w, dtype=np.float32)


# ---- the library handle ---------------------------------------------------------------------------------------------------------------------
class FrontEnd:
    """One configuration of the device front end (``sf_audio_features``): window, twiddles and the compact filterbank."""

    def __init__(self, sr: float, n_fft: int, hop_length: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None,
                 mel_scale: str = "slaney", norm: Optional[str] = "slaney", pad_mode: str = "constant"):
        if pad_mode not in PAD_MODES:
            raise ValueError(f"pad_mode {pad_mode!r}: one of {sorted(PAD_MODES)}")
        self.sr, self.n_fft, self.hop, self.n_mels, self.pad_mode = float(sr), int(n_fft), int(hop_length), int(n_mels), pad_mode
        self.filterbank = mel_filterbank(sr, n_fft, n_mels, fmin, fmax, mel_scale, norm) if n_mels >= 1 and n_fft >= 2 else np.zeros((0, 0))
        first, count, w = compact_filterbank(self.filterbank)
        self._first, self._count, self._w = first, count, w
        h = C.c_void_p()
        _lib.check(_lib.load().sf_audio_features_create(self.n_fft, self.hop, self.n_mels, PAD_MODES[pad_mode], first.ctypes.data, count.ctypes.data,
                                                        w.ctypes.data, int(w.size), C.byref(h)), "sf_audio_features_create")
        self.handle = h.value

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                _lib.load().sf_audio_features_destroy(h)
            except Exception:      # interpreter shutdown
                pass

    def frames(self, L: int) -> int:
        return 1 + int(L) // self.hop

    def workspace_bytes(self, B: int, L: int) -> int:
        return int(_lib.load().sf_audio_features_workspace_bytes(self.handle, int(B), int(L)))

    def _rows(self, wav: Tensor, where: str) -> Tuple[Tensor, Tuple[int, ...]]:
        _lib.require_gpu_tensor(wav, where)
        if wav.dim() < 1 or wav.shape[-1] < 1:
            raise ValueError(f"{where}: (..., samples) waveform expected, got {tuple(wav.shape)}")
        x = _lib.f32c(wav)
        return x.view(-1, x.shape[-1]), tuple(x.shape[:-1])

    def _ws(self, B: int, L: int, device) -> Tensor:
        need = self.workspace_bytes(B, L)
        if need < 0:
            raise ValueError(f"audio front end: B = {B}, L = {L} out of range")
        return torch.empty(need, dtype=torch.uint8, device=device)

    def logmel(self, wav: Tensor, to_db: bool = True, amin: float = 1e-10, top_db: float = 80.0) -> Tensor:
        """``(..., L)`` -> ``(..., n_mels, T)``: mel power, or its dB plane with ``to_db``."""
        x, lead = self._rows(wav, "logmel")
        B, L = x.shape
        out = torch.empty((B, self.n_mels, self.frames(L)), dtype=torch.float32, device=x.device)
        ws = self._ws(B, L, x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().sf_logmel_forward(self.handle, x.data_ptr(), B, L, float(amin), float(top_db), None if to_db else out.data_ptr(),
                                                     out.data_ptr() if to_db else None, ws.data_ptr(), ws.numel(), _lib.stream_ptr(x.device)),
                       "sf_logmel_forward")
        return out.view(lead + out.shape[1:])

    def detect(self, wav: Tensor, delta: float, pre_max: int, post_max: int, pre_avg: int, post_avg: int, wait: int, lag: int = 1,
               conf_interval: Optional[int] = None, capacity: Optional[int] = None, amin: float = 1e-10, top_db: float = 80.0) -> "OnsetBatch":
        x, _ = self._rows(wav, "onset_detect")
        B, L = x.shape
        T = self.frames(L)
        cap = T if capacity is None else int(capacity)
        ci = int(0.05 * self.sr) if conf_interval is None else int(conf_interval)
        dev = x.device
        env = torch.empty((B, T), dtype=torch.float32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        pos = torch.empty((B, max(cap, 1)), dtype=torch.int32, device=dev)
        conf = torch.empty((B, max(cap, 1)), dtype=torch.float32, device=dev)
        strength = torch.empty((B, max(cap, 1)), dtype=torch.float32, device=dev)
        ws = self._ws(B, L, dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sf_onset_detect(self.handle, x.data_ptr(), B, L, float(amin), float(top_db), int(lag), int(pre_max), int(post_max),
                                                   int(pre_avg), int(post_avg), int(wait), float(delta), ci, cap, env.data_ptr(), count.data_ptr(),
                                                   pos.data_ptr(), conf.data_ptr(), strength.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   _lib.stream_ptr(dev)), "sf_onset_detect")
        return OnsetBatch(env, count, pos, conf, strength, self.hop, self.sr)


_front_ends: Dict[tuple, FrontEnd] = {}


def front_end(device, sr: float, n_fft: int, hop_length: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None,
              mel_scale: str = "slaney", norm: Optional[str] = "slaney", pad_mode: str = "constant") -> FrontEnd:
    """The cached ``FrontEnd`` of a configuration on a device (its tables live on the device of its first call)."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else -1),
           float(sr), int(n_fft), int(hop_length), int(n_mels), float(fmin), None if fmax is None else float(fmax), mel_scale, norm, pad_mode)
    if key not in _front_ends:
        _front_ends[key] = FrontEnd(sr, n_fft, hop_length, n_mels, fmin, fmax, mel_scale, norm, pad_mode)
    return _front_ends[key]


@dataclass
class OnsetBatch:
    """Device results of one ``sf_onset_detect`` call.  ``count[b]`` onsets of clip ``b`` sit in the first slots of row ``b``."""
    envelope: Tensor      # (B, T) fp32, un-normalised
    count: Tensor         # (B,) int32; -1: more onsets than the capacity
    positions: Tensor     # (B, capacity) int32 samples, ascending, unused -1
    confidence: Tensor    # (B, capacity) fp32
    strength: Tensor      # (B, capacity) fp32, w[o]
    hop: int
    sr: float

    def to_host(self) -> List[Dict[str, np.ndarray]]:
        """One device-to-host copy of the compact results; raises if a clip overflowed the capacity."""
        B, cap = self.positions.shape
        packed = torch.cat([self.count.view(B, 1).to(torch.float64), self.positions.to(torch.float64), self.confidence.to(torch.float64),
                            self.strength.to(torch.float64)], dim=1).cpu().numpy()
        out = []
        for b in range(B):
            n = int(packed[b, 0])
            if n < 0:
                raise _lib.SyncFusionAmdError(f"onset_detect: clip {b} has more than {cap} onsets (capacity overflow)")
            out.append({"onsets": packed[b, 1:1 + n].astype(np.int64), "confidence": packed[b, 1 + cap:1 + cap + n].astype(np.float32),
                        "strength": packed[b, 1 + 2 * cap:1 + 2 * cap + n].astype(np.float32)})
        return out


def peak_pick_defaults(sr: float, hop_length: int) -> Dict[str, int]:
    """The five window arguments as librosa's ``onset_detect`` derives them from ``sr`` and ``hop`` (1, 1, 4, 5, 1 at 22050 / 512)."""
    return {"pre_max": int(0.03 * sr // hop_length), "post_max": int(0.00 * sr // hop_length + 1), "pre_avg": int(0.10 * sr // hop_length),
            "post_avg": int(0.10 * sr // hop_length + 1), "wait": int(0.03 * sr // hop_length)}


# ---- public surface -------------------------------------------------------------------------------------------------------------------------
class MelSpectrogram:
    """``torchaudio.transforms.MelSpectrogram`` (power 2, ``center=True``, Hann window of ``n_fft`` points) with its argument names; with
    ``to_db=True`` followed by ``power_to_db(ref=1, amin=1e-10, top_db=80)``.  ``(..., L)`` device tensor -> ``(..., n_mels, 1 + L // hop)``.
    SampleLogger's instance: ``MelSpectrogram(sample_rate=sr, n_fft=1024, hop_length=512, n_mels=80, center=True, norm="slaney", to_db=True)``."""

    def __init__(self, sample_rate: int = 22050, n_fft: int = 1024, win_length: Optional[int] = None, hop_length: Optional[int] = None,
                 f_min: float = 0.0, f_max: Optional[float] = None, n_mels: int = 80, power: float = 2.0, center: bool = True,
                 pad_mode: str = "reflect", norm: Optional[str] = None, mel_scale: str = "htk", to_db: bool = False, amin: float = 1e-10,
                 top_db: float = 80.0):
        if win_length not in (None, n_fft) or power != 2.0 or not center:
            raise NotImplementedError("MelSpectrogram: win_length == n_fft, power == 2 and center=True only")
        self.sample_rate, self.n_fft, self.hop_length = sample_rate, n_fft, hop_length if hop_length is not None else n_fft // 2
        self.f_min, self.f_max, self.n_mels, self.pad_mode, self.norm, self.mel_scale = f_min, f_max, n_mels, pad_mode, norm, mel_scale
        self.to_db, self.amin, self.top_db = to_db, amin, top_db

    def __call__(self, waveform: Tensor) -> Tensor:
        fe = front_end(waveform.device, self.sample_rate, self.n_fft, self.hop_length, self.n_mels, self.f_min, self.f_max, self.mel_scale,
                       self.norm, self.pad_mode)
        return fe.logmel(waveform, self.to_db, self.amin, self.top_db)


def onset_detect_batch(wav: Tensor, sr: float = 22050, hop_length: int = 512, n_fft: int = 2048, n_mels: int = 128, delta: float = 0.07,
                       pre_max: Optional[int] = None, post_max: Optional[int] = None, pre_avg: Optional[int] = None,
                       post_avg: Optional[int] = None, wait: Optional[int] = None, lag: int = 1, fmin: float = 0.0, fmax: Optional[float] = None,
                       mel_scale: str = "slaney", norm: Optional[str] = "slaney", pad_mode: str = "constant", amin: float = 1e-10,
                       top_db: float = 80.0, conf_interval: Optional[int] = None, capacity: Optional[int] = None) -> OnsetBatch:
    """``(B, L)`` (or ``(L,)``) device waveforms -> ``OnsetBatch`` (device tensors; nothing is read back)."""
    d = peak_pick_defaults(sr, hop_length)
    given = {"pre_max": pre_max, "post_max": post_max, "pre_avg": pre_avg, "post_avg": post_avg, "wait": wait}
    d.update({k: int(v) for k, v in given.items() if v is not None})
    fe = front_end(wav.device, sr, n_fft, hop_length, n_mels, fmin, fmax, mel_scale, norm, pad_mode)
    return fe.detect(wav, delta, lag=lag, conf_interval=conf_interval, capacity=capacity, amin=amin, top_db=top_db, **d)


def onset_strength(wav: Tensor, sr: float = 22050, hop_length: int = 512, n_fft: int = 2048, n_mels: int = 128, lag: int = 1, **kwargs) -> Tensor:
    """The spectral-flux onset envelope, ``(..., L)`` -> ``(..., T)`` (un-normalised).  Keyword arguments as ``onset_detect_batch``."""
    res = onset_detect_batch(wav.reshape(-1, wav.shape[-1]), sr=sr, hop_length=hop_length, n_fft=n_fft, n_mels=n_mels, lag=lag, capacity=1, **kwargs)
    return res.envelope.view(tuple(wav.shape[:-1]) + (res.envelope.shape[-1],))


def onset_detect(wav: Tensor, sr: float = 22050, hop_length: int = 512, n_fft: int = 2048, n_mels: int = 128, delta: float = 0.07,
                 units: str = "samples", **kwargs) -> Union[np.ndarray, List[np.ndarray]]:
    """``librosa.onset.onset_detect`` on the device: the onsets of a ``(L,)`` waveform as a numpy array, or a list of arrays for ``(B, L)``.
    ``units``: ``"samples"`` (``frame * hop``), ``"frames"`` or ``"time"`` (seconds).  Other keyword arguments as ``onset_detect_batch``."""
    if units not in ("samples", "frames", "time"):
        raise ValueError(f"units {units!r}: 'samples', 'frames' or 'time'")
    host = onset_detect_batch(wav, sr=sr, hop_length=hop_length, n_fft=n_fft, n_mels=n_mels, delta=delta, **kwargs).to_host()
    conv = {"samples": lambda o: o, "frames": lambda o: o // hop_length, "time": lambda o: o / float(sr)}[units]
    rows = [conv(r["onsets"]) for r in host]
    return rows[0] if wav.dim() == 1 else rows
