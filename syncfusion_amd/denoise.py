"""Complex STFT, inverse STFT and spectral-gating noise reduction on the device (``syncfusion_amd/csrc/stft.hip``).

Replaces ``noisereduce.reduce_noise(x, sr, n_fft=1024, hop_length=1024 // 4)`` of the reference's ``--audio_denoise`` preprocessing step
(script/gh_preprocess_videos.py:91-100), which turns every ``*.resampled.wav`` into ``*.resampled_denoised.wav``.

Pinning status.  The numerical core is PINNED on the host against ``scipy.signal.stft`` / ``istft`` / ``filtfilt`` / ``fftconvolve``
(tests/test_denoise_cpu.py): framing, ``boundary='zeros'``, "spectrum" scaling, the overlap-add with its squared-window envelope, the
zero-phase one-pole smoothing and the 2-D mask filter.  The package glue is UNPINNED: ``noisereduce`` is absent from the reference tree and
from this image, so how it strings those pieces together (defaults, the order of ``prop_decrease`` and smoothing, chunking, the stationary
statistics) is restated from recall.  Every such fact is a field of ``SpectralGateConfig``; whoever pins it against the package later should
change defaults, not code.

The algorithm, per mono row and independent of the batch around it:

* ``S = stft(x)``: periodic Hann of ``win_length`` points, ``win_length // 2`` zeros on each side, hop ``hop_length``, bins divided by
  ``sum(w)``; ``T = L // hop + 1`` frames when ``win_length == n_fft``;
* non-stationary (default): ``A = |S|``; ``sm = filtfilt([b], [1, b - 1], A, axis=time, padtype=None)`` with ``t = time_constant_s * sr / hop``,
  ``b = (sqrt(1 + 4 t^2) - 1) / (2 t^2)`` -- one forward and one backward pass of ``y = b x + (1 - b) y_prev``, each started from its first
  input; ``mask = sigmoid(((A - sm) / sm - thresh_n_mult_nonstationary) * sigmoid_slope_nonstationary)``; smooth; ``mask * prop_decrease +
  (1 - prop_decrease)``.  Deviation: where ``sm == 0`` (a bin silent in every frame) the reference has 0 / 0, the device mask is 0; the output
  bin is 0 either way;
* stationary: ``dB = 20 log10(max(|S|, 1e-20))`` floored at the plane maximum - 80; per bin ``thresh = mean_t + n_std_thresh_stationary *
  std_t`` (ddof 0) over the noise clip (``y_noise``, or the row itself; its first ``chunk_size`` samples with ``clip_noise_stationary``);
  ``mask = dB > thresh``; ``prop_decrease``; smooth;
* smoothing: ``fftconvolve(mask, outer(v_f, v_t) / sum, mode="same")`` with ``v = triangle(n)`` of ``2 n + 1`` points,
  ``n_f = int(freq_mask_smooth_hz / (sr / (n_fft / 2)))`` and ``n_t = int(time_mask_smooth_ms / (hop / sr * 1000))``: separable, zeros outside;
* ``istft(S * mask)`` returns ``(T - 1) * hop`` samples; the tail up to ``L`` stays zero;
* chunking: the clip is cut at multiples of ``chunk_size``; every chunk is filtered with ``padding`` samples on each side (zeros outside the
  clip) and only its own samples are kept.  The padded chunks of all channels are the rows of one device batch.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib

Tensor = torch.Tensor
PAD_MODES = {"constant": 0, "reflect": 1}
SCALINGS = ("spectrum", None)
NOLA_TOL = 1e-10


@dataclass(frozen=True)
class SpectralGateConfig:
    """Every parameter and every recalled fact of the denoiser (module docstring).  Defaults: ``noisereduce.reduce_noise`` as recalled, with
    the reference's ``n_fft=1024, hop_length=256``."""
    n_fft: int = 1024
    hop_length: Optional[int] = None          # None: n_fft // 4
    win_length: Optional[int] = None          # None: n_fft
    stationary: bool = False
    prop_decrease: float = 1.0
    time_constant_s: float = 2.0
    freq_mask_smooth_hz: Optional[float] = 500.0
    time_mask_smooth_ms: Optional[float] = 50.0
    thresh_n_mult_nonstationary: float = 2.0
    sigmoid_slope_nonstationary: float = 10.0
    n_std_thresh_stationary: float = 1.5
    clip_noise_stationary: bool = True
    chunk_size: int = 600000
    padding: int = 30000
    clamp_chunk_to_clip: bool = True          # a clip shorter than chunk_size is one chunk of its own length
    pad_mode: str = "constant"                # scipy's boundary='zeros'
    scaling: Optional[str] = "spectrum"
    prop_before_smoothing_stationary: bool = True
    prop_before_smoothing_nonstationary: bool = False

    @property
    def hop(self) -> int:
        return int(self.hop_length) if self.hop_length is not None else int(self.n_fft) // 4

    @property
    def win(self) -> int:
        return int(self.win_length) if self.win_length is not None else int(self.n_fft)


# ---- host pieces (fp64) -----------------------------------------------------------------------------------------------------------------------
def hann_periodic(win_length: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(win_length), dtype=np.float64) / int(win_length))


def nola_min(win_length: int, hop_length: int) -> float:
    """``min over n < hop of sum_k w[n + k hop]^2`` of the periodic Hann window, fp64."""
    w2 = hann_periodic(win_length) ** 2
    return float(min(w2[n::hop_length].sum() for n in range(int(hop_length))))


def check_stft_arguments(n_fft: int, hop_length: int, win_length: int, L: Optional[int] = None, invert: bool = False) -> None:
    """The refusals of the library, raised on the host as ``ValueError`` before any device call."""
    n_fft, hop_length, win_length = int(n_fft), int(hop_length), int(win_length)
    if n_fft < 256 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError(f"n_fft must be a power of two in [256, 4096], got {n_fft}")
    if win_length < 2 or win_length > n_fft:
        raise ValueError(f"win_length must lie in [2, n_fft = {n_fft}], got {win_length}")
    if hop_length < 1:
        raise ValueError(f"hop_length must be at least 1, got {hop_length}")
    if L is not None and int(L) < win_length:
        raise ValueError(f"a clip of {int(L)} samples is shorter than the window of {win_length}")
    if invert and not nola_min(win_length, hop_length) > NOLA_TOL:
        raise ValueError(f"window {win_length} with hop {hop_length} violates NOLA: the STFT is not invertible")


def smoothing_coefficient(time_constant_s: float, sr: float, hop_length: int) -> float:
    t = float(time_constant_s) * float(sr) / float(hop_length)
    if not t > 0.0:
        raise ValueError("time_constant_s * sr / hop_length must be positive")
    return (math.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)


def triangle(n: int) -> np.ndarray:
    """``concatenate([linspace(0, 1, n + 1, endpoint=False), linspace(1, 0, n + 2)])[1:-1]``: ``2 n + 1`` points, peak 1."""
    return np.concatenate([np.linspace(0.0, 1.0, n + 1, endpoint=False), np.linspace(1.0, 0.0, n + 2)])[1:-1]


def smoothing_taps(sr: float, n_fft: int, hop_length: int, freq_mask_smooth_hz: Optional[float], time_mask_smooth_ms: Optional[float]) -> Tuple[np.ndarray, np.ndarray]:
    """The two factors of the mask filter, each normalised to sum 1 (their outer product is the 2-D filter normalised to sum 1)."""
    n_f = 0 if freq_mask_smooth_hz is None else int(freq_mask_smooth_hz / (float(sr) / (n_fft / 2)))
    n_t = 0 if time_mask_smooth_ms is None else int(time_mask_smooth_ms / (hop_length / float(sr) * 1000.0))
    vf, vt = triangle(max(n_f, 0)), triangle(max(n_t, 0))
    return vf / vf.sum(), vt / vt.sum()


class ChunkRow(NamedTuple):
    start: int      # clip index of the row's first sample (negative: zeros in front of the clip)
    length: int     # samples in the row: chunk_size + 2 padding
    keep: int       # offset of the chunk's own samples inside the row
    count: int      # how many of them lie inside the clip
    dest: int       # clip index they go back to


def chunk_rows(L: int, chunk_size: int, padding: int) -> List[ChunkRow]:
    """The rows a clip of ``L`` samples is cut into: one per multiple of ``chunk_size``, each ``chunk_size + 2 padding`` long."""
    L, chunk_size, padding = int(L), int(chunk_size), int(padding)
    if L < 1 or chunk_size < 1 or padding < 0:
        raise ValueError("L >= 1, chunk_size >= 1 and padding >= 0 expected")
    return [ChunkRow(s - padding, chunk_size + 2 * padding, padding, min(chunk_size, L - s), s) for s in range(0, L, chunk_size)]


def split_rows(y, chunks: List[ChunkRow]):
    """``(C, L)`` array or tensor -> ``(C * len(chunks), row length)``, channel-major, zeros where a row reaches outside the clip."""
    Cn, L = y.shape
    n, R = len(chunks), chunks[0].length
    rows = torch.zeros((Cn * n, R), dtype=y.dtype, device=y.device) if isinstance(y, Tensor) else np.zeros((Cn * n, R), dtype=y.dtype)
    for k, ch in enumerate(chunks):
        lo, hi = max(ch.start, 0), min(ch.start + ch.length, L)
        if hi > lo:
            rows[k::n, lo - ch.start:hi - ch.start] = y[:, lo:hi]
    return rows


def merge_rows(rows, chunks: List[ChunkRow], channels: int, L: int):
    """The inverse of ``split_rows`` on the kept samples: ``(C * len(chunks), row length)`` -> ``(C, L)``."""
    n = len(chunks)
    if rows.shape[0] != channels * n:
        raise ValueError(f"{channels} channels of {n} chunks expected, got {rows.shape[0]} rows")
    out = torch.zeros((channels, L), dtype=rows.dtype, device=rows.device) if isinstance(rows, Tensor) else np.zeros((channels, L), dtype=rows.dtype)
    for k, ch in enumerate(chunks):
        out[:, ch.dest:ch.dest + ch.count] = rows[k::n, ch.keep:ch.keep + ch.count]
    return out


# ---- the library handle ---------------------------------------------------------------------------------------------------------------------
class SpectralGate:
    """One configuration on the device (``sf_spectral_gate_handle``): window, twiddles and the two smoothing filters."""

    def __init__(self, n_fft: int, hop_length: int, win_length: Optional[int] = None, center: bool = True, pad_mode: str = "constant",
                 scaling: Optional[str] = "spectrum", freq_taps: Optional[np.ndarray] = None, time_taps: Optional[np.ndarray] = None):
        win_length = int(n_fft) if win_length is None else int(win_length)
        check_stft_arguments(n_fft, hop_length, win_length)
        if pad_mode not in PAD_MODES:
            raise ValueError(f"pad_mode {pad_mode!r}: one of {sorted(PAD_MODES)}")
        if scaling not in SCALINGS:
            raise ValueError(f"scaling {scaling!r}: 'spectrum' or None")
        self.n_fft, self.hop, self.win, self.center, self.pad_mode, self.scaling = int(n_fft), int(hop_length), win_length, bool(center), pad_mode, scaling
        self.pad = self.win // 2 if self.center else 0
        self.bins = self.n_fft // 2 + 1
        self.freq_taps = np.ascontiguousarray([1.0] if freq_taps is None else freq_taps, dtype=np.float32)
        self.time_taps = np.ascontiguousarray([1.0] if time_taps is None else time_taps, dtype=np.float32)
        h = C.c_void_p()
        _lib.check(_lib.load().sf_spectral_gate_create(self.n_fft, self.win, self.hop, int(self.center), PAD_MODES[pad_mode], int(scaling == "spectrum"),
                                                       self.freq_taps.ctypes.data, int(self.freq_taps.size), self.time_taps.ctypes.data,
                                                       int(self.time_taps.size), C.byref(h)), "sf_spectral_gate_create")
        self.handle = h.value

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                _lib.load().sf_spectral_gate_destroy(h)
            except Exception:      # interpreter shutdown
                pass

    def frames(self, L: int) -> int:
        return (int(L) + 2 * self.pad - self.win) // self.hop + 1

    def samples(self, T: int) -> int:
        return self.win + (int(T) - 1) * self.hop - 2 * self.pad

    def workspace_bytes(self, B: int, L: int) -> int:
        return int(_lib.load().sf_spectral_gate_workspace_bytes(self.handle, int(B), int(L)))

    def _rows(self, wav: Tensor, where: str) -> Tensor:
        _lib.require_gpu_tensor(wav, where)
        if wav.dim() != 2:
            raise ValueError(f"{where}: (rows, samples) expected, got {tuple(wav.shape)}")
        check_stft_arguments(self.n_fft, self.hop, self.win, wav.shape[-1])
        return _lib.f32c(wav)

    def _ws(self, B: int, L: int, device) -> Tensor:
        return torch.empty(self.workspace_bytes(B, L), dtype=torch.uint8, device=device)

    def stft(self, wav: Tensor) -> Tensor:
        """``(B, L)`` -> ``(B, T, F, 2)`` fp32."""
        x = self._rows(wav, "stft")
        B, L = x.shape
        spec = torch.empty((B, self.frames(L), self.bins, 2), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().sf_stft_forward(self.handle, x.data_ptr(), B, L, spec.data_ptr(), _lib.stream_ptr(x.device)), "sf_stft_forward")
        return spec

    def istft(self, spec: Tensor, length: Optional[int] = None) -> Tensor:
        """``(B, T, F, 2)`` fp32 -> ``(B, length)``; ``length=None``: the ``win + (T - 1) hop - 2 pad`` samples the frames give."""
        _lib.require_gpu_tensor(spec, "istft")
        if spec.dim() != 4 or spec.shape[2] != self.bins or spec.shape[3] != 2:
            raise ValueError(f"istft: (rows, frames, {self.bins}, 2) expected, got {tuple(spec.shape)}")
        check_stft_arguments(self.n_fft, self.hop, self.win, invert=True)
        s = _lib.f32c(spec)
        B, T = int(s.shape[0]), int(s.shape[1])
        n = self.samples(T) if length is None else int(length)
        out = torch.empty((B, n), dtype=torch.float32, device=s.device)
        ws = self._ws(B, self.samples(T), s.device)
        with torch.cuda.device(s.device):
            _lib.check(_lib.load().sf_istft_forward(self.handle, s.data_ptr(), B, T, out.data_ptr(), n, ws.data_ptr(), ws.numel(),
                                                    _lib.stream_ptr(s.device)), "sf_istft_forward")
        return out

    def noise_threshold(self, noise: Tensor, n_std: float) -> Tensor:
        """``(B, Ln)`` noise clips -> ``(B, F)`` per-bin dB thresholds of the stationary mask."""
        x = self._rows(noise, "noise_threshold")
        B, L = x.shape
        thresh = torch.empty((B, self.bins), dtype=torch.float32, device=x.device)
        ws = self._ws(B, L, x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().sf_spectral_gate_noise_threshold(self.handle, x.data_ptr(), B, L, float(n_std), thresh.data_ptr(), ws.data_ptr(),
                                                                    ws.numel(), _lib.stream_ptr(x.device)), "sf_spectral_gate_noise_threshold")
        return thresh

    def gate(self, wav: Tensor, smooth_b: float = 1.0, thresh_mult: float = 2.0, slope: float = 10.0, prop_decrease: float = 1.0,
             thresh: Optional[Tensor] = None, prop_before_smoothing: Optional[bool] = None) -> Dict[str, Tensor]:
        """``(B, L)`` rows -> ``{"out": (B, L), "spec": (B, T, F, 2), "mask_raw": (B, T, F), "mask_smooth": (B, T, F)}``; the stationary
        mask when ``thresh`` (``(B, F)`` dB) is given, the non-stationary one otherwise.  ``prop_before_smoothing``: ``mask * prop_decrease +
        (1 - prop_decrease)`` before the smoothing filter instead of behind it (None: before it in the stationary mode only)."""
        x = self._rows(wav, "spectral_gate")
        check_stft_arguments(self.n_fft, self.hop, self.win, invert=True)
        B, L = x.shape
        T, dev = self.frames(L), x.device
        if thresh is not None:
            _lib.require_gpu_tensor(thresh, "spectral_gate")
            if tuple(thresh.shape) != (B, self.bins):
                raise ValueError(f"spectral_gate: thresholds of shape {(B, self.bins)} expected, got {tuple(thresh.shape)}")
            thresh = _lib.f32c(thresh)
        spec = torch.empty((B, T, self.bins, 2), dtype=torch.float32, device=dev)
        m0 = torch.empty((B, T, self.bins), dtype=torch.float32, device=dev)
        m1 = torch.empty_like(m0)
        out = torch.empty((B, L), dtype=torch.float32, device=dev)
        ws = self._ws(B, L, dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sf_spectral_gate(self.handle, x.data_ptr(), B, L, int(thresh is not None), float(smooth_b), float(thresh_mult),
                                                    float(slope), float(prop_decrease),
                                                    int(thresh is not None if prop_before_smoothing is None else prop_before_smoothing),
                                                    None if thresh is None else thresh.data_ptr(),
                                                    spec.data_ptr(), m0.data_ptr(), m1.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    _lib.stream_ptr(dev)), "sf_spectral_gate")
        return {"out": out, "spec": spec, "mask_raw": m0, "mask_smooth": m1}


_plans: Dict[tuple, SpectralGate] = {}


def _plan(device, n_fft: int, hop: int, win: int, center: bool, pad_mode: str, scaling: Optional[str], freq_taps=None, time_taps=None) -> SpectralGate:
    """The cached handle of a configuration on a device (its tables live on the device of its first call)."""
    device = torch.device(device)
    index = device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else -1)
    ft = None if freq_taps is None else np.asarray(freq_taps, dtype=np.float32).tobytes()
    tt = None if time_taps is None else np.asarray(time_taps, dtype=np.float32).tobytes()
    key = (device.type, index, int(n_fft), int(hop), int(win), bool(center), pad_mode, scaling, ft, tt)
    if key not in _plans:
        _plans[key] = SpectralGate(n_fft, hop, win, center, pad_mode, scaling, freq_taps, time_taps)
    return _plans[key]


# ---- public surface -------------------------------------------------------------------------------------------------------------------------
def stft(wav: Tensor, n_fft: int, hop_length: int, win_length: Optional[int] = None, center: bool = True, pad_mode: str = "constant",
         scaling: Optional[str] = "spectrum") -> Tensor:
    """``(..., L)`` device waveform -> complex64 ``(..., F, T)``, ``F = n_fft // 2 + 1`` (a transposed view of the kernel's ``(T, F)`` rows).
    Periodic Hann window of ``win_length`` points, zero-padded at its end to ``n_fft``; ``center`` pads ``win_length // 2`` samples on each
    side (``pad_mode`` ``"constant"`` or ``"reflect"``); ``scaling="spectrum"`` divides by ``sum(w)`` as ``scipy.signal.stft`` does."""
    win = int(n_fft) if win_length is None else int(win_length)
    check_stft_arguments(n_fft, hop_length, win, wav.shape[-1] if wav.dim() else 0)
    lead = tuple(wav.shape[:-1])
    spec = _plan(wav.device, n_fft, hop_length, win, center, pad_mode, scaling).stft(wav.reshape(-1, wav.shape[-1]))
    c = torch.view_as_complex(spec)
    return c.view(lead + tuple(c.shape[1:])).transpose(-1, -2)


def istft(spec: Tensor, n_fft: int, hop_length: int, win_length: Optional[int] = None, center: bool = True, scaling: Optional[str] = "spectrum",
          length: Optional[int] = None) -> Tensor:
    """The inverse of ``stft``: complex ``(..., F, T)`` -> ``(..., length)`` (``win + (T - 1) hop - 2 pad`` samples when ``length`` is None,
    zeros behind them otherwise).  Raises ``ValueError`` when window and hop violate NOLA."""
    win = int(n_fft) if win_length is None else int(win_length)
    check_stft_arguments(n_fft, hop_length, win, invert=True)
    if not spec.is_complex() or spec.dim() < 2 or spec.shape[-2] != int(n_fft) // 2 + 1:
        raise ValueError(f"istft: complex (..., {int(n_fft) // 2 + 1}, T) expected, got {tuple(spec.shape)} {spec.dtype}")
    lead = tuple(spec.shape[:-2])
    s = torch.view_as_real(spec.to(torch.complex64).transpose(-1, -2).contiguous())
    out = _plan(spec.device, n_fft, hop_length, win, center, "constant", scaling).istft(s.reshape((-1,) + tuple(s.shape[-3:])), length)
    return out.view(lead + (out.shape[-1],))


def reduce_noise(y, sr: float, stationary: bool = False, y_noise=None, n_fft: int = 1024, hop_length: Optional[int] = None,
                 win_length: Optional[int] = None, prop_decrease: float = 1.0, time_constant_s: float = 2.0,
                 freq_mask_smooth_hz: Optional[float] = 500.0, time_mask_smooth_ms: Optional[float] = 50.0,
                 thresh_n_mult_nonstationary: float = 2.0, sigmoid_slope_nonstationary: float = 10.0, n_std_thresh_stationary: float = 1.5,
                 clip_noise_stationary: bool = True, chunk_size: int = 600000, padding: int = 30000, device="cuda", return_parts: bool = False,
                 config: Optional[SpectralGateConfig] = None):
    """``noisereduce.reduce_noise`` on the device.  ``y``: numpy array or tensor, ``(L,)`` or ``(C, L)``; the result has the same type and
    shape.  ``config`` replaces the keyword arguments.  With ``return_parts`` also a dict of the rows' ``spec`` ``(R, T, F, 2)``,
    ``mask_raw`` and ``mask_smooth`` ``(R, T, F)``, the ``chunks`` and the per-row outputs ``rows``."""
    cfg = config if config is not None else SpectralGateConfig(
        n_fft=n_fft, hop_length=hop_length, win_length=win_length, stationary=stationary, prop_decrease=prop_decrease, time_constant_s=time_constant_s,
        freq_mask_smooth_hz=freq_mask_smooth_hz, time_mask_smooth_ms=time_mask_smooth_ms, thresh_n_mult_nonstationary=thresh_n_mult_nonstationary,
        sigmoid_slope_nonstationary=sigmoid_slope_nonstationary, n_std_thresh_stationary=n_std_thresh_stationary,
        clip_noise_stationary=clip_noise_stationary, chunk_size=chunk_size, padding=padding)
    is_numpy = not isinstance(y, Tensor)
    yt = torch.as_tensor(np.ascontiguousarray(y)) if is_numpy else y
    if yt.dim() not in (1, 2) or yt.shape[-1] < 1:
        raise ValueError(f"reduce_noise: (L,) or (C, L) expected, got {tuple(yt.shape)}")
    in_dtype, in_device, one_d = yt.dtype, yt.device, yt.dim() == 1
    y2 = yt.reshape(1, -1) if one_d else yt
    Cn, L = int(y2.shape[0]), int(y2.shape[1])
    size = min(int(cfg.chunk_size), L) if cfg.clamp_chunk_to_clip else int(cfg.chunk_size)
    chunks = chunk_rows(L, size, cfg.padding)
    check_stft_arguments(cfg.n_fft, cfg.hop, cfg.win, chunks[0].length, invert=True)
    if not 0.0 <= float(cfg.prop_decrease) <= 1.0:
        raise ValueError("prop_decrease must lie in [0, 1]")
    noise = None
    if cfg.stationary:
        noise = y2 if y_noise is None else torch.as_tensor(np.ascontiguousarray(y_noise)) if not isinstance(y_noise, Tensor) else y_noise
        noise = noise.reshape(1, -1).expand(Cn, -1) if noise.dim() == 1 else noise
        if noise.dim() != 2 or noise.shape[0] != Cn:
            raise ValueError(f"reduce_noise: y_noise of shape (Ln,) or ({Cn}, Ln) expected, got {tuple(noise.shape)}")
        if cfg.clip_noise_stationary:
            noise = noise[:, :int(cfg.chunk_size)]
        check_stft_arguments(cfg.n_fft, cfg.hop, cfg.win, noise.shape[-1])
    dev = yt.device if yt.is_cuda else torch.device(device)
    if dev.type != "cuda":
        raise _lib.SyncFusionAmdError(f"reduce_noise: device {dev} -- this build has no CPU execution path")
    vf, vt = smoothing_taps(sr, cfg.n_fft, cfg.hop, cfg.freq_mask_smooth_hz, cfg.time_mask_smooth_ms)
    plan = _plan(dev, cfg.n_fft, cfg.hop, cfg.win, True, cfg.pad_mode, cfg.scaling, vf, vt)
    rows = split_rows(y2.to(dev, torch.float32), chunks)
    if cfg.stationary:
        th = plan.noise_threshold(noise.to(dev, torch.float32).contiguous(), cfg.n_std_thresh_stationary)
        th = th.repeat_interleave(len(chunks), dim=0)
        parts = plan.gate(rows, prop_decrease=cfg.prop_decrease, thresh=th, prop_before_smoothing=cfg.prop_before_smoothing_stationary)
    else:
        parts = plan.gate(rows, smoothing_coefficient(cfg.time_constant_s, sr, cfg.hop), cfg.thresh_n_mult_nonstationary,
                          cfg.sigmoid_slope_nonstationary, cfg.prop_decrease, prop_before_smoothing=cfg.prop_before_smoothing_nonstationary)
    out = merge_rows(parts["out"], chunks, Cn, L)
    out = out.reshape(-1) if one_d else out
    out = out.to(in_device, in_dtype if in_dtype.is_floating_point else torch.float32)
    res = out.numpy() if is_numpy else out
    if return_parts:
        parts = dict(parts, rows=parts["out"], chunks=chunks)
        del parts["out"]
        return res, parts
    return res
