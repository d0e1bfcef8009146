"""Fréchet Audio Distance on the device: VGGish input features, the VGGish network, embedding statistics and the Fréchet distance.

Replaces ``main.evaluation.evaluate_fad`` (main/evaluation.py:7-28), the ``config.evaluation`` target of script/evaluate_diffusion.py:31-36:
``FrechetAudioDistance(model_name="vggish", use_pca=False, use_activation=False).score(gt_path, experiment_path)``.  Neither
``frechet_audio_distance`` nor ``torch.hub``, ``resampy``, ``soundfile``, ``scipy`` or ``pandas`` is needed.  The front end runs in
``csrc/audio_features.hip`` (the same FFT as the onset front end), the convolutions and Linear layers on the library's fp32
implicit-GEMM launcher, the max-pool and the fp64 moments in ``csrc/fad.hip``; the distance of two 128-dimensional Gaussians is host
arithmetic in fp64.  The weights come from a file the user supplies; nothing is ever fetched.

Pinning status: UNPINNED.  The arithmetic lives in packages that are absent from the reference tree and from this image
(``frechet_audio_distance``, ``torchvggish``): restated from the published code as recalled, every recalled value a field of
``VGGishConfig``, and pinned where possible against fp64 numpy / torch (tests/fad_ref.py).  Whoever pins it against upstream later
should change defaults, not code.  The recalled facts:

* input (``vggish_input.py`` / ``mel_features.py``): 16 kHz; window ``round(0.025 sr) = 400`` samples, hop ``round(0.010 sr) = 160``, FFT
  length the next power of two (512), the windowed frame zero-padded at its end; NO centring and no padding of the clip -- frame ``t``
  covers ``[160 t, 160 t + 400)``, ``F = 1 + (L - 400) // 160`` frames; periodic Hann ``0.5 - 0.5 cos(2 pi n / 400)``; magnitude ``|X_k|``
  (not power);
* mel matrix: 64 bands, 125 .. 7500 Hz, ``mel = 1127 ln(1 + f / 700)``, 66 edges equally spaced in mel, triangles linear IN MEL
  (``mel_filterbank`` of audio_features.py draws them in Hz), no area normalisation, the DC bin zeroed;
* ``log(mel + 0.01)``; examples of 96 frames with hop 96, the remainder dropped (15600 samples is the shortest clip with one example);
* network (``torchvggish``): ``64, M, 128, M, 256, 256, M, 512, 512, M`` (3x3 convolutions, pad 1, + ReLU; M = 2x2 max-pool), the
  ``(N, 6, 4, 512)`` map flattened in (h, w, c) order, ``Linear(12288, 4096) + ReLU, Linear(4096, 4096) + ReLU, Linear(4096, 128)`` and a
  final ReLU that ``use_activation=False`` drops; ``use_pca=False`` applies no post-processor (``pproc.*`` keys of a checkpoint are ignored);
* statistics: ``mu = mean``, ``sigma = np.cov(rowvar=False)``; ``FAD = |mu1 - mu2|^2 + tr s1 + tr s2 - 2 tr sqrtm(s1 s2)``.

Where this differs from upstream by construction: files at another rate go through ``syncfusion_amd.resample`` -- this package's
windowed-sinc resampler, NOT resampy -- so such files can differ from upstream by the resamplers' difference; a side with fewer than
two examples raises ``ValueError`` (upstream returns -1); singular covariances need no ``eps`` offset (see ``frechet_distance``).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import _lib
from .audio_features import compact_filterbank
from .generation import load_wav
from .resample import resample

Tensor = torch.Tensor
WEIGHTS_ENV = "SYNCFUSION_VGGISH_WEIGHTS"
IN_LD = 4                              # columns of an example row (one channel + 3 zeros): what the convolution launcher reads


@dataclass
class VGGishConfig:
    """Every recalled value of the VGGish pipeline (module docstring).  ``layout``: channel counts of the 3x3 convolutions, ``"M"`` a 2x2
    max-pool; ``fc``: widths of the Linear stack, the last one the embedding size (at most 128 for the statistics kernel)."""
    sample_rate: int = 16000
    window_seconds: float = 0.025
    hop_seconds: float = 0.010
    n_mels: int = 64
    mel_min_hz: float = 125.0
    mel_max_hz: float = 7500.0
    mel_break_hz: float = 700.0
    mel_q: float = 1127.0
    log_offset: float = 0.01
    example_frames: int = 96
    layout: Tuple[Union[int, str], ...] = (64, "M", 128, "M", 256, 256, "M", 512, 512, "M")
    fc: Tuple[int, ...] = (4096, 4096, 128)
    final_relu: bool = False           # FrechetAudioDistance(use_activation=False) drops VGGish's last ReLU

    @property
    def window_length(self) -> int:
        return int(round(self.window_seconds * self.sample_rate))

    @property
    def hop_length(self) -> int:
        return int(round(self.hop_seconds * self.sample_rate))

    @property
    def n_fft(self) -> int:
        return 1 << max(0, (self.window_length - 1).bit_length())

    def frames(self, L: int) -> int:
        return 0 if L < self.window_length else 1 + (int(L) - self.window_length) // self.hop_length

    def examples(self, L: int) -> int:
        return self.frames(L) // self.example_frames

    def final_map(self) -> Tuple[int, int, int]:
        """(H, W, C) of the map the first Linear layer reads."""
        h, w, c = self.example_frames, self.n_mels, 1
        for v in self.layout:
            if v == "M":
                h, w = h // 2, w // 2
            else:
                c = int(v)
        return h, w, c


def vggish_mel_matrix(cfg: VGGishConfig = VGGishConfig()) -> np.ndarray:
    """``(n_fft // 2 + 1, n_mels)`` fp64: band ``i`` rises from mel edge ``i`` to 1 at edge ``i + 1`` and falls to 0 at edge ``i + 2``, linearly
    in mel, sampled at the mels of the DFT bins; the DC row is zero."""
    bins = cfg.n_fft // 2 + 1
    to_mel = lambda f: cfg.mel_q * np.log(1.0 + np.asarray(f, dtype=np.float64) / cfg.mel_break_hz)
    m = to_mel(np.linspace(0.0, cfg.sample_rate / 2.0, bins))
    edges = np.linspace(float(to_mel(cfg.mel_min_hz)), float(to_mel(cfg.mel_max_hz)), cfg.n_mels + 2)
    lo, c, up = edges[:-2], edges[1:-1], edges[2:]
    lower = (m[:, None] - lo[None, :]) / (c - lo)[None, :]
    upper = (up[None, :] - m[:, None]) / (up - c)[None, :]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w[0, :] = 0.0
    return w


# ---- host arithmetic ------------------------------------------------------------------------------------------------------------------------
def _psd_factor(s: np.ndarray) -> np.ndarray:
    """``R`` with ``R R^T = s`` for a symmetric positive semi-definite ``s``: eigenvectors times the square roots of the eigenvalues,
    keeping those above ``D eps lambda_max`` (the numerical rank; smaller and negative ones are rounding of zeros)."""
    lam, q = np.linalg.eigh(s)
    keep = lam > max(float(lam[-1]), 0.0) * lam.size * np.finfo(np.float64).eps
    return q[:, keep] * np.sqrt(lam[keep])[None, :]


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """``|mu1 - mu2|^2 + tr s1 + tr s2 - 2 sum_i sqrt(lambda_i)`` with ``lambda`` the eigenvalues of ``s1^(1/2) s2 s1^(1/2)``, fp64, numpy only.

    That matrix is symmetric positive semi-definite and similar to ``s1 s2``, so the sum equals ``tr sqrtm(s1 s2)`` of the upstream
    package; it takes two ``eigh`` calls and no scipy.  Eigenvalues below the numerical rank threshold ``D eps lambda_max`` (negative
    ones included) are rounding of zeros and are clipped to 0 in both calls: the square root would turn a 1e-16 residue into 1e-8.
    Unlike ``sqrtm`` of the unsymmetric product the result stays real, finite and accurate for singular covariances -- fewer samples
    than dimensions -- where upstream falls back to adding ``eps`` to both diagonals."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64).reshape(-1), np.asarray(mu2, dtype=np.float64).reshape(-1)
    s1, s2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    if mu1.shape != mu2.shape or s1.shape != s2.shape or s1.shape != (mu1.size, mu1.size):
        raise ValueError(f"frechet_distance: shapes {mu1.shape}, {s1.shape}, {mu2.shape}, {s2.shape} do not match")
    s1, s2 = 0.5 * (s1 + s1.T), 0.5 * (s2 + s2.T)
    r1 = _psd_factor(s1)                                   # (D, rank s1); the non-zero eigenvalues of r1^T s2 r1 are those of s1^(1/2) s2 s1^(1/2)
    cross = 0.0
    if r1.shape[1]:
        mid = r1.T @ s2 @ r1
        ev = np.linalg.eigvalsh(0.5 * (mid + mid.T))
        ev = ev[ev > max(float(ev[-1]), 0.0) * mu1.size * np.finfo(np.float64).eps]
        cross = float(np.sum(np.sqrt(ev)))
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * cross)


@dataclass
class Moments:
    """fp64 sufficient statistics of a set of embeddings: count, column sums and the scatter matrix about the set's own mean."""
    n: int
    sum: np.ndarray
    scatter: np.ndarray

    def merge(self, other: "Moments") -> "Moments":
        """The statistics of the union (pairwise update, fp64 on the host): sets are processed in batches."""
        if self.n == 0:
            return other
        if other.n == 0:
            return self
        n = self.n + other.n
        d = other.sum / other.n - self.sum / self.n
        return Moments(n, self.sum + other.sum, self.scatter + other.scatter + np.outer(d, d) * (self.n * other.n / n))

    def statistics(self) -> Tuple[np.ndarray, np.ndarray, int]:
        """``(mu, sigma, n)`` with ``sigma = np.cov(rowvar=False)``; needs two rows."""
        if self.n < 2:
            raise ValueError(f"the covariance needs at least 2 embeddings, got {self.n}")
        return self.sum / self.n, self.scatter / (self.n - 1), self.n


def embedding_moments(emb: Tensor) -> Moments:
    """``(N, D)`` device embeddings, ``D <= 128`` -> ``Moments`` (``sf_op_moments``: fp64, fixed order, bit-reproducible)."""
    _lib.require_gpu_tensor(emb, "embedding_moments")
    if emb.dim() != 2:
        raise ValueError(f"embedding_moments: (N, D) expected, got {tuple(emb.shape)}")
    x = _lib.f32c(emb)
    N, D = x.shape
    if N == 0:
        return Moments(0, np.zeros(D), np.zeros((D, D)))
    out = torch.empty(D + D * D, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().sf_op_moments(x.data_ptr(), N, D, out.data_ptr(), out.data_ptr() + 8 * D, _lib.stream_ptr(x.device)), "sf_op_moments")
    host = out.cpu().numpy()
    return Moments(int(N), host[:D].copy(), host[D:].reshape(D, D).copy())


def embedding_statistics(emb: Tensor) -> Tuple[np.ndarray, np.ndarray, int]:
    """``(N, D)`` device embeddings -> ``(mu, sigma, n)`` in fp64: the mean and ``np.cov(emb, rowvar=False)``."""
    return embedding_moments(emb).statistics()


# ---- the network ----------------------------------------------------------------------------------------------------------------------------
def _stage_codes(cfg: VGGishConfig) -> List[int]:
    return [0 if v == "M" else int(v) for v in cfg.layout]


class VGGish(nn.Module):
    """VGGish with torchvggish's parameter names (``features.{0,3,6,8,11,13}``, ``embeddings.{0,2,4}`` for the default layout), so an
    upstream ``.pth`` state dict loads; ``pproc.*`` keys are ignored, any other missing or unexpected key is an error.  Inference only."""

    def __init__(self, config: VGGishConfig = VGGishConfig()):
        super().__init__()
        self.config = config
        if not config.layout or config.layout[0] == "M" or not config.fc:
            raise ValueError("VGGishConfig: the layout starts with a convolution and fc is not empty")
        feats: List[nn.Module] = []
        c = 1
        for v in config.layout:            # the index arithmetic of torchvggish's make_layers: Conv2d, ReLU | MaxPool2d
            if v == "M":
                feats.append(nn.MaxPool2d(2, 2))
            else:
                feats += [nn.Conv2d(c, int(v), 3, padding=1), nn.ReLU(inplace=True)]
                c = int(v)
        self.features = nn.Sequential(*feats)
        h, w, c = config.final_map()
        if h < 1 or w < 1:
            raise ValueError(f"VGGishConfig: the layout pools a {config.example_frames} x {config.n_mels} example away")
        emb: List[nn.Module] = []
        k = h * w * c
        for i, n in enumerate(config.fc):
            emb.append(nn.Linear(k, int(n)))
            if i + 1 < len(config.fc):
                emb.append(nn.ReLU(inplace=True))
            k = int(n)
        self.embeddings = nn.Sequential(*emb)
        self.mel_matrix = vggish_mel_matrix(config)
        self._front = None
        self._engine = None
        self._engine_key = None

    # -- state dict: upstream names, pproc.* ignored, strict otherwise
    def load_state_dict(self, state_dict, strict: bool = True, **kwargs):
        state = {k: v for k, v in state_dict.items() if not k.startswith("pproc.")}
        self._drop_engine()
        return super().load_state_dict(state, strict=True, **kwargs)

    def _drop_engine(self):
        h = self.__dict__.get("_engine")
        self.__dict__["_engine"] = None      # (not nn.Module.__setattr__: this also runs at interpreter shutdown)
        if h:
            try:
                _lib.load().sf_vggish_destroy(h)
            except Exception:          # interpreter shutdown
                pass

    def __del__(self):
        self._drop_engine()
        f = self.__dict__.get("_front")
        self.__dict__["_front"] = None
        if f:
            try:
                _lib.load().sf_audio_features_destroy(f)
            except Exception:
                pass

    # -- front end
    def _front_end(self) -> int:
        if self._front is None:
            cfg = self.config
            first, count, w = compact_filterbank(self.mel_matrix.T)
            h = C.c_void_p()
            _lib.check(_lib.load().sf_audio_features_create_framed(cfg.n_fft, cfg.window_length, cfg.hop_length, cfg.n_mels, first.ctypes.data,
                                                                   count.ctypes.data, w.ctypes.data, int(w.size), C.byref(h)),
                       "sf_audio_features_create_framed")
            self._front = h.value
        return self._front

    def _front_call(self, wav: Tensor, want_mel: bool) -> Tuple[Tensor, Optional[Tensor]]:
        _lib.require_gpu_tensor(wav, "VGGish.examples")
        if wav.dim() == 1:
            wav = wav[None]
        if wav.dim() != 2:
            raise ValueError(f"VGGish: (B, L) waveforms expected, got {tuple(wav.shape)}")
        cfg = self.config
        x = _lib.f32c(wav)
        B, L = x.shape
        E, T = cfg.examples(L), cfg.examples(L) * cfg.example_frames
        rows = torch.empty((B * T * cfg.n_mels, IN_LD), dtype=torch.float32, device=x.device)
        mel = torch.empty((B, T, cfg.n_mels), dtype=torch.float32, device=x.device) if want_mel else None
        if B > 0 and E > 0:            # a clip shorter than one example yields nothing, without a launch
            with torch.cuda.device(x.device):
                _lib.check(_lib.load().sf_logmel_examples_forward(self._front_end(), x.data_ptr(), B, L, cfg.example_frames, float(cfg.log_offset),
                                                                  rows.data_ptr(), mel.data_ptr() if want_mel else None,
                                                                  _lib.stream_ptr(x.device)), "sf_logmel_examples_forward")
        return rows, mel

    def example_rows(self, wav: Tensor) -> Tensor:
        """``(B, L)`` device waveforms at the model's rate -> the examples as the network reads them: ``(B E 96 64, 4)`` channels-last rows,
        column 0 the log-mel value and columns 1 .. 3 zero."""
        return self._front_call(wav, False)[0]

    def examples(self, wav: Tensor) -> Tensor:
        """``(B, L)`` device waveforms at the model's rate -> ``(B, E, 96, 64)`` log-mel examples (``E = 0`` for a clip below one example)."""
        cfg = self.config
        rows = self.example_rows(wav)
        B = 1 if wav.dim() == 1 else wav.shape[0]
        return rows[:, 0].reshape(B, -1, cfg.example_frames, cfg.n_mels)

    def mel_magnitude(self, wav: Tensor) -> Tensor:
        """``(B, L)`` -> ``(B, E 96, 64)``: the mel magnitudes of the frames that enter the examples (before the logarithm)."""
        return self._front_call(wav, True)[1]

    # -- network
    def _engine_for(self, device: torch.device) -> int:
        params = [p for p in self.parameters()]
        key = (str(device), tuple((p.data_ptr(), p._version) for p in params))
        if self._engine is None or self._engine_key != key:
            self._drop_engine()
            cfg = self.config
            convs = [m for m in self.features if isinstance(m, nn.Conv2d)]
            fcs = [m for m in self.embeddings if isinstance(m, nn.Linear)]
            keep = [[_lib.f32c(m.weight).to(device) for m in convs], [_lib.f32c(m.bias).to(device) for m in convs],
                    [_lib.f32c(m.weight).to(device) for m in fcs], [_lib.f32c(m.bias).to(device) for m in fcs]]
            stages = np.asarray(_stage_codes(cfg), dtype=np.int32)
            widths = np.asarray(cfg.fc, dtype=np.int32)
            h = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(_lib.load().sf_vggish_create(int(stages.size), stages.ctypes.data, int(widths.size), widths.ctypes.data, cfg.example_frames,
                                                        cfg.n_mels, 1 if cfg.final_relu else 0, _lib.ptr_array(keep[0]), _lib.ptr_array(keep[1]),
                                                        _lib.ptr_array(keep[2]), _lib.ptr_array(keep[3]), _lib.stream_ptr(device), C.byref(h)),
                           "sf_vggish_create")
            self._engine, self._engine_key = h.value, key
        return self._engine

    def embed_rows(self, rows: Tensor, pool_taps: bool = False, chunk: int = 64):
        """Example rows ``(N 96 64, 4)`` (``example_rows``) -> ``(N, D)`` embeddings; with ``pool_taps`` also the list of the max-pools' outputs,
        each ``(N, h, w, channels)`` (tests)."""
        _lib.require_gpu_tensor(rows, "VGGish.embed_rows")
        cfg = self.config
        per = cfg.example_frames * cfg.n_mels
        if rows.dim() != 2 or rows.shape[1] != IN_LD or rows.shape[0] % per:
            raise ValueError(f"VGGish.embed_rows: (N * {per}, {IN_LD}) rows expected, got {tuple(rows.shape)}")
        x = _lib.f32c(rows)
        dev = x.device
        N, D = x.shape[0] // per, int(cfg.fc[-1])
        out = torch.empty((N, D), dtype=torch.float32, device=dev)
        taps: List[Tensor] = []
        shapes = []
        if pool_taps:
            h, w, c = cfg.example_frames, cfg.n_mels, 1
            for v in cfg.layout:
                if v == "M":
                    h, w = h // 2, w // 2
                    shapes.append((h, w, c, (c + 7) // 8 * 8))
                    taps.append(torch.empty((N, h, w, shapes[-1][3]), dtype=torch.float32, device=dev))
                else:
                    c = int(v)
        if N == 0:
            return (out, [t[..., :s[2]] for t, s in zip(taps, shapes)]) if pool_taps else out
        lib = _lib.load()
        eng = self._engine_for(dev)
        chunk = max(1, min(int(chunk), int(lib.sf_vggish_max_examples(eng))))
        ws = torch.empty(int(lib.sf_vggish_workspace_bytes(eng, min(chunk, N))), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            for i in range(0, N, chunk):
                n = min(chunk, N - i)
                tp = _lib.ptr_array([t[i:i + n] for t in taps]) if pool_taps else None
                _lib.check(lib.sf_vggish_forward(eng, x.data_ptr() + i * per * IN_LD * 4, n, out.data_ptr() + i * D * 4, tp, ws.data_ptr(), ws.numel(),
                                                 _lib.stream_ptr(dev)), "sf_vggish_forward")
        return (out, [t[..., :s[2]] for t, s in zip(taps, shapes)]) if pool_taps else out

    def forward(self, wav: Tensor, sr: Optional[int] = None) -> Tensor:
        """``(B, L)`` device waveforms -> ``(B E, D)`` embeddings, clip-major.  ``sr``: the waveforms' rate when it is not the model's; they go
        through ``syncfusion_amd.resample`` first."""
        if sr is not None and int(sr) != self.config.sample_rate:
            wav = resample(wav, int(sr), self.config.sample_rate)
        with torch.no_grad():
            return self.embed_rows(self.example_rows(wav))


# ---- directory level ------------------------------------------------------------------------------------------------------------------------
def load_vggish(weights: Optional[Union[str, Path]] = None, config: VGGishConfig = VGGishConfig()) -> VGGish:
    """A ``VGGish`` with the state dict of ``weights`` (a ``.pth`` file) or of the file ``SYNCFUSION_VGGISH_WEIGHTS`` names.  Nothing is fetched."""
    path = weights if weights is not None else os.environ.get(WEIGHTS_ENV)
    if not path:
        raise RuntimeError(f"the FAD needs VGGish weights: pass weights=<vggish .pth state dict>, model=<a VGGish>, or set {WEIGHTS_ENV} "
                           "(nothing is downloaded)")
    state = torch.load(str(path), map_location="cpu")
    if isinstance(state, dict) and "state_dict" in state and not any(k.startswith("features.") for k in state):
        state = state["state_dict"]
    model = VGGish(config)
    model.load_state_dict(state)
    return model.eval()


def _resolve_device(device) -> torch.device:
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    _lib.require_gpu_tensor(torch.empty(0, device=device), "evaluate_fad")
    return device


def load_dir(audio_dir, config: VGGishConfig, device=None) -> Dict[int, List[Tensor]]:
    """Every ``*.wav`` of a directory as mono host waveforms at the model's rate, grouped by length.  Mono by channel mean; a file at another
    rate goes through ``syncfusion_amd.resample`` on ``device``."""
    by_length: Dict[int, List[Tensor]] = {}
    for p in sorted(Path(audio_dir).glob("*.wav")):
        a, rate = load_wav(p)
        a = a.mean(dim=0)
        if rate != config.sample_rate and a.numel() > 0:
            a = resample(a.to(_resolve_device(device)), rate, config.sample_rate).cpu()
        by_length.setdefault(int(a.numel()), []).append(a)
    return by_length


def embed_clips(by_length: Dict[int, List[Tensor]], model: VGGish, device, batch_size: int = 64) -> Tuple[Moments, List[Tensor]]:
    """``load_dir``'s clips -> the moments of their embeddings and the embeddings themselves (device tensors, one per batch, in the order of
    the lengths and of the files within a length).  Files of equal length run as one batch; a file shorter than one example contributes
    nothing."""
    D = int(model.config.fc[-1])
    total = Moments(0, np.zeros(D), np.zeros((D, D)))
    embs: List[Tensor] = []
    for L, clips in by_length.items():
        if model.config.examples(L) < 1:
            continue
        for i in range(0, len(clips), batch_size):
            emb = model(torch.stack(clips[i:i + batch_size]).to(device))
            embs.append(emb)
            total = total.merge(embedding_moments(emb))
    return total, embs


def evaluate_fad(experiment_path, gt_path, weights: Optional[Union[str, Path]] = None, model: Optional[VGGish] = None, batch_size: int = 64,
                 device=None) -> Dict[str, object]:
    """``main.evaluation.evaluate_fad`` for two directories of wav files -> ``{"FAD", "n_gen", "n_gt"}`` (``n_*``: examples per side).
    ``gt_path`` is the background set, as in ``frechet.score(original_path, generation_path)``.  ``model``: a ``VGGish`` with its weights
    loaded; else ``weights`` / ``SYNCFUSION_VGGISH_WEIGHTS`` name a ``.pth`` state dict.  A side with fewer than two examples raises
    ``ValueError`` before anything runs on the device."""
    experiment_path, gt_path = Path(experiment_path), Path(gt_path)
    if model is None:
        model = load_vggish(weights)
    for path in (experiment_path, gt_path):
        if not path.exists():
            raise FileNotFoundError(str(path))
    cfg = model.config
    clips = {}
    for name, path in (("gt", gt_path), ("gen", experiment_path)):
        clips[name] = load_dir(path, cfg, device)
        n = sum(cfg.examples(L) * len(c) for L, c in clips[name].items())
        if n < 2:
            raise ValueError(f"{path}: {n} VGGish example(s); the covariance needs at least 2 (a clip below "
                             f"{cfg.window_length + (cfg.example_frames - 1) * cfg.hop_length} samples at {cfg.sample_rate} Hz holds none)")
    device = _resolve_device(device)
    model = model.to(device).eval()
    mu_b, s_b, n_b = embed_clips(clips["gt"], model, device, batch_size)[0].statistics()
    mu_e, s_e, n_e = embed_clips(clips["gen"], model, device, batch_size)[0].statistics()
    return {"FAD": frechet_distance(mu_b, s_b, mu_e, s_e), "n_gen": n_e, "n_gt": n_b}


def write_metrics_csv(path, fad: float) -> None:
    """The one-line csv pandas writes for main/evaluation.py:25-26 (``DataFrame(columns=["FAD"]); df.loc[0] = score``)."""
    Path(path).write_text(f",FAD\n0,{fad!r}\n")
