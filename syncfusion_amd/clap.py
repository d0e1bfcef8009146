"""CLAP audio embedder on the device: the conditioning vector of the diffusion model, ``clap_encode_audio``.

Replaces ``laion_clap.CLAP_Module(enable_fusion=False, amodel='HTSAT-tiny')`` (exp/model/diffusion.yaml:45-48) as far as the reference
uses it: ``load_ckpt`` and ``get_audio_embedding_from_data(x, use_tensor=True)`` (main/module_diffusion.py:48-51, 64-67).  Neither
``laion_clap`` nor ``transformers``, ``torchlibrosa`` or ``timm`` is needed.  The mel power comes from the FFT front end
(``csrc/audio_features.hip``); the log / BatchNorm / bicubic / fold pass, the patch embed and the embedding tail run in
``csrc/clap_front.hip``, shifted-window attention and the LayerNorms in ``csrc/swin.hip``, every Linear on the library's fp32
implicit-GEMM launcher (``csrc/clap_engine.cpp``).  The text branch (RoBERTa) lives in ``clap_text.py`` (``ClapEmbedder``, a subclass that
adds it); this class keeps refusing text.  Weights come from a file the user supplies;
nothing is ever fetched.  The default ``config.TARGET_MAP`` still sends ``laion_clap.CLAP_Module`` to the offline stub; opt in with
``_target_: syncfusion_amd.clap.ClapAudioEmbedder`` or ``instantiate(cfg, embedder=ClapAudioEmbedder(), embedder_checkpoint=...)``.

Pinning status: UNPINNED.  The arithmetic lives in ``laion_clap`` (``htsat.py``, ``hook.py``, ``training/data.py``), absent from the
reference tree and from this image: restated from the published code as recalled, every recalled value a field of ``ClapAudioConfig``,
and pinned against an independent fp64 restatement (tests/clap_ref.py).  Whoever pins it against upstream later should change
defaults, not code.  The recalled facts:

* length: clips are ``clip_samples`` (480000 at 48 kHz) long; a shorter clip is tiled ``int(clip_samples / L)`` whole times and
  zero-padded ("repeatpad"), a longer one cut at a host-drawn random start (``rand_trunc``) or at its head;
* log-mel: ``n_fft`` 1024, hop 480, periodic Hann, ``center=True`` with reflect padding, power 2; 64 Slaney mel bands with Slaney
  normalisation from 50 to 14000 Hz; ``10 log10(max(P, 1e-10))``, no ``top_db``; 1001 frames.  A checkpoint's
  ``logmel_extractor.melW`` replaces the computed filterbank;
* ``bn0``: ``BatchNorm2d(64)`` per mel bin in inference form;
* ``reshape_wav2img``: bicubic (A = -0.75, ``align_corners=True``) along time to ``spec_size * freq_ratio`` = 1024 frames, then the
  time axis folded into ``freq_ratio`` = 4 bands of rows: ``image[r * 64 + f][t'] = x[r * 256 + t'][f]``;
* Swin: ``Conv2d(1, 96, 4, 4)`` + LayerNorm patch embed, no absolute position embedding; depths (2, 2, 6, 2), heads (4, 8, 16, 32)
  (head dim 24), window 8, shift 4 on odd blocks (none where the map is one window), relative-position bias ``(dy + 7) * 15 + dx + 7``,
  mask -100 between shift regions, MLP ratio 4 with GELU(erf), PatchMerging ``[(0::2,0::2), (1::2,0::2), (0::2,1::2), (1::2,1::2)]``
  -> LayerNorm -> Linear(4C, 2C, no bias) behind the first three stages;
* head: LayerNorm(768), the mean over the 64 final tokens, ``Linear(768, 512)`` - ReLU - ``Linear(512, 512)``, L2 normalisation.

Parameter and buffer names are upstream's (``model.audio_branch.*``, ``model.audio_projection.{0,2}.*``), so an upstream state dict and
the ``clap.*`` part of a SyncFusion checkpoint load.
"""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib
from .audio_features import compact_filterbank, mel_filterbank

Tensor = torch.Tensor
PATCH = 4
KEY_PREFIXES = ("module.", "clap.", "model.")
# parts of an upstream checkpoint this path never reads
IGNORED_PARTS = ("spectrogram_extractor.", "tscam_conv.", "attn_mask", "relative_position_index", "num_batches_tracked")
OPTIONAL_KEYS = ("model.audio_branch.logmel_extractor.melW", "model.audio_branch.bn0.num_batches_tracked")


@dataclass
class ClapAudioConfig:
    """Every recalled value of the audio path (module docstring)."""
    sample_rate: int = 48000
    clip_samples: int = 480000
    truncation: str = "rand"              # a clip longer than clip_samples: "rand" (upstream's rand_trunc, host RNG) or "head"
    n_fft: int = 1024
    hop: int = 480
    mel_bins: int = 64
    fmin: float = 50.0
    fmax: float = 14000.0
    amin: float = 1e-10
    bn_eps: float = 1e-5
    spec_size: int = 256
    embed_dim: int = 96
    depths: Tuple[int, ...] = (2, 2, 6, 2)
    num_heads: Tuple[int, ...] = (4, 8, 16, 32)
    window_size: int = 8
    mlp_ratio: int = 4
    ln_eps: float = 1e-5
    mask_value: float = -100.0
    joint_dim: int = 512
    projection_act: str = "relu"          # between the two projection Linears: "relu" or "none"
    normalize: bool = True
    seed: int = 2000                      # of the initialisation a missing checkpoint leaves in place

    @property
    def freq_ratio(self) -> int:
        return self.spec_size // self.mel_bins

    @property
    def target_frames(self) -> int:
        return self.spec_size * self.freq_ratio

    @property
    def frames(self) -> int:
        return 1 + self.clip_samples // self.hop

    @property
    def tokens_side(self) -> int:
        return self.spec_size // PATCH

    @property
    def final_dim(self) -> int:
        return self.embed_dim << (len(self.depths) - 1)

    def stage_resolution(self, i: int) -> int:
        return self.tokens_side >> i

    def block_shift(self, i: int, j: int) -> int:
        """Shift of block ``j`` of stage ``i``: half a window on odd blocks, none where the stage's map is a single window."""
        return 0 if self.stage_resolution(i) <= self.window_size or j % 2 == 0 else self.window_size // 2

    def check(self) -> None:
        if self.truncation not in ("rand", "head"):
            raise ValueError(f"truncation {self.truncation!r}: 'rand' or 'head'")
        if self.projection_act not in ("relu", "none"):
            raise ValueError(f"projection_act {self.projection_act!r}: 'relu' or 'none'")
        if len(self.depths) != len(self.num_heads) or not 1 <= len(self.depths) <= _lib.SF_CLAP_MAX_STAGES:
            raise ValueError("depths and num_heads: one entry per stage, 1 .. 8 stages")
        if self.spec_size % self.mel_bins or self.spec_size % (PATCH * self.window_size << (len(self.depths) - 1)):
            raise ValueError(f"spec_size {self.spec_size}: a multiple of mel_bins and of {PATCH * self.window_size << (len(self.depths) - 1)} expected")
        if self.frames > self.target_frames:
            raise ValueError(f"{self.frames} frames exceed the image's {self.target_frames}: a longer spectrogram is not shrunk")
        if self.clip_samples <= self.n_fft // 2:
            raise ValueError("clip_samples must exceed n_fft / 2 (reflect padding)")


def clap_mel_matrix(cfg: ClapAudioConfig) -> np.ndarray:
    """``(n_fft // 2 + 1, mel_bins)`` fp64, upstream's ``melW``: Slaney scale and normalisation (``librosa.filters.mel`` transposed)."""
    return mel_filterbank(cfg.sample_rate, cfg.n_fft, cfg.mel_bins, cfg.fmin, cfg.fmax, "slaney", "slaney").T.copy()


def fit_length(x: Tensor, cfg: ClapAudioConfig, rng=np.random) -> Tensor:
    """``(B, L)`` -> ``(B, clip_samples)``: repeatpad of a short clip, ``cfg.truncation`` of a long one (every clip of the batch at the same start)."""
    B, L = x.shape
    n = cfg.clip_samples
    if L == n:
        return x
    if L > n:
        start = int(rng.randint(0, L - n + 1)) if cfg.truncation == "rand" else 0
        return x[:, start:start + n]
    if L < 1:
        raise ValueError("empty waveform")
    out = x.new_zeros((B, n))
    reps = int(n / L)
    out[:, :reps * L] = x.repeat(1, reps)
    return out


# ---- the module tree: upstream's names ----------------------------------------------------------------------------------------------------
class _Attn(nn.Module):
    def __init__(self, C: int, heads: int, window: int):
        super().__init__()
        self.relative_position_bias_table = nn.Parameter(0.02 * torch.randn((2 * window - 1) ** 2, heads))
        self.qkv = nn.Linear(C, 3 * C)
        self.proj = nn.Linear(C, C)


class _Mlp(nn.Module):
    def __init__(self, C: int, ratio: int):
        super().__init__()
        self.fc1 = nn.Linear(C, ratio * C)
        self.fc2 = nn.Linear(ratio * C, C)


class _Block(nn.Module):
    def __init__(self, C: int, heads: int, cfg: ClapAudioConfig):
        super().__init__()
        self.norm1 = nn.LayerNorm(C, eps=cfg.ln_eps)
        self.attn = _Attn(C, heads, cfg.window_size)
        self.norm2 = nn.LayerNorm(C, eps=cfg.ln_eps)
        self.mlp = _Mlp(C, cfg.mlp_ratio)


class _Merge(nn.Module):
    def __init__(self, C: int, cfg: ClapAudioConfig):
        super().__init__()
        self.norm = nn.LayerNorm(4 * C, eps=cfg.ln_eps)
        self.reduction = nn.Linear(4 * C, 2 * C, bias=False)


class _Stage(nn.Module):
    def __init__(self, C: int, depth: int, heads: int, merge: bool, cfg: ClapAudioConfig):
        super().__init__()
        self.blocks = nn.ModuleList([_Block(C, heads, cfg) for _ in range(depth)])
        if merge:
            self.downsample = _Merge(C, cfg)


class _PatchEmbed(nn.Module):
    def __init__(self, cfg: ClapAudioConfig):
        super().__init__()
        self.proj = nn.Conv2d(1, cfg.embed_dim, PATCH, PATCH)
        self.norm = nn.LayerNorm(cfg.embed_dim, eps=cfg.ln_eps)


class _MelW(nn.Module):
    def __init__(self, cfg: ClapAudioConfig):
        super().__init__()
        self.register_buffer("melW", torch.from_numpy(clap_mel_matrix(cfg)).float())


class _HTSAT(nn.Module):
    def __init__(self, cfg: ClapAudioConfig):
        super().__init__()
        self.logmel_extractor = _MelW(cfg)
        self.bn0 = nn.BatchNorm2d(cfg.mel_bins, eps=cfg.bn_eps)
        self.patch_embed = _PatchEmbed(cfg)
        n = len(cfg.depths)
        self.layers = nn.ModuleList([_Stage(cfg.embed_dim << i, cfg.depths[i], cfg.num_heads[i], i + 1 < n, cfg) for i in range(n)])
        self.norm = nn.LayerNorm(cfg.final_dim, eps=cfg.ln_eps)


class _ClapModel(nn.Module):
    def __init__(self, cfg: ClapAudioConfig):
        super().__init__()
        self.audio_branch = _HTSAT(cfg)
        self.audio_projection = nn.Sequential(nn.Linear(cfg.final_dim, cfg.joint_dim), nn.ReLU(), nn.Linear(cfg.joint_dim, cfg.joint_dim))


AUDIO_PARTS = ("audio_branch.", "audio_projection.")


def normalise_keys(state: Dict[str, Tensor], parts: Tuple[str, ...] = AUDIO_PARTS, ignored: Tuple[str, ...] = IGNORED_PARTS) -> Dict[str, Tensor]:
    """An upstream / Lightning / SyncFusion state dict -> ``{"model.<part>*": tensor}`` for the ``parts`` a class reads (the audio class:
    ``audio_branch.``, ``audio_projection.``): the prefixes ``module.``, ``clap.``, ``model.`` are stripped in any combination; everything
    else (for the audio class the text branch and ``text_*``; ``logit_scale_*``, ``audio_transform.*``) and, inside the parts, whatever
    holds one of ``ignored`` (the STFT convolutions, ``tscam_conv.*``, ``attn_mask``, ``relative_position_index``) and ``head.*`` are dropped."""
    out: Dict[str, Tensor] = {}
    for k, v in state.items():
        key = k
        while key.startswith(KEY_PREFIXES):
            key = key[len(next(p for p in KEY_PREFIXES if key.startswith(p))):]
        if not key.startswith(parts):
            continue
        if key.startswith("audio_branch.head.") or any(part in key for part in ignored):
            continue
        out["model." + key] = v
    return out


class ClapAudioEmbedder(nn.Module):
    """``laion_clap.CLAP_Module`` as the reference uses it, audio side only.  Frozen; behaviour does not depend on ``train()`` /
    ``eval()`` (BatchNorm always uses its running statistics).  The engine copies the weights when it is built: every weight load
    (``load_ckpt``, ``load_state_dict``, a parent's ``load_state_dict``) and every ``.to()`` drops it, and the next call builds it again;
    after editing a parameter in place call ``invalidate()``."""

    # what load_state_dict keeps of a checkpoint: the parts this class owns, minus the keys that hold one of IGNORED (a subclass extends both)
    PARTS: Tuple[str, ...] = AUDIO_PARTS
    IGNORED: Tuple[str, ...] = IGNORED_PARTS

    def __init__(self, config: Optional[ClapAudioConfig] = None, enable_fusion: bool = False, amodel: str = "HTSAT-tiny", **_ignored):
        super().__init__()
        if enable_fusion:
            raise ValueError(f"{type(self).__name__}: enable_fusion=True (the fusion model) is not built")
        if amodel != "HTSAT-tiny":
            raise ValueError(f"{type(self).__name__}: amodel {amodel!r} is not built, only 'HTSAT-tiny'")
        self.config = config = ClapAudioConfig() if config is None else config
        config.check()
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(config.seed)
            self.model = _ClapModel(config)
        for p in self.parameters():
            p.requires_grad = False
        self._fronts: Dict[str, int] = {}
        self._engine: Optional[int] = None
        self._engine_device: Optional[str] = None
        self._scale_shift: Optional[Tuple[Tensor, Tensor]] = None
        self._warned = False
        self._register_load_state_dict_pre_hook(lambda *args: self.invalidate())

    # -- weights
    def _release(self, engine: bool = True, fronts: bool = True) -> None:
        d = self.__dict__
        h = d.get("_engine") if engine else None
        fr = (d.get("_fronts") or {}) if fronts else {}
        if engine:
            d["_engine"], d["_engine_device"] = None, None
        if fronts:
            d["_fronts"] = {}
        if not h and not fr:
            return
        try:
            lib = _lib.load()
            if h:
                lib.sf_clap_audio_destroy(h)
            for f in fr.values():
                lib.sf_audio_features_destroy(f)
        except Exception:               # interpreter shutdown
            pass

    def invalidate(self) -> None:
        """Forget everything derived from the weights (the engine's copy, the folded BatchNorm, the filterbank tables)."""
        self._release()
        self.__dict__["_scale_shift"] = None

    def __del__(self):
        self.invalidate()

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, state_dict, strict: bool = True, **kwargs):
        """Upstream's keys under any of the known prefixes; what the audio path does not read is dropped, ``logmel_extractor.melW`` is
        optional, a missing key or a shape mismatch in the rest raises and names the key."""
        own = super().state_dict()
        state = normalise_keys(state_dict, self.PARTS, self.IGNORED)
        for k in OPTIONAL_KEYS:
            state.setdefault(k, own[k])
        for k, v in own.items():
            if k not in state:
                raise KeyError(f"{type(self).__name__}: the checkpoint has no '{k[len('model.'):]}'")
            if tuple(state[k].shape) != tuple(v.shape):
                raise ValueError(f"{type(self).__name__}: '{k[len('model.'):]}' has shape {tuple(state[k].shape)}, expected {tuple(v.shape)}")
        self.invalidate()
        return super().load_state_dict({k: state[k] for k in own}, strict=True, **kwargs)

    def load_ckpt(self, path=None) -> None:
        """``CLAP_Module.load_ckpt``: a ``torch.save``d state dict (bare or under ``state_dict``), read on the CPU.  ``None`` keeps the seeded
        initialisation (upstream would download a checkpoint; nothing is fetched here) and says so once."""
        if path is None:
            if not self._warned:
                warnings.warn("ClapAudioEmbedder.load_ckpt(None): no checkpoint given, the seeded initialisation stays (nothing is downloaded); "
                              "the embeddings are those of an untrained network", stacklevel=2)
                self._warned = True
            return None
        state = torch.load(str(path), map_location="cpu")
        if isinstance(state, dict) and isinstance(state.get("state_dict"), dict):
            state = state["state_dict"]
        self.load_state_dict(state)
        return None

    def engine_weights(self) -> List[Tuple[str, Tensor]]:
        """The named fp32 tensors ``sf_clap_audio_create`` reads, every LayerNorm affine folded into the Linear behind it in fp64:
        ``W' = W diag(gamma)``, ``b' = b + W beta``."""
        ab = self.model.audio_branch
        d = lambda t: t.detach().double().cpu()
        out: List[Tuple[str, Tensor]] = [("patch.w", d(ab.patch_embed.proj.weight).reshape(self.config.embed_dim, PATCH * PATCH)),
                                         ("patch.b", d(ab.patch_embed.proj.bias)), ("patch.g", d(ab.patch_embed.norm.weight)),
                                         ("patch.beta", d(ab.patch_embed.norm.bias))]

        def folded(norm: nn.LayerNorm, lin: nn.Linear):
            w, g, beta = d(lin.weight), d(norm.weight), d(norm.bias)
            b = w @ beta
            return w * g[None, :], b + d(lin.bias) if lin.bias is not None else b

        for i, st in enumerate(ab.layers):
            for j, blk in enumerate(st.blocks):
                p = f"s{i}.b{j}."
                w, b = folded(blk.norm1, blk.attn.qkv)
                out += [(p + "qkv.w", w), (p + "qkv.b", b), (p + "rpb", d(blk.attn.relative_position_bias_table)),
                        (p + "proj.w", d(blk.attn.proj.weight)), (p + "proj.b", d(blk.attn.proj.bias))]
                w, b = folded(blk.norm2, blk.mlp.fc1)
                out += [(p + "fc1.w", w), (p + "fc1.b", b), (p + "fc2.w", d(blk.mlp.fc2.weight)), (p + "fc2.b", d(blk.mlp.fc2.bias))]
            if hasattr(st, "downsample"):
                w, b = folded(st.downsample.norm, st.downsample.reduction)
                out += [(f"s{i}.merge.w", w), (f"s{i}.merge.b", b)]
        pr = self.model.audio_projection
        out += [("head.g", d(ab.norm.weight)), ("head.beta", d(ab.norm.bias)), ("proj0.w", d(pr[0].weight)), ("proj0.b", d(pr[0].bias)),
                ("proj2.w", d(pr[2].weight)), ("proj2.b", d(pr[2].bias))]
        return [(k, v.float().contiguous()) for k, v in out]

    def bn_scale_shift(self) -> Tuple[Tensor, Tensor]:
        """``bn0`` in inference form as one multiply-add per mel bin, folded in fp64: ``scale = w / sqrt(var + eps)``, ``shift = b - mean scale``."""
        bn = self.model.audio_branch.bn0
        scale = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
        return scale.float(), (bn.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu() * scale).float()

    def engine_config(self) -> "_lib.ClapAudioEngineConfig":
        cfg = self.config
        c = _lib.ClapAudioEngineConfig()
        c.spec_size, c.embed_dim, c.n_stages = cfg.spec_size, cfg.embed_dim, len(cfg.depths)
        for i, (dep, nh) in enumerate(zip(cfg.depths, cfg.num_heads)):
            c.depths[i], c.heads[i] = int(dep), int(nh)
        c.window, c.mlp_ratio, c.joint_dim = cfg.window_size, cfg.mlp_ratio, cfg.joint_dim
        c.ln_eps, c.mask_value = cfg.ln_eps, cfg.mask_value
        c.projection_relu, c.normalize = int(cfg.projection_act == "relu"), int(bool(cfg.normalize))
        return c

    def describe_gemms(self, B: int) -> str:
        """One line per GEMM of the network at batch ``B`` with the kernel family the library's dispatcher gives it (host only)."""
        buf = C.create_string_buffer(1 << 14)
        cfg = self.engine_config()
        _lib.check(_lib.load().sf_clap_audio_describe(C.byref(cfg), int(B), buf, len(buf)), "sf_clap_audio_describe")
        return buf.value.decode()

    # -- device pieces
    def _front(self, device: torch.device) -> int:
        key = str(device)
        if key not in self._fronts:
            cfg = self.config
            first, count, w = compact_filterbank(self.model.audio_branch.logmel_extractor.melW.detach().double().cpu().numpy().T)
            h = C.c_void_p()
            _lib.check(_lib.load().sf_audio_features_create(cfg.n_fft, cfg.hop, cfg.mel_bins, 1, first.ctypes.data, count.ctypes.data, w.ctypes.data,
                                                            int(w.size), C.byref(h)), "sf_audio_features_create")
            self._fronts[key] = h.value
        return self._fronts[key]

    def _engine_for(self, device: torch.device) -> int:
        if self._engine is None or self._engine_device != str(device):
            self._release(fronts=False)
            table = _lib.TensorTable(self.engine_weights(), device)
            cfg = self.engine_config()
            h = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(_lib.load().sf_clap_audio_create(C.byref(cfg), table.array, table.n, _lib.stream_ptr(device), C.byref(h)),
                           "sf_clap_audio_create")
            self._engine, self._engine_device = h.value, str(device)
        return self._engine

    def mel_power(self, wav: Tensor) -> Tensor:
        """``(B, clip_samples)`` device waveforms -> ``(B, mel_bins, frames)`` mel power (``sf_logmel_forward``)."""
        _lib.require_gpu_tensor(wav, "ClapAudioEmbedder.mel_power")
        cfg = self.config
        x = _lib.f32c(wav)
        if x.dim() != 2 or x.shape[1] != cfg.clip_samples:
            raise ValueError(f"ClapAudioEmbedder: (B, {cfg.clip_samples}) waveforms expected, got {tuple(x.shape)}")
        B, L = x.shape
        lib, h = _lib.load(), self._front(x.device)
        need = int(lib.sf_audio_features_workspace_bytes(h, B, L))
        if need < 0:
            raise ValueError(f"ClapAudioEmbedder: B = {B}, L = {L} out of the front end's range")
        mel = torch.empty((B, cfg.mel_bins, cfg.frames), dtype=torch.float32, device=x.device)
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.sf_logmel_forward(h, x.data_ptr(), B, L, float(cfg.amin), 80.0, mel.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                             _lib.stream_ptr(x.device)), "sf_logmel_forward")
        return mel

    def logmel_image(self, mel_power: Tensor) -> Tensor:
        """``(B, mel_bins, T)`` mel power -> the ``(B, spec_size, spec_size)`` image the patch embed reads (``sf_op_logmel_image``)."""
        _lib.require_gpu_tensor(mel_power, "ClapAudioEmbedder.logmel_image")
        cfg = self.config
        m = _lib.f32c(mel_power)
        if m.dim() != 3 or m.shape[1] != cfg.mel_bins:
            raise ValueError(f"ClapAudioEmbedder: (B, {cfg.mel_bins}, T) mel power expected, got {tuple(m.shape)}")
        dev = m.device
        if self._scale_shift is None or self._scale_shift[0].device != dev:
            s, t = self.bn_scale_shift()
            self._scale_shift = (s.to(dev), t.to(dev))
        image = torch.empty((m.shape[0], cfg.spec_size, cfg.spec_size), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sf_op_logmel_image(m.data_ptr(), m.shape[0], cfg.mel_bins, m.shape[2], cfg.freq_ratio, self._scale_shift[0].data_ptr(),
                                                      self._scale_shift[1].data_ptr(), float(cfg.amin), image.data_ptr(), _lib.stream_ptr(dev)),
                       "sf_op_logmel_image")
        return image

    def tap_shapes(self, B: int) -> List[Tuple[int, int]]:
        """``(rows, columns)`` of the token matrix behind the patch embed and behind every stage (after its PatchMerging)."""
        cfg = self.config
        n = len(cfg.depths)
        shapes = [(B * cfg.tokens_side ** 2, cfg.embed_dim)]
        for i in range(n):
            k = min(i + 1, n - 1)
            shapes.append((B * cfg.stage_resolution(k) ** 2, cfg.embed_dim << k))
        return shapes

    def embed_image(self, image: Tensor, taps: bool = False):
        """``(B, spec_size, spec_size)`` image -> ``(B, joint_dim)`` embeddings; with ``taps`` also the token matrices of ``tap_shapes`` (tests)."""
        _lib.require_gpu_tensor(image, "ClapAudioEmbedder.embed_image")
        cfg = self.config
        x = _lib.f32c(image)
        if x.dim() != 3 or tuple(x.shape[1:]) != (cfg.spec_size, cfg.spec_size):
            raise ValueError(f"ClapAudioEmbedder: (B, {cfg.spec_size}, {cfg.spec_size}) images expected, got {tuple(x.shape)}")
        dev, B = x.device, x.shape[0]
        lib, eng = _lib.load(), self._engine_for(x.device)
        need = int(lib.sf_clap_audio_workspace_bytes(eng, B))
        if need < 0:
            raise ValueError(f"ClapAudioEmbedder: batch {B} outside 1 .. {int(lib.sf_clap_audio_max_batch(eng))}")
        out = torch.empty((B, cfg.joint_dim), dtype=torch.float32, device=dev)
        tapped = [torch.empty(s, dtype=torch.float32, device=dev) for s in self.tap_shapes(B)] if taps else []
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sf_clap_audio_forward(eng, x.data_ptr(), B, out.data_ptr(), _lib.ptr_array(tapped) if taps else None, ws.data_ptr(),
                                                 ws.numel(), _lib.stream_ptr(dev)), "sf_clap_audio_forward")
        return (out, tapped) if taps else out

    # -- the members the reference touches
    @torch.no_grad()
    def get_audio_embedding_from_data(self, x, use_tensor: bool = True):
        """``(B, L)`` waveforms at ``sample_rate`` -> ``(B, joint_dim)`` unit-norm fp32 embeddings.  ``use_tensor=True``: a device tensor in, a
        device tensor out, no synchronisation (after one warm-up call the call can be captured in a ``torch.cuda.graph``).
        ``use_tensor=False``: numpy in, upstream's int16 round trip applied, numpy out."""
        if not use_tensor:
            dev = next(self.parameters()).device
            a = torch.as_tensor(np.asarray(x), dtype=torch.float32)
            a = (torch.clip(a, -1.0, 1.0) * 32767.0).to(torch.int16).to(torch.float32) / 32767.0
            return self.get_audio_embedding_from_data(a.to(dev), use_tensor=True).cpu().numpy()
        if not isinstance(x, Tensor):
            raise TypeError("get_audio_embedding_from_data(use_tensor=True): a torch tensor expected")
        _lib.require_gpu_tensor(x, "ClapAudioEmbedder.get_audio_embedding_from_data")
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2:
            raise ValueError(f"ClapAudioEmbedder: (B, L) waveforms expected, got {tuple(x.shape)}")
        wav = fit_length(_lib.f32c(x), self.config)
        return self.embed_image(self.logmel_image(self.mel_power(wav)))

    def get_text_embedding(self, *args, **kwargs):
        raise NotImplementedError("ClapAudioEmbedder: the audio side only, no text branch (RoBERTa); syncfusion_amd.ClapEmbedder has both")
