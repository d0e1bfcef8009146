"""Boundary object of the generation path: mirror of ``main.module_diffusion.Model``.

Reference: main/module_diffusion.py:22-87.  Same constructor arguments, same attributes
(``model``, ``onsets_encoder``, ``clap``), same helper methods (``clap_encode_audio`` /
``clap_encode_text`` / ``step``).  ``pytorch_lightning`` is used as the base class when it is
importable (it is not in this image), otherwise ``torch.nn.Module`` with the two attributes the
callers touch (``device``, ``log``).
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

try:  # pragma: no cover - not installed in the build image
    import pytorch_lightning as pl

    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    class _Base(nn.Module):
        @property
        def device(self) -> torch.device:
            try:
                return next(self.parameters()).device
            except StopIteration:
                return torch.device("cpu")

        def log(self, *args, **kwargs) -> None:  # Lightning's self.log is a no-op without a Trainer
            return None

Tensor = torch.Tensor


def int16_to_float32(x: Tensor) -> Tensor:
    """main/utils.py:22-23."""
    return (x / 32767.0).to(torch.float32)


def float32_to_int16(x: Tensor) -> Tensor:
    """main/utils.py:26-28."""
    x = torch.clip(x, min=-1.0, max=1.0)
    return (x * 32767.0).to(torch.int16)


class RandomEmbedder(nn.Module):
    """Offline stand-in for ``laion_clap.CLAP_Module`` (out of scope).

    Implements the four members the reference touches (main/module_diffusion.py:48-51,67,71) and returns
    deterministic unit-norm ``(B, 512)`` vectors derived from the input, so benchmarks and tests have a
    well-defined conditioning tensor without the CLAP checkpoint."""

    def __init__(self, features: int = 512, **_ignored):
        super().__init__()
        self.features = features
        self.register_buffer("proj", torch.randn(64, features, generator=torch.Generator().manual_seed(2000)))

    def load_ckpt(self, path=None) -> None:
        return None

    def _embed(self, feats: Tensor) -> Tensor:
        e = feats.to(self.proj.dtype) @ self.proj
        return torch.nn.functional.normalize(e, dim=-1)

    def get_audio_embedding_from_data(self, x: Tensor, use_tensor: bool = True) -> Tensor:
        B = x.shape[0]
        frames = x.reshape(B, -1)
        n = frames.shape[1] // 64 * 64
        feats = frames[:, :n].reshape(B, 64, -1).abs().mean(-1) if n else torch.zeros(B, 64, device=x.device)
        return self._embed(feats + 1e-3)

    def get_text_embedding(self, text: List[str], use_tensor: bool = True) -> Tensor:
        feats = torch.zeros(len(text), 64)
        for i, t in enumerate(text):
            for j, ch in enumerate(t.encode()):
                feats[i, (j * 31 + ch) % 64] += 1.0
        return self._embed(feats.to(self.proj.device) + 1e-3)


OPTIMIZERS = ("torch", "hip")


def check_optimizer_choice(optimizer: str) -> str:
    """The ``optimizer`` init-arg of both ``Model`` classes: ``"torch"`` (default: ``torch.optim.AdamW``, fused on the GPU) or ``"hip"``
    (``syncfusion_amd.optim.AdamW``: the same update and the gradient clipping in the HIP library, when every parameter is on the GPU)."""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
    return optimizer


def make_adamw(params, optimizer: str, **hyper) -> torch.optim.AdamW:
    """``configure_optimizers`` of both ``Model`` classes: AdamW over ``params``; on the GPU torch's single-kernel (``fused``) step, or
    with ``optimizer == "hip"`` the HIP class.  CPU parameters get the plain ``torch.optim.AdamW`` whatever ``optimizer`` says."""
    on_gpu = bool(params) and all(p.is_cuda for p in params)
    if optimizer == "hip" and on_gpu:
        from .optim import AdamW

        return AdamW(params, **hyper)
    return torch.optim.AdamW(params, **hyper, **({"fused": True} if on_gpu else {}))


VARIANTS_KEY = "syncfusion_amd.unet_variants"   # checkpoint entry next to `state_dict`: the three [RECALLED] facts of the U-Net


class Model(_Base):
    def __init__(self, lr: float, lr_beta1: float, lr_beta2: float, lr_eps: float, lr_weight_decay: float,
                 model: nn.Module, onsets_encoder: nn.Module, embedder: nn.Module, embedder_checkpoint: Optional[str], optimizer: str = "torch"):
        super().__init__()
        self.optimizer = check_optimizer_choice(optimizer)
        self.lr = lr
        self.lr_beta1 = lr_beta1
        self.lr_beta2 = lr_beta2
        self.lr_eps = lr_eps
        self.lr_weight_decay = lr_weight_decay
        self.model = model
        self.onsets_encoder = onsets_encoder
        print(f"Loading CLAP embedder from {embedder_checkpoint}...")
        self.clap = embedder
        self.clap.load_ckpt(embedder_checkpoint)
        for param in self.clap.parameters():
            param.requires_grad = False

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False, *, hypothesis=None):
        """``model.load_state_dict(checkpoint['state_dict'])`` as main/generation.py:43 calls it.  Accepts this build's key
        layout AND the upstream one (audio_diffusion_pytorch / a-unet / audio_encoders_pytorch module trees; see
        syncfusion_amd/keymap.py for how, and for what is [RECALLED] about it).  The frozen embedder's ``clap.*`` tensors
        are loaded only when this model's embedder actually has those keys (the offline stub does not).  Positional signature =
        ``nn.Module.load_state_dict(state_dict, strict, assign)``; ``hypothesis`` (a ``keymap.OrderHypothesis``) is keyword-only.
        ``strict=False`` tolerates what nn.Module tolerates: with this build's own key layout, missing keys keep their current
        values and unexpected keys are reported in the returned ``_IncompatibleKeys`` instead of raising."""
        from .keymap import IGNORED_PREFIXES, KeyMapError, _DUP_NET, _strip, infer_variants, translate_state_dict

        # [RECALLED] facts that change parameter SHAPES (the time embedder's width, a bias on the attention output projections): when the
        # checkpoint's own tensors decide them differently from how this model was built, the U-Net re-registers those parameters first
        net_sd = _strip({k: v for k, v in state_dict.items() if not _DUP_NET.match(k)}, "model.net.")
        if net_sd and hasattr(self.model.net, "adopt_variants"):
            net = self.model.net
            if True:
                facts = infer_variants(net_sd, net.hparams)
                # The third [RECALLED] fact has no parameters.  A checkpoint whose time embedder has the NumberEmbedder layout (F learned
                # frequencies, Linear(2 F + 1 -> features), F != features / 2) was written by a-unet's embedder, which -- as recalled -- is
                # LearnedPositionalEmbedding -> Linear with NO activation in front of the two (Linear, GELU) layers.  Unless the caller
                # stated time_first_activation explicitly, follow the layout, and say so: the alternative is a silently different time
                # embedding in engine, training composition and oracle.
                deviates = {k: v for k, v in facts.items() if net.hparams.get(k) != v}
                if "time_fourier_features" in deviates and not getattr(net, "time_first_activation_explicit", False) and net.hparams.get("time_first_activation", True):
                    facts["time_first_activation"] = False
                    import warnings

                    warnings.warn(f"checkpoint shows a-unet's NumberEmbedder layout (time_fourier_features={facts['time_fourier_features']}): "
                                  "time_first_activation was not stated and is switched OFF to match it (a-unet's embedder has no activation behind its "
                                  "Linear, [RECALLED]); pass net_t(time_first_activation=True/False) to decide it yourself, or run tools/pin_upstream.py",
                                  stacklevel=2)
                elif deviates:
                    import warnings

                    warnings.warn(f"checkpoint tensors decide {deviates} differently from how this model was built; the affected parameters are "
                                  "re-registered.  time_first_activation has no parameters and stays "
                                  f"{net.hparams.get('time_first_activation', True)} (state it explicitly if the checkpoint needs otherwise)", stacklevel=2)
                net.adopt_variants(**facts)
        own = super().state_dict()
        try:
            mapped = translate_state_dict(state_dict, self, hypothesis)
            extra = {}
        except KeyMapError:
            # strict=False on a partial checkpoint in this build's OWN layout: hand torch what matches, let it report the rest
            if strict or not any(k in own for k in state_dict):
                raise
            mapped = {k: v for k, v in state_dict.items() if k in own}
            extra = {k: v for k, v in state_dict.items() if k not in own and not k.startswith(IGNORED_PREFIXES)}
        if not extra and all(k in state_dict for k in mapped):      # local layout: unexpected non-embedder keys are torch's to report
            extra = {k: v for k, v in state_dict.items() if k not in own and not k.startswith(IGNORED_PREFIXES)
                     and not k.startswith(("model.diffusion.net.", "model.sampler.net."))}
        for k in own:
            if k.startswith(IGNORED_PREFIXES):
                mapped[k] = state_dict[k] if k in state_dict and tuple(state_dict[k].shape) == tuple(own[k].shape) else own[k]
        mapped.update(extra)
        return super().load_state_dict(mapped, strict=strict, assign=assign)

    # Lightning's checkpoint hooks (called by the Trainer around state_dict save / load; call them yourself around torch.save / torch.load
    # without a Trainer): the three [RECALLED] facts this U-Net was built with travel in the checkpoint NEXT TO `state_dict`, so a reload is
    # deterministic -- time_first_activation has no parameters it could be inferred from.
    def on_save_checkpoint(self, checkpoint: dict) -> None:
        net = self.model.net
        checkpoint[VARIANTS_KEY] = {k: net.hparams.get(k) for k in ("time_fourier_features", "time_first_activation", "attention_out_bias")}

    def on_load_checkpoint(self, checkpoint: dict) -> None:
        saved = checkpoint.get(VARIANTS_KEY)
        if isinstance(saved, dict) and hasattr(self.model.net, "adopt_variants"):
            self.model.net.adopt_variants(**{k: saved[k] for k in ("time_fourier_features", "time_first_activation", "attention_out_bias") if k in saved})
            self.model.net.time_first_activation_explicit = True     # decided by the checkpoint: load_state_dict must not second-guess it

    def configure_optimizers(self):
        """main/module_diffusion.py:53-61: AdamW over the U-Net and the onset encoder.  On the GPU the single-kernel (``fused``)
        implementation of the same update is used: 4.2 instead of 8.7 ms for the 215 M parameters.  ``optimizer="hip"`` (init-arg) returns
        ``syncfusion_amd.optim.AdamW`` instead -- a ``torch.optim.AdamW`` whose step and gradient clipping are one call into the HIP library --
        when every parameter is on the GPU."""
        params = list(self.model.parameters()) + list(self.onsets_encoder.parameters())
        return make_adamw(params, self.optimizer, lr=self.lr, betas=(self.lr_beta1, self.lr_beta2), eps=self.lr_eps, weight_decay=self.lr_weight_decay)

    @torch.no_grad()
    def clap_encode_audio(self, x: Tensor) -> Tensor:
        x = int16_to_float32(float32_to_int16(x[:, 0, :])).float()
        return self.clap.get_audio_embedding_from_data(x=x, use_tensor=True).unsqueeze(1)

    @torch.no_grad()
    def clap_encode_text(self, text: List[str]) -> Tensor:
        return self.clap.get_text_embedding(text, use_tensor=True).unsqueeze(1)

    def step(self, batch):
        x, y, z, _, _ = batch
        z_latent = self.clap_encode_audio(z)
        _, y_latent = self.onsets_encoder(y, with_info=True)
        return self.model(x, channels=y_latent["xs"][2:-1], embedding=z_latent)

    def training_step(self, batch, batch_idx):
        """main/module_diffusion.py:79-82.  With autograd recording, ``step`` runs the differentiable fp32 composition
        (syncfusion_amd/training.py: HIP forward + backward kernels), so the returned loss carries a graph onto the U-Net's and
        the onset encoder's parameters.  Called under ``torch.no_grad()`` or with every parameter frozen there is nothing to
        train, and returning a graph-less loss to a trainer would fail inside ``loss.backward()`` with an opaque message."""
        from .training import training_step_scope

        with training_step_scope():
            loss = self.step(batch)
        if not loss.requires_grad:
            raise RuntimeError("training_step: the loss carries no autograd graph (grad mode is off or every parameter is frozen)")
        self.log("train_loss", loss)
        return loss

    def validation_step(self, batch, batch_idx):
        loss = self.step(batch)
        self.log("valid_loss", loss)
        return loss
