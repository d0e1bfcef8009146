"""fp64 CPU restatement of the CLAP audio path (syncfusion_amd/clap.py, csrc/swin.hip, csrc/clap_front.hip, csrc/clap_engine.cpp), written the
textbook way: ``torch.stft``, ``F.interpolate(mode="bicubic", align_corners=True)``, ``torch.roll``, explicit ``window_partition`` /
``window_reverse``, a materialised attention mask, a dense ``relative_position_index``, ``F.layer_norm``, ``F.gelu``.  It shares no index
code with the product: the product does all of this as arithmetic inside its kernels.

State dicts are upstream-named WITHOUT a prefix (``audio_branch.*``, ``audio_projection.*``); every function takes ``dtype`` so that
tools/clap_bench.py can run the same composition in fp32 on the GPU.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from syncfusion_amd.audio_features import mel_filterbank
from syncfusion_amd.clap import ClapAudioConfig

Tensor = torch.Tensor

FULL = ClapAudioConfig()
NARROW = ClapAudioConfig(sample_rate=12000, n_fft=256, hop=120, mel_bins=32, fmin=50.0, fmax=5000.0, spec_size=128, clip_samples=60000,
                         depths=(2, 2, 2), num_heads=(4, 8, 16), embed_dim=96, joint_dim=64)


# ---- weights ----------------------------------------------------------------------------------------------------------------------------------
def seeded_weights(cfg: ClapAudioConfig, seed: int) -> Dict[str, Tensor]:
    """An upstream-named fp32 state dict with non-trivial LayerNorm affines, bn0 running statistics and bias tables."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd: Dict[str, Tensor] = {}

    def linear(name, n_out, n_in, bias=True):
        sd[name + ".weight"] = rn(n_out, n_in) / math.sqrt(n_in)
        if bias:
            sd[name + ".bias"] = 0.1 * rn(n_out)

    def norm(name, n):
        sd[name + ".weight"] = 1.0 + 0.2 * rn(n)
        sd[name + ".bias"] = 0.1 * rn(n)

    a = "audio_branch."
    sd[a + "logmel_extractor.melW"] = torch.from_numpy(mel_filterbank(cfg.sample_rate, cfg.n_fft, cfg.mel_bins, cfg.fmin, cfg.fmax, "slaney", "slaney").T.copy()).float()
    sd[a + "bn0.weight"] = 1.0 + 0.2 * rn(cfg.mel_bins)
    sd[a + "bn0.bias"] = 0.1 * rn(cfg.mel_bins)
    sd[a + "bn0.running_mean"] = -35.0 + 8.0 * rn(cfg.mel_bins)
    sd[a + "bn0.running_var"] = (15.0 + 5.0 * torch.rand(cfg.mel_bins, generator=g)) ** 2
    sd[a + "patch_embed.proj.weight"] = rn(cfg.embed_dim, 1, 4, 4) / 4.0
    sd[a + "patch_embed.proj.bias"] = 0.1 * rn(cfg.embed_dim)
    norm(a + "patch_embed.norm", cfg.embed_dim)
    n = len(cfg.depths)
    for i in range(n):
        C = cfg.embed_dim * 2 ** i
        for j in range(cfg.depths[i]):
            p = f"{a}layers.{i}.blocks.{j}."
            norm(p + "norm1", C)
            linear(p + "attn.qkv", 3 * C, C)
            sd[p + "attn.qkv.weight"][:2 * C] *= 2.0          # q and k: softmax rows neither flat nor one-hot
            sd[p + "attn.relative_position_bias_table"] = 0.5 * rn((2 * cfg.window_size - 1) ** 2, cfg.num_heads[i])
            linear(p + "attn.proj", C, C)
            norm(p + "norm2", C)
            linear(p + "mlp.fc1", cfg.mlp_ratio * C, C)
            linear(p + "mlp.fc2", C, cfg.mlp_ratio * C)
        if i + 1 < n:
            norm(f"{a}layers.{i}.downsample.norm", 4 * C)
            linear(f"{a}layers.{i}.downsample.reduction", 2 * C, 4 * C, bias=False)
    Cf = cfg.embed_dim * 2 ** (n - 1)
    norm(a + "norm", Cf)
    linear("audio_projection.0", cfg.joint_dim, Cf)
    linear("audio_projection.2", cfg.joint_dim, cfg.joint_dim)
    return sd


# ---- front ------------------------------------------------------------------------------------------------------------------------------------
def fit_length(x: Tensor, cfg: ClapAudioConfig, start: int = 0) -> Tensor:
    """repeatpad of a short clip; a long one cut at ``start``."""
    L, n = x.shape[-1], cfg.clip_samples
    if L > n:
        return x[..., start:start + n]
    if L == n:
        return x
    copies = [x] * int(n / L)
    return torch.cat(copies + [torch.zeros(x.shape[:-1] + (n - L * len(copies),), dtype=x.dtype, device=x.device)], dim=-1)


def mel_power(wav: Tensor, sd: Dict[str, Tensor], cfg: ClapAudioConfig, dtype=torch.float64) -> Tensor:
    """``(B, L)`` -> ``(B, mel_bins, T)``: ``torch.stft`` (periodic Hann, centred, reflect padding), ``|X|^2``, ``melW``."""
    w = wav.to(dtype)
    spec = torch.stft(w, cfg.n_fft, hop_length=cfg.hop, win_length=cfg.n_fft, window=torch.hann_window(cfg.n_fft, periodic=True, dtype=dtype, device=w.device),
                      center=True, pad_mode="reflect", return_complex=True)
    return torch.einsum("bkt,km->bmt", spec.real ** 2 + spec.imag ** 2, sd["audio_branch.logmel_extractor.melW"].to(w.device, dtype))


def image(mel: Tensor, sd: Dict[str, Tensor], cfg: ClapAudioConfig, dtype=torch.float64) -> Tensor:
    """mel power ``(B, mel_bins, T)`` -> ``(B, spec_size, spec_size)``: log, bn0 (inference form), ``reshape_wav2img``."""
    dev = mel.device
    x = 10.0 * torch.log10(torch.clamp(mel.to(dtype), min=cfg.amin))
    x = x.transpose(1, 2)[:, None]                                     # (B, 1, T, F) as upstream's extractor leaves it
    x = x.transpose(1, 3)                                              # bn0 normalises the mel bins
    p = lambda k: sd["audio_branch.bn0." + k].to(dev, dtype)
    x = F.batch_norm(x, p("running_mean"), p("running_var"), p("weight"), p("bias"), training=False, eps=cfg.bn_eps)
    x = x.transpose(1, 3)
    B, C, T, Fq = x.shape
    ratio = cfg.spec_size // cfg.mel_bins
    target = cfg.spec_size * ratio
    assert T <= target, "a longer spectrogram is refused"
    if T < target:
        x = F.interpolate(x, (target, Fq), mode="bicubic", align_corners=True)
    x = x.permute(0, 1, 3, 2).contiguous()                             # (B, 1, F, T)
    x = x.reshape(B, C, Fq, ratio, target // ratio).permute(0, 1, 3, 2, 4).contiguous()
    return x.reshape(B, ratio * Fq, target // ratio)


# ---- Swin -------------------------------------------------------------------------------------------------------------------------------------
def window_partition(x: Tensor, ws: int) -> Tensor:
    B, H, W, C = x.shape
    x = x.view(B, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def window_reverse(windows: Tensor, ws: int, H: int, W: int) -> Tensor:
    B = windows.shape[0] // (H * W // ws // ws)
    x = windows.view(B, H // ws, W // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def relative_position_index(ws: int) -> Tensor:
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def shift_mask(H: int, W: int, ws: int, shift: int, mask_value: float, dtype) -> Tensor:
    """``(nW, ws*ws, ws*ws)``: ``mask_value`` between tokens of different regions of the rolled frame, 0 elsewhere."""
    img = torch.zeros(1, H, W, 1, dtype=dtype)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    mw = window_partition(img, ws).view(-1, ws * ws)
    diff = mw[:, None, :] - mw[:, :, None]
    return torch.zeros_like(diff).masked_fill(diff != 0, mask_value)


def window_attention(qkv: Tensor, B: int, H: int, W: int, heads: int, shift: int, table: Tensor, mask_value: float, ws: int = 8) -> Tensor:
    """``qkv`` ``(B H W, 3 C)`` raster rows -> ``(B H W, C)``: roll, partition, attend, reverse, roll back."""
    C = qkv.shape[1] // 3
    D = C // heads
    x = qkv.view(B, H, W, 3 * C)
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    xw = window_partition(x, ws).view(-1, ws * ws, 3, heads, D).permute(2, 0, 3, 1, 4)       # (3, B nW, heads, N, D)
    q, k, v = xw[0] * D ** -0.5, xw[1], xw[2]
    attn = q @ k.transpose(-2, -1)
    bias = table[relative_position_index(ws).view(-1)].view(ws * ws, ws * ws, heads).permute(2, 0, 1)
    attn = attn + bias[None]
    if shift:
        m = shift_mask(H, W, ws, shift, mask_value, attn.dtype).to(attn.device)
        nW = m.shape[0]
        attn = (attn.view(B, nW, heads, ws * ws, ws * ws) + m[None, :, None]).view(-1, heads, ws * ws, ws * ws)
    out = (attn.softmax(-1) @ v).transpose(1, 2).reshape(-1, ws, ws, C)
    y = window_reverse(out, ws, H, W)
    if shift:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    return y.reshape(B * H * W, C)


def dense_window_attention(qkv: Tensor, B: int, H: int, W: int, heads: int, shift: int, table: Tensor, ws: int = 8) -> Tensor:
    """The same attention stated over the whole map: token pairs that do not share a (rolled-frame) window AND region are at -inf."""
    C = qkv.shape[1] // 3
    D = C // heads
    hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    hr, wr = (hh - shift) % H, (ww - shift) % W                          # where the roll puts a token
    win = (hr // ws) * (W // ws) + wr // ws
    reg = lambda p, n: (p >= n - ws).long() + (p >= n - shift).long() if shift else torch.zeros_like(p)
    grp = (win * 9 + reg(hr, H) * 3 + reg(wr, W)).flatten()
    dy, dx = (hr % ws).flatten(), (wr % ws).flatten()
    idx = (dy[:, None] - dy[None, :] + ws - 1) * (2 * ws - 1) + dx[:, None] - dx[None, :] + ws - 1
    same_window = win.flatten()[:, None] == win.flatten()[None, :]
    x = qkv.view(B, H * W, 3, heads, D).permute(2, 0, 3, 1, 4)
    attn = (x[0] * D ** -0.5) @ x[1].transpose(-2, -1)
    attn = attn + table[idx.clamp(0, (2 * ws - 1) ** 2 - 1)].permute(2, 0, 1)[None]
    attn = attn.masked_fill(~(same_window & (grp[:, None] == grp[None, :]))[None, None], float("-inf"))
    return (attn.softmax(-1) @ x[2]).transpose(1, 2).reshape(B * H * W, C)


def network(img: Tensor, sd: Dict[str, Tensor], cfg: ClapAudioConfig, dtype=torch.float64) -> Tuple[Tensor, List[Tensor]]:
    """``(B, S, S)`` image -> ``(embedding (B, joint_dim), taps)``: the token matrix ``(B tokens, C)`` behind the patch embed and behind every
    stage (after its PatchMerging)."""
    dev = img.device
    P = lambda k: sd[k].to(dev, dtype)
    a = "audio_branch."
    ws = cfg.window_size
    x = F.conv2d(img.to(dtype)[:, None], P(a + "patch_embed.proj.weight"), P(a + "patch_embed.proj.bias"), stride=4)
    B, E, H, W = x.shape
    x = x.flatten(2).transpose(1, 2)                                    # (B, H W, E), raster order
    x = F.layer_norm(x, (E,), P(a + "patch_embed.norm.weight"), P(a + "patch_embed.norm.bias"), cfg.ln_eps)
    taps = [x.reshape(B * H * W, E)]
    n = len(cfg.depths)
    for i in range(n):
        C = x.shape[-1]
        for j in range(cfg.depths[i]):
            p = f"{a}layers.{i}.blocks.{j}."
            window, shift = ws, (0 if j % 2 == 0 else ws // 2)
            if min(H, W) <= ws:
                window, shift = min(H, W), 0
            assert window == ws, "the restatement keeps the window at 8"
            h = F.layer_norm(x, (C,), P(p + "norm1.weight"), P(p + "norm1.bias"), cfg.ln_eps)
            qkv = F.linear(h, P(p + "attn.qkv.weight"), P(p + "attn.qkv.bias")).reshape(B * H * W, 3 * C)
            att = window_attention(qkv, B, H, W, cfg.num_heads[i], shift, P(p + "attn.relative_position_bias_table"), cfg.mask_value, ws)
            x = x + F.linear(att.view(B, H * W, C), P(p + "attn.proj.weight"), P(p + "attn.proj.bias"))
            h = F.layer_norm(x, (C,), P(p + "norm2.weight"), P(p + "norm2.bias"), cfg.ln_eps)
            h = F.gelu(F.linear(h, P(p + "mlp.fc1.weight"), P(p + "mlp.fc1.bias")))
            x = x + F.linear(h, P(p + "mlp.fc2.weight"), P(p + "mlp.fc2.bias"))
        if i + 1 < n:
            p = f"{a}layers.{i}.downsample."
            g = x.view(B, H, W, C)
            g = torch.cat([g[:, 0::2, 0::2], g[:, 1::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 1::2]], dim=-1).view(B, -1, 4 * C)
            g = F.layer_norm(g, (4 * C,), P(p + "norm.weight"), P(p + "norm.bias"), cfg.ln_eps)
            x = F.linear(g, P(p + "reduction.weight"))
            H, W = H // 2, W // 2
        taps.append(x.reshape(B * H * W, x.shape[-1]))
    C = x.shape[-1]
    x = F.layer_norm(x, (C,), P(a + "norm.weight"), P(a + "norm.bias"), cfg.ln_eps).mean(dim=1)
    x = F.linear(x, P("audio_projection.0.weight"), P("audio_projection.0.bias"))
    if cfg.projection_act == "relu":
        x = F.relu(x)
    x = F.linear(x, P("audio_projection.2.weight"), P("audio_projection.2.bias"))
    if cfg.normalize:
        x = F.normalize(x, dim=-1)
    return x, taps


def embed(wav: Tensor, sd: Dict[str, Tensor], cfg: ClapAudioConfig, dtype=torch.float64) -> Tensor:
    """waveform -> embedding, everything in ``dtype``."""
    return network(image(mel_power(fit_length(wav, cfg), sd, cfg, dtype), sd, cfg, dtype), sd, cfg, dtype)[0]


def chirp(cfg: ClapAudioConfig, L: int, B: int, seed: int) -> Tensor:
    """``(B, L)`` fp32: a rising chirp plus a noise floor, so that no frame is near-silent."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / cfg.sample_rate
    out = []
    for b in range(B):
        f0, f1 = 200.0 * (b + 1), 0.4 * cfg.sample_rate
        phase = 2 * math.pi * (f0 * t + 0.5 * (f1 - f0) * t ** 2 / max(float(t[-1]), 1e-9))
        out.append(0.5 * torch.sin(phase) + 0.02 * torch.randn(L, generator=g, dtype=torch.float64))
    return torch.stack(out).float()
