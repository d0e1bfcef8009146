"""fp64 CPU restatement of the CLAP text path (syncfusion_amd/clap_text.py, csrc/clap_text.hip, csrc/clap_text_engine.cpp), written the textbook
way in plain torch: ``F.embedding``, a cumulative sum for the pad-aware position ids, ``F.layer_norm``, a dense ``softmax`` over scores with
``-inf`` at padded keys, ``F.gelu``.  It imports nothing from ``syncfusion_amd``; tests/test_clap_text_cpu.py holds it to
``transformers.RobertaModel`` where that package is importable.

State dicts are upstream-named WITHOUT a prefix (``text_branch.*`` with ``transformers``' names below, ``text_projection.{0,2}.*``).
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor


@dataclass(frozen=True)
class TextConfig:
    """The fields of ``syncfusion_amd.ClapTextConfig`` the arithmetic depends on, under the same names (``ClapTextConfig(**asdict(cfg))``)."""
    vocab_size: int = 50265
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    intermediate: int = 3072
    max_positions: int = 514
    pad_id: int = 1
    bos_id: int = 0
    eos_id: int = 2
    unk_id: int = 3
    ln_eps: float = 1e-5
    max_length: int = 77
    pooling: str = "pooler"
    joint_dim: int = 512
    projection_act: str = "relu"
    normalize: bool = True


NARROW = TextConfig(vocab_size=300, hidden=128, layers=2, heads=2, intermediate=256, max_positions=80, joint_dim=64)
# full depth and width on a small vocabulary: seconds, not a 150 MB embedding table
WIDE = TextConfig(vocab_size=512)


# ---- weights ----------------------------------------------------------------------------------------------------------------------------------
def seeded_weights(cfg: TextConfig, seed: int) -> Dict[str, Tensor]:
    """An upstream-named fp32 state dict with non-trivial LayerNorm affines; q and k scaled so softmax rows are neither flat nor one-hot."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    sd: Dict[str, Tensor] = {}

    def linear(name, n_out, n_in, scale=1.0):
        sd[name + ".weight"] = scale * rn(n_out, n_in) / math.sqrt(n_in)
        sd[name + ".bias"] = 0.1 * rn(n_out)

    def norm(name, n):
        sd[name + ".weight"] = 1.0 + 0.2 * rn(n)
        sd[name + ".bias"] = 0.1 * rn(n)

    C = cfg.hidden
    e = "text_branch.embeddings."
    sd[e + "word_embeddings.weight"] = rn(cfg.vocab_size, C)
    sd[e + "position_embeddings.weight"] = rn(cfg.max_positions, C)
    sd[e + "token_type_embeddings.weight"] = rn(1, C)
    norm(e + "LayerNorm", C)
    for i in range(cfg.layers):
        p = f"text_branch.encoder.layer.{i}."
        linear(p + "attention.self.query", C, C, 2.0)
        linear(p + "attention.self.key", C, C, 2.0)
        linear(p + "attention.self.value", C, C)
        linear(p + "attention.output.dense", C, C)
        norm(p + "attention.output.LayerNorm", C)
        linear(p + "intermediate.dense", cfg.intermediate, C)
        linear(p + "output.dense", C, cfg.intermediate)
        norm(p + "output.LayerNorm", C)
    linear("text_branch.pooler.dense", C, C)
    linear("text_projection.0", cfg.joint_dim, C)
    linear("text_projection.2", cfg.joint_dim, cfg.joint_dim)
    return sd


def tokens(cfg: TextConfig, lengths, S: int, seed: int) -> Tuple[Tensor, Tensor]:
    """int64 ``(B, S)`` ids and mask: ``<s>``, ``lengths[b] - 2`` ordinary ids, ``</s>``, pads."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lengths), S), cfg.pad_id, dtype=torch.int64)
    mask = torch.zeros((len(lengths), S), dtype=torch.int64)
    for b, n in enumerate(lengths):
        assert 2 <= n <= S
        ids[b, 0], ids[b, n - 1] = cfg.bos_id, cfg.eos_id
        ids[b, 1:n - 1] = torch.randint(4, cfg.vocab_size, (n - 2,), generator=g)
        mask[b, :n] = 1
    return ids, mask


# ---- the pieces -------------------------------------------------------------------------------------------------------------------------------
def position_ids(ids: Tensor, pad_id: int) -> Tensor:
    real = (ids != pad_id).long()
    return torch.cumsum(real, dim=1) * real + pad_id


def embeddings(ids: Tensor, sd: Dict[str, Tensor], cfg: TextConfig, dtype=torch.float64) -> Tensor:
    """``(B, S)`` ids -> ``(B, S, C)``."""
    e = lambda k: sd["text_branch.embeddings." + k].to(dtype)
    x = F.embedding(ids.long(), e("word_embeddings.weight")) + e("token_type_embeddings.weight")[0] + \
        F.embedding(position_ids(ids.long(), cfg.pad_id), e("position_embeddings.weight"))
    return F.layer_norm(x, (cfg.hidden,), e("LayerNorm.weight"), e("LayerNorm.bias"), cfg.ln_eps)


def masked_attention(qkv: Tensor, mask: Tensor, heads: int) -> Tensor:
    """``(B, S, 3 C)`` rows ``[q | k | v]`` and a ``(B, S)`` mask -> ``(B, S, C)``: dense softmax attention with ``-inf`` at masked keys; masked
    keys' K / V rows are replaced by zeros first, so whatever they hold cannot reach the result."""
    B, S, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    keep = (mask != 0)
    q, k, v = (t.reshape(B, S, heads, D).transpose(1, 2) for t in qkv.split(C, dim=2))
    k = torch.where(keep[:, None, :, None], k, torch.zeros_like(k))
    v = torch.where(keep[:, None, :, None], v, torch.zeros_like(v))
    scores = q @ k.transpose(2, 3) / math.sqrt(D)
    scores = scores.masked_fill(~keep[:, None, None, :], float("-inf"))
    return (torch.softmax(scores, dim=-1) @ v).transpose(1, 2).reshape(B, S, C)


def layer(x: Tensor, mask: Tensor, sd: Dict[str, Tensor], i: int, cfg: TextConfig, dtype=torch.float64) -> Tensor:
    p = f"text_branch.encoder.layer.{i}."
    w = lambda k: sd[p + k].to(dtype)
    lin = lambda t, k: F.linear(t, w(k + ".weight"), w(k + ".bias"))
    qkv = torch.cat([lin(x, "attention.self.query"), lin(x, "attention.self.key"), lin(x, "attention.self.value")], dim=2)
    a = lin(masked_attention(qkv, mask, cfg.heads), "attention.output.dense") + x
    a = F.layer_norm(a, (cfg.hidden,), w("attention.output.LayerNorm.weight"), w("attention.output.LayerNorm.bias"), cfg.ln_eps)
    h = lin(F.gelu(lin(a, "intermediate.dense")), "output.dense") + a
    return F.layer_norm(h, (cfg.hidden,), w("output.LayerNorm.weight"), w("output.LayerNorm.bias"), cfg.ln_eps)


def encode(ids: Tensor, mask: Tensor, sd: Dict[str, Tensor], cfg: TextConfig, dtype=torch.float64) -> Tuple[Tensor, List[Tensor]]:
    """``(B, S)`` ids and mask -> the ``(B, joint_dim)`` embedding and the taps: the ``(B S, C)`` hidden state behind the embeddings and behind
    every layer, then the ``(B, C)`` pooled vector."""
    B, S = ids.shape
    x = embeddings(ids, sd, cfg, dtype)
    taps = [x.reshape(B * S, cfg.hidden)]
    for i in range(cfg.layers):
        x = layer(x, mask, sd, i, cfg, dtype)
        taps.append(x.reshape(B * S, cfg.hidden))
    w = lambda k: sd[k].to(dtype)
    pooled = x[:, 0]
    if cfg.pooling == "pooler":
        pooled = torch.tanh(F.linear(pooled, w("text_branch.pooler.dense.weight"), w("text_branch.pooler.dense.bias")))
    taps.append(pooled)
    h = F.linear(pooled, w("text_projection.0.weight"), w("text_projection.0.bias"))
    if cfg.projection_act == "relu":
        h = F.relu(h)
    out = F.linear(h, w("text_projection.2.weight"), w("text_projection.2.bias"))
    if cfg.normalize:
        out = F.normalize(out, dim=-1)
    return out, taps


# ---- tokenizer files for the tests -------------------------------------------------------------------------------------------------------------
SPECIALS = ["<s>", "<pad>", "</s>", "<unk>"]


def byte_symbols():
    """GPT-2's byte -> character table, written independently of the product's: printable Latin-1 bytes keep their character."""
    printable = [b for b in range(256) if 33 <= b <= 126 or 161 <= b <= 172 or 174 <= b <= 255]
    rest = [b for b in range(256) if b not in printable]
    table = {b: chr(b) for b in printable}
    table.update({b: chr(256 + i) for i, b in enumerate(rest)})
    return table


def write_tokenizer(path, merges, drop=()):
    """vocab.json / merges.txt: the specials at 0 .. 3, byte b at 4 + b, merge k at 260 + k; ``drop`` leaves symbols out of the vocabulary."""
    sym = byte_symbols()
    vocab = {s: i for i, s in enumerate(SPECIALS)}
    vocab.update({sym[b]: 4 + b for b in range(256)})
    for k, (a, b) in enumerate(merges):
        vocab[a + b] = 260 + k
    for s in drop:
        del vocab[s]
    path.mkdir(exist_ok=True)
    (path / "vocab.json").write_text(json.dumps(vocab, ensure_ascii=False), encoding="utf-8")
    (path / "merges.txt").write_text("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in merges), encoding="utf-8")
    return str(path / "vocab.json"), str(path / "merges.txt")


HAND_MERGES = [("a", "b"), ("ab", "c"), ("Ġ", "a"), ("Ġa", "b"), ("'", "s")]       # Ġ: the space byte's character
