"""CLAP text embedder on the device: the conditioning vector of text-prompted generation, ``clap_encode_text``.

``ClapEmbedder`` is ``laion_clap.CLAP_Module(enable_fusion=False, amodel='HTSAT-tiny', tmodel='roberta')`` as far as the reference uses
it: the audio side of ``ClapAudioEmbedder`` plus ``get_text_embedding(text, use_tensor=True)`` (main/module_diffusion.py:69-71, reached
with ``cond_text: True``, exp/evaluate_gh_gen_text.yaml:29).  Neither ``laion_clap`` nor ``transformers`` / ``tokenizers`` is needed: the
byte-level BPE runs on the host (``ClapTokenizer``), the embeddings, LayerNorms and the masked attention in ``csrc/clap_text.hip``, every
Linear on the library's fp32 implicit-GEMM launcher (``csrc/clap_text_engine.cpp``).  The vocabulary and merges files are the user's, like
the checkpoint: nothing is ever fetched.

Pinning status, in two parts.

PINNED on the CPU, wherever the packages are importable (tests/test_clap_text_cpu.py): the encoder arithmetic -- embeddings with pad-aware
position ids, post-LN layers, the key-padding mask, the pooler -- against ``transformers.RobertaModel`` through the fp64 restatement of
tests/clap_text_ref.py, and the tokenizer id for id against ``tokenizers.ByteLevelBPETokenizer``.

UNPINNED, [RECALLED] from ``laion_clap`` (absent from the reference tree and from this image); each is a field of ``ClapTextConfig``, so
whoever pins it later changes defaults, not code:

* the tokenizer call: ``max_length=77`` with ``padding="max_length"`` and truncation (``max_length``; the padding itself does not change the
  embedding, see below);
* ``pooler_output`` (``pooling="pooler"``) into ``text_projection = Linear(768, 512) - ReLU - Linear(512, 512)`` (``joint_dim``,
  ``projection_act``), then L2 normalisation (``normalize``);
* the key names ``text_branch.*`` (``transformers``' own names below that) and ``text_projection.{0,2}.*``;
* ``text_transform.*`` takes no part in ``get_text_embedding`` (dropped from a checkpoint, like ``audio_transform.*`` and ``logit_scale_*``).

Unless ``pad_to_max_length`` is set, the engine runs at ``S`` = the longest real length of the batch instead of 77 columns.  Padded keys carry
softmax weight exactly 0 in fp32 (``exp(-inf)``; the kernel skips them), position ids count real tokens only and only token 0 is pooled, so
the embedding is the same function of the text at ``B S`` rows instead of ``B 77``.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import unicodedata
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import nn

from . import _lib
from .clap import IGNORED_PARTS, AUDIO_PARTS, ClapAudioConfig, ClapAudioEmbedder

Tensor = torch.Tensor
TOKENIZER_ENV = "SYNCFUSION_ROBERTA_TOKENIZER"
HEAD_DIM = 64
MAX_TOKENS = 128
CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")       # in the pattern's order
# \s as the pre-tokeniser's regex engine sees it: Unicode White_Space
WHITE_SPACE = frozenset("\t\n\x0b\x0c\r \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a\u2028\u2029\u202f\u205f\u3000")


@dataclass
class ClapTextConfig:
    """Every recalled value of the text path (module docstring)."""
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
    pooling: str = "pooler"               # "pooler": tanh(Linear) of token 0 (``pooler_output``); "cls": token 0 as it is
    joint_dim: int = 512
    projection_act: str = "relu"          # between the two projection Linears: "relu" or "none"
    normalize: bool = True
    pad_to_max_length: bool = False       # run every batch at max_length columns, as upstream's padding="max_length" does
    seed: int = 2001                      # of the initialisation a missing checkpoint leaves in place

    def check(self) -> None:
        if self.hidden != HEAD_DIM * self.heads:
            raise ValueError(f"hidden {self.hidden} with {self.heads} heads: only head dim {HEAD_DIM} is built (hidden = {HEAD_DIM} heads)")
        if self.hidden > 1024:
            raise ValueError(f"hidden {self.hidden}: at most 1024 is built")
        if not 2 <= self.max_length <= MAX_TOKENS:
            raise ValueError(f"max_length {self.max_length}: 2 .. {MAX_TOKENS} tokens are built")
        if self.max_length + self.pad_id + 1 > self.max_positions:
            raise ValueError(f"max_length {self.max_length} needs position ids up to {self.max_length + self.pad_id}, the table has {self.max_positions} rows")
        if self.pooling not in ("pooler", "cls"):
            raise ValueError(f"pooling {self.pooling!r}: 'pooler' or 'cls'")
        if self.projection_act not in ("relu", "none"):
            raise ValueError(f"projection_act {self.projection_act!r}: 'relu' or 'none'")
        if self.layers < 1 or self.intermediate < 1 or not 1 <= self.joint_dim <= 1024:
            raise ValueError("layers, intermediate >= 1 and joint_dim in 1 .. 1024 expected")
        if not all(0 <= i < self.vocab_size for i in (self.pad_id, self.bos_id, self.eos_id, self.unk_id)):
            raise ValueError("pad_id, bos_id, eos_id and unk_id must lie inside the vocabulary")


# ---- the tokenizer ----------------------------------------------------------------------------------------------------------------------------
def bytes_to_unicode() -> Dict[int, str]:
    """GPT-2's table: every byte as one printable character (the printable Latin-1 bytes stand for themselves, the rest move to 256 + n)."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + list(range(ord("\xae"), ord("\xff") + 1))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + n)
            n += 1
    return table


def _kind(ch: str) -> int:
    """0 white space, 1 ``\\p{L}``, 2 ``\\p{N}``, 3 anything else."""
    if ch in WHITE_SPACE:
        return 0
    cat = unicodedata.category(ch)
    return 1 if cat[0] == "L" else 2 if cat[0] == "N" else 3


def pretokenize(text: str) -> List[str]:
    """The matches of ``'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+`` in order, by a scanner: no regex
    engine with Unicode classes is needed."""
    out: List[str] = []
    i, n = 0, len(text)
    while i < n:
        ch = text[i]
        if ch == "'":
            hit = next((c for c in CONTRACTIONS if text.startswith(c, i)), None)
            if hit:
                out.append(hit)
                i += len(hit)
                continue
        start = i + 1 if ch == " " and i + 1 < n and _kind(text[i + 1]) != 0 else i     # " ?": one plain space in front of a run
        kind = _kind(text[start])
        end = start + 1
        while end < n and _kind(text[end]) == kind:
            end += 1
        if kind == 0 and end < n and end - i >= 2:        # \s+(?!\S): the run gives its last character back to what follows
            end -= 1
        out.append(text[i:end])
        i = end
    return out


class ClapTokenizer:
    """RoBERTa's byte-level BPE on the host: ``vocab.json`` (symbol -> id) and ``merges.txt`` (one merge per line, best first)."""

    def __init__(self, vocab_file, merges_file, config: Optional[ClapTextConfig] = None):
        self.config = config or ClapTextConfig()
        for path in (vocab_file, merges_file):
            if not os.path.isfile(str(path)):
                raise FileNotFoundError(f"ClapTokenizer: {path} does not exist (RoBERTa's vocab.json and merges.txt are the user's files; nothing is downloaded)")
        with open(str(vocab_file), encoding="utf-8") as f:
            self.vocab: Dict[str, int] = json.load(f)
        self.ranks: Dict[Tuple[str, str], int] = {}
        with open(str(merges_file), encoding="utf-8") as f:
            for line in f.read().split("\n"):
                if line.startswith("#version") or not line.strip():
                    continue
                a, b = line.split(" ")[:2]
                self.ranks.setdefault((a, b), len(self.ranks))
        self.byte_symbol = bytes_to_unicode()
        self._cache: Dict[str, List[int]] = {}

    @classmethod
    def from_dir(cls, tokenizer_dir=None, config: Optional[ClapTextConfig] = None) -> "ClapTokenizer":
        """``tokenizer_dir`` or the directory ``SYNCFUSION_ROBERTA_TOKENIZER`` names, holding ``vocab.json`` and ``merges.txt``."""
        where = tokenizer_dir or os.environ.get(TOKENIZER_ENV)
        if not where:
            raise FileNotFoundError(f"ClapTokenizer: no tokenizer files: pass tokenizer_dir= or set {TOKENIZER_ENV} to the directory that holds "
                                    "RoBERTa's vocab.json and merges.txt (looked nowhere else; nothing is downloaded)")
        return cls(os.path.join(str(where), "vocab.json"), os.path.join(str(where), "merges.txt"), config)

    def bpe(self, symbols: List[str]) -> List[str]:
        """Merges applied lowest rank first (the leftmost occurrence of the best pair, then every occurrence of that pair)."""
        word = list(symbols)
        while len(word) > 1:
            ranked = [(self.ranks[pair], i) for i, pair in enumerate(zip(word, word[1:])) if pair in self.ranks]
            if not ranked:
                break
            first = min(ranked)[1]
            a, b = word[first], word[first + 1]
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                    merged.append(a + b)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = merged
        return word

    def encode(self, text: str) -> List[int]:
        """The ids of ``text`` without the special tokens."""
        ids: List[int] = []
        for piece in pretokenize(text):
            got = self._cache.get(piece)
            if got is None:
                symbols = [self.byte_symbol[b] for b in piece.encode("utf-8")]
                got = [self.vocab.get(s, self.config.unk_id) for s in self.bpe(symbols)]
                self._cache[piece] = got
            ids += got
        return ids

    def __call__(self, texts: Union[str, Sequence[str]], max_length: Optional[int] = None) -> Tuple[Tensor, Tensor]:
        """CPU int32 ``(B, max_length)`` ``ids`` and ``mask``: ``<s> ... </s>``, the first ``max_length - 2`` tokens kept, right-padded with
        ``pad_id``; ``mask`` is 1 on real tokens."""
        cfg = self.config
        texts = [texts] if isinstance(texts, str) else list(texts)
        L = int(cfg.max_length if max_length is None else max_length)
        if L < 2:
            raise ValueError("max_length must leave room for <s> and </s>")
        ids = torch.full((len(texts), L), cfg.pad_id, dtype=torch.int32)
        mask = torch.zeros((len(texts), L), dtype=torch.int32)
        for r, t in enumerate(texts):
            if not isinstance(t, str):
                raise TypeError(f"ClapTokenizer: a str expected, got {type(t).__name__}")
            row = [cfg.bos_id] + self.encode(t)[:L - 2] + [cfg.eos_id]
            ids[r, :len(row)] = torch.tensor(row, dtype=torch.int32)
            mask[r, :len(row)] = 1
        return ids, mask


# ---- the module tree: transformers' names -----------------------------------------------------------------------------------------------------
class _Embeddings(nn.Module):
    def __init__(self, cfg: ClapTextConfig):
        super().__init__()
        self.word_embeddings = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.position_embeddings = nn.Embedding(cfg.max_positions, cfg.hidden)
        self.token_type_embeddings = nn.Embedding(1, cfg.hidden)
        self.LayerNorm = nn.LayerNorm(cfg.hidden, eps=cfg.ln_eps)


class _SelfAttention(nn.Module):
    def __init__(self, C: int):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C)


class _Output(nn.Module):
    def __init__(self, n_in: int, C: int, eps: float):
        super().__init__()
        self.dense = nn.Linear(n_in, C)
        self.LayerNorm = nn.LayerNorm(C, eps=eps)


class _Dense(nn.Module):
    def __init__(self, n_in: int, n_out: int):
        super().__init__()
        self.dense = nn.Linear(n_in, n_out)


class _Attention(nn.Module):
    def __init__(self, cfg: ClapTextConfig):
        super().__init__()
        self.add_module("self", _SelfAttention(cfg.hidden))
        self.output = _Output(cfg.hidden, cfg.hidden, cfg.ln_eps)


class _Layer(nn.Module):
    def __init__(self, cfg: ClapTextConfig):
        super().__init__()
        self.attention = _Attention(cfg)
        self.intermediate = _Dense(cfg.hidden, cfg.intermediate)
        self.output = _Output(cfg.intermediate, cfg.hidden, cfg.ln_eps)


class _Encoder(nn.Module):
    def __init__(self, cfg: ClapTextConfig):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(cfg) for _ in range(cfg.layers)])


class _Roberta(nn.Module):
    def __init__(self, cfg: ClapTextConfig):
        super().__init__()
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.pooler = _Dense(cfg.hidden, cfg.hidden)


class ClapEmbedder(ClapAudioEmbedder):
    """``laion_clap.CLAP_Module`` as the reference uses it, both sides: ``get_audio_embedding_from_data`` (inherited) and
    ``get_text_embedding``.  Frozen.  Each side has an engine of its own that copies the weights when it is built; every weight load and every
    ``.to()`` drops both."""

    PARTS = AUDIO_PARTS + ("text_branch.", "text_projection.")
    IGNORED = IGNORED_PARTS + ("text_branch.embeddings.position_ids", "text_branch.embeddings.token_type_ids")

    def __init__(self, config: Optional[ClapAudioConfig] = None, text_config: Optional[ClapTextConfig] = None, tokenizer_dir=None,
                 enable_fusion: bool = False, amodel: str = "HTSAT-tiny", tmodel: str = "roberta", **_ignored):
        super().__init__(config, enable_fusion=enable_fusion, amodel=amodel)
        if tmodel != "roberta":
            raise ValueError(f"ClapEmbedder: tmodel {tmodel!r} is not built, only 'roberta'")
        self.text_config = tc = ClapTextConfig() if text_config is None else text_config
        tc.check()
        self.tokenizer_dir = tokenizer_dir
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(tc.seed)
            self.model.text_branch = _Roberta(tc)
            self.model.text_projection = nn.Sequential(nn.Linear(tc.hidden, tc.joint_dim), nn.ReLU(), nn.Linear(tc.joint_dim, tc.joint_dim))
        for p in self.parameters():
            p.requires_grad = False
        self._tokenizer: Optional[ClapTokenizer] = None
        self._text_engine: Optional[int] = None
        self._text_engine_device: Optional[str] = None

    # -- weights
    def _release_text(self) -> None:
        d = self.__dict__
        h = d.get("_text_engine")
        d["_text_engine"], d["_text_engine_device"] = None, None
        if not h:
            return
        try:
            _lib.load().sf_clap_text_destroy(h)
        except Exception:               # interpreter shutdown
            pass

    def invalidate(self) -> None:
        super().invalidate()
        self._release_text()

    def text_engine_weights(self) -> List[Tuple[str, Tensor]]:
        """The named fp32 tensors ``sf_clap_text_create`` reads; query, key and value of a layer concatenated into one ``(3 C, C)`` matrix."""
        tb = self.model.text_branch
        d = lambda t: t.detach().float()
        e = tb.embeddings
        out: List[Tuple[str, Tensor]] = [("emb.word", d(e.word_embeddings.weight)), ("emb.pos", d(e.position_embeddings.weight)),
                                         ("emb.type", d(e.token_type_embeddings.weight)[0]), ("emb.g", d(e.LayerNorm.weight)),
                                         ("emb.beta", d(e.LayerNorm.bias))]
        for i, layer in enumerate(tb.encoder.layer):
            p = f"l{i}."
            att = getattr(layer.attention, "self")
            out += [(p + "qkv.w", torch.cat([d(att.query.weight), d(att.key.weight), d(att.value.weight)])),
                    (p + "qkv.b", torch.cat([d(att.query.bias), d(att.key.bias), d(att.value.bias)])),
                    (p + "ao.w", d(layer.attention.output.dense.weight)), (p + "ao.b", d(layer.attention.output.dense.bias)),
                    (p + "ln1.g", d(layer.attention.output.LayerNorm.weight)), (p + "ln1.beta", d(layer.attention.output.LayerNorm.bias)),
                    (p + "fc1.w", d(layer.intermediate.dense.weight)), (p + "fc1.b", d(layer.intermediate.dense.bias)),
                    (p + "fc2.w", d(layer.output.dense.weight)), (p + "fc2.b", d(layer.output.dense.bias)),
                    (p + "ln2.g", d(layer.output.LayerNorm.weight)), (p + "ln2.beta", d(layer.output.LayerNorm.bias))]
        pr = self.model.text_projection
        out += [("pool.w", d(tb.pooler.dense.weight)), ("pool.b", d(tb.pooler.dense.bias)), ("proj0.w", d(pr[0].weight)), ("proj0.b", d(pr[0].bias)),
                ("proj2.w", d(pr[2].weight)), ("proj2.b", d(pr[2].bias))]
        return [(k, v.contiguous()) for k, v in out]

    def text_engine_config(self) -> "_lib.ClapTextEngineConfig":
        tc = self.text_config
        c = _lib.ClapTextEngineConfig()
        c.vocab_size, c.hidden, c.layers, c.heads, c.intermediate = tc.vocab_size, tc.hidden, tc.layers, tc.heads, tc.intermediate
        c.max_positions, c.pad_id, c.max_length, c.joint_dim, c.ln_eps = tc.max_positions, tc.pad_id, tc.max_length, tc.joint_dim, tc.ln_eps
        c.pooling, c.projection_relu, c.normalize = int(tc.pooling == "cls"), int(tc.projection_act == "relu"), int(bool(tc.normalize))
        return c

    def describe_gemms(self, B: int, S: Optional[int] = None) -> str:
        """With ``S``: one line per GEMM of a text layer at ``B`` texts of ``S`` columns with the kernel family the library's dispatcher gives
        it (host only).  Without: the audio network's at batch ``B``."""
        if S is None:
            return super().describe_gemms(B)
        buf = C.create_string_buffer(1 << 12)
        cfg = self.text_engine_config()
        _lib.check(_lib.load().sf_clap_text_describe(C.byref(cfg), int(B), int(S), buf, len(buf)), "sf_clap_text_describe")
        return buf.value.decode()

    # -- device pieces
    def _text_engine_for(self, device: torch.device) -> int:
        if self._text_engine is None or self._text_engine_device != str(device):
            self._release_text()
            table = _lib.TensorTable(self.text_engine_weights(), device)
            cfg = self.text_engine_config()
            h = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(_lib.load().sf_clap_text_create(C.byref(cfg), table.array, table.n, _lib.stream_ptr(device), C.byref(h)),
                           "sf_clap_text_create")
            self._text_engine, self._text_engine_device = h.value, str(device)
        return self._text_engine

    def embed_device(self, ids: Tensor, mask: Tensor, taps: bool = False):
        """The device part of ``embed_tokens``: int32 ``(B, S)`` device ``ids`` and ``mask`` (already validated) -> ``(B, joint_dim)``; no
        synchronisation, so after one warm-up call it can be captured in a ``torch.cuda.graph``."""
        _lib.require_gpu_tensor(ids, "ClapEmbedder.embed_device")
        _lib.require_gpu_tensor(mask, "ClapEmbedder.embed_device")
        tc = self.text_config
        if ids.dtype != torch.int32 or mask.dtype != torch.int32 or ids.dim() != 2 or ids.shape != mask.shape or not (ids.is_contiguous() and mask.is_contiguous()):
            raise ValueError("ClapEmbedder.embed_device: contiguous int32 (B, S) ids and mask expected")
        dev, (B, S) = ids.device, ids.shape
        lib, eng = _lib.load(), self._text_engine_for(dev)
        need = int(lib.sf_clap_text_workspace_bytes(eng, B, S))
        if need < 0:
            raise ValueError(f"ClapEmbedder: {B} texts of {S} columns out of range (at most {tc.max_length} columns)")
        out = torch.empty((B, tc.joint_dim), dtype=torch.float32, device=dev)
        tapped = [torch.empty((B * S, tc.hidden), dtype=torch.float32, device=dev) for _ in range(tc.layers + 1)] if taps else []
        if taps:
            tapped.append(torch.empty((B, tc.hidden), dtype=torch.float32, device=dev))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sf_clap_text_forward(eng, ids.data_ptr(), mask.data_ptr(), B, S, out.data_ptr(), _lib.ptr_array(tapped) if taps else None,
                                                ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "sf_clap_text_forward")
        return (out, tapped) if taps else out

    def embed_tokens(self, ids: Tensor, mask: Tensor, taps: bool = False):
        """CPU integer ``(B, S)`` ``ids`` and ``mask`` (non-zero on real tokens, every row starting with one) -> ``(B, joint_dim)`` embeddings on
        the device of the parameters; with ``taps`` also the hidden state behind the embeddings and behind every layer (``(B S', hidden)``
        each, ``S'`` the columns the engine ran at) and the pooled ``(B, hidden)`` vector (tests)."""
        dev = next(self.parameters()).device
        _lib.require_gpu_tensor(torch.empty(0, device=dev), "ClapEmbedder.embed_tokens")
        tc = self.text_config
        for name, t in (("ids", ids), ("mask", mask)):
            if not isinstance(t, Tensor) or t.is_cuda or t.is_floating_point() or t.dim() != 2:
                raise ValueError(f"ClapEmbedder.embed_tokens: {name}: a CPU integer (B, S) tensor expected")
        if ids.shape != mask.shape or ids.shape[0] < 1 or not 1 <= ids.shape[1] <= tc.max_length:
            raise ValueError(f"ClapEmbedder.embed_tokens: ids and mask of one shape (B >= 1, 1 .. {tc.max_length} columns) expected, got "
                             f"{tuple(ids.shape)} and {tuple(mask.shape)}")
        if int(ids.min()) < 0 or int(ids.max()) >= tc.vocab_size:
            raise ValueError(f"ClapEmbedder.embed_tokens: ids outside 0 .. {tc.vocab_size - 1}")
        real = mask != 0
        if not bool(real[:, 0].all()):
            raise ValueError("ClapEmbedder.embed_tokens: every row must start with a real token")
        ids32, mask32 = ids.to(torch.int32), real.to(torch.int32)
        cols = torch.arange(1, ids.shape[1] + 1)
        S = tc.max_length if tc.pad_to_max_length else int((real * cols).max())      # the longest real length: nothing behind it but pads
        if S < ids.shape[1]:
            ids32, mask32 = ids32[:, :S], mask32[:, :S]
        elif S > ids.shape[1]:
            grow = S - ids.shape[1]
            ids32 = torch.cat([ids32, torch.full((ids.shape[0], grow), tc.pad_id, dtype=torch.int32)], dim=1)
            mask32 = torch.cat([mask32, torch.zeros((ids.shape[0], grow), dtype=torch.int32)], dim=1)
        return self.embed_device(ids32.contiguous().to(dev), mask32.contiguous().to(dev), taps=taps)

    # -- the member the reference touches
    def tokenizer(self) -> ClapTokenizer:
        if self._tokenizer is None:
            self._tokenizer = ClapTokenizer.from_dir(self.tokenizer_dir, self.text_config)
        return self._tokenizer

    @torch.no_grad()
    def get_text_embedding(self, text, use_tensor: bool = True):
        """A ``str`` or a list of ``str`` -> ``(B, joint_dim)`` fp32 embeddings (unit norm with ``normalize``) on the device of the parameters;
        ``use_tensor=False`` gives numpy.  Tokenised on the host."""
        _lib.require_gpu_tensor(next(self.parameters()), "ClapEmbedder.get_text_embedding")
        texts = [text] if isinstance(text, str) else list(text)
        if not texts:
            raise ValueError("ClapEmbedder.get_text_embedding: no text")
        ids, mask = self.tokenizer()(texts)
        out = self.embed_tokens(ids, mask)
        return out if use_tensor else out.cpu().numpy()
