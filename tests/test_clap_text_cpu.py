"""CLAP text embedder, the parts that need no device: configuration refusals, the byte-level BPE tokenizer (by hand and, where importable, id
for id against ``tokenizers``), the fp64 restatement of tests/clap_text_ref.py against ``transformers.RobertaModel`` (where importable), the
state-dict handling, loading through ``Model.load_state_dict``, the C ABI's declarations and refusals, the GEMM dispatch of every shape the
GPU tests run, and the restatement's own check that trimming the padding does not change the embedding.  tests/test_gpu_clap_text.py holds
the kernels and the engine to the restatement."""
import collections
import ctypes as C
import os
import re
import warnings
from dataclasses import asdict, replace

import pytest
import torch

import clap_ref
import clap_text_ref
from clap_text_ref import HAND_MERGES, NARROW, byte_symbols, write_tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_SYMBOLS = ("sf_op_text_embed", "sf_op_layernorm_affine", "sf_op_masked_attention", "sf_clap_text_create", "sf_clap_text_destroy",
                "sf_clap_text_workspace_bytes", "sf_clap_text_forward", "sf_clap_text_describe")
AWKWARD = ["Hello world", "it's we're they'd I'VE don't 'll", "x² + y³ = ½ of 1234567 items", "  leading, trailing  ", "a  b   c    d",
           "tab\tseparated\t\tvalues\nnew\n\nlines \n", "café déjà vu naïve", "日本語のテキスト 中文", "🎉 party 🎶!!", "", " ", "...!?'s", "a", "the dog barks, the cat   sleeps"]


def text_config(cfg=NARROW, **changes):
    from syncfusion_amd.clap_text import ClapTextConfig

    return replace(ClapTextConfig(**asdict(cfg)), **changes)


def embedder(cfg=NARROW, seed=None, **kwargs):
    from syncfusion_amd.clap_text import ClapEmbedder

    m = ClapEmbedder(clap_ref.NARROW, text_config(cfg), **kwargs)
    if seed is not None:
        m.load_state_dict(both_halves(cfg, seed))
    return m


def both_halves(cfg, seed):
    return {**clap_ref.seeded_weights(clap_ref.NARROW, seed), **clap_text_ref.seeded_weights(cfg, seed)}


# ---- configuration ----------------------------------------------------------------------------------------------------------------------------
def test_config_refusals_and_the_default_size():
    from syncfusion_amd.clap_text import ClapEmbedder, ClapTextConfig

    for bad, match in ((dict(hidden=768, heads=8), "head dim"), (dict(max_length=129), "max_length"), (dict(max_length=77, max_positions=78), "position"),
                       (dict(pooling="mean"), "pooling"), (dict(projection_act="gelu"), "projection_act")):
        with pytest.raises(ValueError, match=match):
            replace(ClapTextConfig(), **bad).check()
    ClapTextConfig(max_length=128, max_positions=130).check()                # the largest the kernels take
    with pytest.raises(ValueError, match="max_length"):
        ClapEmbedder(clap_ref.NARROW, replace(ClapTextConfig(), max_length=512))
    with pytest.raises(ValueError, match="bert"):
        ClapEmbedder(clap_ref.NARROW, text_config(), tmodel="bert")
    with pytest.raises(ValueError, match="enable_fusion"):
        ClapEmbedder(clap_ref.NARROW, text_config(), enable_fusion=True)
    assert asdict(ClapTextConfig()).items() >= asdict(clap_text_ref.TextConfig()).items()
    m = ClapEmbedder(clap_ref.NARROW, None, enable_fusion=False, amodel="HTSAT-tiny", tmodel="roberta", device="cpu", some_upstream_kwarg=1)
    n = sum(p.numel() for k, p in m.named_parameters() if k.startswith(("model.text_branch.", "model.text_projection.")))
    assert 124e6 < n < 126e6, n
    assert all(not p.requires_grad for p in m.parameters())
    from syncfusion_amd._lib import SyncFusionAmdError

    with pytest.raises(SyncFusionAmdError, match="no CPU execution path"):
        m.get_text_embedding(["a dog barks"], use_tensor=True)
    with pytest.raises(SyncFusionAmdError, match="no CPU execution path"):
        m.embed_tokens(torch.tensor([[0, 5, 2]]), torch.tensor([[1, 1, 1]]))


def test_target_path_instantiates_and_the_default_map_stays():
    from syncfusion_amd import ClapEmbedder, instantiate
    from syncfusion_amd.config import TARGET_MAP

    m = instantiate({"_target_": "syncfusion_amd.clap_text.ClapEmbedder", "enable_fusion": False, "amodel": "HTSAT-tiny", "tmodel": "roberta",
                     "config": clap_ref.NARROW, "text_config": text_config()})
    assert isinstance(m, ClapEmbedder) and m.text_config.hidden == 128
    assert TARGET_MAP["laion_clap.CLAP_Module"] == "syncfusion_amd.module.RandomEmbedder"


# ---- the tokenizer ----------------------------------------------------------------------------------------------------------------------------
def test_tokenizer_by_hand(tmp_path):
    from syncfusion_amd.clap_text import ClapTokenizer

    tok = ClapTokenizer(*write_tokenizer(tmp_path / "t", HAND_MERGES))
    a, b, c, sp = 4 + ord("a"), 4 + ord("b"), 4 + ord("c"), 4 + ord(" ")
    assert tok.encode("abc") == [261]                                   # a b -> ab, ab c -> abc
    assert tok.encode("cab") == [c, 260]                                # (c, ab) is no merge
    assert tok.encode("ab ab") == [260, sp, 260]                        # " ab": a b (rank 0) goes before Ġ a (rank 2); (Ġ, ab) is no merge
    assert tok.encode(" a") == [262] and tok.encode(" ac") == [262, c]
    assert tok.encode("a's") == [a, 264] and tok.encode("a 's") == [a, sp, 4 + ord("'"), 4 + ord("s")]   # "'s" is a piece; " '" + "s" are two
    assert tok.encode("a  b") == [a, sp, sp, b]                         # "a", " ", " b"
    assert tok.encode("é") == [4 + 0xC3, 4 + 0xA9]
    ids, mask = tok(["abc", "", "abc abc abc abc"], max_length=6)
    assert ids.dtype == torch.int32 and mask.dtype == torch.int32 and not ids.is_cuda
    assert ids.tolist() == [[0, 261, 2, 1, 1, 1], [0, 2, 1, 1, 1, 1], [0, 261, sp, 261, sp, 2]]     # truncated to the first max_length - 2 tokens
    assert mask.tolist() == [[1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]]
    assert tok("abc")[0].shape == (1, 77)                               # a str is one text; the default length is the config's
    holes = ClapTokenizer(*write_tokenizer(tmp_path / "holes", HAND_MERGES, drop=("z",)))
    assert holes.encode("az") == [a, 3]                                 # a symbol outside the vocabulary: unk_id


def test_tokenizer_files_are_the_users(tmp_path, monkeypatch):
    from syncfusion_amd.clap_text import TOKENIZER_ENV, ClapTokenizer

    monkeypatch.delenv(TOKENIZER_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        ClapTokenizer.from_dir(None)
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / "nowhere"))):
        ClapTokenizer.from_dir(str(tmp_path / "nowhere"))
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        ClapTokenizer(str(tmp_path / "vocab.json"), str(tmp_path / "merges.txt"))
    write_tokenizer(tmp_path / "t", HAND_MERGES)
    (tmp_path / "t" / "merges.txt").unlink()
    with pytest.raises(FileNotFoundError, match="merges.txt"):
        ClapTokenizer.from_dir(str(tmp_path / "t"))
    write_tokenizer(tmp_path / "t", HAND_MERGES)
    monkeypatch.setenv(TOKENIZER_ENV, str(tmp_path / "t"))
    assert ClapTokenizer.from_dir(None).encode("abc") == [261]
    assert embedder(tokenizer_dir=str(tmp_path / "t")).tokenizer().encode("abc") == [261]


def learned_merges(corpus, n):
    """A small BPE training run over byte symbols (most frequent pair first, ties by first appearance), pieces split at spaces."""
    sym = byte_symbols()
    words = collections.Counter()
    for line in corpus:
        for i, w in enumerate(line.split(" ")):
            words[tuple(sym[b] for b in ((" " if i else "") + w).encode("utf-8"))] += 1
    merges = []
    for _ in range(n):
        pairs = collections.Counter()
        for w, k in words.items():
            for p in zip(w, w[1:]):
                pairs[p] += k
        if not pairs:
            break
        (a, b), _count = max(pairs.items(), key=lambda kv: kv[1])
        merges.append((a, b))
        merged = collections.Counter()
        for w, k in words.items():
            out, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and w[i] == a and w[i + 1] == b:
                    out.append(a + b)
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            merged[tuple(out)] += k
        words = merged
    return merges


def test_tokenizer_equals_the_tokenizers_package(tmp_path):
    tokenizers = pytest.importorskip("tokenizers")
    from syncfusion_amd.clap_text import ClapTokenizer

    merges = learned_merges(AWKWARD + ["the cat and the dog and the hat", "hello hello world world's"], 120)
    assert len(merges) > 60
    files = write_tokenizer(tmp_path / "t", merges)
    theirs = tokenizers.ByteLevelBPETokenizer(*files, add_prefix_space=False)
    ours = ClapTokenizer(*files)
    for text in AWKWARD + [" ".join(AWKWARD), "".join(AWKWARD)]:
        assert ours.encode(text) == theirs.encode(text).ids, repr(text)


def test_scanner_equals_the_pattern():
    regex = pytest.importorskip("regex")
    from syncfusion_amd.clap_text import pretokenize

    pat = regex.compile(r"""'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+""")
    for text in AWKWARD + [" ".join(AWKWARD), "a b　c  d", "'s's ' s'", "\t a", " \tb", "x \n"]:
        assert pretokenize(text) == pat.findall(text), repr(text)
        assert "".join(pretokenize(text)) == text


# ---- the restatement against transformers -------------------------------------------------------------------------------------------------------
def padded_batch(cfg, seed=3):
    """Rows of 12, 2 and 7 real tokens in 12 columns: one without a pad, one with two real tokens."""
    return clap_text_ref.tokens(cfg, (12, 2, 7), 12, seed)


def test_restatement_equals_transformers_roberta():
    transformers = pytest.importorskip("transformers")
    cfg = NARROW
    sd = clap_text_ref.seeded_weights(cfg, 11)
    hf_cfg = transformers.RobertaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                                        intermediate_size=cfg.intermediate, max_position_embeddings=cfg.max_positions, type_vocab_size=1,
                                        pad_token_id=cfg.pad_id, bos_token_id=cfg.bos_id, eos_token_id=cfg.eos_id, layer_norm_eps=cfg.ln_eps,
                                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, hidden_act="gelu")
    model = transformers.RobertaModel(hf_cfg, add_pooling_layer=True).double().eval()
    state = {k[len("text_branch."):]: v.double() for k, v in sd.items() if k.startswith("text_branch.")}
    result = model.load_state_dict(state, strict=False)
    assert not result.unexpected_keys and all(k.endswith(("position_ids", "token_type_ids")) for k in result.missing_keys), result
    ids, mask = padded_batch(cfg)
    out = model(input_ids=ids, attention_mask=mask)
    _, taps = clap_text_ref.encode(ids, mask, sd, cfg)
    hidden = taps[-2].reshape(3, 12, cfg.hidden)
    err_h = float((out.last_hidden_state - hidden).abs().max())
    err_p = float((out.pooler_output - taps[-1]).abs().max())
    print(f"restatement vs transformers {transformers.__version__}: last hidden state {err_h:.2e}, pooler output {err_p:.2e}")
    assert err_h < 1e-12 and err_p < 1e-12
    assert float(hidden.abs().max()) > 1.0


def test_trimming_the_padding_does_not_change_the_embedding():
    cfg = NARROW
    sd = clap_text_ref.seeded_weights(cfg, 11)
    ids, mask = clap_text_ref.tokens(cfg, (9, 2, 5), cfg.max_length, 4)
    full, taps_full = clap_text_ref.encode(ids, mask, sd, cfg)
    trimmed, taps = clap_text_ref.encode(ids[:, :9], mask[:, :9], sd, cfg)
    assert float((full - trimmed).abs().max()) < 1e-12
    last = taps_full[-2].reshape(3, cfg.max_length, cfg.hidden)[:, :9]
    assert float((last - taps[-2].reshape(3, 9, cfg.hidden)).abs().max()) < 1e-12     # every kept row, padded query rows included
    alone, _ = clap_text_ref.encode(ids[1:2, :2], mask[1:2, :2], sd, cfg)
    assert float((alone - full[1:2]).abs().max()) < 1e-12
    for c in (replace(cfg, pooling="cls"), replace(cfg, projection_act="none", normalize=False)):
        assert float((clap_text_ref.encode(ids, mask, sd, c)[0] - full).abs().max()) > 1e-3


# ---- keys -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["", "module.", "model.", "clap.model."])
def test_state_dict_loads_under_every_prefix_and_drops_what_is_not_read(prefix, tmp_path):
    sd = both_halves(NARROW, 5)
    state = {prefix + k: v for k, v in sd.items()}
    junk = {"logit_scale_a": torch.zeros(()), "logit_scale_t": torch.zeros(()), "text_transform.sequential.0.weight": torch.zeros(2, 2),
            "text_transform.sequential.0.bias": torch.zeros(2), "audio_transform.sequential.0.weight": torch.zeros(2, 2),
            "text_branch.embeddings.position_ids": torch.arange(80)[None], "text_branch.embeddings.token_type_ids": torch.zeros(1, 80, dtype=torch.long),
            "audio_branch.tscam_conv.weight": torch.zeros(5, 5), "audio_branch.head.weight": torch.zeros(7, 7)}
    state.update({prefix + k: v for k, v in junk.items()})
    m = embedder()
    m.load_state_dict(state)
    own = m.state_dict()
    assert len(own) == len(sd) + 1                                         # (+ bn0.num_batches_tracked)
    for k, v in sd.items():
        assert torch.equal(own["model." + k], v), k
    for i, payload in enumerate((state, {"state_dict": state, "epoch": 3})):
        path = tmp_path / f"ckpt{i}.pt"
        torch.save(payload, path)
        m2 = embedder()
        m2.load_ckpt(str(path))
        assert all(torch.equal(m2.state_dict()["model." + k], v) for k, v in sd.items())


def test_missing_and_mis_shaped_text_keys_are_named():
    sd = both_halves(NARROW, 5)
    key = "text_branch.encoder.layer.1.attention.self.key.weight"
    with pytest.raises(KeyError, match=re.escape(key)):
        embedder().load_state_dict({k: v for k, v in sd.items() if k != key})
    bad = dict(sd)
    bad["text_projection.2.bias"] = torch.zeros(3)
    with pytest.raises(ValueError, match=re.escape("text_projection.2.bias")):
        embedder().load_state_dict(bad)
    with pytest.raises(KeyError, match="text_branch"):
        embedder().load_state_dict(clap_ref.seeded_weights(clap_ref.NARROW, 5))       # a checkpoint with the audio half only
    with pytest.raises(KeyError, match="audio_branch"):
        embedder().load_state_dict(clap_text_ref.seeded_weights(NARROW, 5))
    from syncfusion_amd.clap import ClapAudioEmbedder

    audio_only = ClapAudioEmbedder(clap_ref.NARROW)
    audio_only.load_state_dict(sd)                                          # the audio class still drops the text half
    assert not any("text_" in k for k in audio_only.state_dict())


def test_every_weight_load_invalidates_both_engines():
    m = embedder()
    sd = both_halves(NARROW, 6)
    for load in (lambda: m.load_state_dict(sd), lambda: torch.nn.Module.load_state_dict(m, m.state_dict()), lambda: m.float(), lambda: m.invalidate()):
        m.__dict__["_engine"], m.__dict__["_text_engine"], m.__dict__["_scale_shift"] = 0, 0, ("stale", "stale")   # (0: nothing to destroy)
        load()
        assert m._engine is None and m._text_engine is None and m._scale_shift is None


def test_engine_weights_concatenate_query_key_value():
    m = embedder(seed=5)
    sd = clap_text_ref.seeded_weights(NARROW, 5)
    w = dict(m.text_engine_weights())
    p = "text_branch.encoder.layer.1.attention.self."
    assert torch.equal(w["l1.qkv.w"], torch.cat([sd[p + "query.weight"], sd[p + "key.weight"], sd[p + "value.weight"]]))
    assert torch.equal(w["l1.qkv.b"], torch.cat([sd[p + "query.bias"], sd[p + "key.bias"], sd[p + "value.bias"]]))
    assert w["emb.type"].shape == (128,) and w["emb.pos"].shape == (80, 128) and w["pool.w"].shape == (128, 128)
    assert len(w) == 5 + 12 * NARROW.layers + 6 and all(t.dtype == torch.float32 and t.is_contiguous() for t in w.values())


def test_model_load_state_dict_reaches_both_halves():
    import functools

    from helpers import SMALL_ENCODER, SMALL_UNET
    from syncfusion_amd import DiffusionModel, Encoder1d, Model, UNetV0, VDiffusion, VSampler

    net = DiffusionModel(net_t=functools.partial(UNetV0, seed=1), diffusion_t=VDiffusion, sampler_t=VSampler, use_embedding_cfg=True, **SMALL_UNET)
    emb = embedder(seed=5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = Model(lr=1e-4, lr_beta1=0.9, lr_beta2=0.99, lr_eps=1e-8, lr_weight_decay=0.0, model=net, onsets_encoder=Encoder1d(seed=1, **SMALL_ENCODER),
                      embedder=emb, embedder_checkpoint=None)
    assert all(not p.requires_grad for p in model.clap.parameters())
    state = {k: v.clone() for k, v in model.state_dict().items()}
    rest_before = {k: v.clone() for k, v in state.items() if not k.startswith("clap.")}
    other = both_halves(NARROW, 9)
    for k, v in other.items():
        assert "clap.model." + k in state, k
        state["clap.model." + k] = v
    emb.__dict__["_engine"], emb.__dict__["_text_engine"] = 0, 0
    model.load_state_dict(state)
    assert emb._engine is None and emb._text_engine is None, "the parent's load must invalidate both engines"
    after = model.state_dict()
    for k, v in other.items():
        assert torch.equal(after["clap.model." + k], v), k
    k = "text_branch.encoder.layer.0.attention.self.query.weight"
    assert not torch.equal(other[k], both_halves(NARROW, 5)[k]) and not torch.equal(other["audio_projection.0.weight"], both_halves(NARROW, 5)["audio_projection.0.weight"])
    assert all(torch.equal(after[k], v) for k, v in rest_before.items()), "the U-Net and the onset encoder must not change"


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_text_symbols_declared_bound_and_exported():
    import syncfusion_amd
    from syncfusion_amd import _lib

    header = open(os.path.join(ROOT, "include", "syncfusion_amd.h")).read()
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in TEXT_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/syncfusion_amd.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    for name in ("clap_text", "ClapEmbedder", "ClapTextConfig", "ClapTokenizer"):
        assert name in syncfusion_amd.__all__ and hasattr(syncfusion_amd, name)
    assert "main/module_diffusion.py:69-71" in header and "exp/evaluate_gh_gen_text.yaml:29" in header


def test_refusals_that_need_no_device():
    """Everything here is refused before the first HIP call: the pointers are never dereferenced."""
    from syncfusion_amd import _lib

    lib = _lib.load()
    P = 4096                                                               # a non-null pointer nobody reads
    emb = lambda ids=P, B=1, S=4, C_=128, vocab=300, n_pos=80, word=P, out=P, eps=1e-5: lib.sf_op_text_embed(ids, B, S, C_, vocab, n_pos, 1, word, P, P, P, P, eps, out, None)
    assert emb(ids=None) == 1 and emb(word=None) == 1 and emb(out=None) == 1 and emb(B=0) == 1 and emb(S=0) == 1 and emb(eps=0.0) == 1 and emb(vocab=0) == 1
    assert emb(C_=96) == 6 and emb(C_=1088) == 6 and emb(C_=0) == 6
    ln = lambda x=P, rows=3, C_=128, g=P, y=P: lib.sf_op_layernorm_affine(x, rows, C_, g, P, 1e-5, y, None)
    assert ln(x=None) == 1 and ln(g=None) == 1 and ln(y=None) == 1 and ln(rows=0) == 1
    assert ln(C_=100) == 6 and ln(C_=2048) == 6 and b"multiple of 64" in lib.sf_last_error()
    att = lambda q=P, m=P, B=1, S=8, heads=2, o=P: lib.sf_op_masked_attention(q, m, B, S, heads, o, None)
    assert att(q=None) == 1 and att(m=None) == 1 and att(o=None) == 1 and att(B=0) == 1 and att(S=0) == 1 and att(heads=0) == 1
    assert att(S=129) == 6 and b"128" in lib.sf_last_error()
    m = embedder()
    h = C.c_void_p()
    table = (_lib.SfTensor * 2)()
    table[0].name, table[0].data, table[0].numel = b"emb.word", P, 300 * 128
    table[1].name, table[1].data, table[1].numel = b"emb.pos", P, 80 * 128 - 1
    cfg = m.text_engine_config()
    assert lib.sf_clap_text_create(C.byref(cfg), table, 1, None, C.byref(h)) == 2 and b"emb.pos" in lib.sf_last_error() and not h.value
    assert lib.sf_clap_text_create(C.byref(cfg), table, 2, None, C.byref(h)) == 2 and b"emb.pos" in lib.sf_last_error()      # mis-sized
    assert lib.sf_clap_text_create(None, table, 1, None, C.byref(h)) == 1 and lib.sf_clap_text_create(C.byref(cfg), table, 0, None, C.byref(h)) == 1

    def changed(**kw):
        c = m.text_engine_config()
        for k, v in kw.items():
            setattr(c, k, v)
        return lib.sf_clap_text_create(C.byref(c), table, 1, None, C.byref(h))

    assert changed(heads=4) == 6 and changed(hidden=1088, heads=17) == 6 and changed(max_length=129, max_positions=514) == 6      # head dim 32; C > 1024; S > 128
    assert changed(max_positions=78) == 3 and changed(joint_dim=2048) == 3
    assert changed(layers=0) == 1 and changed(pooling=2) == 1
    assert lib.sf_clap_text_workspace_bytes(None, 1, 4) == -1
    assert lib.sf_clap_text_forward(None, P, P, 1, 4, P, None, P, 1 << 30, None) == 1
    buf = C.create_string_buffer(4096)
    assert lib.sf_clap_text_describe(C.byref(cfg), 1, 78, buf, len(buf)) == 3 and lib.sf_clap_text_describe(C.byref(cfg), 0, 4, buf, len(buf)) == 1
    assert lib.sf_clap_text_describe(C.byref(cfg), 1, 200, buf, len(buf)) == 6 and lib.sf_clap_text_describe(C.byref(cfg), 1, 4, buf, 8) == 1


def test_every_gemm_of_both_configurations_has_a_kernel():
    from syncfusion_amd.clap_text import ClapEmbedder, ClapTextConfig

    shapes = ((1, 2), (1, 5), (3, 77), (8, 16), (16, 128))         # (S = 128 needs max_length = 128: the largest the kernels take)
    for m, cfg in ((embedder(replace(NARROW, max_length=128, max_positions=130)), NARROW), (ClapEmbedder(clap_ref.NARROW, ClapTextConfig(max_length=128)), ClapTextConfig())):
        for B, S in shapes:
            text = m.describe_gemms(B, S)
            lines = text.strip().splitlines()
            assert len(lines) == 4 and "invalid" not in text, text
            assert f"M {B * S} N {3 * cfg.hidden} K {cfg.hidden}" in lines[0] and f"N {cfg.hidden} K {cfg.intermediate}" in lines[3]
    assert "stage 0 qkv" in embedder().describe_gemms(2)                # without S: the audio network's, as before
