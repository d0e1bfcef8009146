"""CLAP text embedder on the device (MI355X) against the fp64 restatement of tests/clap_text_ref.py: the embedding gather, the affine
LayerNorm, the masked attention, the network (narrow and full-width configurations, every tap), the whole path from strings, graph capture,
weight reloads, refusals, guard bands and a ``Model`` that generates from a text prompt with the embedder inside."""
import ctypes as C
import functools
from dataclasses import asdict, replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clap_ref
import clap_text_ref
from clap_text_ref import HAND_MERGES, NARROW, WIDE, write_tokenizer
from guards import Guards
from numerics import check_close

pytestmark = pytest.mark.gpu

FP32_GATE = 1e-4             # the project's fp32 rel-L2 figure (check_close adds the max-error bound)
# end to end from strings against the all-fp64 path at 77 columns: measured relative L2 error of the embeddings on MI355X (test_end_to_end), gated
# at 10 x that because summation orders differ between boxes through the layers, and never above 1e-3
E2E_MEASURED = 4.4e-7
E2E_CEILING = 1e-3
PROMPTS = ["abc cab", "a's ab  ab abc!", "", "cab " * 40]            # (the last one is truncated at 77 tokens)


def text_config(cfg, **changes):
    from syncfusion_amd.clap_text import ClapTextConfig

    return replace(ClapTextConfig(**asdict(cfg)), **changes)


@functools.lru_cache(maxsize=None)
def weights(kind, seed):
    return clap_text_ref.seeded_weights(NARROW if kind == "narrow" else WIDE, seed)


def embedder(kind, seed, device, audio_cfg=clap_ref.NARROW, audio_seed=None, tokenizer_dir=None, **changes):
    from syncfusion_amd.clap_text import ClapEmbedder

    cfg = NARROW if kind == "narrow" else WIDE
    m = ClapEmbedder(audio_cfg, text_config(cfg, **changes), tokenizer_dir=tokenizer_dir)
    audio = clap_ref.seeded_weights(audio_cfg, audio_seed) if audio_seed is not None else {k[len("model."):]: v for k, v in m.state_dict().items() if "audio_" in k}
    m.load_state_dict({**audio, **weights(kind, seed)})
    return m.to(device)


def stream(device):
    from syncfusion_amd import _lib

    return _lib.stream_ptr(device)


# ---- the embedding gather ---------------------------------------------------------------------------------------------------------------------
def embed_case(B, S, C_, seed):
    """ids with a full row and rows padded in the tail; tables whose rows are independent draws (a wrong index cannot pass)."""
    cfg = replace(NARROW, vocab_size=50, hidden=C_, max_positions=S + 2)
    g = torch.Generator().manual_seed(seed)
    ids, _ = clap_text_ref.tokens(cfg, [S, 2, (S + 2) // 2][:B], S, seed)
    e = "text_branch.embeddings."
    sd = {e + "word_embeddings.weight": torch.randn(50, C_, generator=g), e + "position_embeddings.weight": 2.0 * torch.randn(S + 2, C_, generator=g),
          e + "token_type_embeddings.weight": torch.randn(1, C_, generator=g), e + "LayerNorm.weight": 1.0 + 0.2 * torch.randn(C_, generator=g),
          e + "LayerNorm.bias": 0.1 * torch.randn(C_, generator=g)}
    return cfg, ids, sd


def run_embed(device, cfg, ids, sd, guards=None):
    from syncfusion_amd import _lib

    B, S = ids.shape
    e = "text_branch.embeddings."
    names = ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias")
    ins = [ids.to(torch.int32).to(device)] + [sd[e + n].to(device).contiguous() for n in names]
    if guards is None:
        out = torch.full((B * S, cfg.hidden), float("nan"), device=device)
        ptrs, optr = [t.data_ptr() for t in ins], out.data_ptr()
    else:
        ptrs = [guards.inp(t, f"in{i}").ptr for i, t in enumerate(ins)]
        o = guards.out((B * S, cfg.hidden), name="out")
        out, optr = o.payload, o.ptr
    _lib.check(_lib.load().sf_op_text_embed(ptrs[0], B, S, cfg.hidden, cfg.vocab_size, cfg.max_positions, cfg.pad_id, *ptrs[1:], cfg.ln_eps, optr,
                                            stream(device)), "sf_op_text_embed")
    return out


@pytest.mark.parametrize("C_", [128, 768])
@pytest.mark.parametrize("B,S", [(1, 2), (3, 13), (2, 77)])
def test_text_embed_against_fp64(cuda, B, S, C_):
    cfg, ids, sd = embed_case(B, S, C_, 100 + S + C_)
    assert bool((ids[0] != cfg.pad_id).all()) and (B == 1 or bool((ids[1:] == cfg.pad_id).any()))
    ref = clap_text_ref.embeddings(ids, sd, cfg).reshape(B * S, C_)
    check_close(run_embed(cuda, cfg, ids, sd), ref, FP32_GATE, f"text embed B {B} S {S} C {C_}", dims=("row", "channel"))


# ---- the affine LayerNorm ---------------------------------------------------------------------------------------------------------------------
def run_layernorm(device, x, gamma, beta, guards=None):
    from syncfusion_amd import _lib

    rows, C_ = x.shape
    if guards is None:
        xd, g, b, out = x.to(device), gamma.to(device), beta.to(device), torch.full((rows, C_), float("nan"), device=device)
        ptrs = (xd.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr())
    else:
        xd, g, b, o = guards.inp(x.to(device), "x"), guards.inp(gamma.to(device), "gamma"), guards.inp(beta.to(device), "beta"), guards.out((rows, C_), name="y")
        ptrs, out = (xd.ptr, g.ptr, b.ptr, o.ptr), o.payload
    _lib.check(_lib.load().sf_op_layernorm_affine(ptrs[0], rows, C_, ptrs[1], ptrs[2], 1e-5, ptrs[3], stream(device)), "sf_op_layernorm_affine")
    return out


def layernorm_case(rows, C_):
    g = torch.Generator().manual_seed(rows * 7 + C_)
    return 1e3 + torch.randn(rows, C_, generator=g), 1.0 + 0.2 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)


@pytest.mark.parametrize("rows", [1, 77])
@pytest.mark.parametrize("C_", [64, 128, 768, 1024])
def test_layernorm_affine_against_fp64_at_offset_inputs(cuda, C_, rows):
    """Inputs offset by 1e3: a one-pass variance (E[x^2] - E[x]^2) loses every digit here; the reference normalises the fp32 inputs in fp64."""
    x, gamma, beta = layernorm_case(rows, C_)
    ref = F.layer_norm(x.double(), (C_,), gamma.double(), beta.double(), 1e-5)
    check_close(run_layernorm(cuda, x, gamma, beta), ref, FP32_GATE, f"layernorm rows {rows} C {C_}", dims=("row", "channel"))


# ---- masked attention -------------------------------------------------------------------------------------------------------------------------
def attention_case(B, S, heads, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3, heads, 64, generator=g)
    qkv[:, :2] *= (0.6 + 0.25 * torch.arange(heads, dtype=torch.float32))[None, None, :, None].clamp(max=1.6)   # per head: neither flat nor one-hot rows
    lengths = [S, 2, max(2, S // 2 + 1)][:B] if B > 1 else [max(2, 2 * S // 3)]
    mask = torch.zeros(B, S, dtype=torch.int32)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    return qkv.reshape(B * S, 3 * heads * 64).contiguous(), mask


def poisoned(qkv, mask, heads, value):
    """The K and V rows of masked positions filled with ``value``; Q rows stay (padded query rows are computed)."""
    C_ = heads * 64
    out = qkv.clone()
    gone = (mask.reshape(-1) == 0)
    out[gone, C_:] = value
    return out


def run_masked_attention(device, qkv, mask, heads, guards=None):
    from syncfusion_amd import _lib

    B, S = mask.shape
    C_ = heads * 64
    if guards is None:
        q, m, out = qkv.to(device), mask.to(device), torch.full((B * S, C_), float("nan"), device=device)
        ptrs = (q.data_ptr(), m.data_ptr(), out.data_ptr())
    else:
        q, m, o = guards.inp(qkv.to(device), "qkv"), guards.inp(mask.to(device), "mask"), guards.out((B * S, C_), name="out")
        ptrs, out = (q.ptr, m.ptr, o.ptr), o.payload
    _lib.check(_lib.load().sf_op_masked_attention(ptrs[0], ptrs[1], B, S, heads, ptrs[2], stream(device)), "sf_op_masked_attention")
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("S", [2, 5, 64, 65, 77, 128])
def test_masked_attention_against_fp64(cuda, S, heads, B):
    qkv, mask = attention_case(B, S, heads, 1000 + 7 * S + heads + B)
    ref = clap_text_ref.masked_attention(qkv.double().reshape(B, S, -1), mask, heads).reshape(B * S, heads * 64)
    out = run_masked_attention(cuda, qkv, mask, heads)
    check_close(out, ref, FP32_GATE, f"masked attention S {S} heads {heads} B {B}", dims=("row", "channel"))
    if bool((mask == 0).any()):
        # whatever the K / V rows of masked keys hold, the output is the same bits: they carry weight exactly 0 and are not multiplied in
        for value in (1e30, float("nan")):
            again = run_masked_attention(cuda, poisoned(qkv, mask, heads, value), mask, heads)
            assert bool(torch.isfinite(again).all()) and torch.equal(again, out), f"masked K / V rows filled with {value} reach the output"
    else:
        assert S == 2
    if B == 3:      # a text's rows do not depend on the batch
        alone = run_masked_attention(cuda, qkv[:S], mask[:1], heads)
        assert torch.equal(alone, out[:S])


def test_masked_attention_without_any_key_gives_zeros(cuda):
    qkv, mask = attention_case(3, 5, 2, 5)
    mask[1] = 0
    out = run_masked_attention(cuda, poisoned(qkv, mask, 2, float("nan")), mask, 2)
    assert bool((out[5:10] == 0).all()) and bool(torch.isfinite(out).all()) and float(out[:5].abs().max()) > 0


# ---- the network ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def network_reference(kind, seed):
    """(ids, mask, embedding, taps) for 3 texts of 12 columns (narrow) / 2 of 16 (wide); text 0 fills its row, the others are padded."""
    cfg, lengths, S = (NARROW, (12, 2, 7), 12) if kind == "narrow" else (WIDE, (16, 5), 16)
    ids, mask = clap_text_ref.tokens(cfg, lengths, S, 60 + seed)
    emb, taps = clap_text_ref.encode(ids, mask, weights(kind, seed), cfg)
    return cfg, ids, mask, emb, taps


def run_network(cuda, kind, B, seed=31):
    cfg, ids, mask, emb_ref, taps_ref = network_reference(kind, seed)
    m = embedder(kind, seed, cuda)
    S, Bref = ids.shape[1], ids.shape[0]
    emb, taps = m.embed_tokens(ids[:B], mask[:B], taps=True)
    assert len(taps) == len(taps_ref) == cfg.layers + 2
    for i, (t, r) in enumerate(zip(taps, taps_ref)):
        rows = r.shape[0] // Bref * B
        check_close(t, r[:rows], FP32_GATE, f"{kind} B={B} tap {i} {tuple(t.shape)}", dims=("row", "channel"))
    check_close(emb, emb_ref[:B], FP32_GATE, f"{kind} B={B} embedding", dims=("text", "dim"))
    assert float((emb.double().norm(dim=1) - 1).abs().max()) < 1e-6
    assert taps[0].shape == (B * S, cfg.hidden)
    return emb, taps


def test_network_narrow_against_fp64_and_batch_independence(cuda):
    emb1, taps1 = run_network(cuda, "narrow", 1)
    emb3, taps3 = run_network(cuda, "narrow", 3)
    for i, (a, b) in enumerate(zip(taps1, taps3)):
        assert torch.equal(a, b[:a.shape[0]]), f"tap {i}: the rows of text 0 depend on the batch"
    assert torch.equal(emb1[0], emb3[0])


def test_network_wide_against_fp64(cuda):
    run_network(cuda, "wide", 2)


def test_cls_pooling_and_plain_projection(cuda):
    cfg, ids, mask, _, _ = network_reference("narrow", 31)
    other = replace(cfg, pooling="cls", projection_act="none", normalize=False)
    want, taps_ref = clap_text_ref.encode(ids, mask, weights("narrow", 31), other)
    got, taps = embedder("narrow", 31, cuda, pooling="cls", projection_act="none", normalize=False).embed_tokens(ids, mask, taps=True)
    check_close(taps[-1], taps_ref[-1], FP32_GATE, "cls pooled rows", dims=("text", "channel"))
    check_close(got, want, FP32_GATE, "cls / no ReLU / no normalisation", dims=("text", "dim"))


def test_trimmed_equals_padded_to_max_length(cuda):
    cfg = NARROW
    ids, mask = clap_text_ref.tokens(cfg, (9, 2, 5), cfg.max_length, 4)
    trimmed, taps = embedder("narrow", 31, cuda).embed_tokens(ids, mask, taps=True)
    padded, taps_padded = embedder("narrow", 31, cuda, pad_to_max_length=True).embed_tokens(ids[:, :20], mask[:, :20], taps=True)
    assert taps[0].shape == (3 * 9, cfg.hidden) and taps_padded[0].shape == (3 * cfg.max_length, cfg.hidden)
    rel = float((trimmed.double() - padded.double()).norm() / padded.double().norm())
    print(f"trimmed (S = 9) against padded (S = {cfg.max_length}): rel-L2 {rel:.3e}")
    assert rel < 1e-5


# ---- strings -> embedding ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_from_strings(cuda, tmp_path):
    """Measured on MI355X (relative L2 of the embeddings of PROMPTS, trimmed to 77 real tokens at most, against the all-fp64 path at 77 padded
    columns): 4.4e-7 (E2E_MEASURED).  The gate is 10 x the measured figure and never above 1e-3."""
    write_tokenizer(tmp_path / "tok", HAND_MERGES)
    m = embedder("narrow", 31, cuda, tokenizer_dir=str(tmp_path / "tok"))
    got = m.get_text_embedding(PROMPTS, use_tensor=True)
    assert got.shape == (len(PROMPTS), NARROW.joint_dim) and got.dtype == torch.float32 and got.is_cuda
    ids, mask = m.tokenizer()(PROMPTS)
    assert ids.shape == (len(PROMPTS), 77) and mask.sum(1).tolist()[2:] == [2, 77] and 2 < int(mask[0].sum()) < int(mask[1].sum()) < 20
    ref, _ = clap_text_ref.encode(ids.long(), mask.long(), weights("narrow", 31), NARROW)
    rel = float((got.double().cpu() - ref).norm() / ref.norm())
    gate = min(10 * E2E_MEASURED, E2E_CEILING)
    print(f"end to end from strings: rel-L2 {rel:.3e} (measured {E2E_MEASURED:.1e}, gate {gate:.1e})")
    assert bool(torch.isfinite(got).all()) and rel <= gate
    one = m.get_text_embedding(PROMPTS[1], use_tensor=False)                      # a str is one text; numpy out
    assert isinstance(one, np.ndarray) and one.shape == (1, NARROW.joint_dim)
    check_close(torch.from_numpy(one), ref[1:2], FP32_GATE, "one prompt, trimmed to its own length", dims=("text", "dim"))


# ---- graph, reload ----------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager(cuda):
    cfg, ids, mask, _, _ = network_reference("narrow", 31)
    ids2, mask2 = clap_text_ref.tokens(cfg, (3, 12, 8), 12, 99)
    m = embedder("narrow", 31, cuda)
    dev = lambda t: t.to(torch.int32).to(cuda)
    static_ids, static_mask = dev(ids).clone(), dev(mask).clone()
    m.embed_device(static_ids, static_mask)                          # the warm-up: builds the engine
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.embed_device(static_ids, static_mask)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.embed_device(static_ids, static_mask)
    for i, k in ((ids2, mask2), (ids, mask)):
        static_ids.copy_(dev(i))
        static_mask.copy_(dev(k))
        graph.replay()
        assert torch.equal(out, m.embed_device(dev(i), dev(k)))


def test_reload_changes_the_output_to_the_new_weights(cuda):
    cfg, ids, mask, emb_ref, _ = network_reference("narrow", 31)
    _, _, _, emb_ref2, _ = network_reference("narrow", 32)
    ids2, mask2 = network_reference("narrow", 32)[1:3]
    m = embedder("narrow", 31, cuda)
    check_close(m.embed_tokens(ids, mask), emb_ref, FP32_GATE, "seed 31", dims=("text", "dim"))
    audio = {k[len("model."):]: v.cpu() for k, v in m.state_dict().items() if "audio_" in k}
    m.load_state_dict({"clap.model." + k: v for k, v in {**audio, **weights("narrow", 32)}.items()})
    check_close(m.embed_tokens(ids2, mask2), emb_ref2, FP32_GATE, "seed 32 after reload", dims=("text", "dim"))
    assert float((clap_text_ref.encode(ids2, mask2, weights("narrow", 31), cfg)[0] - emb_ref2).norm()) > 0.1


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing(cuda):
    from syncfusion_amd import _lib

    lib, s = _lib.load(), stream(cuda)
    cfg, ids, mask, _, _ = network_reference("narrow", 31)
    m = embedder("narrow", 31, cuda)
    eng = m._text_engine_for(cuda)
    out = torch.full((4096,), 7.0, device=cuda)
    some = torch.zeros(1 << 16, device=cuda)
    i32 = torch.ones(4096, dtype=torch.int32, device=cuda)
    P, O, I = some.data_ptr(), out.data_ptr(), i32.data_ptr()
    assert lib.sf_op_text_embed(I, 1, 4, 96, 300, 80, 1, P, P, P, P, P, 1e-5, O, s) == 6
    assert lib.sf_op_layernorm_affine(P, 4, 100, P, P, 1e-5, O, s) == 6 and lib.sf_op_layernorm_affine(P, 0, 128, P, P, 1e-5, O, s) == 1
    assert lib.sf_op_masked_attention(P, I, 1, 129, 2, O, s) == 6 and lib.sf_op_masked_attention(P, None, 1, 8, 2, O, s) == 1
    B, S = 3, 12
    need = int(lib.sf_clap_text_workspace_bytes(eng, B, S))
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    fwd = lambda B=B, S=S, ws_bytes=need, ids=I: lib.sf_clap_text_forward(eng, ids, I, B, S, O, None, ws.data_ptr(), ws_bytes, s)
    assert fwd(ids=None) == 1 and fwd(B=0) == 1 and fwd(S=0) == 1
    assert fwd(S=78) == 3 and fwd(S=129) == 6                               # beyond max_length / beyond what the kernels take
    assert fwd(ws_bytes=need - 1) == 5
    assert lib.sf_clap_text_workspace_bytes(eng, B, 78) == -1 and lib.sf_clap_text_workspace_bytes(eng, 0, S) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call must not launch"
    with pytest.raises(ValueError, match="ids outside"):
        m.embed_tokens(torch.tensor([[0, 300, 2]]), torch.tensor([[1, 1, 1]]))
    with pytest.raises(ValueError, match="start with a real token"):
        m.embed_tokens(torch.tensor([[0, 5, 2], [1, 1, 1]]), torch.tensor([[1, 1, 1], [0, 0, 0]]))
    with pytest.raises(ValueError, match="columns"):
        m.embed_tokens(torch.zeros(1, 78, dtype=torch.long), torch.ones(1, 78, dtype=torch.long))
    with pytest.raises(ValueError, match="CPU integer"):
        m.embed_tokens(torch.zeros(1, 3), torch.ones(1, 3, dtype=torch.long))


# ---- guard bands ------------------------------------------------------------------------------------------------------------------------------
def test_guard_bands_text_embed(cuda):
    for B, S, C_ in ((3, 13, 128), (2, 77, 768)):
        cfg, ids, sd = embed_case(B, S, C_, 9)
        with Guards(cuda) as g:
            out = run_embed(cuda, cfg, ids, sd, guards=g)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all())


def test_guard_bands_layernorm_affine(cuda):
    for rows, C_ in ((1, 64), (77, 1024), (5, 768)):
        with Guards(cuda) as g:
            out = run_layernorm(cuda, *layernorm_case(rows, C_), guards=g)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all())


def test_guard_bands_masked_attention(cuda):
    for B, S, heads in ((3, 128, 2), (3, 65, 12), (1, 2, 2), (3, 5, 2)):
        qkv, mask = attention_case(B, S, heads, 9)
        with Guards(cuda) as g:
            out = run_masked_attention(cuda, qkv, mask, heads, guards=g)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("B", [1, 3])
def test_guard_bands_engine_forward(cuda, B):
    from syncfusion_amd import _lib

    cfg, ids, mask, emb_ref, taps_ref = network_reference("narrow", 31)
    m = embedder("narrow", 31, cuda)
    lib, eng = _lib.load(), m._text_engine_for(cuda)
    S = ids.shape[1]
    need = int(lib.sf_clap_text_workspace_bytes(eng, B, S))
    assert need > 0
    with Guards(cuda) as g:
        i, k = g.inp(ids[:B].to(torch.int32).to(cuda), "ids"), g.inp(mask[:B].to(torch.int32).to(cuda), "mask")
        emb = g.out((B, cfg.joint_dim), name="embedding")
        taps = [g.out((B * S, cfg.hidden), name=f"tap{j}") for j in range(cfg.layers + 1)] + [g.out((B, cfg.hidden), name="pooled")]
        ws = g.ws(need)                                            # exactly the queried size
        arr = (C.c_void_p * len(taps))(*[t.ptr for t in taps])
        _lib.check(lib.sf_clap_text_forward(eng, i.ptr, k.ptr, B, S, emb.ptr, arr, ws.ptr, need, stream(cuda)), "sf_clap_text_forward")
        torch.cuda.synchronize()
        check_close(emb.payload, emb_ref[:B], FP32_GATE, "guarded embedding", dims=("text", "dim"))
        assert lib.sf_clap_text_forward(eng, i.ptr, k.ptr, B, S, emb.ptr, arr, ws.ptr, need - 1, stream(cuda)) == 5   # one byte short: refused


# ---- inside a Model ---------------------------------------------------------------------------------------------------------------------------
def test_model_generates_from_a_text_prompt(cuda, tmp_path):
    """A ``Model`` built with the embedder: ``clap_encode_text`` is the restatement's embedding, ``generate_batch(cond_text=True)`` conditions on
    it, and the audio side of the same object still computes ``clap_ref.embed``."""
    from helpers import SMALL_ENCODER, SMALL_UNET
    from syncfusion_amd import DiffusionModel, Encoder1d, Model, UNetV0, VDiffusion, VSampler
    from syncfusion_amd.clap_text import ClapEmbedder
    from syncfusion_amd.generation import generate_batch

    J = SMALL_UNET["embedding_features"]
    acfg, tcfg = replace(clap_ref.NARROW, joint_dim=J), replace(NARROW, joint_dim=J)
    write_tokenizer(tmp_path / "tok", HAND_MERGES)
    emb = ClapEmbedder(acfg, text_config(tcfg), tokenizer_dir=str(tmp_path / "tok"))
    sd_a, sd_t = clap_ref.seeded_weights(acfg, 41), clap_text_ref.seeded_weights(tcfg, 41)
    emb.load_state_dict({**sd_a, **sd_t})
    torch.manual_seed(3)
    dm = DiffusionModel(net_t=functools.partial(UNetV0, seed=5), diffusion_t=VDiffusion, sampler_t=VSampler, use_embedding_cfg=True, **SMALL_UNET)
    with pytest.warns(UserWarning, match="seeded initialisation"):
        model = Model(1e-3, 0.95, 0.999, 1e-6, 1e-3, dm, Encoder1d(seed=6, **SMALL_ENCODER), emb, None).to(cuda)
    B, L0 = 2, 16 * 24
    g = torch.Generator().manual_seed(9)
    y = (torch.rand(B, 1, L0, generator=g) < 0.02).float().to(cuda)
    texts, others = ["abc cab", "a's ab"], ["cab cab cab", "abc"]
    got = model.clap_encode_text(texts)
    assert got.shape == (B, 1, J)
    ids, mask = emb.tokenizer()(texts)
    want, _ = clap_text_ref.encode(ids.long(), mask.long(), sd_t, tcfg)
    check_close(got[:, 0], want, FP32_GATE, "clap_encode_text", dims=("text", "dim"))
    noise = torch.randn(B, 1, L0, generator=g).to(cuda)
    a = generate_batch(model, y, None, texts, cond_text=True, num_steps=3, length=L0, embedding_scale=2.0, noise=noise.clone())
    b = generate_batch(model, y, None, others, cond_text=True, num_steps=3, length=L0, embedding_scale=2.0, noise=noise.clone())
    assert a.shape[0] == B and bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert not torch.equal(a, b), "the sample must depend on the prompt"
    z = torch.stack([clap_ref.chirp(acfg, 6000, 1, 80 + i)[0] for i in range(B)]).reshape(B, 1, 6000).to(cuda)
    q = (torch.clip(z[:, 0].cpu(), -1, 1) * 32767.0).to(torch.int16).float() / 32767.0
    check_close(model.clap_encode_audio(z)[:, 0], clap_ref.embed(q.double(), sd_a, acfg), FP32_GATE, "clap_encode_audio of the same object", dims=("clip", "dim"))
