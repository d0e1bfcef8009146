"""CLAP audio embedder, the parts that need no device: geometry and refusals, repeatpad / truncation, the state-dict handling, loading through
``Model.load_state_dict``, the weight folding, the C ABI's declarations and the self-check of the fp64 restatement (tests/clap_ref.py).
The product computes the token permutation, the region ids, the bias index and the bicubic weights inside its kernels, so there is no host
index map or host bicubic table to compare here; tests/test_gpu_clap.py holds the kernels to the restatement."""
import ctypes as C
import os
import re
import warnings
from dataclasses import replace

import numpy as np
import pytest
import torch

import clap_ref
from clap_ref import FULL, NARROW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLAP_SYMBOLS = ("sf_op_logmel_image", "sf_op_window_attention", "sf_clap_audio_create", "sf_clap_audio_destroy", "sf_clap_audio_max_batch",
                "sf_clap_audio_workspace_bytes", "sf_clap_audio_forward", "sf_clap_audio_describe")


def embedder(cfg=NARROW, seed=None):
    from syncfusion_amd.clap import ClapAudioEmbedder

    m = ClapAudioEmbedder(cfg)
    if seed is not None:
        m.load_state_dict(clap_ref.seeded_weights(cfg, seed))
    return m


# ---- geometry and refusals --------------------------------------------------------------------------------------------------------------------
def test_geometry_of_both_configurations():
    assert (FULL.frames, FULL.target_frames, FULL.freq_ratio, FULL.tokens_side, FULL.final_dim) == (1001, 1024, 4, 64, 768)
    assert (NARROW.frames, NARROW.target_frames, NARROW.freq_ratio, NARROW.tokens_side, NARROW.final_dim) == (501, 512, 4, 32, 384)
    assert [FULL.stage_resolution(i) for i in range(4)] == [64, 32, 16, 8]
    assert [[FULL.block_shift(i, j) for j in range(d)] for i, d in enumerate(FULL.depths)] == [[0, 4], [0, 4], [0, 4, 0, 4, 0, 4], [0, 0]]
    assert [[NARROW.block_shift(i, j) for j in range(d)] for i, d in enumerate(NARROW.depths)] == [[0, 4], [0, 4], [0, 0]]
    assert all(c // h == 24 for c, h in zip((96, 192, 384, 768), FULL.num_heads))
    n = sum(p.numel() for p in embedder(FULL).parameters())
    assert 27.5e6 < n < 29e6, n


def test_filterbanks_have_no_empty_filter():
    from syncfusion_amd.audio_features import compact_filterbank
    from syncfusion_amd.clap import clap_mel_matrix

    for cfg, least in ((NARROW, 3), (FULL, 2)):
        w = clap_mel_matrix(cfg)
        assert w.shape == (cfg.n_fft // 2 + 1, cfg.mel_bins)
        first, count, packed = compact_filterbank(w.T)
        assert int(count.min()) >= least, (cfg.mel_bins, int(count.min()))


def test_constructor_refusals_and_text_branch():
    from syncfusion_amd.clap import ClapAudioConfig, ClapAudioEmbedder

    with pytest.raises(ValueError, match="enable_fusion"):
        ClapAudioEmbedder(NARROW, enable_fusion=True)
    with pytest.raises(ValueError, match="HTSAT-base"):
        ClapAudioEmbedder(NARROW, amodel="HTSAT-base")
    with pytest.raises(ValueError, match="frames exceed"):
        ClapAudioEmbedder(replace(NARROW, clip_samples=61440))          # 513 frames > 512
    with pytest.raises(ValueError, match="truncation"):
        ClapAudioEmbedder(replace(NARROW, truncation="tail"))
    m = ClapAudioEmbedder(NARROW, enable_fusion=False, amodel="HTSAT-tiny", device="cpu", some_upstream_kwarg=1)
    with pytest.raises(NotImplementedError, match="RoBERTa"):
        m.get_text_embedding(["a dog"], use_tensor=True)
    assert all(not p.requires_grad for p in m.parameters()) and len(list(m.parameters())) > 50
    assert isinstance(ClapAudioConfig(), ClapAudioConfig) and ClapAudioEmbedder().config == FULL


def test_cpu_tensor_is_refused():
    from syncfusion_amd._lib import SyncFusionAmdError

    m = embedder()
    with pytest.raises(SyncFusionAmdError, match="no CPU execution path"):
        m.get_audio_embedding_from_data(torch.zeros(1, 1000), use_tensor=True)
    with pytest.raises(SyncFusionAmdError, match="no CPU execution path"):
        m.embed_image(torch.zeros(1, 128, 128))


def test_load_ckpt_none_warns_once_and_keeps_the_seeded_initialisation():
    m = embedder()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.warns(UserWarning, match="seeded initialisation"):
        m.load_ckpt(None)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.load_ckpt(None)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert all(torch.equal(v, before[k]) for k, v in embedder().state_dict().items()), "the initialisation is seeded"


# ---- length -----------------------------------------------------------------------------------------------------------------------------------
def test_repeatpad_and_truncations():
    from syncfusion_amd.clap import fit_length

    cfg = replace(NARROW, clip_samples=10)
    x = torch.arange(1.0, 9.0).reshape(2, 4)
    y = fit_length(x, cfg)
    assert torch.equal(y, torch.tensor([[1, 2, 3, 4, 1, 2, 3, 4, 0, 0], [5, 6, 7, 8, 5, 6, 7, 8, 0, 0]], dtype=torch.float32))
    assert torch.equal(y, clap_ref.fit_length(x, cfg))
    six = torch.arange(12.0).reshape(2, 6)
    assert torch.equal(fit_length(six, cfg), torch.cat([six, torch.zeros(2, 4)], dim=1))            # int(10 / 6) = 1 copy
    assert fit_length(torch.ones(1, 10), cfg).shape == (1, 10)
    long = torch.arange(25.0)[None]
    assert torch.equal(fit_length(long, replace(cfg, truncation="head")), long[:, :10])
    rng = np.random.RandomState(3)
    start = np.random.RandomState(3).randint(0, 25 - 10 + 1)
    assert torch.equal(fit_length(long, cfg, rng=rng), long[:, start:start + 10])
    starts = {int(fit_length(long, cfg, rng=rng)[0, 0]) for _ in range(200)}
    assert min(starts) == 0 and max(starts) == 15                                                  # both ends of randint(0, L - n + 1)


# ---- keys -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["", "module.", "model.", "clap.model."])
def test_state_dict_loads_under_every_prefix_and_drops_what_is_not_read(prefix, tmp_path):
    sd = clap_ref.seeded_weights(NARROW, 5)
    state = {prefix + k: v for k, v in sd.items()}
    junk = {"text_branch.embeddings.word_embeddings.weight": torch.zeros(3, 3), "logit_scale_a": torch.zeros(()), "logit_scale_t": torch.zeros(()),
            "text_projection.0.weight": torch.zeros(2, 2), "text_transform.sequential.0.weight": torch.zeros(2, 2),
            "audio_transform.sequential.0.weight": torch.zeros(2, 2), "audio_branch.spectrogram_extractor.stft.conv_real.weight": torch.zeros(129, 1, 256),
            "audio_branch.spectrogram_extractor.stft.conv_imag.weight": torch.zeros(129, 1, 256), "audio_branch.tscam_conv.weight": torch.zeros(5, 5),
            "audio_branch.head.weight": torch.zeros(7, 7), "audio_branch.head.bias": torch.zeros(7), "audio_branch.layers.0.blocks.1.attn_mask": torch.zeros(16, 64, 64),
            "audio_branch.layers.0.blocks.0.attn.relative_position_index": torch.zeros(64, 64, dtype=torch.long),
            "audio_branch.bn0.num_batches_tracked": torch.tensor(7)}
    state.update({prefix + k: v for k, v in junk.items()})
    m = embedder()
    m.load_state_dict(state)
    own = m.state_dict()
    for k, v in sd.items():
        assert torch.equal(own["model." + k], v), k
    # the same through a file, bare and under `state_dict`
    for i, payload in enumerate((state, {"state_dict": state, "epoch": 3})):
        path = tmp_path / f"ckpt{i}.pt"
        torch.save(payload, path)
        m2 = embedder()
        m2.load_ckpt(str(path))
        assert all(torch.equal(m2.state_dict()["model." + k], v) for k, v in sd.items())


def test_missing_and_mis_shaped_keys_are_named():
    sd = clap_ref.seeded_weights(NARROW, 5)
    key = "audio_branch.layers.1.blocks.0.attn.qkv.weight"
    with pytest.raises(KeyError, match=re.escape(key)):
        embedder().load_state_dict({k: v for k, v in sd.items() if k != key})
    bad = dict(sd)
    bad[key] = torch.zeros(3, 3)
    with pytest.raises(ValueError, match=re.escape(key)):
        embedder().load_state_dict(bad)
    without_melw = {k: v for k, v in sd.items() if "melW" not in k}
    m = embedder()
    m.load_state_dict(without_melw)                                       # optional: the computed filterbank stays
    assert torch.equal(m.state_dict()["model.audio_branch.logmel_extractor.melW"], sd["audio_branch.logmel_extractor.melW"])
    custom = dict(sd)
    custom["audio_branch.logmel_extractor.melW"] = sd["audio_branch.logmel_extractor.melW"] * 2
    m.load_state_dict(custom)
    assert torch.equal(m.model.audio_branch.logmel_extractor.melW, custom["audio_branch.logmel_extractor.melW"])


def test_every_weight_load_invalidates_the_engine():
    m = embedder()
    sd = clap_ref.seeded_weights(NARROW, 6)
    for load in (lambda: m.load_state_dict(sd), lambda: torch.nn.Module.load_state_dict(m, m.state_dict()), lambda: m.float()):
        m.__dict__["_engine"], m.__dict__["_scale_shift"] = 0, ("stale", "stale")       # (0: nothing for the library to destroy)
        load()
        assert m._engine is None and m._scale_shift is None


def test_model_load_state_dict_reaches_the_embedder():
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
    unet_before = {k: v.clone() for k, v in state.items() if not k.startswith("clap.")}
    other = clap_ref.seeded_weights(NARROW, 9)
    for k, v in other.items():
        assert "clap.model." + k in state, k
        state["clap.model." + k] = v
    emb.__dict__["_engine"] = 0
    model.load_state_dict(state)
    assert emb._engine is None, "the parent's load must invalidate the embedder's engine"
    after = model.state_dict()
    changed = 0
    for k, v in other.items():
        assert torch.equal(after["clap.model." + k], v), k
        changed += int(not torch.equal(v, clap_ref.seeded_weights(NARROW, 5)[k])) if k.endswith("qkv.weight") else 0
    assert changed > 0
    assert all(torch.equal(after[k], v) for k, v in unet_before.items()), "the U-Net and the onset encoder must not change"


def test_target_path_instantiates():
    from syncfusion_amd import ClapAudioEmbedder, instantiate

    m = instantiate({"_target_": "syncfusion_amd.clap.ClapAudioEmbedder", "enable_fusion": False, "amodel": "HTSAT-tiny"})
    assert isinstance(m, ClapAudioEmbedder) and m.config == FULL
    from syncfusion_amd.config import TARGET_MAP

    assert TARGET_MAP["laion_clap.CLAP_Module"] == "syncfusion_amd.module.RandomEmbedder"       # the stub stays the default


# ---- folding ----------------------------------------------------------------------------------------------------------------------------------
def test_folded_weights_state_the_same_network():
    m = embedder(seed=5)
    sd = clap_ref.seeded_weights(NARROW, 5)
    w = dict(m.engine_weights())
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 96, generator=g, dtype=torch.float64)
    p = "audio_branch.layers.0.blocks.1."
    ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(x, (96,), sd[p + "norm1.weight"].double(), sd[p + "norm1.bias"].double(), 1e-5),
                                     sd[p + "attn.qkv.weight"].double(), sd[p + "attn.qkv.bias"].double())
    got = torch.nn.functional.linear(torch.nn.functional.layer_norm(x, (96,), None, None, 1e-5), w["s0.b1.qkv.w"].double(), w["s0.b1.qkv.b"].double())
    assert float((got - ref).norm() / ref.norm()) < 1e-6
    x4 = torch.randn(5, 384, generator=g, dtype=torch.float64)
    p = "audio_branch.layers.0.downsample."
    ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(x4, (384,), sd[p + "norm.weight"].double(), sd[p + "norm.bias"].double(), 1e-5),
                                     sd[p + "reduction.weight"].double())
    got = torch.nn.functional.linear(torch.nn.functional.layer_norm(x4, (384,), None, None, 1e-5), w["s0.merge.w"].double(), w["s0.merge.b"].double())
    assert float((got - ref).norm() / ref.norm()) < 1e-6
    scale, shift = m.bn_scale_shift()
    v = torch.randn(4, 32, generator=g, dtype=torch.float64) * 30 - 40
    bn = lambda k: sd["audio_branch.bn0." + k].double()
    ref = (v - bn("running_mean")) / torch.sqrt(bn("running_var") + 1e-5) * bn("weight") + bn("bias")
    assert float((v * scale.double() + shift.double() - ref).abs().max()) < 1e-5
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in w.values())


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_clap_symbols_declared_bound_and_exported():
    import syncfusion_amd
    from syncfusion_amd import _lib

    header = open(os.path.join(ROOT, "include", "syncfusion_amd.h")).read()
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in CLAP_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/syncfusion_amd.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    for name in ("clap", "ClapAudioConfig", "ClapAudioEmbedder"):
        assert name in syncfusion_amd.__all__ and hasattr(syncfusion_amd, name)
    assert "main/module_diffusion.py:64-67" in header and "exp/model/diffusion.yaml:45-48" in header


def test_refusals_that_need_no_device():
    """Everything here is refused before the first HIP call: the pointers are never dereferenced."""
    from syncfusion_amd import _lib

    lib = _lib.load()
    P = 4096                                                               # a non-null pointer nobody reads
    att = lambda B=1, H=16, W=16, C=96, heads=4, shift=0, q=P, t=P, o=P: lib.sf_op_window_attention(q, B, H, W, C, heads, shift, t, -100.0, o, None)
    assert att(q=None) == 1 and att(t=None) == 1 and att(o=None) == 1 and att(B=0) == 1
    assert att(H=12) == 3 and att(W=20) == 3 and att(heads=5) == 3                # H, W multiples of 8; heads divide C
    assert att(H=8, shift=4) == 3 and att(W=8, H=16, shift=4) == 3                # a shifted window needs more than one window per side
    assert att(shift=2) == 6 and att(C=96, heads=16) == 6 and att(C=144, heads=4) == 6   # shift 0 / 4; head dim 6 and 36
    assert b"head dim 36" in lib.sf_last_error()
    img = lambda B=1, n=32, T=501, r=4, m=P, s=P, t=P, o=P, amin=1e-10: lib.sf_op_logmel_image(m, B, n, T, r, s, t, amin, o, None)
    assert img(m=None) == 1 and img(s=None) == 1 and img(o=None) == 1 and img(B=0) == 1 and img(amin=0.0) == 1 and img(T=1) == 1
    assert img(T=513) == 3 and b"not shrunk" in lib.sf_last_error()
    cfg = embedder().engine_config()
    h = C.c_void_p()
    table = (_lib.SfTensor * 1)()
    table[0].name, table[0].data, table[0].numel = b"patch.w", P, 96 * 16
    assert lib.sf_clap_audio_create(C.byref(cfg), table, 1, None, C.byref(h)) == 2 and b"patch.b" in lib.sf_last_error() and not h.value
    bad = embedder().engine_config()
    bad.window = 7
    assert lib.sf_clap_audio_create(C.byref(bad), table, 1, None, C.byref(h)) == 6
    bad = embedder().engine_config()
    bad.spec_size = 96
    assert lib.sf_clap_audio_create(C.byref(bad), table, 1, None, C.byref(h)) == 3
    assert lib.sf_clap_audio_workspace_bytes(None, 1) == -1 and lib.sf_clap_audio_max_batch(None) == -1
    assert lib.sf_clap_audio_forward(None, P, 1, P, None, P, 1 << 30, None) == 1


def test_every_gemm_of_both_configurations_has_a_kernel():
    for cfg, batches in ((NARROW, (1, 3)), (FULL, (2, 4, 10))):
        m = embedder(cfg)
        for B in batches:
            text = m.describe_gemms(B)
            lines = text.strip().splitlines()
            assert len(lines) == 5 * len(cfg.depths) - 1 and "invalid" not in text, text
            assert f"M {B * cfg.tokens_side ** 2} N {3 * cfg.embed_dim} K {cfg.embed_dim}" in lines[0]


# ---- the restatement's self-check -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,shift", [(8, 8, 0), (16, 16, 0), (16, 16, 4), (16, 24, 4)])
def test_reference_windowed_attention_equals_dense_attention(H, W, shift):
    g = torch.Generator().manual_seed(H * 100 + W + shift)
    B, heads, D = 2, 4, 24
    C = heads * D
    qkv = torch.randn(B * H * W, 3 * C, generator=g, dtype=torch.float64)
    table = 0.5 * torch.randn(225, heads, generator=g, dtype=torch.float64)
    win = clap_ref.window_attention(qkv, B, H, W, heads, shift, table, -100.0)
    dense = clap_ref.dense_window_attention(qkv, B, H, W, heads, shift, table)
    # a finite mask leaves exp(-100 + score spread) of the weight on the other regions: far below the fp64 rounding of the two orders of summation
    assert float((win - dense).abs().max()) < 1e-12
    if shift:
        assert float((win - clap_ref.window_attention(qkv, B, H, W, heads, 0, table, -100.0)).abs().max()) > 1e-3
