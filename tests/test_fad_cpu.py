"""FAD evaluation, the parts that need no device: the mel matrix, example counts, the Fréchet distance, the state dict, evaluate_fad's
refusals and the C ABI's declarations and create-time refusals.  References: tests/fad_ref.py (fp64 numpy / torch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAD_SYMBOLS = ("sf_audio_features_create_framed", "sf_logmel_examples_count", "sf_logmel_examples_forward", "sf_vggish_create", "sf_vggish_destroy",
               "sf_vggish_max_examples", "sf_vggish_workspace_bytes", "sf_vggish_forward", "sf_op_maxpool2x2_cl",
               "sf_op_moments")


def narrow_config():
    from syncfusion_amd.fad import VGGishConfig

    return VGGishConfig(layout=fad_ref.NARROW_LAYOUT, fc=fad_ref.NARROW_FC)


# ---- mel matrix and framing -----------------------------------------------------------------------------------------------------------------
def test_mel_matrix_shape_support_and_reference():
    from syncfusion_amd.audio_features import compact_filterbank
    from syncfusion_amd.fad import vggish_mel_matrix

    w = vggish_mel_matrix()
    assert w.shape == (257, 64) and w.dtype == np.float64
    assert not w[0].any()                                            # the DC row
    total = 0
    for i in range(64):
        nz = np.nonzero(w[:, i])[0]
        assert 1 <= nz.size <= 17, (i, nz.size)
        assert nz[-1] - nz[0] + 1 == nz.size, f"band {i} is not contiguous"
        total += nz.size
    assert total == 461
    first, count, packed = compact_filterbank(w.T)                   # the compact form the library takes applies: no empty band
    assert count.min() >= 1 and int(count.sum()) == 461 == packed.size
    assert np.abs(w - fad_ref.mel_matrix()).max() <= 1e-12


@pytest.mark.parametrize("L,E,F", [(399, 0, 0), (15599, 0, 95), (15600, 1, 96), (30959, 1, 191), (31000, 2, 192), (32000, 2, 198)])
def test_example_counts(L, E, F):
    from syncfusion_amd.fad import VGGishConfig

    cfg = VGGishConfig()
    assert (cfg.window_length, cfg.hop_length, cfg.n_fft) == (400, 160, 512)
    assert cfg.frames(L) == F == fad_ref.frame_count(L)
    assert cfg.examples(L) == E == fad_ref.example_count(L)


def test_example_count_of_the_library_agrees():
    from syncfusion_amd import _lib
    from syncfusion_amd.fad import VGGish

    m = VGGish(narrow_config())
    lib = _lib.load()
    for L, E in [(399, 0), (15599, 0), (15600, 1), (30959, 1), (31000, 2), (32000, 2)]:
        assert lib.sf_logmel_examples_count(m._front_end(), L, 96) == E
    assert lib.sf_logmel_examples_count(None, 16000, 96) == -1 and lib.sf_logmel_examples_count(m._front_end(), 16000, 0) == -1


# ---- Fréchet distance -----------------------------------------------------------------------------------------------------------------------
def _sample_stats(n, D, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, D)) * rng.uniform(0.2, 3.0, size=D) + shift * rng.normal(size=D)
    return fad_ref.statistics(x)


def test_frechet_identical_statistics_give_zero():
    from syncfusion_amd.fad import frechet_distance

    for n in (300, 40):                                              # full rank and rank deficient
        mu, s = _sample_stats(n, 128, 1)
        d = frechet_distance(mu, s, mu, s)
        print(f"n = {n}: {d:.3e} of trace {np.trace(s):.3e}")
        assert abs(d) <= 1e-12 * np.trace(s)


def test_frechet_closed_form_commuting_covariances():
    from syncfusion_amd.fad import frechet_distance

    rng = np.random.default_rng(2)
    D = 128
    q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    a, b = rng.uniform(0.01, 4.0, size=D), rng.uniform(0.01, 4.0, size=D)
    s1, s2 = (q * a) @ q.T, (q * b) @ q.T
    mu1, mu2 = rng.normal(size=D), rng.normal(size=D)
    want = np.sum((mu1 - mu2) ** 2) + np.sum((np.sqrt(a) - np.sqrt(b)) ** 2)
    got = frechet_distance(mu1, s1, mu2, s2)
    print(f"closed form {want:.12g}, got {got:.12g}")
    assert abs(got - want) <= 1e-10 * (np.trace(s1) + np.trace(s2))


def test_frechet_symmetric_on_rank_deficient_pair():
    from syncfusion_amd.fad import frechet_distance

    mu1, s1 = _sample_stats(40, 128, 3)
    mu2, s2 = _sample_stats(47, 128, 4, shift=1.0)
    d12, d21 = frechet_distance(mu1, s1, mu2, s2), frechet_distance(mu2, s2, mu1, s1)
    tr = np.trace(s1) + np.trace(s2)
    print(f"d12 {d12:.12g} d21 {d21:.12g} difference / trace sum {abs(d12 - d21) / tr:.2e}")
    assert np.isfinite(d12) and np.isfinite(d21) and abs(d12 - d21) <= 1e-8 * tr


def test_frechet_against_scipy_sqrtm_full_rank():
    pytest.importorskip("scipy")
    from syncfusion_amd.fad import frechet_distance

    mu1, s1 = _sample_stats(300, 128, 5)
    mu2, s2 = _sample_stats(307, 128, 6, shift=1.0)
    got, want = frechet_distance(mu1, s1, mu2, s2), fad_ref.frechet_sqrtm(mu1, s1, mu2, s2)
    tr = np.trace(s1) + np.trace(s2)
    print(f"sqrtm {want:.12g} got {got:.12g} difference / trace sum {abs(got - want) / tr:.2e}")
    assert abs(got - want) <= 1e-9 * tr


def test_moments_merge_equals_one_set():
    from syncfusion_amd.fad import Moments

    rng = np.random.default_rng(7)
    x = rng.normal(size=(50, 24)) + 30.0

    def mom(a):
        return Moments(len(a), a.sum(axis=0), (a - a.mean(axis=0)).T @ (a - a.mean(axis=0)))

    mu, sigma, n = mom(x[:13]).merge(mom(x[13:])).statistics()
    assert n == 50
    assert np.abs(mu - x.mean(axis=0)).max() <= 1e-12 * np.abs(mu).max()
    ref = np.cov(x, rowvar=False)
    assert np.abs(sigma - ref).max() <= 1e-12 * np.abs(ref).max()
    with pytest.raises(ValueError):
        mom(x[:1]).statistics()


# ---- state dict -----------------------------------------------------------------------------------------------------------------------------
def test_state_dict_upstream_names_and_shapes_load():
    from syncfusion_amd.fad import VGGish

    m = VGGish()
    want = {f"features.{i}.{p}" for i in (0, 3, 6, 8, 11, 13) for p in ("weight", "bias")} | \
           {f"embeddings.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")}
    sd = m.state_dict()
    assert set(sd) == want
    assert tuple(sd["features.0.weight"].shape) == (64, 1, 3, 3) and tuple(sd["features.13.weight"].shape) == (512, 512, 3, 3)
    assert tuple(sd["embeddings.0.weight"].shape) == (4096, 512 * 6 * 4) and tuple(sd["embeddings.4.weight"].shape) == (128, 4096)
    assert m.config.final_relu is False                              # use_activation=False: no ReLU after the last Linear


def test_state_dict_pproc_ignored_missing_and_unexpected_raise():
    from syncfusion_amd.fad import VGGish

    m = VGGish(narrow_config())
    state = fad_ref.seeded_weights(fad_ref.NARROW_LAYOUT, fad_ref.NARROW_FC, 11)
    assert set(state) == set(m.state_dict())
    m.load_state_dict({**state, "pproc.pca_eigen_vectors": torch.zeros(128, 128), "pproc.pca_means": torch.zeros(128, 1)})
    assert torch.equal(m.features[0].weight, state["features.0.weight"]) and torch.equal(m.embeddings[4].bias, state["embeddings.4.bias"])
    missing = dict(state)
    del missing["features.3.bias"]
    with pytest.raises(RuntimeError, match="features.3.bias"):
        m.load_state_dict(missing)
    with pytest.raises(RuntimeError, match="classifier.weight"):
        m.load_state_dict({**state, "classifier.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="Missing"):
        m.load_state_dict(missing, strict=False)                     # strictness is not optional


# ---- evaluate_fad refusals ------------------------------------------------------------------------------------------------------------------
def test_evaluate_fad_without_weights_names_the_variable(tmp_path, monkeypatch):
    from syncfusion_amd.fad import evaluate_fad

    monkeypatch.delenv("SYNCFUSION_VGGISH_WEIGHTS", raising=False)
    with pytest.raises(RuntimeError, match="SYNCFUSION_VGGISH_WEIGHTS"):
        evaluate_fad(tmp_path, tmp_path)


def test_evaluate_fad_fewer_than_two_examples_raises(tmp_path):
    from syncfusion_amd.fad import VGGish, evaluate_fad
    from syncfusion_amd.generation import save_wav

    gen, gt = tmp_path / "gen", tmp_path / "gt"
    gen.mkdir(), gt.mkdir()
    for i in range(3):
        save_wav(gt / f"{i}.wav", 0.1 * torch.randn(1, 16000), 16000)            # one example each
    save_wav(gen / "a.wav", 0.1 * torch.randn(1, 16000), 16000)                  # one example
    save_wav(gen / "b.wav", 0.1 * torch.randn(2, 15599), 16000)                  # one frame short of an example: contributes nothing
    model = VGGish(narrow_config())
    with pytest.raises(ValueError, match="1 VGGish example"):
        evaluate_fad(gen, gt, model=model)
    with pytest.raises(ValueError, match="0 VGGish example"):
        evaluate_fad(gt, tmp_path, model=model)                                  # a directory without wav files


def test_metrics_csv_shape(tmp_path):
    from syncfusion_amd.fad import write_metrics_csv

    write_metrics_csv(tmp_path / "metrics.csv", 1.25)
    assert (tmp_path / "metrics.csv").read_text() == ",FAD\n0,1.25\n"


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_fad_symbols_declared_bound_and_exported():
    import syncfusion_amd
    from syncfusion_amd import _lib

    header = open(os.path.join(ROOT, "include", "syncfusion_amd.h")).read()
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in FAD_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/syncfusion_amd.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    for name in ("fad", "VGGish", "VGGishConfig", "embedding_statistics", "frechet_distance", "evaluate_fad"):
        assert name in syncfusion_amd.__all__ and hasattr(syncfusion_amd, name)
    assert "main/evaluation.py:7-28" in header and "script/evaluate_diffusion.py:31-36" in header      # the declarations cite what they replace


def _create_framed(lib, n_fft=512, win=400, hop=160, n_mels=64, first=None, count=None, weights=None, out=True):
    from syncfusion_amd.audio_features import compact_filterbank
    from syncfusion_amd.fad import vggish_mel_matrix

    f, c, w = compact_filterbank(vggish_mel_matrix().T)
    f = f if first is None else np.asarray(first, dtype=np.int32)
    c = c if count is None else np.asarray(count, dtype=np.int32)
    h = C.c_void_p()
    rc = lib.sf_audio_features_create_framed(n_fft, win, hop, n_mels, f.ctypes.data if first is not False else None, c.ctypes.data,
                                             w.ctypes.data if weights is not False else None, int(w.size), C.byref(h) if out else None)
    return rc, h.value


def test_framed_create_refusals_need_no_device():
    from syncfusion_amd import _lib

    lib = _lib.load()
    rc, h = _create_framed(lib)
    assert rc == 0 and h
    # a framed handle is refused by the centred entry points, and the other way round (before any HIP call: wav is a null pointer)
    assert lib.sf_audio_features_workspace_bytes(h, 1, 16000) > 0
    assert lib.sf_logmel_examples_forward(h, None, 1, 16000, 96, 0.01, None, None, None) == 1
    lib.sf_audio_features_destroy(h)
    assert _create_framed(lib, out=False)[0] == 1                    # null pointers
    assert _create_framed(lib, first=False)[0] == 1
    assert _create_framed(lib, weights=False)[0] == 1
    from syncfusion_amd.audio_features import compact_filterbank
    from syncfusion_amd.fad import vggish_mel_matrix

    _, count, _ = compact_filterbank(vggish_mel_matrix().T)
    empty = count.copy()
    empty[5] = 0
    rc, h = _create_framed(lib, count=empty)                         # an empty band
    assert rc == 1 and not h and b"empty" in lib.sf_last_error()
    rc, h = _create_framed(lib, n_fft=500)                           # FFT length not a power of two
    assert rc == 1 and not h and b"power of two" in lib.sf_last_error()
    rc, h = _create_framed(lib, win=513)                             # window longer than the FFT
    assert rc == 1 and not h and b"window" in lib.sf_last_error()
    assert _create_framed(lib, win=0)[0] == 1 and _create_framed(lib, hop=0)[0] == 1


def test_engine_and_op_refusals_need_no_device():
    from syncfusion_amd import _lib

    lib = _lib.load()
    stages = np.asarray([8, 0], dtype=np.int32)
    fc = np.asarray([24], dtype=np.int32)
    h = C.c_void_p()
    null4 = (C.c_void_p * 4)()
    assert lib.sf_vggish_create(2, stages.ctypes.data, 1, fc.ctypes.data, 96, 64, 0, None, null4, null4, null4, None, C.byref(h)) == 1
    assert lib.sf_vggish_create(2, stages.ctypes.data, 1, fc.ctypes.data, 96, 64, 0, null4, null4, null4, null4, None, C.byref(h)) == 2   # null weight
    assert lib.sf_vggish_create(0, stages.ctypes.data, 1, fc.ctypes.data, 96, 64, 0, null4, null4, null4, null4, None, C.byref(h)) == 1
    pools = np.asarray([0, 0, 8], dtype=np.int32)
    assert lib.sf_vggish_create(3, pools.ctypes.data, 1, fc.ctypes.data, 2, 2, 0, null4, null4, null4, null4, None, C.byref(h)) == 3      # 1 x 1 map pooled
    assert not h.value
    assert lib.sf_vggish_workspace_bytes(None, 1) == -1 and lib.sf_vggish_max_examples(None) == -1
    assert lib.sf_vggish_forward(None, None, 1, None, None, None, 0, None) == 1
    assert lib.sf_op_maxpool2x2_cl(None, 1, 4, 4, 8, None, None) == 1
    assert lib.sf_op_moments(None, 2, 24, None, None, None) == 1
