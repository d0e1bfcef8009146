"""CPU suite for the audio front end and the onset-sync evaluation (syncfusion_amd/audio_features.py, evaluation.py, sf_audio_features_*,
sf_logmel_forward, sf_onset_detect): the fp64 restatement (tests/audio_features_ref.py) against ``torch.stft`` in fp64 -- code we did not
write --, the host-built mel filterbank, the peak picker, NMS / matcher / AP on hand-worked onset lists, and the C ABI's symbols, workspace
query and refusals.  No kernel runs here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import audio_features_ref as ref
from helpers import ROOT

AUDIO_SYMBOLS = ("sf_audio_features_create", "sf_audio_features_destroy", "sf_audio_features_workspace_bytes", "sf_logmel_forward", "sf_onset_detect")
LIBROSA_WINDOWS = dict(pre_max=1, post_max=1, pre_avg=4, post_avg=5, wait=1)      # 22050 / 512


# ---- STFT power against torch.stft (fp64) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3000, 10000, 10240, 44100])
@pytest.mark.parametrize("n_fft,hop", [(2048, 512), (1024, 512)])
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_stft_power_matches_torch_stft(pad_mode, n_fft, hop, L):
    x = ref.make_input("bursts", 1, L, seed=3)[0]
    mine = ref.stft_power(x, n_fft, hop, pad_mode)
    X = torch.stft(torch.from_numpy(x).double(), n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64),
                   center=True, pad_mode=pad_mode, normalized=False, onesided=True, return_complex=True)
    theirs = (X.real ** 2 + X.imag ** 2).numpy()
    assert mine.shape == theirs.shape == (n_fft // 2 + 1, 1 + L // hop)
    assert np.abs(mine - theirs).max() <= 1e-10 * theirs.max()


# ---- mel filterbank --------------------------------------------------------------------------------------------------------------------------
FB_CASES = [(2048, 128, "slaney", "slaney"), (1024, 80, "htk", None), (256, 20, "slaney", "slaney"), (1024, 80, "slaney", None), (2048, 128, "htk", "slaney")]


@pytest.mark.parametrize("n_fft,n_mels,scale,norm", FB_CASES)
def test_filterbank_properties(n_fft, n_mels, scale, norm):
    from syncfusion_amd.audio_features import compact_filterbank, mel_filterbank, mel_frequencies

    sr = 22050
    fb = mel_filterbank(sr, n_fft, n_mels, 0.0, None, mel_scale=scale, norm=norm)
    assert fb.shape == (n_mels, n_fft // 2 + 1) and fb.dtype == np.float64 and fb.min() >= 0.0
    f = mel_frequencies(n_mels + 2, 0.0, sr / 2, scale)
    first, count, w = compact_filterbank(fb)
    assert first.dtype == count.dtype == np.int32 and w.dtype == np.float32 and w.size == int(count.sum()) and count.min() >= 1
    off = 0
    for m in range(n_mels):                                   # one contiguous support per filter, nothing outside it
        nz = np.nonzero(fb[m])[0]
        assert np.array_equal(nz, np.arange(first[m], first[m] + count[m]))
        assert np.array_equal(w[off:off + count[m]], fb[m, first[m]:first[m] + count[m]].astype(np.float32))
        off += count[m]
    raw = mel_filterbank(sr, n_fft, n_mels, 0.0, None, mel_scale=scale, norm=None)
    assert raw.max() <= 1.0 + 1e-12
    bins = np.linspace(0, sr / 2, n_fft // 2 + 1)
    interior = (bins >= f[1]) & (bins <= f[-2])              # between the first and the last peak adjacent triangles add up to 1
    assert np.abs(raw[:, interior].sum(axis=0) - 1.0).max() < 1e-12
    if norm == "slaney":
        assert np.allclose(fb, raw * (2.0 / (f[2:] - f[:-2]))[:, None], rtol=1e-14, atol=0)
    assert np.abs(fb - ref.mel_filterbank_ref(sr, n_fft, n_mels, 0.0, sr / 2, scale, norm)).max() <= 1e-12 * fb.max()


def test_mel_scales():
    from syncfusion_amd.audio_features import hz_to_mel, mel_filterbank, mel_to_hz

    assert np.allclose(hz_to_mel([0.0, 200.0, 1000.0], "slaney"), [0.0, 3.0, 15.0], rtol=1e-15)            # linear: hz / (200 / 3)
    assert math.isclose(float(hz_to_mel(6400.0, "slaney")), 15.0 + 27.0, rel_tol=1e-14)                     # log: 27 mels per factor 6.4
    assert math.isclose(float(hz_to_mel(2000.0, "slaney")) - 15.0, math.log(2.0) / (math.log(6.4) / 27.0), rel_tol=1e-14)
    assert math.isclose(float(hz_to_mel(1000.0, "htk")), 2595.0 * math.log10(1.0 + 1000.0 / 700.0), rel_tol=1e-15)
    for scale in ("slaney", "htk"):
        f = np.array([0.0, 55.0, 999.0, 1000.0, 1001.0, 4000.0, 11025.0])
        assert np.allclose(mel_to_hz(hz_to_mel(f, scale), scale), f, rtol=1e-12, atol=1e-9)
    with pytest.raises(ValueError):
        hz_to_mel(1.0, "bark")
    with pytest.raises(ValueError):
        mel_filterbank(22050, 1024, 80, norm="l1")


def test_peak_pick_defaults_follow_librosa():
    from syncfusion_amd.audio_features import peak_pick_defaults

    assert peak_pick_defaults(22050, 512) == LIBROSA_WINDOWS
    assert peak_pick_defaults(44100, 256) == dict(pre_max=5, post_max=1, pre_avg=17, post_avg=18, wait=5)


# ---- peak picker on hand-written envelopes ---------------------------------------------------------------------------------------------------
def test_peak_pick_edge_clipped_windows():
    assert ref.peak_pick(np.array([5.0, 0, 0, 0, 0, 0, 0, 0]), delta=0.07, **LIBROSA_WINDOWS)[0] == [0]      # windows cut at the left edge
    assert ref.peak_pick(np.array([0.0, 0, 0, 0, 0, 0, 0, 3.0]), delta=0.07, **LIBROSA_WINDOWS)[0] == [7]    # ... and at the right edge
    # frame 1 is lower than frame 0 and frame 2 has no left neighbour above it: [max(0, n - 1), n + 1) is what is compared
    assert ref.peak_pick(np.array([4.0, 1.0, 1.5, 0, 0, 0, 0, 0, 0, 0, 0, 8.0]), delta=0.07, **{**LIBROSA_WINDOWS, "wait": 0})[0] == [0, 2, 11]


def test_peak_pick_plateau_and_wait():
    e = np.array([0.0, 0, 2, 2, 0, 0, 0, 0])
    assert ref.peak_pick(e, delta=0.07, **LIBROSA_WINDOWS)[0] == [2]                      # frame 3 equals its window maximum too, wait = 1 drops it
    assert ref.peak_pick(e, delta=0.07, **{**LIBROSA_WINDOWS, "wait": 0})[0] == [2, 3]
    ramp = np.array([0.0, 1, 2, 3, 0, 0, 0, 0, 0, 0])
    assert ref.peak_pick(ramp, delta=0.07, **{**LIBROSA_WINDOWS, "wait": 0})[0] == [2, 3]   # frame 1: 1/3 < mean 1/3 + delta
    assert ref.peak_pick(ramp, delta=0.07, **LIBROSA_WINDOWS)[0] == [2]
    far = np.array([0.0, 0, 3, 0, 0, 3, 0, 0, 0, 0, 0, 0])
    assert ref.peak_pick(far, delta=0.07, **{**LIBROSA_WINDOWS, "wait": 2})[0] == [2, 5]     # 5 - 2 > 2
    assert ref.peak_pick(far, delta=0.07, **{**LIBROSA_WINDOWS, "wait": 3})[0] == [2]


def test_peak_pick_zero_envelope_and_exact_delta():
    onsets, margin = ref.peak_pick(np.zeros(12), delta=0.07, **LIBROSA_WINDOWS)
    assert onsets == [] and margin == float("inf")
    e = np.array([0.0, 0, 0, 0, 1, 0, 0, 0, 0, 0])
    w = dict(pre_max=1, post_max=1, pre_avg=4, post_avg=4, wait=1)                          # mean over 8 frames = 1/8, exact in binary
    onsets, margin = ref.peak_pick(e, delta=0.875, **w)
    assert onsets == [4] and margin == 0.0                                                  # x >= mean + delta holds with equality
    assert ref.peak_pick(e, delta=0.875 + 2.0 ** -40, **w)[0] == []


def test_peak_pick_margin_is_the_distance_to_a_flip():
    e = np.array([0.0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0, 0.5, 0, 0, 0, 0])
    onsets, margin = ref.peak_pick(e, delta=0.3, **LIBROSA_WINDOWS)
    assert onsets == [4, 10]
    assert math.isclose(margin, 0.5 - 0.5 / 9 - 0.3, rel_tol=1e-12)                         # frame 10: mean over [6, 15) = 0.5 / 9


# ---- NMS, matcher, AP on hand-worked lists (both restatements) ---------------------------------------------------------------------------------
def _both_nms(onsets, conf):
    from syncfusion_amd.evaluation import onset_nms

    a, b = onset_nms(onsets, conf), ref.nms_ref(onsets, conf)
    assert a == b
    return a


def _both_match(tar, gen, conf, strength, delta=0.1):
    from syncfusion_amd.evaluation import match_onsets

    a = match_onsets(tar, gen, conf, strength, delta)
    b = ref.match_ref(tar, gen, dict(zip(gen, conf)), dict(zip(gen, strength)), delta)
    assert a[0] == b[0] and a[2] == b[2] and (a[1] == pytest.approx(b[1], abs=1e-15) or (math.isnan(a[1]) and math.isnan(b[1])))
    return a


def test_nms_removes_the_weaker_neighbour_and_keeps_the_reference_order_dependence():
    assert _both_nms([10000, 10500, 30000], [0.9, 0.4, 0.5]) == [10000, 30000]            # 500 samples < 0.05 s = 1102.5
    assert _both_nms([10000, 10500, 30000], [0.4, 0.9, 0.5]) == [10500, 30000]
    assert _both_nms([10000, 11200], [0.9, 0.4]) == [10000, 11200]                         # 1200 samples apart: both stay
    # 10900 is 900 samples from 10000, but it follows the deleted 10500 in the list the reference walks while deleting: never examined
    assert _both_nms([10000, 10500, 10900], [0.9, 0.4, 0.3]) == [10000, 10900]
    # ... it then runs as its own survivor and has nothing left to drop
    assert _both_nms([10000, 10500, 10900, 11000], [0.9, 0.4, 0.3, 0.2]) == [10000, 10900]
    assert _both_nms([10000, 10500], [0.5, 0.5]) == [10500]                                # equal confidences: the later onset goes first
    assert _both_nms([], []) == []


def test_match_generated_onset_inside_two_target_windows():
    acc, ap, flags = _both_match([10000, 12000], [11000], [0.8], [0.5])
    assert (acc, ap, flags) == (0.5, 1.0, [1])          # the first target takes it; nothing is free afterwards, the second is never scored


def test_match_more_targets_than_generated_onsets_breaks_early():
    acc, ap, flags = _both_match([1000, 20000, 30000], [20100], [0.6], [0.6])
    # target 1000: a positive scored 0; 20000: hit; then the list is empty and 30000 is not scored: labels [1, 1], scores [0, 0.6]
    assert acc == pytest.approx(1 / 3) and ap == 1.0 and flags == [1]


def test_match_false_positive_and_strength_choice():
    acc, ap, flags = _both_match([10000], [10100, 20000], [0.5, 0.9], [0.5, 0.9])
    assert (acc, ap, flags) == (1.0, 0.5, [1, 0])       # scores (0.9, negative), (0.5, positive): recall 1 at precision 1/2
    # two candidates in the window (1500 apart, so the NMS keeps both): the larger w[o] wins, not the nearer one; a tie goes to the later
    acc, ap, flags = _both_match([10000], [9000, 10500], [0.3, 0.3], [0.2, 0.1])
    assert flags == [1, 0] and acc == 1.0 and ap == 0.5          # equal scores are one threshold: 1 true positive of 2 at recall 1
    acc, ap, flags = _both_match([10000], [9000, 10500], [0.3, 0.4], [0.2, 0.2])
    assert flags == [0, 1] and ap == 1.0
    acc, ap, flags = _both_match([5000, 10000], [9000], [0.7], [0.7], delta=0.1)
    assert (acc, flags) == (0.5, [1]) and ap == 1.0      # target 5000 missed (score 0), 10000 hit: all positives


def test_average_precision_ties_and_no_positive():
    from syncfusion_amd.evaluation import average_precision
    from onset_metrics_ref import average_precision as ap_ref

    y, s = [1, 0, 1, 0, 1], [0.9, 0.9, 0.4, 0.3, 0.0]
    # thresholds 0.9: tp 1 of 2, recall 1/3; 0.4: tp 2 of 3, recall 2/3; 0.3: no recall step; 0.0: tp 3 of 5
    want = (1 / 3) * (1 / 2) + (1 / 3) * (2 / 3) + (1 / 3) * (3 / 5)
    assert average_precision(y, s) == pytest.approx(want, abs=1e-15) and ap_ref(np.array(y), np.array(s)) == pytest.approx(want, abs=1e-15)
    assert math.isnan(average_precision([0, 0], [0.3, 0.2])) and average_precision([1, 1], [0.0, 0.5]) == 1.0


def _file(onsets, conf=None, strength=None):
    n = len(onsets)
    return {"onsets": np.asarray(onsets, dtype=np.int64), "confidence": np.asarray(conf if conf is not None else [0.5] * n, dtype=np.float32),
            "strength": np.asarray(strength if strength is not None else [0.5] * n, dtype=np.float32)}


def _both_score(tar, gen, **kw):
    from syncfusion_amd.evaluation import score_file

    a = score_file(tar, gen, **kw)
    b = ref.evaluate_ref({"x.wav": gen}, {"x.wav": tar} if tar is not None else {}, **kw)["per_file"]["x.wav"]
    assert a["count_match"] == b["count_match"] and a["acc"] == pytest.approx(b["acc"], abs=1e-15) and a["ap"] == pytest.approx(b["ap"], abs=1e-15)
    return a["count_match"], a["acc"], a["ap"]


def test_score_file_empty_side_and_remove_head():
    assert _both_score(_file([]), _file([1000])) == (False, 0.0, 0.0)
    assert _both_score(_file([1000]), _file([])) == (False, 0.0, 0.0)
    assert _both_score(None, _file([1000])) == (False, 0.0, 0.0)                            # no target file of that name
    assert _both_score(_file([1000, 30000]), _file([1100, 30100])) == (True, 1.0, 1.0)
    assert _both_score(_file([1000, 30000]), _file([30100])) == (False, 0.5, 1.0)
    # remove_head = 0.5 s = 11025 samples, applied to both sides after the emptiness test
    assert _both_score(_file([1000, 30000]), _file([30100]), remove_head=0.5) == (True, 1.0, 1.0)
    assert _both_score(_file([1000, 30000]), _file([1100]), remove_head=0.5) == (False, 0.0, 1.0)     # a missed positive scored 0: AP 1, acc 0
    assert _both_score(_file([1000]), _file([1100, 30000]), remove_head=0.5) == (False, 0.0, 0.0)     # no positive left: AP undefined -> 0
    assert _both_score(_file([1000]), _file([1100]), remove_head=0.5) == (True, 0.0, 0.0)             # nothing left on either side


def test_score_file_multi_delta():
    # 3000 samples = 0.136 s apart: missed at delta 0.1 (acc 0, AP 1/2: the free generated onset outranks the missed positive), hit at 0.15, 0.2
    got = _both_score(_file([10000]), _file([13000]), delta=0.2, multi_delta=True)
    assert got[0] is True and got[1] == pytest.approx(2 / 3) and got[2] == pytest.approx((0.5 + 1 + 1) / 3)
    assert _both_score(_file([10000]), _file([13000]), delta=0.1) == (True, 0.0, 0.5)


def test_summary_line_format():
    from syncfusion_amd.evaluation import summary_line

    line = summary_line({"onset_num_acc": 0.5, "detection_acc": 1 / 3, "detection_ap": 0.98765})
    assert line == "#onset acc: 0.5000, detection acc: 0.3333, detection ap: 0.9877"


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------
def _create(lib, n_fft=2048, hop=512, n_mels=128, pad=0, first=None, count=None, weights=None, n_weights=None):
    from syncfusion_amd.audio_features import compact_filterbank, mel_filterbank

    f, c, w = compact_filterbank(mel_filterbank(22050, max(n_fft, 2), max(n_mels, 1)))
    first, count, weights = f if first is None else first, c if count is None else count, w if weights is None else weights
    h = C.c_void_p()
    rc = lib.sf_audio_features_create(n_fft, hop, n_mels, pad, first.ctypes.data if first is not False else None, count.ctypes.data, weights.ctypes.data,
                                      int(weights.size) if n_weights is None else n_weights, C.byref(h))
    return rc, h.value


def test_audio_symbols_declared_bound_and_exported():
    import syncfusion_amd
    from syncfusion_amd import _lib

    header = open(os.path.join(ROOT, "include", "syncfusion_amd.h")).read()
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in AUDIO_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/syncfusion_amd.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    for name in ("audio_features", "evaluation", "MelSpectrogram", "mel_filterbank", "onset_detect", "onset_strength", "evaluate_onsets"):
        assert name in syncfusion_amd.__all__ and hasattr(syncfusion_amd, name)
    assert "script/evaluate_onset.py:30" in header and "main/module_diffusion.py:120-152" in header      # each declaration cites what it replaces


def test_workspace_query_is_monotone():
    from syncfusion_amd import _lib

    lib = _lib.load()
    rc, h = _create(lib)
    assert rc == 0 and h
    ws = lib.sf_audio_features_workspace_bytes
    assert ws(None, 1, 3000) == -1 and ws(h, 0, 3000) == -1 and ws(h, 1, 0) == -1
    T = 1 + 3000 // 512
    assert ws(h, 1, 3000) >= 4 * (128 * T + 2 * T)             # the mel plane, the normalised envelope and the peak flags
    for B in (1, 2, 5, 64):
        for L in (1, 511, 512, 3000, 10000, 10240, 44100):
            assert ws(h, B + 1, L) >= ws(h, B, L) > 0 and ws(h, B, L + 512) >= ws(h, B, L) and ws(h, B, L + 1) >= ws(h, B, L)
    lib.sf_audio_features_destroy(h)


def test_create_refuses_bad_configurations():
    from syncfusion_amd import _lib

    lib = _lib.load()
    SF_ERR_INVALID = 1
    for n_fft in (0, 128, 1000, 3000, 8192):
        assert _create(lib, n_fft=n_fft) == (SF_ERR_INVALID, None) and b"n_fft" in lib.sf_last_error()
    assert _create(lib, hop=0) == (SF_ERR_INVALID, None) and b"hop" in lib.sf_last_error()
    assert _create(lib, n_mels=0) == (SF_ERR_INVALID, None) and b"n_mels" in lib.sf_last_error()
    assert _create(lib, pad=2) == (SF_ERR_INVALID, None)
    assert _create(lib, first=False) == (SF_ERR_INVALID, None) and b"null" in lib.sf_last_error()
    from syncfusion_amd.audio_features import compact_filterbank, mel_filterbank

    f, c, w = compact_filterbank(mel_filterbank(22050, 2048, 128))
    empty = c.copy()
    empty[7] = 0
    assert _create(lib, count=empty) == (SF_ERR_INVALID, None) and b"filter 7 has an empty bin range" in lib.sf_last_error()
    outside = f.copy()
    outside[127] = 1025
    assert _create(lib, first=outside) == (SF_ERR_INVALID, None) and b"outside" in lib.sf_last_error()
    assert _create(lib, n_weights=int(w.size) - 1) == (SF_ERR_INVALID, None)
    for n_fft in (256, 512, 1024, 2048, 4096):              # every size in range is taken (host-only: no device needed)
        f2, c2, w2 = compact_filterbank(mel_filterbank(22050, n_fft, 20))
        rc, h = _create(lib, n_fft=n_fft, n_mels=20, first=f2, count=c2, weights=w2)
        assert rc == 0 and h
        lib.sf_audio_features_destroy(h)
    # a filterbank with a filter narrower than the bin spacing reaches the library as an empty range and is refused there
    from syncfusion_amd.audio_features import FrontEnd

    with pytest.raises(_lib.SyncFusionAmdError, match="empty bin range"):
        FrontEnd(22050, 256, 64, 128)


def test_calls_refuse_bad_arguments_without_a_device():
    from syncfusion_amd import _lib

    lib = _lib.load()
    INVALID, SHAPE, WORKSPACE = 1, 3, 5
    rc, h = _create(lib)
    rcr, hr = _create(lib, pad=1)
    assert rc == 0 and rcr == 0
    buf = torch.zeros(1 << 16, dtype=torch.float32)
    p, big = buf.data_ptr(), 1 << 40
    need = lib.sf_audio_features_workspace_bytes(h, 1, 3000)
    lm, od = lib.sf_logmel_forward, lib.sf_onset_detect
    win = (1, 1, 1, 4, 5, 1)                                  # lag, pre_max, post_max, pre_avg, post_avg, wait
    assert lm(None, p, 1, 3000, 1e-10, 80.0, p, p, p, big, None) == INVALID and b"null" in lib.sf_last_error()
    assert lm(h, None, 1, 3000, 1e-10, 80.0, p, p, p, big, None) == INVALID and b"null" in lib.sf_last_error()
    assert lm(h, p, 1, 3000, 1e-10, 80.0, None, None, p, big, None) == INVALID and b"null" in lib.sf_last_error()
    assert lm(h, p, 0, 3000, 1e-10, 80.0, p, p, p, big, None) == INVALID
    assert lm(h, p, 1, 0, 1e-10, 80.0, p, p, p, big, None) == INVALID
    assert lm(h, p, 1, 3000, 1e-10, 80.0, p, p, None, big, None) == WORKSPACE and b"workspace" in lib.sf_last_error()
    assert lm(h, p, 1, 3000, 1e-10, 80.0, p, p, p, need - 1, None) == WORKSPACE and str(need).encode() in lib.sf_last_error()
    assert lm(hr, p, 1, 1024, 1e-10, 80.0, p, p, p, big, None) == SHAPE and b"reflect" in lib.sf_last_error()      # L <= n_fft / 2
    assert lm(hr, p, 1, 1, 1e-10, 80.0, p, p, p, big, None) == SHAPE
    assert lm(h, p, 1, 3000, 0.0, 80.0, p, p, p, big, None) == INVALID and lm(h, p, 1, 3000, 1e-10, -1.0, p, p, p, big, None) == INVALID
    ok = dict(envelope=p, count=p, positions=p, confidence=p, strength=p)
    for missing in ok:
        a = dict(ok, **{missing: None})
        assert od(h, p, 1, 3000, 1e-10, 80.0, *win, 0.3, 1102, 6, a["envelope"], a["count"], a["positions"], a["confidence"], a["strength"], p, big,
                  None) == INVALID and b"null" in lib.sf_last_error()
    full = (p, p, p, p, p)
    assert od(None, p, 1, 3000, 1e-10, 80.0, *win, 0.3, 1102, 6, *full, p, big, None) == INVALID
    assert od(h, None, 1, 3000, 1e-10, 80.0, *win, 0.3, 1102, 6, *full, p, big, None) == INVALID
    assert od(h, p, 0, 3000, 1e-10, 80.0, *win, 0.3, 1102, 6, *full, p, big, None) == INVALID
    assert od(h, p, 1, 0, 1e-10, 80.0, *win, 0.3, 1102, 6, *full, p, big, None) == INVALID
    assert od(h, p, 1, 3000, 1e-10, 80.0, *win, 0.3, 1102, 6, *full, p, need - 1, None) == WORKSPACE
    assert od(h, p, 1, 3000, 1e-10, 80.0, *win, 0.3, 1102, 6, *full, None, big, None) == WORKSPACE
    assert od(hr, p, 1, 1024, 1e-10, 80.0, *win, 0.3, 1102, 6, *full, p, big, None) == SHAPE
    for bad in ((0, 1, 1, 4, 5, 1), (1, -1, 1, 4, 5, 1), (1, 1, 0, 4, 5, 1), (1, 1, 1, -1, 5, 1), (1, 1, 1, 4, 0, 1), (1, 1, 1, 4, 5, -1)):
        assert od(h, p, 1, 3000, 1e-10, 80.0, *bad, 0.3, 1102, 6, *full, p, big, None) == INVALID
    assert od(h, p, 1, 3000, 1e-10, 80.0, *win, 0.3, 0, 6, *full, p, big, None) == INVALID          # conf_interval
    assert od(h, p, 1, 3000, 1e-10, 80.0, *win, 0.3, 1102, 0, *full, p, big, None) == INVALID       # capacity
    lib.sf_audio_features_destroy(h)
    lib.sf_audio_features_destroy(hr)


def test_device_front_end_has_no_cpu_path():
    from syncfusion_amd import MelSpectrogram, onset_detect, onset_strength
    from syncfusion_amd._lib import SyncFusionAmdError

    x = torch.zeros(2, 3000)
    with pytest.raises(SyncFusionAmdError):
        MelSpectrogram(to_db=True)(x)
    with pytest.raises(SyncFusionAmdError):
        onset_detect(x)
    with pytest.raises(SyncFusionAmdError):
        onset_strength(x)
    with pytest.raises(NotImplementedError):
        MelSpectrogram(power=1.0)


def test_reference_inputs_are_reproducible_and_batch_independent():
    for kind in ref.KINDS:
        a, b = ref.make_input(kind, 5, 3000), ref.make_input(kind, 1, 3000)
        assert a.dtype == np.float32 and a.shape == (5, 3000) and np.array_equal(a[:1], b)
    assert not ref.make_input("zeros", 2, 100).any()
    assert (ref.make_input("clicks", 3, 5000) != 0).sum(axis=1).tolist() == [2, 2, 2]
