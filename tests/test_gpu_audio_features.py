"""GPU suite for the audio front end (syncfusion_amd/csrc/audio_features.hip through sf_logmel_forward / sf_onset_detect) against the fp64
restatement in tests/audio_features_ref.py.

Configurations: A = librosa's onset front end (n_fft 2048, hop 512, 128 slaney mels, zero padding), B = SampleLogger's (n_fft 1024, hop 512,
80 htk mels, reflect padding), C = one tiny configuration (n_fft 256, hop 64, 20 mels) that takes its scale and padding from B (htk,
reflect): the reflected edge then spans a different share of a frame than in B.  Lengths: 3000 (T = 6, every frame of A holds padding),
10000 (no multiple of the hop), 10240 (a multiple: the last frame is all right-hand padding), 44100.  B = 1 and B = 5.

Gates (fixed by the fp32 error of a plain FFT pipeline measured against fp64, 6-14 x above it): dB plane <= 5e-3 dB, un-normalised envelope
<= 2e-4, mel power <= 2e-6 of the plane's maximum.  Onsets, counts and positions are compared exactly wherever every decision of the fp64
detector is at least 1e-3 (normalised-envelope units) from flipping; confidences and w[o] to 1e-6.

Measured on an MI355X (largest over all clips): mel power 5.8e-7 of the maximum, dB 3.0e-3, envelope 3.1e-5 for A and B and 1.97e-4 for C on
the gated tones at L = 44100 -- the one figure near its gate; an fp32 torch.stft restatement of the pipeline gives 1.4e-4 ... 2.3e-4 on the
same clips (bins 80 dB below a tone sit on fp32's rounding floor, and C averages over 20 mels only).  No case is left out by the margin rule.
"""
import functools

import numpy as np
import pytest
import torch

import audio_features_ref as ref
from guards import Guards

pytestmark = pytest.mark.gpu

SR = 22050
CONFIGS = {
    "A": dict(n_fft=2048, hop_length=512, n_mels=128, mel_scale="slaney", norm="slaney", pad_mode="constant"),
    "B": dict(n_fft=1024, hop_length=512, n_mels=80, mel_scale="htk", norm="slaney", pad_mode="reflect"),
    "C": dict(n_fft=256, hop_length=64, n_mels=20, mel_scale="htk", norm="slaney", pad_mode="reflect"),
}
LENGTHS = (3000, 10000, 10240, 44100)
DELTAS = (0.3, 0.07)
NB = 5
DB_GATE, ENV_GATE, MEL_GATE, CONF_GATE, MARGIN = 5e-3, 2e-4, 2e-6, 1e-6, 1e-3
CASES = [(c, L, k) for c in CONFIGS for L in LENGTHS for k in ref.KINDS]


def _front_end(cfg, device):
    from syncfusion_amd.audio_features import front_end

    return front_end(device, SR, **CONFIGS[cfg])


def _windows(cfg):
    from syncfusion_amd.audio_features import peak_pick_defaults

    return peak_pick_defaults(SR, CONFIGS[cfg]["hop_length"])


@functools.lru_cache(maxsize=None)
def reference(cfg, L, kind):
    """fp64 results for the NB clips of a case: one dict per clip, with the detector's output per delta.  Computed once, never modified."""
    from syncfusion_amd.audio_features import mel_filterbank

    c = CONFIGS[cfg]
    fb = mel_filterbank(SR, c["n_fft"], c["n_mels"], 0.0, None, c["mel_scale"], c["norm"])
    wav = ref.make_input(kind, NB, L)
    out = []
    for i in range(NB):
        P = fb @ ref.stft_power(wav[i], c["n_fft"], c["hop_length"], c["pad_mode"])
        db = ref.power_to_db(P)
        env = ref.onset_envelope(db, c["n_fft"], c["hop_length"])
        det = {}
        for delta in DELTAS:
            frames, margin = ref.peak_pick(env, delta=delta, **_windows(cfg))
            onsets = [n * c["hop_length"] for n in frames]
            conf, strength = ref.confidences(wav[i], onsets, int(0.05 * SR)) if onsets else (np.zeros(0), np.zeros(0))
            det[delta] = {"onsets": np.asarray(onsets, dtype=np.int64), "margin": margin, "confidence": conf, "strength": strength}
        out.append({"mel": P, "db": db, "env": env, "det": det})
    return wav, out


def _detect(fe, wav_dev, cfg, delta, capacity=None):
    return fe.detect(wav_dev, delta, capacity=capacity, **_windows(cfg))


@functools.lru_cache(maxsize=None)
def device_results(cfg, L, kind, B):
    wav, _ = reference(cfg, L, kind)
    dev = torch.device("cuda:0")
    fe = _front_end(cfg, dev)
    x = torch.from_numpy(wav[:B]).to(dev)
    res = {"mel": fe.logmel(x, to_db=False).cpu().numpy(), "db": fe.logmel(x, to_db=True).cpu().numpy()}
    for delta in DELTAS:
        r = _detect(fe, x, cfg, delta)
        res[delta] = {"env": r.envelope.cpu().numpy(), "count": r.count.cpu().numpy(), "positions": r.positions.cpu().numpy(),
                      "confidence": r.confidence.cpu().numpy(), "strength": r.strength.cpu().numpy()}
    return res


@pytest.mark.parametrize("cfg,L,kind", CASES)
def test_mel_db_and_envelope_against_fp64(cuda, cfg, L, kind):
    _, want = reference(cfg, L, kind)
    for B in (1, NB):
        got = device_results(cfg, L, kind, B)
        T = 1 + L // CONFIGS[cfg]["hop_length"]
        assert got["mel"].shape == got["db"].shape == (B, CONFIGS[cfg]["n_mels"], T) and got[0.3]["env"].shape == (B, T)
        for i in range(B):
            w = want[i]
            mel_err = np.abs(got["mel"][i] - w["mel"]).max()
            db_err = np.abs(got["db"][i] - w["db"]).max()
            env_err = max(np.abs(got[d]["env"][i] - w["env"]).max() for d in DELTAS)
            print(f"{cfg} L={L} {kind} B={B} clip {i}: mel {mel_err / max(w['mel'].max(), 1e-300):.2e} of max, dB {db_err:.2e}, envelope {env_err:.2e}")
            assert mel_err <= MEL_GATE * w["mel"].max()
            assert db_err <= DB_GATE
            assert env_err <= ENV_GATE
            assert np.array_equal(got[0.3]["env"][i], got[0.07]["env"][i])            # delta does not touch the envelope
            if kind == "zeros":
                assert not got["mel"][i].any() and bool((got["db"][i] == -100.0).all()) and not got[0.3]["env"][i].any()


@pytest.mark.parametrize("cfg,L,kind", CASES)
def test_onsets_against_fp64(cuda, cfg, L, kind):
    _, want = reference(cfg, L, kind)
    hop = CONFIGS[cfg]["hop_length"]
    for B in (1, NB):
        got = device_results(cfg, L, kind, B)
        for delta in DELTAS:
            g = got[delta]
            assert g["positions"].shape == g["confidence"].shape == g["strength"].shape == (B, 1 + L // hop)
            for i in range(B):
                w = want[i]["det"][delta]
                n = int(g["count"][i])
                assert 0 <= n <= 1 + L // hop
                assert bool((g["positions"][i, n:] == -1).all()) and not g["confidence"][i, n:].any() and not g["strength"][i, n:].any()
                if kind == "zeros":
                    assert n == 0
                if w["margin"] < MARGIN:
                    print(f"{cfg} L={L} {kind} delta={delta} clip {i}: left out, margin {w['margin']:.2e}")
                    continue
                assert n == w["onsets"].size, f"clip {i} delta {delta}: {n} onsets, reference {w['onsets'].size} (margin {w['margin']:.2e})"
                assert np.array_equal(g["positions"][i, :n], w["onsets"])
                if n:
                    assert np.abs(g["confidence"][i, :n] - w["confidence"]).max() <= CONF_GATE
                    assert np.abs(g["strength"][i, :n] - w["strength"]).max() <= CONF_GATE


def test_margin_rule_leaves_out_at_most_one_case_in_ten():
    """Host only: which (configuration, length, input, delta, clip) cases the exact comparison above skips, and that some onsets are found."""
    total = left_out = with_onsets = 0
    smallest = float("inf")
    for cfg, L, kind in CASES:
        if kind == "zeros":
            continue
        _, want = reference(cfg, L, kind)
        for w in want:
            for delta in DELTAS:
                total += 1
                left_out += w["det"][delta]["margin"] < MARGIN
                with_onsets += w["det"][delta]["onsets"].size > 0
                smallest = min(smallest, w["det"][delta]["margin"])
    print(f"{left_out} of {total} cases left out, smallest margin {smallest:.2e}, {with_onsets} cases with onsets")
    assert left_out * 10 <= total
    assert with_onsets * 2 >= total


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("L", [3000, 10000])
def test_clip_of_a_batch_is_bit_equal_to_the_clip_alone(cuda, cfg, L):
    wav, _ = reference(cfg, L, "bursts")
    fe = _front_end(cfg, cuda)
    batch = device_results(cfg, L, "bursts", NB)
    for i in range(NB):
        x = torch.from_numpy(wav[i:i + 1]).to(cuda)
        assert np.array_equal(fe.logmel(x, to_db=False).cpu().numpy()[0], batch["mel"][i])
        assert np.array_equal(fe.logmel(x, to_db=True).cpu().numpy()[0], batch["db"][i])
        r = _detect(fe, x, cfg, 0.07)
        for name, t in (("env", r.envelope), ("count", r.count), ("positions", r.positions), ("confidence", r.confidence), ("strength", r.strength)):
            assert np.array_equal(t.cpu().numpy()[0], batch[0.07][name][i]), name


@pytest.mark.parametrize("cfg", ["A", "C"])
def test_non_default_stream_gives_the_same_bits(cuda, cfg):
    L = 10000
    wav, _ = reference(cfg, L, "gated")
    fe = _front_end(cfg, cuda)
    x = torch.from_numpy(wav).to(cuda)
    base = device_results(cfg, L, "gated", NB)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        db = fe.logmel(x, to_db=True)
        r = _detect(fe, x, cfg, 0.3)
    side.synchronize()
    assert np.array_equal(db.cpu().numpy(), base["db"])
    for name, t in (("env", r.envelope), ("count", r.count), ("positions", r.positions), ("confidence", r.confidence), ("strength", r.strength)):
        assert np.array_equal(t.cpu().numpy(), base[0.3][name]), name


@pytest.mark.parametrize("cfg", ["A", "C"])
@pytest.mark.parametrize("L", [3000, 10000])
def test_guard_bands(cuda, cfg, L):
    """Every buffer of both entry points is a guarded one; the workspace has exactly the queried size."""
    from syncfusion_amd import _lib

    lib = _lib.load()
    fe = _front_end(cfg, cuda)
    B, c = 3, CONFIGS[cfg]
    T, M = 1 + L // c["hop_length"], c["n_mels"]
    wav = torch.from_numpy(ref.make_input("bursts", B, L))
    nws = fe.workspace_bytes(B, L)
    st = _lib.stream_ptr(cuda)
    for which in ("mel", "db", "both"):
        with Guards(cuda) as g:
            x = g.inp(wav.to(cuda), name="wav")
            mel = g.out((B, M, T), name="mel_power") if which != "db" else None
            db = g.out((B, M, T), name="db") if which != "mel" else None
            ws = g.ws(nws, name="ws")
            with torch.cuda.device(cuda):
                rc = lib.sf_logmel_forward(fe.handle, x.ptr, B, L, 1e-10, 80.0, mel.ptr if mel else None, db.ptr if db else None, ws.ptr, nws, st)
            assert rc == 0, lib.sf_last_error()
            torch.cuda.synchronize(cuda)
            for t in g.outputs():
                assert not bool(torch.isnan(t.payload).any()), f"{which}: {t.name} keeps fill bytes"
    for cap in (T, 2):
        with Guards(cuda) as g:
            x = g.inp(wav.to(cuda), name="wav")
            env, cnt = g.out((B, T), name="envelope"), g.out((B,), torch.int32, name="count")
            pos, conf, stren = g.out((B, cap), torch.int32, name="positions"), g.out((B, cap), name="confidence"), g.out((B, cap), name="strength")
            ws = g.ws(nws, name="ws")
            w = _windows(cfg)
            with torch.cuda.device(cuda):
                rc = lib.sf_onset_detect(fe.handle, x.ptr, B, L, 1e-10, 80.0, 1, w["pre_max"], w["post_max"], w["pre_avg"], w["post_avg"], w["wait"], 0.07,
                                         int(0.05 * SR), cap, env.ptr, cnt.ptr, pos.ptr, conf.ptr, stren.ptr, ws.ptr, nws, st)
            assert rc == 0, lib.sf_last_error()
            torch.cuda.synchronize(cuda)
            for t in (env, conf, stren):
                assert not bool(torch.isnan(t.payload).any()), f"{t.name} keeps fill bytes"
            assert bool((cnt.payload >= -1).all()) and bool((cnt.payload <= T).all()) and bool((pos.payload >= -1).all()) and bool((pos.payload <= L).all())


def test_capacity_overflow_is_reported_not_truncated(cuda):
    from syncfusion_amd._lib import SyncFusionAmdError

    L = 44100
    wav, want = reference("A", L, "bursts")
    n_ref = [w["det"][0.07]["onsets"].size for w in want]
    assert max(n_ref) >= 2
    fe = _front_end("A", cuda)
    r = _detect(fe, torch.from_numpy(wav).to(cuda), "A", 0.07, capacity=1)
    full = device_results("A", L, "bursts", NB)[0.07]
    count = r.count.cpu().numpy()
    for i in range(NB):
        assert count[i] == (-1 if full["count"][i] > 1 else full["count"][i])
        if full["count"][i] >= 1:
            assert int(r.positions[i, 0]) == full["positions"][i, 0]
    with pytest.raises(SyncFusionAmdError, match="capacity"):
        r.to_host()


def test_python_surface(cuda):
    from syncfusion_amd import MelSpectrogram, onset_detect, onset_strength

    L = 10000
    wav, want = reference("A", L, "bursts")
    x = torch.from_numpy(wav).to(cuda)
    full = device_results("A", L, "bursts", NB)
    rows = onset_detect(x, delta=0.07)                                   # librosa's defaults = configuration A
    assert isinstance(rows, list) and len(rows) == NB
    for i in range(NB):
        assert np.array_equal(rows[i], full[0.07]["positions"][i, :full[0.07]["count"][i]])
    one = onset_detect(x[2], delta=0.07, units="frames")
    assert isinstance(one, np.ndarray) and np.array_equal(one * 512, rows[2])
    assert np.allclose(onset_detect(x[2], delta=0.07, units="time"), rows[2] / SR)
    assert np.array_equal(onset_strength(x.view(1, NB, L)).cpu().numpy()[0], full[0.07]["env"])
    mel = MelSpectrogram(sample_rate=SR, n_fft=2048, hop_length=512, n_mels=128, pad_mode="constant", norm="slaney", mel_scale="slaney", to_db=True)
    assert np.array_equal(mel(x.view(NB, 1, L)).cpu().numpy()[:, 0], full["db"])
    b = CONFIGS["B"]
    logger = MelSpectrogram(sample_rate=SR, n_fft=1024, hop_length=512, n_mels=80, center=True, norm="slaney", to_db=True)      # SampleLogger's call
    assert np.array_equal(logger(torch.from_numpy(reference("B", L, "tone")[0]).to(cuda)).cpu().numpy(), device_results("B", L, "tone", NB)["db"])
    assert b["mel_scale"] == "htk" and b["pad_mode"] == "reflect"
