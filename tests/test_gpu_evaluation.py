"""End to end on the GPU: ``evaluate_onsets`` and ``tools/evaluate_onset.py`` on two directories of wav files against the fp64 pipeline of
tests/audio_features_ref.py run on the same arrays (detector and scoring both restated there)."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import audio_features_ref as ref
from helpers import ROOT

pytestmark = pytest.mark.gpu

SR, L = 22050, 44100
A = dict(n_fft=2048, hop=512, pad_mode="constant", pre_max=1, post_max=1, pre_avg=4, post_avg=5, wait=1)
TARGET_BURSTS = [[4000, 16000, 30000], [6000, 21000], [3000, 13000, 24000, 36000], [9000, 26000, 38000], [5000, 18000, 33000], [8000, 22000]]


def _clip(i, positions):
    return ref.burst_clip(np.random.default_rng([11, i]), L, positions=positions).astype(np.float32)


def clips():
    """6 targets; generated = the targets with their bursts shifted by 0, 0.05 and 0.15 s, one burst removed, one added, and a silent file."""
    tar = {f"clip{i}.wav": _clip(i, p) for i, p in enumerate(TARGET_BURSTS)}
    shift = lambda p, s: [q + int(s * SR) for q in p]      # noqa: E731
    gen_pos = [TARGET_BURSTS[0], shift(TARGET_BURSTS[1], 0.05), shift(TARGET_BURSTS[2], 0.15), TARGET_BURSTS[3][:-1], TARGET_BURSTS[4] + [40000]]
    gen = {f"clip{i}.wav": _clip(i, p) for i, p in enumerate(gen_pos)}
    gen["clip5.wav"] = np.zeros(L, dtype=np.float32)
    return tar, gen


def detect_ref(wavs):
    from syncfusion_amd.audio_features import mel_filterbank

    fb = mel_filterbank(SR, 2048, 128)
    return {name: ref.detect(w, fb, delta=0.3, ci=int(0.05 * SR), **A) for name, w in wavs.items()}


def write_dir(path, wavs, rate=SR):
    from syncfusion_amd.generation import save_wav

    os.makedirs(path, exist_ok=True)
    for name, w in wavs.items():
        save_wav(os.path.join(path, name), torch.from_numpy(w)[None], rate)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tar, gen = clips()
    root = tmp_path_factory.mktemp("onset_eval")
    write_dir(root / "tar", tar)
    write_dir(root / "gen", gen)
    dt, dg = detect_ref(tar), detect_ref(gen)
    margins = [d["margin"] for d in list(dt.values()) + list(dg.values())]
    assert min(margins) >= 1e-3, f"a reference decision is {min(margins):.2e} from flipping: these clips cannot be compared exactly"
    assert all(d["onsets"].size >= 2 for d in dt.values()) and dg["clip5.wav"]["onsets"].size == 0
    return str(root / "gen"), str(root / "tar"), dg, dt


@pytest.mark.parametrize("kw", [dict(), dict(delta=0.2), dict(delta=0.2, multi_delta=True), dict(remove_head=0.3), dict(delta=0.05)], ids=str)
def test_evaluate_onsets_equals_the_fp64_pipeline(cuda, case, kw):
    from syncfusion_amd import evaluate_onsets

    gen_dir, tar_dir, dg, dt = case
    got = evaluate_onsets(gen_dir, tar_dir, batch_size=4, device=cuda, **kw)
    want = ref.evaluate_ref(dg, dt, **kw)
    assert list(got["per_file"]) == sorted(dg)
    for name, w in want["per_file"].items():
        g = got["per_file"][name]
        print(name, g, w)
        assert (g["n_tar"], g["n_gen"], g["count_match"]) == (w["n_tar"], w["n_gen"], w["count_match"]) and g["resampled_from"] is None
        assert abs(g["acc"] - w["acc"]) <= 1e-6 and abs(g["ap"] - w["ap"]) <= 1e-6
    for key in ("onset_num_acc", "detection_acc", "detection_ap"):
        assert abs(got[key] - want[key]) <= 1e-6, key
    assert got["per_file"]["clip5.wav"] == {"count_match": False, "acc": 0.0, "ap": 0.0, "n_tar": dt["clip5.wav"]["onsets"].size, "n_gen": 0,
                                            "resampled_from": None}
    if not kw:
        assert 0.0 < want["detection_acc"] < 1.0 and 0.0 < want["onset_num_acc"] < 1.0      # the set exercises hits and misses


def test_command_line_summary_parses_to_the_same_values(cuda, case, capsys):
    gen_dir, tar_dir, dg, dt = case
    spec = importlib.util.spec_from_file_location("evaluate_onset_tool", os.path.join(ROOT, "tools", "evaluate_onset.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for argv, kw in ((["--gen_dir", gen_dir, "--tar_dir", tar_dir], {}),
                     (["--gen_dir", gen_dir, "--tar_dir", tar_dir, "--delta", "0.2", "--multi_delta", "--remove_head", "0.3"],
                      dict(delta=0.2, multi_delta=True, remove_head=0.3))):
        capsys.readouterr()
        assert tool.main(argv) == 0
        line = capsys.readouterr().out.strip().splitlines()[-1]
        m = re.fullmatch(r"#onset acc: (\d\.\d{4}), detection acc: (\d\.\d{4}), detection ap: (\d\.\d{4})", line)
        assert m, line
        want = ref.evaluate_ref(dg, dt, **kw)
        for text, key in zip(m.groups(), ("onset_num_acc", "detection_acc", "detection_ap")):
            assert abs(float(text) - want[key]) <= 0.5e-4 + 1e-6, (key, line)


def test_file_at_another_rate_goes_through_the_resampler(cuda, tmp_path):
    from syncfusion_amd import evaluate_onsets

    n = 2 * 48000
    x = ref.burst_clip(np.random.default_rng(5), n, positions=[20000, 60000]).astype(np.float32)
    write_dir(tmp_path / "tar", {"a.wav": x}, rate=48000)
    write_dir(tmp_path / "gen", {"a.wav": x}, rate=48000)
    write_dir(tmp_path / "gen", {"b.wav": _clip(0, TARGET_BURSTS[0])})          # no target of that name
    got = evaluate_onsets(str(tmp_path / "gen"), str(tmp_path / "tar"), device=cuda)
    a = got["per_file"]["a.wav"]
    assert a["resampled_from"] == 48000 and a["n_tar"] == a["n_gen"] >= 2 and a["count_match"] is True and 0.0 < a["acc"] <= 1.0 and a["ap"] > 0.0
    assert got["per_file"]["b.wav"] == {"count_match": False, "acc": 0.0, "ap": 0.0, "n_tar": 0, "n_gen": got["per_file"]["b.wav"]["n_gen"],
                                        "resampled_from": None}
    assert got["onset_num_acc"] == 0.5 and got["detection_acc"] == a["acc"] / 2 and got["detection_ap"] == a["ap"] / 2
