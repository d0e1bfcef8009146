"""GPU suite for the onset net's test stage (syncfusion_amd/onset_test.py over csrc/onset_test.hip): the table rows against the numpy
restatement of tests/onset_test_ref.py (exact integers), the epoch accumulator against the fp64 weighted mean of what ``balanced_bce`` /
``step_metrics`` return for the same batches (those values themselves are gated in test_gpu_onset_loss.py), ``step()`` without a host
synchronisation, the stage over a frame directory against the reference's file route, the file route against the in-memory hand-off
(``onsets_to_track``), and the FAD ground-truth preparation with device resampling.

Logits lie on the 1/64 grid of ``onset_metrics_ref.grid_logits`` (it contains 0.5 exactly), with rows overwritten by the threshold's edge
cases (``onset_test_ref.special_rows``)."""
from __future__ import annotations

import io
import json
import math
import os
import tarfile
import types
import wave

import numpy as np
import pytest
import torch

import onset_metrics_ref as mref
import onset_test_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (3, 30), (5, 64), (4, 65), (2, 130), (17, 30)]
SENTINEL = -7


def _batch(N, T, seed, density=0.3):
    rng = np.random.default_rng(seed)
    return ref.special_rows(mref.grid_logits(rng, (N, T))), mref.random_labels(rng, (N, T), density)


@pytest.mark.parametrize("N,T", SHAPES)
def test_rows_match_ref(cuda, N, T):
    """``annotation_rows`` (clip0 = 0, capacity = N), then the entry point at clip0 = 3 into sentinel-filled tables of N + 5 rows: the
    batch's rows equal the ref's integers (padding -1), every other row keeps the sentinel."""
    from syncfusion_amd import _lib, annotation_rows

    z, t = _batch(N, T, 100 * N + T)
    want = ref.rows_ref(z, t)
    zd, td = torch.from_numpy(z).to(cuda), torch.from_numpy(t).to(cuda)
    got = annotation_rows(zd, td)
    for g, w in zip(got, want):
        assert g.dtype == torch.int32 and g.is_cuda and np.array_equal(g.cpu().numpy(), w)
    lib = _lib.load()
    clip0, cap = 3, N + 5
    tables = [torch.full(s, SENTINEL, dtype=torch.int32, device=cuda) for s in ((cap,), (cap, T), (cap,), (cap, T))]
    sums = torch.zeros(5, dtype=torch.float64, device=cuda)
    nws = int(lib.sf_op_onset_test_workspace_bytes(N, T))
    ws = torch.empty(nws, dtype=torch.uint8, device=cuda)
    _lib.check(lib.sf_op_onset_test_step(zd.data_ptr(), td.data_ptr(), N, T, 0.5, 0.75, clip0, cap, *[x.data_ptr() for x in tables], sums.data_ptr(),
                                         ws.data_ptr(), nws, _lib.stream_ptr(cuda)), "sf_op_onset_test_step")
    for g, w in zip(tables, want):
        g = g.cpu().numpy()
        assert np.array_equal(g[clip0: clip0 + N], w)
        assert np.all(g[:clip0] == SENTINEL) and np.all(g[clip0 + N:] == SENTINEL)
    assert float(sums[4]) == N


# ---- the epoch accumulator ------------------------------------------------------------------------------------------------------------------
T15 = 30
FIGURES = ("loss/test", "metrics/test/AP", "metrics/test/Acc", "metrics/test/OnsNumAcc")


def _clips(n, first, video="vid"):
    return [dict(video_name=video, start_frame=(first + i) * T15, end_frame=(first + i + 1) * T15, frame_rate=15) for i in range(n)]


def _epoch_batches(one_class=False):
    rng = np.random.default_rng(11)
    out, first = [], 0
    for k, n in enumerate((4, 4, 3)):
        z = mref.grid_logits(rng, (n, T15))
        t = mref.random_labels(rng, (n, T15), 0.25)
        t[0, 0], t[0, 1] = 1.0, 0.0
        z[1], t[1] = -3.0, 0.0                    # a clip whose three predicted onsets are its three labelled ones: OnsNumAcc > 0
        z[1, [2, 9, 20]], t[1, [2, 9, 20]] = 3.0, 1.0
        if one_class and k == 1:
            t[:] = 1.0
        out.append((z, t, _clips(n, first)))
        first += n
    return out


def _run_stage(cuda, batches, out_dir=None, capacity=None):
    from syncfusion_amd import OnsetTestStage

    stage = OnsetTestStage(types.SimpleNamespace(model=None), out_dir, capacity=capacity)
    for z, t, clips in batches:
        stage.step_logits(torch.from_numpy(z).to(cuda), torch.from_numpy(t).to(cuda), clips)
    return stage, stage.finish()


def test_epoch_figures_are_the_weighted_fp64_mean(cuda, tmp_path):
    from syncfusion_amd.onset_loss import balanced_bce, step_metrics

    batches = _epoch_batches()
    sums = np.zeros(5, dtype=np.float64)
    for z, t, clips in batches:
        zd, td = torch.from_numpy(z).to(cuda), torch.from_numpy(t).to(cuda)
        loss = float(balanced_bce(zd, td).double().cpu())
        m = step_metrics(zd, td).cpu().numpy()
        sums += len(clips) * np.array([loss, m[0], m[1], m[2], 1.0], dtype=np.float64)
    # capacity 2: the tables grow 4 -> 8 -> 16 between the steps; the rows written before a growth must survive it
    stage, res = _run_stage(cuda, batches, str(tmp_path / "got"), capacity=2)
    for i, k in enumerate(FIGURES):
        want = sums[i] / sums[4]
        print(f"{k}: stage {res[k]!r} mean {float(want)!r} difference {abs(res[k] - want):.3e}")
        assert math.isfinite(res[k]) and want > 0 and abs(res[k] - want) <= 1e-12 * abs(want)
    assert ref.read_dir(str(tmp_path / "got")) == ref.file_route(str(tmp_path / "ref"), batches)
    _, again = _run_stage(cuda, batches)
    for k in FIGURES:
        assert again[k] == res[k]                                         # bit-equal: one thread adds in a fixed order
    assert again["videos"] == res["videos"]


def test_one_class_batch_makes_ap_and_acc_nan(cuda):
    _, res = _run_stage(cuda, _epoch_batches(one_class=True))
    assert math.isnan(res["metrics/test/AP"]) and math.isnan(res["metrics/test/Acc"])
    assert math.isfinite(res["metrics/test/OnsNumAcc"]) and 0.0 <= res["metrics/test/OnsNumAcc"] <= 1.0


# ---- the net in front ---------------------------------------------------------------------------------------------------------------------
def _seeded_net(seed=7):
    from helpers import seeded_state
    from syncfusion_amd import VideoOnsetNet

    net = VideoOnsetNet(False)
    net.load_state_dict(seeded_state(net, seed))
    return net


def test_step_does_not_synchronise(cuda):
    from syncfusion_amd import OnsetTestStage

    net = _seeded_net().to(cuda).eval()
    g = torch.Generator().manual_seed(3)
    frames = torch.randn(2, 3, 4, 32, 32, generator=g).to(cuda)
    labels = torch.tensor([[1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0]]).to(cuda)

    def clips(k):
        return [dict(video_name="v", start_frame=(2 * k + i) * 4, end_frame=(2 * k + i + 1) * 4, frame_rate=2.0) for i in range(2)]

    stage = OnsetTestStage(net, capacity=2)
    stage.step(frames, labels, clips(0))           # lazy initialisation (library load, engine build, workspace growth) outside the checked calls
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=cuda).item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            stage.step(frames, labels, clips(1))   # grows the tables 2 -> 4
            stage.step(frames, labels, clips(2))   # and 4 -> 8
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this torch build does not honour torch.cuda.set_sync_debug_mode('error'): .item() did not raise under it")
    res = stage.finish()
    assert stage.capacity == 0 and math.isfinite(res["loss/test"]) and len(res["videos"]["v"]["target"]) == 9


def _frame_directory(root):
    """Two videos of 32 x 32 JPEG frames at 4 frames per second: ``va`` 6.2 s (three 2-second chunks), ``vb`` 2.3 s (one)."""
    from PIL import Image

    rs = np.random.RandomState(5)
    for name, frames, duration, times in (("va", 25, 6.2, "0.3,hit\n1.6,hit\n2.2,hit\n4.9,hit\n5.5,hit\n"), ("vb", 10, 2.3, "0.8,hit\n")):
        d = root / name / "frames"
        d.mkdir(parents=True)
        base = rs.randint(0, 256, size=(8, 8, 3))
        for i in range(frames):
            img = np.kron(np.roll(base, i, axis=1), np.ones((4, 4, 1))).astype(np.uint8)
            Image.fromarray(img).save(d / f"{i + 1}.jpg", quality=95)
        (root / name / f"{name}.metadata.json").write_text(json.dumps({"processed": {"video_frame_rate": 4.0, "video_duration": duration}}))
        (root / name / f"{name}.times.csv").write_text(times)


def test_frame_directory_to_annotation_files(cuda, tmp_path):
    """``test_onset_model`` with batch_size 3 (the second batch is ``vb``'s only chunk, the first ends ``va``): files byte-equal to the
    reference's file route on the logits the same net gives for the same batches -- the same logits, so there is no margin."""
    from syncfusion_amd import OnsetModel, onset_test
    from syncfusion_amd import video_chunks as vc

    root = tmp_path / "data"
    _frame_directory(root)
    table = vc.chunk_table(str(root), ["va", "vb"])
    assert [(c["video_name"], c["start_frame"], c["end_frame"]) for c in table] == [("va", 0, 8), ("va", 8, 16), ("va", 16, 24), ("vb", 0, 8)]
    net = _seeded_net().to(cuda).eval()
    first = torch.cat([net(f) for f, _, _ in vc.iter_clips(table, 4, cuda)])
    with torch.no_grad():                     # a seeded net's logits sit on one side of 0.5: centre them so that some frames are onsets
        net.fc[2].bias += 0.5 - first.median()
    model = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, net).to(cuda)
    batches = [(model.model(f).cpu().numpy(), lab.cpu().numpy(), part) for f, lab, part in vc.iter_clips(table, 3, cuda)]
    assert [len(b[2]) for b in batches] == [3, 1]
    n_pred = sum(int((b[0] > 0.5).sum()) for b in batches)
    assert 0 < n_pred < 32, n_pred
    want = ref.file_route(str(tmp_path / "ref"), batches)
    res = onset_test.test_onset_model(model, str(root), ["va", "vb"], str(tmp_path / "w0"), batch_size=3)
    assert ref.read_dir(str(tmp_path / "w0")) == want
    assert want["target"]["va"] == b"0.2500\n1.5000\n2.0000\n4.7500\n5.5000\n" and want["target"]["vb"] == b"0.7500\n"
    assert all(math.isfinite(res[k]) for k in FIGURES) and set(res["videos"]) == {"va", "vb"}
    split = tmp_path / "test.txt"
    split.write_text("va\nvb\n")
    res2 = onset_test.test_onset_model(model, str(root), str(split), str(tmp_path / "w2"), batch_size=3, num_workers=2)
    assert ref.read_dir(str(tmp_path / "w2")) == want and all(res2[k] == res[k] for k in FIGURES)


# ---- file route = in-memory route ---------------------------------------------------------------------------------------------------------
def _add(tf, name, data: bytes):
    ti = tarfile.TarInfo(name)
    ti.size = len(data)
    tf.addfile(ti, io.BytesIO(data))


@pytest.mark.parametrize("rate", [4, 15])
def test_file_route_equals_in_memory_route(cuda, tmp_path, rate):
    """Predicted-onset files -> ``pack_onset_preds`` -> ``sfx_chunks``: the ``y`` track of the shard route equals ``onsets_to_track`` on the
    same logits.  Frame rates 4 and 15 only: there (idx + start) / rate * 1e4 is never a half-integer, so ``"%.4f"`` and the kernel's
    ``rint`` cannot disagree."""
    from syncfusion_amd import OnsetTestStage, onsets_to_track, pack_onset_preds, shards

    sr, T, n = 8000, 2 * rate, 3
    chunk, length = 2 * sr, 2 * sr * n
    rng = np.random.default_rng(rate)
    z = mref.grid_logits(rng, (n, T))
    z[:, 1] = 2.0                                                          # every chunk predicts at least one onset
    t = mref.random_labels(rng, (n, T), 0.3)
    t[0, 0], t[0, 1] = 1.0, 0.0
    order = [2, 0, 1]                                                      # fed out of order: the merge sorts by start frame
    clips = [dict(video_name="clip_001", start_frame=i * T, end_frame=(i + 1) * T, frame_rate=rate) for i in order]
    zd = torch.from_numpy(z[order]).to(cuda)
    stage = OnsetTestStage(types.SimpleNamespace(model=None), str(tmp_path / "run"))
    stage.step_logits(zd, torch.from_numpy(t[order]).to(cuda), clips)
    stage.finish()
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.random.RandomState(0).randn(length) * 3000).astype("<i2").tobytes())
    with tarfile.open(tmp_path / "in.tar", "w") as tf:
        _add(tf, "set/clip_001.resampled.wav", buf.getvalue())
        _add(tf, "set/clip_001.times.csv", b"0.5,hit\n2.5,hit\n4.5,hit\n")        # an annotated onset in every 2-second chunk
    missing, empty = pack_onset_preds(str(tmp_path / "in.tar"), str(tmp_path / "run" / "media" / "annotations" / "pred"), str(tmp_path / "out.tar"))
    assert missing == [] and empty == []
    got = list(shards.sfx_chunks(str(tmp_path / "out.tar"), sample_rate=sr, chunk_size=chunk, cut_prefix=False, one_chunk_per_track=False))
    assert len(got) == n
    y = torch.cat([g[1] for g in got], dim=1)                              # (1, length)
    start = torch.tensor([c["start_frame"] for c in clips], dtype=torch.int32)
    track = onsets_to_track(zd, length, frame_rate=float(rate), sample_rate=float(sr), start_frame=start).amax(dim=0).cpu()
    assert float(track.sum()) == float((z > 0.5).sum()) > 0
    assert torch.equal(y, track)


def test_prepare_gt_for_fad_with_device_resampling(cuda, tmp_path):
    from syncfusion_amd import prepare_gt_for_fad, resample
    from syncfusion_amd.generation import load_wav

    g = torch.Generator().manual_seed(2)
    data = [(torch.randn(1, 4801, generator=g) * 0.3, torch.zeros(1, 4801), torch.randn(1, 50, generator=g), "hit", f"set/clip_{i:03d}")
            for i in range(3)]
    written = prepare_gt_for_fad(tmp_path / "gt", data, batch_size=2, sample_rate=48000, downsample_rate=22050)
    assert [p.name for p in written] == ["0.wav", "1.wav", "2.wav"]
    for i, p in enumerate(written):
        wav, sr = load_wav(p)
        want = resample(data[i][0].to(cuda), orig_freq=48000, new_freq=22050).cpu()
        assert sr == 22050 and wav.shape == want.shape == (1, math.ceil(22050 * 4801 / 48000)) and torch.equal(wav, want)
