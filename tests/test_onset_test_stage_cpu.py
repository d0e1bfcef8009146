"""CPU suite for the onset net's test stage (syncfusion_amd/onset_test.py), the shard packing and the FAD ground-truth preparation
(syncfusion_amd/generation.py): the CPU path of ``annotation_rows`` and the merged annotation files against the file route of
tests/onset_test_ref.py, ``pack_onset_preds`` through the shard reader, ``prepare_gt_for_fad`` without resampling, and ``OnsetModel`` with
and without ``annotations_dir``.  No kernel runs here."""
import io
import os
import tarfile
import types
import wave

import numpy as np
import pytest
import torch

import onset_metrics_ref as mref
import onset_test_ref as ref

SHAPES = [(1, 1), (2, 3), (3, 30), (5, 64), (4, 65), (2, 130), (17, 30)]


def _batch(N, T, seed, density=0.3):
    rng = np.random.default_rng(seed)
    z = ref.special_rows(mref.grid_logits(rng, (N, T)))
    t = mref.random_labels(rng, (N, T), density)
    return z, t


@pytest.mark.parametrize("N,T", SHAPES)
def test_cpu_annotation_rows_match_ref(N, T):
    from syncfusion_amd import annotation_rows

    z, t = _batch(N, T, 100 * N + T)
    got = annotation_rows(torch.from_numpy(z), torch.from_numpy(t))
    want = ref.rows_ref(z, t)
    for g, w in zip(got, want):
        assert g.dtype == torch.int32 and np.array_equal(g.numpy(), w)


# ---- merged files -------------------------------------------------------------------------------------------------------------------------
T15 = 30          # 2 s at 15 frames per second


def _clip(video, start, rate=15, T=T15):
    return dict(video_name=video, start_frame=start, end_frame=start + T, frame_rate=rate)


def _stage_batches():
    """Three batches over six videos.  ``a``: chunks at frames 1000, 30, 0 and 120, fed out of order (lexicographically 1000 sorts before
    120 and 30); ``solo``: one chunk with a single predicted and a single annotated onset; ``none``: one chunk without any; ``v1`` and ``v10``
    with two chunks each (``v1.*`` must not pick up ``v10``'s chunks); every batch holds both label classes (BCLoss.evaluate needs them)."""
    rng = np.random.default_rng(5)
    clips = [[_clip("a", 1000), _clip("v10", 30), _clip("solo", 60), _clip("a", 30)],
             [_clip("v1", 30), _clip("a", 0), _clip("none", 0), _clip("v10", 0)],
             [_clip("v1", 0), _clip("a", 120)]]
    out = []
    for part in clips:
        z = mref.grid_logits(rng, (len(part), T15))
        t = mref.random_labels(rng, (len(part), T15), 0.2)
        t[0, 3], t[0, 4] = 1.0, 0.0
        for i, c in enumerate(part):
            if c["video_name"] == "solo":
                z[i], t[i] = -2.0, 0.0
                z[i, 7], t[i, 11] = 2.0, 1.0
            if c["video_name"] == "none":
                z[i], t[i] = -2.0, 0.0
        out.append((z, t, part))
    return out


def _stub_model():
    return types.SimpleNamespace(model=None)          # step_logits never calls the net


def test_merged_files_equal_the_file_route(tmp_path):
    from syncfusion_amd import OnsetTestStage
    from syncfusion_amd.module_onset import BCLoss

    batches = _stage_batches()
    want = ref.file_route(str(tmp_path / "ref"), batches)
    stage = OnsetTestStage(_stub_model(), str(tmp_path / "got"))
    for z, t, part in batches:
        stage.step_logits(torch.from_numpy(z), torch.from_numpy(t), part)
    res = stage.finish()
    got = ref.read_dir(str(tmp_path / "got"))
    assert set(want["pred"]) == {"a", "solo", "none", "v1", "v10"}
    assert got == want                                                   # the same file names (no chunk file left) and bytes, both kinds
    assert want["pred"]["none"] == b"" and want["target"]["none"] == b""
    assert want["pred"]["solo"] == b"4.4667\n" and want["target"]["solo"] == b"4.7333\n"      # (7 + 60) / 15, (11 + 60) / 15
    for kind in ("target", "pred"):
        for video, data in want[kind].items():
            assert res["videos"][video][kind] == [float(s) for s in data.decode().split()]
    a = res["videos"]["a"]["target"]
    assert a == sorted(a) and a[-1] >= 1000 / 15                          # chunk order by start frame, not by name
    # epoch figures: the mean over batches weighted by batch size of what BCLoss gives per batch
    crit, sums = BCLoss(), np.zeros(5)
    for z, t, part in batches:
        m = crit.evaluate(torch.from_numpy(z), torch.from_numpy(t))
        sums += len(part) * np.array([float(crit(torch.from_numpy(z), torch.from_numpy(t))), m["AP"], m["Acc"], m["OnsNumAcc"], 1.0])
    for i, k in enumerate(("loss/test", "metrics/test/AP", "metrics/test/Acc", "metrics/test/OnsNumAcc")):
        assert res[k] == pytest.approx(sums[i] / sums[4], rel=1e-12)
    assert stage.clips == 0 and stage.finish()["videos"] == {}           # finish() empties the stage


def test_dotted_video_name_raises():
    from syncfusion_amd import OnsetTestStage

    z, t = _batch(2, T15, 1)
    stage = OnsetTestStage(_stub_model())
    with pytest.raises(ValueError, match="contains '.'"):
        stage.step_logits(torch.from_numpy(z), torch.from_numpy(t), [_clip("ok", 0), _clip("2015-02-16.mic", 0)])
    assert stage.clips == 0


def test_stage_takes_one_clip_length():
    from syncfusion_amd import OnsetTestStage

    stage = OnsetTestStage(_stub_model())
    z, t = _batch(2, 8, 1)
    stage.step_logits(torch.from_numpy(z), torch.from_numpy(t), [_clip("x", 0, 4, 8), _clip("x", 8, 4, 8)])
    z, t = _batch(1, 9, 2)
    with pytest.raises(ValueError, match="one clip length"):
        stage.step_logits(torch.from_numpy(z), torch.from_numpy(t), [_clip("x", 16, 4, 9)])
    with pytest.raises(ValueError, match="chunk records"):
        stage.step_logits(torch.from_numpy(z[:, :8]), torch.from_numpy(t[:, :8]), [])


# ---- shard packing ------------------------------------------------------------------------------------------------------------------------
def _wav_bytes(x: np.ndarray, sr: int) -> bytes:
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(x.shape[0])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(x.T.astype("<i2").tobytes())
    return buf.getvalue()


def _add(tf, name, data: bytes):
    ti = tarfile.TarInfo(name)
    ti.size = len(data)
    tf.addfile(ti, io.BytesIO(data))


def test_pack_onset_preds_round_trip(tmp_path):
    from syncfusion_amd import pack_onset_preds, shards

    rs = np.random.RandomState(0)
    src, keys = tmp_path / "test.tar", ["set/a_001", "set/b_002", "c_003", "set/d_004"]
    with tarfile.open(src, "w") as tf:
        for key in keys:
            _add(tf, f"{key}.resampled.wav", _wav_bytes((rs.randn(1, 400) * 3000).astype(np.int16), 8000))
            _add(tf, f"{key}.times.csv", b"0.01,hit\n0.03,None\n")
            if key == "set/d_004":
                _add(tf, f"{key}.times.pred.csv", b"9.0\n")              # a stale prediction: replaced
    pred = tmp_path / "pred"
    pred.mkdir()
    (pred / "a_001.times.csv").write_text("0.0667\n1.2000\n")
    (pred / "b_002.times.csv").write_text("")
    (pred / "d_004.times.csv").write_text("0.5000\n")
    missing, empty = pack_onset_preds(str(src), str(pred), str(tmp_path / "out.tar"))
    assert missing == ["c_003"] and empty == ["set/b_002"]
    got = list(shards.iter_shard_samples(str(tmp_path / "out.tar")))
    before = list(shards.iter_shard_samples(str(src)))
    assert [s["__key__"] for s in got] == keys
    assert got[0]["times.pred.csv"] == {0.0667: None, 1.2: None} and got[1]["times.pred.csv"] == {} and "times.pred.csv" not in got[2]
    assert got[3]["times.pred.csv"] == {0.5: None}
    for a, b in zip(got, before):
        assert torch.equal(a["resampled.wav"][0], b["resampled.wav"][0]) and a["times.csv"] == b["times.csv"]
    with tarfile.open(tmp_path / "out.tar") as tf:                         # the prediction sits right behind its sample's members
        names = tf.getnames()
    assert names[:3] == ["set/a_001.resampled.wav", "set/a_001.times.csv", "set/a_001.times.pred.csv"]
    assert names.count("set/d_004.times.pred.csv") == 1
    missing, empty = pack_onset_preds(str(src), str(pred), str(tmp_path / "kept.tar"), skip_empty=True)
    assert missing == ["c_003"] and empty == ["set/b_002"]
    assert [s["__key__"] for s in shards.iter_shard_samples(str(tmp_path / "kept.tar"))] == ["set/a_001", "set/d_004"]


# ---- ground truth for FAD -----------------------------------------------------------------------------------------------------------------
def _chunks(n, length=300):
    g = torch.Generator().manual_seed(2)
    return [(torch.randn(1, length, generator=g), torch.zeros(1, length), torch.randn(1, 50, generator=g), "hit", f"set/clip_{i:03d}")
            for i in range(n)]


def test_prepare_gt_for_fad_without_downsampling(tmp_path, capsys):
    from syncfusion_amd import prepare_gt_for_fad
    from syncfusion_amd.generation import load_wav

    data = _chunks(5)
    written = prepare_gt_for_fad(tmp_path / "gt", data, batch_size=2, sample_rate=16000)
    assert [p.name for p in written] == [f"{i}.wav" for i in range(5)] and sorted(os.listdir(tmp_path / "gt")) == sorted(p.name for p in written)
    for i, p in enumerate(written):
        wav, sr = load_wav(p)
        assert sr == 16000 and torch.equal(wav, data[i][0])
    # the crude resume: a batch whose last file exists is skipped; remove 2.wav (batch 1 ends at 3.wav, which exists): nothing is rewritten
    os.remove(tmp_path / "gt" / "2.wav")
    capsys.readouterr()
    assert prepare_gt_for_fad(tmp_path / "gt", data, batch_size=2, sample_rate=16000) == []
    assert capsys.readouterr().out.count("Skipping path") == 3 and not (tmp_path / "gt" / "2.wav").exists()
    # one file per track: named after the key's base name, and "Skipping" only prints
    named = prepare_gt_for_fad(tmp_path / "tracks", data, batch_size=2, sample_rate=16000, one_chunk_per_track=True)
    assert [p.name for p in named] == [f"clip_{i:03d}.wav" for i in range(5)]
    capsys.readouterr()
    again = prepare_gt_for_fad(tmp_path / "tracks", data, batch_size=2, sample_rate=16000, one_chunk_per_track=True)
    assert len(again) == 5 and capsys.readouterr().out.count("Skipping path") == 3
    assert torch.equal(load_wav(tmp_path / "tracks" / "clip_004.wav")[0], data[4][0])


# ---- OnsetModel ---------------------------------------------------------------------------------------------------------------------------
class _TinyNet(torch.nn.Module):
    """(N, 3, T, H, W) -> (N, T) on the CPU: a stand-in for the net (which has no CPU path)."""

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor(4.0))

    def forward(self, x):
        return x.mean(dim=(1, 3, 4)) * self.scale


def _model_batch():
    g = torch.Generator().manual_seed(4)
    frames = torch.randn(3, 3, 8, 4, 4, generator=g)
    label = (torch.rand(3, 8, generator=g) < 0.4).float()
    label[0, 0], label[0, 1] = 1.0, 0.0
    return {"frames": frames, "label": label, "video_name": ["p", "q", "p"], "start_frame": torch.tensor([8, 0, 0]),
            "end_frame": torch.tensor([16, 8, 8]), "frame_rate": torch.tensor([4.0, 4.0, 4.0])}


def test_onset_model_default_test_step_writes_nothing(tmp_path, monkeypatch):
    from syncfusion_amd import OnsetModel

    monkeypatch.chdir(tmp_path)
    m = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, _TinyNet())
    batch = _model_batch()
    loss = m.test_step(batch, 0)
    assert torch.equal(loss, m.loss(m.model(batch["frames"]), batch["label"])) and loss.dim() == 0
    m.on_test_epoch_end()
    assert m.annotations_dir is None and m.test_stage is None and m.test_results is None and os.listdir(tmp_path) == []


def test_onset_model_with_annotations_dir_on_the_cpu(tmp_path):
    from syncfusion_amd import OnsetModel

    m = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, _TinyNet(), annotations_dir=str(tmp_path / "run"))
    batch = _model_batch()
    plain = {k: batch[k] for k in ("frames", "label")}
    loss = m.test_step(batch, 0)
    assert torch.equal(loss, m._step(plain, 0, "test"))
    assert torch.equal(m.test_step(plain, 1), loss) and m.test_stage.clips == 3      # a batch without names: loss only
    m.on_test_epoch_end()
    logits = m.model(batch["frames"]).detach().numpy()
    clips = [dict(video_name=n, start_frame=s, end_frame=e, frame_rate=4.0) for n, s, e in zip(["p", "q", "p"], [8, 0, 0], [16, 8, 8])]
    want = ref.file_route(str(tmp_path / "ref"), [(logits, batch["label"].numpy(), clips)])
    assert ref.read_dir(str(tmp_path / "run")) == want
    assert m.test_results["loss/test"] == pytest.approx(float(loss), rel=1e-12) and set(m.test_results["videos"]) == {"p", "q"}


# ---- the entry point's refusals (host-only: every one comes before any HIP call) -------------------------------------------------------------
def test_entry_point_is_declared_and_refuses_bad_arguments():
    from syncfusion_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "syncfusion_amd.h")).read()
    for name in ("sf_op_onset_test_workspace_bytes", "sf_op_onset_test_step"):
        assert name in header and name in _lib.SYMBOLS and hasattr(lib, name)
    q = lib.sf_op_onset_test_workspace_bytes
    assert q(16, 30) >= lib.sf_op_onset_loss_workspace_bytes(480) + 36 and q(16, 30) % 8 == 0
    assert q(0, 30) == -1 and q(16, 0) == -1 and q(1 << 13, 1 << 12) == -1 and q(1 << 12, 1 << 12) > 0
    p, big = 0x1000, 1 << 40                                               # never dereferenced: every call below is refused on the host
    INVALID, SHAPE, WORKSPACE, UNSUPPORTED = 1, 3, 5, 6

    def step(logits=p, labels=p, N=4, T=8, clip0=0, capacity=4, pc=p, pf=p, tc=p, tf=p, sums=p, ws=p, ws_bytes=big):
        return lib.sf_op_onset_test_step(logits, labels, N, T, 0.5, 0.75, clip0, capacity, pc, pf, tc, tf, sums, ws, ws_bytes, None)

    for arg in ("logits", "labels", "pc", "pf", "tc", "tf", "sums", "ws"):
        assert step(**{arg: None}) == INVALID and b"null" in lib.sf_last_error(), arg
    assert step(N=0) == INVALID and step(T=0) == INVALID and step(clip0=-1) == INVALID
    assert step(clip0=1) == SHAPE and step(capacity=3) == SHAPE and step(clip0=5, capacity=4) == SHAPE and b"capacity" in lib.sf_last_error()
    assert step(N=1 << 13, T=1 << 12, capacity=1 << 13) == UNSUPPORTED and b"2^24" in lib.sf_last_error()
    assert step(ws_bytes=q(4, 8) - 1) == WORKSPACE and b"workspace" in lib.sf_last_error()
    assert step(ws=p + 4) == INVALID and b"misaligned" in lib.sf_last_error()
