"""The onset data's training transforms on the device (``frame_transforms.Compose`` -> ``sf_frames_augment``) against the restated
oracle ``tests/frames_augment_ref.py`` (resize + crop + normalize pinned to ATen; colour jitter restated from torchvision 0.14.1).

Gate of every comparison (set by the reference arithmetic's own error, not by what the kernels give):
    max |device - oracle(fp64)| <= max(2e-5, 4 * e32),   e32 = max |oracle(fp32, CPU) - oracle(fp64)| of the same case
2e-5 is the gate ``frames_to_clip`` has at this output scale; 4 x covers fused multiply-adds and the summation order of the contrast mean.
Every case prints e32 and the device error (``pytest -s``)."""
import itertools
import json

import pytest
import torch

import frames_augment_ref as R

pytestmark = pytest.mark.gpu

# (N, T, H, W), Resize size: 240 x 320 is what script/gh_preprocess_videos.py extracts (-> 128 x 170 -> 112); portrait; upscaling with an odd
# aspect; 112 x 112 with Resize(112): the crop is the whole frame (no random draw)
GEOMETRIES = [((2, 30, 240, 320), 128), ((1, 4, 320, 240), 128), ((3, 5, 130, 100), 128), ((1, 3, 112, 112), 112)]
SINGLE_OPS = [("brightness", 0, 0.6), ("brightness", 0, 1.4), ("contrast", 1, 0.8), ("contrast", 1, 1.2), ("saturation", 2, 0.6),
              ("saturation", 2, 1.4), ("hue", 3, -0.1), ("hue", 3, 0.1)]          # both ends of the reference's ranges


def _chain(size=128, crop="random", jitter=(0.4, 0.2, 0.4, 0.1)):
    from syncfusion_amd import frame_transforms as ft

    ts = [ft.Resize(size, antialias=True)]
    if crop == "random":
        ts.append(ft.RandomCrop(112))
    elif crop == "center":
        ts.append(ft.CenterCrop(112))
    if jitter is not None:
        ts.append(ft.ColorJitter(*jitter))
    ts.append(ft.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]))
    return ft.Compose(ts)


def _sector_shares(probe):
    s = torch.cat([v.flatten() for v in probe["hue_sector"]])
    return [float((s == k).double().mean()) for k in range(6)]


def _clamp_shares(probe, name):
    v = torch.cat([x.flatten() for x in probe["preclamp_" + name]])
    return float((v <= 0.0).double().mean()), float((v >= 1.0).double().mean())


def _compare(label, chain, u8, params, cuda):
    """device vs oracle(fp64) under the gate; returns the oracle's probe for the fixture conditions"""
    probe = {}
    r64 = R.transform_batch(u8, params, chain.normalize.mean, chain.normalize.std, torch.float64, probe)
    r32 = R.transform_batch(u8, params, chain.normalize.mean, chain.normalize.std, torch.float32)
    e32 = float((r32.double() - r64).abs().max())
    got = chain(u8.to(cuda), params=params)
    assert got.shape == r64.shape and got.dtype == torch.float32
    d = (got.cpu().double() - r64).abs()
    err = float(d.max())
    gate = max(2e-5, 4.0 * e32)
    where = [int(i) for i in torch.unravel_index(d.argmax(), d.shape)] if hasattr(torch, "unravel_index") else int(d.argmax())
    print(f"frames_augment {label}: e32 {e32:.3e}  device {err:.3e}  gate {gate:.3e}  worst at {where}")
    assert err <= gate, f"{label}: device error {err:.3e} above max(2e-5, 4 * e32 = {4 * e32:.3e}) at {where}"
    return probe


@pytest.mark.parametrize("shape,size", GEOMETRIES)
def test_crop_only_and_center_crop(cuda, shape, size):
    N, T, H, W = shape
    u8 = R.make_frames(N, T, H, W, seed=H)
    for crop in ("random", "center"):
        chain = _chain(size, crop, jitter=None)
        params = chain.sample(N, (H, W), torch.Generator().manual_seed(3))
        assert int(params.mask.max()) == 0
        if crop == "center":
            rh, rw = params.resized_hw
            assert params.top.tolist() == [int(round((rh - 112) / 2.0))] * N and params.left.tolist() == [int(round((rw - 112) / 2.0))] * N
        _compare(f"{shape} {crop} crop", chain, u8, params, cuda)


@pytest.mark.parametrize("name,op,f", SINGLE_OPS)
@pytest.mark.parametrize("shape,size", GEOMETRIES)
def test_single_colour_operation(cuda, shape, size, name, op, f):
    N, T, H, W = shape
    u8 = R.make_frames(N, T, H, W, seed=H)
    chain = _chain(size)
    params = chain.sample(N, (H, W), torch.Generator().manual_seed(4))
    params.mask[:] = 1 << op
    params.factor[:, op] = f
    probe = _compare(f"{shape} {name} {f}", chain, u8, params, cuda)
    # conditions on the FIXTURE, from the oracle's own intermediates
    if name == "hue":
        shares = _sector_shares(probe)
        assert min(shares) >= 0.01, f"hue sectors {shares}: the frames do not exercise every sector"
    if (name, f) in (("brightness", 1.4), ("contrast", 1.2)):
        lo, hi = _clamp_shares(probe, name)
        assert lo >= 0.005 and hi >= 0.005, f"{name} {f}: {lo:.4f} of the values reach the lower clamp, {hi:.4f} the upper"


@pytest.mark.parametrize("shape,size", [((24, 2, 240, 320), 128), ((24, 2, 130, 100), 128)])
def test_all_24_orders_of_the_full_jitter(cuda, shape, size):
    """one clip per order; the factors vary from clip to clip inside the reference's ranges (drawn by ``sample``)"""
    N, T, H, W = shape
    u8 = R.make_frames(N, T, H, W, seed=H + 1)
    chain = _chain(size)
    params = chain.sample(N, (H, W), torch.Generator().manual_seed(5))
    params.order[:] = torch.tensor(list(itertools.permutations(range(4))), dtype=torch.int32)
    assert int(params.mask.min()) == 15
    probe = _compare(f"{shape} all 24 orders", chain, u8, params, cuda)
    assert min(_sector_shares(probe)) >= 0.01


@pytest.mark.parametrize("shape,size", GEOMETRIES + [((6, 3, 240, 320), 128)])
def test_reference_training_chain_with_sampled_parameters(cuda, shape, size):
    """cfg/data/data-onset-greatesthit-augment.yaml:8-28; the 6-clip batch mixes orders, masks and crops in ONE launch sequence: clips 1 and 4
    lose contrast (one pass among two-pass clips), clip 2 keeps hue only, clip 3 has no colour operation at all."""
    N, T, H, W = shape
    u8 = R.make_frames(N, T, H, W, seed=H + 2)
    chain = _chain(size)
    params = chain.sample(N, (H, W), torch.Generator().manual_seed(6))
    if N == 6:
        params.mask[1] = params.mask[4] = 15 & ~2
        params.mask[2] = 8
        params.mask[3] = 0
        assert len({tuple(o) for o in params.order.tolist()}) > 1 and len(set(zip(params.top.tolist(), params.left.tolist()))) > 1
    probe = _compare(f"{shape} full chain", chain, u8, params, cuda)
    assert min(_sector_shares(probe)) >= 0.01


def test_bit_equal_to_what_exists(cuda):
    """the evaluation chain through the new kernels == ``frames_to_clip``; a jitter of strength 0 == no jitter"""
    from syncfusion_amd import frame_transforms as ft
    from syncfusion_amd.input_pipeline import frames_to_clip

    for (N, T, H, W) in [(2, 5, 240, 320), (1, 3, 112, 112), (2, 4, 100, 130), (1, 3, 64, 48)]:
        u8 = R.make_frames(N, T, H, W, seed=W).to(cuda)
        noise = torch.randint(0, 256, (N, T, H, W, 3), generator=torch.Generator().manual_seed(H), dtype=torch.uint8).to(cuda)
        chain = ft.Compose([ft.Resize((112, 112), antialias=True), ft.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])])
        for x in (u8, noise):
            assert torch.equal(chain(x), frames_to_clip(x))
        assert torch.equal(ft.default_chain()(u8), frames_to_clip(u8))
    u8 = R.make_frames(3, 4, 240, 320, seed=9).to(cuda)
    with_zero, without = _chain(128, "random", (0, 0, 0, 0)), _chain(128, "random", None)
    for k in range(3):   # clip by clip: ColorJitter draws its permutation even when every operation is absent
        a = with_zero(u8[k: k + 1], generator=torch.Generator().manual_seed(20 + k))
        b = without(u8[k: k + 1], generator=torch.Generator().manual_seed(20 + k))
        assert torch.equal(a, b)


def test_deterministic_and_independent_of_the_batch(cuda):
    N, T, H, W = 5, 6, 240, 320
    u8 = R.make_frames(N, T, H, W, seed=11).to(cuda)
    chain = _chain(128)
    params = chain.sample(N, (H, W), torch.Generator().manual_seed(12))
    params.mask[3] = 15 & ~2         # one single-pass clip among the two-pass ones
    a, b = chain(u8, params=params), chain(u8, params=params)
    assert torch.equal(a, b)
    for k in range(N):
        alone = chain(u8[k: k + 1], params=params.select([k]))
        assert torch.equal(alone[0], a[k]), k
    # the same generator state -> the same batch
    c = chain(u8, generator=torch.Generator().manual_seed(13))
    d = chain(u8, generator=torch.Generator().manual_seed(13))
    assert torch.equal(c, d) and not torch.equal(c, a)


def test_rejections(cuda):
    from syncfusion_amd import frame_transforms as ft
    from syncfusion_amd._lib import SyncFusionAmdError

    u8 = R.make_frames(2, 2, 240, 320, seed=1)
    chain = _chain(128)
    with pytest.raises(SyncFusionAmdError, match="no CPU execution path"):
        chain(u8)
    with pytest.raises(SyncFusionAmdError, match="uint8"):
        chain(u8.to(cuda).float())
    with pytest.raises(SyncFusionAmdError, match="larger than the resized frame"):
        _chain(64)(u8.to(cuda))                                 # 64 x 85 cannot hold a 112 x 112 crop (torchvision would need padding)
    good = chain.sample(2, (240, 320), torch.Generator().manual_seed(2))
    bad = good.select([0, 1])
    bad.order[1] = torch.tensor([0, 0, 1, 2], dtype=torch.int32)
    with pytest.raises(SyncFusionAmdError, match="not a permutation"):
        chain(u8.to(cuda), params=bad)
    bad = good.select([0, 1])
    bad.left[0] = 170 - 112 + 1
    with pytest.raises(SyncFusionAmdError, match="outside the resized frame"):
        chain(u8.to(cuda), params=bad)
    bad = good.select([0, 1])
    bad.factor[1, 2] = float("nan")
    with pytest.raises(SyncFusionAmdError, match="not finite"):
        chain(u8.to(cuda), params=bad)
    with pytest.raises(SyncFusionAmdError, match="parameters for 1 clips"):
        chain(u8.to(cuda), params=good.select([0]))
    torch.cuda.synchronize()
    assert torch.isfinite(chain(u8.to(cuda), params=good)).all()      # and the valid table still runs afterwards


@pytest.mark.autograd
def test_frame_directory_to_training_step(cuda, tmp_path):
    """frame directory -> ``iter_clips(frames_transforms=..., shuffle=True, drop_last=True)`` -> the oracle on the decoded frames with
    ``sample``'s parameters for the same generator state; then one ``OnsetModel.training_step`` + ``backward()`` on such a batch."""
    import numpy as np
    from PIL import Image

    from helpers import seeded_state
    from syncfusion_amd import OnsetModel, VideoOnsetNet
    from syncfusion_amd import video_chunks as vc

    d = tmp_path / "v1" / "frames"
    d.mkdir(parents=True)
    src = R.make_frames(1, 21, 120, 160, seed=3)[0]
    imgs = []
    for i in range(21):
        Image.fromarray(src[i].numpy()).save(d / f"{i + 1}.jpg", quality=95)
        imgs.append(np.asarray(Image.open(d / f"{i + 1}.jpg").convert("RGB")))     # what a JPEG decoder returns
    (tmp_path / "v1" / "v1.metadata.json").write_text(json.dumps({"processed": {"video_frame_rate": 4.0, "video_duration": 5.1}}))
    (tmp_path / "v1" / "v1.times.csv").write_text("0.3,hit\n1.6,hit\n2.2,hit\n3.9,hit\n4.5,hit\n")
    table = vc.chunk_table(str(tmp_path), ["v1"], chunk_length_in_seconds=1.0)
    assert len(table) == 5
    chain = _chain(128)
    with torch.no_grad():
        batches = list(vc.iter_clips(table, batch_size=2, device=cuda, frames_transforms=chain, shuffle=True, drop_last=True,
                                     generator=torch.Generator().manual_seed(31)))
    assert len(batches) == 2                                                       # 5 chunks, batch 2, drop_last
    g = torch.Generator().manual_seed(31)
    perm = torch.randperm(5, generator=g).tolist()
    for b, (clips, labels, part) in enumerate(batches):
        idx = perm[2 * b: 2 * b + 2]
        assert [c["start_frame"] for c in part] == [4 * i for i in idx]
        assert torch.equal(labels.cpu(), torch.stack([table[i]["labels"] for i in idx]))
        u8 = torch.from_numpy(np.stack([np.stack(imgs[4 * i: 4 * i + 4]) for i in idx]))
        params = chain.sample(2, (120, 160), g)
        r64 = R.transform_batch(u8, params, dtype=torch.float64)
        e32 = float((R.transform_batch(u8, params, dtype=torch.float32).double() - r64).abs().max())
        err = float((clips.cpu().double() - r64).abs().max())
        print(f"frames_augment end to end batch {b}: e32 {e32:.3e}  device {err:.3e}")
        assert clips.shape == (2, 3, 4, 112, 112) and err <= max(2e-5, 4.0 * e32)
    net = VideoOnsetNet(False)
    net.load_state_dict(seeded_state(net, 7))
    model = OnsetModel(1e-3, 0.9, 0.999, 1e-8, 1e-2, net.to(cuda).train()).to(cuda)
    clips, labels, _ = batches[0]
    loss = model.training_step({"frames": clips, "label": labels}, 0)
    loss.backward()
    assert torch.isfinite(loss.detach()).item()
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert all(gr is not None and torch.isfinite(gr).all() for gr in grads)
